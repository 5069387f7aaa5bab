"""RB-WebFace evaluation: TPR @ FPR = 1e-3 / 1e-4 per ethnic group (the reference's rb-webface/scripts/test_RB_Webface.py).

    python rb-webface/scripts/test_RB_Webface.py --data_path <WebFace images> --partition_path <pair lists> \\
        --model_ckpt_path <Backbone_....pth> --config_name configs/<config>.py

Same command line, list files (``pos_pairs_samples_<Group>.txt`` / ``neg_pairs_samples_<Group>.txt``), thresholds and
printed lines as the reference; what runs underneath differs:

* host workers only decode; Resize(128) -> CenterCrop(112) -> ToTensor -> Normalize(0.5) is one launch of the device
  transform per batch (``fr_augment_u8``, bit-exact with Pillow), the forward is the BN-folded forward-only plan, and the
  embeddings stay on the device;
* per group, ONE mode-0 and ONE mode-1 call of ``frhip.pairwise.pair_counts`` give the FMR / FNMR tallies of all
  thresholds (the reference forms the float64 M x M cosine matrix on the host once per threshold);
* any backbone ``train.build_backbone`` builds is accepted, with the config's ``COMPUTE_DTYPE``.

Divergences: scores are fp32; any number of embeddings works (the reference's ``calc_FMR`` needs a
multiple of its batch size); one GPU.  ``--cpu_batch_size`` / ``--cpu_n_jobs`` are accepted and unused.
"""
import argparse
import importlib
import os
import sys

import numpy as np
import torch

_PRODUCT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for _p in (_PRODUCT, "."):  # the product root, and the reference's "run from the project root"
    if _p not in sys.path:
        sys.path.append(_p)

from frhip import set_compute_dtype  # noqa: E402
from frhip.input_pipeline import GpuTrainTransform  # noqa: E402
from frhip.pairwise import pair_counts  # noqa: E402
from util.utils import l2_norm  # noqa: E402

class2race = {"African": 0, "Asian": 1, "Caucasian": 2, "Indian": 3}
race2class = {v: k for k, v in class2race.items()}
DEFAULT_THRESHOLDS = (0.3, 0.6, 20)  # covers FPR 1e-3 .. 1e-4 of a strong model; --thresholds moves it for a weaker one
DEVICE = "cuda:0"


def initialize_model(config_name, checkpoint):
    from train import build_backbone
    sys.path.append(os.path.dirname(config_name))
    name = os.path.basename(config_name).replace(".py", "").replace("/", ".")
    cfg = importlib.import_module(name).configurations[1]
    torch.manual_seed(cfg["SEED"])
    backbone = build_backbone(cfg)
    if not (os.path.exists(checkpoint) and os.path.isfile(checkpoint)):
        raise Exception("checkpoint cannot be opened")
    print("Loading Backbone Checkpoint '{}'".format(checkpoint))
    backbone.load_state_dict(torch.load(checkpoint, map_location="cpu"))
    set_compute_dtype(backbone, cfg.get("COMPUTE_DTYPE"))
    backbone.eval()
    backbone.to(DEVICE)
    return backbone


class ImageDataset(torch.utils.data.Dataset):
    """Decodes only: a sample is the uint8 HWC image as stored."""

    def __init__(self, paths_list=None):
        super().__init__()
        self.paths = paths_list

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, index):
        from PIL import Image
        with Image.open(self.paths[index]) as img:
            return torch.from_numpy(np.asarray(img.convert("RGB")).copy())


def _as_list(batch):
    return batch


_TRANSFORM = {}


def center_crop_batch(images, device=DEVICE):
    """list of uint8 [H, W, 3] host tensors -> float32 [B, 3, 112, 112] on the device: Resize([128, 128]),
    CenterCrop([112, 112]), ToTensor, Normalize(0.5, 0.5).  The device transform takes one image size per launch; a batch
    of mixed sizes is split by size (and put back in order), never transformed on the host."""
    tf = _TRANSFORM.get("tf")
    if tf is None:
        tf = _TRANSFORM["tf"] = GpuTrainTransform(112, (0.5, 0.5, 0.5), (0.5, 0.5, 0.5))
    top = int(round((128 - 112) / 2.0))
    by_size = {}
    for i, im in enumerate(images):
        by_size.setdefault(tuple(im.shape[:2]), []).append(i)
    out = None
    for idx in by_size.values():
        u8 = torch.stack([images[i] for i in idx]).pin_memory().to(device, non_blocking=True)
        key = (str(device), len(idx))
        if key not in _TRANSFORM:  # constant offsets, kept on the device
            _TRANSFORM[key] = (torch.full((len(idx), 2), top, dtype=torch.int32, device=device),
                               torch.zeros(len(idx), dtype=torch.uint8, device=device))
        crop, flip = _TRANSFORM[key]
        x = tf(u8, crop, flip, validate=False)
        if len(by_size) == 1:
            return x
        if out is None:
            out = torch.empty(len(images), 3, 112, 112, device=device)
        out[torch.as_tensor(idx, device=device)] = x
    return out


def calc_embeddings(backbone, names, data_dir, batch_size=50, num_workers=8):
    """L2-normalised embeddings of ``names``, float32 [N, D] ON THE DEVICE (the reference returns a numpy array)."""
    absnames = [os.path.join(data_dir, name) for name in names]
    loader = torch.utils.data.DataLoader(ImageDataset(absnames), batch_size=batch_size, num_workers=num_workers,
                                         drop_last=False, shuffle=False, collate_fn=_as_list)
    all_emb, done = None, 0
    with torch.no_grad():
        for images in loader:
            emb = l2_norm(backbone(center_crop_batch(images)).float())
            if all_emb is None:
                all_emb = torch.empty(len(absnames), emb.shape[1], device=emb.device)
            all_emb[done:done + emb.shape[0]] = emb
            done += emb.shape[0]
    return all_emb


def _on_device(emb):
    if isinstance(emb, torch.Tensor):
        return emb.to(DEVICE, torch.float32)
    return torch.from_numpy(np.ascontiguousarray(emb, dtype=np.float32)).to(DEVICE)


def group_rates(pos_emb, neg_emb, thresholds, n_names_per_grp=5):
    """(FMR [T], FNMR [T]) as float64 numpy arrays: one tally launch per list for all thresholds, one read-back."""
    fm, fm_seen = pair_counts(_on_device(neg_emb), thresholds)
    fnm, fnm_seen = pair_counts(_on_device(pos_emb), thresholds, group=n_names_per_grp)
    both = torch.cat([fm, fnm]).cpu().numpy()
    return both[:fm.numel()] / fm_seen, both[fm.numel():] / fnm_seen


def calc_FNMR(pos_emb, threshold, n_names_per_grp=5):
    """Fraction of genuine pairs (inside each run of ``n_names_per_grp`` rows) that score below ``threshold``."""
    c, seen = pair_counts(_on_device(pos_emb), [float(threshold)], group=n_names_per_grp)
    return int(c.cpu()[0]) / seen


def calc_FMR(neg_emb, threshold, n_jobs=1, batch_size=1000):
    """Fraction of all pairs i < j that score above ``threshold``.  ``n_jobs`` / ``batch_size``: the reference's host
    chunking, unused here."""
    c, seen = pair_counts(_on_device(neg_emb), [float(threshold)])
    return int(c.cpu()[0]) / seen


def evaluate_model(config_name, checkpoint, data_dir, test_names_dir, cpu_batch_size=1000, cpu_n_jobs=8, gpu_batch_size=50,
                   thresholds=None, num_workers=8):
    tpr_at3, tpr_at4 = dict(), dict()
    print("initializing model...")
    backbone = initialize_model(config_name, checkpoint)
    all_thresholds = np.linspace(*DEFAULT_THRESHOLDS) if thresholds is None else np.asarray(thresholds, np.float64)

    for grp_no in range(4):
        grp = race2class[grp_no]
        names_for_pos_pairs = open(os.path.join(test_names_dir, f"pos_pairs_samples_{grp}.txt")).read().splitlines()
        names_for_neg_pairs = open(os.path.join(test_names_dir, f"neg_pairs_samples_{grp}.txt")).read().splitlines()

        print("calculating embeddings for positive names")
        pos_emb = calc_embeddings(backbone, names_for_pos_pairs, data_dir, gpu_batch_size, num_workers)
        print("calculating embeddings for negative names")
        neg_emb = calc_embeddings(backbone, names_for_neg_pairs, data_dir, gpu_batch_size, num_workers)

        # n_names_per_grp = 5: how many consecutive entries of pos_pairs_samples_*.txt are the same person
        fmr, fnmr = group_rates(pos_emb, neg_emb, all_thresholds, n_names_per_grp=5)
        all_fpr, all_fnr = list(fmr), list(fnmr)
        for threshold, a, b in zip(all_thresholds, all_fnr, all_fpr):
            print("threshold", threshold, "fnmr", a, "fmr", b)

        print("=" * 20)
        print("Group ", grp)
        print("TPR@FPR=1e-3", 1 - np.interp(1e-3, all_fpr[::-1], all_fnr[::-1]))
        print("TPR@FPR=1e-4", 1 - np.interp(1e-4, all_fpr[::-1], all_fnr[::-1]))
        print()

        tpr_at3[grp] = 1 - np.interp(1e-3, all_fpr[::-1], all_fnr[::-1])
        tpr_at4[grp] = 1 - np.interp(1e-4, all_fpr[::-1], all_fnr[::-1])

    return tpr_at3, tpr_at4


if __name__ == "__main__":
    parser = argparse.ArgumentParser(description="RB-WebFace evaluation: TPR at FPR = 1e-3 / 1e-4 per ethnic group.")
    parser.add_argument("--data_path", type=str, default="../", help="root folder of the WebFace images")
    parser.add_argument("--partition_path", type=str, default="../",
                        help="folder with the pos_/neg_pairs_samples_<Group>.txt lists")
    parser.add_argument("--model_ckpt_path", type=str, help="backbone checkpoint written by train.py (Backbone_*.pth)")
    parser.add_argument("--config_name", type=str, help="config file the checkpoint was trained with (backbone name, COMPUTE_DTYPE)")
    parser.add_argument("--cpu_batch_size", type=int, default=1000, help="accepted for compatibility; the tallies run on the GPU")
    parser.add_argument("--cpu_n_jobs", type=int, default=2, help="accepted for compatibility; the tallies run on the GPU")
    parser.add_argument("--gpu_batch_size", type=int, default=50, help="images per forward pass")
    parser.add_argument("--thresholds", type=float, nargs=3, metavar=("LO", "HI", "N"), default=None,
                        help="np.linspace(LO, HI, N) instead of the default 0.3 0.6 20 (weaker models need a higher range)")
    args = parser.parse_args()
    thresholds = None if args.thresholds is None else np.linspace(args.thresholds[0], args.thresholds[1], int(args.thresholds[2]))
    evaluate_model(args.config_name, args.model_ckpt_path, args.data_path, args.partition_path,
                   cpu_batch_size=args.cpu_batch_size, cpu_n_jobs=args.cpu_n_jobs, gpu_batch_size=args.gpu_batch_size,
                   thresholds=thresholds)
    # printing is done inside evaluate_model(...)
