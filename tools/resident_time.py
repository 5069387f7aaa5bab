#!/usr/bin/env python3
"""Measure the device-resident training set (frhip/resident.py) on the GPU.

(a) fr_augment_u8_gather at B = 256, 112x112, drawing random slots of an M = 100 000 store (3.8 GB), against fr_augment_u8 on
    the same 256 images gathered beforehand.  The two alternate in one process; every round times a run of launches of each
    with device events.  Reported: the median and the spread of the rounds, and of the per-round ratio.
(b) images/s of the two input paths alone (no training step) over a directory of JPEG files the tool writes itself: the
    loader path (DataLoader with 16 workers decoding, pinned uint8 batch, copy, fr_augment_u8) and the resident path
    (ResidentLoader), alternating, plus the one-time build of the store.

    python tools/resident_time.py [--out FILE] [--files 8192] [--store 100000] [--workers 16]

Needs a GPU: there is no host fallback, and a time taken elsewhere would say nothing."""
import argparse
import os
import shutil
import statistics
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from dataset import FacesDataset, StageTransform  # noqa: E402
from frhip import ops  # noqa: E402
from frhip.input_pipeline import GpuTrainTransform  # noqa: E402
from frhip.resident import ResidentLoader, ResidentStore  # noqa: E402
from util.utils import collate_fn_ignore_none  # noqa: E402

B, SIDE, SEED = 256, 112, 900
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def spread(values, unit, scale=1.0):
    v = sorted(x * scale for x in values)
    return "median %.2f %s (min %.2f, max %.2f, %d rounds)" % (statistics.median(v), unit, v[0], v[-1], len(v))


def kernel_times(m, rounds, launches):
    dev = torch.device("cuda")
    tf = GpuTrainTransform(SIDE)
    gen = torch.Generator().manual_seed(SEED)
    store = torch.randint(0, 256, (m, SIDE, SIDE, 3), dtype=torch.uint8, device=dev)
    labels = torch.arange(m, dtype=torch.int64, device=dev)
    idx = torch.randint(0, m, (B,), generator=gen, dtype=torch.int32).to(dev)
    crop, flip = tf.draw(B, gen)
    crop, flip = crop.to(dev), flip.to(dev)
    staged = store[idx.long()].contiguous()
    xtab, ytab, lut, kx, ky = tf.tables(dev, SIDE, SIDE)
    out_g = torch.empty(B, 3, SIDE, SIDE, device=dev)
    out_s = torch.empty_like(out_g)
    label_out = torch.empty(B, dtype=torch.int64, device=dev)
    stream = ops.current_stream_ptr()
    gather = ops.call("fr_augment_u8_gather", store, labels, idx, xtab, ytab, crop, flip, lut, out_g, label_out, m, B, SIDE,
                      SIDE, tf.big, tf.big, SIDE, kx, ky, stream)
    sibling = ops.call("fr_augment_u8", staged, xtab, ytab, crop, flip, lut, out_s, B, SIDE, SIDE, tf.big, tf.big, SIDE, kx,
                       ky, stream)
    for _ in range(20):
        gather()
        sibling()
    torch.cuda.synchronize()
    if not torch.equal(out_g, out_s) or not torch.equal(label_out, labels[idx.long()]):
        sys.exit("resident_time: the two kernels disagree")

    def timed(launch):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            launch()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / launches * 1e3  # us per launch

    tg, ts = [], []
    for r in range(rounds):
        first, second = (gather, sibling) if r % 2 == 0 else (sibling, gather)
        a, b = timed(first), timed(second)
        tg.append(a if r % 2 == 0 else b)
        ts.append(b if r % 2 == 0 else a)
    algo = B * (SIDE * SIDE * 3 + 3 * SIDE * SIDE * 4)  # image bytes read once + the float32 batch written
    say("(a) kernel, B = %d, %dx%d, store of %d images (%.2f GB), random slots; %d launches per round, device events"
        % (B, SIDE, SIDE, m, store.numel() / 1e9, launches))
    say("    fr_augment_u8_gather : %s" % spread(tg, "us"))
    say("    fr_augment_u8        : %s   (the same 256 images, gathered beforehand)" % spread(ts, "us"))
    say("    ratio gather/sibling : %s" % spread([g / s for g, s in zip(tg, ts)], "x"))
    say("    algorithmic bytes    : %.1f MB per batch -> %.0f GB/s at the gather's median"
        % (algo / 1e6, algo / statistics.median(tg) / 1e3))
    say("    outputs and labels of the two are equal bit for bit")


def write_files(root, files):
    from PIL import Image
    ids = 64
    rng = np.random.default_rng(SEED)
    for ident in range(ids):
        os.makedirs(os.path.join(root, "id_%03d" % ident))
    for k in range(files):
        base = rng.integers(32, 224, (8, 8, 3)).repeat(SIDE // 8, 0).repeat(SIDE // 8, 1)
        img = np.clip(base + rng.integers(-24, 24, (SIDE, SIDE, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "id_%03d" % (k % ids), "%05d.jpg" % k), quality=90)


def path_rates(files, workers, rounds):
    dev = torch.device("cuda")
    root = tempfile.mkdtemp(prefix="resident_time_")
    try:
        t0 = time.perf_counter()
        write_files(root, files)
        say("(b) input paths alone, %d JPEG files of %dx%d (written in %.1f s), batches of %d, no training step"
            % (files, SIDE, SIDE, time.perf_counter() - t0, B))
        ds = FacesDataset(root, StageTransform())
        tf = GpuTrainTransform(SIDE)
        rng = torch.Generator().manual_seed(SEED)
        sampler = torch.utils.data.distributed.DistributedSampler(ds, 1, 0, shuffle=True, seed=SEED)
        loader = torch.utils.data.DataLoader(ds, batch_size=B, sampler=sampler, shuffle=False, pin_memory=True,
                                             num_workers=workers, drop_last=True, collate_fn=collate_fn_ignore_none)
        t0 = time.perf_counter()
        store = ResidentStore.build(ds, dev, workers)
        build_s = time.perf_counter() - t0
        resident = ResidentLoader(store, tf, B, True, 1, 0, SEED, generator=rng)

        def loader_epochs(n):
            seen = 0
            for epoch in range(n):
                sampler.set_epoch(epoch)
                for inputs, labels in loader:
                    x = tf(inputs.to(dev, non_blocking=True), generator=rng)
                    labels = labels.to(dev, non_blocking=True).long()
                    seen += x.shape[0]
            torch.cuda.synchronize()
            return seen

        def resident_epochs(n):
            seen = 0
            for epoch in range(n):
                resident.set_epoch(epoch)
                for x, labels in resident:
                    seen += x.shape[0]
            torch.cuda.synchronize()
            return seen

        loader_epochs(1)  # warm-up of every shape either window uses
        resident_epochs(2)
        t0 = time.perf_counter()
        resident_epochs(4)
        per_epoch = (time.perf_counter() - t0) / 4
        many = max(4, int(2.0 / per_epoch))  # a window of about two seconds
        rl, rr = [], []
        for _ in range(rounds):
            t0 = time.perf_counter()
            n = loader_epochs(2)
            rl.append(n / (time.perf_counter() - t0))
            t0 = time.perf_counter()
            n = resident_epochs(many)
            rr.append(n / (time.perf_counter() - t0))
        say("    loader path   (%2d workers decode every epoch, 2 epochs per round): %s"
            % (workers, spread(rl, "k img/s", 1e-3)))
        say("    resident path (no worker after the build, %d epochs per round)   : %s" % (many, spread(rr, "k img/s", 1e-3)))
        say("    one-time build of the store: %.1f s for %d images with %d workers (%.1f k img/s), %.3f GB on the device"
            % (build_s, files, workers, files / build_s / 1e3, store.data.numel() / 1e9))
        say("    host wall clock around loops that end in a device synchronise; the two paths alternate in one process")
    finally:
        shutil.rmtree(root, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--files", type=int, default=8192)
    ap.add_argument("--store", type=int, default=100000)
    ap.add_argument("--workers", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=2000)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("resident_time: needs a GPU")
    say("# tools/resident_time.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    kernel_times(args.store, args.rounds, args.launches)
    say()
    path_rates(args.files, args.workers, 3)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
