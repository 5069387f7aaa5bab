"""GPU tests of RandAugment on the input pipeline (fr_randaug_u8 in csrc/input_pipeline.hip, frhip.input_pipeline.GpuRandAugment,
config key GPU_RANDAUGMENT).  Every comparison is bit for bit against the numpy restatement of tests/randaug_ref.py, which
tests/test_randaug_host.py pins against Pillow:

  single steps      each served operation alone, 10 magnitudes x 2 signs (+ a constant and a low-range image) in one batch, in
                    guarded buffers, at 112x112, 37x53 (row bytes no multiple of 4), 9x7 (fewer pixels than lanes) and 128x128
                    (the largest shape of the LDS budget); 148x148 is refused and nothing is launched
  chains            K = 1, 4, 6, 16 with the order-sensitive pairs, identity padding inside and at the end, twice: same bytes
  gather            idx with repeats and in reverse from a 40-image store, the labels, idx = NULL against idx = arange
  the transform     GpuTrainTransform under the profiler: randaug=None is the one launch of before, set it is one more, and
                    the float batch is oracle/input_ref.py's train transform of the restatement's image
  train.py          finite losses, resume at the epoch boundary, the resident run equal to the loader run
"""
import re

import numpy as np
import pytest
import torch

import head_support as HS
import randaug_ref as R

pytestmark = pytest.mark.gpu

SIZES = [(112, 112), (37, 53), (9, 7), (128, 128)]


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _ranges():
    from frhip.input_pipeline import RANDAUG_RANGES
    return RANDAUG_RANGES


class Bytes(object):
    """A uint8 buffer of ``shape`` inside ``HS.Guarded`` (whose element is a float: up to 3 slack bytes follow the buffer
    inside the interior and are held to their sentinel pattern as well)."""

    def __init__(self, *shape):
        self.n = int(np.prod(shape))
        self.g = HS.Guarded((self.n + 3) // 4)
        self.raw = self.g.t.view(torch.uint8)
        self.t = self.raw[:self.n].view(*shape)
        self.slack = self.raw[self.n:].clone()
        self.before = self.t.clone()

    def assert_guards(self, what):
        self.g.assert_guards(what)
        assert torch.equal(self.raw[self.n:], self.slack), (what, "bytes behind the buffer written")


def _launch(src, op, par, h, w, idx=None, labels=None, m=None):
    """fr_randaug_u8 at the C ABI into guarded buffers: (uint8 [B,h,w,3] numpy, int64 labels or None)."""
    from frhip import ops
    b, k = op.shape
    dst = Bytes(b, h, w, 3)
    lab = HS.Guarded(2 * b) if labels is not None else None
    label_out = lab.t.view(torch.int64) if lab is not None else None
    before = src.clone()
    ops.call("fr_randaug_u8", src, labels, idx, torch.as_tensor(op, dtype=torch.uint8).cuda(),
             torch.as_tensor(par, dtype=torch.float32).cuda(), dst.t, label_out, src.shape[0] if m is None else m, b, k, h, w,
             ops.current_stream_ptr())()
    torch.cuda.synchronize()
    dst.assert_guards("dst")
    if lab is not None:
        lab.assert_guards("label_out")
    assert torch.equal(src, before), "the source was written"
    return dst.t.cpu().numpy(), (label_out.clone() if lab is not None else None)


def _step(name, m, sign, h, w):
    return R.CODE[name], R.parameter(name, _ranges()[name][m], sign, h, w)


def _want(images, op, par):
    return np.stack([R.chain(img, op[b], par[b]) for b, img in enumerate(images)])


# ------------------------------------------------------------------------------------------------ single steps


@pytest.mark.parametrize("h,w", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("name", R.SERVED)
def test_each_operation_alone_is_the_restatement(name, h, w):
    _need_gpu()
    rng = np.random.default_rng(h * 1000 + w)
    images = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(20)]
    steps = [_step(name, m, sign, h, w) for m in range(10) for sign in (-1, 1)]
    for sign in (-1, 1):  # a flat image (hi <= lo in autocontrast, the contrast of a constant) and one of range 90..153
        images += [np.broadcast_to(np.array([200, 17, 90], np.uint8), (h, w, 3)).copy(),
                   rng.integers(90, 154, (h, w, 3), dtype=np.uint8)]
        steps += [_step(name, 9, sign, h, w)] * 2
    op = np.array([[s[0]] for s in steps], np.uint8)
    par = np.array([[s[1]] for s in steps], np.float32)
    got, _ = _launch(torch.from_numpy(np.stack(images)).cuda(), op, par, h, w)
    want = _want(images, op, par)
    bad = [b for b in range(len(images)) if not np.array_equal(got[b], want[b])]
    assert not bad, (name, h, w, bad, int((got != want).sum()))
    if name not in ("equalize", "autocontrast"):  # the step did something (autocontrast: a full-range image stays)
        assert any(not np.array_equal(want[b], images[b]) for b in range(len(images))), name


def test_an_image_beyond_the_lds_budget_is_refused_and_nothing_is_launched():
    _need_gpu()
    from frhip import _lib, ops
    h = w = 148
    src = torch.zeros(2, h, w, 3, dtype=torch.uint8, device="cuda")
    dst = Bytes(2, h, w, 3)
    op, par = torch.full((2, 1), 9, dtype=torch.uint8).cuda(), torch.zeros(2, 1).cuda()
    launch = ops.call("fr_randaug_u8", src, None, None, op, par, dst.t, None, 2, 2, 1, h, w, ops.current_stream_ptr())
    failures = []

    def run():
        try:
            launch()
        except _lib.FrhipError as e:
            failures.append(str(e))

    names = HS.profiled_names(run)
    assert len(failures) == 1 and "fr_randaug_u8" in failures[0] and "LDS" in failures[0], failures
    assert not [n for n in names if "randaug" in n and "kernel" in n], sorted(set(names))
    assert torch.equal(dst.t, dst.before)
    dst.assert_guards("dst of the refused call")
    # the largest square inside the budget launches (control of the profiler's view)
    src = torch.zeros(1, 128, 128, 3, dtype=torch.uint8, device="cuda")
    out = torch.empty_like(src)
    ok = ops.call("fr_randaug_u8", src, None, None, op[:1], par[:1], out, None, 1, 1, 1, 128, 128, ops.current_stream_ptr())
    assert any("randaug_u8_kernel" in n for n in HS.profiled_names(ok))
    assert bool((out == 255).all())


# ------------------------------------------------------------------------------------------------ chains

ORDER_SENSITIVE = [
    [("color", 7, -1), ("contrast", 9, 1)],  # contrast after color: the mean is that of the recoloured image
    [("brightness", 9, 1), ("autocontrast", 0, 1)],  # brightness 1.3 saturates a channel before the table is built
    [("translateX", 6, 1), ("contrast", 8, 1)],  # the black pixels enter the mean
    [("translateX", 5, -1), ("translateY", 7, 1)],  # two shifts in a row (they commute: both orders give one image)
    [("contrast", 9, 1), ("contrast", 9, -1)],  # two contrasts in a row: two different means
]
PADDED = [("solarize", 9, 1), ("equalize", 0, 1), ("posterize", 9, 1), ("equalize", 0, 1), ("invert", 0, 1),
          ("autocontrast", 0, 1)]  # the identity inside a chain


def _chains(k, h, w, rng):
    """One chain per image, each padded with code 0 to ``k`` steps: the order-sensitive pairs in both orders, the chain
    with the identity inside, and random chains of full length."""
    chains = [c[:k] for c in ORDER_SENSITIVE] + [c[::-1][:k] for c in ORDER_SENSITIVE] + [PADDED[:k]]
    names = [n for n in R.SERVED]
    for _ in range(5):
        chains.append([(names[rng.integers(len(names))], int(rng.integers(10)), int(rng.choice([-1, 1]))) for _ in range(k)])
    op, par = np.zeros((len(chains), k), np.uint8), np.zeros((len(chains), k), np.float32)
    for b, chain in enumerate(chains):
        for j, (name, m, sign) in enumerate(chain):
            op[b, j], par[b, j] = _step(name, m, sign, h, w)
    return op, par


@pytest.mark.parametrize("h,w", [(112, 112), (37, 53)], ids=["112x112", "37x53"])
@pytest.mark.parametrize("k", [1, 4, 6, 16])
def test_chains_are_the_restatement_and_repeat_bit_for_bit(k, h, w):
    _need_gpu()
    rng = np.random.default_rng(100 * k + h)
    op, par = _chains(k, h, w, rng)
    base = rng.integers(20, 236, (h, w, 3), dtype=np.uint8)  # one image for all (short of the full range, so autocontrast acts)
    images = [base] * len(op)
    src = torch.from_numpy(np.stack(images)).cuda()
    got, _ = _launch(src, op, par, h, w)
    want = _want(images, op, par)
    bad = [b for b in range(len(images)) if not np.array_equal(got[b], want[b])]
    assert not bad, (k, h, w, bad, [op[b].tolist() for b in bad])
    if k >= 2:  # the order matters to the reference on these inputs, so a kernel that ignored it would fail above
        n = len(ORDER_SENSITIVE)
        differ = [not np.array_equal(want[b], want[n + b]) for b in range(n)]
        assert differ == [True, True, True, False, True], differ
        assert (op[:n, 2:] == 0).all()  # and these chains end in identity padding
    again, _ = _launch(src, op, par, h, w)
    assert np.array_equal(again, got)


# ------------------------------------------------------------------------------------------------ gather


@pytest.mark.parametrize("h,w,offset", [(112, 112, 0), (112, 112, 4), (37, 53, 0)], ids=["112x112", "112x112+4", "37x53"])
def test_gather_from_a_store(h, w, offset):
    """``offset``: the store starts that many bytes behind a 16-byte boundary, so its images are read bytewise while the
    batch is written in 16-byte pieces."""
    _need_gpu()
    M = 40
    rng = np.random.default_rng(h + offset)
    data = rng.integers(0, 256, (M, h, w, 3), dtype=np.uint8)
    flat = torch.zeros(offset + data.size, dtype=torch.uint8, device="cuda")
    flat[offset:] = torch.from_numpy(data).cuda().view(-1)
    store = flat[offset:].view(M, h, w, 3)
    assert store.data_ptr() % 16 == offset
    labels = torch.from_numpy(rng.integers(0, 2 ** 40, M, dtype=np.int64)).cuda()
    idx_list = list(range(M - 1, -1, -1)) + [5, 5, M - 1, 0]  # reverse order, repeats, both ends of the store
    B, K = len(idx_list), 3
    names = list(R.SERVED)
    op, par = np.zeros((B, K), np.uint8), np.zeros((B, K), np.float32)
    for b in range(B):
        for j in range(K):
            op[b, j], par[b, j] = _step(names[rng.integers(len(names))], int(rng.integers(10)), int(rng.choice([-1, 1])), h, w)
    idx = torch.tensor(idx_list, dtype=torch.int32).cuda()
    got, lab = _launch(store, op, par, h, w, idx, labels)
    want = _want([data[i] for i in idx_list], op, par)
    assert np.array_equal(got, want), int((got != want).sum())
    assert torch.equal(lab, labels[idx.long()])
    got2, none = _launch(store, op, par, h, w, idx, None)  # no labels at either end
    assert none is None and np.array_equal(got2, want)
    # idx = NULL is idx = arange
    a, la = _launch(store, op[:M], par[:M], h, w, torch.arange(M, dtype=torch.int32).cuda(), labels)
    b_, lb = _launch(store, op[:M], par[:M], h, w, None, labels)
    assert np.array_equal(a, b_) and np.array_equal(a, _want(list(data), op[:M], par[:M]))
    assert torch.equal(la, labels) and torch.equal(lb, labels)


# ------------------------------------------------------------------------------------------------ the transform


def _kernels(fn):
    """Names of the device-side kernel events of ``fn`` (copies and memsets left out), in order of launch."""
    from torch.autograd import DeviceType
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA
          and not any(s in e.name.lower() for s in ("memcpy", "memset", "copy"))]
    return [e.name for e in sorted(ev, key=lambda e: e.time_range.start)]


def test_train_transform_with_and_without_randaug():
    _need_gpu()
    from frhip.input_pipeline import GpuRandAugment, GpuTrainTransform
    from oracle import input_ref
    B, h, w = 6, 112, 112
    rng = np.random.default_rng(9)
    images = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    u8 = torch.from_numpy(images).cuda()
    plain, ra = GpuTrainTransform(112), GpuRandAugment(num=4)
    withra = GpuTrainTransform(112, randaug=ra)
    assert plain.randaug is None and withra.randaug is ra
    crop, flip = plain.draw(B, torch.Generator().manual_seed(1))
    op, par = ra.draw(B, torch.Generator().manual_seed(2), (h, w))
    plain(u8, crop, flip), withra(u8, crop, flip, op=op, par=par)  # first calls: tables, allocator
    torch.cuda.synchronize()

    out = {}
    k_plain = _kernels(lambda: out.__setitem__("plain", plain(u8, crop, flip)))
    k_ra = _kernels(lambda: out.__setitem__("ra", withra(u8, crop, flip, op=op, par=par)))
    assert len(k_plain) == 1 and "augment_u8_kernel" in k_plain[0], k_plain  # the one launch of before
    assert len(k_ra) == 2 and "randaug_u8_kernel" in k_ra[0] and k_ra[1] == k_plain[0], k_ra  # one more, in front

    def oracle(imgs):
        return np.stack([input_ref.train_transform(imgs[b], 112, (int(crop[b, 0]), int(crop[b, 1])), bool(flip[b]))
                         for b in range(B)])

    assert np.array_equal(out["plain"].cpu().numpy(), oracle(images))
    aug = _want(list(images), op.numpy(), par.numpy())
    assert any(not np.array_equal(aug[b], images[b]) for b in range(B))
    assert np.array_equal(out["ra"].cpu().numpy(), oracle(aug))
    assert np.array_equal(ra(u8, op, par).cpu().numpy(), aug)  # the class alone: the uint8 batch

    # drawn inside the call: crop / flip first, then the chain, from the one generator
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    got = withra(u8, generator=g1)
    crop2, flip2 = withra.draw(B, g2)
    op2, par2 = ra.draw(B, g2, (h, w))
    assert torch.equal(got, withra(u8, crop2, flip2, op=op2, par=par2)) and torch.equal(g1.get_state(), g2.get_state())
    with pytest.raises(ValueError, match="LDS budget"):
        withra(torch.zeros(1, 148, 148, 3, dtype=torch.uint8, device="cuda"))


# ------------------------------------------------------------------------------------------------ train.py

LOADER = dict(HEAD_NAME="ArcFace", GPU_INPUT_PIPELINE=True, GPU_RANDAUGMENT=True)
RESIDENT = dict(LOADER, GPU_RESIDENT_DATASET=True)


def _loss_lines(log):
    return [l for l in log.splitlines() if "Training Loss" in l]


def _assert_same_state_file(a_dir, b_dir, last):
    sa = torch.load(HS.ckpt(a_dir, "State_ArcFace_" + last), map_location="cpu")
    sb = torch.load(HS.ckpt(b_dir, "State_ArcFace_" + last), map_location="cpu")
    assert list(sa.keys()) == list(sb.keys()), (list(sa.keys()), list(sb.keys()))
    for key in sa:
        same = torch.equal(sa[key], sb[key]) if torch.is_tensor(sa[key]) else sa[key] == sb[key]
        assert same, ("State_", key)


@pytest.fixture(scope="module")
def randaug_runs(tmp_path_factory):
    """Two epochs of the loader run with RandAugment straight, and stopped at the epoch boundary and resumed (``HS.resumed``
    compares the Backbone_*, Head_* and Optimizer_* files of the two end states bit for bit)."""
    _need_gpu()
    return HS.resumed(tmp_path_factory.mktemp("randaug"), LOADER, "ArcFace")


def test_train_with_randaug_resumes_bit_for_bit(randaug_runs):
    r = randaug_runs
    losses = [float(m.group(1)) for m in re.finditer(r"Training Loss ([0-9.eE+-]+|nan|inf) \(", r.a_log)]
    print("losses per step:", losses)
    assert len(losses) == 12 and all(np.isfinite(losses)), "%s\n%s" % (losses, r.a_log[-2000:])
    assert "Prec@1" in r.a_log and "nan" not in r.a_log.lower(), r.a_log[-2000:]
    assert r.a_log.count("GPU RandAugment: 5 operations per image") == 1, r.a_log[:3000]
    _assert_same_state_file(r.a_dir, r.b2_dir, "Epoch_2_Batch_12_")  # the fourth checkpoint file


def test_train_resident_run_equals_the_loader_run(randaug_runs, tmp_path):
    r = randaug_runs
    d, log = HS.run_train(tmp_path, "resident", RESIDENT)
    assert log.count("Resident dataset: 120 images") == 1 and "GPU RandAugment" in log
    assert len(_loss_lines(log)) == 14 and _loss_lines(log) == _loss_lines(r.a_log), (log[-1500:], r.a_log[-1500:])
    for last in ("Epoch_1_Batch_6_", "Epoch_2_Batch_12_"):
        HS.assert_same_checkpoints(r.a_dir, d, "ArcFace", last)
        _assert_same_state_file(r.a_dir, d, last)


def test_train_refuses_randaug_on_the_host_workers(tmp_path):
    _need_gpu()
    out = HS.run_train(tmp_path, "refused", dict(HEAD_NAME="ArcFace", GPU_RANDAUGMENT=True), max_steps=1, ok=False, limit=120)
    assert out.returncode != 0 and "GPU_RANDAUGMENT=True needs GPU_INPUT_PIPELINE=True" in out.stderr, out.stderr[-1500:]
    assert "Number of Training Classes" not in out.stdout  # before any device work
