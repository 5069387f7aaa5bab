"""The loss, accuracy and optimiser kernels at the C ABI (fr_ce_rows, fr_rank_rows, fr_topk_precision, fr_focal_finalize,
fr_focal_bwd, fr_sgd_step, fr_adam_step), each called through ``ops.call`` with every output in a guarded buffer and held
to the numpy restatement of tests/loss_optim_ref.py (which tests/test_loss_optim_host.py holds to torch on the host).

Bars, and where each comes from:
  lse                 2e-6 relative + absolute against float64, the suite's bar for it (test_sharded_softmax_kernels)
  ce                  the worst row's |ce - ce64| / ce64 of a case, and |mean - mean64| / mean64 of its batch mean, at most
                      twice the same figure of fp32 ``F.cross_entropy`` on the host on the same input, or one fp32 ulp of
                      ce64 where that is more (__expf and the order of the sum account for the factor).  Both figures are
                      printed per case; profiles/ce_rows_error.txt keeps them
  rank, precision@k   exact
  finalize            scalars[4] within one fp32 ulp of the float64 mean, [2..3] exact; [0..1] against the float64 formula
                      at the fp32 mean the kernel left in [4]: at most 4 times the error of the same expression in fp32
                      torch on the host, or 4 ulp where that is more
  focal gradient      1e-5 of the largest entry against float64 (the suite's bar), rows sum to 0 within 1e-6 of it
  SGD                 bit for bit on operands whose every product and sum is exact in fp32; on random operands the bound
                      of ``test_sgd_random_operands_within_three_roundings``
  Adam                bit for bit the np.float32 restatement, operation by operation"""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_optim_ref as R
from head_support import SENTINEL, Guarded

pytestmark = pytest.mark.gpu

from frhip import _lib, ops  # noqa: E402

EPS32 = 2.0 ** -24


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def ulp32(x):
    """The spacing of fp32 at |x| (float64 in, float64 out)."""
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


def as_i32(g):
    """The interior of a guarded buffer as int32 (the sentinel bands stay what they are)."""
    return g.t.view(torch.int32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------------------------------------ fr_ce_rows, fr_rank_rows


def run_ce_rows(z, label, ld):
    """fr_ce_rows on z [rows, N] laid out at pitch ld with R.PAD behind every row: (lse, ce, rank) as numpy."""
    rows, N = z.shape
    zc, yc = dev(R.pitched(z, ld, R.PAD)), dev(label)
    lse, ce, rank = Guarded(rows), Guarded(rows), Guarded(rows)
    ops.call("fr_ce_rows", zc, yc, lse.t, ce.t, as_i32(rank), rows, N, ld, ops.current_stream_ptr())()
    torch.cuda.synchronize()
    for g, what in ((lse, "lse"), (ce, "ce"), (rank, "rank")):
        g.assert_guards("fr_ce_rows " + what)
    return lse.t.cpu().numpy(), ce.t.cpu().numpy(), as_i32(rank).cpu().numpy()


def run_rank_rows(z, label, ld):
    rows, N = z.shape
    rank = Guarded(rows)
    ops.call("fr_rank_rows", dev(R.pitched(z, ld, R.PAD)), dev(label), as_i32(rank), rows, N, ld,
             ops.current_stream_ptr())()
    torch.cuda.synchronize()
    rank.assert_guards("fr_rank_rows")
    return as_i32(rank).cpu().numpy()


def ce_figures(ce, ce64):
    """(worst row's relative error, relative error of the batch mean, one fp32 ulp of ce64 in the same units for each).
    A row whose float64 ce is exactly 0 (N = 1) must be exactly 0 and counts as error 0."""
    ce = np.asarray(ce, dtype=np.float64)
    zero = ce64 == 0
    assert (ce[zero] == 0).all(), ce[zero]
    safe = np.where(zero, 1.0, ce64)
    rel = np.where(zero, 0.0, np.abs(ce - ce64) / safe)
    floor = np.where(zero, 0.0, ulp32(ce64) / safe)
    m64 = ce64.mean()
    if m64 == 0:
        return rel.max(), 0.0, floor.max(), 0.0
    return rel.max(), abs(ce.mean() - m64) / m64, floor.max(), float(ulp32(m64)) / m64


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("rows,N,ld", R.CE_CASES)
def test_ce_rows(rows, N, ld, regime):
    """lse, ce and rank of Gaussian logits (std 3) and of confident logits s cos (s = 30, 64; float64 ce in 1e-3 .. 1e-1,
    tests/test_loss_optim_host.py checks the range), at a pitch ld >= N with 1e30 in the padding columns."""
    z, y = R.ce_case(rows, N, regime)
    lse64, ce64, rank64 = R.rows_ref(z, y)
    lse, ce, rank = run_ce_rows(z, y, ld)
    assert np.array_equal(rank, rank64), (rank, rank64)
    assert (np.abs(lse - lse64) <= 2e-6 * np.abs(lse64) + 2e-6).all(), np.abs(lse - lse64).max()
    t32 = F.cross_entropy(torch.from_numpy(z), torch.from_numpy(y), reduction="none").numpy()
    k_row, k_mean, floor_row, floor_mean = ce_figures(ce, ce64)
    t_row, t_mean, _, _ = ce_figures(t32, ce64)
    print("ce_rows rows=%d N=%d ld=%d %s: ce64 %.3e..%.3e | worst row rel err: kernel %.3e torch-fp32 %.3e | "
          "batch mean rel err: kernel %.3e torch-fp32 %.3e" % (rows, N, ld, regime, ce64.min(), ce64.max(), k_row, t_row,
                                                                 k_mean, t_mean))
    assert k_row <= max(2 * t_row, floor_row), (k_row, t_row, floor_row)
    assert k_mean <= max(2 * t_mean, floor_mean), (k_mean, t_mean, floor_mean)


@pytest.mark.parametrize("rows,N,ld", R.CE_CASES)
def test_ce_and_rank_rows_on_the_special_rows(rows, N, ld):
    """All-equal logits, the label at 0 and at N - 1, the label tied with two others, labels -1 and N (ce == lse bit for
    bit, rank N), an all-NaN row, a NaN off the label and a NaN label logit: rank exact against the restatement from both
    kernels, finite rows within the lse bar, and NaN exactly where float64 has it."""
    z, y, names = R.special_rows(N)
    lse64, ce64, rank64 = R.rows_ref(z, y)
    lse, ce, rank = run_ce_rows(z, y, ld)
    only_rank = run_rank_rows(z, y, ld)
    for i, name in enumerate(names):
        assert rank[i] == rank64[i] and only_rank[i] == rank64[i], (name, rank[i], only_rank[i], rank64[i])
        if name in ("label -1", "label N"):
            assert rank[i] == N and ce[i].tobytes() == lse[i].tobytes(), (name, rank[i], ce[i], lse[i])
        if name in ("all NaN", "NaN label logit"):
            assert rank[i] == N, (name, rank[i])
        if name == "all equal" or name.endswith("at the top"):
            assert rank[i] == 0, (name, rank[i])
        if np.isnan(lse64[i]):
            assert np.isnan(lse[i]) and np.isnan(ce[i]), (name, lse[i], ce[i])
        else:
            assert abs(lse[i] - lse64[i]) <= 2e-6 * abs(lse64[i]) + 2e-6, (name, lse[i], lse64[i])
            assert abs(ce[i] - ce64[i]) <= 2e-6 * abs(lse64[i]) + 4e-6, (name, ce[i], ce64[i])


@pytest.mark.parametrize("regime", R.REGIMES)
@pytest.mark.parametrize("rows,N,ld", R.CE_CASES)
def test_rank_rows_equals_ce_rows(rows, N, ld, regime):
    z, y = R.ce_case(rows, N, regime)
    rank = run_rank_rows(z, y, ld)
    assert np.array_equal(rank, R.rows_ref(z, y)[2]) and np.array_equal(rank, run_ce_rows(z, y, ld)[2])


def test_accuracy_counts_a_nan_row_and_a_missing_label_as_misses():
    """util.utils.accuracy end to end: of four rows whose label leads, one turned to NaN and one given the target -1 are
    misses at every k, as the reference's pred.eq(target) counts them."""
    from util.utils import accuracy
    z, y = R.ce_case(4, 33, "s30")
    z[1] = np.nan
    y[2] = -1
    p1, p5, p33 = accuracy(dev(z), dev(y), topk=(1, 5, 33))
    assert float(p1) == 50.0 and float(p5) == 50.0 and float(p33) == 50.0


# ------------------------------------------------------------------------------------------------ fr_topk_precision


@pytest.mark.parametrize("ks", [(1,), (1, 5), (1, 5, 10), (1, 3, 5, 1000), (0, 12), (5, 1, 0, 3)])
@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_topk_precision(rows, ks):
    """out[j] = float32(count_j) * float32(scale) bit for bit for nk = 1 .. 4, a k of 0 and a k above every rank included;
    out beyond nk keeps the sentinel."""
    rng = np.random.default_rng([rows, len(ks)])
    rank = rng.integers(0, 12, size=rows).astype(np.int32)
    scale = 100.0 / rows
    out = Guarded(4)
    kk = list(ks) + [7] * (4 - len(ks))  # the unused slots hold a k that would count if it were read
    ops.call("fr_topk_precision", dev(rank), rows, len(ks), kk[0], kk[1], kk[2], kk[3], scale, out.t,
             ops.current_stream_ptr())()
    torch.cuda.synchronize()
    out.assert_guards("fr_topk_precision")
    got = out.t.cpu().numpy()
    want = R.topk_ref(rank, ks, scale)
    assert got[:len(ks)].tobytes() == want.tobytes(), (got, want)
    assert (got[len(ks):] == np.float32(SENTINEL)).all(), got


# ------------------------------------------------------------------------------------------------ fr_focal_finalize


def _focal_torch32(l, gamma):
    """The kernel's expressions in fp32 torch on the host, at the fp32 mean l."""
    l = torch.tensor(float(l), dtype=torch.float32)
    p = torch.exp(-l)
    w = (1 - p) ** gamma
    return float(w * l), float(gamma * (1 - p) ** (gamma - 1.0) * p * l + w)


@pytest.mark.parametrize("rows", [1, 300])
@pytest.mark.parametrize("level", [1e-3, 0.02, 1.0, 9.0])
@pytest.mark.parametrize("gamma", [0.0, 0.5, 1.0, 2.0, 3.5])
def test_focal_finalize(gamma, level, rows):
    rng = np.random.default_rng([int(gamma * 2), int(level * 1000), rows])
    ce = (level * rng.uniform(0.5, 1.5, size=rows)).astype(np.float32)
    rank = rng.integers(0, 9, size=rows).astype(np.int32)
    sc = Guarded(8)
    ops.call("fr_focal_finalize", dev(ce), dev(rank), rows, float(gamma), sc.t, ops.current_stream_ptr())()
    torch.cuda.synchronize()
    sc.assert_guards("fr_focal_finalize")
    got = sc.t.cpu().numpy()
    assert (got[5:] == np.float32(SENTINEL)).all(), got
    ref = R.finalize_ref(ce, rank, gamma)
    assert abs(float(got[4]) - ref["mean"]) <= ulp32(ref["mean"]), (got[4], ref["mean"])
    assert got[2] == ref["prec1"] and got[3] == ref["prec5"], (got[2:4], ref["prec1"], ref["prec5"])
    want = R.focal_head(float(got[4]), gamma)  # float64, at the kernel's own fp32 mean
    t32 = _focal_torch32(got[4], gamma)
    for j, name in ((0, "loss"), (1, "slope")):
        k_err, t_err, floor = abs(float(got[j]) - want[j]), abs(t32[j] - want[j]), 4 * float(ulp32(want[j]))
        print("focal_finalize gamma=%g level=%g rows=%d %s: float64 %.9e | error: kernel %.3e torch-fp32 %.3e (ulp %.3e)"
              % (gamma, level, rows, name, want[j], k_err, t_err, floor / 4))
        assert k_err <= max(4 * t_err, floor), (name, got[j], want[j], k_err, t_err, floor)


# ------------------------------------------------------------------------------------------------ fr_focal_bwd


@pytest.mark.parametrize("padded", [False, True], ids=["ld=N", "ld>N"])
@pytest.mark.parametrize("N", [1, 33, 1023, 1024, 1025, 4133])
def test_focal_bwd(N, padded):
    """grad = k (softmax - onehot), k = gup * slope / rows, for slope in {1, 0.37} and gup in {1, -2.5}, against float64 at
    1e-5 of the largest entry; rows with a label sum to 0 within 1e-6 of their largest entry, the row whose label is -1 is
    k softmax, and the padding columns keep the sentinel.  lse is the float64 log-sum-exp rounded to fp32."""
    rows = 5
    ld = (N + 3) // 4 * 4 + 4 if padded else N
    rng = np.random.default_rng([N, ld])
    z = (3.0 * rng.standard_normal((rows, N))).astype(np.float32)
    y = rng.integers(0, N, size=rows)
    y[0], y[1], y[3] = 0, N - 1, -1
    lse64, _, _ = R.rows_ref(z, y)
    zc, yc, lc = dev(R.pitched(z, ld, R.PAD)), dev(y), dev(lse64.astype(np.float32))
    for slope in (1.0, 0.37):
        for gup in (1.0, -2.5):
            scalars = torch.full((8,), float("nan"), device="cuda")
            scalars[1] = slope
            grad = Guarded(rows, ld)
            ops.call("fr_focal_bwd", zc, yc, lc, scalars, torch.tensor([gup], device="cuda"), grad.t, rows, N, ld,
                     ops.current_stream_ptr())()
            torch.cuda.synchronize()
            grad.assert_guards("fr_focal_bwd")
            got = grad.t.cpu().numpy().astype(np.float64)
            assert (got[:, N:] == SENTINEL).all(), "fr_focal_bwd wrote padding columns"
            k = float(np.float32(gup)) * float(np.float32(slope)) / rows
            want = R.grad_ref(z, y, k)
            top = np.abs(want).max()
            assert np.abs(got[:, :N] - want).max() <= 1e-5 * top, (slope, gup, np.abs(got[:, :N] - want).max() / top)
            for m in range(rows):
                big = np.abs(got[m, :N]).max()
                if y[m] >= 0:
                    if N > 1:
                        assert abs(got[m, :N].sum()) <= 1e-6 * big, (m, got[m, :N].sum(), big)
                    else:
                        assert abs(got[m, 0]) <= 1e-6 * abs(k), (m, got[m, 0])  # softmax 1 minus onehot 1
                else:
                    sm = R.grad_ref(z[m:m + 1], np.array([-1]), k)[0]
                    assert np.abs(got[m, :N] - sm).max() <= 1e-5 * np.abs(sm).max(), (m, "k softmax")


# ------------------------------------------------------------------------------------------------ fr_sgd_step, fr_adam_step

SIZES = (1, 255, 257, 4095, 4096, 4097, 12289)
IDLE = 100  # one more tensor, in the table and in no chunk
GAP = 67  # sentinel floats between neighbours: odd, so the offsets run through every residue modulo 4


class Arena(object):
    """``names`` x (SIZES + IDLE) float32 tensors carved from ONE guarded buffer, a GAP of sentinels in front of each, at
    offsets that are multiples of 4 bytes and never of 16."""

    def __init__(self, names):
        self.names = names
        self.off, at = {}, 0
        for name in names:
            for t, n in enumerate(SIZES + (IDLE,)):
                at += GAP
                if at % 4 == 0:
                    at += 1
                self.off[name, t] = (at, n)
                at += n
        self.g = Guarded(at + GAP)
        self.base = self.g.t.data_ptr()
        assert self.base % 16 == 0 and all(o % 4 for o, _ in self.off.values())
        self.host = np.full(at + GAP, SENTINEL, dtype=np.float32)

    def set(self, name, t, values):
        o, n = self.off[name, t]
        self.host[o:o + n] = values

    def upload(self):
        self.g.t.copy_(torch.from_numpy(self.host))

    def ptr(self, name, t):
        return self.base + 4 * self.off[name, t][0]

    def download(self, what):
        """The arena as numpy after asserting the guards; the gaps between the tensors must hold the sentinel."""
        torch.cuda.synchronize()
        self.g.assert_guards(what)
        got = self.g.t.cpu().numpy()
        inside = np.zeros(got.shape, dtype=bool)
        for o, n in self.off.values():
            inside[o:o + n] = True
        assert (got[~inside] == np.float32(SENTINEL)).all(), (what, "a band between two tensors was written",
                                                               int((got[~inside] != np.float32(SENTINEL)).sum()))
        return got

    def get(self, got, name, t):
        o, n = self.off[name, t]
        return got[o:o + n]


def device_table(struct, records):
    arr = (struct * len(records))()
    for i, rec in enumerate(records):
        for key, value in rec.items():
            setattr(arr[i], key, value)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return raw, ctypes.cast(ctypes.c_void_p(raw.data_ptr()), ctypes.POINTER(struct))


def shuffled_chunks(seed):
    """(tensor, chunk) pairs of every tensor but the idle one, in a shuffled order, as a device int32 array."""
    chunk = _lib.lib.fr_sgd_chunk_elems()
    assert chunk == 4096  # SIZES straddle it
    pairs = [(t, c) for t, n in enumerate(SIZES) for c in range((n + chunk - 1) // chunk)]
    order = np.random.default_rng(seed).permutation(len(pairs))
    assert not np.array_equal(order, np.arange(len(pairs)))
    flat = np.array([pairs[i] for i in order], dtype=np.int32).reshape(-1)
    return dev(flat), len(pairs)


WD = (0.5, 0.25, 0.125, 0.0, 0.5, 0.125, 0.25, 0.5)  # per tensor, the idle one last; powers of two (and 0)


def _sgd_setup(fill, wds=WD):
    arena = Arena(("p", "g", "buf"))
    start = {}
    for name in arena.names:
        for t, n in enumerate(SIZES + (IDLE,)):
            start[name, t] = fill(name, t, n)
            arena.set(name, t, start[name, t])
    arena.upload()
    raw, table = device_table(_lib.FrSgdTensor, [dict(p=arena.ptr("p", t), g=arena.ptr("g", t), buf=arena.ptr("buf", t),
                                                      n=n, wd=wds[t]) for t, n in enumerate(SIZES + (IDLE,))])
    return arena, start, raw, table


def test_sgd_step_bit_for_bit_on_exact_operands():
    """Integer p, g, buf in [-64, 64], wd in {0, 1/8, 1/4, 1/2} per tensor, momentum 1/2, lr 1/4: after two steps every
    value is a multiple of 2^-10 below 2^8, so each product and sum is exact in fp32 with or without FMA contraction, and p
    and buf equal the float64 restatement bit for bit.  g, the bands and the tensor that has no chunk are untouched; a
    chunk tail updated twice, or with the neighbour's wd, changes bits."""
    rng = np.random.default_rng(11)
    arena, start, raw, table = _sgd_setup(lambda name, t, n: rng.integers(-64, 65, size=n).astype(np.float32))
    chunks, nchunks = shuffled_chunks(12)
    momentum, lr = 0.5, 0.25
    p = {t: start["p", t].astype(np.float64) for t in range(len(SIZES))}
    buf = {t: start["buf", t].astype(np.float64) for t in range(len(SIZES))}
    for step in range(2):
        ops.Launch("fr_sgd_step", [table, ctypes.c_void_p(chunks.data_ptr()), nchunks, lr, momentum,
                                   ops.current_stream_ptr()])()
        got = arena.download("fr_sgd_step, step %d" % step)
        for t in range(len(SIZES)):
            p[t], buf[t] = R.sgd_step_ref(p[t], start["g", t], buf[t], WD[t], momentum, lr)
            for name, want in (("p", p[t]), ("buf", buf[t])):
                w32 = want.astype(np.float32)
                assert (w32.astype(np.float64) == want).all()  # the restatement itself is exact in fp32
                assert arena.get(got, name, t).tobytes() == w32.tobytes(), (step, name, t, SIZES[t])
            assert arena.get(got, "g", t).tobytes() == start["g", t].tobytes(), (step, "g", t)
        for name in arena.names:
            assert arena.get(got, name, len(SIZES)).tobytes() == start[name, len(SIZES)].tobytes(), (step, "idle tensor", name)
    assert all(np.abs(p[t] * 1024 - np.round(p[t] * 1024)).max() == 0 and np.abs(p[t]).max() < 256 for t in p)


def test_sgd_random_operands_within_three_roundings():
    """Gaussian operands, wd = WD / 250, momentum 0.9, lr 0.03, one step, against float64 on the same fp32 inputs and
    scalars.  The kernel rounds three times per element: d = fma(wd, p, g), b = fma(momentum, buf, d), p' = p - lr b
    (four times if the last product is not contracted).  With e = 2^-24 per rounding, to first order:
    |b - b64| <= e (|d| + |b|) and |p' - p'64| <= lr |b - b64| + e (|lr b| + |p'|); the bar is that bound times 1.001 for
    the terms of second order."""
    rng = np.random.default_rng(13)
    wds = [float(np.float32(w / 250)) for w in WD]
    arena, start, raw, table = _sgd_setup(lambda name, t, n: rng.standard_normal(n).astype(np.float32), wds)
    chunks, nchunks = shuffled_chunks(14)
    momentum, lr = 0.9, 0.03
    m32, lr32 = float(np.float32(momentum)), float(np.float32(lr))  # the scalars cross the C ABI as fp32
    ops.Launch("fr_sgd_step", [table, ctypes.c_void_p(chunks.data_ptr()), nchunks, lr, momentum, ops.current_stream_ptr()])()
    got = arena.download("fr_sgd_step, random operands")
    for t in range(len(SIZES)):
        p0, g0, b0 = (start[name, t].astype(np.float64) for name in ("p", "g", "buf"))
        p64, b64 = R.sgd_step_ref(p0, g0, b0, wds[t], m32, lr32)
        d64 = g0 + wds[t] * p0
        bound_b = 1.001 * EPS32 * (np.abs(d64) + np.abs(b64))
        bound_p = lr32 * bound_b + 1.001 * EPS32 * (np.abs(lr32 * b64) + np.abs(p64))
        eb = np.abs(arena.get(got, "buf", t) - b64)
        ep = np.abs(arena.get(got, "p", t) - p64)
        assert (eb <= bound_b).all() and (ep <= bound_p).all(), (t, SIZES[t], (eb / bound_b).max(), (ep / bound_p).max())
        assert (eb > 0).any() or SIZES[t] == 1  # the bound is not vacuous: fp32 does round here
        assert arena.get(got, "g", t).tobytes() == start["g", t].tobytes()
    for name in arena.names:
        assert arena.get(got, name, len(SIZES)).tobytes() == start[name, len(SIZES)].tobytes(), ("idle tensor", name)


def test_sgd_and_adam_launch_nothing_without_chunks():
    """nchunks = 0 returns 0 and writes nothing, whatever the tables hold."""
    arena, start, raw, table = _sgd_setup(lambda name, t, n: np.full(n, float(t + 1), dtype=np.float32))
    before = arena.download("before").copy()
    chunks, _ = shuffled_chunks(15)
    assert _lib.lib.fr_sgd_step(table, ctypes.c_void_p(chunks.data_ptr()), 0, 0.25, 0.5, ops.current_stream_ptr()) == 0
    adam_table = ctypes.cast(ctypes.c_void_p(raw.data_ptr()), ctypes.POINTER(_lib.FrAdamTensor))
    assert _lib.lib.fr_adam_step(adam_table, ctypes.c_void_p(chunks.data_ptr()), 0, 1e-3, 0.1, 0.999, 0.001, 1e-8, 0.03,
                                 ops.current_stream_ptr()) == 0
    assert arena.download("nchunks = 0").tobytes() == before.tobytes()


def test_adam_step_bit_for_bit():
    """Three steps from m = v = 0 with Gaussian p and gradients scaled 1e-3, 1 and 1e3: p, m and v are bit for bit the
    np.float32 restatement after each step (lerp; mul + addcmul; sqrt / bc2_sqrt + eps; addcdiv, every operation rounded
    on its own), g, the bands and the tensor without a chunk untouched."""
    rng = np.random.default_rng(17)
    arena = Arena(("p", "g", "m", "v"))
    state = {}
    for t, n in enumerate(SIZES + (IDLE,)):
        state["p", t] = rng.standard_normal(n).astype(np.float32)
        state["m", t], state["v", t] = np.zeros(n, np.float32), np.zeros(n, np.float32)
    raw, table = device_table(_lib.FrAdamTensor, [dict(p=arena.ptr("p", t), g=arena.ptr("g", t), m=arena.ptr("m", t),
                                                       v=arena.ptr("v", t), n=n) for t, n in enumerate(SIZES + (IDLE,))])
    chunks, nchunks = shuffled_chunks(18)
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    for step, scale in enumerate((1e-3, 1.0, 1e3), 1):
        for t in range(len(SIZES) + 1):
            state["g", t] = (scale * rng.standard_normal(state["p", t].size)).astype(np.float32)
            for name in arena.names:
                arena.set(name, t, state[name, t])
        arena.upload()
        sc = R.adam_scalars(lr, betas, eps, step)
        ops.Launch("fr_adam_step", [table, ctypes.c_void_p(chunks.data_ptr()), nchunks] +
                   [float(sc[key]) for key in ("step_size", "w1", "beta2", "w2", "eps", "bc2_sqrt")] +
                   [ops.current_stream_ptr()])()
        got = arena.download("fr_adam_step, step %d" % step)
        for t in range(len(SIZES)):
            p, m, v = R.adam_step_ref(state["p", t], state["g", t], state["m", t], state["v", t], sc)
            for name, want in (("p", p), ("m", m), ("v", v)):
                mine = arena.get(got, name, t)
                diff = int((mine.view(np.int32) != want.view(np.int32)).sum())
                assert diff == 0, (step, name, t, SIZES[t], diff, "elements differ from the fp32 restatement")
            assert arena.get(got, "g", t).tobytes() == state["g", t].tobytes()
            state["p", t], state["m", t], state["v", t] = p, m, v
        for name in arena.names:
            assert arena.get(got, name, len(SIZES)).tobytes() == state[name, len(SIZES)].tobytes(), (step, "idle", name)
