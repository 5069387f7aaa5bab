"""Integer-valued operands for the bf16 convolution kernels, float64 references and bit-exact comparators.

Why: on Gaussian data a bf16 kernel can only be compared to a tolerance (tests/test_gpu_kernels.py), and an addressing
or coverage defect smaller than one rounding passes.  Here every operand is a small integer (or a small integer times a
power of two) and every true result fits the format it is stored in: bf16 MFMA products with fp32 accumulation, the
one-fmaf prologues, the fp32 epilogue sums, the slab sums and the bf16 store are then exact in ANY summation order, and a
kernel must equal an integer reference bit for bit -- at every pixel, part row and weight-gradient element.

A plain helper module (like shard_ref.py), used by test_exact_operands_host.py (no GPU) and test_gpu_exact_conv.py.
Layout: activations NHWC ``[B, H, W, C]``, weights packed ``[O][kh*kw][I]`` -- what the C ABI takes.
"""
import math

import torch
import torch.nn.functional as F

from frhip import synth

FP32_HALF_RANGE = float(2 ** 23)  # half of the fp32 integer range: the margin every sum keeps
BASE_IMAGES = 8                   # images drawn from the counter-based generator; a batch repeats them channel-rolled

PRO = {"none": 0, "bn": 1, "prelu": 2}


# ------------------------------------------------------------------------------------------------------------ densities
# Share of non-zero entries of a ternary tensor, keyed (cin, W) of the layer that reads it.  Default sqrt(64 / (9 cin)):
# a 3x3 output is then a sum of ~64 * sqrt(64 / (9 cin)) * ... non-zero products, |output| 73 .. 126 on the project's shapes.
# 112x112: the per-image, per-channel sum of y^2 must stay below 2^23 (assert_exact_range), which the default misses
# (1.28e7 with a BatchNorm prologue): 12544 pixels x E[y^2] <= 2^23 needs E[y^2] < 668; p = 0.2 gives ~ 110.
DENSITY = {(64, 112): 0.2}


def density(cin, W=0, taps=9):
    return DENSITY.get((cin, W), min(1.0, math.sqrt(64.0 / (taps * cin))))


# ------------------------------------------------------------------------------------------------------------ generators
def ternary(seed, tag, shape, p, neg=-1.0, pos=1.0):
    """float32 tensor with values {neg, 0, pos}: P(neg) = P(pos) = p / 2 (frhip.synth counter-based stream)."""
    u = synth.uniform(seed, tag, shape, 0.0, 1.0)
    t = torch.zeros(shape)
    t[u < p / 2] = neg
    t[u >= 1.0 - p / 2] = pos
    return t


def pick(seed, tag, n, values, weights=None):
    """n values drawn from the list `values` (optionally with cumulative shares `weights` that add up to 1)."""
    u = synth.uniform(seed, tag, (n,), 0.0, 1.0).double()
    if weights is None:
        idx = (u * len(values)).long().clamp_max(len(values) - 1)
    else:
        edges = torch.tensor(weights, dtype=torch.float64).cumsum(0)
        idx = torch.bucketize(u, edges, right=True).clamp_max(len(values) - 1)
    return torch.tensor(values, dtype=torch.float32)[idx]


def activations(seed, tag, hwc, p, pro="none", nb=BASE_IMAGES):
    """Base images [nb, H, W, C].  Behind a PReLU prologue the negative value is -4, so that slopes 0.25 / 0.5 leave
    integers (-1 / -2) and the convolution stays an integer sum."""
    return ternary(seed, tag, (nb,) + tuple(hwc), p, neg=-4.0 if pro == "prelu" else -1.0)


def prologue_coeffs(seed, tag, C, pro):
    """(a, b) of the prologue: BN scale from {1, 2, -1}, shift from {-1, 0, 1} with 7 / 8 of the channels at 0 (a shift
    turns every zero of a sparse activation into a term); PReLU slopes from {0.25, 0.5}."""
    if pro == "bn":
        return pick(seed, tag + ".a", C, [1.0, 2.0, -1.0]), pick(seed, tag + ".b", C, [0.0, -1.0, 1.0], [0.875, 0.0625, 0.0625])
    if pro == "prelu":
        return pick(seed, tag + ".a", C, [0.25, 0.5]), torch.zeros(C)
    return torch.ones(C), torch.zeros(C)


def batch(base, B, sel=None, device=None):
    """Images `sel` (default: all B) of the batch built on `base`: image b = base[b % nb] with its channels rolled by
    b // nb -- distinct images from nb generated ones, identical on host and device."""
    nb = base.shape[0]
    if device is not None:
        base = base.to(device)
    if sel is None:
        reps = [torch.roll(base, k, dims=-1) for k in range((B + nb - 1) // nb)]
        return torch.cat(reps, 0)[:B].contiguous()
    return torch.stack([torch.roll(base[b % nb], b // nb, dims=-1) for b in sel], 0)


def padded(t, ld, fill=float("nan")):
    """[rows..., C] -> a view with row stride ld >= C inside a buffer whose padding columns hold `fill` (NaN: an operand read
    from the padding poisons the result)."""
    C = t.shape[-1]
    if ld == C:
        return t.contiguous()
    buf = torch.full(tuple(t.shape[:-1]) + (ld,), fill, dtype=t.dtype, device=t.device)
    buf[..., :C] = t
    return buf[..., :C]


# ------------------------------------------------------------------------------------------------------------ references
def _ch(v, like):
    return v.to(like.device, torch.float64)


def apply_prologue(x, pro, a, b):
    """float64 NHWC operand the MFMAs see."""
    x = x.double()
    if pro == "bn":
        return x * _ch(a, x) + _ch(b, x)
    if pro == "prelu":
        return torch.where(x > 0, x, x * _ch(a, x))
    return x


def _oihw(w, k):
    O, taps, Ci = w.shape
    return w.double().view(O, k, k, Ci).permute(0, 3, 1, 2)


def conv_forward(xin, w, stride=1, k=3):
    """xin: float64 NHWC (prologue applied), w [O][k*k][I] -> float64 NHWC accumulators."""
    y = F.conv2d(xin.double().permute(0, 3, 1, 2), _oihw(w, k), stride=stride, padding=k // 2)
    return y.permute(0, 2, 3, 1).contiguous()


def conv_dgrad(g, w, stride, H, k=3):
    """Data gradient (autograd's backward of F.conv2d): g NHWC [B, H/stride, H/stride, O], w [O][k*k][I] -> [B, H, H, I]."""
    gx = torch.nn.grad.conv2d_input((g.shape[0], w.shape[2], H, H), _oihw(w, k), g.double().permute(0, 3, 1, 2),
                                    stride=stride, padding=k // 2)
    return gx.permute(0, 2, 3, 1).contiguous()


def conv_wgrad(g, xin, stride=1, k=3):
    """Weight gradient (autograd's backward of F.conv2d), packed [O][k*k][I]."""
    O, Ci = g.shape[-1], xin.shape[-1]
    gw = torch.nn.grad.conv2d_weight(xin.double().permute(0, 3, 1, 2), (O, Ci, k, k), g.double().permute(0, 3, 1, 2),
                                     stride=stride, padding=k // 2)
    return gw.permute(0, 2, 3, 1).reshape(O, k * k, Ci).contiguous()


def epilogue(kind, acc, aux=None, ea=None, eb=None):
    """What an FR_EPI_* kind stores and sums (include/frhip.h), in float64 on any device.
    Returns (stored [B,H,W,C], terms): `terms` = the elementwise summands of each part vector, in part order."""
    v = acc.double()
    x = aux.double() if aux is not None else None
    if kind == "store":
        return v, []
    if kind == "stats":
        return v, [v, v * v]
    if kind == "stats_x":
        return v, [v, v * v, v * x]
    if kind == "prelu_bwd":
        pos = x > 0
        return torch.where(pos, v, v * _ch(ea, v)), [torch.where(pos, torch.zeros_like(v), v * x)]
    if kind == "bnbwd":
        return v, [v, v * ((x - _ch(ea, v)) * _ch(eb, v))]
    if kind == "bias_res":
        return v + _ch(ea, v) + _ch(eb, v) + x, []
    raise ValueError(kind)


def column_sums(terms):
    """[k][C] float64 per-channel sums over all images and pixels."""
    return torch.stack([t.sum((0, 1, 2)) for t in terms], 0)


def images_per_part_row(nparts, B):
    """1, 2 or 4: rows are whole strips / items of one image, or one row per group of 2 / 4 images (7x7)."""
    return 1 if nparts >= B else -(-B // nparts)


# ------------------------------------------------------------------------------------------------------------ preconditions
def _quantum(t, quantum):
    m = t.double() / quantum
    return m, bool((m == m.round()).all())


def assert_exact_range(stored=(), terms=(), images_per_row=1, quantum=1.0, term_quantum=None, wgrad_abs=None, what=""):
    """The preconditions of exactness, asserted on the REFERENCE before anything is compared.
      stored   : tensors the kernel stores as bf16 -- multiples of `quantum` (a power of two), every element with at most 8
                 significant bits (for plain integers: |v| <= 256), i.e. unchanged by a round trip through bf16
      terms    : per sum kind the elementwise summands [B, H, W, C] -- multiples of `term_quantum` (default quantum^2) whose
                 per-image, per-channel sum of magnitudes, times the images one part row can hold, is <= 2^23 quanta (half
                 the fp32 integer range)
      wgrad_abs: an upper bound of sum |g * x| over every weight-gradient element, <= 2^23 quanta."""
    assert math.log2(quantum) == round(math.log2(quantum)), "quantum must be a power of two"
    for i, t in enumerate(stored):
        m, whole = _quantum(t, quantum)
        assert whole, "%s: stored tensor %d is not a multiple of %g" % (what, i, quantum)
        if quantum == 1.0:
            assert float(m.abs().max()) <= 256, "%s: stored tensor %d reaches %g (> 256)" % (what, i, float(m.abs().max()))
        assert torch.equal(t.double().to(torch.bfloat16).double(), t.double()), "%s: stored tensor %d is not bf16" % (what, i)
    for i, t in enumerate(terms):
        q2 = quantum * quantum if term_quantum is None else term_quantum
        m, whole = _quantum(t, q2)
        assert whole, "%s: summand %d is not a multiple of %g" % (what, i, q2)
        worst = float(m.abs().sum((1, 2)).max()) * images_per_row
        assert worst <= FP32_HALF_RANGE, "%s: sum %d reaches %.3g quanta per part row (> 2^23); lower the density" % (
            what, i, worst)
    if wgrad_abs is not None:
        q2 = quantum * quantum if term_quantum is None else term_quantum
        assert float(wgrad_abs) / q2 <= FP32_HALF_RANGE, "%s: weight-gradient sums reach %.3g" % (
            what, float(wgrad_abs))


def wgrad_abs_bound(g, xin):
    """sum over all pixels of |g[., co]| times max |x|: an upper bound of sum |g * x| of any dW element."""
    return g.double().abs().sum((0, 1, 2)).max() * xin.double().abs().max()


# ------------------------------------------------------------------------------------------------------------ comparators
def _clusters(idx, B, H, W):
    """Where the differing pixels lie: shares at the image border, at a 16-pixel MFMA tile edge, in the first / last row of
    an image (the boundary between consecutive images)."""
    b, h, w = idx[:, 0], idx[:, 1], idx[:, 2]
    n = float(idx.shape[0])
    lin = h * W + w
    border = ((h == 0) | (h == H - 1) | (w == 0) | (w == W - 1)).sum().item() / n
    tile = ((lin % 16 == 0) | (lin % 16 == 15)).sum().item() / n
    seam = ((h == 0) | (h == H - 1)).sum().item() / n
    imgs = sorted(set(b.tolist()))
    return "border %.0f%%, tile edge %.0f%%, image boundary rows %.0f%%, images %s%s" % (
        100 * border, 100 * tile, 100 * seam, imgs[:8], "..." if len(imgs) > 8 else "")


def assert_equal_nhwc(got, ref, what=""):
    """torch.equal on [B, H, W, C] values (compared as float64: -0.0 == 0.0); on failure says how many elements differ, the
    first differing (image, row, column, channel) and where the differences cluster."""
    assert got.shape == ref.shape, "%s: shape %s vs %s" % (what, tuple(got.shape), tuple(ref.shape))
    g, r = got.double(), ref.double().to(got.device)
    if torch.equal(g, r):
        return
    bad = (g != r) | torch.isnan(g)
    idx = bad.nonzero()
    B, H, W, C = got.shape
    f = tuple(idx[0].tolist())
    raise AssertionError("%s: %d of %d elements differ; first at (image %d, row %d, column %d, channel %d): got %r, want %r; %s"
                         % (what, idx.shape[0], bad.numel(), f[0], f[1], f[2], f[3], float(g[f]), float(r[f]),
                            _clusters(idx.cpu(), B, H, W)))


def assert_equal_tensor(got, ref, what="", names=None):
    """torch.equal on a tensor of any shape (weight gradients: [O][tap][I]); reports the count and the first index."""
    g, r = got.double(), ref.double().to(got.device)
    assert g.shape == r.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(r.shape))
    if torch.equal(g, r):
        return
    bad = (g != r) | torch.isnan(g)
    idx = bad.nonzero()
    f = tuple(idx[0].tolist())
    per = ""
    if names:
        per = "; " + ", ".join("%s %s" % (n, sorted(set(idx[:, k].tolist()))[:8]) for k, n in enumerate(names))
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r%s" % (
        what, idx.shape[0], bad.numel(), f, float(g[f]), float(r[f]), per))


def assert_sums_equal(part, ref, what=""):
    """part [nparts][k][C] fp32 rows of a kernel, ref [k][C] float64: the rows are added in float64 over ALL rows (exact: every
    row is an integer number of quanta) and must equal the reference sums."""
    got = part.double().sum(0)
    ref = ref.double().to(got.device)
    assert got.shape == ref.shape, "%s: part rows hold %s, reference %s" % (what, tuple(got.shape), tuple(ref.shape))
    if torch.equal(got, ref):
        return
    idx = (got != ref).nonzero()
    k, c = idx[0].tolist()
    raise AssertionError("%s: %d of %d per-channel sums differ; first: sum %d, channel %d: got %r, want %r (difference %r); "
                         "channels %s" % (what, idx.shape[0], got.numel(), k, c, float(got[k, c]), float(ref[k, c]),
                                          float(got[k, c] - ref[k, c]), sorted(set(idx[:, 1].tolist()))[:16]))
