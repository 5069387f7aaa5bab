"""Integer-valued operands for the bf16 convolution kernels and the channel-wise passes, float64 references and bit-exact
comparators.

Why: on Gaussian data a bf16 kernel can only be compared to a tolerance (tests/test_gpu_kernels.py), and an addressing
or coverage defect smaller than one rounding passes.  Here every operand is a small integer (or a small integer times a
power of two) and every true result fits the format it is stored in: bf16 MFMA products with fp32 accumulation, the
one-fmaf prologues, the fp32 epilogue sums, the slab sums and the bf16 store are then exact in ANY summation order, and a
kernel must equal an integer reference bit for bit -- at every pixel, part row and weight-gradient element.

The channel-wise passes of frhip/csrc/elementwise.hip (BatchNorm apply / backward, channel and image statistics, the
squeeze-excite squeezes and backward) are chains of fmaf and sums of the same kind: on small dyadic operands every
intermediate is an fp32 number and every sum is exact in any order, so they are pinned the same way (second half of the
references below; the recipes assert their own preconditions before anything is compared).

The GEMMs of the output layer (Linear forward in K slices, data and weight gradient on the fp32 master weight, the split-K
slab epilogue) and the Flatten-order hand-over in front of them are the third group (last section; test_gpu_exact_output.py).

The ArcFace / CosFace head and the cosine backward every head shares are the fourth group (the section behind that;
test_gpu_exact_head.py): operands whose norms are powers of two, so that the normalised rows, the cosines the GEMM forms from
them and the whole CosFace chain are dyadic fractions, exact in fp32 in any order.

A plain helper module (like shard_ref.py), used by test_exact_operands_host.py (no GPU), test_gpu_exact_conv.py,
test_gpu_exact_elementwise.py, test_gpu_exact_output.py and test_gpu_exact_head.py.
Layout: activations NHWC ``[B, H, W, C]``, weights packed ``[O][kh*kw][I]`` -- what the C ABI takes.
"""
import math

import numpy as np
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


def assert_exact_range(stored=(), terms=(), images_per_row=1, quantum=1.0, term_quantum=None, wgrad_abs=None, fp32=(), what=""):
    """The preconditions of exactness, asserted on the REFERENCE before anything is compared.
      stored   : tensors the kernel stores as bf16 -- multiples of `quantum` (a power of two), every element with at most 8
                 significant bits (for plain integers: |v| <= 256), i.e. unchanged by a round trip through bf16
      terms    : per sum kind the elementwise summands [B, H, W, C] -- multiples of `term_quantum` (default quantum^2) whose
                 per-image, per-channel sum of magnitudes, times the images one part row can hold, is <= 2^23 quanta (half
                 the fp32 integer range)
      wgrad_abs: an upper bound of sum |g * x| over every weight-gradient element, <= 2^23 quanta.
      fp32     : (value, magnitude, q) triples of results a kernel leaves as fp32 behind a sum it may take in any order (the
                 squeeze-excite backward): `value` is a multiple of the power of two q and an fp32 number, `magnitude` -- the
                 sum of the magnitudes of its summands, same shape -- is <= 2^23 q, so every partial sum is an fp32 number."""
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
    for i, (value, magnitude, q) in enumerate(fp32):
        assert math.log2(q) == round(math.log2(q)), "quantum must be a power of two"
        _, whole = _quantum(value, q)
        assert whole, "%s: fp32 result %d is not a multiple of %g" % (what, i, q)
        assert torch.equal(value.double().float().double(), value.double()), "%s: fp32 result %d is not an fp32 number" % (what, i)
        worst = float(magnitude.double().abs().max()) / q
        assert worst <= FP32_HALF_RANGE, "%s: the sum behind fp32 result %d reaches %.3g quanta (> 2^23)" % (what, i, worst)


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


# ------------------------------------------------------------------------------------------------------------ channel-wise passes
# References of the passes of frhip/csrc/elementwise.hip, written from the formulas of include/frhip.h in float64, and the
# operand recipes of test_gpu_exact_elementwise.py.  Part rows of these kernels are not tied to images (a workgroup strides
# over all rows), so every range condition takes the sum over ALL rows (all_rows).
SCALES = [1.0, 2.0, -1.0, 0.5]       # BatchNorm scale / rscale
SHIFTS = [-1.0, 0.0, 1.0]
GATES = [0.5, 1.0, 2.0]              # squeeze-excite gates of the BatchNorm passes
SLOPES = [0.25, 0.5]
INV_COUNT = 2.0 ** -10               # fr_bn_bwd_apply takes 1 / count as an argument: a power of two, whatever the row count

# (B, H, W, C, nblocks): the smallest shapes that reach each edge of the [row-thread][channel-chunk] kernels (256 threads; the
# lean bf16 kernels: 4 channels per thread, 4 forward / 3 backward rows in flight)
EW_SHAPES = [(3, 5, 7, 64, 7),       # 105 rows: below one block trip, idle blocks, non-square
             (5, 7, 7, 128, 2),      # 49-row images straddle the rows in flight; several grid-stride trips, ragged last trip
             (2, 14, 14, 256, 3),    # 392 rows
             (37, 2, 6, 512, 5),     # many 12-row images
             (1, 2, 2, 64, 1),       # fewer rows than row-threads
             (2, 4, 4, 1024, 4),     # one row-thread per trip
             (2, 3, 3, 2048, 2),     # bf16 only, not lean-eligible: the general kernel
             # BatchNorm1d of the output layer: [B][512] rows with H = W = 1, nblocks = ops.grid_blocks(B, 512, FR_F32)
             (2, 1, 1, 512, 1),      # the smallest training batch: one block, two of its rows live
             (5, 1, 1, 512, 3),      # two rows per fp32 block: a ragged last block
             (256, 1, 1, 512, 128)]  # the benchmark's batch
SCATTER_SHAPES = [(3, 6, 10, 64), (2, 4, 2, 128), (5, 14, 14, 256)]   # add_kind 2, stride 2 (lean bf16 / general fp32)
SCATTER_S3 = (2, 9, 6, 64)                                            # add_kind 2, stride 3: the general kernel
STATS_LONG = (2, 56, 56, 64, 5)                                       # HW = 3136: many trips per thread
SE_HW = [16, 49, 64, 196]
SE_SQUEEZE = [(3, 4, 64), (5, 7, 128), (2, 8, 256), (3, 14, 256), (2, 4, 2048), (3, 7, 512)]   # (B, H, C) of the squeezes
SE_CHAIN = [(5, 4, 128), (3, 8, 256), (130, 4, 64)]   # (B, H, C), power-of-two HW: the full squeeze-excite backward
SE_REAL_HW = [(5, 7, 128), (3, 14, 256)]              # HW 49 and 196: the per-image sums only (w1 = 0)


def small_ints(seed, tag, shape, p=0.5):
    """Integers -3 .. 3: a ternary tensor plus twice a sparser one."""
    return ternary(seed, tag + ".1", shape, p) + 2.0 * ternary(seed, tag + ".2", shape, p / 2)


def nonzero_ints(seed, tag, shape):
    """Integers from {-2, -1, 1, 2}: never zero, so a missed or an extra hit of a scattered tensor shows."""
    return pick(seed, tag, int(math.prod(shape)), [-2.0, -1.0, 1.0, 2.0]).view(shape)


def per_image(seed, tag, B, C, values, weights=None):
    return pick(seed, tag, B * C, values, weights).view(B, C)


def all_rows(t):
    """[B, H, W, C] -> [1, 1, B*H*W, C]: the view assert_exact_range sums over when part rows are not tied to images."""
    return t.reshape(1, 1, -1, t.shape[-1])


def _img(v, like):
    """[B][C] per-image values against [B, H, W, C]."""
    return v.to(like.device, torch.float64).view(v.shape[0], 1, 1, v.shape[1])


def bn_apply(x, scale, shift, se=None, slope=None, res=None, rscale=None, rshift=None, res_stride=1):
    """out = [prelu](x*scale + shift [* se[b][c]]) [+ res*rscale + rshift]; res_stride > 1: the identity shortcut reads
    res[b, h*stride, w*stride] of a [B, H*stride, W*stride, C] tensor.  Returns (out, [out, out^2])."""
    v = x.double() * _ch(scale, x) + _ch(shift, x)
    if se is not None:
        v = v * _img(se, x)
    if slope is not None:
        v = torch.where(v > 0, v, v * _ch(slope, x))
    if res is not None:
        r = res.double()[:, ::res_stride, ::res_stride]
        if rscale is not None:
            r = r * _ch(rscale, x) + _ch(rshift, x)
        v = v + r
    return v, [v, v * v]


def bn_bwd_gprime(g, x, scale=None, shift=None, slope=None, se=None, gse=None):
    """(g', g*u*[u <= 0]): g' = g | g * prelu'(u), u = x*scale + shift | g * se[b][c] + gse[b][c]."""
    gp = g.double()
    st = torch.zeros_like(gp)
    if slope is not None:
        u = x.double() * _ch(scale, x) + _ch(shift, x)
        st = torch.where(u > 0, st, gp * u)
        gp = torch.where(u > 0, gp, gp * _ch(slope, x))
    if se is not None:
        gp = gp * _img(se, x)
        if gse is not None:
            gp = gp + _img(gse, x)
    return gp, st


def xhat(x, mean, invstd):
    return (x.double() - _ch(mean, x)) * _ch(invstd, x)


def scatter(add, H, W, stride):
    """MaxPool2d(1, stride) backwards: add[b, h/stride, w/stride] lands on the pixels with h % stride == w % stride == 0."""
    B, _, _, C = add.shape
    full = torch.zeros(B, H, W, C, dtype=torch.float64, device=add.device)
    full[:, ::stride, ::stride] = add.double()
    return full


def bn_bwd_apply(gp, xh, gamma, invstd, s0, s1, inv_count, add=None):
    """gx = gamma*invstd*(g' - s0*inv_count - xhat*s1*inv_count) [+ add], add of gx's geometry."""
    gx = _ch(gamma, gp) * _ch(invstd, gp) * (gp - _ch(s0, gp) * inv_count - xh * (_ch(s1, gp) * inv_count))
    return gx if add is None else gx + add.double()


def _bn_images(seed, tag, B, hwc, p):
    return batch(ternary(seed, tag, (BASE_IMAGES,) + tuple(hwc), p), B)


def bn_apply_case(B, H, W, C, res_kind=0, gate=False, slope=False, res_stride=1, seed=211):
    """Operands and reference of fr_bn_apply: x and res small integers (behind a slope: -4, 0, 1, as activations(.., "prelu")),
    scale / rscale from {1, 2, -1, 1/2}, shifts from {-1, 0, 1}, gates from {1/2, 1, 2}, slopes from {1/4, 1/2}.  Everything is a
    multiple of 1/16.  Returns (operands, out, [out, out^2])."""
    hwc = (H, W, C)
    x = batch(activations(seed, "a.xp", hwc, 0.6, "prelu") if slope else small_ints(seed, "a.x", (BASE_IMAGES,) + hwc), B)
    o = dict(x=x, scale=pick(seed, "a.scale", C, SCALES), shift=pick(seed, "a.shift", C, SHIFTS))
    if gate:
        o["se"] = per_image(seed, "a.se", B, C, GATES)
    if slope:
        o["slope"] = pick(seed, "a.slope", C, SLOPES)
    if res_kind:
        o["res"] = batch(small_ints(seed, "a.res", (BASE_IMAGES, H * res_stride, W * res_stride, C)), B)
    if res_kind == 2:
        o.update(rscale=pick(seed, "a.rscale", C, SCALES), rshift=pick(seed, "a.rshift", C, SHIFTS))
    out, terms = bn_apply(res_stride=res_stride, **o)
    what = "bn_apply %s res%d gate%d slope%d" % ((B, H, W, C), res_kind, gate, slope)
    assert_exact_range(stored=[out], terms=[all_rows(t) for t in terms], quantum=1.0 / 16, what=what)
    assert float((out != 0).double().mean()) > 0.4, what + ": mostly zeros"
    return o, out, terms


def bn_bwd_case(B, H, W, C, mode="plain", seed=223):
    """Operands and reference sums of fr_bn_bwd_reduce.  mode: plain | slope | gate | gate_gse.  g and x ternary, mean from
    {-1, 0, 1}, invstd from {1/2, 1, 2}, gse from the multiples of 1/4 up to 1/2.  Returns (operands, g', xhat, the three
    elementwise summands)."""
    hwc = (H, W, C)
    o = dict(g=_bn_images(seed, "b.g", B, hwc, 0.5), x=_bn_images(seed, "b.x", B, hwc, 0.6),
             mean=pick(seed, "b.mean", C, SHIFTS), invstd=pick(seed, "b.invstd", C, [0.5, 1.0, 2.0]))
    if mode == "slope":
        o.update(scale=pick(seed, "b.scale", C, SCALES), shift=pick(seed, "b.shift", C, SHIFTS), slope=pick(seed, "b.slope", C, SLOPES))
    if mode in ("gate", "gate_gse"):
        o["se"] = per_image(seed, "b.se", B, C, GATES)
    if mode == "gate_gse":
        o["gse"] = per_image(seed, "b.gse", B, C, [-0.5, -0.25, 0.0, 0.25, 0.5])
    gp, st = bn_bwd_gprime(o["g"], o["x"], o.get("scale"), o.get("shift"), o.get("slope"), o.get("se"), o.get("gse"))
    xh = xhat(o["x"], o["mean"], o["invstd"])
    terms = [gp, gp * xh, st]
    assert_exact_range(terms=[all_rows(t) for t in terms], term_quantum=1.0 / 8, what="bn_bwd %s %s" % ((B, H, W, C), mode))
    return o, gp, xh, terms


def bn_bwd_apply_case(B, H, W, C, mode="plain", add_kind=0, add_stride=2, nxt=False, seed=223):
    """Operands and reference of fr_bn_bwd_apply on the data of bn_bwd_case: gamma from {1, 2, -1}, inv_count = 2^-10, s0 and s1
    multiples of 2^9 (both quotients multiples of 1/2 up to 1), add from {-2, -1, 1, 2} on EVERY pixel.  gx is a multiple of 1/8
    below 32 in magnitude: at most 8 significant bits.  nxt: nx ternary, nmean / ninvstd as mean / invstd.
    Returns (operands, gx, [gx, gx * xhat_n] or [])."""
    o, gp, xh, _ = bn_bwd_case(B, H, W, C, mode, seed)
    halves = [-1.0, -0.5, 0.0, 0.5, 1.0]
    o.update(gamma=pick(seed, "c.gamma", C, [1.0, 2.0, -1.0]), s0=pick(seed, "c.s0", C, halves) / INV_COUNT,
             s1=pick(seed, "c.s1", C, halves) / INV_COUNT, inv_count=INV_COUNT)
    add = None
    if add_kind == 1:
        o["add"] = add = batch(nonzero_ints(seed, "c.add", (BASE_IMAGES, H, W, C)), B)
    elif add_kind == 2:
        assert H % add_stride == 0 and W % add_stride == 0
        o["add"] = batch(nonzero_ints(seed, "c.add", (BASE_IMAGES, H // add_stride, W // add_stride, C)), B)
        add = scatter(o["add"], H, W, add_stride)
    gx = bn_bwd_apply(gp, xh, o["gamma"], o["invstd"], o["s0"], o["s1"], INV_COUNT, add)
    what = "bn_bwd_apply %s %s add%d" % ((B, H, W, C), mode, add_kind)
    terms = []
    if nxt:
        o.update(nx=_bn_images(seed, "c.nx", B, (H, W, C), 0.6), nmean=pick(seed, "c.nmean", C, SHIFTS),
                 ninvstd=pick(seed, "c.ninvstd", C, [0.5, 1.0, 2.0]))
        terms = [gx, gx * xhat(o["nx"], o["nmean"], o["ninvstd"])]
    assert_exact_range(stored=[gx], terms=[all_rows(t) for t in terms], quantum=1.0 / 8, term_quantum=1.0 / 16, what=what)
    assert float((gx != 0).double().mean()) > 0.4, what + ": mostly zeros"
    return o, gx, terms


def image_sums(terms):
    """[B][k][C] float64 per-image sums."""
    return torch.stack([t.sum((1, 2)) for t in terms], 1)


def stats_case(B, H, W, C, seed=229):
    """fr_channel_stats / fr_image_moments: x small integers; the summands (x, x^2)."""
    x = batch(small_ints(seed, "s.x", (BASE_IMAGES, H, W, C)), B)
    terms = [x.double(), x.double() * x.double()]
    assert_exact_range(stored=[x], terms=[all_rows(t) for t in terms], what="stats %s" % ((B, H, W, C),))
    return x, terms


def se_squeeze_case(B, H, C, seed=233):
    """fr_se_gscale (gs[b][c] = sum_hw g*(x*scale + shift), any HW) and fr_se_pool (pooled[b][c] = scale*mean_hw(x) + shift: the
    kernel DIVIDES the sum by HW, so it is exact at power-of-two HW only -- H = 4, 8; elsewhere `pooled` is None)."""
    hwc = (H, H, C)
    g, x = _bn_images(seed, "q.g", B, hwc, 0.5), batch(small_ints(seed, "q.x", (BASE_IMAGES,) + hwc), B)
    scale, shift = pick(seed, "q.scale", C, SCALES), pick(seed, "q.shift", C, SHIFTS)
    t = g.double() * (x.double() * _ch(scale, x) + _ch(shift, x))
    gs = t.sum((1, 2))
    what = "se squeeze %s" % ((B, H, C),)
    assert_exact_range(stored=[g, x], fp32=[(gs, t.abs().sum((1, 2)), 0.5)], what=what)
    pooled = None
    HW = H * H
    if HW & (HW - 1) == 0:
        sx = x.double().sum((1, 2))
        pooled = sx / HW * scale.double() + shift.double()
        assert_exact_range(fp32=[(sx, x.double().abs().sum((1, 2)), 1.0), (pooled, pooled, 0.5 / HW)], what=what + " pool")
    return dict(g=g, x=x, scale=scale, shift=shift), gs, pooled


def se_mlp_bwd(gs, s, hidden, w1, w2, HW):
    """Backward of s = sigmoid(W2 relu(W1 pooled)) from gs = dL/ds: gz = gs*s*(1-s) at the fc2 output, gh = relu'(hidden) *
    (W2^T gz) at the fc1 output, gpooled = (W1^T gh) / HW.  w1 [R][C], w2 [C][R]."""
    gz = gs.double() * s.double() * (1.0 - s.double())
    gh = torch.where(hidden.double() > 0, gz @ w2.double(), torch.zeros((), dtype=torch.float64))
    return gz, gh, (gh @ w1.double()) / HW


def se_mlp_wgrad(gz, gh, hidden, pooled):
    """dW1[r][c] = sum_b gh[b][r] * pooled[b][c], dW2[c][r] = sum_b gz[b][c] * hidden[b][r]."""
    return gh.double().t() @ pooled.double(), gz.double().t() @ hidden.double()


def se_bwd_case(B, H, C, zero_w1=False, seed=239):
    """The squeeze-excite backward (fr_se_gscale_mlp_bwd[_sums], fr_se_mlp_wgrad): g and x ternary (g sparse), gates s from
    {1/4, 1/2, 3/4} (s*(1-s) is 3/16 or 1/4), w1 / w2 ternary, hidden from {0, 1/2, 1, 2} with half of it exactly 0 (the ReLU mask
    matters), pooled a small multiple of 1/4.  gpooled multiplies by 1 / HW: the full chain is exact at power-of-two HW only;
    zero_w1 (gse = 0) serves the per-image sums at the real HW values 49 and 196.
    Returns (operands, reference dict): gs, gz, gh, gpooled, dw1, dw2, parts [B][4][C] (per image: gs, sum g, sum g*xhat, sum
    xhat) and bn [B][2][C] (sum g', sum g'*xhat with g' = g*s + gpooled)."""
    HW, R = H * H, max(C // 16, 1)
    assert zero_w1 or HW & (HW - 1) == 0, "gpooled is exact at power-of-two HW only"
    hwc = (H, H, C)
    o = dict(g=_bn_images(seed, "e.g", B, hwc, 0.25), x=_bn_images(seed, "e.x", B, hwc, 0.5),
             scale=pick(seed, "e.scale", C, SCALES), shift=pick(seed, "e.shift", C, [0.0, -1.0, 1.0], [0.875, 0.0625, 0.0625]),
             mean=pick(seed, "e.mean", C, SHIFTS), invstd=pick(seed, "e.invstd", C, [0.5, 1.0, 2.0]),
             s=per_image(seed, "e.s", B, C, [0.25, 0.5, 0.75]),
             hidden=per_image(seed, "e.hidden", B, R, [0.0, 0.5, 1.0, 2.0], [0.5, 0.2, 0.2, 0.1]),
             pooled=per_image(seed, "e.pooled", B, C, [-0.5, -0.25, 0.0, 0.25, 0.5, 1.0]),
             w1=torch.zeros(R, C) if zero_w1 else ternary(seed, "e.w1", (R, C), 0.5), w2=ternary(seed, "e.w2", (C, R), 0.25))
    g, x = o["g"].double(), o["x"].double()
    t = g * (x * o["scale"].double() + o["shift"].double())
    gs = t.sum((1, 2))
    gz, gh, gpooled = se_mlp_bwd(gs, o["s"], o["hidden"], o["w1"], o["w2"], HW)
    dw1, dw2 = se_mlp_wgrad(gz, gh, o["hidden"], o["pooled"])
    xh = xhat(o["x"], o["mean"], o["invstd"])
    parts = image_sums([t, g, g * xh, xh])
    gp = g * _img(o["s"], g) + _img(gpooled, g)
    bn = image_sums([gp, gp * xh])
    what = "se backward %s" % ((B, H, C),)
    q = 1.0 / 32                                     # gs is a multiple of 1/2, s*(1-s) of 1/16
    qp = q / (1 << (HW - 1).bit_length())            # gpooled (exact: zero, or HW a power of two)
    sd, G, GX, XH = o["s"].double(), parts[:, 1], parts[:, 2], parts[:, 3]
    assert_exact_range(stored=[o["g"], o["x"]], what=what, fp32=[
        (gs, t.abs().sum((1, 2)), 0.5), (G, g.abs().sum((1, 2)), 1.0), (GX, (g * xh).abs().sum((1, 2)), 0.5),
        (XH, xh.abs().sum((1, 2)), 0.5), (gz, gz, q), (gh, gz.abs() @ o["w2"].double().abs(), q),
        (gpooled * HW, gh.abs() @ o["w1"].double().abs(), q), (gpooled, gpooled, qp),
        (dw1, gh.abs().t() @ o["pooled"].double().abs(), q / 4), (dw2, gz.abs().t() @ o["hidden"].double().abs(), q / 2),
        # the rows of BN2's sums as the kernel forms them: s*G + HW*gse and s*GX + gse*XH, one fused multiply-add each
        (gpooled * XH, gpooled * XH, qp / 2), (bn[:, 0], (sd * G).abs() + (HW * gpooled).abs(), q),
        (bn[:, 1], (sd * GX).abs() + (gpooled * XH).abs(), qp / 2)])
    assert float((gh != 0).double().mean()) > 0.2 and float((o["hidden"] == 0).double().mean()) > 0.3, what + ": the ReLU mask"
    return o, dict(gs=gs, gz=gz, gh=gh, gpooled=gpooled, dw1=dw1, dw2=dw2, parts=parts, bn=bn)


# ------------------------------------------------------------------------------------------------------------ output-layer GEMMs
# Linear(25088, 512) of the output layer (include/frhip.h: fr_linear_fwd / fr_linear_dgrad on the fp32 master weight, the dense
# fr_conv_wgrad with taps = 1, FR_EPI_SLAB of fr_conv_igemm) and the Flatten-order hand-over from fr_bn_dropout_cm: operand recipes
# and float64 references of test_gpu_exact_output.py.  a [B][K] and g [B][O] are ternary, W [O][K] is the fp32 master: half of it
# zero, the rest small integers -- or, with frac, values around 1 that sit on and next to the ties of the fp32 -> bf16 rounding the
# kernels do in registers.  The references round W with torch (W.to(torch.bfloat16): round to nearest even IS the specification).
_T = 2.0 ** -8                       # half a bf16 step in [1, 2): 1 + _T is a tie
FRAC_POS = [1.0 + _T,                # tie, down to the even neighbour 1
            1.0 + 3 * _T,            # tie, up to the even neighbour 1 + 2^-6
            1.0 + _T + 2.0 ** -16,   # just above a tie: 1 + 2^-7
            1.0 + _T - 2.0 ** -16,   # just below it: 1
            1.0 - _T / 2 - 2.0 ** -17,   # just below the tie under 1 (steps of 2^-8 there): 1 - 2^-8
            1.0 - _T / 2]            # that tie: up to the even neighbour 1
FRAC_ROUNDED = [1.0, 1.0 + 2.0 ** -6, 1.0 + 2.0 ** -7, 1.0, 1.0 - _T, 1.0]   # what bf16 makes of FRAC_POS: multiples of 2^-8
FRAC_WEIGHTS = FRAC_POS + [-v for v in FRAC_POS]
INT_WEIGHTS = [-2.0, -1.0, 1.0, 2.0]

# (B, O, K, slices) of fr_linear_fwd: a workgroup owns 64 features x 256 rows x one K slice, a wave 64 rows, a K step is 32 wide,
# a loop trip takes two steps (two register slots) and an odd step count ends in a tail; ksteps = K / 32 / slices
LINEAR_REAL = (5, 512, 25088)        # the output layer's K and O; the batch is small: the reference is formed on the CPU
LINEAR_FWD = [(1, 64, 32, 1),        # one step (the tail alone), one row: 255 clamped rows
              (65, 64, 192, 2),      # ksteps = 3: one trip + the odd tail; one row into the second wave
              (257, 128, 320, 2),    # ksteps = 5; a second 256-row block with one live row; two feature tiles
              (256, 64, 128, 4),     # ksteps = 1 in four slices; exactly one full row block
              (63, 512, 256, 1),     # ksteps = 8: trips only; all eight feature tiles; one row short of a wave
              LINEAR_REAL + (16,),   # the real K at a slice count the library does not recommend: ksteps = 49, odd
              LINEAR_REAL + (None,)]  # ... and at fr_linear_slices(512, 25088) (None: asked of the library; 28 -> ksteps = 28)
LINEAR_FWD_ONE_HOT = [(64, 128, 256, 1), (64, 128, 256, 4), (257, 64, 192, 2)]
# (B, O, K) of fr_linear_dgrad: a workgroup owns 128 columns of K x 128 rows, a wave 32 rows; the reduction runs over O in steps of
# 32, four steps (ring slots) per trip
LINEAR_DGRAD = [(1, 128, 128),       # one trip, one row
                (33, 128, 384),      # one row into the second wave; three column blocks
                (129, 256, 128),     # a second 128-row block with one live row; two trips
                (128, 512, 256),     # exactly one full row block; four trips
                LINEAR_REAL]         # the real shape: 196 column blocks
LINEAR_DGRAD_ONE_HOT = [(129, 128, 256), (33, 512, 128)]
# (B, Cout, SC, dtype) of the dense fr_conv_wgrad (taps = 1, GH = GW = 1): the batch is the reduction, 32 rows per step, rows past
# it are masked; tiles Cout x SC: 128 x 128, 128 x 64 (SC < 128), 64 x 64 (Cout < 128), 64 x 32 (SC < 64)
LINEAR_WGRAD = [s + (d,) for s in [(1, 64, 32),       # one row, 31 masked; the 64 x 32 tile
                                   (31, 128, 64),     # one row short of a step; 128 x 64
                                   (33, 64, 64),      # one row into a second step; 64 x 64
                                   (256, 128, 128),   # eight full steps; 128 x 128
                                   (40, 200, 512)]    # the head's dW = g^T a: Cout = 200 ends 56 rows short of its second tile
                for d in ("bf16", "f32")] + [LINEAR_REAL + ("bf16",)]   # the output layer's own: 4 x 196 tiles
# (M, N, SC, splitk, dtype) of fr_conv_igemm with FR_EPI_SLAB (1x1, RH = RW = 1): 128-row tiles, 64 columns wide at N <= 64, else
# 128; ldc = N rounded up to 16
SLAB_GEMM = [s + (d,) for s in [(37, 64, 224, 3),     # nk = 7 cut 2 + 2 + 3; the 64-wide tile; a ragged row tile
                                (130, 200, 224, 3),   # the same cut; two row tiles; N = 200 in rows of ldc = 208
                                (128, 512, 96, 1),    # splitk = 1: one slab with the bias; four column tiles, a full row tile
                                (5, 200, 160, 5)]     # one step per slice
             for d in ("bf16", "f32")] + [LINEAR_REAL + (49, "f32")]   # the engine's own launch on the fp32 path: 16 steps each
FLATTEN_CASE = (3, 128, 49, 128)     # (B, C, HW, O): K = 6272


def one_hot_rows(B, n, pick):
    """[B][n] float32: row b holds a single 1 at column pick(b)."""
    t = torch.zeros(B, n)
    t[torch.arange(B), torch.tensor([pick(b) for b in range(B)])] = 1.0
    return t


def stride_pick(n, mult=37):
    """pick(b) = mult * b mod n.  mult is odd: any 32 consecutive rows hit all 32 positions of a step of 32; which steps and
    slots the rows of a geometry reach is asserted where the geometry is listed (test_exact_operands_host.py)."""
    return lambda b: (mult * b) % n


def normal_weight(O, K, seed=257):
    """Weights for the one-hot tests, where nothing is summed and any finite, normal fp32 value is exact: N(0, 0.02^2) -- the
    real weight scale -- with the frac list planted at every 7th element.  No subnormals, infinities or NaN (what the bf16 MFMA
    makes of a subnormal is the hardware's business, and 0 * inf would poison a row)."""
    W = (synth.normal(seed, "l.wn", (O, K)) * 0.02).reshape(-1)
    W[W.abs() < 2.0 ** -100] = 0.02
    n = W[::7].numel()
    W[::7] = torch.tensor(FRAC_WEIGHTS, dtype=torch.float32).repeat(-(-n // len(FRAC_WEIGHTS)))[:n]
    assert bool(torch.isfinite(W).all()) and float(W.abs().min()) >= 2.0 ** -100
    return W.view(O, K).contiguous()


def round_bf16(W):
    """float64 values of the weight as the kernels use it."""
    return W.to(torch.bfloat16).double()


def linear_case(B, O, K, seed=251, frac=False, density=0.5, wdensity=0.5):
    """Operands of Linear(K, O) at batch B: a [B][K] and g [B][O] ternary with `density` non-zeros, W [O][K] fp32 with `wdensity`
    non-zeros from {-2, -1, 1, 2} (frac: from FRAC_WEIGHTS), bias integers in [-3, 3]; Wq = bf16(W) in float64.  Asserted here:
    every forward output is a multiple of the quantum (1; frac: 2^-8) whose sum of magnitudes over ALL of K -- and with it every
    partial sum of every slice, in any order -- is at most 2^23 quanta, and every weight-gradient element is an integer of at
    most B."""
    a, g = ternary(seed, "l.a", (B, K), density), ternary(seed, "l.g", (B, O), density)
    W = pick(seed, "l.w", O * K, FRAC_WEIGHTS if frac else INT_WEIGHTS).view(O, K)
    W = (W * (synth.uniform(seed, "l.wz", (O, K), 0.0, 1.0) < wdensity)).contiguous()
    bias = small_ints(seed, "l.bias", (O,))
    c = dict(B=B, O=O, K=K, a=a, g=g, W=W, bias=bias, Wq=round_bf16(W), frac=frac, quantum=_T if frac else 1.0)
    what = "linear %s%s" % ((B, O, K), " frac" if frac else "")
    full = linear_forward(c, 1)[0]
    assert_exact_range(fp32=[(full, a.double().abs() @ c["Wq"].abs().t() + bias.double().abs(), c["quantum"])], what=what + " forward")
    dw = linear_wgrad(c)
    assert_exact_range(fp32=[(dw, g.double().abs().t() @ a.double().abs(), 1.0)], what=what + " weight gradient")
    assert float(dw.abs().max()) <= B, what + ": a weight-gradient element beyond the batch"
    assert K < 64 or float((full != 0).double().mean()) > 0.5, what + ": mostly zeros"
    return c


def k_slices(K, slices):
    """fr_linear_fwd: `slices` equal K ranges."""
    assert K % slices == 0
    return [(s * (K // slices), (s + 1) * (K // slices)) for s in range(slices)]


def splitk_cut(nk, splitk):
    """FR_EPI_SLAB (include/frhip.h): slice z sums the K steps [nk*z/splitk, nk*(z+1)/splitk) -- as channel ranges of 32 per step."""
    n = max(splitk, 1)
    return [(32 * (nk * z // n), 32 * (nk * (z + 1) // n)) for z in range(n)]


def linear_forward(c, slices=1, bias=True, cuts=None):
    """[slices][B][O] float64: slab s = a[:, ks:ke] @ Wq[:, ks:ke].T, plus the bias in slab 0 ONLY.  cuts: the K ranges (default:
    `slices` equal ones)."""
    a, Wq = c["a"].double(), c["Wq"]
    out = torch.stack([a[:, ks:ke] @ Wq[:, ks:ke].t() for ks, ke in (cuts or k_slices(c["K"], slices))], 0)
    if bias:
        out[0] += c["bias"].double()
    return out


def linear_dgrad(c):
    """ga = g @ Wq [B][K], which the kernel stores as bf16: integers of at most 256 (so not with frac weights)."""
    ga = c["g"].double() @ c["Wq"]
    what = "linear %s data gradient" % ((c["B"], c["O"], c["K"]),)
    assert_exact_range(stored=[ga], fp32=[(ga, c["g"].double().abs() @ c["Wq"].abs(), 1.0)], what=what)
    return ga


def linear_wgrad(c):
    """dW = g^T a [O][K]."""
    return c["g"].double().t() @ c["a"].double()


def one_hot_forward(W, bias, picks, slices):
    """[slices][B][O] float64 of fr_linear_fwd on one-hot rows: bf16(W[o][pick(b)]) in the slice that owns pick(b), 0 elsewhere,
    the bias on top in slice 0 -- ONE fp32 add there (exact in float64, rounded once as the kernel's add is)."""
    O, K = W.shape
    Wq = round_bf16(W)
    out = torch.zeros(slices, len(picks), O, dtype=torch.float64)
    for b, k in enumerate(picks):
        out[k // (K // slices), b] = Wq[:, k]
    if bias is not None:
        out[0] = (out[0] + bias.double()).float().double()
    return out


def flatten_case(B, C, HW, O, keep, p, seed=263):
    """The hand-over BatchNorm2d -> Dropout -> Flatten -> Linear (backbone/model_irse.py:143-147) as a float64 torch module on NCHW
    tensors: x [B, HW, C] ternary (NHWC), scale from {1, 2, -1} and shift from {-1, 0, 1}, keep [B][C*HW] the dropout mask in
    Flatten order, W / g of linear_case(B, O, C*HW).  Returns the operands, a [B][C*HW] (what fr_bn_dropout_cm must write), f = a @
    Wq^T, and autograd's gradients: gy [B, HW, C] (NHWC) for the BatchNorm output and dW.  Asserted: a holds integers -3 .. 3 times
    1 / (1 - p) (p = 1/2: {0, +-2, +-4, +-6}), and what is stored as bf16 -- a, ga and gy -- keeps to integers of at most 256."""
    K = C * HW
    c = linear_case(B, O, K, seed)
    x = ternary(seed, "f.x", (B, HW, C), 0.5)
    scale, shift = prologue_coeffs(seed, "f.bn", C, "bn")
    inv_keep = 1.0 / (1.0 - p)
    y = (x.double() * scale.double() + shift.double()).permute(0, 2, 1).contiguous().requires_grad_(True)   # NCHW with H*W = HW
    lin = torch.nn.Linear(K, O, bias=False, dtype=torch.float64)
    with torch.no_grad():
        lin.weight.copy_(c["Wq"])
    a = torch.flatten(y * keep.view(B, C, HW).double() * inv_keep, 1)
    f = lin(a)
    gy, dW = torch.autograd.grad(f, [y, lin.weight], c["g"].double())
    a, f, gy = a.detach(), f.detach(), gy.permute(0, 2, 1).contiguous()
    what = "flatten hand-over %s p=%g" % ((B, C, HW, O), p)
    allowed = torch.arange(-3, 4, dtype=torch.float64) * inv_keep
    assert bool(torch.isin(a, allowed).all()) and float(a.abs().max()) == 3 * inv_keep, what + ": a outside its value set"
    ga = c["g"].double() @ c["Wq"]
    assert_exact_range(stored=[a, ga, gy], fp32=[(f, a.abs() @ c["Wq"].abs().t(), 1.0), (dW, c["g"].double().abs().t() @ a.abs(), 1.0)],
                       what=what)
    return dict(c, x=x, scale=scale, shift=shift), a, f, gy, dW


# ------------------------------------------------------------------------------------------------------------ margin head
# ArcFace / CosFace at the C ABI (FR_EPI_MARGIN of fr_conv_igemm, fr_margin_bwd) and the cosine backward every head shares
# (frhip/functional.py::_cosine_backward: the head-shaped fr_conv_wgrad, FR_EPI_SLAB + fr_reduce_parts, fr_normalize_bwd,
# fr_col_normalize_bwd): operand recipes, float64 references and comparators of test_gpu_exact_head.py.
#
# A weight row has nnz non-zeros of +-2^j (nnz a power of 4), so its norm is sqrt(nnz) 2^j, the reciprocal norm a power of two and
# the normalised row +-1 / sqrt(nnz) on its support.  An embedding row is the sign pattern of its label's weight row with k signs
# flipped -- target cosine (nnz - 2k) / nnz -- and, for the odd numerators, one non-zero moved off the support (where D > nnz),
# times its own 2^j.  Every cosine is then a multiple of 1 / nnz that the GEMM forms without a rounding, in any order.
HEAD_SHAPES = [(1, 4, 32),           # one row, one vector, Np = 32, split-K 1
               (37, 203, 64),        # N % 4 = 3: ld = 204, ragged vector and column tile, Np = 224 < 256: per-row transposed copy
               (129, 65, 32),        # one row in the second 128-row tile, one column in the second column tile
               (5, 500, 32),         # Np = 512: split-K 2 in the data gradient, tiled transpose
               (130, 1000, 512)]     # the product's D, split-K 4
HEAD_COL_SHAPES = HEAD_SHAPES + [(37, 203, 96)]   # fr_col_normalize[_bwd]: a ragged 64-tile in D as well
HEAD_NNZ = {32: 16, 64: 64, 96: 64, 512: 256}
HEAD_CONFIGS = {"arcface": (0, 64.0, 0.5, 0), "arcface_easy": (0, 64.0, 0.5, 1), "cosface": (1, 30.0, 0.35, 0)}  # kind, s, m, easy
HEAD_TH = math.cos(math.pi - 0.5)    # ArcFace's branch threshold at m = 0.5: the target cosines lie on both sides of it
HEAD_TH_CLEARANCE = 2.0 ** -10       # see head_case
PHI_ROUNDINGS = 8 * 2.0 ** -24       # the derived bound of the two ArcFace expressions, in units of their larger term
EPS32 = float(np.float32(1e-10))     # the clamp of 1 - c^2 as the kernels hold it: [1e-10f, 1.0f - 1e-10f] = [1e-10f, 1.0f]


def _f32(v):
    return float(np.float32(v))


def _ulp32(v):
    return float(np.spacing(np.float32(abs(v))))


def pad_to(n, m):
    return (n + m - 1) // m * m


def margin_constants(name):
    """What frhip/functional.py::margin_forward hands to the kernels for a HEAD_CONFIGS entry, rounded to fp32 as the float
    arguments of the C ABI are."""
    kind, s, m, easy = HEAD_CONFIGS[name]
    if kind == 0:
        cos_m, sin_m, th, mm = math.cos(m), math.sin(m), math.cos(math.pi - m), math.sin(math.pi - m) * m
    else:
        cos_m, sin_m, th, mm = m, 0.0, 0.0, 0.0
    return dict(name=name, kind=kind, easy=easy, s=_f32(s), cos_m=_f32(cos_m), sin_m=_f32(sin_m), th=_f32(th), mm=_f32(mm))


def head_label_columns(N):
    """The columns the labels must reach, in the order in which rows are spent on them: N - 1, the first column of the last
    16-byte vector, the last and the first column of the last full 64-column tile, 63, 64, 0, and both sides of a vector boundary
    inside a tile (3 | 4)."""
    full = N // 64
    cols = [N - 1, 4 * ((N - 1) // 4)] + ([64 * full - 1, 64 * (full - 1)] if full else []) + [63, 64, 0, 3, 4]
    out = []
    for c in cols:
        if 0 <= c < N and c not in out:
            out.append(c)
    return out


def head_labels(B, N):
    """Placed, not drawn: (labels [B] int64, ordinal [B]).  Rows 1 and B - 2 carry -1 (the sharded head's "not my class") where
    B >= 4.  The other rows take head_label_columns(N) in order -- the last row first: at B = 129 it is the one row of the second
    row tile -- then (37 i + 11) mod N.  ordinal[b]: the position of row b in that order (-1: no label)."""
    none = [1, B - 2] if B >= 4 else []
    order = []
    for b in [B - 1, 0] + list(range(2, B)):
        if b not in none and b not in order:
            order.append(b)
    cols = head_label_columns(N)
    labels, ordinal = torch.full((B,), -1, dtype=torch.int64), [-1] * B
    for i, b in enumerate(order):
        labels[b] = cols[i] if i < len(cols) else (37 * i + 11) % N
        ordinal[b] = i
    return labels, ordinal


def head_targets(nnz, D):
    """(k, move) by ordinal: k sign flips and `move` (0 | 1) non-zeros off the support give the cosine (nnz - move - 2k) / nnz.
    First +1, -1, 0, the two cosines next to HEAD_TH, the two next to 0; then every other one, visited with a stride coprime to
    their number."""
    combos = [(k, 0) for k in range(nnz + 1)] + ([(k, 1) for k in range(nnz)] if D > nnz else [])
    cosv = lambda c: (nnz - c[1] - 2 * c[0]) / nnz  # noqa: E731
    first = [(0, 0), (nnz, 0), (nnz // 2, 0),
             min((c for c in combos if cosv(c) > HEAD_TH), key=cosv), max((c for c in combos if cosv(c) < HEAD_TH), key=cosv),
             min((c for c in combos if cosv(c) > 0), key=cosv), max((c for c in combos if cosv(c) < 0), key=cosv)]
    rest = [c for c in sorted(combos, key=cosv) if c not in first]
    stride = int(0.382 * len(rest)) | 1
    while math.gcd(stride, len(rest)) != 1:
        stride += 2
    return lambda i: first[i] if i < len(first) else rest[((i - len(first)) * stride) % len(rest)]


def _pow2_quantum(t):
    """The largest power of two that divides every element."""
    m = t.double().reshape(-1)
    m = m[m != 0]
    if m.numel() == 0:
        return 1.0
    for e in range(40, -80, -1):
        q = 2.0 ** e
        if bool((m / q == (m / q).round()).all()):
            return q
    raise AssertionError("no dyadic quantum above 2^-80")


def assert_f32(t, what):
    assert torch.equal(t.double().float().double(), t.double()), "%s does not survive a round trip through float32" % what


def assert_gemm_exact(a, b, what):
    """a [M][K] @ b [K][N]: the sum of the magnitudes of the terms of every element stays below 2^24 quanta of the smallest
    term (the power of two that divides every product), so fp32 sums them exactly in any order."""
    q = _pow2_quantum(a) * _pow2_quantum(b)
    worst = float((a.double().abs() @ b.double().abs()).max()) / q
    assert worst < 2.0 ** 24, "%s: the sums reach %.3g quanta (>= 2^24)" % (what, worst)
    return worst


def assert_rows_exact(a, b, what):
    """The row-wise dot products a[r] . b[r] under the same condition."""
    q = _pow2_quantum(a) * _pow2_quantum(b)
    worst = float((a.double() * b.double()).abs().sum(1).max()) / q
    assert worst < 2.0 ** 24, "%s: the sums reach %.3g quanta (>= 2^24)" % (what, worst)
    return worst


def cosine_backward(xn, inv_x, wn, inv_w, gcos):
    """The float64 restatement of frhip/functional.py::_cosine_backward from gcos [B][N] on normalised operands xn [B][D], wn
    [N][D]: G = gcos @ wn, GW = gcos^T @ xn, and the backward of the normalisation, g_in = (G - xhat (xhat . G)) * inv, for both.
    The intermediates a kernel rounds (the dot product, its product with xhat, the difference) are returned too."""
    G, GW = gcos @ wn, gcos.t() @ xn
    dx, dw = (xn * G).sum(1, keepdim=True), (wn * GW).sum(1, keepdim=True)
    gx, gw = (G - xn * dx) * inv_x[:, None], (GW - wn * dw) * inv_w[:, None]
    return dict(G=G, GW=GW, gx=gx, gw=gw, dot_x=dx, dot_w=dw, proj_x=xn * dx, proj_w=wn * dw, diff_x=G - xn * dx,
                diff_w=GW - wn * dw)


def head_case(B, N, D, seed=281):
    """Operands and float64 references of the margin head at (B, N, D); see the head of this section.  Keys: x [B][D], w [N][D],
    labels, g [B][N] (upstream gradient from {-2 .. 2}, about half zeros; never zero on a label column, where d phi must show),
    xn, inv_x, wn [Np][D] (rows N.. zero), wt = wn^T, inv_w, cos [B][N], and the CosFace chain at s = 30: gcos [B][Np], G, GW
    [N4][D], gx, gw.  Asserted here, on the reference:
      - every value of the chain (and every intermediate a kernel rounds) is an fp32 number;
      - each GEMM keeps the sum of magnitudes of its terms below 2^24 quanta of its smallest term (assert_gemm_exact);
      - no cosine is closer to ArcFace's threshold th than HEAD_TH_CLEARANCE = 2^-10.  The cosines are exact fp32 numbers and the
        kernels compare them to the fp32 th without a rounding, so ANY non-zero distance decides the branch as float64 does;
        2^-10 is 2^13 ulps of the cosines there.  (Half the spacing of the cosines, 1 / (2 nnz), cannot be kept by a set that
        has a cosine on either side of th next to it: the spacing is 1 / nnz and th = -0.87758 lies 0.0026 below -14/16 = -56/64
        and 0.0013 above -225/256.)"""
    nnz, Np, N4 = HEAD_NNZ[D], pad_to(N, 32), pad_to(N, 4)
    what = "head %s" % ((B, N, D),)
    order = torch.argsort(synth.uniform(seed, "h.w.pos", (N, D), 0.0, 1.0), dim=1)[:, :nnz]
    sign = torch.where(synth.uniform(seed, "h.w.sign", (N, D), 0.0, 1.0) < 0.5, -1.0, 1.0)
    wj = pick(seed, "h.w.j", N, [2.0 ** j for j in range(-3, 4)])
    w = torch.zeros(N, D).scatter_(1, order, torch.gather(sign, 1, order)) * wj[:, None]
    labels, ordinal = head_labels(B, N)
    target = head_targets(nnz, D)
    x = torch.zeros(B, D)
    for b in range(B):
        lab = int(labels[b])
        pattern = torch.sign(w[lab if lab >= 0 else b % N])
        sup = pattern.nonzero().flatten()
        k, move = target(ordinal[b]) if lab >= 0 else ((5 * b) % nnz, 0)
        row = pattern.clone()
        row[sup[[(b + t) % nnz for t in range(k)]]] *= -1.0
        if move:
            off = (pattern == 0).nonzero().flatten()
            row[sup[(b + nnz - 1) % nnz]] = 0.0
            row[off[b % off.numel()]] = 1.0
        x[b] = row * 2.0 ** (b % 7 - 3)
    g = pick(seed, "h.g", B * N, [-2.0, -1.0, 0.0, 1.0, 2.0], [0.125, 0.125, 0.5, 0.125, 0.125]).view(B, N)
    for b in range(B):
        if labels[b] >= 0:
            g[b, labels[b]] = (1.0 + b % 2) * (-1.0 if (b // 2) % 2 else 1.0)
    xd, wd = x.double(), w.double()
    inv_x, inv_w = 1.0 / (xd * xd).sum(1).sqrt(), 1.0 / (wd * wd).sum(1).sqrt()
    xn = xd * inv_x[:, None]
    wn = torch.zeros(Np, D, dtype=torch.float64)
    wn[:N] = wd * inv_w[:, None]
    cos = xn @ wn[:N].t()
    s = margin_constants("cosface")["s"]
    gcos = torch.zeros(B, Np, dtype=torch.float64)
    gcos[:, :N] = s * g.double()
    r = cosine_backward(xn, inv_x, wn[:N], inv_w, gcos[:, :N])
    GW = torch.zeros(N4, D, dtype=torch.float64)
    GW[:N] = r["GW"]
    c = dict(B=B, N=N, D=D, nnz=nnz, Np=Np, N4=N4, ld=N4, x=x, w=w, labels=labels, g=g, xn=xn, inv_x=inv_x, wn=wn,
             wt=wn.t().contiguous(), inv_w=inv_w, cos=cos, gcos=gcos, G=r["G"], GW=GW, gx=r["gx"], gw=r["gw"], chain=r)
    # the preconditions
    for name in ("inv_x", "inv_w"):
        lg = torch.log2(c[name] * math.sqrt(nnz))
        assert torch.equal(lg, lg.round()), "%s: %s is not a power of two over sqrt(nnz)" % (what, name)
    assert bool(((xn * math.sqrt(nnz)).abs() == (xn != 0)).all()) and bool(((wn * math.sqrt(nnz)).abs() == (wn != 0)).all()), what
    assert torch.equal(cos * nnz, (cos * nnz).round()) and float(cos.abs().max()) <= 1.0, what + ": cosines off the 1 / nnz grid"
    for name, t in [("xn", xn), ("wn", wn), ("cos", cos), ("s * cos", s * cos), ("gcos", gcos)] + sorted(r.items()):
        assert_f32(t, "%s: %s" % (what, name))
    c["quanta"] = dict(cos=assert_gemm_exact(xn, wn[:N].t(), what + " cosine GEMM"),
                       G=assert_gemm_exact(gcos[:, :N], wn[:N], what + " data-gradient GEMM"),
                       GW=assert_gemm_exact(gcos[:, :N].t(), xn, what + " weight-gradient GEMM"),
                       dot_x=assert_rows_exact(xn, r["G"], what + " xhat . G"),
                       dot_w=assert_rows_exact(wn[:N], r["GW"], what + " what . GW"))
    near = float((cos - HEAD_TH).abs().min())
    assert near >= HEAD_TH_CLEARANCE, "%s: a cosine lies %.3g from th" % (what, near)
    return c


def head_target_cosines(c):
    """[B] float64: cos[b][label[b]], NaN where the row has no label."""
    lab = c["labels"]
    t = torch.full((c["B"],), float("nan"), dtype=torch.float64)
    has = lab >= 0
    t[has] = c["cos"][has, lab[has]]
    return t


def margin_logits_ref(c, k):
    """What FR_EPI_MARGIN must store for the constants k (margin_constants): (ref [B][N] float64, bound [B][N], moved [B][N]
    bool).  bound = 0 demands equality: s * c off the label column (one exact product) and in rows without a label; on the label
    column (c - m) * s for CosFace, (c - mm) * s for ArcFace at c <= th -- two fp32 operations, evaluated in numpy float32 --
    and s * c under the easy margin at c <= 0.  On ArcFace's phi branch, phi = c cos_m - sqrt(clamp(1 - c^2)) sin_m in float64
    from the fp32 constants, within PHI_ROUNDINGS * max(|c cos_m|, |sine sin_m|), carried through * s, plus one ulp of the
    result.  moved: where ref differs from s * c -- the label columns, except where the margin is the identity."""
    s32, f = np.float32(k["s"]), np.float32
    plain = k["s"] * c["cos"]
    ref, bound = plain.clone(), torch.zeros_like(plain)
    for b in range(c["B"]):
        lab = int(c["labels"][b])
        if lab < 0:
            continue
        cc = float(c["cos"][b, lab])
        if k["kind"] == 1:
            ref[b, lab] = float((f(cc) - f(k["cos_m"])) * s32)
        elif not (cc > 0.0 if k["easy"] else cc > k["th"]):
            ref[b, lab] = k["s"] * cc if k["easy"] else float((f(cc) - f(k["mm"])) * s32)
        else:
            sine = math.sqrt(min(max(1.0 - cc * cc, EPS32), 1.0))
            ref[b, lab] = k["s"] * (cc * k["cos_m"] - sine * k["sin_m"])
            bound[b, lab] = k["s"] * PHI_ROUNDINGS * max(abs(cc * k["cos_m"]), abs(sine * k["sin_m"])) + _ulp32(ref[b, lab])
    return ref, bound, ref != plain


def dphi_ref(cc, k):
    """(d phi / d cos, bound) of fr_margin_bwd at the fp32 target cosine cc: 1 off the phi branch and for CosFace, cos_m where the
    clamp of t = 1 - c^2 does not pass (t as fp32 at or outside [1e-10f, 1.0f]) -- both exact -- else cos_m + sin_m c / sqrt(t)
    within PHI_ROUNDINGS * max(cos_m, |sin_m c / sine|)."""
    if k["kind"] == 1 or not (cc > 0.0 if k["easy"] else cc > k["th"]):
        return 1.0, 0.0
    t = 1.0 - cc * cc
    if not (_f32(t) > EPS32 and _f32(t) < 1.0):
        return k["cos_m"], 0.0
    slope = k["sin_m"] * cc / math.sqrt(t)
    return k["cos_m"] + slope, PHI_ROUNDINGS * max(k["cos_m"], abs(slope))


def margin_gcos_ref(g, labels, cos_t, k, Np):
    """What fr_margin_bwd must store: (ref [B][Np] float64, bound).  s * g off the label column and in rows without a label (one
    exact product), +0 in the columns N..Np; on the label column (s g) * dphi: one more fp32 rounding where dphi is exact
    (equality with that rounding), else within |s g| times dphi's bound plus one ulp of the result.  cos_t: the fp32 target
    cosines the kernel reads, as float64 (unread for rows without a label)."""
    B, N = g.shape
    ref = torch.zeros(B, Np, dtype=torch.float64)
    ref[:, :N] = k["s"] * g.double()
    bound = torch.zeros_like(ref)
    for b in range(B):
        lab = int(labels[b])
        if lab < 0:
            continue
        d, db = dphi_ref(float(cos_t[b]), k)
        sg = float(ref[b, lab])
        ref[b, lab] = sg * d if db else _f32(sg * d)
        if db:
            bound[b, lab] = abs(sg) * db + _ulp32(sg * d)
    return ref, bound


def assert_within(got, ref, bound, what="", names=None):
    """|got - ref| <= bound element for element, bound = 0 meaning equality (a NaN never passes); reports the count, the first
    index, both values and the bound there."""
    g, r, bd = got.double().cpu(), ref.double().cpu(), bound.double().cpu()
    assert g.shape == r.shape == bd.shape, "%s: shape %s vs %s" % (what, tuple(g.shape), tuple(r.shape))
    bad = ~((g - r).abs() <= bd)
    if not bool(bad.any()):
        return
    idx = bad.nonzero()
    f = tuple(idx[0].tolist())
    per = ""
    if names:
        per = "; " + ", ".join("%s %s" % (n, sorted(set(idx[:, i].tolist()))[:8]) for i, n in enumerate(names))
    raise AssertionError("%s: %d of %d elements differ; first at %s: got %r, want %r within %r%s" % (
        what, idx.shape[0], bad.numel(), f, float(g[f]), float(r[f]), float(bd[f]), per))


def check_margin_forward(logits, cos_t, c, k, sentinel, what=""):
    """Everything FR_EPI_MARGIN owes: the logits [B][N] (margin_logits_ref), cos_t[m] = the label cosine for labelled rows and the
    untouched `sentinel` for rows with label -1, and the set of elements that differ from s * c is exactly the set of label
    columns on which the margin is not the identity."""
    ref, bound, moved = margin_logits_ref(c, k)
    assert_within(logits, ref, bound, what + " logits", ("row", "column"))
    want_t = head_target_cosines(c)
    want_t[torch.isnan(want_t)] = sentinel
    assert_equal_tensor(cos_t.reshape(-1).cpu(), want_t, what + " cos_t", ("row",))
    plain = k["s"] * c["cos"]
    diff = logits.double().cpu() != plain
    if not torch.equal(diff, moved):
        f = tuple((diff != moved).nonzero()[0].tolist())
        raise AssertionError("%s: the elements that differ from s * cos are not the label set; first at %s (label %d): got %r, "
                             "s * cos %r" % (what, f, int(c["labels"][f[0]]), float(logits[f]), float(plain[f])))


def check_margin_backward(gcos, g, labels, cos_t, k, what=""):
    """Everything fr_margin_bwd owes (margin_gcos_ref), the padding columns N..Np as +0 bit for bit."""
    N = g.shape[1]
    ref, bound = margin_gcos_ref(g, labels, cos_t, k, gcos.shape[1])
    assert_within(gcos, ref, bound, what + " gcos", ("row", "column"))
    pad = gcos[:, N:].contiguous().cpu()
    assert bool((pad.view(torch.int32) == 0).all()), "%s: a padding column of gcos is not +0" % what
