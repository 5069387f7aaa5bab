"""The ArcFace / CosFace head and the cosine backward all heads share, at the C ABI on exact operands (tests/exact_operands.py, last
section).

The fourth sibling of test_gpu_exact_conv.py, test_gpu_exact_elementwise.py and test_gpu_exact_output.py.  The weight rows and
the embeddings have norms that are powers of two (times sqrt(nnz), nnz a power of 4), so the normalised operands are +-1 /
sqrt(nnz), the cosines the GEMM forms from them are multiples of 1 / nnz without a rounding in any order, and CosFace's whole chain
-- logits, gcos, both gradient GEMMs, both normalisation backwards -- consists of fp32 numbers (exact_operands.head_case asserts it
on the reference).  The cosines are produced by the GEMM itself, the labels are placed on the columns where a vector, a tile or
the row ends, and the target cosines include -1, +1, 0 and the neighbours of ArcFace's threshold.

Pinned, every element against float64 formed on the host from the same operands:
  fr_row_normalize (xn, inv, the zero rows N..Np, the transposed copy by both of its kernels), fr_col_normalize (the same bits from
  the transposed weight), FR_EPI_MARGIN of fr_conv_igemm (FR_F32, out_f32, ldc = ld and ld + 8: the logits, cos_t, rows with label
  -1), fr_margin_bwd (FR_F32; from the GEMM's cos_t and on hand-written cosines next to every branch), and the launches of
  frhip/functional.py::_cosine_backward: fr_fill_rows + the head-shaped fr_conv_wgrad (1x1, Cout = pad4(N), ldg = Np > Cout),
  FR_EPI_SLAB at the product's split-K rule + fr_reduce_parts, fr_normalize_bwd for both operands, fr_col_normalize_bwd; and
  FRF.margin_forward / margin_backward once, which must carry the bits of the C-ABI launches.
Every comparison is an equality, except the two ArcFace expressions the compiler may contract -- phi = c cos_m - sine sin_m and
d phi / d c = cos_m + sin_m c / sine -- which get the derived bound of exact_operands.margin_logits_ref / dphi_ref (four roundings of
one ulp of the larger term, doubled; carried through * s [* g], plus one ulp of the result).  Where those expressions are not
evaluated (CosFace, c <= th, the easy margin at c <= 0, d phi at the clamp) equality is demanded of ArcFace too.

Every buffer a kernel writes is a sentinel-filled Buf between guard bands, every operand sits between NaN bands, every test
launches twice into the same buffers and requires the same bits.

Not pinned: the bf16 instantiations of the margin epilogue and of fr_margin_bwd -- the product launches neither (the head always
computes in FR_F32, frhip/functional.py) --, the row kernels of the nine later heads (their own test files), and timing.
test_gpu_kernels.py::test_margin_head_* and the sharded-head tests keep the random-data and golden-vector checks that exact data
cannot give (rounding behaviour, the reference's own vectors).
"""
import functools

import numpy as np
import pytest
import torch

import exact_operands as X
from test_gpu_exact_conv import SENTINEL, Buf, _same_bits
from test_gpu_exact_elementwise import dev, guarded, launch_twice
from test_gpu_exact_output import _seq
from test_gpu_kernels import K  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

F32 = torch.float32
head_case = functools.lru_cache(maxsize=None)(X.head_case)
SHAPE_IDS = ["%d_%d_%d" % s for s in X.HEAD_SHAPES]
COL_IDS = ["%d_%d_%d" % s for s in X.HEAD_COL_SHAPES]
CONFIGS = sorted(X.HEAD_CONFIGS)


def _f32(t):
    """An exact float64 reference as the fp32 tensor a kernel reads (head_case asserts that nothing is lost)."""
    return t.to(F32)


def _positive_zero(t):
    return bool((t.contiguous().view(torch.int32) == 0).all())


def _gemm_kw(B, N, D, lda=None):
    return dict(B=B, RH=1, RW=1, SH=1, SW=1, SC=D, N=N, KH=1, KW=1, stride=1, pad=0, mode=0, lda=lda or D, pro=0, out_f32=1)


# ------------------------------------------------------------------------------------------------ normalisation (steps 1, 2)
@pytest.mark.parametrize("B,N,D", X.HEAD_COL_SHAPES, ids=COL_IDS)
def test_normalized_operands(K, B, N, D):
    """fr_row_normalize on x (no transposed copy) and on w (rows_pad = ldt = Np: the per-row transposed copy below Np = 256, the
    tiled one from there on): xn, inv_x, wn, wt and inv_w equal float64; the rows N..Np of wn and the columns N..Np of wt are +0;
    wt is wn^T.  fr_col_normalize on w^T, the [D][N] kernel of the column-normalised heads, leaves the same bits in kn, kt, inv."""
    c = head_case(B, N, D)
    Np, st = c["Np"], K.current_stream_ptr()
    what = "normalize %s" % ((B, N, D),)
    xn, inv_x = Buf(B, D, dtype=F32), Buf(1, B, dtype=F32)
    wn, wt, inv_w = Buf(Np, D, dtype=F32), Buf(D, Np, dtype=F32), Buf(1, N, dtype=F32)
    kn, kt, inv_k = Buf(Np, D, dtype=F32), Buf(D, Np, dtype=F32), Buf(1, N, dtype=F32)
    run = _seq(K.call("fr_row_normalize", guarded(c["x"]), xn.t, None, inv_x.t, B, B, D, 0, K.FR_F32, st),
               K.call("fr_row_normalize", guarded(c["w"]), wn.t, wt.t, inv_w.t, N, Np, D, Np, K.FR_F32, st),
               K.call("fr_col_normalize", guarded(c["w"].t().contiguous()), kn.t, kt.t, inv_k.t, D, N, Np, st))

    def check():
        X.assert_equal_tensor(xn.t, c["xn"], what + " xn", ("row", "d"))
        X.assert_equal_tensor(inv_x.t.view(-1), c["inv_x"], what + " inv_x", ("row",))
        X.assert_equal_tensor(wn.t, c["wn"], what + " wn", ("class", "d"))
        X.assert_equal_tensor(wt.t, c["wt"], what + " wt", ("d", "class"))
        X.assert_equal_tensor(inv_w.t.view(-1), c["inv_w"], what + " inv_w", ("class",))
        assert _positive_zero(wn.t[N:]) and _positive_zero(wt.t[:, N:]), what + ": the padding of wn / wt is not +0"
        assert torch.equal(wt.t, wn.t.t()), what + ": wt is not wn^T"
        for name, a, b in (("kn", kn, wn), ("kt", kt, wt), ("inv", inv_k, inv_w)):
            assert _same_bits(a.flat, b.flat), "%s: fr_col_normalize's %s does not carry fr_row_normalize's bits" % (what, name)

    launch_twice(what, run, dict(xn=xn, inv_x=inv_x, wn=wn, wt=wt, inv_w=inv_w, kn=kn, kt=kt, inv_k=inv_k), check)


# ------------------------------------------------------------------------------------------------ margin epilogue, margin backward
def _margin_launches(K, c, k, logits, cos_t, gcos, label, xn, wn, g):
    """The two launches of a training step's head, as frhip/functional.py makes them: the cosine GEMM with FR_EPI_MARGIN, and
    fr_margin_bwd from the cos_t it left."""
    B, N, D, st = c["B"], c["N"], c["D"], K.current_stream_ptr()
    fwd = K.conv(st, K.FR_F32, src=xn, w=wn, out=logits.t, ldc=logits.ld, epi=K.EPI_MARGIN, margin_kind=k["kind"],
                 easy_margin=k["easy"], cos_m=k["cos_m"], sin_m=k["sin_m"], th=k["th"], mm=k["mm"], scale=k["s"], label=label,
                 cos_t=cos_t.t, **_gemm_kw(B, N, D))
    bwd = K.call("fr_margin_bwd", g, label, cos_t.t, gcos.t, B, N, c["Np"], k["kind"], k["easy"], k["cos_m"], k["sin_m"], k["th"],
                 k["s"], K.FR_F32, st)
    return fwd, bwd


@pytest.mark.parametrize("name", CONFIGS)
@pytest.mark.parametrize("B,N,D", X.HEAD_SHAPES, ids=SHAPE_IDS)
def test_margin_epilogue_and_backward(K, B, N, D, name):
    """Steps 3 and 4.  FR_EPI_MARGIN on the GEMM's own cosines, at ldc = ld and ld + 8: s * c off the label column and in rows
    with label -1, the margin on the label column and nowhere else, cos_t the label cosine, the sentinel kept where the label is
    -1 (exact_operands.check_margin_forward).  fr_margin_bwd from that cos_t: s * g off the label column, in label -1 rows and
    for CosFace everywhere, (s g) dphi on ArcFace's label column with dphi = cos_m exactly at c = +-1, +0 in the columns N..Np
    (check_margin_backward)."""
    c, k = head_case(B, N, D), X.margin_constants(name)
    label = dev(c["labels"])
    xn, wn, g = guarded(_f32(c["xn"])), guarded(_f32(c["wn"])), guarded(c["g"])
    for ldc in (c["ld"], c["ld"] + 8):
        what = "%s %s ldc %d" % (name, (B, N, D), ldc)
        logits, cos_t, gcos = Buf(B, N, ldc, dtype=F32), Buf(1, B, dtype=F32), Buf(B, c["Np"], dtype=F32)
        fwd, bwd = _margin_launches(K, c, k, logits, cos_t, gcos, label, xn, wn, g)

        def check():
            X.check_margin_forward(logits.t, cos_t.t, c, k, SENTINEL, what)
            X.check_margin_backward(gcos.t, c["g"], c["labels"], cos_t.t.view(-1).double().cpu(), k, what)

        launch_twice(what, _seq(fwd, bwd), dict(logits=logits, cos_t=cos_t, gcos=gcos), check)


def _neighbours(v):
    v = np.float32(v)
    return [float(np.nextafter(v, np.float32(-np.inf))), float(v), float(np.nextafter(v, np.float32(np.inf)))]


@pytest.mark.parametrize("name", ["arcface", "arcface_easy"])
def test_margin_backward_on_hand_written_cosines(K, name):
    """Step 5: fr_margin_bwd alone, cos_t written by hand: the fp32 neighbours of the branch threshold on both sides (th; 0 under
    the easy margin) and the threshold itself, 1 - 2^-24 (t = 2^-23: inside the clamp, the steepest slope fp32 reaches), 1 + 2^-23
    (t < 0: clamped, dphi = cos_m), +-1, and two ordinary values.  scale = 1 and g = 1 on the label column make gcos there dphi
    itself: the branch (dphi == 1) and the mask (dphi == cos_m) are read exactly, the slope within its bound; one row more has no
    label."""
    k = dict(X.margin_constants(name), s=1.0)
    edge = 0.0 if k["easy"] else k["th"]
    values = _neighbours(edge) + [1.0 - 2.0 ** -24, 1.0 + 2.0 ** -23, 1.0, -1.0, 0.5, -0.5 if k["easy"] else -0.9375, 0.25]
    B, N, Np = len(values), 7, 32
    labels = torch.tensor([(3 * b) % N for b in range(B - 1)] + [-1])
    cos_t = torch.tensor(values, dtype=F32)
    assert torch.equal(cos_t.double(), torch.tensor(values, dtype=torch.float64))
    g = X.small_ints(293, "hand.g", (B, N))
    g[torch.arange(B - 1), labels[:-1]] = 1.0
    want = [X.dphi_ref(v, k) for v in values[:-1]]
    # the decisions this list is there for, on the reference: off the phi branch below and on the threshold, on it above; the
    # mask open at 1 - 2^-24, shut at and beyond +1; -1 lies below either threshold
    assert want[0] == want[1] == (1.0, 0.0) and want[2][0] != 1.0
    assert want[3][1] > 0 and want[3][0] > 1000 and want[4] == want[5] == (k["cos_m"], 0.0) and want[6] == (1.0, 0.0)
    what = "margin_bwd %s on hand-written cosines" % name
    gcos = Buf(B, Np, dtype=F32)
    run = K.call("fr_margin_bwd", guarded(g), dev(labels), guarded(cos_t), gcos.t, B, N, Np, k["kind"], k["easy"], k["cos_m"],
                 k["sin_m"], k["th"], 1.0, K.FR_F32, K.current_stream_ptr())

    def check():
        X.check_margin_backward(gcos.t, g, labels, cos_t.double(), k, what)
        got = gcos.t.cpu()[torch.arange(B - 1), labels[:-1]].double()
        for b, (d, bound) in enumerate(want):
            if bound == 0.0:
                assert float(got[b]) == d, "%s: row %d, cos_t %r: dphi %r, want exactly %r" % (what, b, values[b], float(got[b]), d)

    launch_twice(what, run, dict(gcos=gcos), check)


# ------------------------------------------------------------------------------------------------ the shared backward (step 6)
def _splitk(Np):
    """frhip/functional.py::_cosine_backward."""
    nk = Np // 32
    return max(1, min(nk, 64, nk // 8))


def _backward_launches(K, c, gcos, xn, x, w, wn, wt, inv_x, inv_w, GW, gw, slab, G, gx, gK, st):
    """The launches of frhip/functional.py::_cosine_backward, both halves on one stream, plus the column-normalised heads'
    fr_col_normalize_bwd from the same GW."""
    B, N, D, Np, N4 = c["B"], c["N"], c["D"], c["Np"], c["N4"]
    splitk = _splitk(Np)
    launches = [K.call("fr_fill_rows", GW.t, None, N4, D, st),
                K.wgrad(st, K.FR_F32, g=gcos, src=xn, dw=GW.t, B=B, GH=1, GW=1, Cout=N4, SH=1, SW=1, SC=D, KH=1, KW=1, stride=1, pad=0,
                        ldg=Np, lda=D, pro=0, nsplit=1),
                K.call("fr_normalize_bwd", GW.t, w, inv_w, gw.t, N, D, st),
                K.conv(st, K.FR_F32, src=gcos, w=wt, out=slab.t, ldc=D, epi=K.EPI_SLAB, splitk=splitk, **_gemm_kw(B, D, Np)),
                K.call("fr_reduce_parts", slab.t, splitk, 1, B * D, G.t, None, None, st),
                K.call("fr_normalize_bwd", G.t, x, inv_x, gx.t, B, D, st)]
    if gK is not None:
        launches.append(K.call("fr_col_normalize_bwd", GW.t, wn, inv_w, gK.t, D, N, st))
    return launches


@pytest.mark.parametrize("B,N,D", X.HEAD_SHAPES, ids=SHAPE_IDS)
def test_shared_cosine_backward(K, B, N, D):
    """From CosFace's exact gcos [B][Np] (columns N..Np zero): GW = gcos^T xn by fr_fill_rows + the head-shaped fr_conv_wgrad (its
    rows N..N4 zero), gw by fr_normalize_bwd; G = gcos wn through FR_EPI_SLAB at the product's split-K (1, 1, 1, 2, 4 over the
    shapes) + fr_reduce_parts, gx by fr_normalize_bwd; gK = gw^T by fr_col_normalize_bwd.  Every element equals float64, and the
    float64 sum of the slabs is G too."""
    c = head_case(B, N, D)
    Np, N4, st = c["Np"], c["N4"], K.current_stream_ptr()
    splitk = _splitk(Np)
    what = "cosine backward %s splitk %d" % ((B, N, D), splitk)
    GW, gw, gK = Buf(N4, D, dtype=F32), Buf(N, D, dtype=F32), Buf(D, N, dtype=F32)
    slab, G, gx = Buf(splitk * B, D, dtype=F32), Buf(B, D, dtype=F32), Buf(B, D, dtype=F32)
    launches = _backward_launches(K, c, guarded(_f32(c["gcos"])), guarded(_f32(c["xn"])), guarded(c["x"]), guarded(c["w"]),
                                  guarded(_f32(c["wn"])), guarded(_f32(c["wt"])), guarded(_f32(c["inv_x"])),
                                  guarded(_f32(c["inv_w"])), GW, gw, slab, G, gx, gK, st)

    def check():
        X.assert_equal_tensor(GW.t, c["GW"], what + " GW", ("class", "d"))
        X.assert_equal_tensor(gw.t, c["gw"], what + " gw", ("class", "d"))
        X.assert_equal_tensor(slab.t.view(splitk, B, D).double().sum(0), c["G"], what + " float64 sum of the slabs", ("row", "d"))
        X.assert_equal_tensor(G.t, c["G"], what + " G", ("row", "d"))
        X.assert_equal_tensor(gx.t, c["gx"], what + " gx", ("row", "d"))
        X.assert_equal_tensor(gK.t, c["gw"].t(), what + " gK", ("d", "class"))

    launch_twice(what, _seq(*launches), dict(GW=GW, gw=gw, slab=slab, G=G, gx=gx, gK=gK), check)


def test_column_normalize_backward_ragged_in_both_directions(K):
    """fr_col_normalize_bwd at D = 96 and N = 203: a ragged 64-tile in D and in N; gK = gw^T element for element."""
    B, N, D = X.HEAD_COL_SHAPES[-1]
    c = head_case(B, N, D)
    what = "col_normalize_bwd %s" % ((B, N, D),)
    gK = Buf(D, N, dtype=F32)
    run = K.call("fr_col_normalize_bwd", guarded(_f32(c["GW"])), guarded(_f32(c["wn"])), guarded(_f32(c["inv_w"])), gK.t, D, N,
                 K.current_stream_ptr())
    launch_twice(what, run, dict(gK=gK), lambda: X.assert_equal_tensor(gK.t, c["gw"].t(), what, ("d", "class")))


# ------------------------------------------------------------------------------------------------ the Python layer (step 7)
@pytest.mark.parametrize("name", CONFIGS)
def test_functional_layer_carries_the_same_bits(K, name):
    """FRF.margin_forward / margin_backward at (37, 203, 64) against the C-ABI launches of this file on the same operands: the
    logits, cos_t (0, the layer's own fill, where the label is -1), gx and gw carry the same bits -- the constants, the Np / ld
    choice and the side stream of the Python layer.  For CosFace those bits are the float64 reference's."""
    from frhip import functional as FRF
    B, N, D = 37, 203, 64
    c, k = head_case(B, N, D), X.margin_constants(name)
    kind, s, m, easy = X.HEAD_CONFIGS[name]
    x, w, label, g = dev(c["x"]), dev(c["w"]), dev(c["labels"]), dev(c["g"])
    logits, saved, cfg = FRF.margin_forward(x, w, label, kind, s, m, bool(easy))
    gx, gw = FRF.margin_backward(saved, cfg, g, True, True)
    torch.cuda.synchronize()
    assert (cfg.Np, cfg.ld) == (c["Np"], c["ld"]) and tuple(logits.shape) == (B, N) and logits.stride(0) == c["ld"]
    # the same step at the C ABI
    st = K.current_stream_ptr()
    lo, cos_t, gcos = Buf(B, N, c["ld"], dtype=F32), Buf(1, B, dtype=F32), Buf(B, c["Np"], dtype=F32)
    xn, wn = guarded(_f32(c["xn"])), guarded(_f32(c["wn"]))
    fwd, bwd = _margin_launches(K, c, k, lo, cos_t, gcos, label, xn, wn, g)
    GW, gw2 = Buf(c["N4"], D, dtype=F32), Buf(N, D, dtype=F32)
    slab, G, gx2 = Buf(_splitk(c["Np"]) * B, D, dtype=F32), Buf(B, D, dtype=F32), Buf(B, D, dtype=F32)
    _seq(fwd, bwd, *_backward_launches(K, c, gcos.t, xn, x, w, wn, guarded(_f32(c["wt"])), guarded(_f32(c["inv_x"])),
                                       guarded(_f32(c["inv_w"])), GW, gw2, slab, G, gx2, None, st))()
    torch.cuda.synchronize()
    what = "functional %s" % name
    has = (c["labels"] >= 0).cuda()
    for tag, got, ref in (("logits", logits, lo.t), ("gx", gx, gx2.t), ("gw", gw, gw2.t),
                          ("cos_t", saved.cos_t[has], cos_t.t.view(-1)[has])):
        assert torch.equal(got.contiguous().view(torch.int32), ref.contiguous().view(torch.int32)), "%s: %s differs in bits" % (what, tag)
    assert _positive_zero(saved.cos_t[~has]), what + ": cos_t of a row without a label"
    X.check_margin_forward(logits, torch.where(has, saved.cos_t, torch.full_like(saved.cos_t, SENTINEL)), c, k, SENTINEL, what)
    if kind == 1:
        X.assert_equal_tensor(gx, c["gx"], what + " gx", ("row", "d"))
        X.assert_equal_tensor(gw, c["gw"], what + " gw", ("class", "d"))
