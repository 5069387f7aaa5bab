"""Bit-exact checks of the output layer's GEMMs on integer operands (tests/exact_operands.py, last section).

The third sibling of test_gpu_exact_conv.py and test_gpu_exact_elementwise.py, for BatchNorm2d -> Dropout -> Flatten ->
Linear(25088, 512) (backbone/model_irse.py:143-148) at the C ABI: fr_linear_fwd / fr_linear_dgrad on the fp32 master weight
(csrc/linear_gemm.hip), the dense weight gradient (fr_conv_wgrad with taps = 1), the split-K slab epilogue of fr_conv_igemm
(FR_EPI_SLAB: the Linear forward of the fp32 path) and the Flatten-order buffer fr_bn_dropout_cm hands to all of them.  They are
GEMMs and one-fmaf passes: on small integer operands every product, every fp32 partial sum in any order, every slab and every
bf16 store is exact, so every element must EQUAL a float64 reference.  There is no tolerance in this file.  The BatchNorm1d
behind the Linear is covered by the [B][512] geometries of exact_operands.EW_SHAPES in test_gpu_exact_elementwise.py.

Two kinds of operands.  Sums: ternary activations against a weight of small integers, or (frac) of values on and next to the
ties of the fp32 -> bf16 rounding the kernels do in registers -- a dropped K step, a bias in a second slice, a truncating cast all
move a sum by at least one quantum.  One-hot rows: a single 1 per row selects ONE weight, so the output must be exactly
bf16(W[o][k]) for weights of any finite value (N(0, 0.02^2) plus the frac list) -- addressing and rounding in one test.

Every buffer a kernel writes is a sentinel-filled Buf between guard bands (a store past row B of the last slab, past the last
column block, in front of the buffer shows in a guard; an unwritten element keeps its sentinel); every operand is sized exactly
between NaN bands (a read past its end poisons the result); every test launches twice into the same buffers and requires the same
bits.  The geometry lists (exact_operands.LINEAR_FWD and the others) name the edge each entry is there for.
"""
import functools

import pytest
import torch

import exact_operands as X
from test_gpu_dropout import host_keep_mask
from test_gpu_exact_conv import SENTINEL, Buf, _same_bits
from test_gpu_exact_elementwise import dev, guarded, launch_twice
from test_gpu_kernels import K  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
DTYPE = {"bf16": BF, "f32": F32}
DROPOUT_SEED = 0x5EED0FFACE5

linear_case = functools.lru_cache(maxsize=None)(X.linear_case)


def _real(shape):
    return tuple(shape[:3]) == X.LINEAR_REAL


def _seq(*launches):
    def run():
        for l in launches:
            l()
    return run


# ------------------------------------------------------------------------------------------------ fr_linear_fwd
# the small geometries with integer and with frac weights; the real K once per entry: frac at 16 slices, integers at the
# library's own slice count
FWD = [s + (frac,) for s in X.LINEAR_FWD for frac in ((False, True) if not _real(s) else (s[3] == 16,))]


@pytest.mark.parametrize("B,O,Kd,slices,frac", FWD, ids=["%d_%d_%d_s%s_frac%d" % s for s in FWD])
def test_linear_forward_slabs(K, B, O, Kd, slices, frac):
    """fr_linear_fwd: every slab equals a[:, ks:ke] @ bf16(W)[:, ks:ke]^T of its own K range element for element, the bias is in
    slab 0 only (and nowhere with bias = NULL), the guards around [slices][B][O] are intact, and fr_reduce_parts over the slabs
    gives the whole sum."""
    slices = slices or int(K.lib.fr_linear_slices(O, Kd))
    assert slices >= 1 and (Kd // 32) % slices == 0
    c = linear_case(B, O, Kd, frac=frac)
    st = K.current_stream_ptr()
    a, W, bias = guarded(c["a"], BF), guarded(c["W"]), guarded(c["bias"])
    for with_bias in (True, False):
        what = "linear_fwd %s slices %d frac%d bias%d" % ((B, O, Kd), slices, frac, with_bias)
        ref = X.linear_forward(c, slices, bias=with_bias)
        assert float(ref.abs().max()) < SENTINEL
        slab, out = Buf(slices * B, O, dtype=F32), Buf(B, O, dtype=F32)
        run = _seq(K.call("fr_linear_fwd", a, W, bias if with_bias else None, slab.t, B, O, Kd, slices, st),
                   K.call("fr_reduce_parts", slab.t, slices, 1, B * O, out.t, None, None, st))

        def check():
            X.assert_equal_tensor(slab.t.view(slices, B, O), ref, what + " slabs", ("slice", "row", "feature"))
            X.assert_equal_tensor(out.t, ref.sum(0), what + " sum of the slabs", ("row", "feature"))

        launch_twice(what, run, {"slab": slab, "out": out}, check)


@pytest.mark.parametrize("B,O,Kd,slices", X.LINEAR_FWD_ONE_HOT, ids=["%d_%d_%d_s%d" % s for s in X.LINEAR_FWD_ONE_HOT])
def test_linear_forward_reads_each_weight_where_it_lies(K, B, O, Kd, slices):
    """One-hot rows: slab[s][b][o] is exactly bf16(W[o][pick(b)]) in the slice that owns column pick(b) -- plus the bias, one
    fp32 add, where that is slice 0 -- and exactly the bias (slice 0) or zero in every other slice.  The rows reach every position
    of a K step, both register slots and the first and last step of a slice (test_exact_operands_host.py); the weights are
    Gaussian at the real scale with the ties of the bf16 rounding planted among them: addressing and round-to-nearest-even of the
    in-register cast."""
    pick = X.stride_pick(Kd)
    picks = [pick(b) for b in range(B)]
    Wh, bh = X.normal_weight(O, Kd), X.small_ints(271, "oh.bias", (O,))
    st = K.current_stream_ptr()
    a, W, bias = guarded(X.one_hot_rows(B, Kd, pick), BF), guarded(Wh), guarded(bh)
    for with_bias in (True, False):
        what = "linear_fwd one-hot %s slices %d bias%d" % ((B, O, Kd), slices, with_bias)
        ref = X.one_hot_forward(Wh, bh if with_bias else None, picks, slices)
        slab = Buf(slices * B, O, dtype=F32)
        launch_twice(what, K.call("fr_linear_fwd", a, W, bias if with_bias else None, slab.t, B, O, Kd, slices, st), {"slab": slab},
                     lambda: X.assert_equal_tensor(slab.t.view(slices, B, O), ref, what, ("slice", "row", "feature")))


# ------------------------------------------------------------------------------------------------ fr_linear_dgrad
@pytest.mark.parametrize("B,O,Kd", X.LINEAR_DGRAD, ids=["%d_%d_%d" % s for s in X.LINEAR_DGRAD])
def test_linear_data_gradient(K, B, O, Kd):
    """fr_linear_dgrad: the bf16 ga equals g @ bf16(W) (integers of at most 256: linear_dgrad asserts it) element for element."""
    c = linear_case(B, O, Kd)
    ref = X.linear_dgrad(c)
    what = "linear_dgrad %s" % ((B, O, Kd),)
    ga = Buf(B, Kd)
    launch_twice(what, K.call("fr_linear_dgrad", guarded(c["g"], BF), guarded(c["W"]), ga.t, B, O, Kd, K.current_stream_ptr()),
                 {"ga": ga}, lambda: X.assert_equal_tensor(ga.t, ref, what, ("row", "column")))


@pytest.mark.parametrize("B,O,Kd", X.LINEAR_DGRAD_ONE_HOT, ids=["%d_%d_%d" % s for s in X.LINEAR_DGRAD_ONE_HOT])
def test_linear_data_gradient_reads_each_weight_where_it_lies(K, B, O, Kd):
    """One-hot g: ga[b][:] is exactly bf16(W[pick(b)][:]) -- the row of W that the LDS staging, the transposing read and the
    permuted g fragment must agree on, for every position of a reduction step, all four ring slots, the first and the last step."""
    pick = X.stride_pick(O)
    Wh = X.normal_weight(O, Kd)
    ref = X.round_bf16(Wh)[[pick(b) for b in range(B)]]
    what = "linear_dgrad one-hot %s" % ((B, O, Kd),)
    ga = Buf(B, Kd)
    launch_twice(what, K.call("fr_linear_dgrad", guarded(X.one_hot_rows(B, O, pick), BF), guarded(Wh), ga.t, B, O, Kd,
                              K.current_stream_ptr()),
                 {"ga": ga}, lambda: X.assert_equal_tensor(ga.t, ref, what, ("row", "column")))


# ------------------------------------------------------------------------------------------------ the dense fr_conv_wgrad
def _dense_wgrad_kw(g, a, B, Cout, SC):
    return dict(g=g, src=a, B=B, GH=1, GW=1, Cout=Cout, SH=1, SW=1, SC=SC, KH=1, KW=1, stride=1, pad=0, ldg=Cout, lda=SC, pro=0)


@pytest.mark.parametrize("B,Cout,SC,dname", X.LINEAR_WGRAD, ids=["%d_%d_%d_%s" % s for s in X.LINEAR_WGRAD])
def test_linear_weight_gradient(K, B, Cout, SC, dname):
    """fr_conv_wgrad with taps = 1, GH = GW = 1: dW = g^T a, the batch being the reduction (32 rows per step, the rest masked).
    nsplit = 1 adds onto dw (the header says +=): onto zeros the result is g^T a, onto small integers it is those plus g^T a.
    With a slab and nsplit = 3 the slices (empty ones included) are stored and added in a fixed order: dw, which starts as
    sentinels, is overwritten with the same bits."""
    dtype = DTYPE[dname]
    c = linear_case(B, Cout, SC)
    ref = X.linear_wgrad(c)
    pre = X.small_ints(277, "wg.pre", (Cout, SC))
    st, fr = K.current_stream_ptr(), K.fr_dtype(torch.empty(0, dtype=dtype))
    kw = _dense_wgrad_kw(guarded(c["g"], dtype), guarded(c["a"], dtype), B, Cout, SC)
    dw = Buf(Cout, SC, dtype=F32)
    for name, start, want in (("zeros", torch.zeros(Cout, SC), ref), ("integers", pre, pre.double() + ref)):
        what = "dense wgrad %s %s onto %s" % ((B, Cout, SC), dname, name)
        start_d = dev(start)
        launch = K.wgrad(st, fr, dw=dw.t, nsplit=1, **kw)

        def run():
            dw.t.copy_(start_d)
            launch()

        launch_twice(what, run, {"dw": dw}, lambda: X.assert_equal_tensor(dw.t, want, what, ("cout", "k")))
        if name == "zeros":
            onto_zeros = dw.bits()
    what = "dense wgrad %s %s slabs" % ((B, Cout, SC), dname)
    dw2, slab = Buf(Cout, SC, dtype=F32), Buf(3, Cout * SC, dtype=F32)

    def check():
        X.assert_equal_tensor(dw2.t, ref, what, ("cout", "k"))
        X.assert_equal_tensor(slab.t.double().sum(0).view(Cout, SC), ref, what + " sum of the slabs", ("cout", "k"))
        assert _same_bits(onto_zeros, dw2.flat), what + ": not the bits of the single slice"

    launch_twice(what, K.wgrad(st, fr, dw=dw2.t, slab=slab.t, nsplit=3, **kw), {"dw": dw2, "slab": slab}, check)


# ------------------------------------------------------------------------------------------------ FR_EPI_SLAB of fr_conv_igemm
SLAB = [s + (frac,) for s in X.SLAB_GEMM for frac in ((False, True) if not _real(s) else (True,))]


@pytest.mark.parametrize("M,N,SC,splitk,dname,frac", SLAB, ids=["%d_%d_%d_k%d_%s_frac%d" % s for s in SLAB])
def test_split_k_slab_gemm(K, M, N, SC, splitk, dname, frac):
    """fr_conv_igemm as a dense GEMM with FR_EPI_SLAB (the Linear forward of the fp32 path): slab z equals the partial sum over
    the K steps [nk*z/splitk, nk*(z+1)/splitk) -- the cut include/frhip.h states, uneven at nk = 7, splitk = 3 -- slab 0 alone
    carries the bias, the float64 sum of the slabs and fr_reduce_parts(out, splitk, 1, rows*ldc) both give the whole product, and
    the padding columns N .. ldc of every slab row keep their sentinels.  The weight is the bf16-rounded one in both dtypes (w is
    in the compute dtype)."""
    dtype = DTYPE[dname]
    c = linear_case(M, N, SC, frac=frac)
    ldc = (N + 15) // 16 * 16
    cuts = X.splitk_cut(SC // 32, splitk)
    ref = X.linear_forward(c, cuts=cuts)
    assert len(cuts) == splitk and float(ref.abs().max()) < SENTINEL
    assert not torch.equal(ref[0], X.linear_forward(c, cuts=cuts, bias=False)[0]), "the bias changes nothing: test data"
    what = "slab gemm %s splitk %d %s frac%d" % ((M, N, SC), splitk, dname, frac)
    st, fr = K.current_stream_ptr(), K.fr_dtype(torch.empty(0, dtype=dtype))
    slab, out = Buf(splitk * M, N, ldc, dtype=F32), Buf(M, ldc, dtype=F32)
    conv = K.conv(st, fr, src=guarded(c["a"], dtype), w=guarded(c["Wq"], dtype), bias=guarded(c["bias"]), out=slab.t, B=M, RH=1,
                  RW=1, SH=1, SW=1, SC=SC, N=N, KH=1, KW=1, stride=1, pad=0, mode=0, lda=SC, ldc=ldc, pro=0, epi=K.EPI_SLAB,
                  out_f32=1, splitk=splitk)
    run = _seq(conv, K.call("fr_reduce_parts", slab.t, splitk, 1, M * ldc, out.t, None, None, st))

    def check():
        X.assert_equal_tensor(slab.t.reshape(splitk, M, N), ref, what + " slabs", ("slice", "row", "column"))
        X.assert_equal_tensor(slab.t.reshape(splitk, M, N).double().sum(0), ref.sum(0), what + " float64 sum of the slabs")
        X.assert_equal_tensor(out.t[:, :N], ref.sum(0), what + " fr_reduce_parts", ("row", "column"))

    launch_twice(what, run, {"slab": slab, "out": out}, check)


# ------------------------------------------------------------------------------------------------ the Flatten-order hand-over
@pytest.mark.parametrize("p", [0.5, 0.0])
def test_flatten_order_hand_over(K, p):
    """fr_bn_dropout_cm writes a[b][c*HW + hw]; that buffer, unchanged, is the operand of fr_linear_fwd and of the weight
    gradient, both against the master weight in torch's own [O][C*HW] layout; back, fr_linear_dgrad feeds fr_dropout_bwd_cm, which
    returns to NHWC.  Producer and consumers must agree with the reference module's Flatten of the NCHW tensor: a, f = a @ W^T, dW
    and the NHWC gradient equal exact_operands.flatten_case -- float64 torch with the host restatement of the dropout mask
    (test_gpu_dropout.host_keep_mask), autograd for both gradients."""
    B, C, HW, O = X.FLATTEN_CASE
    Kd = C * HW
    keep = torch.from_numpy(host_keep_mask(DROPOUT_SEED, B, C, HW, p))
    o, a_ref, f_ref, gy_ref, dw_ref = X.flatten_case(B, C, HW, O, keep, p)
    st, fr = K.current_stream_ptr(), K.fr_dtype(torch.empty(0, dtype=BF))
    slices = int(K.lib.fr_linear_slices(O, Kd))
    assert slices >= 1
    what = "flatten hand-over %s p=%g" % (X.FLATTEN_CASE, p)
    x, g, W = guarded(o["x"].reshape(B * HW, C), BF), guarded(o["g"], BF), guarded(o["W"])
    scale, shift = dev(o["scale"]), dev(o["shift"])
    a, ga, gy = Buf(B, Kd), Buf(B, Kd), Buf(B * HW, C)
    slab, f, dw = Buf(slices * B, O, dtype=F32), Buf(B, O, dtype=F32), Buf(O, Kd, dtype=F32)
    wgrad = K.wgrad(st, fr, dw=dw.t, nsplit=1, **_dense_wgrad_kw(g, a.t, B, O, Kd))
    run = _seq(K.call("fr_bn_dropout_cm", x, a.t, scale, shift, B, C, HW, float(p), DROPOUT_SEED, fr, st),
               K.call("fr_linear_fwd", a.t, W, None, slab.t, B, O, Kd, slices, st),
               K.call("fr_reduce_parts", slab.t, slices, 1, B * O, f.t, None, None, st),
               lambda: dw.t.zero_(), wgrad,
               K.call("fr_linear_dgrad", g, W, ga.t, B, O, Kd, st),
               K.call("fr_dropout_bwd_cm", ga.t, gy.t, B, C, HW, float(p), DROPOUT_SEED, fr, st))

    def check():
        X.assert_equal_tensor(a.t, a_ref, what + " a", ("row", "c*HW + hw"))
        X.assert_equal_tensor(f.t, f_ref, what + " f", ("row", "feature"))
        X.assert_equal_tensor(dw.t, dw_ref, what + " dW", ("feature", "c*HW + hw"))
        X.assert_equal_tensor(gy.t.view(B, HW, C), gy_ref, what + " NHWC gradient", ("image", "pixel", "channel"))

    launch_twice(what, run, {"a": a, "ga": ga, "gy": gy, "slab": slab, "f": f, "dw": dw}, check)
