"""Bit-exact checks of the channel-wise passes (frhip/csrc/elementwise.hip) on small dyadic operands (tests/exact_operands.py).

The sibling of test_gpu_exact_conv.py for BatchNorm apply / backward, the channel and image statistics and the squeeze-excite
squeezes and backward: fmaf chains and sums that are exact on this data in ANY summation order, so every element of every
output and the float64 sum of ALL part rows must EQUAL a float64 reference written from the formulas of include/frhip.h.
There is no tolerance in this file.  (test_gpu_kernels.py keeps the checks of the rounding behaviour, which integer data cannot
see.)

Every output, part-row block and scratch result lives in a sentinel-filled buffer between guard bands (Buf): an unwritten row
-- an idle workgroup that skipped its part row, a row in flight that was dropped -- shows as a sentinel, a store one row past the
end shows in the guard, and a second launch into the same buffers must leave the same bits.  What a kernel indexes by image or
by strided pixel (se, gse, add, res; the maps of the squeeze-excite passes) is sized exactly and sits between NaN bands: a read
from a neighbour poisons the result.

Shapes (exact_operands.EW_SHAPES) against the constants of the source -- NT = 256 threads, lean bf16 kernels LV = 4 channels per
thread, LUNR = 4 forward / LUNRB = 3 backward rows in flight: row-threads per block rtc = 256 / (C / 4), a block trip covers
rtc * LUNR rows.  Not covered: the forward squeeze-excite MLP (a sigmoid) and dropout (test_gpu_dropout.py).
"""
import functools

import pytest
import torch

import exact_operands as X
from test_gpu_exact_conv import GUARD, Buf, _same_bits
from test_gpu_kernels import K  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
EW = X.EW_SHAPES
EW_IDS = ["%d_%d_%d_%d_nb%d" % s for s in EW]
DTYPES = [("bf16", BF), ("f32", F32)]


def served(C, dtype):
    """chan_ok of the launchers: 16-byte chunks per row must tile the 256-thread block (fp32: C <= 1024, bf16: C <= 2048)."""
    return C // (4 if dtype == F32 else 8) <= 256


# (shape, dtype) pairs the launchers serve: fp32 rows of 2048 channels do not tile the block and are refused
EW_DT = [(s, n, d) for s in EW for n, d in DTYPES if served(s[3], d)]
EW_DT_IDS = ["%s_%s" % (EW_IDS[EW.index(s)], n) for s, n, d in EW_DT]


def dev(t, dtype=None):
    return None if t is None else t.to("cuda", dtype or t.dtype).contiguous()


def guarded(t, dtype=None):
    """The tensor at its exact size between two NaN bands."""
    if t is None:
        return None
    t = t.to(dtype or t.dtype)
    n = t.numel()
    flat = torch.full((2 * GUARD + n,), float("nan"), device="cuda", dtype=t.dtype)
    flat[GUARD:GUARD + n] = t.reshape(-1).cuda()
    return flat[GUARD:GUARD + n].view(t.shape)


def launch_twice(what, run, bufs, check):
    """Launch, guards, `check`; launch again into the same buffers: the same bits."""
    run()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        b.assert_guards("%s %s" % (what, name))
    check()
    bits = {name: b.bits() for name, b in bufs.items()}
    run()
    torch.cuda.synchronize()
    for name, b in bufs.items():
        assert _same_bits(bits[name], b.flat), "%s: second launch changed %s" % (what, name)


apply_case = functools.lru_cache(maxsize=None)(X.bn_apply_case)
bwd_case = functools.lru_cache(maxsize=None)(X.bn_bwd_case)
bwd_apply_case = functools.lru_cache(maxsize=None)(X.bn_bwd_apply_case)
stats_case = functools.lru_cache(maxsize=None)(X.stats_case)
se_squeeze_case = functools.lru_cache(maxsize=None)(X.se_squeeze_case)
se_bwd_case = functools.lru_cache(maxsize=None)(X.se_bwd_case)


# ------------------------------------------------------------------------------------------------ fr_bn_apply
def _apply(K, dtype, shape, res_kind=0, gate=False, slope=False, stats=True, res_stride=1):
    B, H, W, C, nb = shape
    o, ref, terms = apply_case(B, H, W, C, res_kind, gate, slope, res_stride)
    what = "bn_apply %s %s res%d/%d gate%d slope%d stats%d" % (shape, dtype, res_kind, res_stride, gate, slope, stats)
    out = Buf(B * H * W, C, dtype=dtype)
    bufs = {"out": out}
    kw = dict(x=dev(o["x"], dtype), out=out.t, scale=dev(o["scale"]), shift=dev(o["shift"]), se=guarded(o.get("se")),
              slope=dev(o.get("slope")), res=guarded(o.get("res"), dtype), rscale=dev(o.get("rscale")),
              rshift=dev(o.get("rshift")), B=B, H=H, W=W, C=C, res_kind=res_kind, res_stride=res_stride, nblocks=nb)
    if stats:
        bufs["part"] = part = Buf(nb, 2 * C, dtype=F32)
        kw["part"] = part.t

    def check():
        X.assert_equal_nhwc(out.t.reshape(B, H, W, C), ref, what + " out")
        if stats:
            X.assert_sums_equal(part.t.reshape(nb, 2, C), X.column_sums(terms), what + " part rows")

    launch_twice(what, K.bn_apply(K.current_stream_ptr(), K.fr_dtype(out.t), **kw), bufs, check)


@pytest.mark.parametrize("shape", EW, ids=EW_IDS)
def test_bn_apply_plain_gate_and_residual(K, shape):
    """fr_bn_apply in bf16 without a slope and without a strided shortcut: lean_ok(C) (C / 4 threads per row tile the block: C <=
    1024) selects bn_apply_lean_kernel<RES, STATS, SE> -- every residual kind, with and without a gate, with and without part rows;
    C = 2048 is not lean-eligible and takes bn_apply_kernel<bf16_t> (8 channels per thread, one row in flight)."""
    for res_kind in (0, 1, 2):
        for gate in (False, True):
            for stats in (True, False):
                _apply(K, BF, shape, res_kind, gate, stats=stats)


@pytest.mark.parametrize("shape,name,dtype", EW_DT, ids=EW_DT_IDS)
def test_bn_apply_general_kernel(K, shape, name, dtype):
    """The arguments that route fr_bn_apply to bn_apply_kernel<T>: fp32 always (the lean kernels are bf16), bf16 with a PReLU
    slope (`!args->slope` fails) -- every residual kind with and without a gate, part rows on half of them -- and with the strided
    identity shortcut (res_kind 1, res_stride 2: the source is [B, 2H, 2W, C], non-square on the non-square shapes; gate and
    slope each on and off): the lean kernels serve none of them.  fp32 also runs the full cross product without a slope."""
    for res_kind in (0, 1, 2):
        for gate in (False, True):
            _apply(K, dtype, shape, res_kind, gate, slope=True, stats=(res_kind + gate) % 2 == 0)
            if dtype == F32:  # without a slope, where bf16 takes the lean kernel
                for stats in (True, False):
                    _apply(K, dtype, shape, res_kind, gate, stats=stats)
    for gate, slope, stats in ((False, False, True), (True, False, False), (True, True, True), (False, True, False)):
        _apply(K, dtype, shape, 1, gate, slope=slope, res_stride=2, stats=stats)


# ------------------------------------------------------------------------------------------------ fr_bn_bwd_reduce
def _bwd_kw(o, dtype, B, H, W, C, nb):
    return dict(g=dev(o["g"], dtype), x=dev(o["x"], dtype), mean=dev(o["mean"]), invstd=dev(o["invstd"]),
                scale=dev(o.get("scale")), shift=dev(o.get("shift")), slope=dev(o.get("slope")), se=guarded(o.get("se")),
                gse=guarded(o.get("gse")), rows=B * H * W, C=C, rows_per_image=H * W, nblocks=nb)


@pytest.mark.parametrize("shape,name,dtype", EW_DT, ids=EW_DT_IDS)
def test_bn_bwd_reduce(K, shape, name, dtype):
    """fr_bn_bwd_reduce, g' plain, behind a PReLU slope, behind a gate with and without gse.  bf16 with lean_ok(C): the lean
    kernel serves all four (bn_bwd_reduce_lean_kernel<SLOPE, SE>; only gate AND slope together, or a slope without scale / shift,
    fall through); fp32, and bf16 at C = 2048, take bn_bwd_reduce_kernel<T>.  All three part vectors are compared (the third is
    the slope gradient, zeros without a slope)."""
    B, H, W, C, nb = shape
    for mode in ("plain", "slope", "gate", "gate_gse"):
        o, _, _, terms = bwd_case(B, H, W, C, mode)
        what = "bn_bwd_reduce %s %s %s" % (shape, name, mode)
        part = Buf(nb, 3 * C, dtype=F32)
        run = K.bn_bwd_reduce(K.current_stream_ptr(), K.fr_dtype(torch.empty(0, dtype=dtype)), part=part.t,
                              **_bwd_kw(o, dtype, B, H, W, C, nb))
        launch_twice(what, run, {"part": part},
                     lambda: X.assert_sums_equal(part.t.reshape(nb, 3, C), X.column_sums(terms), what + " part rows"))


# ------------------------------------------------------------------------------------------------ fr_bn_bwd_apply
def _bwd_apply(K, dtype, shape, mode="plain", add_kind=0, add_stride=2, nxt=False):
    B, H, W, C, nb = shape
    o, ref, terms = bwd_apply_case(B, H, W, C, mode, add_kind, add_stride, nxt)
    what = "bn_bwd_apply %s %s %s add%d/%d nx%d" % (shape, dtype, mode, add_kind, add_stride, nxt)
    gx = Buf(B * H * W, C, dtype=dtype)
    bufs = {"gx": gx}
    kw = _bwd_kw(o, dtype, B, H, W, C, nb)
    kw.update(gx=gx.t, gamma=dev(o["gamma"]), s0=dev(o["s0"]), s1=dev(o["s1"]), inv_count=o["inv_count"], add_kind=add_kind,
              add=guarded(o.get("add"), dtype), H=H, W=W, add_stride=add_stride if add_kind == 2 else 0)
    if nxt:
        bufs["npart"] = npart = Buf(nb, 2 * C, dtype=F32)
        kw.update(nx=dev(o["nx"], dtype), nmean=dev(o["nmean"]), ninvstd=dev(o["ninvstd"]), npart=npart.t)

    def check():
        X.assert_equal_nhwc(gx.t.reshape(B, H, W, C), ref, what + " gx")
        if nxt:
            X.assert_sums_equal(npart.t.reshape(nb, 2, C), X.column_sums(terms), what + " npart rows")

    launch_twice(what, K.bn_bwd_apply(K.current_stream_ptr(), K.fr_dtype(gx.t), **kw), bufs, check)


@pytest.mark.parametrize("shape", EW, ids=EW_IDS)
def test_bn_bwd_apply_lean(K, shape):
    """fr_bn_bwd_apply in bf16 without a slope, add_kind 0 and 1: lean_ok(C) selects bn_bwd_apply_lean_kernel<ADD, SE, NEXT> --
    with a gate (SE; with and without gse), and without one with and without nx / npart (NEXT: the rows of the BatchNorm in
    front, from the stored gx); C = 2048 takes bn_bwd_apply_kernel<bf16_t>, which has no nx.  A gate together with nx is served
    by no kernel and must be refused, not dropped: where the arguments are lean-eligible the refusal is the check inside the
    gated branch of the launcher; at C = 2048, with or without a gate, it is the older check in front of the general kernel
    ("nx ... is served by the bf16 lean kernel only")."""
    from frhip import _lib
    lean = shape[3] <= 1024
    for add_kind in (0, 1):
        for mode in ("plain", "gate", "gate_gse"):
            _bwd_apply(K, BF, shape, mode, add_kind)
        if lean:
            _bwd_apply(K, BF, shape, "plain", add_kind, nxt=True)
    for mode in ("plain", "gate_gse") if not lean else ("gate_gse",):
        with pytest.raises(_lib.FrhipError):
            _bwd_apply(K, BF, shape, mode, 0, nxt=True)


@pytest.mark.parametrize("shape,name,dtype", EW_DT, ids=EW_DT_IDS)
def test_bn_bwd_apply_general_kernel(K, shape, name, dtype):
    """bn_bwd_apply_kernel<T>: fp32 always, bf16 behind a PReLU slope (`!args->slope` fails for the lean kernel) -- add_kind 0
    and 1, plain / slope / gate."""
    for add_kind in (0, 1):
        for mode in ("slope",) if dtype == BF else ("plain", "slope", "gate_gse"):
            _bwd_apply(K, dtype, shape, mode, add_kind)


SCATTER = [s + (nb,) for s, nb in zip(X.SCATTER_SHAPES, (3, 1, 7))]


@pytest.mark.parametrize("shape", SCATTER, ids=["%d_%d_%d_%d_nb%d" % s for s in SCATTER])
def test_bn_bwd_apply_strided_scatter(K, shape):
    """add_kind 2 against the reference (a scatter written with slices): the add tensor is non-zero on EVERY pixel and sized
    exactly between NaN bands, the shapes are non-square.  bf16, stride 2, even H and W, no gate, rows < 2^24 (scatter_ok): the
    lean kernel (fast_divmod with float reciprocals; Wh = W / 2, HWq = HW / 4), with and without nx.  fp32, or bf16 with a gate
    or a slope: bn_bwd_apply_kernel<T> (integer division)."""
    _bwd_apply(K, BF, shape, "plain", 2)
    _bwd_apply(K, BF, shape, "plain", 2, nxt=True)
    _bwd_apply(K, F32, shape, "plain", 2)
    _bwd_apply(K, F32, shape, "gate_gse", 2)
    _bwd_apply(K, BF, shape, "gate_gse", 2)
    _bwd_apply(K, BF, shape, "slope", 2)


@pytest.mark.parametrize("name,dtype", DTYPES)
def test_bn_bwd_apply_scatter_stride_3(K, name, dtype):
    """add_kind 2 with add_stride 3 at (2, 9, 6, 64): scatter_ok needs stride 2, so both dtypes take bn_bwd_apply_kernel<T>."""
    _bwd_apply(K, dtype, X.SCATTER_S3 + (2,), "plain", 2, add_stride=3)


# ------------------------------------------------------------------------------------------------ statistics
@pytest.mark.parametrize("shape", EW + [X.STATS_LONG], ids=EW_IDS + ["%d_%d_%d_%d_nb%d" % X.STATS_LONG])
def test_channel_and_image_statistics(K, shape):
    """fr_channel_stats (channel_stats_kernel<T>, both dtypes where the launcher serves C) over all part rows and
    fr_image_moments (bf16; one block per image) element for element; HW = 3136 with 5 blocks: many trips per thread."""
    B, H, W, C, nb = shape
    x, terms = stats_case(B, H, W, C)
    st = K.current_stream_ptr()
    for dtype in (BF, F32):
        if not served(C, dtype):
            continue
        what = "channel_stats %s %s" % (shape, dtype)
        part = Buf(nb, 2 * C, dtype=F32)
        xd = guarded(x, dtype)
        run = K.call("fr_channel_stats", xd, B * H * W, C, part.t, nb, K.fr_dtype(xd), st)
        launch_twice(what, run, {"part": part},
                     lambda: X.assert_sums_equal(part.t.reshape(nb, 2, C), X.column_sums(terms), what))
    out = Buf(B, 2 * C, dtype=F32)
    what = "image_moments %s" % (shape,)
    launch_twice(what, K.call("fr_image_moments", guarded(x, BF), B, H * W, C, out.t, st), {"out": out},
                 lambda: X.assert_equal_tensor(out.t.reshape(B, 2, C), X.image_sums(terms), what, ("image", "moment", "channel")))


# ------------------------------------------------------------------------------------------------ squeeze-excite


SE_SQUEEZE_DT = [s + (n, d) for s in X.SE_SQUEEZE for n, d in DTYPES if served(s[2], d)]


@pytest.mark.parametrize("B,H,C,name,dtype", SE_SQUEEZE_DT, ids=["%d_%d_%d_%s" % s[:4] for s in SE_SQUEEZE_DT])
def test_se_squeezes(K, B, H, C, name, dtype):
    """fr_se_gscale (se_pool_kernel<T, true, 1024>) at HW 16, 49, 64 and 196 and fr_se_pool (se_pool_kernel<T, false, 256>) at the
    power-of-two HW 16 and 64 only: it divides the sum by HW."""
    o, gs_ref, pooled_ref = se_squeeze_case(B, H, C)
    st, fr = K.current_stream_ptr(), K.fr_dtype(torch.empty(0, dtype=dtype))
    g, x, scale, shift = guarded(o["g"], dtype), guarded(o["x"], dtype), dev(o["scale"]), dev(o["shift"])
    what = "se_gscale %s %s" % ((B, H, C), name)
    gs = Buf(B, C, dtype=F32)
    launch_twice(what, K.call("fr_se_gscale", g, x, scale, shift, gs.t, B, H * H, C, fr, st), {"gs": gs},
                 lambda: X.assert_equal_tensor(gs.t, gs_ref, what, ("image", "channel")))
    if pooled_ref is not None:
        what = "se_pool %s %s" % ((B, H, C), name)
        pooled = Buf(B, C, dtype=F32)
        launch_twice(what, K.call("fr_se_pool", x, scale, shift, pooled.t, B, H * H, C, fr, st), {"pooled": pooled},
                     lambda: X.assert_equal_tensor(pooled.t, pooled_ref, what, ("image", "channel")))


SE_CHAIN = [s + (False,) for s in X.SE_CHAIN] + [s + (True,) for s in X.SE_REAL_HW]
SE_IDS = ["%d_%d_%d%s" % (s[0], s[1], s[2], "_sums_only" if s[3] else "") for s in SE_CHAIN]


class SeBufs(object):
    def __init__(self, B, C, R, rows_part, nv):
        self.gpooled, self.gz, self.gh = Buf(B, C, dtype=F32), Buf(B, C, dtype=F32), Buf(B, R, dtype=F32)
        self.dw1, self.dw2 = Buf(R, C, dtype=F32), Buf(C, R, dtype=F32)
        self.gs_part, self.bn_part = Buf(rows_part, nv * C, dtype=F32), Buf(B, 2 * C, dtype=F32)

    def all(self):
        return dict(self.__dict__)


def _check_mlp(b, r, what):
    X.assert_equal_tensor(b.gz.t, r["gz"], what + " gz", ("image", "channel"))
    X.assert_equal_tensor(b.gh.t, r["gh"], what + " gh", ("image", "hidden"))
    X.assert_equal_tensor(b.gpooled.t, r["gpooled"], what + " gpooled", ("image", "channel"))


@pytest.mark.parametrize("name,dtype", DTYPES)
@pytest.mark.parametrize("B,H,C,zero_w1", SE_CHAIN, ids=SE_IDS)
def test_se_backward(K, B, H, C, zero_w1, name, dtype):
    """fr_se_gscale_mlp_bwd on its two paths -- gs_part == NULL: se_gscale_mlp_bwd_kernel<T>, gs stays in LDS; gs_part given:
    se_gsq_part_kernel<T> over row slices + se_mlp_bwd_parts_kernel -- with dw1 / dw2 (se_mlp_wgrad_kernel behind it) and
    without (the buffers keep their sentinels), and fr_se_gscale_mlp_bwd_sums (se_gsq_part_kernel<T, true>: four vectors per
    slice, and the rows of BN2's backward sums).  Power-of-two HW: the full chain gz, gh, gpooled, dW1, dW2, bn_part element for
    element.  HW 49 and 196 (w1 = 0, so gse = 0): the per-image sums -- gs through gz and gh, the slices of gs_part added up,
    bn_part."""
    HW, R = H * H, max(C // 16, 1)
    o, r = se_bwd_case(B, H, C, zero_w1)
    st, fr = K.current_stream_ptr(), K.fr_dtype(torch.empty(0, dtype=dtype))
    S = int(K.lib.fr_se_gscale_slices(B, HW))
    g, x = guarded(o["g"], dtype), guarded(o["x"], dtype)
    d = {k: guarded(o[k]) for k in ("scale", "shift", "mean", "invstd", "s", "hidden", "pooled", "w1", "w2")}
    for path, with_dw in (("lds", True), ("lds", False), ("sliced", True), ("sliced", False)):
        what = "se_gscale_mlp_bwd %s %s %s dw%d" % ((B, H, C), name, path, with_dw)
        b = SeBufs(B, C, R, B * S, 1)
        run = K.call("fr_se_gscale_mlp_bwd", g, x, d["scale"], d["shift"], d["s"], d["hidden"], d["pooled"], d["w1"], d["w2"],
                     b.gpooled.t, b.dw1.t if with_dw else None, b.dw2.t if with_dw else None, b.gz.t, b.gh.t,
                     b.gs_part.t if path == "sliced" else None, B, C, R, HW, fr, st)

        def check():
            _check_mlp(b, r, what)
            if path == "sliced":
                X.assert_equal_tensor(b.gs_part.t.reshape(B, S, C).double().sum(1), r["gs"], what + " gs_part", ("image", "channel"))
            if with_dw:
                X.assert_equal_tensor(b.dw1.t, r["dw1"], what + " dw1", ("hidden", "channel"))
                X.assert_equal_tensor(b.dw2.t, r["dw2"], what + " dw2", ("channel", "hidden"))

        launch_twice(what, run, b.all(), check)
    what = "se_gscale_mlp_bwd_sums %s %s" % ((B, H, C), name)
    b = SeBufs(B, C, R, B * S, 4)
    run = K.call("fr_se_gscale_mlp_bwd_sums", g, x, d["scale"], d["shift"], d["mean"], d["invstd"], d["s"], d["hidden"], d["w1"],
                 d["w2"], b.gpooled.t, b.gz.t, b.gh.t, b.gs_part.t, b.bn_part.t, B, C, R, HW, fr, st)

    def check_sums():
        _check_mlp(b, r, what)
        X.assert_equal_tensor(b.gs_part.t.reshape(B, S, 4, C).double().sum(1), r["parts"], what + " gs_part", ("image", "sum", "channel"))
        X.assert_equal_tensor(b.bn_part.t.reshape(B, 2, C), r["bn"], what + " bn_part", ("image", "sum", "channel"))
        X.assert_sums_equal(b.bn_part.t.reshape(B, 2, C), r["bn"].sum(0), what + " bn_part rows")

    launch_twice(what, run, b.all(), check_sums)


@pytest.mark.parametrize("B,H,C", X.SE_CHAIN, ids=["%d_%d_%d" % s for s in X.SE_CHAIN])
def test_se_mlp_wgrad(K, B, H, C):
    """fr_se_mlp_wgrad on its own (se_mlp_wgrad_kernel: 64 channels x 4 batch quarters per block; B = 130: eight images in
    flight per thread and a ragged tail, B = 3 and 5: quarters with one image or none) on the reference's gz and gh."""
    R = max(C // 16, 1)
    o, r = se_bwd_case(B, H, C, False)
    what = "se_mlp_wgrad %s" % ((B, H, C),)
    dw1, dw2 = Buf(R, C, dtype=F32), Buf(C, R, dtype=F32)
    run = K.call("fr_se_mlp_wgrad", guarded(r["gz"], F32), guarded(r["gh"], F32), guarded(o["hidden"]), guarded(o["pooled"]), dw1.t,
                 dw2.t, B, C, R, K.current_stream_ptr())

    def check():
        X.assert_equal_tensor(dw1.t, r["dw1"], what + " dw1", ("hidden", "channel"))
        X.assert_equal_tensor(dw2.t, r["dw2"], what + " dw2", ("channel", "hidden"))
        assert float(dw1.t.abs().max()) > 0 and float(dw2.t.abs().max()) > 0

    launch_twice(what, run, {"dw1": dw1, "dw2": dw2}, check)
