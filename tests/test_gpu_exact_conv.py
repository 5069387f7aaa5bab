"""Bit-exact checks of the bf16 convolution kernels on integer-valued operands (tests/exact_operands.py).

Every operand is a small integer (or a small integer times a power of two) and every true result fits bf16 / fp32, so the
kernels must EQUAL an integer reference: every pixel of every image, the float64 sum of ALL part rows, every weight-gradient
element.  Two links, both equalities: the kernel against the project's generic implicit GEMM in fp32 (fr_conv_igemm /
fr_conv_wgrad with FR_F32: no shape-specific walk, exact on this data for the same reason) on all images, and that
reference against float64 CPU convolutions on a subset of the images.  Outputs, part rows, weight gradients and slabs live
in sentinel-filled buffers with guard bands and (one launch per family at least) padded row strides; the guards must stay
untouched, and a second launch into the same buffers must leave the same bits.

The case tables are those of test_gpu_kernels.py, which keeps the checks of the rounding behaviour (integer data cannot
see rounding).  Not covered here because they divide or multiply by 1 / rows: the moments -> statistics finalisation
(fr_bn_finalize_res) and the BatchNorm-backward weight gradient of the stem (fr_stem_wgrad_bn / _r).
The channel-wise passes (BatchNorm apply / backward, statistics, squeeze-excite) are pinned the same way by the sibling
test_gpu_exact_elementwise.py.
"""
import pytest
import torch

import exact_operands as X
import test_gpu_kernels as T
from test_gpu_kernels import K, s2_walk  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
SENTINEL = 24576.0   # a bf16 value no result reaches (assert_exact_range keeps them <= 256)
GUARD = 4096         # elements in front of and behind every buffer a kernel writes


def _cases(test):
    """The parametrize list of a test of test_gpu_kernels.py (the mark closest to the function)."""
    return list(test.pytestmark[0].args[1])


RES_CASES = _cases(T.test_residual_sum_by_its_consumer_and_statistics_from_moments)
RES_SE_CASES = _cases(T.test_residual_sum_behind_a_squeeze_excite_unit)
STREAM_CASES = _cases(T.test_conv1x1_stream_equals_the_generic_gemm)
STEM_M = sorted({16, 1000, 4099, 16 * 37 + 5, 64 * 5 + 23, 64 * 2048 + 64 * 3 + 9})  # the M grids of the stem tests


class Buf(object):
    """[rows][cols] with row stride ld >= cols, sentinel-filled, between two guard bands."""

    def __init__(self, rows, cols, ld=None, dtype=BF):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.flat = torch.full((2 * GUARD + rows * self.ld,), SENTINEL, device="cuda", dtype=dtype)
        self.view = self.flat[GUARD:GUARD + rows * self.ld].view(rows, self.ld)
        self.t = self.view[:, :cols]  # what the kernel gets: data_ptr() is the first payload element

    def assert_guards(self, what):
        assert bool((self.flat[:GUARD] == SENTINEL).all()), "%s: store in front of the buffer" % what
        assert bool((self.flat[GUARD + self.rows * self.ld:] == SENTINEL).all()), "%s: store behind the buffer" % what
        if self.ld > self.cols:
            assert bool((self.view[:, self.cols:] == SENTINEL).all()), "%s: store into the row padding" % what

    def bits(self):
        return self.flat.clone()


def _same_bits(a, b):
    return torch.equal(a.view(torch.int16), b.view(torch.int16))


def _anchor(B):
    """Images convolved in float64 on the host: all up to 8, else the first, a middle and the last of T._image_subset."""
    sel = T._image_subset(B)
    return sel if B <= 8 else [sel[0], sel[len(sel) // 2], sel[-1]]


def _generic(K, src32, w32, rows_out, N, geom, mode, pro=0, pa=None, pb=None, extra=None):
    """fp32 accumulators [rows_out][N] of the generic implicit GEMM."""
    acc = torch.full((rows_out, N), float("nan"), device="cuda")
    K.conv(K.current_stream_ptr(), K.FR_F32, src=src32, w=w32, out=acc, mode=mode, lda=src32.shape[-1], ldc=N, pro=pro,
           pro_a=pa, pro_b=pb, epi=K.EPI_STORE, **geom, **(extra or {}))()
    torch.cuda.synchronize()
    assert not torch.isnan(acc).any(), "the generic reference left rows unwritten"
    return acc


EPI = {"store": "EPI_STORE", "stats": "EPI_STATS", "stats_x": "EPI_STATS_X", "prelu_bwd": "EPI_PRELU_BWD",
       "bnbwd": "EPI_BNBWD", "bias_res": "EPI_BIAS_RES"}
TERM_QUANTUM = {"bnbwd": 0.5}  # (aux - mean) * invstd is a multiple of 1/2


def check_conv(K, launch, nparts, src, w_dev, w_ref, out_shape, geom, mode, kind, pro="none", pa=None, pb=None, aux=None,
               ea=None, eb=None, pads=(0, 0, 0), host=None, what="", extra=None, stored_quantum=1.0):
    """One kernel launch on exact operands against the generic fp32 GEMM (all images) and float64 on the host (`host`:
    (sel, function of sel -> float64 accumulators)).
    src [B, SH, SW, SC] / aux [B, RH, RW, N] bf16-exact float tensors on the device; w_dev the weights the kernel reads
    (plain or fragment order), w_ref [N][taps][SC] the same weights in plain order; pads = (lda, ldc, ldaux) - channels."""
    B, RH, RW, N = out_shape
    SC = src.shape[-1]
    rows = B * RH * RW
    dev = lambda v: None if v is None else v.cuda()  # noqa: E731
    pa_d, pb_d, ea_d, eb_d = dev(pa), dev(pb), dev(ea), dev(eb)
    par = {k: v for k, v in (extra or {}).items() if k.startswith("par_")}
    acc = _generic(K, src.float().contiguous(), w_ref.float().contiguous(), rows, N, geom, mode, X.PRO[pro], pa_d, pb_d, par)
    acc = acc.view(B, RH, RW, N)
    if host is not None:
        sel, fn = host
        X.assert_equal_nhwc(acc[sel].cpu(), fn(sel), what + " [generic fp32 GEMM vs float64 host]")
    stored, terms = X.epilogue(kind, acc, aux, ea_d, eb_d)
    ipr = X.images_per_part_row(nparts, B) if terms else 1
    X.assert_exact_range(stored=[stored], terms=terms, images_per_row=ipr, quantum=stored_quantum,
                         term_quantum=TERM_QUANTUM.get(kind, 1.0), what=what)
    lda, ldc, ldaux = SC + pads[0], N + pads[1], N + pads[2]
    src_b = X.padded(src.to(BF), lda)
    aux_b = None if aux is None else X.padded(aux.to(BF), ldaux)
    out = Buf(rows, N, ldc)
    nv = 3 if kind == "stats_x" else 2  # a part row always holds [2][N] ([3][N]: STATS_X), whatever the kind sums (frhip.h)
    part = Buf(nparts, nv * N, dtype=torch.float32) if terms else None
    kw = dict(src=src_b, w=w_dev, out=out.t, mode=mode, lda=lda, ldc=ldc, pro=X.PRO[pro], pro_a=pa_d, pro_b=pb_d,
              epi=getattr(K, EPI[kind]), **geom)
    if aux is not None:
        kw.update(aux=aux_b, ldaux=ldaux)
    if ea is not None:
        kw.update(epi_a=ea_d)
    if eb is not None:
        kw.update(epi_b=eb_d)
    if part is not None:
        kw.update(part=part.t)
    kw.update(extra or {})
    run = launch(K.current_stream_ptr(), **kw)
    run()
    torch.cuda.synchronize()
    out.assert_guards(what + " out")
    X.assert_equal_nhwc(out.t.reshape(B, RH, RW, N), stored, what + " out")
    if part is not None:
        part.assert_guards(what + " part")
        X.assert_sums_equal(part.t.reshape(nparts, nv, N)[:, :len(terms)], X.column_sums(terms), what + " part rows")
    first = (out.bits(), part.bits() if part is not None else None)
    run()
    torch.cuda.synchronize()
    assert _same_bits(first[0], out.flat), what + ": second launch changed the output"
    if part is not None:
        assert _same_bits(first[1], part.flat), what + ": second launch changed the part rows"
    return acc


# ------------------------------------------------------------------------------------------------ operands of a 3x3 layer
class Layer(object):
    """Exact operands of a cin -> cout 3x3 layer on W x W inputs (stride 1 or 2), batch B: forward input per prologue, output
    gradient, aux tensors and coefficients of the gradient epilogues."""

    def __init__(self, seed, cin, cout, W, B, stride=1):
        self.cin, self.cout, self.W, self.B, self.stride, self.seed = cin, cout, W, B, stride, seed
        self.Wo = W // stride
        self.p = X.density(cin, W)
        self.w = X.ternary(seed, "w", (cout, 9, cin), self.p)                       # [cout][9][cin]
        self.wt = self.w.permute(2, 1, 0).contiguous()                              # [cin][9][cout]: data gradient
        self.sel = _anchor(B)

    def x(self, pro):
        return X.activations(self.seed, "x." + pro, (self.W, self.W, self.cin), self.p, pro)

    def pro(self, pro):
        return X.prologue_coeffs(self.seed, "pro", self.cin, pro)

    def g(self):
        return X.ternary(self.seed, "g", (X.BASE_IMAGES, self.Wo, self.Wo, self.cout), X.density(self.cout, self.W))

    def aux(self, tag, C, W):
        return X.ternary(self.seed, tag, (X.BASE_IMAGES, W, W, C), 0.5)

    def geom(self, mode):
        if mode == 0:
            return dict(B=self.B, RH=self.Wo, RW=self.Wo, SH=self.W, SW=self.W, SC=self.cin, N=self.cout, KH=3, KW=3,
                        stride=self.stride, pad=1)
        return dict(B=self.B, RH=self.W, RW=self.W, SH=self.Wo, SW=self.Wo, SC=self.cout, N=self.cin, KH=3, KW=3,
                    stride=self.stride, pad=1)

    def forward(self, K, launch, nparts, kind, pro, pads=(0, 0, 0), w_dev=None, what="", extra=None, aux_base=None, ea=None,
                eb=None):
        base = self.x(pro)
        pa, pb = self.pro(pro)
        host = (self.sel, lambda sel: X.conv_forward(X.apply_prologue(X.batch(base, self.B, sel), pro, pa, pb), self.w,
                                                     self.stride))
        aux = None if aux_base is None else X.batch(aux_base, self.B, device="cuda")
        return check_conv(K, launch, nparts, X.batch(base, self.B, device="cuda"),
                          self.w.to("cuda", BF) if w_dev is None else w_dev, self.w.cuda(),
                          (self.B, self.Wo, self.Wo, self.cout), self.geom(0), 0, kind, pro,
                          pa if pro != "none" else None, pb if pro == "bn" else None, aux=aux, ea=ea, eb=eb, pads=pads,
                          host=host, what="%s fwd %s/%s" % (what, pro, kind), extra=extra)

    def dgrad(self, K, launch, nparts, kind, mode, pads=(0, 0, 0), w_dev=None, what="", extra=None):
        gb = self.g()
        host = (self.sel, lambda sel: X.conv_dgrad(X.batch(gb, self.B, sel), self.w, self.stride, self.W))
        aux = X.batch(self.aux("aux", self.cin, self.W), self.B, device="cuda") if kind != "store" else None
        ea = eb = None
        quantum = 1.0
        if kind == "prelu_bwd":
            ea, quantum = X.pick(self.seed, "slope", self.cin, [0.25, 0.5]), 0.25
        elif kind == "bnbwd":
            ea = X.pick(self.seed, "mean", self.cin, [-1.0, 0.0, 1.0])
            eb = X.pick(self.seed, "invstd", self.cin, [0.5, 1.0, 2.0])
        ex = dict(extra or {})
        if mode == 2:
            ex.update(par_h=-1, par_w=-1)
        return check_conv(K, launch, nparts, X.batch(gb, self.B, device="cuda"),
                          self.wt.to("cuda", BF) if w_dev is None else w_dev, self.wt.cuda(),
                          (self.B, self.W, self.W, self.cin), self.geom(mode), mode, kind, aux=aux, ea=ea, eb=eb, pads=pads,
                          host=host, what="%s dgrad %s" % (what, kind), extra=ex, stored_quantum=quantum)


# ------------------------------------------------------------------------------------------------ fr_conv3x3_strip
@pytest.mark.parametrize("cin,cout,W,B", T.STRIP_CASES, ids=["%d_%d_%d_b%d" % s for s in T.STRIP_CASES])
def test_strip_forward_and_data_gradient(K, cin, cout, W, B):
    """fr_conv3x3_strip (LDS strip and conv3x3_roll64): forward with the three prologues + STATS over all part rows, data
    gradient with the PRELU_BWD and BNBWD epilogues -- every image.  Padded lda / ldc / ldaux on the BN-prologue forward
    and the BNBWD gradient."""
    L = Layer(131, cin, cout, W, B)
    store_only = (cin, cout, W) == (256, 512, 14)  # two 256-channel passes: plain store only
    kind = "store" if store_only else "stats"
    nparts = K.strip_parts(B, cin, cout, W, getattr(K, EPI[kind]))
    assert nparts > 0
    for pro in ("none", "bn", "prelu"):
        L.forward(K, K.conv_strip, nparts, kind, pro, pads=(8, 16, 0) if pro == "bn" else (0, 0, 0), what="strip")
    nparts = K.strip_parts(B, cout, cin, W, K.EPI_BNBWD)
    if nparts == 0:  # the dispatch table has no data gradient with sums for this shape (test_gpu_kernels.test_conv3x3_strip)
        return
    L.dgrad(K, K.conv_strip, nparts, "prelu_bwd", 1, what="strip")
    L.dgrad(K, K.conv_strip, nparts, "bnbwd", 1, pads=(8, 16, 24), what="strip")


@pytest.mark.parametrize("cin,cout,W,B", T.FRAG_CASES, ids=["%d_%d_%d_b%d" % s for s in T.FRAG_CASES])
def test_strip_fragment_order_weights(K, cin, cout, W, B):
    """The same with the weights in MFMA-fragment order (FrConvArgs.w_frag): BN prologue + STATS forward, plain data gradient."""
    from frhip import _lib
    assert _lib.lib.fr_conv3x3_strip_takes_frag(B, cin, cout, W) == 1
    L = Layer(137, cin, cout, W, B)
    kind = "store" if (cin, cout, W) == (256, 512, 14) else "stats"
    nparts = K.strip_parts(B, cin, cout, W, getattr(K, EPI[kind]))
    assert nparts > 0
    L.forward(K, K.conv_strip, nparts, kind, "bn", w_dev=T.to_frag(L.w.to("cuda", BF)), extra=dict(w_frag=1), what="strip frag")
    if K.strip_parts(B, cout, cin, W, K.EPI_STORE):
        L.dgrad(K, K.conv_strip, 1, "store", 1, w_dev=T.to_frag(L.wt.to("cuda", BF)), extra=dict(w_frag=1), what="strip frag")


# ------------------------------------------------------------------------------------------------ residual sum by its consumer
def _resbn(K, B, C, W, Cn, se):
    from frhip import _lib
    st = K.current_stream_ptr()
    what = "resbn%s %d_%d_%d_b%d" % ("_se" if se else "", C, Cn, W, B)
    geom = dict(B=B, RH=W, RW=W, SH=W, SW=W, SC=C, N=Cn, KH=3, KW=3, stride=1, pad=1)
    if not _lib.lib.fr_conv3x3_strip_serves_resbn(B, C, W):  # a shape that is not served must be refused, not computed
        t = lambda c: torch.zeros(B * W * W, c, device="cuda", dtype=BF)  # noqa: E731
        one = torch.ones(C, device="cuda")
        with pytest.raises(_lib.FrhipError):
            K.conv_strip(st, src=t(C), src2=t(C), pro_out=t(C), out=t(Cn), w=torch.zeros(Cn, 9, C, device="cuda", dtype=BF),
                         pro=K.PRO_RESBN, pro_a=one, pro_b=one, pro_c=one, pro_d=one, mode=0, lda=C, ldc=Cn, epi=K.EPI_STORE,
                         **geom)()
        return
    # (1) conv2 with FR_EPI_STATS_X: PReLU prologue, aux = the unit's input; three sums per part row
    L2 = Layer(139, C, C, W, B)
    nparts = K.strip_parts(B, C, C, W, K.EPI_STATS_X)
    assert nparts > 0
    L2.forward(K, K.conv_strip, nparts, "stats_x", "prelu", pads=(0, 0, 8), aux_base=L2.aux("xin", C, W), what=what)
    # (2) the next conv1 forms o = a * y2 + b (* gate) + x2 and stores it, operand c * o + d
    p = X.density(C, W) * (0.3 if se else 0.5)  # (gates up to 2 and half-integers: keep conv1's output within 8 bits)
    y2 = X.batch(X.ternary(141, "y2", (X.BASE_IMAGES, W, W, C), p), B, device="cuda")
    x2 = X.batch(X.ternary(141, "x2", (X.BASE_IMAGES, W, W, C), p), B, device="cuda")
    a, b = (v.cuda() for v in X.prologue_coeffs(141, "ab", C, "bn"))
    c, d = (v.cuda() for v in X.prologue_coeffs(141, "cd", C, "bn"))
    w = X.ternary(141, "w1n", (Cn, 9, C), X.density(C, W))
    o = y2.double() * a.double() + b.double()
    gate = None
    if se:
        gate = X.pick(141, "gate", B * C, [0.5, 1.0, 2.0]).view(B, C).cuda()
        o = o * gate.double().view(B, 1, 1, C)
    o = o + x2.double()
    X.assert_exact_range(stored=[o], quantum=0.5 if se else 1.0, what=what + " residual sum")
    acc = _generic(K, o.float().contiguous(), w.cuda(), B * W * W, Cn, geom, 0, X.PRO["bn"], c, d).view(B, W, W, Cn)
    sel = _anchor(B)
    X.assert_equal_nhwc(acc[sel].cpu(), X.conv_forward(X.apply_prologue(o[sel].cpu(), "bn", c.cpu(), d.cpu()), w),
                        what + " [generic vs host]")
    X.assert_exact_range(stored=[acc], quantum=0.5 if se else 1.0, what=what + " conv1")
    lda, ldc = C + 8, Cn + 8
    z, out1 = Buf(B * W * W, Cn, ldc), Buf(B * W * W, C, lda)
    kw = dict(src=X.padded(y2.to(BF), lda), src2=X.padded(x2.to(BF), lda), pro_out=out1.t, out=z.t, w=w.to("cuda", BF),
              pro=K.PRO_RESBN_SE if se else K.PRO_RESBN, pro_a=a, pro_b=b, pro_c=c, pro_d=d, mode=0, lda=lda, ldc=ldc,
              epi=K.EPI_STORE, **geom)
    if se:
        kw.update(pro_g=gate)
    run = K.conv_strip(st, **kw)
    run()
    torch.cuda.synchronize()
    z.assert_guards(what + " out")
    out1.assert_guards(what + " pro_out")
    X.assert_equal_nhwc(out1.t.reshape(B, W, W, C), o, what + " pro_out")
    X.assert_equal_nhwc(z.t.reshape(B, W, W, Cn), acc, what + " out")
    bits = (z.bits(), out1.bits())
    run()
    torch.cuda.synchronize()
    assert _same_bits(bits[0], z.flat) and _same_bits(bits[1], out1.flat), what + ": second launch changed the result"


@pytest.mark.parametrize("B,C,W,Cn", RES_CASES)
def test_residual_sum_by_its_consumer(K, B, C, W, Cn):
    """FR_EPI_STATS_X (output + the three sums over all part rows) and FR_PRO_RESBN (pro_out and the convolution of it), with a
    padded lda (src, src2 and pro_out share it).  The moments -> statistics finalisation divides and is not in scope.  Shapes
    the kernel does not serve must be refused."""
    _resbn(K, B, C, W, Cn, se=False)


@pytest.mark.parametrize("B,C,W,Cn", RES_SE_CASES)
def test_residual_sum_behind_a_squeeze_excite_unit(K, B, C, W, Cn):
    """FR_PRO_RESBN_SE: per-image gates from {1/2, 1, 2}."""
    _resbn(K, B, C, W, Cn, se=True)


# ------------------------------------------------------------------------------------------------ fr_conv3x3_s2_strip
S2_ALL = [c + (None,) for c in T.S2_CASES] + [(C, WL, B, "", ws) for (C, WL, B) in T.S2_FRAG_CASES for ws in (1, 0)]


@pytest.mark.parametrize("C,WL,B,walk,ws", S2_ALL, ids=["%d_%d_b%d%s_ws%s" % s for s in S2_ALL])
def test_s2_strip_forward_and_data_gradient(K, s2_walk, C, WL, B, walk, ws):  # noqa: F811
    """fr_conv3x3_s2_strip: forward (strip, conv3x3_s2_roll64 incl. the whole-image walk, conv3x3_s2_ws; both settings of
    FRHIP_S2_WS on the S2_FRAG_CASES, there with fragment-order weights) with three prologues + STATS, data gradient with the
    PRELU_BWD and BNBWD epilogues (the 64-channel rolling-window gradient serves PRELU_BWD only and refuses the other)."""
    s2_walk(walk)
    L = Layer(149, C, C, 2 * WL, B, stride=2)
    frag = ws is not None
    prev = K.set_option("FRHIP_S2_WS", ws) if frag else None
    try:
        wf = dict(w_dev=T.to_frag(L.w.to("cuda", BF)), extra=dict(w_frag=1)) if frag else {}
        wb = dict(w_dev=T.to_frag(L.wt.to("cuda", BF)), extra=dict(w_frag=1)) if frag else {}
        n = K.s2_strip_parts(B, C, C, WL, 0)
        assert n > 0
        for pro in ("none", "bn", "prelu"):
            L.forward(K, K.conv_s2_strip, n, "stats", pro, pads=(8, 16, 0) if pro == "bn" else (0, 0, 0), what="s2", **wf)
        n2 = K.s2_strip_parts(B, C, C, WL, 2)
        assert n2 > 0
        L.dgrad(K, K.conv_s2_strip, n2, "prelu_bwd", 2, pads=(8, 16, 24), what="s2", **wb)
        if C != 64:
            L.dgrad(K, K.conv_s2_strip, n2, "bnbwd", 2, what="s2", **wb)
    finally:
        if frag:
            K.set_option("FRHIP_S2_WS", prev)


# ------------------------------------------------------------------------------------------------ fr_conv1x1_stream
@pytest.mark.parametrize("Kc,N,B,Ho,stride", STREAM_CASES)
def test_conv1x1_stream(K, Kc, N, B, Ho, stride):
    """fr_conv1x1_stream: the strided shortcut convolutions and (stride 1, N < Kc) their data gradients, output + STATS sums."""
    H = Ho * stride
    p = X.density(Kc, 0, taps=1)
    base = X.ternary(151, "x", (X.BASE_IMAGES, H, H, Kc), p)
    w = X.ternary(151, "w", (N, 1, Kc), p)
    nps = K.conv1x1_stream_parts(B, Ho, Ho, Kc, N)
    assert nps > 0
    geom = dict(B=B, RH=Ho, RW=Ho, SH=H, SW=H, SC=Kc, N=N, KH=1, KW=1, stride=stride, pad=0)
    host = (list(range(min(B, 8))), lambda s: X.conv_forward(X.batch(base, B, s), w, stride, k=1))
    for kind, pads in (("stats", (8, 16, 0)), ("store", (0, 0, 0))):
        check_conv(K, K.conv1x1_stream, nps, X.batch(base, B, device="cuda"), w.view(N, Kc).to("cuda", BF), w.cuda(),
                   (B, Ho, Ho, N), geom, 0, kind, pads=pads, host=host, what="1x1 stream %s" % kind)


# ------------------------------------------------------------------------------------------------ FR_EPI_BIAS_RES
@pytest.mark.parametrize("name,dtype,C,H,stride", T.BIAS_RES_CASES, ids=[c[0] for c in T.BIAS_RES_CASES])
def test_bias_residual_epilogue(K, name, dtype, C, H, stride):
    """FR_EPI_BIAS_RES on every kernel that serves it: bias, shift and shortcut as integers (PReLU prologue)."""
    B = 3
    L = Layer(157, C, C, H, B, stride=stride)
    ea, eb = X.pick(157, "ea", C, [-1.0, 0.0, 1.0, 2.0]), X.pick(157, "eb", C, [-2.0, 0.0, 1.0])
    res = L.aux("res", C, H // stride)
    pads = (8, 16, 24)
    if name.startswith("igemm"):
        fr = K.fr_dtype(torch.empty(0, dtype=dtype))
        if dtype == torch.float32:  # the reference kernel itself with this epilogue: fp32 tensors, against float64 on the host
            pa, _ = L.pro("prelu")
            x, r = X.batch(L.x("prelu"), B, device="cuda"), X.batch(res, B, device="cuda")
            out = torch.full((B * L.Wo * L.Wo, C), float("nan"), device="cuda")
            K.conv(K.current_stream_ptr(), fr, src=x, w=L.w.cuda(), out=out, mode=0, lda=C, ldc=C, ldaux=C, pro=K.PRO_PRELU,
                   pro_a=pa.cuda(), epi=K.EPI_BIAS_RES, epi_a=ea.cuda(), epi_b=eb.cuda(), aux=r, **L.geom(0))()
            torch.cuda.synchronize()
            acc = X.conv_forward(X.apply_prologue(x.cpu(), "prelu", pa, None), L.w, stride)
            want, _ = X.epilogue("bias_res", acc, r.cpu(), ea, eb)
            X.assert_equal_nhwc(out.view(B, L.Wo, L.Wo, C).cpu(), want, "bias_res igemm f32")
            return
        launch = lambda st, **kw: K.conv(st, fr, **kw)  # noqa: E731
    elif name.startswith("s2"):
        assert K.s2_strip_parts(B, C, C, H // stride, 0) > 0
        launch = K.conv_s2_strip
    else:
        assert K.strip_parts(B, C, C, H, K.EPI_BIAS_RES) > 0
        launch = K.conv_strip
    L.forward(K, launch, 1, "bias_res", "prelu", pads=pads, aux_base=res, ea=ea, eb=eb, what="bias_res " + name)


# ------------------------------------------------------------------------------------------------ fr_conv_wgrad_strip
def _wgrad_operands(seed, cout, cin, W, B, pro, stride):
    Wo = W // stride
    x = X.batch(X.activations(seed, "x", (W, W, cin), X.density(cin, W), pro), B)
    g = X.batch(X.ternary(seed, "g", (X.BASE_IMAGES, Wo, Wo, cout), X.density(cin, W)), B)
    pa, pb = X.prologue_coeffs(seed, "pro", cin, pro)
    return x, g, pa, pb


def _wgrad_reference(K, x, g, pa, pb, pro, stride, what):
    """float64 on the host and the generic fp32 weight gradient (one slice, atomics onto zeros) on the device: equal, in range."""
    B, W, _, cin = x.shape
    cout, Wo = g.shape[-1], g.shape[1]
    xin = X.apply_prologue(x, pro, pa, pb)
    X.assert_exact_range(wgrad_abs=X.wgrad_abs_bound(g, xin), what=what)
    ref = X.conv_wgrad(g, xin, stride)
    dw = torch.zeros(cout, 9, cin, device="cuda")
    K.wgrad(K.current_stream_ptr(), K.FR_F32, g=g.cuda().contiguous(), src=x.cuda().contiguous(), dw=dw, B=B, GH=Wo, GW=Wo,
            Cout=cout, SH=W, SW=W, SC=cin, KH=3, KW=3, stride=stride, pad=1, ldg=cout, lda=cin, pro=X.PRO[pro], nsplit=1,
            pro_a=pa.cuda(), pro_b=pb.cuda())()
    torch.cuda.synchronize()
    X.assert_equal_tensor(dw, ref, what + " [generic fp32 vs float64 host]", ("cout", "tap", "cin"))
    assert float(dw.abs().max()) > 0
    return dw


def _wgrad_strip(K, cout, cin, W, B, pro, groups, stride, seed, pads=(0, 0), kernel=None):
    what = "wgrad %d_%d_%d_%s_b%d_g%d_s%d" % (cout, cin, W, pro, B, groups, stride)
    x, g, pa, pb = _wgrad_operands(seed, cout, cin, W, B, pro, stride)
    ref = _wgrad_reference(K, x, g, pa, pb, pro, stride, what)
    n = cout * 9 * cin
    dw, slab = Buf(1, n, dtype=torch.float32), Buf(1, groups * n, dtype=torch.float32)
    Wo = W // stride
    ldg, lda = cout + pads[0], cin + pads[1]
    run = K.wgrad_strip(K.current_stream_ptr(), g=X.padded(g.to("cuda", BF), ldg), src=X.padded(x.to("cuda", BF), lda), dw=dw.t,
                        slab=slab.t, B=B, GH=Wo, GW=Wo, Cout=cout, SH=W, SW=W, SC=cin, KH=3, KW=3, stride=stride, pad=1,
                        ldg=ldg, lda=lda, pro=X.PRO[pro], nsplit=groups, pro_a=pa.cuda(), pro_b=pb.cuda())
    if kernel is not None:
        assert K.wgrad_strip_kernel(run.keep[0]) == kernel, what + ": fr_conv_wgrad_strip_kernel"
    run()
    torch.cuda.synchronize()
    dw.assert_guards(what + " dW")
    slab.assert_guards(what + " slab")
    X.assert_equal_tensor(dw.t.view(cout, 9, cin), ref, what + " dW", ("cout", "tap", "cin"))
    bits = dw.bits()
    run()
    torch.cuda.synchronize()
    assert torch.equal(bits, dw.flat), what + ": second launch changed dW"


@pytest.mark.parametrize("cout,cin,W,pro,B,groups", T.WGS_CASES, ids=["%d_%d_%d_%s_b%d_g%d" % s for s in T.WGS_CASES])
def test_wgrad_strip(K, cout, cin, W, pro, B, groups):
    """fr_conv_wgrad_strip, stride 1 (strip and warp-specialised kernels): every dW element; dW and the slabs start as sentinels.
    Padded ldg / lda where the group count is 3."""
    assert K.wgrad_strip_supported(cout, cin, W)
    _wgrad_strip(K, cout, cin, W, B, pro, groups, 1, 163, pads=(8, 16) if groups == 3 else (0, 0))


@pytest.mark.parametrize("C,WL", T.S2_SHAPES, ids=["%d_%d" % s for s in T.S2_SHAPES])
@pytest.mark.parametrize("groups", [1, 3, 5])
def test_wgrad_strip_stride2(K, C, WL, groups):
    """fr_conv_wgrad_strip on the stride-2 layers (parity planes; the stride-2 rolling kernel), PReLU prologue."""
    _wgrad_strip(K, C, C, 2 * WL, 3, "prelu", groups, 2, 167, pads=(8, 16) if groups == 3 else (0, 0))


# (stride, gradient width, B, groups, kernel): the group count AT each warp-specialised line's limit -- one image (7x7,
# 14x14), phase (28x28: 7 per image; stride 2: 1 at 7x7, 4 at 14x14) per group -- and one past it at the stride-2 7x7 line,
# where the launch goes to the strip kernel instead
WGS_LIMIT_CASES = [(1, 7, 2, 2, "WGRAD_ROLL"), (1, 14, 2, 2, "WGRAD_ROLL"), (1, 28, 2, 14, "WGRAD_ROLL"),
                   (2, 7, 3, 3, "WGRAD_S2ROLL"), (2, 14, 3, 12, "WGRAD_S2ROLL"), (2, 7, 3, 4, "WGRAD_STRIP_S2")]


@pytest.mark.parametrize("stride,WG,B,groups,kernel", WGS_LIMIT_CASES, ids=["s%d_%d_b%d_g%d_%s" % s for s in WGS_LIMIT_CASES])
def test_wgrad_strip_at_the_group_limits_of_the_table(K, stride, WG, B, groups, kernel):
    """The smallest launches at which a limit of select_wgrad can be off by one (64 channels): the instance
    fr_conv_wgrad_strip_kernel names for the arguments is the expected one, and every dW element is exact."""
    assert K.lib.fr_get_option(b"FRHIP_WGRAD_ROLL", 1) == 1
    _wgrad_strip(K, 64, 64, WG * stride, B, "prelu", groups, stride, 173, kernel=getattr(K, kernel))


def test_wgrad_deferred_slab_chain(K):
    """The deferred-slab chain of test_conv_wgrad_deferred_slab_sum_is_bit_identical (each launch leaves the sum of its slabs to
    the next one, fr_reduce_slabs flushes the last): every dW of the chain equals the integer reference, twice over."""
    st = K.current_stream_ptr()
    layers = [(256, 256, 14, 37, 5, 2), (128, 64, 28, 5, 9, 1), (64, 192, 14, 6, 6, 0), (128, 128, 28, 3, 4, 2),
              (64, 64, 56, 3, 40, 1), (512, 512, 7, 9, 3, 2), (128, 128, 28, 5, 6, 2, 2), (64, 64, 56, 2, 20, 0)]
    names = {0: "none", 1: "bn", 2: "prelu"}
    refs, dws, slabs, kws = [], [], [], []
    for k, layer in enumerate(layers):
        cout, cin, W, B, groups, pro = layer[:6]
        stride = layer[6] if len(layer) > 6 else 1
        x, g, pa, pb = _wgrad_operands(170 + k, cout, cin, W, B, names[pro], stride)
        refs.append(_wgrad_reference(K, x, g, pa, pb, names[pro], stride, "chain layer %d" % k))
        n = cout * 9 * cin
        dws.append(Buf(1, n, dtype=torch.float32))
        slabs.append(Buf(1, groups * n, dtype=torch.float32))
        kws.append(dict(g=g.to("cuda", BF), src=x.to("cuda", BF), B=B, GH=W // stride, GW=W // stride, Cout=cout, SH=W, SW=W,
                        SC=cin, KH=3, KW=3, stride=stride, pad=1, ldg=cout, lda=cin, pro=pro, nsplit=groups, pro_a=pa.cuda(),
                        pro_b=pb.cuda()))
    for rep in range(2):  # the second pass runs the whole chain again into the same buffers
        prev = None
        for k, kw in enumerate(kws):
            extra = {}
            if prev is not None:
                pk = kws[prev]
                extra = dict(prev_slab=slabs[prev].t, prev_dw=dws[prev].t, prev_groups=pk["nsplit"],
                             prev_n=pk["Cout"] * 9 * pk["SC"])
            K.wgrad_strip(st, dw=dws[k].t, slab=slabs[k].t, defer=1, **extra, **kw)()
            prev = k
        last = kws[-1]
        K.call("fr_reduce_slabs", slabs[-1].t, last["nsplit"], last["Cout"] * 9 * last["SC"], dws[-1].t, st)()
        torch.cuda.synchronize()
        for k, layer in enumerate(layers):
            dws[k].assert_guards("chain layer %d dW" % k)
            slabs[k].assert_guards("chain layer %d slab" % k)
            X.assert_equal_tensor(dws[k].t.view(layer[0], 9, layer[1]), refs[k], "chain layer %d pass %d dW" % (k, rep),
                                  ("cout", "tap", "cin"))


# ------------------------------------------------------------------------------------------------ stem
@pytest.mark.parametrize("Kp", [32, 64])
@pytest.mark.parametrize("M", STEM_M)
def test_stem_gemms(K, Kp, M):
    """fr_stem_gemm (rows + statistics), fr_stem_gemm_bn_prelu (the two-pass forward: y, z = PReLU(BN(y)) and the statistics
    of z), fr_stem_wgrad (slabs -> dW) and fr_stem_bwd_sums (backward sums on recomputed rows) on the row grids of the stem
    tests: ragged 16-row tiles and 64-row trips.  Scale from {1, 2, -1}, shift from {-1, 0, 1}, slopes from {1/2, 1}: z is a
    multiple of 1/2.  (fr_stem_wgrad_bn[_r] multiply by 1 / M: not exact; test_gpu_kernels.py compares them bit for bit
    with each other.)  Part rows here are not tied to images: the range condition takes the sum over ALL rows."""
    st = K.current_stream_ptr()
    p = 0.125 * (64.0 / Kp) ** 0.5
    x = X.ternary(181, "x%d" % M, (M, Kp), 1.5 * p).cuda()
    w = X.ternary(181, "w", (64, Kp), p).cuda()
    geom = dict(B=M, RH=1, RW=1, SH=1, SW=1, SC=Kp, N=64, KH=1, KW=1, stride=1, pad=0)
    y = _generic(K, x, w, M, 64, geom, 0).double()
    X.assert_equal_tensor(y.cpu(), x.cpu().double() @ w.cpu().double().t(), "stem [generic vs host]")
    assert float(y.abs().max()) > 0
    yv = y.view(1, 1, M, 64)
    nb = 13
    X.assert_exact_range(stored=[yv], terms=[yv, yv * yv], images_per_row=1, what="stem gemm")
    xb, wb = x.to(BF), w.to(BF)
    out, part = Buf(M, 64), Buf(nb, 128, dtype=torch.float32)
    run = K.call("fr_stem_gemm", xb, wb, out.t, part.t, M, Kp, nb, st)
    scale, shift = (v.cuda() for v in X.prologue_coeffs(181, "bn", 64, "bn"))
    slope = X.pick(181, "slope", 64, [0.5, 1.0]).cuda()
    u = y * scale.double() + shift.double()
    z = torch.where(u > 0, u, u * slope.double()).view(1, 1, M, 64)
    X.assert_exact_range(stored=[z], terms=[z, z * z], quantum=0.5, images_per_row=1, what="stem two-pass")
    y1, z1, pz = Buf(M, 64), Buf(M, 64), Buf(nb, 128, dtype=torch.float32)
    run2 = K.call("fr_stem_gemm_bn_prelu", xb, wb, scale, shift, slope, y1.t, z1.t, pz.t, M, Kp, nb, st)
    g = X.ternary(181, "g%d" % M, (M, 64), 0.5).cuda()
    gb = g.to(BF)
    ns = 7
    slab = Buf(ns, 64 * Kp, dtype=torch.float32)
    run3 = K.call("fr_stem_wgrad", gb, xb, slab.t, M, Kp, ns, st)
    dw_ref = g.double().t() @ x.double()
    X.assert_exact_range(wgrad_abs=X.wgrad_abs_bound(g.view(1, 1, M, 64), x), what="stem wgrad")
    # backward sums on recomputed rows: g' = g * (u > 0 ? 1 : slope), sums g', g' * xhat, g * u * [u <= 0]
    mean = X.pick(181, "mean", 64, [-1.0, 0.0, 1.0]).cuda()
    invstd = X.pick(181, "invstd", 64, [0.5, 1.0, 2.0]).cuda()
    gp = torch.where(u > 0, g.double(), g.double() * slope.double())
    xhat = (y - mean.double()) * invstd.double()
    bterms = [t.view(1, 1, M, 64) for t in (gp, gp * xhat, torch.where(u > 0, torch.zeros_like(u), g.double() * u))]
    X.assert_exact_range(terms=bterms, term_quantum=0.25, images_per_row=1, what="stem backward sums")
    nbs = 11
    pb = Buf(nbs, 192, dtype=torch.float32)
    run4 = K.call("fr_stem_bwd_sums", xb, wb, gb, mean, invstd, scale, shift, slope, pb.t, M, Kp, nbs, st)
    bufs = (out, part, y1, z1, pz, slab, pb)
    bits = None
    for rep in range(2):
        run(), run2(), run3(), run4()
        torch.cuda.synchronize()
        for b, n in zip(bufs, ("out", "part", "y", "z", "part z", "slab", "backward part")):
            b.assert_guards("stem " + n)
        X.assert_equal_tensor(out.t, y, "stem gemm rows", ("row", "column"))
        X.assert_sums_equal(part.t.reshape(nb, 2, 64), X.column_sums([yv, yv * yv]), "stem gemm part rows")
        X.assert_equal_tensor(y1.t, y, "stem two-pass y", ("row", "column"))
        X.assert_equal_tensor(z1.t, z.view(M, 64), "stem two-pass z", ("row", "column"))
        X.assert_sums_equal(pz.t.reshape(nb, 2, 64), X.column_sums([z, z * z]), "stem two-pass part rows")
        X.assert_equal_tensor(slab.t.double().sum(0).view(64, Kp), dw_ref, "stem wgrad", ("cout", "k"))
        X.assert_sums_equal(pb.t.reshape(nbs, 3, 64), X.column_sums(bterms), "stem backward sums")
        now = [b.bits() for b in bufs]
        if bits is not None:
            assert all(_same_bits(a, b) for a, b in zip(bits, now)), "stem: second launch changed a result"
        bits = now
