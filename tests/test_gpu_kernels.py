"""GPU parity of the individual HIP kernels (through the C ABI) against plain fp32 CPU PyTorch.

Sizes are tiny (the CPU side finishes in seconds) but chosen to hit the edges: row counts that are not a
multiple of the 128-row tile, stride-2 gathers, class counts that are not a multiple of the vector width.
Tolerances: fp32 path 2e-4 relative to the output scale.  bf16 path 8e-3 of max|ref|: the reference inputs are
quantised to bf16 first (``q()``), accumulation is fp32 on both sides, so the only legitimate difference is the ONE
rounding of the output to bf16 (2^-9 = 2e-3 of the value) plus a rare 1-ulp flip of a prologue result; a dropped
32-channel chunk of one tap at K = 2304 is ~2.6e-2 of max and fails.  The 1e-3 logits bar of BASELINE.json applies
to the fp32 path only.
"""
import math

import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from frhip import synth  # noqa: E402


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from frhip import _lib, ops
    _lib.self_check()
    return ops


BF16_TOL = 8e-3
DT = [("f32", torch.float32, 2e-4), ("bf16", torch.bfloat16, BF16_TOL)]


def nhwc(t, dtype):
    """NCHW cpu tensor -> NHWC contiguous device tensor of dtype."""
    return t.permute(0, 2, 3, 1).contiguous().to("cuda", dtype)


def from_nhwc(t):
    return t.float().cpu().permute(0, 3, 1, 2).contiguous()


def pack_w(w, dtype):
    """OIHW -> [O][kh*kw][I] device"""
    o, i, kh, kw = w.shape
    return w.permute(0, 2, 3, 1).reshape(o, kh * kw, i).contiguous().to("cuda", dtype)


def relerr(a, b):
    return float((a - b).abs().max() / (b.abs().max() + 1e-12))


def q(t, dtype):
    """Quantise reference inputs the way the device sees them."""
    return t.to(dtype).float()


@pytest.mark.parametrize("name,dtype,tol", DT)
@pytest.mark.parametrize("cin,cout,stride,ksz", [(64, 64, 1, 3), (64, 128, 2, 3), (128, 64, 1, 3), (64, 128, 2, 1),
                                                 (32, 64, 1, 1)])
@pytest.mark.parametrize("pro", ["none", "bn", "prelu"])
def test_conv_forward(K, name, dtype, tol, cin, cout, stride, ksz, pro):
    B, H = 3, 10  # M = 300 / 75 rows: not a multiple of 128
    pad = 1 if ksz == 3 else 0
    x = q(synth.normal(1, "cx", (B, cin, H, H)), dtype)
    w = q(synth.normal(1, "cw", (cout, cin, ksz, ksz), std=0.1), dtype)
    pa = synth.uniform(1, "pa", (cin,), 0.5, 1.5)
    pb = synth.uniform(1, "pb", (cin,), -0.5, 0.5)
    if pro == "bn":
        xin = x * pa.view(1, -1, 1, 1) + pb.view(1, -1, 1, 1)
    elif pro == "prelu":
        xin = F.prelu(x, pa * 0.25)
    else:
        xin = x
    if dtype == torch.bfloat16:
        xin = q(xin, dtype)
    ref = F.conv2d(xin, w, stride=stride, padding=pad)
    Ho = ref.shape[2]
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    xd, wd = nhwc(x, dtype), pack_w(w, dtype)
    out = torch.zeros(B, Ho, Ho, cout, device="cuda", dtype=dtype)
    mt = (B * Ho * Ho + 127) // 128
    part = torch.zeros(mt, 2, cout, device="cuda")
    a_dev = (pa * 0.25 if pro == "prelu" else pa).cuda()
    K.conv(K.current_stream_ptr(), fr, src=xd, w=wd, out=out, B=B, RH=Ho, RW=Ho, SH=H, SW=H, SC=cin, N=cout, KH=ksz,
           KW=ksz, stride=stride, pad=pad, mode=0, lda=cin, ldc=cout, pro={"none": 0, "bn": 1, "prelu": 2}[pro],
           pro_a=a_dev, pro_b=pb.cuda(), epi=K.EPI_STATS, part=part)()
    torch.cuda.synchronize()
    got = from_nhwc(out)
    assert relerr(got, ref) < tol
    s = part.sum(0).cpu()
    refq = ref if dtype == torch.float32 else ref
    np.testing.assert_allclose(s[0], refq.sum((0, 2, 3)), rtol=tol * 5, atol=tol * 5 * float(ref.abs().sum() / cout))
    np.testing.assert_allclose(s[1], (refq * refq).sum((0, 2, 3)), rtol=tol * 5)


@pytest.mark.parametrize("name,dtype,tol", DT)
@pytest.mark.parametrize("cin,cout,stride,ksz", [(64, 64, 1, 3), (64, 128, 2, 3), (64, 128, 2, 1)])
def test_conv_dgrad(K, name, dtype, tol, cin, cout, stride, ksz):
    B, H = 2, 12
    pad = 1 if ksz == 3 else 0
    x = synth.normal(2, "dx", (B, cin, H, H)).requires_grad_(True)
    w = q(synth.normal(2, "dw", (cout, cin, ksz, ksz), std=0.1), dtype)
    y = F.conv2d(x, w, stride=stride, padding=pad)
    Ho = y.shape[2]
    g = q(synth.normal(2, "dg", tuple(y.shape)), dtype)
    (gx,) = torch.autograd.grad(y, [x], g)
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    # transposed weights [Cin][taps][Cout]
    wt = w.permute(1, 2, 3, 0).reshape(cin, ksz * ksz, cout).contiguous().to("cuda", dtype)
    gd = nhwc(g, dtype)
    out = torch.zeros(B, H, H, cin, device="cuda", dtype=dtype)
    K.conv(K.current_stream_ptr(), fr, src=gd, w=wt, out=out, B=B, RH=H, RW=H, SH=Ho, SW=Ho, SC=cout, N=cin, KH=ksz,
           KW=ksz, stride=stride, pad=pad, mode=1, lda=cout, ldc=cin, pro=0, epi=K.EPI_STORE)()
    torch.cuda.synchronize()
    assert relerr(from_nhwc(out), gx) < tol


@pytest.mark.parametrize("name,dtype,tol", DT)
def test_conv_dgrad_fused_epilogues(K, name, dtype, tol):
    """PReLU-backward and BN-backward-sums epilogues."""
    B, H, C = 2, 9, 64
    g = q(synth.normal(3, "eg", (B, C, H, H)), dtype)
    w = q(synth.normal(3, "ew", (C, C, 3, 3), std=0.1), dtype)
    aux = q(synth.normal(3, "ea", (B, C, H, H)), dtype)
    slope = synth.uniform(3, "es", (C,), 0.1, 0.4)
    mean = synth.uniform(3, "em", (C,), -0.3, 0.3)
    invstd = synth.uniform(3, "ei", (C,), 0.5, 2.0)
    acc = F.conv2d(g, w, padding=1)  # any conv works as the accumulator
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    gd, wd, auxd = nhwc(g, dtype), pack_w(w, dtype), nhwc(aux, dtype)
    mt = (B * H * H + 127) // 128
    for epi in ("prelu", "bnbwd"):
        out = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
        part = torch.zeros(mt, 2, C, device="cuda")
        kw = dict(src=gd, w=wd, out=out, B=B, RH=H, RW=H, SH=H, SW=H, SC=C, N=C, KH=3, KW=3, stride=1, pad=1, mode=0,
                  lda=C, ldc=C, ldaux=C, pro=0, aux=auxd, part=part)
        if epi == "prelu":
            K.conv(K.current_stream_ptr(), fr, epi=K.EPI_PRELU_BWD, epi_a=slope.cuda(), **kw)()
            ref = torch.where(aux > 0, acc, acc * slope.view(1, -1, 1, 1))
            s0 = (acc * aux * (aux <= 0)).sum((0, 2, 3))
            torch.cuda.synchronize()
            assert relerr(from_nhwc(out), ref) < tol
            np.testing.assert_allclose(part.sum(0)[0].cpu(), s0, rtol=tol * 10, atol=tol * 50)
        else:
            K.conv(K.current_stream_ptr(), fr, epi=K.EPI_BNBWD, epi_a=mean.cuda(), epi_b=invstd.cuda(), **kw)()
            xh = (aux - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
            torch.cuda.synchronize()
            assert relerr(from_nhwc(out), acc) < tol
            np.testing.assert_allclose(part.sum(0)[0].cpu(), acc.sum((0, 2, 3)), rtol=tol * 10, atol=tol * 50)
            np.testing.assert_allclose(part.sum(0)[1].cpu(), (acc * xh).sum((0, 2, 3)), rtol=tol * 10, atol=tol * 50)


@pytest.mark.parametrize("name,dtype,tol", DT)
@pytest.mark.parametrize("cin,cout,stride,ksz", [(64, 64, 1, 3), (64, 128, 2, 3), (128, 128, 1, 3), (64, 128, 2, 1),
                                                 (32, 64, 1, 1), (256, 128, 1, 3)])
@pytest.mark.parametrize("pro", ["none", "bn", "prelu"])
@pytest.mark.parametrize("nsplit", [1, 3])
def test_conv_wgrad(K, name, dtype, tol, cin, cout, stride, ksz, pro, nsplit):
    B, H = 2, 10
    pad = 1 if ksz == 3 else 0
    x = q(synth.normal(4, "wx", (B, cin, H, H)), dtype)
    pa = synth.uniform(4, "wpa", (cin,), 0.5, 1.5)
    pb = synth.uniform(4, "wpb", (cin,), -0.5, 0.5)
    if pro == "bn":
        xin = x * pa.view(1, -1, 1, 1) + pb.view(1, -1, 1, 1)
    elif pro == "prelu":
        xin = F.prelu(x, pa * 0.25)
    else:
        xin = x
    if dtype == torch.bfloat16:
        xin = q(xin, dtype)
    w = synth.normal(4, "ww", (cout, cin, ksz, ksz), std=0.1).requires_grad_(True)
    y = F.conv2d(xin, w, stride=stride, padding=pad)
    Ho = y.shape[2]
    g = q(synth.normal(4, "wg", tuple(y.shape)), dtype)
    (gw,) = torch.autograd.grad(y, [w], g)
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    dw = torch.zeros(cout, ksz * ksz, cin, device="cuda")
    a_dev = (pa * 0.25 if pro == "prelu" else pa).cuda()
    K.wgrad(K.current_stream_ptr(), fr, g=nhwc(g, dtype), src=nhwc(x, dtype), dw=dw, B=B, GH=Ho, GW=Ho, Cout=cout,
            SH=H, SW=H, SC=cin, KH=ksz, KW=ksz, stride=stride, pad=pad, ldg=cout, lda=cin,
            pro={"none": 0, "bn": 1, "prelu": 2}[pro], nsplit=nsplit, pro_a=a_dev, pro_b=pb.cuda())()
    torch.cuda.synchronize()
    got = dw.cpu().reshape(cout, ksz, ksz, cin).permute(0, 3, 1, 2)
    assert relerr(got, gw) < tol


@pytest.mark.parametrize("name,dtype,tol", DT)
def test_gemm_bias_and_splitk(K, name, dtype, tol):
    """Dense rows x K GEMM (Linear / head shapes), N not a multiple of 8, split-K atomics onto a bias seed."""
    M, Kd, N = 37, 512, 100
    a = q(synth.normal(5, "ga", (M, Kd)), dtype)
    w = q(synth.normal(5, "gw", (N, Kd), std=0.1), dtype)
    bias = synth.normal(5, "gb", (N,))
    ref = a @ w.t() + bias
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    ad, wd = a.to("cuda", dtype), w.to("cuda", dtype)
    out = torch.zeros(M, N, device="cuda")
    st = K.current_stream_ptr()
    kw = dict(src=ad, w=wd, B=M, RH=1, RW=1, SH=1, SW=1, SC=Kd, N=N, KH=1, KW=1, stride=1, pad=0, mode=0, lda=Kd,
              ldc=N, pro=0, out_f32=1)
    K.conv(st, fr, out=out, epi=K.EPI_STORE, bias=bias.cuda(), **kw)()
    torch.cuda.synchronize()
    assert relerr(out.cpu(), ref) < tol
    out2 = torch.empty(M, N, device="cuda")
    K.call("fr_fill_rows", out2, bias.cuda(), M, N, st)()
    K.conv(st, fr, out=out2, epi=K.EPI_ATOMIC, splitk=4, **kw)()
    torch.cuda.synchronize()
    assert relerr(out2.cpu(), ref) < tol


def test_margin_head_matches_golden(K, golden_dir):
    """ArcFace / CosFace logits + gradients on the reference's own vectors (g1_head), fp32 path.
    Label select must be exact: the margin lands on exactly the label column of every row."""
    import os
    from oracle import irse_ref as O
    g = np.load(os.path.join(golden_dir, "g1_head.npz"))
    from head.metrics import ArcFace, CosFace
    for kind, cls in (("ArcFace", ArcFace), ("CosFace", CosFace)):
        head = cls(512, 100, None).cuda()
        with torch.no_grad():
            head.weight.copy_(torch.from_numpy(g["w"]))
        x = torch.from_numpy(g["x"]).cuda().requires_grad_(True)
        label = torch.from_numpy(g["label"]).cuda()
        y = head(x, label)
        ref = torch.from_numpy(g[kind + ".logits"])
        got = y.detach().cpu()
        diff = (got - ref).abs()
        # Two label entries of the fixture are ill-conditioned *in the reference itself* (ArcFace only):
        #   row 4: cos = +1 -> sine = sqrt(clamp(1-cos^2)) turns a 1-ulp cosine difference into ~1e-2 logits
        #   row 6: cos = th exactly -> the where(cos > th) branch is decided by the last bit (7.5 logits apart)
        # Everything else must meet the 1e-3 north-star bar.
        loose = torch.zeros(8, 100, dtype=torch.bool)
        if kind == "ArcFace":
            loose[4, 13] = loose[6, 34] = True
        assert float(diff[~loose].max()) < 1e-3
        if kind == "ArcFace":
            assert float(diff[4, 13]) < 0.1
            c6 = float(O.cosine_logits(torch.from_numpy(g["x"]), torch.from_numpy(g["w"]))[6, 34])
            cm, sm, th, mm = O.arcface_constants(0.5)
            branches = (64 * (c6 * cm - math.sqrt(max(1 - c6 * c6, 1e-10)) * sm), 64 * (c6 - mm))
            assert min(abs(float(got[6, 34]) - b) for b in branches) < 1e-2
        # bit-exact scatter: the set of positions where logits differ from s*cos is exactly the label set
        cos = O.cosine_logits(torch.from_numpy(g["x"]), torch.from_numpy(g["w"])) * 64.0
        mask = (got - cos).abs() > 1e-2
        onehot = torch.zeros(8, 100, dtype=torch.bool).scatter_(1, torch.from_numpy(g["label"]).view(-1, 1), True)
        assert torch.equal(mask, onehot)
        y.backward(torch.from_numpy(g["gout"]).cuda())
        rows = [0, 1, 2, 3, 5, 7] if kind == "ArcFace" else list(range(8))
        np.testing.assert_allclose(x.grad.cpu()[rows], g[kind + ".gx"][rows], atol=2e-3, rtol=2e-3)
        cls_ok = [c for c in range(100) if kind != "ArcFace" or c not in (13, 34)]
        gw_got, gw_ref = head.weight.grad.cpu(), torch.from_numpy(g[kind + ".gw"])
        np.testing.assert_allclose(gw_got[cls_ok], gw_ref[cls_ok], atol=5e-2 if kind == "ArcFace" else 2e-3,
                                   rtol=5e-2 if kind == "ArcFace" else 2e-3)


def test_margin_head_backward_vs_oracle(K):
    """Well-conditioned head case (random features, N = 1000 not a multiple of 128): logits and both gradients
    against the CPU oracle; 1e-3 abs on logits, 1e-3 rel on gradients."""
    from oracle import irse_ref as O
    from head.metrics import ArcFace, CosFace
    B, N = 37, 1000
    x0 = synth.normal(21, "hx", (B, 512))
    w0 = synth.uniform(21, "hw", (N, 512), -0.1, 0.1)
    label = synth.labels(21, "hl", B, N)
    gout = synth.normal(21, "hg", (B, N))
    for kind, cls, f in (("ArcFace", ArcFace, O.arcface_forward), ("CosFace", CosFace, O.cosface_forward)):
        xr, wr = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        yr = f(xr, wr, label)
        gxr, gwr = torch.autograd.grad(yr, [xr, wr], gout)
        head = cls(512, N, None).cuda()
        with torch.no_grad():
            head.weight.copy_(w0)
        x = x0.cuda().requires_grad_(True)
        y = head(x, label.cuda())
        assert float((y.detach().cpu() - yr.detach()).abs().max()) < 1e-3
        y.backward(gout.cuda())
        assert relerr(x.grad.cpu(), gxr) < 1e-3
        assert relerr(head.weight.grad.cpu(), gwr) < 1e-3


@pytest.mark.parametrize("rows,dt", [(100, "f32"), (1000, "f32"), (7000, "f32"), (28000, "f32"), (1000, "bf16"), (333, "bf16")])
def test_row_normalize_and_transposed_copy(K, rows, dt):
    """F.normalize rows (eps 1e-12, head/metrics.py:103) + the zero-padded transposed copy the head GEMMs read; padded
    row counts below / above the tiled-transpose threshold, both dtypes."""
    from frhip._lib import FR_BF16, FR_F32
    ops = K
    D = 512
    pad = (rows + 31) // 32 * 32
    x = synth.normal(51, "rn", (rows, D))
    x[3] = 0.0  # a zero row: 0 / max(0, eps) = 0
    tdt = torch.float32 if dt == "f32" else torch.bfloat16
    xn = torch.full((pad, D), 7.0, device="cuda", dtype=tdt)
    xt = torch.full((D, pad), 7.0, device="cuda", dtype=tdt)
    inv = torch.empty(rows, device="cuda")
    ops.call("fr_row_normalize", x.cuda(), xn, xt, inv, rows, pad, D, pad, FR_F32 if dt == "f32" else FR_BF16,
             ops.current_stream_ptr())()
    ref = torch.nn.functional.normalize(x)
    tol = 1e-6 if dt == "f32" else 4e-3
    assert float((xn[:rows].float().cpu() - ref).abs().max()) <= tol
    assert bool((xn[rows:] == 0).all()) and bool((xt[:, rows:] == 0).all())
    assert torch.equal(xt, xn.t().contiguous())
    nrm = x.norm(dim=1).clamp_min(1e-12)
    torch.testing.assert_close(inv.cpu(), 1.0 / nrm, rtol=1e-6, atol=0)


def test_margin_head_easy_margin_and_custom_scale(K, golden_dir):
    """ArcFace(s=30, m=0.35, easy_margin=True) (head/metrics.py:120-121: phi where cos > 0, cos elsewhere) and
    CosFace(s=30, m=0.35): logits against the reference's own vector where the fixture has one, gradients against the
    oracle; includes rows on both sides of the easy-margin switch."""
    import os
    from oracle import irse_ref as O
    from head.metrics import ArcFace, CosFace
    g = np.load(os.path.join(golden_dir, "g1_head.npz"))
    head = ArcFace(512, 100, None, s=30.0, m=0.35, easy_margin=True).cuda()
    with torch.no_grad():
        head.weight.copy_(torch.from_numpy(g["w"]))
    x = torch.from_numpy(g["x"]).cuda()
    label = torch.from_numpy(g["label"]).cuda()
    got = head(x, label).cpu()
    ref = torch.from_numpy(g["ArcFace.easy.logits"])
    loose = torch.zeros_like(ref, dtype=torch.bool)
    loose[4, 13] = True  # cos = +1: sqrt of a clamped difference, ill-conditioned in the reference itself
    assert float((got - ref).abs()[~loose].max()) < 1e-3 and float((got - ref).abs()[4, 13]) < 0.1
    # random case with negative label cosines too (easy margin leaves those rows untouched)
    B, N = 29, 203
    x0 = synth.normal(31, "ex", (B, 512))
    w0 = synth.uniform(31, "ew", (N, 512), -0.1, 0.1)
    lab = synth.labels(31, "el", B, N)
    with torch.no_grad():
        cos = O.cosine_logits(x0, w0)
    sel = cos[torch.arange(B), lab]
    assert bool((sel > 0).any()) and bool((sel < 0).any())
    gout = synth.normal(31, "eg", (B, N))
    for cls, f, kw in ((ArcFace, O.arcface_forward, dict(s=30.0, m=0.35, easy_margin=True)),
                       (CosFace, O.cosface_forward, dict(s=30.0, m=0.35))):
        xr, wr = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
        yr = f(xr, wr, lab, **kw)
        gxr, gwr = torch.autograd.grad(yr, [xr, wr], gout)
        h = cls(512, N, None, **kw).cuda()
        with torch.no_grad():
            h.weight.copy_(w0)
        xg = x0.cuda().requires_grad_(True)
        y = h(xg, lab.cuda())
        assert float((y.detach().cpu() - yr.detach()).abs().max()) < 1e-3
        y.backward(gout.cuda())
        assert relerr(xg.grad.cpu(), gxr) < 1e-3 and relerr(h.weight.grad.cpu(), gwr) < 1e-3


@pytest.mark.parametrize("gamma", [0.0, 1.0, 2.0, 3.5])
def test_focal_loss_other_gammas(K, gamma):
    """FocalLoss(gamma) for gamma != 2 (loss/focal.py:9-21; gamma = 0 is plain mean cross entropy): value and gradient
    against the oracle, N not a multiple of the vector width, a row whose label has the largest logit."""
    from oracle import irse_ref as O
    from loss.focal import FocalLoss
    B, N = 19, 333
    z0 = synth.normal(41, "fz", (B, N)) * 3.0
    y = synth.labels(41, "fy", B, N)
    z0[0, y[0]] = 50.0
    zr = z0.clone().requires_grad_(True)
    lr = O.focal_loss(zr, y, gamma)
    gr, = torch.autograd.grad(lr, [zr])
    z = z0.cuda().requires_grad_(True)
    loss, extra = FocalLoss(gamma=gamma)(z, y.cuda())
    loss.backward()
    assert extra is None
    assert abs(float(loss.detach()) - float(lr)) < 1e-5 * max(1.0, abs(float(lr)))
    assert relerr(z.grad.cpu(), gr) < 1e-4


def test_focal_and_accuracy_match_golden(K, golden_dir):
    import os
    g = np.load(os.path.join(golden_dir, "g2_focal.npz"))
    from loss.focal import FocalLoss
    from util.utils import accuracy
    logits = torch.from_numpy(g["logits"]).cuda().requires_grad_(True)
    label = torch.from_numpy(g["label"]).cuda()
    loss, aux = FocalLoss()(logits, label)
    assert aux is None
    assert abs(float(loss.detach()) - float(g["loss"])) < 1e-5 * max(1.0, abs(float(g["loss"])))
    loss.backward()
    np.testing.assert_allclose(logits.grad.cpu(), g["grad"], atol=1e-6, rtol=1e-4)
    p1, p5 = accuracy(logits.data, label, topk=(1, 5))
    assert float(p1) == float(g["prec1"]) and float(p5) == float(g["prec5"])


def test_sgd_matches_torch(K):
    from frhip.optim import SGD
    torch.manual_seed(0)
    ps = [torch.nn.Parameter(synth.normal(6, "p%d" % i, shp).cuda()) for i, shp in
          enumerate([(5000,), (64, 3, 3, 3), (7,), (300, 40)])]
    ref = [torch.nn.Parameter(p.detach().cpu().clone()) for p in ps]
    opt = SGD([{"params": ps[:2], "weight_decay": 2e-3}, {"params": ps[2:]}], lr=0.03, momentum=0.9)
    ropt = torch.optim.SGD([{"params": ref[:2], "weight_decay": 2e-3}, {"params": ref[2:]}], lr=0.03, momentum=0.9)
    for step in range(3):
        for i, (p, r) in enumerate(zip(ps, ref)):
            gr = synth.normal(7, "g%d.%d" % (i, step), tuple(p.shape))
            p.grad = gr.cuda()
            r.grad = gr.clone()
        opt.step()
        ropt.step()
    for p, r in zip(ps, ref):
        np.testing.assert_allclose(p.detach().cpu(), r.detach(), rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("name,dtype,tol", DT)
def test_bn_apply_and_backward(K, name, dtype, tol):
    """BN statistics -> apply (+PReLU +identity shortcut) -> backward, vs autograd on CPU."""
    B, H, C, s = 2, 8, 64, 2
    x = q(synth.normal(8, "bx", (B, C, H, H)), dtype).requires_grad_(True)
    res = q(synth.normal(8, "br", (B, C, H * s, H * s)), dtype)
    gamma = synth.uniform(8, "bg", (C,), 0.8, 1.2).requires_grad_(True)
    beta = synth.uniform(8, "bb", (C,), -0.1, 0.1).requires_grad_(True)
    rm, rv = torch.zeros(C), torch.ones(C)
    y = F.batch_norm(x, rm, rv, gamma, beta, True, 0.1, 1e-5) + res[:, :, ::s, ::s]
    g = q(synth.normal(8, "bgo", tuple(y.shape)), dtype)
    gx, gg, gb = torch.autograd.grad(y, [x, gamma, beta], g)
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    st = K.current_stream_ptr()
    xd = nhwc(x.detach(), dtype)
    rows = B * H * H
    nb = K.grid_blocks(rows, C, fr)
    part = torch.zeros(nb, 2, C, device="cuda")
    K.call("fr_channel_stats", xd, rows, C, part, nb, fr, st)()
    mean, invstd, scale, shift = (torch.zeros(C, device="cuda") for _ in range(4))
    rmd, rvd, nbt = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda"), torch.zeros((), dtype=torch.int64,
                                                                                              device="cuda")
    K.call("fr_bn_finalize", part, nb, C, float(rows), gamma.detach().cuda(), beta.detach().cuda(), 1e-5, 0.1, rmd,
           rvd, nbt, mean, invstd, scale, shift, st)()
    out = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
    part2 = torch.zeros(nb, 2, C, device="cuda")
    K.bn_apply(st, fr, x=xd, out=out, scale=scale, shift=shift, res=nhwc(res, dtype), part=part2, B=B, H=H, W=H, C=C,
               res_kind=1, res_stride=s, nblocks=nb)()
    torch.cuda.synchronize()
    assert relerr(from_nhwc(out), y.detach()) < tol
    np.testing.assert_allclose(rmd.cpu(), rm, atol=1e-4)
    np.testing.assert_allclose(rvd.cpu(), rv, atol=1e-3)
    assert int(nbt) == 1
    np.testing.assert_allclose(part2.sum(0)[0].cpu(), from_nhwc(out).sum((0, 2, 3)), rtol=1e-3, atol=1e-2)
    # backward
    gd = nhwc(g, dtype)
    part3 = torch.zeros(nb, 3, C, device="cuda")
    common = dict(g=gd, x=xd, mean=mean, invstd=invstd, rows=rows, C=C, rows_per_image=H * H, nblocks=nb)
    K.bn_bwd_reduce(st, fr, part=part3, **common)()
    s0, s1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    K.call("fr_reduce_parts", part3, nb, 3, C, s0, s1, None, st)()
    gxd = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
    K.bn_bwd_apply(st, fr, gx=gxd, gamma=gamma.detach().cuda(), s0=s0, s1=s1, inv_count=1.0 / rows, **common)()
    torch.cuda.synchronize()
    np.testing.assert_allclose(s0.cpu(), gb, rtol=tol * 5, atol=tol * 20)
    np.testing.assert_allclose(s1.cpu(), gg, rtol=tol * 5, atol=tol * 20)
    assert relerr(from_nhwc(gxd), gx) < tol * 2


@pytest.mark.parametrize("C,H", [(64, 9), (128, 5), (512, 3)])
@pytest.mark.parametrize("res_kind", [0, 1, 2])
def test_bn_lean_bf16_variants(K, C, H, res_kind):
    """The 4-channel x 4-row bf16 kernels (same-geometry shortcut, folded shortcut BN, add in the backward) on row
    counts that are not a multiple of the rows in flight, against the same arithmetic in fp32 on the CPU."""
    dtype, tol = torch.bfloat16, BF16_TOL
    B = 3
    rows = B * H * H
    x = q(synth.normal(21, "lx", (B, C, H, H)), dtype)
    res = q(synth.normal(21, "lr", (B, C, H, H)), dtype)
    scale, shift = synth.uniform(21, "ls", (C,), 0.5, 1.5), synth.uniform(21, "lh", (C,), -0.2, 0.2)
    rscale, rshift = synth.uniform(21, "lrs", (C,), 0.5, 1.5), synth.uniform(21, "lrh", (C,), -0.2, 0.2)
    v = lambda t: t.view(1, C, 1, 1)  # noqa: E731
    y = x * v(scale) + v(shift)
    if res_kind == 1:
        y = y + res
    elif res_kind == 2:
        y = y + (res * v(rscale) + v(rshift))
    fr, st = K.fr_dtype(torch.empty(0, dtype=dtype)), K.current_stream_ptr()
    nb = 7
    out = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
    part = torch.zeros(nb, 2, C, device="cuda")
    kw = dict(x=nhwc(x, dtype), out=out, scale=scale.cuda(), shift=shift.cuda(), part=part, B=B, H=H, W=H, C=C,
              res_kind=res_kind, res_stride=1, nblocks=nb)
    if res_kind:
        kw["res"] = nhwc(res, dtype)
    if res_kind == 2:
        kw.update(rscale=rscale.cuda(), rshift=rshift.cuda())
    K.bn_apply(st, fr, **kw)()
    torch.cuda.synchronize()
    assert relerr(from_nhwc(out), y) < tol
    o32 = from_nhwc(out)
    np.testing.assert_allclose(part.sum(0)[0].cpu(), o32.sum((0, 2, 3)), rtol=1e-3, atol=1e-2)
    np.testing.assert_allclose(part.sum(0)[1].cpu(), (o32 * o32).sum((0, 2, 3)), rtol=1e-3, atol=1e-2)
    # backward of a training-mode BN on x, with the shortcut gradient added (add_kind 1) when res_kind != 0
    xg = x.clone().requires_grad_(True)
    gamma = synth.uniform(21, "lg", (C,), 0.8, 1.2).requires_grad_(True)
    beta = torch.zeros(C, requires_grad=True)
    z = F.batch_norm(xg, None, None, gamma, beta, True, 0.1, 1e-5)
    g = q(synth.normal(21, "lgo", tuple(z.shape)), dtype)
    gx, gg, gb = torch.autograd.grad(z, [xg, gamma, beta], g)
    if res_kind:
        gx = gx + res
    mean = x.mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(x.var((0, 2, 3), unbiased=False) + 1e-5)
    common = dict(g=nhwc(g, dtype), x=nhwc(x, dtype), mean=mean.cuda(), invstd=invstd.cuda(), rows=rows, C=C,
                  rows_per_image=H * H, nblocks=nb)
    part3 = torch.zeros(nb, 3, C, device="cuda")
    K.bn_bwd_reduce(st, fr, part=part3, **common)()
    s0, s1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    K.call("fr_reduce_parts", part3, nb, 3, C, s0, s1, None, st)()
    gxd = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
    extra = dict(add=nhwc(res, dtype), add_kind=1) if res_kind else {}
    K.bn_bwd_apply(st, fr, gx=gxd, gamma=gamma.detach().cuda(), s0=s0, s1=s1, inv_count=1.0 / rows, **common, **extra)()
    torch.cuda.synchronize()
    np.testing.assert_allclose(s0.cpu(), gb, rtol=tol * 5, atol=tol * 20)
    np.testing.assert_allclose(s1.cpu(), gg, rtol=tol * 5, atol=tol * 20)
    assert relerr(from_nhwc(gxd), gx) < tol * 2


@pytest.mark.parametrize("nparts", [1, 5, 130, 1024, 3000])
def test_partial_sum_reductions_are_exact_in_double(K, nparts):
    """fr_bn_finalize / fr_reduce_parts over many partial rows == float64 column sums."""
    C = 72  # not a multiple of the 8 columns a workgroup owns * anything special; exercises the column guard
    part = synth.normal(23, "pp%d" % nparts, (nparts, 3, C)).abs() + 0.5
    pd = part.cuda()
    st = K.current_stream_ptr()
    o = [torch.zeros(C, device="cuda") for _ in range(3)]
    K.call("fr_reduce_parts", pd, nparts, 3, C, o[0], o[1], o[2], st)()
    ref = part.double().sum(0)
    for k in range(3):
        np.testing.assert_allclose(o[k].cpu().double(), ref[k], rtol=2e-7)
    count = 1000.0 * nparts
    p2 = pd[:, :2].contiguous()
    p2[:, 1] += 4.0 * nparts  # keep the variance positive
    mean, invstd, scale, shift = (torch.zeros(C, device="cuda") for _ in range(4))
    K.call("fr_bn_finalize", p2, nparts, C, count, None, None, 1e-5, 0.1, None, None, None, mean, invstd, scale, shift,
           st)()
    torch.cuda.synchronize()
    s = p2.cpu().double().sum(0)
    m = s[0] / count
    var = s[1] / count - m * m
    np.testing.assert_allclose(mean.cpu().double(), m, rtol=1e-6)
    np.testing.assert_allclose(invstd.cpu().double(), 1.0 / torch.sqrt(var + 1e-5), rtol=1e-6)


@pytest.mark.parametrize("name,dtype,tol", DT)
def test_permute_linear_layouts(K, name, dtype, tol):
    """Linear(C*HW, O) weight: torch [O][C*HW] -> packed [O][HW*C] and its transpose; gradient back (dir 1)."""
    O, C, HW = 70, 128, 49
    w = q(synth.normal(25, "plw", (O, C * HW)), dtype)
    fr, st = K.fr_dtype(torch.empty(0, dtype=dtype)), K.current_stream_ptr()
    out = torch.zeros(O, HW * C, device="cuda", dtype=dtype)
    wt = torch.zeros(HW * C, O, device="cuda", dtype=dtype)
    K.call("fr_permute_linear", w.cuda(), out, wt, O, C, HW, 0, fr, st)()
    ref = w.view(O, C, HW).permute(0, 2, 1).reshape(O, HW * C)
    torch.cuda.synchronize()
    assert torch.equal(out.float().cpu(), ref)
    assert torch.equal(wt.float().cpu(), ref.t())
    g = synth.normal(25, "plg", (O, HW * C))
    gout = torch.zeros(O, C * HW, device="cuda")
    K.call("fr_permute_linear", g.cuda(), gout, None, O, C, HW, 1, K.FR_F32, st)()
    torch.cuda.synchronize()
    assert torch.equal(gout.cpu(), g.view(O, HW, C).permute(0, 2, 1).reshape(O, C * HW))


STRIP_SHAPES = [(64, 64, 112), (64, 64, 56), (64, 128, 56), (128, 64, 56), (128, 128, 28), (128, 256, 28),
                (256, 128, 28), (256, 256, 14), (256, 512, 14), (512, 256, 14), (512, 512, 7)]


# B = 3: every shape of the dispatch table; (512, 512, 7, B): B = 4 / 6 -> two images per workgroup at 7x7, output channels
# over four workgroups (256 resident channels, two channel stages: the small-batch instance, B <= 160), B = 164 -> four
# images per workgroup (128 resident channels, four stages: the instance bench.py's B = 256 runs), 41 strips;
# B = 162 (> 160, even): the instances bench.py's B = 256 step runs -- conv3x3_strip_kernel<256,256,14,14,8,8,1,...>
# (NSPL = 1, the kernel ``roofline.kernel`` names; B <= 160 takes the split-channel NSPL = 2 instance) and the
# 256 -> 512 two-pass path built on it -- against CPU F.conv2d / autograd (~40 GFLOP on the host)
# 64 -> 64 (rolling-window kernel, conv3x3_roll64.hip): B = 3 walks 2-iteration row segments (14 per band); B = 162 @56
# and B = 130 @112 give more work items than the 256 persistent workgroups (item loop, one 14- / 28-iteration walk per
# item); B = 40 @56 takes 7-iteration segments
STRIP_CASES = [s + (3,) for s in STRIP_SHAPES] + [(512, 512, 7, 4), (512, 512, 7, 6), (512, 512, 7, 164),
                                                  (256, 256, 14, 162), (256, 512, 14, 162),
                                                  (64, 64, 56, 162), (64, 64, 112, 130), (64, 64, 56, 40)]


def _image_subset(B):
    """Images whose results are compared with the CPU reference: all of them up to 32; beyond that three blocks (the first 8, 8
    in the middle, the last 8-11, block starts multiples of 4 so that a block is whole partial rows of the multi-image 7x7
    workgroups).  A convolution is independent per image and the large-batch cases exist for the workgroup / item geometry:
    every image is still computed by the kernel, the host just stops convolving 130-164 of them at 112x112 (22 s per case)."""
    if B <= 32:
        return list(range(B))
    mid = (B // 2) // 8 * 8
    return list(range(8)) + list(range(mid, mid + 8)) + list(range((B - 8) // 4 * 4, B))


def _operand(B, sel, seed, tag, shape, dtype):
    """A quantised NCHW activation as (CPU fp32 tensor of the images `sel`, device NHWC tensor of all images).  Up to 32 images
    it comes from the repo's counter-based generator; the large-batch cases draw it on the device (104 M elements per tensor at
    112x112 x 130 images took the host generator 3 s each) and copy the subset back."""
    if B <= 32:
        t = q(synth.normal(seed, tag, shape), dtype)
        return t[sel], nhwc(t, dtype)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(seed * 1000 + sum((i + 1) * ord(c) for i, c in enumerate(tag)))
    t = torch.randn(shape, device="cuda", generator=gen).to(dtype)
    return t[sel].float().cpu(), t.permute(0, 2, 3, 1).contiguous()


def _part_rows(nparts, B, sel):
    """Partial rows that belong to the images `sel` (rows are image-major: whole strips / items of one image, or -- 7x7 -- one
    row per group of 2 / 4 consecutive images)."""
    if nparts % B == 0:
        rpi = nparts // B
        return [r for b in sel for r in range(b * rpi, (b + 1) * rpi)]
    assert B % nparts == 0
    ipr = B // nparts
    rows = sorted({b // ipr for b in sel})
    assert all(b in sel for r in rows for b in range(r * ipr, (r + 1) * ipr))
    return rows


def _assert_all_part_rows_match_the_stored_output(part, out, what):
    """Device-side check over ALL part rows and ALL images: the sum of the rows' first vector (taken from the fp32 accumulators,
    before the bf16 store) against the per-channel sum of the kernel's own stored output.  The bar is derived, not measured:
    the two differ by ONE bf16 rounding per element (2^-9 relative, round to nearest) plus the fp32 summation error of the
    n elements one part row adds (n * 2^-24 relative; the rows themselves are added in float64):
    |difference| <= (2^-9 + n * 2^-24) * sum |out| per channel."""
    o = out.double().reshape(-1, out.shape[-1])
    n = -(-o.shape[0] // part.shape[0])
    bound = (2.0 ** -9 + n * 2.0 ** -24) * o.abs().sum(0)
    diff = (part.double().sum(0)[0] - o.sum(0)).abs()
    assert bool((diff <= bound).all()), "%s: all part rows vs the stored output: worst %.3g of the bound" % (
        what, float((diff / bound.clamp_min(1e-30)).max()))


@pytest.mark.parametrize("cin,cout,W,B", STRIP_CASES, ids=["%d_%d_%d_b%d" % s for s in STRIP_CASES])
def test_conv3x3_strip(K, cin, cout, W, B):
    """LDS-resident-strip 3x3 s1 conv (bf16): forward with BN prologue + statistics, and the mirrored-tap data
    gradient with the PReLU-backward and BN-backward epilogues, every shape of its dispatch table (B = 3; the 7x7
    stage also with an even batch, which takes the two-images-per-workgroup / split-channel instance)."""
    dtype, tol = torch.bfloat16, BF16_TOL
    assert K.strip_parts(B, cin, cout, W) > 0
    st = K.current_stream_ptr()
    sel = _image_subset(B)
    xs, xd = _operand(B, sel, 31, "sx", (B, cin, W, W), dtype)
    w = q(synth.normal(31, "sw", (cout, cin, 3, 3), std=0.05), dtype)
    pa = synth.uniform(31, "spa", (cin,), 0.5, 1.5)
    pb = synth.uniform(31, "spb", (cin,), -0.5, 0.5)
    # the kernel's prologue is one fmaf: form the reference product-sum in double so that it is rounded once, too
    xin = q((xs.double() * pa.double().view(1, -1, 1, 1) + pb.double().view(1, -1, 1, 1)).float(), dtype)
    ref = F.conv2d(xin, w, padding=1)
    out = torch.zeros(B, W, W, cout, device="cuda", dtype=dtype)
    nparts = K.strip_parts(B, cin, cout, W)
    part = torch.zeros(nparts, 2, cout, device="cuda")
    common = dict(B=B, RH=W, RW=W, SH=W, SW=W, KH=3, KW=3, stride=1, pad=1)
    store_only = (cin, cout, W) == (256, 512, 14)  # served as two 256-channel passes, plain store epilogue only
    K.conv_strip(st, src=xd, w=pack_w(w, dtype), out=out, SC=cin, N=cout, mode=0, lda=cin, ldc=cout, pro=K.PRO_BN,
                 pro_a=pa.cuda(), pro_b=pb.cuda(), epi=K.EPI_STORE if store_only else K.EPI_STATS, part=part,
                 **common)()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all()
    assert relerr(from_nhwc(out[sel]), ref) < tol
    if not store_only:
        s = part[_part_rows(nparts, B, sel)].sum(0).cpu()
        np.testing.assert_allclose(s[0], ref.sum((0, 2, 3)), rtol=1e-2, atol=1e-2 * float(ref.abs().sum() / cout))
        np.testing.assert_allclose(s[1], (ref * ref).sum((0, 2, 3)), rtol=1e-2)
        _assert_all_part_rows_match_the_stored_output(part, out, "forward")
    # data gradient: g [B, cout, W, W] -> gx [B, cin, W, W] with weights given as [cin][tap][cout]
    gs_, gd = _operand(B, sel, 31, "sg", (B, cout, W, W), dtype)
    xg = synth.normal(31, "sxx", (len(sel), cin, W, W)).requires_grad_(True)
    (gx,) = torch.autograd.grad(F.conv2d(xg, w, padding=1), [xg], gs_)
    wt = w.permute(1, 2, 3, 0).reshape(cin, 9, cout).contiguous().to("cuda", dtype)
    auxs, auxd = _operand(B, sel, 31, "sa", (B, cin, W, W), dtype)
    slope = synth.uniform(31, "ss", (cin,), 0.1, 0.4)
    mean = synth.uniform(31, "sm", (cin,), -0.3, 0.3)
    invstd = synth.uniform(31, "si", (cin,), 0.5, 2.0)
    nparts = K.strip_parts(B, cout, cin, W, K.EPI_BNBWD)
    if nparts == 0:
        return
    for epi in ("prelu", "bnbwd"):
        o = torch.zeros(B, W, W, cin, device="cuda", dtype=dtype)
        part = torch.zeros(nparts, 2, cin, device="cuda")
        kw = dict(src=gd, w=wt, out=o, SC=cout, N=cin, mode=1, lda=cout, ldc=cin, ldaux=cin, pro=0, aux=auxd, part=part,
                  **common)
        if epi == "prelu":
            K.conv_strip(st, epi=K.EPI_PRELU_BWD, epi_a=slope.cuda(), **kw)()
            torch.cuda.synchronize()
            want = torch.where(auxs > 0, gx, gx * slope.view(1, -1, 1, 1))
            assert torch.isfinite(o.float()).all() and relerr(from_nhwc(o[sel]), want) < tol
            ps = part[_part_rows(nparts, B, sel)].sum(0)
            np.testing.assert_allclose(ps[0].cpu(), (gx * auxs * (auxs <= 0)).sum((0, 2, 3)), rtol=1e-2,
                                       atol=1e-2 * float((gx * auxs).abs().sum() / cin))
        else:
            K.conv_strip(st, epi=K.EPI_BNBWD, epi_a=mean.cuda(), epi_b=invstd.cuda(), **kw)()
            torch.cuda.synchronize()
            xh = (auxs - mean.view(1, -1, 1, 1)) * invstd.view(1, -1, 1, 1)
            assert torch.isfinite(o.float()).all() and relerr(from_nhwc(o[sel]), gx) < tol
            ps = part[_part_rows(nparts, B, sel)].sum(0)
            np.testing.assert_allclose(ps[0].cpu(), gx.sum((0, 2, 3)), rtol=1e-2,
                                       atol=1e-2 * float(gx.abs().sum() / cin))
            np.testing.assert_allclose(ps[1].cpu(), (gx * xh).sum((0, 2, 3)), rtol=1e-2,
                                       atol=1e-2 * float((gx * xh).abs().sum() / cin))
            _assert_all_part_rows_match_the_stored_output(part, o, "data gradient (BNBWD)")




def to_frag(w):
    """[N][taps][K] -> MFMA-fragment order [N / 16][taps][K / 32][64 lanes = (k % 32) / 8 * 16 + n % 16][8] (FrConvArgs.w_frag)."""
    N, taps, Kc = w.shape
    return w.view(N // 16, 16, taps, Kc // 32, 4, 8).permute(0, 2, 3, 4, 1, 5).contiguous()


FRAG_CASES = [(256, 256, 14, 5), (256, 256, 14, 200), (128, 128, 28, 3), (64, 128, 56, 3), (128, 64, 56, 2), (128, 256, 28, 3),
              (256, 128, 28, 3), (256, 512, 14, 3), (512, 256, 14, 3), (512, 512, 7, 3), (512, 512, 7, 6), (512, 512, 7, 8),
              (512, 512, 7, 200)]


@pytest.mark.parametrize("cin,cout,W,B", FRAG_CASES, ids=["%d_%d_%d_b%d" % s for s in FRAG_CASES])
def test_conv3x3_strip_fragment_order_weights(K, cin, cout, W, B):
    """FrConvArgs.w_frag (round 6): the same launch with the weights in MFMA-fragment order -- forward (BN prologue, statistics)
    and mirrored-tap data gradient, every instance of the dispatch table incl. the channel-split / multi-image / channel-staged
    ones -- is BIT-IDENTICAL to the plain layout: only the addresses of the weight loads differ.  The rolling-window kernel and
    the generic GEMM refuse the flag."""
    from frhip import _lib
    dtype = torch.bfloat16
    st = K.current_stream_ptr()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4100 + cin + cout + W + B)
    x = torch.randn(B, W, W, cin, device="cuda", generator=gen).to(dtype)
    w = (torch.randn(cout, 9, cin, device="cuda", generator=gen) * 0.05).to(dtype)
    wt = w.permute(2, 1, 0).contiguous()
    pa, pb = synth.uniform(41, "fa", (cin,), 0.5, 1.5).cuda(), synth.uniform(41, "fb", (cin,), -0.5, 0.5).cuda()
    assert _lib.lib.fr_conv3x3_strip_takes_frag(B, cin, cout, W) == 1
    common = dict(B=B, RH=W, RW=W, SH=W, SW=W, KH=3, KW=3, stride=1, pad=1)
    store_only = (cin, cout, W) == (256, 512, 14)
    res = []
    for frag in (0, 1):
        out = torch.full((B, W, W, cout), float("nan"), device="cuda", dtype=dtype)
        nparts = K.strip_parts(B, cin, cout, W)
        part = torch.zeros(nparts, 2, cout, device="cuda")
        K.conv_strip(st, src=x, w=to_frag(w) if frag else w, out=out, SC=cin, N=cout, mode=0, lda=cin, ldc=cout, pro=K.PRO_BN,
                     pro_a=pa, pro_b=pb, epi=K.EPI_STORE if store_only else K.EPI_STATS, part=part, w_frag=frag, **common)()
        g = out  # the data gradient of a cout-channel tensor back to cin channels
        gx = torch.full((B, W, W, cin), float("nan"), device="cuda", dtype=dtype)
        nb = K.strip_parts(B, cout, cin, W, K.EPI_STORE)
        if nb:
            K.conv_strip(st, src=g, w=to_frag(wt) if frag else wt, out=gx, SC=cout, N=cin, mode=1, lda=cout, ldc=cin, pro=0,
                         epi=K.EPI_STORE, w_frag=frag, **common)()
        torch.cuda.synchronize()
        res.append((out, part, gx))
    assert torch.isfinite(res[0][0].float()).all()
    assert torch.equal(res[0][0], res[1][0]) and torch.equal(res[0][1], res[1][1])
    assert torch.equal(res[0][2].view(torch.int16), res[1][2].view(torch.int16))
    with pytest.raises(_lib.FrhipError):
        K.conv(st, _lib.FR_BF16, src=x, w=w, out=res[0][0], SC=cin, N=cout, mode=0, lda=cin, ldc=cout, pro=0, epi=K.EPI_STORE,
               w_frag=1, **common)()


def test_fragment_order_is_refused_by_the_rolling_window_kernel(K):
    from frhip import _lib
    assert _lib.lib.fr_conv3x3_strip_takes_frag(4, 64, 64, 56) == 0 and _lib.lib.fr_conv3x3_strip_takes_frag(4, 96, 96, 14) == 0
    x = torch.zeros(2, 56, 56, 64, device="cuda", dtype=torch.bfloat16)
    w = torch.zeros(64, 9, 64, device="cuda", dtype=torch.bfloat16)
    with pytest.raises(_lib.FrhipError):
        K.conv_strip(K.current_stream_ptr(), src=x, w=w, out=torch.zeros_like(x), B=2, RH=56, RW=56, SH=56, SW=56, KH=3, KW=3,
                     stride=1, pad=1, SC=64, N=64, mode=0, lda=64, ldc=64, pro=0, epi=K.EPI_STORE, w_frag=1)()


@pytest.mark.parametrize("name,dtype,tol", DT)
def test_fused_se_launches_are_bit_identical(K, name, dtype, tol):
    """fr_se_pool_parts_mlp_fwd == fr_se_pool_parts + fr_se_mlp_fwd and fr_se_gscale_mlp_bwd == fr_se_gscale + fr_se_mlp_bwd
    (round 3: one launch less per IR-SE unit in each direction), bit for bit on every output."""
    B, HW, C, R, NS = 5, 49, 128, 8, 2
    st = K.current_stream_ptr()
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    dev = lambda t: t.cuda()  # noqa: E731
    part = dev(synth.normal(91, "sp", (B * NS, 2, C)))
    scale, shift = dev(synth.uniform(91, "ssc", (C,), 0.5, 1.5)), dev(synth.uniform(91, "ssh", (C,), -0.3, 0.3))
    w1, w2 = dev(synth.normal(91, "sw1", (R, C), std=0.2)), dev(synth.normal(91, "sw2", (C, R), std=0.2))
    outs = []
    for fused in (False, True):
        pooled, hidden, s = torch.zeros(B, C, device="cuda"), torch.zeros(B, R, device="cuda"), torch.zeros(B, C, device="cuda")
        if fused:
            K.call("fr_se_pool_parts_mlp_fwd", part, NS, scale, shift, w1, w2, pooled, hidden, s, B, HW, C, R, st)()
        else:
            K.call("fr_se_pool_parts", part, NS, scale, shift, pooled, B, HW, C, st)()
            K.call("fr_se_mlp_fwd", pooled, w1, w2, hidden, s, B, C, R, st)()
        torch.cuda.synchronize()
        outs.append((pooled, hidden, s))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    pooled, hidden, s = outs[0]
    g = nhwc(q(synth.normal(91, "sg", (B, C, 7, 7)), dtype), dtype)
    x = nhwc(q(synth.normal(91, "sx", (B, C, 7, 7)), dtype), dtype)
    outs = []
    for fused in (False, True, "slices"):
        gpooled, dw1, dw2 = torch.zeros(B, C, device="cuda"), torch.zeros(R, C, device="cuda"), torch.zeros(C, R, device="cuda")
        gz, gh, gs = torch.zeros(B, C, device="cuda"), torch.zeros(B, R, device="cuda"), torch.zeros(B, C, device="cuda")
        if fused:
            part = torch.full((B * 8 * C,), float("nan"), device="cuda") if fused == "slices" else None
            K.call("fr_se_gscale_mlp_bwd", g, x, scale, shift, s, hidden, pooled, w1, w2, gpooled, dw1, dw2, gz, gh, part, B, C,
                   R, HW, fr, st)()
        else:
            K.call("fr_se_gscale", g, x, scale, shift, gs, B, HW, C, fr, st)()
            K.call("fr_se_mlp_bwd", gs, s, hidden, pooled, w1, w2, gpooled, dw1, dw2, gz, gh, B, C, R, HW, st)()
        torch.cuda.synchronize()
        outs.append((gpooled, dw1, dw2, gz, gh))
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b) and torch.isfinite(a).all()
    # round 5: the squeeze over row slices adds the rows of an image in another order -- fp32 rounding of sums of HW terms
    for a, c in zip(outs[0], outs[2]):
        assert torch.isfinite(c).all() and float((a - c).abs().max()) <= 2e-5 * float(a.abs().max()) + 1e-12
    assert float(outs[0][1].abs().max()) > 0


def test_bf16_engine_with_and_without_strip_agree():
    """The LDS-strip convolutions and the generic implicit-GEMM path are two implementations of the same layers: a
    full bf16 IR-50 step must give (nearly) the same features and gradients through either."""
    import os
    from backbone.model_irse import IR_50
    from head.metrics import ArcFace
    from loss.focal import FocalLoss
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    res = []
    for no_strip in ("0", "1"):
        os.environ["FRHIP_NO_STRIP"] = no_strip
        m = IR_50([112, 112])
        synth.fill_state_dict(m.state_dict(), 15)
        m.output_layer[1].p = 0.0
        m.compute_dtype = torch.bfloat16
        m = m.cuda().train()
        head = ArcFace(512, 100, None).cuda()
        with torch.no_grad():
            head.weight.copy_(synth.uniform(16, "full.head", (100, 512), -0.1, 0.1))
        x = synth.uniform(16, "full.x", (16, 3, 112, 112)).cuda()
        y = synth.labels(16, "full.label", 16, 100).cuda()
        feats = m(x)
        loss, _ = FocalLoss()(head(feats, y), y)
        loss.backward()
        torch.cuda.synchronize()
        res.append((feats.detach().clone(), {n: p.grad.detach().clone() for n, p in m.named_parameters()}))
    os.environ.pop("FRHIP_NO_STRIP")
    (f0, g0), (f1, g1) = res
    assert float(torch.nn.functional.cosine_similarity(f0, f1, dim=1).min()) > 0.999
    for n in ("body.23.res_layer.3.weight", "body.10.res_layer.1.weight", "body.0.res_layer.2.weight",
              "input_layer.0.weight", "body.7.res_layer.0.weight"):
        d = float((g0[n] - g1[n]).norm() / (g1[n].norm() + 1e-12))
        c = float(torch.nn.functional.cosine_similarity(g0[n].reshape(1, -1), g1[n].reshape(1, -1)))
        print("   strip vs generic %-32s rel diff %.4f cos %.5f" % (n, d, c))
        # two bf16 implementations against EACH OTHER (noise of both), batch 16.  The 64 PReLU slopes of unit 0 sit behind
        # the rounding of the whole backward pass (measured 0.154 / 0.9882; the conv weights 0.12 / 0.992 and better); the
        # test against the reference itself is test_bf16_full_step_tracks_reference.
        if n.endswith("res_layer.2.weight"):
            assert d < 0.2 and c > 0.98, (n, d, c)
        else:
            assert d < 0.15 and c > 0.99, (n, d, c)


WGS_SHAPES = [(64, 64, 112, "bn"), (64, 64, 56, "prelu"), (128, 64, 56, "bn"), (128, 128, 28, "prelu"),
              (256, 128, 28, "bn"), (256, 256, 14, "prelu"), (512, 256, 14, "bn"), (512, 512, 7, "prelu"),
              (128, 128, 28, "none")]


# (cout, cin, W, prologue, B, strip groups).  Small cases: B = 5 exercises the ragged last fill of the 7x7 kernel.
# "bench" cases: the group counts engine._wgrad computes for the B = 256 step (min(fills, 256 / tiles)) with batches
# large enough to reach them, and B = 162 for the two 14x14 / 7x7 instances that carry most of the weight-gradient time.
WGS_CASES = [s + (5 if s[2] <= 14 else 2, g) for s in WGS_SHAPES for g in (1, 3)] + [
    (256, 256, 14, "prelu", 162, 16), (256, 256, 14, "bn", 162, 16), (512, 512, 7, "prelu", 162, 4),
    (512, 256, 14, "bn", 40, 8), (128, 128, 28, "prelu", 18, 64), (64, 64, 56, "prelu", 20, 256),
    (64, 64, 112, "bn", 6, 256)]


@pytest.mark.parametrize("cout,cin,W,pro,B,groups", WGS_CASES, ids=["%d_%d_%d_%s_b%d_g%d" % s for s in WGS_CASES])
def test_conv_wgrad_strip(K, cout, cin, W, pro, B, groups):
    """LDS-strip weight gradient (bf16) vs CPU autograd."""
    dtype, tol = torch.bfloat16, BF16_TOL
    assert K.wgrad_strip_supported(cout, cin, W)
    x = q(synth.normal(41, "wsx", (B, cin, W, W)), dtype)
    pa = synth.uniform(41, "wspa", (cin,), 0.5, 1.5)
    pb = synth.uniform(41, "wspb", (cin,), -0.5, 0.5)
    if pro == "bn":
        xin = (x.double() * pa.double().view(1, -1, 1, 1) + pb.double().view(1, -1, 1, 1)).float()  # one rounding (fmaf)
    elif pro == "prelu":
        xin = F.prelu(x, pa * 0.25)
    else:
        xin = x
    xin = q(xin, dtype)
    w = synth.normal(41, "wsw", (cout, cin, 3, 3), std=0.1).requires_grad_(True)
    y = F.conv2d(xin, w, padding=1)
    g = q(synth.normal(41, "wsg", tuple(y.shape)), dtype)
    (gw,) = torch.autograd.grad(y, [w], g)
    dw = torch.full((cout, 9, cin), 7.0, device="cuda")  # must be overwritten, not accumulated
    slab = torch.zeros(groups * cout * 9 * cin, device="cuda")
    a_dev = (pa * 0.25 if pro == "prelu" else pa).cuda()
    K.wgrad_strip(K.current_stream_ptr(), g=nhwc(g, dtype), src=nhwc(x, dtype), dw=dw, slab=slab, B=B, GH=W, GW=W,
                  Cout=cout, SH=W, SW=W, SC=cin, KH=3, KW=3, stride=1, pad=1, ldg=cout, lda=cin,
                  pro={"none": 0, "bn": 1, "prelu": 2}[pro], nsplit=groups, pro_a=a_dev, pro_b=pb.cuda())()
    torch.cuda.synchronize()
    got = dw.cpu().reshape(cout, 3, 3, cin).permute(0, 3, 1, 2)
    assert relerr(got, gw) < tol


def test_conv_wgrad_deferred_slab_sum_is_bit_identical(K):
    """FrWgradArgs.defer / prev_* (round 3): a launch that leaves the sum of its slabs to the NEXT weight-gradient launch
    of the stream (whose workgroups add them while their first tiles load) or to fr_reduce_slabs must give bit for bit the
    dW of the launch that sums its own slabs -- three layers chained A -> B -> C -> flush against three plain launches,
    ragged group sizes included, through both kernels behind fr_conv_wgrad_strip (warp-specialised: 14x14 / 28x28; strip:
    56x56, 7x7, stride 2) and with more than 16 slabs (chunked summation order, csrc/slab_sum.h)."""
    from frhip import _lib
    dtype = torch.bfloat16
    st = K.current_stream_ptr()
    # cout, cin, W, B, groups, pro -- 14x14 (whole images per group) and 28x28 (runs of phases that start inside images)
    layers = [(256, 256, 14, 37, 5, 2), (128, 64, 28, 5, 9, 1), (64, 192, 14, 6, 6, 0), (128, 128, 28, 3, 4, 2),
              (64, 64, 56, 3, 40, 1), (512, 512, 7, 9, 3, 2), (128, 128, 28, 5, 6, 2, 2), (64, 64, 56, 2, 20, 0)]
    plain, chained, slabs, kws = [], [], [], []
    for k, layer in enumerate(layers):
        cout, cin, W, B, groups, pro = layer[:6]
        stride = layer[6] if len(layer) > 6 else 1  # W = input side; the gradient is W / stride wide
        g = (torch.randn(B, W // stride, W // stride, cout, device="cuda") * 0.5).to(dtype)
        x = torch.randn(B, W, W, cin, device="cuda").to(dtype)
        pa, pb = torch.rand(cin, device="cuda") + 0.25, torch.rand(cin, device="cuda") - 0.5
        kw = dict(g=g, src=x, B=B, GH=W // stride, GW=W // stride, Cout=cout, SH=W, SW=W, SC=cin, KH=3, KW=3, stride=stride,
                  pad=1, ldg=cout, lda=cin, pro=pro, nsplit=groups, pro_a=pa, pro_b=pb)
        dw = torch.full((cout, 9, cin), 3.0, device="cuda")
        K.wgrad_strip(st, dw=dw, slab=torch.zeros(groups * cout * 9 * cin, device="cuda"), **kw)()
        plain.append(dw)
        kws.append(kw)
        chained.append(torch.full((cout, 9, cin), 5.0, device="cuda"))
        slabs.append(torch.zeros(groups * cout * 9 * cin, device="cuda"))
    probe = K._fill(_lib.FrWgradArgs(), dw=chained[0], slab=slabs[0], **kws[0])
    assert _lib.lib.fr_conv_wgrad_strip_defers(ctypes.byref(probe)) == 1
    prev = None
    for k, kw in enumerate(kws):
        extra = {}
        if prev is not None:
            pk = kws[prev]
            extra = dict(prev_slab=slabs[prev], prev_dw=chained[prev], prev_groups=pk["nsplit"],
                         prev_n=pk["Cout"] * 9 * pk["SC"])
        K.wgrad_strip(st, dw=chained[k], slab=slabs[k], defer=1, **extra, **kw)()
        prev = k
    last = kws[-1]
    K.call("fr_reduce_slabs", slabs[-1], last["nsplit"], last["Cout"] * 9 * last["SC"], chained[-1], st)()
    torch.cuda.synchronize()
    for k in range(len(layers)):
        assert torch.equal(plain[k], chained[k]), "layer %d: deferred sum differs by %g" % (
            k, float((plain[k] - chained[k]).abs().max()))


@pytest.mark.parametrize("name,dtype,tol", DT)
@pytest.mark.parametrize("fused", [False, True], ids=["four_launches", "one_launch"])
def test_conv_dgrad_stride2_by_parity(K, name, dtype, tol, fused):
    """mode 2: the stride-2 3x3 data gradient by output-pixel parity class (only the taps that hit an input pixel),
    as four launches or as one launch over all classes (par = -1), with the PReLU-backward epilogue; must equal
    autograd through the strided convolution."""
    B, H, cin, cout = 3, 12, 64, 128
    x = synth.normal(51, "px", (B, cin, H, H)).requires_grad_(True)
    w = q(synth.normal(51, "pw", (cout, cin, 3, 3), std=0.1), dtype)
    y = F.conv2d(x, w, stride=2, padding=1)
    g = q(synth.normal(51, "pg", tuple(y.shape)), dtype)
    (gx,) = torch.autograd.grad(y, [x], g)
    aux = q(synth.normal(51, "pa", (B, cin, H, H)), dtype)
    slope = synth.uniform(51, "ps", (cin,), 0.1, 0.4)
    want = torch.where(aux > 0, gx, gx * slope.view(1, -1, 1, 1))
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    wt = w.permute(1, 2, 3, 0).reshape(cin, 9, cout).contiguous().to("cuda", dtype)
    out = torch.zeros(B, H, H, cin, device="cuda", dtype=dtype)
    mtc = (B * (H // 2) ** 2 + 127) // 128
    part = torch.zeros(4 * mtc, 2, cin, device="cuda")
    for c, (ph, pw) in enumerate(((-1, -1),) if fused else ((0, 0), (0, 1), (1, 0), (1, 1))):
        K.conv(K.current_stream_ptr(), fr, src=nhwc(g, dtype), w=wt, out=out, B=B, RH=H, RW=H, SH=H // 2, SW=H // 2,
               SC=cout, N=cin, KH=3, KW=3, stride=2, pad=1, mode=2, par_h=ph, par_w=pw, lda=cout, ldc=cin, ldaux=cin,
               pro=0, epi=K.EPI_PRELU_BWD, aux=nhwc(aux, dtype), epi_a=slope.cuda(), part=part[c * mtc:])()
    torch.cuda.synchronize()
    assert relerr(from_nhwc(out), want) < tol
    np.testing.assert_allclose(part.sum(0)[0].cpu(), (gx * aux * (aux <= 0)).sum((0, 2, 3)), rtol=tol * 10,
                               atol=tol * 10 * float((gx * aux).abs().sum() / cin))


S2_SHAPES = [(64, 56), (128, 28), (256, 14), (512, 7)]
# 64 channels run on the rolling-window kernel (conv3x3_s2_roll64.hip), whose walk depends on the batch: B = 3 / 2: 28 row
# segments per image (2-row walks); B = 20: 14 segments; B = 40: 7 segments, 280 work items on 256 persistent workgroups
# (item loop); B = 64: 4 segments; B = 130: 2 segments; "whole": FRHIP_S2ROLL_NSEG=1 = the 56-row walk of the B >= 256 step, on three images
# (512, 7, B even): the forward runs two images per workgroup with the output channels over four workgroups (one and
# three strips); (256, 14): the forward owns whole images, output channels over two workgroups (any batch)
S2_CASES = [s + (3, "") for s in S2_SHAPES] + [(64, 56, 20, ""), (64, 56, 40, ""), (64, 56, 64, ""), (64, 56, 130, ""),
                                                (64, 56, 3, "whole"), (512, 7, 2, ""), (512, 7, 6, "")]


@pytest.fixture
def s2_walk(K):
    """FRHIP_S2ROLL_NSEG = 1 (test hook of the library): walks of whole images at small batches."""
    def set_walk(walk):
        if walk == "whole":
            K.set_option("FRHIP_S2ROLL_NSEG", 1)
    yield set_walk
    K.set_option("FRHIP_S2ROLL_NSEG", -1)


@pytest.mark.parametrize("C,WL,B,walk", S2_CASES, ids=["%d_%d_b%d%s" % s for s in S2_CASES])
@pytest.mark.parametrize("pro", ["none", "bn", "prelu"])
def test_conv3x3_s2_strip_forward(K, s2_walk, C, WL, B, walk, pro):
    """fr_conv3x3_s2_strip mode 0: stride-2 3x3 forward on LDS parity planes (+ prologue, + BN statistics) vs
    F.conv2d on the CPU, and vs the generic implicit-GEMM kernel's partial-sum contract (column totals)."""
    dtype, tol = torch.bfloat16, BF16_TOL
    s2_walk(walk)
    H = 2 * WL
    if B > 6 and pro != "prelu":
        pytest.skip("large batches: the prologue the step uses")
    sel = _image_subset(B)
    x, xd = _operand(B, sel, 61, "sx", (B, C, H, H), dtype)  # x: the images `sel` (all of them up to 32)
    w = q(synth.normal(61, "sw", (C, C, 3, 3), std=0.05), dtype)
    pa = synth.uniform(61, "spa", (C,), 0.5, 1.5)
    pb = synth.uniform(61, "spb", (C,), -0.3, 0.3)
    v = lambda t: t.view(1, C, 1, 1)  # noqa: E731
    if pro == "bn":
        xin = q(x * v(pa) + v(pb), dtype)
    elif pro == "prelu":
        xin = q(torch.where(x > 0, x, x * v(pa * 0.25)), dtype)
    else:
        xin = x
    y = F.conv2d(xin, w, stride=2, padding=1)
    n = K.s2_strip_parts(B, C, C, WL, 0)
    assert n > 0
    out = torch.zeros(B, WL, WL, C, device="cuda", dtype=dtype)
    part = torch.zeros(n, 2, C, device="cuda")
    a_dev = (pa * 0.25 if pro == "prelu" else pa).cuda()
    K.conv_s2_strip(K.current_stream_ptr(), src=xd, w=pack_w(w, dtype), out=out, B=B, RH=WL, RW=WL, SH=H,
                    SW=H, SC=C, N=C, KH=3, KW=3, stride=2, pad=1, mode=0, lda=C, ldc=C,
                    pro={"none": 0, "bn": 1, "prelu": 2}[pro], pro_a=a_dev, pro_b=pb.cuda(), epi=K.EPI_STATS,
                    part=part)()
    torch.cuda.synchronize()
    got = from_nhwc(out[sel])
    assert torch.isfinite(out.float()).all() and relerr(got, y) < tol
    ps = part[_part_rows(n, B, sel)].sum(0)  # forward rows are image-major, the same number per image
    np.testing.assert_allclose(ps[0].cpu(), y.sum((0, 2, 3)), rtol=tol, atol=tol * float(y.abs().sum() / C))
    np.testing.assert_allclose(ps[1].cpu(), (y * y).sum((0, 2, 3)), rtol=tol)
    _assert_all_part_rows_match_the_stored_output(part, out, "stride-2 forward")


@pytest.mark.parametrize("C,WL,B,walk", S2_CASES, ids=["%d_%d_b%d%s" % s for s in S2_CASES])
def test_conv3x3_s2_strip_dgrad(K, s2_walk, C, WL, B, walk):
    """fr_conv3x3_s2_strip mode 2: all four parity classes of the stride-2 data gradient with the PReLU-backward
    epilogue, vs autograd through F.conv2d(stride=2)."""
    dtype, tol = torch.bfloat16, BF16_TOL
    s2_walk(walk)
    H = 2 * WL
    sel = _image_subset(B)
    x = synth.normal(63, "dx", (len(sel), C, H, H)).requires_grad_(True)
    w = q(synth.normal(63, "dw", (C, C, 3, 3), std=0.05), dtype)
    y = F.conv2d(x, w, stride=2, padding=1)
    g, gd = _operand(B, sel, 63, "dg", (B,) + tuple(y.shape[1:]), dtype)
    (gx,) = torch.autograd.grad(y, [x], g)
    aux, auxd = _operand(B, sel, 63, "da", (B, C, H, H), dtype)
    slope = synth.uniform(63, "ds", (C,), 0.1, 0.4)
    want = torch.where(aux > 0, gx, gx * slope.view(1, -1, 1, 1))
    wt = w.permute(1, 2, 3, 0).reshape(C, 9, C).contiguous().to("cuda", dtype)
    out = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
    n = K.s2_strip_parts(B, C, C, WL, 2)
    assert n > 0
    part = torch.zeros(n, 2, C, device="cuda")
    K.conv_s2_strip(K.current_stream_ptr(), src=gd, w=wt, out=out, B=B, RH=H, RW=H, SH=WL, SW=WL, SC=C, N=C,
                    KH=3, KW=3, stride=2, pad=1, mode=2, par_h=-1, par_w=-1, lda=C, ldc=C, ldaux=C, pro=0,
                    epi=K.EPI_PRELU_BWD, aux=auxd, epi_a=slope.cuda(), part=part)()
    torch.cuda.synchronize()
    assert torch.isfinite(out.float()).all() and relerr(from_nhwc(out[sel]), want) < tol
    if len(sel) == B:  # (beyond 32 images only a subset is convolved on the host; the slope sums of the large-batch geometry
        #                are part of every bench-size training step compared with the reference: g13)
        np.testing.assert_allclose(part.sum(0)[0].cpu(), (gx * aux * (aux <= 0)).sum((0, 2, 3)), rtol=tol * 10,
                                   atol=tol * 10 * float((gx * aux).abs().sum() / C))


S2_FRAG_CASES = [(128, 28, 3), (128, 28, 40), (256, 14, 3), (256, 14, 8), (512, 7, 3), (512, 7, 6), (512, 7, 8)]


@pytest.mark.parametrize("C,WL,B", S2_FRAG_CASES, ids=["%d_%d_b%d" % s for s in S2_FRAG_CASES])
def test_conv3x3_s2_strip_fragment_order_weights(K, C, WL, B):
    """FrConvArgs.w_frag on the stride-2 kernels (the warp-specialised forward, the strip data gradient, and -- FRHIP_S2_WS = 0 --
    the strip forward): bit-identical to the plain weight layout, outputs and partial rows."""
    from frhip import _lib
    dtype, st, H = torch.bfloat16, K.current_stream_ptr(), 2 * WL
    gen = torch.Generator(device="cuda")
    gen.manual_seed(4300 + C + B)
    x = torch.randn(B, H, H, C, device="cuda", generator=gen).to(dtype)
    g = torch.randn(B, WL, WL, C, device="cuda", generator=gen).to(dtype)
    w = (torch.randn(C, 9, C, device="cuda", generator=gen) * 0.05).to(dtype)
    wt = w.permute(2, 1, 0).contiguous()
    slope = synth.uniform(43, "fs", (C,), 0.1, 0.4).cuda()
    assert _lib.lib.fr_conv3x3_s2_strip_takes_frag(B, C, WL, 0) == 1 and _lib.lib.fr_conv3x3_s2_strip_takes_frag(B, C, WL, 2) == 1
    assert _lib.lib.fr_conv3x3_s2_strip_takes_frag(B, 64, 56, 0) == 0
    for ws in (1, 0):
        prev = K.set_option("FRHIP_S2_WS", ws)
        try:
            res = []
            for frag in (0, 1):
                n = K.s2_strip_parts(B, C, C, WL, 0)
                out = torch.full((B, WL, WL, C), float("nan"), device="cuda", dtype=dtype)
                part = torch.zeros(n, 2, C, device="cuda")
                K.conv_s2_strip(st, src=x, w=to_frag(w) if frag else w, out=out, B=B, RH=WL, RW=WL, SH=H, SW=H, SC=C, N=C, KH=3,
                                KW=3, stride=2, pad=1, mode=0, lda=C, ldc=C, pro=2, pro_a=slope, epi=K.EPI_STATS, part=part,
                                w_frag=frag)()
                n2 = K.s2_strip_parts(B, C, C, WL, 2)
                gx = torch.full((B, H, H, C), float("nan"), device="cuda", dtype=dtype)
                part2 = torch.zeros(n2, 2, C, device="cuda")
                K.conv_s2_strip(st, src=g, w=to_frag(wt) if frag else wt, out=gx, B=B, RH=H, RW=H, SH=WL, SW=WL, SC=C, N=C, KH=3,
                                KW=3, stride=2, pad=1, mode=2, par_h=-1, par_w=-1, lda=C, ldc=C, ldaux=C, pro=0,
                                epi=K.EPI_PRELU_BWD, aux=x, epi_a=slope, part=part2, w_frag=frag)()
                torch.cuda.synchronize()
                res.append((out, part, gx, part2))
        finally:
            K.set_option("FRHIP_S2_WS", prev)
        assert torch.isfinite(res[0][0].float()).all() and torch.isfinite(res[0][2].float()).all()
        for a, b in zip(res[0], res[1]):
            assert torch.equal(a, b), "FRHIP_S2_WS=%d" % ws


@pytest.mark.parametrize("Cavg,ldk", [(0, 32), (3, 64)], ids=["ir", "psp"])
@pytest.mark.parametrize("B,S", [(3, 9), (2, 112)])
@pytest.mark.parametrize("dt", ["bf16", "f32"])
def test_stem_im2col_rows(K, Cavg, ldk, B, S, dt):
    """fr_stem_im2col: row p = pixel (b, h, w), column (kh*3 + kw) * Ct + c = input (or average-image) channel c at
    (h + kh - 1, w + kw - 1), zero outside the image and in the K tail -- both the row-per-thread bf16 kernel of the two
    shipped stems and the generic one, against F.unfold."""
    dtype = torch.bfloat16 if dt == "bf16" else torch.float32
    x = synth.normal(75, "ix", (B, 3, S, S))
    avg = synth.normal(75, "ia", (Cavg, S, S)) if Cavg else None
    full = x if avg is None else torch.cat([x, avg.unsqueeze(0).expand(B, -1, -1, -1)], 1)
    Ct = 3 + Cavg
    cols = F.unfold(full, 3, padding=1).view(B, Ct, 9, S * S)          # [b][c][tap][pixel]
    want = torch.zeros(B * S * S, ldk)
    want[:, :9 * Ct] = cols.permute(0, 3, 2, 1).reshape(B * S * S, 9 * Ct)
    out = torch.full((B * S * S, ldk), 7.0, device="cuda", dtype=dtype)
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    K.call("fr_stem_im2col", x.cuda(), avg.cuda() if avg is not None else None, out, B, S, S, 3, Cavg, ldk, fr,
           K.current_stream_ptr())()
    torch.cuda.synchronize()
    assert torch.equal(out.float().cpu(), want.to(dtype).float())


@pytest.mark.parametrize("Kp", [32, 64])
@pytest.mark.parametrize("M", [16, 1000, 4099])
def test_stem_gemm_and_wgrad(K, Kp, M):
    """fr_stem_gemm / fr_stem_wgrad: the 64-column input-layer GEMMs over im2col rows (row counts that are not a
    multiple of the 16-row tile or the 64-row staging chunk), forward + column statistics + weight gradient."""
    dtype, tol = torch.bfloat16, BF16_TOL
    x = q(synth.normal(71, "gx%d" % M, (M, Kp)), dtype)
    w = q(synth.normal(71, "gw", (64, Kp), std=0.2), dtype)
    y = x @ w.t()
    st = K.current_stream_ptr()
    nb = 5
    out = torch.zeros(M, 64, device="cuda", dtype=dtype)
    part = torch.zeros(nb, 2, 64, device="cuda")
    K.call("fr_stem_gemm", x.to("cuda", dtype), w.to("cuda", dtype), out, part, M, Kp, nb, st)()
    torch.cuda.synchronize()
    got = out.float().cpu()
    assert relerr(got, y) < tol
    np.testing.assert_allclose(part.sum(0)[0].cpu(), got.sum(0), rtol=1e-3, atol=1e-2)
    np.testing.assert_allclose(part.sum(0)[1].cpu(), (got * got).sum(0), rtol=1e-3, atol=1e-2)
    g = q(synth.normal(71, "gg%d" % M, (M, 64)), dtype)
    want = g.t() @ x
    ns = 7
    slab = torch.zeros(ns, 64, Kp, device="cuda")
    K.call("fr_stem_wgrad", g.to("cuda", dtype), x.to("cuda", dtype), slab, M, Kp, ns, st)()
    dw = torch.zeros(64 * Kp, device="cuda")
    K.call("fr_reduce_parts", slab, ns, 1, 64 * Kp, dw, None, None, st)()
    torch.cuda.synchronize()
    assert relerr(dw.cpu().view(64, Kp), want) < tol


@pytest.mark.parametrize("C,WL", S2_SHAPES, ids=["%d_%d" % s for s in S2_SHAPES])
@pytest.mark.parametrize("groups", [1, 3, 5])
def test_conv_wgrad_strip_stride2(K, C, WL, groups):
    """fr_conv_wgrad_strip on a stride-2 layer (input tile = four parity planes) with the PReLU prologue, vs autograd.
    128 / 256 / 512 channels run on the warp-specialised kernel (conv_wgrad_s2roll_kernel): 42 / 12 / 3 phases at B = 3,
    so 5 groups give runs that start inside an image, an odd number of phases, and (14x14, 7x7) a group without work."""
    dtype, tol = torch.bfloat16, BF16_TOL
    B, H = 3, 2 * WL
    x = q(synth.normal(65, "wx", (B, C, H, H)), dtype)
    slope = synth.uniform(65, "ws", (C,), 0.1, 0.4)
    xin = q(torch.where(x > 0, x, x * slope.view(1, -1, 1, 1)), dtype)
    w = synth.normal(65, "ww", (C, C, 3, 3), std=0.05).requires_grad_(True)
    y = F.conv2d(xin, w, stride=2, padding=1)
    g = q(synth.normal(65, "wg", tuple(y.shape)), dtype)
    (gw,) = torch.autograd.grad(y, [w], g)
    dw = torch.zeros(C, 9, C, device="cuda")
    slab = torch.zeros(groups * C * 9 * C, device="cuda")
    K.wgrad_strip(K.current_stream_ptr(), g=nhwc(g, dtype), src=nhwc(x, dtype), dw=dw, slab=slab, B=B, GH=WL, GW=WL,
                  Cout=C, SH=H, SW=H, SC=C, KH=3, KW=3, stride=2, pad=1, ldg=C, lda=C, pro=2, nsplit=groups,
                  pro_a=slope.cuda())()
    torch.cuda.synchronize()
    got = dw.cpu().reshape(C, 3, 3, C).permute(0, 3, 1, 2)
    assert relerr(got, gw) < tol


@pytest.mark.parametrize("name,dtype,tol", DT)
def test_bn_prelu_backward(K, name, dtype, tol):
    """Stem pattern BN -> PReLU (model_irse.py:141-142): backward sums (incl. the slope gradient) and input gradient
    vs autograd; the bf16 reduce takes the lean SLOPE variant."""
    B, H, C = 3, 7, 64
    rows = B * H * H
    x = q(synth.normal(81, "px", (B, C, H, H)), dtype).requires_grad_(True)
    gamma = synth.uniform(81, "pg", (C,), 0.8, 1.2).requires_grad_(True)
    beta = synth.uniform(81, "pb", (C,), -0.3, 0.3).requires_grad_(True)
    slope = synth.uniform(81, "ps", (C,), 0.1, 0.4).requires_grad_(True)
    z = F.prelu(F.batch_norm(x, None, None, gamma, beta, True, 0.1, 1e-5), slope)
    g = q(synth.normal(81, "pgo", tuple(z.shape)), dtype)
    gx, gg, gb, gs = torch.autograd.grad(z, [x, gamma, beta, slope], g)
    xd = x.detach()
    mean = xd.mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(xd.var((0, 2, 3), unbiased=False) + 1e-5)
    scale = (gamma.detach() * invstd)
    shift = beta.detach() - mean * scale
    fr, st = K.fr_dtype(torch.empty(0, dtype=dtype)), K.current_stream_ptr()
    nb = 6
    common = dict(g=nhwc(g, dtype), x=nhwc(xd, dtype), mean=mean.cuda(), invstd=invstd.cuda(), scale=scale.cuda(),
                  shift=shift.cuda(), slope=slope.detach().cuda(), rows=rows, C=C, rows_per_image=H * H, nblocks=nb)
    part = torch.zeros(nb, 3, C, device="cuda")
    K.bn_bwd_reduce(st, fr, part=part, **common)()
    s0, s1, s2 = (torch.zeros(C, device="cuda") for _ in range(3))
    K.call("fr_reduce_parts", part, nb, 3, C, s0, s1, s2, st)()
    gxd = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
    K.bn_bwd_apply(st, fr, gx=gxd, gamma=gamma.detach().cuda(), s0=s0, s1=s1, inv_count=1.0 / rows, **common)()
    torch.cuda.synchronize()
    np.testing.assert_allclose(s0.cpu(), gb, rtol=tol * 5, atol=tol * 20)
    np.testing.assert_allclose(s1.cpu(), gg, rtol=tol * 5, atol=tol * 20)
    np.testing.assert_allclose(s2.cpu(), gs, rtol=tol * 5, atol=tol * 20)
    assert relerr(from_nhwc(gxd), gx) < tol * 2


@pytest.mark.parametrize("Kp", [32, 64])
def test_stem_wgrad_bn_equals_unfused(K, Kp):
    """fr_stem_wgrad_bn == fr_bn_bwd_apply (BN -> PReLU backward) followed by fr_stem_wgrad, bit for bit."""
    dtype = torch.bfloat16
    M, C = 4099, 64
    st = K.current_stream_ptr()
    fr = K.fr_dtype(torch.empty(0, dtype=dtype))
    g = synth.normal(91, "fg", (M, C)).to("cuda", dtype)
    y = synth.normal(91, "fy", (M, C)).to("cuda", dtype)
    x = synth.normal(91, "fx", (M, Kp)).to("cuda", dtype)
    vec = lambda n, lo, hi: synth.uniform(91, n, (C,), lo, hi).cuda()  # noqa: E731
    mean, invstd, gamma, slope = vec("m", -0.3, 0.3), vec("i", 0.5, 2.0), vec("g", 0.8, 1.2), vec("s", 0.1, 0.4)
    s0, s1 = vec("s0", -50.0, 50.0), vec("s1", -50.0, 50.0)
    scale = gamma * invstd
    shift = vec("b", -0.2, 0.2) - mean * scale
    gy = torch.zeros(M, C, device="cuda", dtype=dtype)
    K.bn_bwd_apply(st, fr, g=g, x=y, gx=gy, mean=mean, invstd=invstd, scale=scale, shift=shift, slope=slope, gamma=gamma,
                   s0=s0, s1=s1, rows=M, inv_count=1.0 / M, C=C, rows_per_image=M, nblocks=8)()
    ns = 9
    slab_a = torch.zeros(ns, 64, Kp, device="cuda")
    slab_b = torch.zeros(ns, 64, Kp, device="cuda")
    K.call("fr_stem_wgrad", gy, x, slab_a, M, Kp, ns, st)()
    K.call("fr_stem_wgrad_bn", g, y, x, mean, invstd, scale, shift, slope, gamma, s0, s1, 1.0 / M, slab_b, M, Kp, ns,
           st)()
    torch.cuda.synchronize()
    assert torch.equal(slab_a, slab_b)
    assert float(slab_a.abs().max()) > 0


@pytest.mark.parametrize("name,dtype,tol", DT)
@pytest.mark.parametrize("with_add", [False, True])
def test_bn_backward_with_se_gate(K, name, dtype, tol, with_add):
    """BN followed by the SE excite (bottleneck_IR_SE, model_irse.py:86-87): g' = g * s[b][c] + gs[b][c] feeds the BN
    backward sums and input gradient (the bf16 case takes the lean SE kernels), vs the same algebra in fp32 on the CPU."""
    B, H, C = 5, 7, 128   # 49 rows per image: a thread's rows in flight straddle image boundaries
    HW, rows = H * H, B * H * H
    x = q(synth.normal(83, "sx", (B, C, H, H)), dtype)
    g = q(synth.normal(83, "sg", (B, C, H, H)), dtype)
    add = q(synth.normal(83, "sa", (B, C, H, H)), dtype)
    se = synth.uniform(83, "ss", (B, C), 0.1, 0.9)
    gse = synth.uniform(83, "sq", (B, C), -0.05, 0.05)
    gamma = synth.uniform(83, "sw", (C,), 0.8, 1.2)
    mean = x.mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(x.var((0, 2, 3), unbiased=False) + 1e-5)
    gp = g * se.view(B, C, 1, 1) + gse.view(B, C, 1, 1)
    xhat = (x - mean.view(1, C, 1, 1)) * invstd.view(1, C, 1, 1)
    r0, r1 = gp.sum((0, 2, 3)), (gp * xhat).sum((0, 2, 3))
    want = (gamma * invstd).view(1, C, 1, 1) * (gp - (r0 / rows).view(1, C, 1, 1) - xhat * (r1 / rows).view(1, C, 1, 1))
    if with_add:
        want = want + add
    fr, st = K.fr_dtype(torch.empty(0, dtype=dtype)), K.current_stream_ptr()
    nb = 6
    common = dict(g=nhwc(g, dtype), x=nhwc(x, dtype), mean=mean.cuda(), invstd=invstd.cuda(), se=se.cuda(),
                  gse=gse.cuda(), rows=rows, C=C, rows_per_image=HW, nblocks=nb)
    part = torch.zeros(nb, 3, C, device="cuda")
    K.bn_bwd_reduce(st, fr, part=part, **common)()
    s0, s1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    K.call("fr_reduce_parts", part, nb, 3, C, s0, s1, None, st)()
    gx = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
    extra = dict(add=nhwc(add, dtype), add_kind=1) if with_add else {}
    K.bn_bwd_apply(st, fr, gx=gx, gamma=gamma.cuda(), s0=s0, s1=s1, inv_count=1.0 / rows, **common, **extra)()
    torch.cuda.synchronize()
    np.testing.assert_allclose(s0.cpu(), r0, rtol=tol * 5, atol=tol * 20)
    np.testing.assert_allclose(s1.cpu(), r1, rtol=tol * 5, atol=tol * 20)
    assert relerr(from_nhwc(gx), want) < tol * 2


@pytest.mark.parametrize("add_kind", [0, 1, 2])
@pytest.mark.parametrize("B,H,C", [(5, 8, 64), (3, 14, 128), (37, 6, 64)])
def test_bn_backward_leaves_the_sums_of_the_batchnorm_in_front(K, B, H, C, add_kind):
    """FrBnBwdArgs.nx (round 6): fr_bn_bwd_apply also leaves the partial rows fr_bn_bwd_reduce would find with a pass of its
    own over (gx, nx) -- gx and the added rows BIT-IDENTICAL to the two launches (same rows per thread, same order)."""
    from frhip import _lib
    dtype = torch.bfloat16
    rows, HW = B * H * H, H * H
    x = q(synth.normal(89, "nx", (B, C, H, H)), dtype)
    y2 = q(synth.normal(89, "ny", (B, C, H, H), std=1.5), dtype)
    g = q(synth.normal(89, "ng", (B, C, H, H)), dtype)
    gamma = synth.uniform(89, "nw", (C,), 0.8, 1.2).cuda()
    s0 = synth.normal(89, "n0", (C,), std=3.0).cuda()
    s1 = synth.normal(89, "n1", (C,), std=3.0).cuda()
    mean, invstd = x.mean((0, 2, 3)).cuda(), (1.0 / torch.sqrt(x.var((0, 2, 3), unbiased=False) + 1e-5)).cuda()
    nmean, ninvstd = y2.mean((0, 2, 3)).cuda(), (1.0 / torch.sqrt(y2.var((0, 2, 3), unbiased=False) + 1e-5)).cuda()
    fr, st = K.fr_dtype(torch.empty(0, dtype=dtype)), K.current_stream_ptr()
    nb = 7
    kw = dict(g=nhwc(g, dtype), x=nhwc(x, dtype), mean=mean, invstd=invstd, gamma=gamma, s0=s0, s1=s1, rows=rows,
              inv_count=1.0 / rows, C=C, rows_per_image=HW, nblocks=nb)
    if add_kind == 1:
        kw.update(add=nhwc(q(synth.normal(89, "na", (B, C, H, H)), dtype), dtype), add_kind=1)
    elif add_kind == 2:
        kw.update(add=nhwc(q(synth.normal(89, "na", (B, C, H // 2, H // 2)), dtype), dtype), add_kind=2, H=H, W=H, add_stride=2)
    y2d = nhwc(y2, dtype)
    gx0 = torch.zeros(B, H, H, C, device="cuda", dtype=dtype)
    K.bn_bwd_apply(st, fr, gx=gx0, **kw)()
    part0 = torch.zeros(nb, 3, C, device="cuda")
    K.bn_bwd_reduce(st, fr, part=part0, g=gx0, x=y2d, mean=nmean, invstd=ninvstd, rows=rows, C=C, rows_per_image=HW,
                    nblocks=nb)()
    a0, a1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    K.call("fr_reduce_parts", part0, nb, 3, C, a0, a1, None, st)()
    gx1 = torch.full((B, H, H, C), 7.0, device="cuda", dtype=dtype)
    part1 = torch.full((nb, 2, C), 7.0, device="cuda")
    K.bn_bwd_apply(st, fr, gx=gx1, nx=y2d, nmean=nmean, ninvstd=ninvstd, npart=part1, **kw)()
    b0, b1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    K.call("fr_reduce_parts", part1, nb, 2, C, b0, b1, None, st)()
    torch.cuda.synchronize()
    assert torch.equal(gx0, gx1)
    assert torch.equal(part0[:, :2], part1)
    assert torch.equal(a0, b0) and torch.equal(a1, b1)
    gq = from_nhwc(gx0).double()
    xh = (y2.double() - nmean.cpu().double().view(1, C, 1, 1)) * ninvstd.cpu().double().view(1, C, 1, 1)
    mag = gq.abs().sum((0, 2, 3)) + 1e-9
    assert float(((b0.cpu().double() - gq.sum((0, 2, 3))).abs() / mag).max()) < 2e-6
    assert float(((b1.cpu().double() - (gq * xh).sum((0, 2, 3))).abs() / (gq * xh).abs().sum((0, 2, 3))).max()) < 2e-6
    with pytest.raises(_lib.FrhipError):  # fp32 has no such kernel: refused, never a silent second pass
        K.bn_bwd_apply(st, K.FR_F32, gx=gx1.float(), nx=y2d, nmean=nmean, ninvstd=ninvstd, npart=part1,
                       **dict(kw, g=kw["g"].float(), x=kw["x"].float()))()


@pytest.mark.parametrize("name,dtype,tol", DT)
@pytest.mark.parametrize("B,H,C", [(5, 7, 128), (3, 14, 256), (130, 4, 64)])
def test_se_backward_leaves_the_sums_of_bn2(K, name, dtype, tol, B, H, C):
    """Round 6: fr_se_gscale_mlp_bwd_sums == fr_se_gscale_mlp_bwd (gz, gh, gpooled bit for bit: same squeeze, same MLP) AND its
    per-image rows add up to what fr_bn_bwd_reduce(se, gse) finds with a pass of its own over (g, x): behind the excite gate
    BatchNorm2d(depth) of bottleneck_IR_SE (backbone/model_irse.py:76-80, 86-87) sees g' = g * s + gse, constant over an
    image.  Also against the same algebra in float64 on the host."""
    HW, rows, R = H * H, B * H * H, max(C // 16, 1)
    x = q(synth.normal(87, "x", (B, C, H, H)), dtype)
    g = q(synth.normal(87, "g", (B, C, H, H)), dtype)
    gamma, beta = synth.uniform(87, "w", (C,), 0.8, 1.2), synth.uniform(87, "b", (C,), -0.2, 0.2)
    mean = x.mean((0, 2, 3))
    invstd = 1.0 / torch.sqrt(x.var((0, 2, 3), unbiased=False) + 1e-5)
    scale = gamma * invstd
    shift = beta - mean * scale
    w1, w2 = synth.normal(87, "w1", (R, C)) * 0.2, synth.normal(87, "w2", (C, R)) * 0.2
    s_gate = synth.uniform(87, "s", (B, C), 0.1, 0.9)
    hidden = synth.uniform(87, "h", (B, R), -0.5, 1.0).clamp_min(0.0)
    pooled = synth.normal(87, "p", (B, C))
    fr, st = K.fr_dtype(torch.empty(0, dtype=dtype)), K.current_stream_ptr()
    dev = lambda t: t.cuda().contiguous()  # noqa: E731
    gd, xd = nhwc(g, dtype), nhwc(x, dtype)
    S = int(K.lib.fr_se_gscale_slices(B, HW))
    outs = []
    for sums in (False, True):
        gpooled, gz, gh = torch.zeros(B, C, device="cuda"), torch.zeros(B, C, device="cuda"), torch.zeros(B, R, device="cuda")
        gs_part = torch.zeros(B * S * 4 * C, device="cuda")
        bn_part = torch.zeros(B, 2, C, device="cuda")
        if sums:
            K.call("fr_se_gscale_mlp_bwd_sums", gd, xd, dev(scale), dev(shift), dev(mean), dev(invstd), dev(s_gate), dev(hidden),
                   dev(w1), dev(w2), gpooled, gz, gh, gs_part, bn_part, B, C, R, HW, fr, st)()
        else:
            K.call("fr_se_gscale_mlp_bwd", gd, xd, dev(scale), dev(shift), dev(s_gate), dev(hidden), dev(pooled), dev(w1), dev(w2),
                   gpooled, None, None, gz, gh, gs_part, B, C, R, HW, fr, st)()
        torch.cuda.synchronize()
        outs.append((gpooled, gz, gh, bn_part))
    for a, b in zip(outs[0][:3], outs[1][:3]):
        assert torch.equal(a, b) and float(a.abs().max()) > 0
    gpooled, bn_part = outs[1][0], outs[1][3]
    s0, s1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    K.call("fr_reduce_parts", bn_part, B, 2, C, s0, s1, None, st)()
    nb = 6
    part = torch.zeros(nb, 3, C, device="cuda")
    K.bn_bwd_reduce(st, fr, part=part, g=gd, x=xd, mean=dev(mean), invstd=dev(invstd), se=dev(s_gate), gse=gpooled, rows=rows,
                    C=C, rows_per_image=HW, nblocks=nb)()
    r0, r1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    K.call("fr_reduce_parts", part, nb, 3, C, r0, r1, None, st)()
    torch.cuda.synchronize()
    gp = g.double() * s_gate.double().view(B, C, 1, 1) + gpooled.cpu().double().view(B, C, 1, 1)
    xhat = (x.double() - mean.double().view(1, C, 1, 1)) * invstd.double().view(1, C, 1, 1)
    t0, t1 = gp.sum((0, 2, 3)), (gp * xhat).sum((0, 2, 3))
    mag = (gp.abs().sum((0, 2, 3)) + 1.0)
    for got, ref_pass, truth in ((s0, r0, t0), (s1, r1, t1)):
        assert float(((got.cpu().double() - truth).abs() / mag).max()) < 2e-6, "sums from the squeeze pass vs float64"
        assert float(((ref_pass.cpu().double() - truth).abs() / mag).max()) < 2e-6, "fr_bn_bwd_reduce vs float64"


BIAS_RES_CASES = [("igemm_f32", torch.float32, 64, 10, 1), ("igemm_bf16", torch.bfloat16, 64, 10, 1),
                  ("igemm_f32_s2", torch.float32, 128, 12, 2), ("strip_256_14", torch.bfloat16, 256, 14, 1),
                  ("strip_128_28", torch.bfloat16, 128, 28, 1), ("roll64_56", torch.bfloat16, 64, 56, 1),
                  ("s2_128_56", torch.bfloat16, 128, 56, 2), ("s2_512_14", torch.bfloat16, 512, 14, 2)]


@pytest.mark.parametrize("name,dtype,C,H,stride", BIAS_RES_CASES, ids=[c[0] for c in BIAS_RES_CASES])
def test_conv_bias_residual_epilogue(K, name, dtype, C, H, stride):
    """FR_EPI_BIAS_RES (inference, BatchNorm folded into the weights): out = conv(PReLU(y1)) + a[n] + b[n] + shortcut, on
    every kernel that serves conv2 of a residual unit -- generic implicit GEMM (both dtypes), LDS strip, rolling 64-channel
    kernel, stride-2 strip -- against CPU F.conv2d."""
    B = 3
    tol = 2e-4 if dtype == torch.float32 else BF16_TOL
    Ho = H // stride
    y1 = q(synth.normal(81, "br.y", (B, C, H, H)), dtype)
    w = q(synth.normal(81, "br.w", (C, C, 3, 3), std=0.05), dtype)
    slope = synth.uniform(81, "br.s", (C,), 0.1, 0.4)
    a, b2 = synth.uniform(81, "br.a", (C,), -0.5, 0.5), synth.uniform(81, "br.b", (C,), -0.5, 0.5)
    res = q(synth.normal(81, "br.r", (B, C, Ho, Ho)), dtype)
    xin = q(torch.where(y1 > 0, y1, y1 * slope.view(1, -1, 1, 1)), dtype)
    ref = F.conv2d(xin, w, stride=stride, padding=1) + (a + b2).view(1, -1, 1, 1) + res
    out = torch.zeros(B, Ho, Ho, C, device="cuda", dtype=dtype)
    kw = dict(src=nhwc(y1, dtype), w=pack_w(w, dtype), out=out, B=B, RH=Ho, RW=Ho, SH=H, SW=H, SC=C, N=C, KH=3, KW=3,
              stride=stride, pad=1, mode=0, lda=C, ldc=C, ldaux=C, pro=K.PRO_PRELU, pro_a=slope.cuda(),
              epi=K.EPI_BIAS_RES, epi_a=a.cuda(), epi_b=b2.cuda(), aux=nhwc(res, dtype))
    st = K.current_stream_ptr()
    if name.startswith("igemm"):
        K.conv(st, K.fr_dtype(torch.empty(0, dtype=dtype)), **kw)()
    elif name.startswith("s2"):
        assert K.s2_strip_parts(B, C, C, Ho, 0) > 0
        K.conv_s2_strip(st, **kw)()
    else:
        assert K.strip_parts(B, C, C, H, K.EPI_BIAS_RES) > 0
        K.conv_strip(st, **kw)()
    torch.cuda.synchronize()
    assert relerr(from_nhwc(out), ref) < tol


# ------------------------------------------------------------------------------------------------ in-launch reductions


def _bn_outputs(C):
    return [torch.zeros(C, device="cuda") for _ in range(4)]


def ops_epi(name):
    from frhip import _lib
    return getattr(_lib, "EPI_" + name)


# ------------------------------------------------------------------------------------------------ BN2 backward in the data gradient


# ------------------------------------------------------------------------------------------------ residual sum formed by its consumer


@pytest.mark.parametrize("B,C,W,Cn", [(162, 256, 14, 256), (6, 256, 14, 256), (40, 128, 28, 128), (12, 512, 7, 512),
                                      (16, 512, 7, 512), (3, 512, 7, 512), (40, 128, 28, 256), (162, 256, 14, 512),
                                      (6, 256, 14, 512)])
def test_residual_sum_by_its_consumer_and_statistics_from_moments(K, B, C, W, Cn):
    """Round 4: the forward pass of an identity unit without the BN-apply pass behind conv2.
    (1) FR_EPI_STATS_X: conv2 stores y2 and the (sum, sum of squares) rows exactly as FR_EPI_STATS does, plus the cross
        moment sum(y2 * x) with the unit's input x.
    (2) fr_bn_finalize_res: BN2's coefficients and running statistics bit-identical to fr_bn_finalize on the same rows; the
        statistics of out = a*y2 + b + x (the NEXT unit's BN1) derived from the moments agree with the statistics fr_bn_apply
        measures on the materialised tensor.
    (3) FR_PRO_RESBN: the next conv1 forms out from (y2, x), stores it once per pixel -- bit-identical to fr_bn_apply's
        tensor -- and its own result is bit-identical to conv1 with the FR_PRO_BN prologue on that tensor.
    Instances as in the BNBWD2 test (whole images, channel-split workgroups, 7-row strips, multi-image 7x7 workgroups), and
    Cn != C: the consumer is the first convolution of the next stage (128 -> 256 @28; 256 -> 512 @14 = two passes over 256
    output channels, the second one reading the tensor the first one stored).
    Reference: bottleneck_IR.forward, backbone/model_irse.py:57-66 (BN -> conv -> PReLU -> conv -> BN, res + shortcut)."""
    from frhip import _lib
    if not _lib.lib.fr_conv3x3_strip_serves_resbn(B, C, W):
        pytest.skip("not served")
    st, bf, fr = K.current_stream_ptr(), torch.bfloat16, _lib.FR_BF16
    rows = B * W * W
    dev = lambda t: t.cuda()  # noqa: E731
    x = dev((synth.normal(67, "x", (rows, C)) * 1.3 + 0.2).to(bf))       # the unit's input (residual term)
    y1 = dev(synth.normal(67, "y1", (rows, C)).to(bf))
    w2 = dev((synth.normal(67, "w2", (C, 9, C)) * 0.03).to(bf))
    w1n = dev((synth.normal(67, "w1n", (Cn, 9, C)) * 0.03).to(bf))
    slope = dev(synth.uniform(67, "sl", (C,), 0.1, 0.4))
    vec = lambda n, lo, hi: dev(synth.uniform(67, n, (C,), lo, hi))  # noqa: E731
    g2, b2, g1n, b1n = vec("g2", 0.5, 1.5), vec("b2", -0.3, 0.3), vec("g1n", 0.5, 1.5), vec("b1n", -0.3, 0.3)
    # statistics of x as the unit's own BN1 holds them
    nb = K.grid_blocks(rows, C, fr)
    px = torch.zeros(nb, 2, C, device="cuda")
    K.call("fr_channel_stats", x, rows, C, px, nb, fr, st)()
    bnx = [torch.zeros(C, device="cuda") for _ in range(4)]
    K.call("fr_bn_finalize", px, nb, C, float(rows), None, None, 1e-5, 0.1, None, None, None, *bnx, st)()
    conv2 = dict(src=y1, w=w2, B=B, RH=W, RW=W, SH=W, SW=W, SC=C, N=C, KH=3, KW=3, stride=1, pad=1, mode=0, lda=C, ldc=C,
                 ldaux=C, pro=_lib.PRO_PRELU, pro_a=slope)
    nparts = K.strip_parts(B, C, C, W, _lib.EPI_STATS_X)
    assert nparts == K.strip_parts(B, C, C, W, _lib.EPI_STATS)
    # ---- (1)
    y2a, pa = torch.zeros(rows, C, device="cuda", dtype=bf), torch.zeros(nparts, 2, C, device="cuda")
    y2b, pb = torch.zeros(rows, C, device="cuda", dtype=bf), torch.zeros(nparts, 3, C, device="cuda")
    K.conv_strip(st, out=y2a, part=pa, epi=_lib.EPI_STATS, **conv2)()
    K.conv_strip(st, out=y2b, part=pb, epi=_lib.EPI_STATS_X, aux=x, **conv2)()
    torch.cuda.synchronize()
    assert torch.equal(y2a, y2b) and torch.equal(pa, pb[:, :2].contiguous())
    cross_ref = (y2b.double() * x.double()).sum(0)
    sq_ref = (y2b.double() ** 2).sum(0)
    cross = pb[:, 2].double().sum(0)
    # (the kernel multiplies the fp32 accumulators, the reference their bf16 roundings: 2^-9 relative per term, random sign)
    assert float((cross - cross_ref).abs().max()) < 2e-3 * float(torch.sqrt(sq_ref * (x.double() ** 2).sum(0)).max())
    # ---- (2)
    rm = [torch.zeros(C, device="cuda") for _ in range(4)]
    rv = [torch.ones(C, device="cuda") for _ in range(4)]
    nbt = [torch.zeros(1, dtype=torch.int64, device="cuda") for _ in range(4)]
    bn2a = [torch.zeros(C, device="cuda") for _ in range(4)]
    bn2b = [torch.zeros(C, device="cuda") for _ in range(4)]
    bn1a = [torch.zeros(C, device="cuda") for _ in range(4)]
    bn1b = [torch.zeros(C, device="cuda") for _ in range(4)]
    K.call("fr_bn_finalize", pa, nparts, C, float(rows), g2, b2, 1e-5, 0.1, rm[0], rv[0], nbt[0], *bn2a, st)()
    K.call("fr_bn_finalize_res", pb, nparts, C,
           K.bn_fin(rows, g2, b2, 1e-5, 0.1, rm[1], rv[1], nbt[1], *bn2b), bnx[0], bnx[1], 1e-5,
           K.bn_fin(rows, g1n, b1n, 1e-5, 0.1, rm[3], rv[3], nbt[3], *bn1b), st)()
    # the two-pass path: out = BN2(y2) + x with the statistics of what was stored, then their finalize
    out_ref = torch.zeros(rows, C, device="cuda", dtype=bf)
    po = torch.zeros(nb, 2, C, device="cuda")
    K.bn_apply(st, fr, x=y2a, out=out_ref, scale=bn2a[2], shift=bn2a[3], part=po, B=B, H=W, W=W, C=C, nblocks=nb, res=x,
               res_kind=1, res_stride=1)()
    K.call("fr_bn_finalize", po, nb, C, float(rows), g1n, b1n, 1e-5, 0.1, rm[2], rv[2], nbt[2], *bn1a, st)()
    torch.cuda.synchronize()
    for a, b in zip(bn2a, bn2b):
        assert torch.equal(a, b)
    assert torch.equal(rm[0], rm[1]) and torch.equal(rv[0], rv[1]) and int(nbt[1]) == 1 and int(nbt[3]) == 1
    std = 1.0 / bn1a[1]
    # the moments see conv2's fp32 accumulators, the pass over the tensor their bf16 roundings (2^-9 relative per element,
    # random sign): the two means differ by that noise averaged over the pixels of a channel (3.4e-4 sigma at 588 pixels)
    noise = 8 * 2.0 ** -9 / rows ** 0.5
    assert float(((bn1b[0] - bn1a[0]).abs() / std).max()) < 1e-4 + noise, "mean of the residual sum from moments"
    assert float((bn1b[1] / bn1a[1] - 1).abs().max()) < 3e-4 + noise, "invstd of the residual sum from moments"
    assert float((bn1b[2] / bn1a[2] - 1).abs().max()) < 3e-4 + noise
    assert float((bn1b[3] - bn1a[3]).abs().max()) < (1e-3 + noise) * float(bn1a[3].abs().max() + 1)
    # (running_var moves by momentum x the difference of the variances: measured 1.4e-4 at 1176 pixels per channel)
    assert float((rm[3] - rm[2]).abs().max()) < (1e-4 + noise) * float(std.max())
    assert float((rv[3] / rv[2] - 1).abs().max()) < 2e-4 + noise
    # ---- (3)
    conv1 = dict(w=w1n, B=B, RH=W, RW=W, SH=W, SW=W, SC=C, N=Cn, KH=3, KW=3, stride=1, pad=1, mode=0, lda=C, ldc=Cn,
                 epi=_lib.EPI_STORE)
    z0, z1 = torch.zeros(rows, Cn, device="cuda", dtype=bf), torch.zeros(rows, Cn, device="cuda", dtype=bf)
    K.conv_strip(st, src=out_ref, out=z0, pro=_lib.PRO_BN, pro_a=bn1a[2], pro_b=bn1a[3], **conv1)()
    out1 = torch.full((rows, C), float("nan"), device="cuda", dtype=bf)
    K.conv_strip(st, src=y2a, src2=x, pro_out=out1, out=z1, pro=_lib.PRO_RESBN, pro_a=bn2a[2], pro_b=bn2a[3],
                 pro_c=bn1a[2], pro_d=bn1a[3], **conv1)()
    torch.cuda.synchronize()
    assert not torch.isnan(out1.float()).any(), "pro_out has pixels nobody wrote"
    assert torch.equal(out1, out_ref), "the residual stream formed by conv1 differs from fr_bn_apply's"
    assert torch.equal(z1, z0)
    # refused: without the second source / the output pointer, as a data gradient, with a tail on the cross-moment rows
    with pytest.raises(_lib.FrhipError):
        K.conv_strip(st, src=y2a, out=z1, pro=_lib.PRO_RESBN, pro_a=bn2a[2], pro_b=bn2a[3], pro_c=bn1a[2], pro_d=bn1a[3],
                     **conv1)()
    with pytest.raises(_lib.FrhipError):
        K.conv_strip(st, out=y2b, part=pb, epi=_lib.EPI_STATS_X, **conv2)()


@pytest.mark.parametrize("B,C,W,Cn", [(162, 256, 14, 256), (6, 256, 14, 256), (40, 128, 28, 128), (40, 128, 28, 256),
                                      (6, 256, 14, 512)])
def test_residual_sum_behind_a_squeeze_excite_unit(K, B, C, W, Cn):
    """The squeeze-excite form of the test above: out = gate[image][c] * BN2(y2) + x.
    fr_bn_finalize_res(next = NULL) on rows of three vectors == fr_bn_finalize on rows of two; fr_image_moments against torch;
    fr_se_pool_parts_mlp_fwd_res gives the pooled vector, hidden layer and gates of fr_se_pool_parts_mlp_fwd bit for bit and
    per-image moments of `out` that agree with the materialised tensor (fr_bn_apply with the gates); the next BatchNorm's
    statistics from those moments agree with the ones fr_bn_apply measures; FR_PRO_RESBN_SE forms the same tensor bit for bit.
    Reference: bottleneck_IR_SE.forward, backbone/model_irse.py:84-91, SEModule :23-46."""
    from frhip import _lib
    st, bf, fr = K.current_stream_ptr(), torch.bfloat16, _lib.FR_BF16
    rows, HW, R = B * W * W, W * W, C // 16
    dev = lambda t: t.cuda()  # noqa: E731
    x = dev((synth.normal(71, "x", (rows, C)) * 1.3 + 0.2).to(bf))
    y1 = dev(synth.normal(71, "y1", (rows, C)).to(bf))
    w2 = dev((synth.normal(71, "w2", (C, 9, C)) * 0.03).to(bf))
    w1n = dev((synth.normal(71, "w1n", (Cn, 9, C)) * 0.03).to(bf))
    fc1, fc2 = dev(synth.normal(71, "fc1", (R, C)) * 0.2), dev(synth.normal(71, "fc2", (C, R)) * 0.5)
    slope = dev(synth.uniform(71, "sl", (C,), 0.1, 0.4))
    vec = lambda n, lo, hi: dev(synth.uniform(71, n, (C,), lo, hi))  # noqa: E731
    g2, b2, g1n, b1n = vec("g2", 0.5, 1.5), vec("b2", -0.3, 0.3), vec("g1n", 0.5, 1.5), vec("b1n", -0.3, 0.3)
    conv2 = dict(src=y1, w=w2, B=B, RH=W, RW=W, SH=W, SW=W, SC=C, N=C, KH=3, KW=3, stride=1, pad=1, mode=0, lda=C, ldc=C,
                 ldaux=C, pro=_lib.PRO_PRELU, pro_a=slope)
    nparts = K.strip_parts(B, C, C, W, _lib.EPI_STATS_X)
    assert nparts % B == 0
    y2, pa = torch.zeros(rows, C, device="cuda", dtype=bf), torch.zeros(nparts, 2, C, device="cuda")
    y2b, pb = torch.zeros(rows, C, device="cuda", dtype=bf), torch.zeros(nparts, 3, C, device="cuda")
    K.conv_strip(st, out=y2, part=pa, epi=_lib.EPI_STATS, **conv2)()
    K.conv_strip(st, out=y2b, part=pb, epi=_lib.EPI_STATS_X, aux=x, **conv2)()
    bn2a = [torch.zeros(C, device="cuda") for _ in range(4)]
    bn2b = [torch.zeros(C, device="cuda") for _ in range(4)]
    K.call("fr_bn_finalize", pa, nparts, C, float(rows), g2, b2, 1e-5, 0.1, None, None, None, *bn2a, st)()
    K.call("fr_bn_finalize_res", pb, nparts, C, K.bn_fin(rows, g2, b2, 1e-5, 0.1, None, None, None, *bn2b), None,
           None, 0.0, None, st)()
    xm = torch.zeros(B, 2, C, device="cuda")
    K.call("fr_image_moments", x, B, HW, C, xm, st)()
    mk = lambda *sh: torch.zeros(*sh, device="cuda")  # noqa: E731
    pooled0, hidden0, s0 = mk(B, C), mk(B, R), mk(B, C)
    pooled1, hidden1, s1, om = mk(B, C), mk(B, R), mk(B, C), mk(B, 2, C)
    K.call("fr_se_pool_parts_mlp_fwd", pa, nparts // B, bn2a[2], bn2a[3], fc1, fc2, pooled0, hidden0, s0, B, HW, C, R, st)()
    K.call("fr_se_pool_parts_mlp_fwd_res", pb, nparts // B, 3, bn2b[2], bn2b[3], fc1, fc2, pooled1, hidden1, s1, B, HW, C, R,
           xm, om, st)()
    # the two-pass path
    nb = K.grid_blocks(rows, C, fr)
    out_ref, po = torch.zeros(rows, C, device="cuda", dtype=bf), torch.zeros(nb, 2, C, device="cuda")
    K.bn_apply(st, fr, x=y2, out=out_ref, scale=bn2a[2], shift=bn2a[3], part=po, B=B, H=W, W=W, C=C, nblocks=nb, res=x,
               res_kind=1, res_stride=1, se=s0)()
    bn1a = [torch.zeros(C, device="cuda") for _ in range(4)]
    bn1b = [torch.zeros(C, device="cuda") for _ in range(4)]
    K.call("fr_bn_finalize", po, nb, C, float(rows), g1n, b1n, 1e-5, 0.1, None, None, None, *bn1a, st)()
    K.call("fr_bn_finalize", om, B, C, float(rows), g1n, b1n, 1e-5, 0.1, None, None, None, *bn1b, st)()
    torch.cuda.synchronize()
    assert torch.equal(y2, y2b)
    for a, b in zip(bn2a, bn2b):
        assert torch.equal(a, b)
    assert torch.equal(pooled0, pooled1) and torch.equal(hidden0, hidden1) and torch.equal(s0, s1)
    assert float(s0.min()) > 0.002 and float(s0.max()) < 0.998 and float(s0.std()) > 0.05  # gates that differ per image
    xd = x.double().view(B, HW, C)
    assert float((xm[:, 0].double() - xd.sum(1)).abs().max()) < 1e-4 * float(xd.abs().sum(1).max())
    assert float((xm[:, 1].double() / (xd ** 2).sum(1) - 1).abs().max()) < 1e-5
    od = out_ref.double().view(B, HW, C)
    sq = (od ** 2).sum(1)
    # per image: the moments see conv2's fp32 accumulators and the unrounded sum, the tensor their bf16 roundings
    assert float(((om[:, 0].double() - od.sum(1)).abs() / torch.sqrt(sq * HW)).max()) < 2e-3
    assert float((om[:, 1].double() / sq - 1).abs().max()) < 4e-3
    noise = 8 * 2.0 ** -9 / rows ** 0.5
    std = 1.0 / bn1a[1]
    assert float(((bn1b[0] - bn1a[0]).abs() / std).max()) < 1e-4 + noise
    assert float((bn1b[1] / bn1a[1] - 1).abs().max()) < 3e-4 + noise
    # FR_PRO_RESBN_SE
    conv1 = dict(w=w1n, B=B, RH=W, RW=W, SH=W, SW=W, SC=C, N=Cn, KH=3, KW=3, stride=1, pad=1, mode=0, lda=C, ldc=Cn,
                 epi=_lib.EPI_STORE)
    z0, z1 = torch.zeros(rows, Cn, device="cuda", dtype=bf), torch.zeros(rows, Cn, device="cuda", dtype=bf)
    K.conv_strip(st, src=out_ref, out=z0, pro=_lib.PRO_BN, pro_a=bn1a[2], pro_b=bn1a[3], **conv1)()
    out1 = torch.full((rows, C), float("nan"), device="cuda", dtype=bf)
    K.conv_strip(st, src=y2, src2=x, pro_out=out1, out=z1, pro=_lib.PRO_RESBN_SE, pro_a=bn2a[2], pro_b=bn2a[3],
                 pro_c=bn1a[2], pro_d=bn1a[3], pro_g=s0, **conv1)()
    torch.cuda.synchronize()
    assert not torch.isnan(out1.float()).any(), "pro_out has pixels nobody wrote"
    assert torch.equal(out1, out_ref), "the residual stream formed by conv1 differs from fr_bn_apply's"
    assert torch.equal(z1, z0)
    # refused: the multi-image 7x7 workgroups do not take per-image gates
    t = lambda *sh: torch.zeros(*sh, device="cuda", dtype=bf)  # noqa: E731
    one = torch.ones(512, device="cuda")
    with pytest.raises(_lib.FrhipError):
        K.conv_strip(st, src=t(196, 512), src2=t(196, 512), pro_out=t(196, 512), out=t(196, 512), pro=_lib.PRO_RESBN_SE,
                     pro_a=one, pro_b=one, pro_c=one, pro_d=one, pro_g=torch.ones(4, 512, device="cuda"), w=t(512, 9, 512),
                     B=4, RH=7, RW=7, SH=7, SW=7, SC=512, N=512, KH=3, KW=3, stride=1, pad=1, mode=0, lda=512, ldc=512,
                     epi=_lib.EPI_STORE)()


# ------------------------------------------------------------------------------------------------ Linear on the master weight


@pytest.mark.parametrize("B,C,HW,p", [(5, 512, 49, 0.5), (3, 128, 196, 0.0), (2, 64, 9, 0.3)])
@pytest.mark.parametrize("dname", ["bf16", "f32"])
def test_dropout_in_flatten_order_equals_the_nhwc_kernels(K, dname, B, C, HW, p):
    """fr_bn_dropout_cm / fr_dropout_bwd_cm (round 4): BatchNorm -> Dropout with the result in the reference's Flatten order
    a[b][c*HW + hw] (model_irse.py:144-146), and the way back for the gradient.  Same arithmetic and the same counter-hash
    mask as the NHWC pair, so the two layouts must hold the same bits."""
    dtype = torch.float32 if dname == "f32" else torch.bfloat16
    fr, st = K.fr_dtype(torch.empty(0, dtype=dtype)), K.current_stream_ptr()
    x = synth.normal(71, "dx", (B * HW, C)).to("cuda", dtype)
    sc, sh = synth.uniform(71, "ds", (C,), 0.5, 1.5).cuda(), synth.uniform(71, "dh", (C,), -0.3, 0.3).cuda()
    seed = 0x1234ABCD5678
    a0 = torch.zeros(B, HW * C, device="cuda", dtype=dtype)
    a1 = torch.zeros(B, C * HW, device="cuda", dtype=dtype)
    K.call("fr_bn_dropout", x, a0, sc, sh, B * HW, C, HW, float(p), seed, fr, st)()
    K.call("fr_bn_dropout_cm", x, a1, sc, sh, B, C, HW, float(p), seed, fr, st)()
    torch.cuda.synchronize()
    assert torch.equal(a0.view(B, HW, C).transpose(1, 2).contiguous().view(B, -1), a1)
    if p > 0:
        frac = float((a1 == 0).float().mean())
        assert abs(frac - p) < 0.02, frac
    g1 = synth.normal(71, "dg", (B, C * HW)).to("cuda", dtype)                     # gradient in Flatten order
    g0 = g1.view(B, C, HW).transpose(1, 2).contiguous().view(B * HW, C).clone()     # the same values, NHWC
    out = torch.zeros(B * HW, C, device="cuda", dtype=dtype)
    K.call("fr_dropout_bwd", g0, B * HW, C, HW, float(p), seed, fr, st)()           # in place
    K.call("fr_dropout_bwd_cm", g1, out, B, C, HW, float(p), seed, fr, st)()
    torch.cuda.synchronize()
    assert torch.equal(g0, out)


@pytest.mark.parametrize("B,O,Kd", [(256, 512, 25088), (5, 512, 25088), (300, 128, 2048), (17, 128, 128), (257, 512, 4736)])
def test_linear_on_the_master_weight(K, B, O, Kd):
    """fr_linear_fwd / fr_linear_dgrad (csrc/linear_gemm.hip): Linear(K, O) with the fp32 master weight as the GEMM operand
    (rounded to bf16 in registers), bf16 activations, fp32 accumulation -- against torch on the same rounded operands.
    256 x 512 x 25088 is the output layer of the bs-256 step; the others cover rows past a 64-row wave tile, a second 256-row
    block and one-slice / one-tile shapes.  Reference: nn.Linear(512*7*7, 512), backbone/model_irse.py:147."""
    from frhip import _lib
    st, bf = K.current_stream_ptr(), torch.bfloat16
    a = synth.normal(73, "la", (B, Kd)).to(bf)
    W = synth.normal(73, "lw", (O, Kd)) * 0.02
    bias = synth.uniform(73, "lb", (O,), -0.5, 0.5)
    g = synth.normal(73, "lg", (B, O)).to(bf)
    Wq = W.to(bf).float()
    ref_f = a.float() @ Wq.t() + bias
    ref_g = g.float() @ Wq
    slices = int(_lib.lib.fr_linear_slices(O, Kd))
    assert slices >= 1 and (Kd // 32) % slices == 0
    slab = torch.full((slices, B, O), float("nan"), device="cuda")
    out = torch.zeros(B, O, device="cuda")
    K.call("fr_linear_fwd", a.cuda(), W.cuda(), bias.cuda(), slab, B, O, Kd, slices, st)()
    K.call("fr_reduce_parts", slab, slices, 1, B * O, out, None, None, st)()
    ga = torch.full((B, Kd), float("nan"), device="cuda", dtype=bf)
    K.call("fr_linear_dgrad", g.cuda(), W.cuda(), ga, B, O, Kd, st)()
    torch.cuda.synchronize()
    assert not torch.isnan(slab).any() and not torch.isnan(ga.float()).any()
    assert relerr(out.cpu(), ref_f) < 2e-4          # fp32 accumulation of identical bf16 products: order only
    assert relerr(ga.float().cpu(), ref_g) < BF16_TOL
    # one slice must give the same sums (up to the order of the fp32 adds)
    slab1 = torch.zeros(1, B, O, device="cuda")
    K.call("fr_linear_fwd", a.cuda(), W.cuda(), bias.cuda(), slab1, B, O, Kd, 1, st)()
    torch.cuda.synchronize()
    assert relerr(slab1[0].cpu(), ref_f) < 2e-4


# ------------------------------------------------------------------------------------------------ implicit-GEMM tile width


@pytest.mark.parametrize("epi_name", ["STORE", "STATS", "PRELU_BWD", "BNBWD"])
@pytest.mark.parametrize("mode,N,C", [(0, 128, 64), (0, 256, 96), (1, 512, 64), (2, 128, 128)])
@pytest.mark.parametrize("dname", ["f32", "bf16"])
def test_igemm_tile_width_changes_only_the_partial_sum_order(K, dname, mode, N, C, epi_name):
    """Round-3 finding, root-caused: with the 64-wide instance of fr_conv_igemm chosen for every small
    launch, six fp32 fixture tests moved past their bars (3.2e-3 against 2e-3 on a loss of 43.8).  FRHIP_IGEMM_BN forces an
    instance; for N in {128, 256, 512}, modes 0 / 1 / 2 and the four epilogues that matter the two instances must give
    BIT-IDENTICAL outputs (same K order, same MFMA), and their per-tile partial sums must agree to fp32 summation noise
    (the 64-wide tile adds a column's 128 rows as 16 groups of 8, the 128-wide one as 8 groups of 16): no defect in the
    narrow instance's epilogue -- the fixtures' bars were within 2x of the noise of an equally valid selection."""
    import os
    from frhip import _lib
    dtype, tol = (torch.float32, 2e-4) if dname == "f32" else (torch.bfloat16, BF16_TOL)
    fr, st = K.fr_dtype(torch.empty(0, dtype=dtype)), K.current_stream_ptr()
    epi = getattr(_lib, "EPI_" + epi_name)
    B, H = 3, 10
    if mode == 2:   # stride-2 data gradient: rows = output pixels (2H x 2H), source = low-res gradient
        src_t = q(synth.normal(91, "ig.s", (B, C, H, H)), dtype)
        Ro = 2 * H
        kw = dict(B=B, RH=Ro, RW=Ro, SH=H, SW=H, SC=C, N=N, KH=3, KW=3, stride=2, pad=1, mode=2, par_h=-1, par_w=-1)
    else:
        src_t = q(synth.normal(91, "ig.s", (B, C, H, H)), dtype)
        Ro = H
        kw = dict(B=B, RH=H, RW=H, SH=H, SW=H, SC=C, N=N, KH=3, KW=3, stride=1, pad=1, mode=mode)
    w_t = q(synth.normal(91, "ig.w", (N, C, 3, 3)) * 0.1, dtype)
    rows = B * Ro * Ro
    src = nhwc(src_t, dtype)
    w = pack_w(w_t, dtype)
    aux = q(synth.normal(91, "ig.a", (rows, N)), dtype).to("cuda", dtype)
    ea, eb = synth.uniform(91, "ig.ea", (N,), -0.3, 0.3).cuda(), synth.uniform(91, "ig.eb", (N,), 0.5, 1.5).cuda()
    nparts = (4 if mode == 2 else 1) * (((rows // 4 if mode == 2 else rows) + 127) // 128)
    res = {}
    for width in ("128", "64"):
        K.set_option("FRHIP_IGEMM_BN", int(width))
        try:
            out = torch.zeros(rows, N, device="cuda", dtype=dtype)
            part = torch.zeros(nparts, 2, N, device="cuda")
            K.conv(st, fr, src=src, w=w, out=out, lda=C, ldc=N, ldaux=N, pro=0, epi=epi, aux=aux, epi_a=ea, epi_b=eb,
                   part=part if epi != _lib.EPI_STORE else None, **kw)()
            torch.cuda.synchronize()
            res[width] = (out, part)
        finally:
            K.set_option("FRHIP_IGEMM_BN", 0)
    (o128, p128), (o64, p64) = res["128"], res["64"]
    assert torch.equal(o128, o64), "the two tile widths give different OUTPUTS"
    if epi != _lib.EPI_STORE:
        scale = float(p128.abs().max()) + 1e-12
        d = float((p128 - p64).abs().max())
        assert d <= 4e-6 * scale, (d, scale)           # fp32: order of 128 adds; identical products
        assert float(p128.abs().sum()) > 0
    if mode == 0 and epi == _lib.EPI_STORE:
        ref = F.conv2d(src_t, w_t, padding=1)
        assert relerr(from_nhwc(o64.view(B, H, H, N)), ref) < tol


# ------------------------------------------------------------------------------------------------ SE branch against autograd


@pytest.mark.parametrize("B,C,H", [(6, 256, 14), (5, 64, 9), (4, 512, 7)])
def test_se_branch_against_autograd_with_every_gate_decided(K, B, C, H):
    """The squeeze-excite branch (SEModule, backbone/model_irse.py:23-46, behind BN2: :84-87) forward and backward against
    float64 autograd on inputs whose hidden pre-activations are all at least 0.05 away from zero -- no ReLU gate hangs on a
    rounding, so the comparison is tight (2e-5 of each tensor's size, fp32 kernels) and a single wrong gate is far outside it
    (checked: the reference with ONE gate flipped is > 1e-3 away).  The full-model tests have to give the fc1 weights a loose
    bar (SE_FC1_BARS: their gates flip with the rounding of pooled means); this is the test that pins the gate logic."""
    st, fr, HW, R = K.current_stream_ptr(), K.fr_dtype(torch.empty(0)), H * H, C // 16
    for seed in range(200, 260):
        y2 = synth.normal(seed, "y2", (B, HW, C))
        g = synth.normal(seed, "g", (B, HW, C))
        scale, shift = synth.uniform(seed, "sc", (C,), 0.5, 1.5), synth.uniform(seed, "sh", (C,), -0.3, 0.3)
        w1, w2 = synth.normal(seed, "w1", (R, C), std=0.4), synth.normal(seed, "w2", (C, R), std=0.4)
        pooled = (y2.mean(1) * scale + shift)
        pre = pooled.double() @ w1.double().t()
        if float(pre.abs().min()) > 0.05 and bool((pre > 0).any()) and bool((pre < 0).any()):
            break
    else:
        pytest.fail("no seed with every hidden pre-activation away from zero")
    # float64 autograd
    W1, W2 = w1.double().requires_grad_(True), w2.double().requires_grad_(True)
    y = y2.double() * scale.double() + shift.double()
    pl = y.mean(1).requires_grad_(True)
    hid = torch.relu(pl @ W1.t())
    sg = torch.sigmoid(hid @ W2.t())
    ((y * sg[:, None, :]) * g.double()).sum().backward()
    dev = lambda t: t.cuda()  # noqa: E731
    mk = lambda *sh: torch.zeros(*sh, device="cuda")  # noqa: E731
    hidden, s = mk(B, R), mk(B, C)
    pooled_d = dev(pooled)
    K.call("fr_se_mlp_fwd", pooled_d, dev(w1), dev(w2), hidden, s, B, C, R, st)()
    gpooled, dw1, dw2, gz, gh = mk(B, C), mk(R, C), mk(C, R), mk(B, C), mk(B, R)
    K.call("fr_se_gscale_mlp_bwd", dev(g), dev(y2), dev(scale), dev(shift), s, hidden, pooled_d, dev(w1), dev(w2), gpooled,
           dw1, dw2, gz, gh, mk(B * 8 * C), B, C, R, HW, fr, st)()
    torch.cuda.synchronize()
    rel = lambda a, b: float((a.double().cpu() - b).abs().max() / b.abs().max())  # noqa: E731
    assert rel(hidden, hid.detach()) < 2e-5 and rel(s, sg.detach()) < 2e-5
    assert torch.equal(hidden.cpu() > 0, hid.detach() > 0), "a ReLU gate differs"
    assert rel(dw1, W1.grad) < 2e-5 and rel(dw2, W2.grad) < 2e-5
    assert rel(gpooled * HW, pl.grad) < 2e-5
    # sensitivity of the bar: one flipped gate
    gh64 = (gz.double().cpu() @ w2.double()) * (hid.detach() > 0)
    flip = gh64.clone()
    b0, r0 = (int(v) for v in (gh64.abs() == gh64.abs().max()).nonzero()[0])
    flip[b0, r0] = 0.0
    assert float(((flip - gh64).t() @ pl.detach()).abs().max() / W1.grad.abs().max()) > 1e-3


# ------------------------------------------------------------------------------------------------ stem without im2col rows


@pytest.mark.parametrize("Kp", [32, 64])
@pytest.mark.parametrize("M", [16 * 37 + 5, 64 * 2048 + 64 * 3 + 9])
def test_stem_two_pass_forward_equals_gemm_then_bn_apply(K, Kp, M):
    """Round 4: input_layer = Conv2d -> BatchNorm2d -> PReLU (backbone/model_irse.py:140-142) as two passes over the im2col rows.
    fr_stem_gemm(out = NULL) leaves the statistics rows of fr_stem_gemm bit for bit and stores nothing; fr_stem_gemm_bn_prelu
    stores y and z = PReLU(BN(y)) equal to fr_stem_gemm -> fr_bn_apply(slope) bit for bit (also with y = NULL), and statistics
    of z that agree with fr_bn_apply's to fp32 summation order (ragged last tile; more 16-row tiles than 4 * nblocks)."""
    st, bf = K.current_stream_ptr(), torch.bfloat16
    fr = K.fr_dtype(torch.empty(0, dtype=bf))
    rows = (synth.normal(83, "r", (M, Kp)) * 0.7).to("cuda", bf)
    w = (synth.normal(83, "w", (64, Kp)) * 0.2).to("cuda", bf)
    vec = lambda n, lo, hi: synth.uniform(83, n, (64,), lo, hi).cuda()  # noqa: E731
    scale, shift, slope = vec("sc", 0.5, 1.5), vec("sh", -0.3, 0.3), vec("sl", 0.1, 0.4)
    nb = 13
    y0, p0 = torch.zeros(M, 64, device="cuda", dtype=bf), torch.zeros(nb, 2, 64, device="cuda")
    K.call("fr_stem_gemm", rows, w, y0, p0, M, Kp, nb, st)()
    p1 = torch.zeros(nb, 2, 64, device="cuda")
    K.call("fr_stem_gemm", rows, w, None, p1, M, Kp, nb, st)()
    nba = K.grid_blocks(M, 64, fr)
    z0, pz0 = torch.zeros(M, 64, device="cuda", dtype=bf), torch.zeros(nba, 2, 64, device="cuda")
    K.bn_apply(st, fr, x=y0, out=z0, scale=scale, shift=shift, slope=slope, part=pz0, B=1, H=1, W=M, C=64, res_kind=0,
               res_stride=1, nblocks=nba)()
    y1 = torch.full((M, 64), float("nan"), device="cuda", dtype=bf)
    z1 = torch.full((M, 64), float("nan"), device="cuda", dtype=bf)
    pz1 = torch.zeros(nb, 2, 64, device="cuda")
    K.call("fr_stem_gemm_bn_prelu", rows, w, scale, shift, slope, y1, z1, pz1, M, Kp, nb, st)()
    z2, pz2 = torch.full((M, 64), float("nan"), device="cuda", dtype=bf), torch.zeros(nb, 2, 64, device="cuda")
    K.call("fr_stem_gemm_bn_prelu", rows, w, scale, shift, slope, None, z2, pz2, M, Kp, nb, st)()
    torch.cuda.synchronize()
    assert torch.equal(p0, p1) and float(p0.abs().max()) > 0
    assert torch.equal(y1, y0) and torch.equal(z1, z0) and torch.equal(z2, z0) and torch.equal(pz2, pz1)
    assert float((z0.float() < 0).float().mean()) > 0.1  # both PReLU branches taken
    ref = pz0.double().sum(0)
    got = pz1.double().sum(0)
    assert float((got[0] - ref[0]).abs().max()) < 1e-5 * float(z0.float().abs().sum(0).max())
    assert float((got[1] / ref[1] - 1).abs().max()) < 1e-5
    with pytest.raises(K._lib.FrhipError):
        K.call("fr_stem_gemm", rows, w, None, None, M, Kp, nb, st)()


@pytest.mark.parametrize("Kp", [32, 64])
@pytest.mark.parametrize("M", [64 * 5 + 23, 64 * 2048 + 64 * 3 + 9])
def test_stem_backward_on_recomputed_rows(K, Kp, M):
    """Round 4: the backward of input_layer (Conv2d -> BatchNorm2d -> PReLU, backbone/model_irse.py:140-142) without the stored
    GEMM output.  fr_stem_bwd_sums == fr_bn_bwd_reduce(slope) over (g, y) + the same fixed-order row sums (fp32 summation
    order aside: 1e-5); fr_stem_wgrad_bn_r == fr_stem_wgrad_bn, slab for slab, BIT FOR BIT (y recomputed per 64-row trip and
    rounded as the forward pass rounded it; ragged last trip, more trips than workgroups)."""
    st, bf = K.current_stream_ptr(), torch.bfloat16
    fr = K.fr_dtype(torch.empty(0, dtype=bf))
    rows = (synth.normal(85, "r", (M, Kp)) * 0.7).to("cuda", bf)
    w = (synth.normal(85, "w", (64, Kp)) * 0.2).to("cuda", bf)
    g = synth.normal(85, "g", (M, 64)).to("cuda", bf)
    vec = lambda n, lo, hi: synth.uniform(85, n, (64,), lo, hi).cuda()  # noqa: E731
    mean, invstd, gamma, slope = vec("m", -0.3, 0.3), vec("i", 0.5, 2.0), vec("ga", 0.8, 1.2), vec("sl", 0.1, 0.4)
    scale = gamma * invstd
    shift = vec("b", -0.2, 0.2) - mean * scale
    y, p = torch.zeros(M, 64, device="cuda", dtype=bf), torch.zeros(8, 2, 64, device="cuda")
    K.call("fr_stem_gemm", rows, w, y, p, M, Kp, 8, st)()
    nb = K.grid_blocks(M, 64, fr)
    pa = torch.zeros(nb, 3, 64, device="cuda")
    K.bn_bwd_reduce(st, fr, part=pa, g=g, x=y, mean=mean, invstd=invstd, scale=scale, shift=shift, slope=slope, rows=M, C=64,
                    rows_per_image=M, nblocks=nb)()
    nbs = 11
    pb = torch.zeros(nbs, 3, 64, device="cuda")
    K.call("fr_stem_bwd_sums", rows, w, g, mean, invstd, scale, shift, slope, pb, M, Kp, nbs, st)()
    torch.cuda.synchronize()
    a, b = pa.double().sum(0), pb.double().sum(0)
    mag = (g.double().abs().sum(0) * 4).clamp_min(1.0)
    assert float(((a - b).abs() / mag).max()) < 1e-5, float(((a - b).abs() / mag).max())
    assert float(a[2].abs().max()) > 0 and float(a[1].abs().max()) > 0
    s0, s1 = a[0].float().cuda(), a[1].float().cuda()
    ns = 9
    slab0, slab1 = torch.zeros(ns, 64, Kp, device="cuda"), torch.zeros(ns, 64, Kp, device="cuda")
    K.call("fr_stem_wgrad_bn", g, y, rows, mean, invstd, scale, shift, slope, gamma, s0, s1, 1.0 / M, slab0, M, Kp, ns, st)()
    K.call("fr_stem_wgrad_bn_r", g, rows, w, mean, invstd, scale, shift, slope, gamma, s0, s1, 1.0 / M, slab1, M, Kp, ns,
           st)()
    torch.cuda.synchronize()
    assert torch.equal(slab0, slab1) and float(slab0.abs().max()) > 0


@pytest.mark.parametrize("Kp", [32, 64])
@pytest.mark.parametrize("add_kind,B,H", [(2, 3, 12), (2, 37, 16), (1, 2, 10), (0, 5, 6)])
def test_stem_backward_sums_fed_by_the_first_unit(K, Kp, add_kind, B, H):
    """Round 6: fr_stem_bwd_sums_from forms the first residual unit's input gradient itself -- gx = BN1-backward(g) [+ the
    shortcut gradient: MaxPool2d(1, 2) scatter (add_kind 2) or the residual stream (add_kind 1)], backbone/model_irse.py:52-57,
    64-66 -- instead of reading it back from fr_bn_bwd_apply: gx and the partial rows are BIT-IDENTICAL to the two launches
    (ragged last tile, more tiles than waves, several images)."""
    st, bf = K.current_stream_ptr(), torch.bfloat16
    fr = K.fr_dtype(torch.empty(0, dtype=bf))
    M = B * H * H
    rows = (synth.normal(86, "r", (M, Kp)) * 0.7).to("cuda", bf)
    w = (synth.normal(86, "w", (64, Kp)) * 0.2).to("cuda", bf)
    g = synth.normal(86, "g", (M, 64)).to("cuda", bf)
    x = synth.normal(86, "x", (M, 64)).to("cuda", bf)
    add = None
    if add_kind == 1:
        add = synth.normal(86, "a1", (M, 64)).to("cuda", bf)
    elif add_kind == 2:
        add = synth.normal(86, "a2", (B * (H // 2) * (H // 2), 64)).to("cuda", bf)
    vec = lambda n, lo, hi: synth.uniform(86, n, (64,), lo, hi).cuda()  # noqa: E731
    mean, invstd, gamma, slope = vec("m", -0.3, 0.3), vec("i", 0.5, 2.0), vec("ga", 0.8, 1.2), vec("sl", 0.1, 0.4)
    scale = gamma * invstd
    shift = vec("b", -0.2, 0.2) - mean * scale
    umean, uinvstd, ugamma = vec("um", -0.3, 0.3), vec("ui", 0.5, 2.0), vec("ug", 0.8, 1.2)
    s0, s1 = vec("s0", -3.0, 3.0) * M / 50, vec("s1", -3.0, 3.0) * M / 50
    gx0 = torch.zeros(M, 64, device="cuda", dtype=bf)
    gx1 = torch.zeros_like(gx0)
    kw = dict(g=g, x=x, mean=umean, invstd=uinvstd, gamma=ugamma, s0=s0, s1=s1, rows=M, inv_count=1.0 / M, C=64,
              rows_per_image=H * H, nblocks=K.grid_blocks(M, 64, fr))
    if add_kind == 1:
        kw.update(add=add, add_kind=1)
    elif add_kind == 2:
        kw.update(add=add, add_kind=2, H=H, W=H, add_stride=2)
    K.bn_bwd_apply(st, fr, gx=gx0, **kw)()
    nbs = 7
    p0, p1 = torch.zeros(nbs, 3, 64, device="cuda"), torch.zeros(nbs, 3, 64, device="cuda")
    K.call("fr_stem_bwd_sums", rows, w, gx0, mean, invstd, scale, shift, slope, p0, M, Kp, nbs, st)()
    from frhip import _lib
    unit = K._fill(_lib.FrBnBwdArgs(), gx=gx1, **kw)
    K.call("fr_stem_bwd_sums_from", unit, rows, w, mean, invstd, scale, shift, slope, p1, M, Kp, nbs, st)()
    torch.cuda.synchronize()
    assert torch.equal(gx0, gx1) and float(gx0.float().abs().max()) > 0
    assert torch.equal(p0, p1) and float(p0.abs().max()) > 0
    # unit.x = NULL: the unit's input is the stem's own output z = PReLU(BN0(rows w^T)) -- recomputed from the rows, bit for bit
    z = torch.zeros(M, 64, device="cuda", dtype=bf)
    pz = torch.zeros(8, 2, 64, device="cuda")
    K.call("fr_stem_gemm_bn_prelu", rows, w, scale, shift, slope, None, z, pz, M, Kp, 8, st)()
    gx2, gx3 = torch.zeros_like(gx0), torch.zeros_like(gx0)
    p2, p3 = torch.zeros_like(p0), torch.zeros_like(p0)
    kwz = dict(kw, x=z)
    K.call("fr_stem_bwd_sums_from", K._fill(_lib.FrBnBwdArgs(), gx=gx2, **kwz), rows, w, mean, invstd, scale, shift, slope, p2,
           M, Kp, nbs, st)()
    K.call("fr_stem_bwd_sums_from", K._fill(_lib.FrBnBwdArgs(), gx=gx3, **dict(kwz, x=None)), rows, w, mean, invstd, scale, shift,
           slope, p3, M, Kp, nbs, st)()
    torch.cuda.synchronize()
    assert torch.equal(gx2, gx3) and torch.equal(p2, p3) and float(gx2.float().abs().max()) > 0
    # a gated / sloped BatchNorm backward is not what this entry point fuses: refused, not silently mis-computed
    bad = K._fill(_lib.FrBnBwdArgs(), gx=gx1, slope=slope, scale=scale, shift=shift, **kw)
    with pytest.raises(_lib.FrhipError):
        K.call("fr_stem_bwd_sums_from", bad, rows, w, mean, invstd, scale, shift, slope, p1, M, Kp, nbs, st)()


@pytest.mark.parametrize("fold", [False, True])
def test_pack_weights_64_tiles_equal_32_tiles(K, fold):
    """fr_pack_weights_multi (round 4): the 64 x 64-tile chunks (16-byte loads and stores; chunk index < 0) write the same bf16
    copy [Cout][tap][Cin] and transposed copy [Cin][tap][Cout] as the 32 x 32-tile chunks, bit for bit, for 3x3 and 1x1 tensors,
    with and without the per-output-channel scale of the BN-folded inference path, tensors of both kinds in one launch."""
    import ctypes
    from frhip import _lib
    st, bf = K.current_stream_ptr(), torch.bfloat16
    shapes = [(128, 9, 64), (64, 1, 128), (256, 9, 256), (96, 9, 32)]  # the last one: 32-tiles only
    ws = [synth.normal(87, "w%d" % i, sh).cuda() for i, sh in enumerate(shapes)]
    osc = [synth.uniform(87, "o%d" % i, (sh[0],), 0.5, 1.5).cuda() if fold else None for i, sh in enumerate(shapes)]

    def run(use64, frag=False):
        arr = (_lib.FrPackTensor * len(shapes))()
        outs, chunks = [], []
        for i, (co, taps, ci) in enumerate(shapes):
            wp = torch.full((co, taps, ci), float("nan"), device="cuda", dtype=bf)
            wt = torch.full((ci, taps, co), float("nan"), device="cuda", dtype=bf)
            outs.append((wp, wt))
            arr[i].w, arr[i].wp, arr[i].wt = ws[i].data_ptr(), wp.data_ptr(), wt.data_ptr()
            arr[i].oscale = osc[i].data_ptr() if fold else None
            arr[i].Cout, arr[i].taps, arr[i].Cin = co, taps, ci
            arr[i].frag = 3 if (frag and co % 64 == 0 and ci % 64 == 0) else 0
            if use64 and co % 64 == 0 and ci % 64 == 0:
                chunks.extend((i, -(t + 1)) for t in range(taps * (co // 64) * (ci // 64)))
            else:
                chunks.extend((i, t) for t in range(taps * ((co + 31) // 32) * ((ci + 31) // 32)))
        table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
        ch = torch.tensor(chunks, dtype=torch.int32).reshape(-1).cuda()
        K.call("fr_pack_weights_multi", ctypes.cast(ctypes.c_void_p(table.data_ptr()), ctypes.POINTER(_lib.FrPackTensor)), ch,
               len(chunks), _lib.FR_BF16, st)()
        torch.cuda.synchronize()
        return outs

    a, b = run(False), run(True)
    c = run(True, frag=True)  # round 6: both copies of the 64-tile tensors in MFMA-fragment order (FrPackTensor.frag)
    for i, ((wp0, wt0), (wpf, wtf)) in enumerate(zip(a, c)):
        co, taps, ci = shapes[i]
        if co % 64 == 0 and ci % 64 == 0:
            assert torch.equal(wpf.view(-1), to_frag(wp0).view(-1)) and torch.equal(wtf.view(-1), to_frag(wt0).view(-1)), shapes[i]
        else:
            assert torch.equal(wpf, wp0) and torch.equal(wtf, wt0)
    for i, ((wp0, wt0), (wp1, wt1)) in enumerate(zip(a, b)):
        assert not torch.isnan(wp1.float()).any() and not torch.isnan(wt1.float()).any(), shapes[i]
        assert torch.equal(wp0, wp1) and torch.equal(wt0, wt1), shapes[i]
        ref = ws[i] * (osc[i].view(-1, 1, 1) if fold else 1.0)
        assert torch.equal(wp0, ref.to(bf)) and torch.equal(wt0, ref.to(bf).permute(2, 1, 0).contiguous())


@pytest.mark.parametrize("Kc,N,B,Ho,stride", [(64, 128, 5, 28, 2), (128, 256, 6, 14, 2), (256, 512, 9, 7, 2), (256, 512, 40, 7, 2),
                                             (128, 64, 5, 28, 1), (256, 128, 6, 14, 1), (512, 256, 9, 7, 1), (64, 128, 3, 9, 1)])
def test_conv1x1_stream_equals_the_generic_gemm(K, Kc, N, B, Ho, stride):
    """fr_conv1x1_stream (round 4): shortcut_layer's Conv2d(in, depth, (1, 1), stride) (backbone/model_irse.py:52-56) and its
    data gradient as row-streaming GEMMs with the weights in registers.  Same MFMA K order as fr_conv_igemm, same rounding:
    the output is bit-identical; the BatchNorm partial rows (of the fp32 accumulators, as fr_conv_igemm's) agree as sums
    (another number of rows, fp32 order); against
    F.conv2d in float64; ragged last tile; refusals."""
    from frhip import _lib
    st, bf = K.current_stream_ptr(), torch.bfloat16
    H = Ho * stride
    x = synth.normal(89, "x", (B, H, H, Kc)).to("cuda", bf)
    w = (synth.normal(89, "w", (N, Kc)) * 0.1).to("cuda", bf)
    rows = B * Ho * Ho
    kw = dict(src=x, w=w, B=B, RH=Ho, RW=Ho, SH=H, SW=H, SC=Kc, N=N, KH=1, KW=1, stride=stride, pad=0, mode=0, lda=Kc, ldc=N,
              pro=0)
    o0, p0 = torch.zeros(rows, N, device="cuda", dtype=bf), torch.zeros((rows + 127) // 128, 2, N, device="cuda")
    K.conv(st, _lib.FR_BF16, out=o0, epi=_lib.EPI_STATS, part=p0, **kw)()
    nps = K.conv1x1_stream_parts(B, Ho, Ho, Kc, N)
    assert nps > 0
    o1, p1 = torch.full((rows, N), float("nan"), device="cuda", dtype=bf), torch.zeros(nps, 2, N, device="cuda")
    K.conv1x1_stream(st, out=o1, epi=_lib.EPI_STATS, part=p1, **kw)()
    o2 = torch.full((rows, N), float("nan"), device="cuda", dtype=bf)
    K.conv1x1_stream(st, out=o2, epi=_lib.EPI_STORE, **kw)()
    torch.cuda.synchronize()
    assert torch.equal(o1, o0) and torch.equal(o2, o0)
    ref = torch.nn.functional.conv2d(x.double().cpu().permute(0, 3, 1, 2), w.double().cpu().view(N, Kc, 1, 1), stride=stride)
    assert relerr(o1.double().cpu().view(B, Ho, Ho, N).permute(0, 3, 1, 2), ref) < BF16_TOL
    a, b = p0.double().sum(0), p1.double().sum(0)
    assert float((a[0] - b[0]).abs().max()) < 1e-5 * float(o0.float().abs().sum(0).max()) + 1e-6
    assert float((a[1] / b[1] - 1).abs().max()) < 1e-5
    with pytest.raises(_lib.FrhipError):  # not a served shape
        K.conv1x1_stream(st, out=o2, epi=_lib.EPI_STORE, **dict(kw, N=N // 2))()
    assert K.conv1x1_stream_parts(B, Ho, Ho, Kc, 96) == 0



def test_completion_event_of_a_launch_orders_another_stream(K):
    """fr_arm_stop_event / fr_finish_stop_event (ABI v6): the event rides on the kernel's own completion signal when the
    entry point launches exactly one kernel through FR_LAUNCH_KERNEL (fr_reduce_parts here: returns 1) and is recorded the
    ordinary way otherwise (fr_bn_finalize: returns 0) -- either way a second stream that waits for it sees the launch's
    results.  This is the edge between the main stream's data gradients and the weight-gradient stream (engine.py
    _side_after_main; reference: autograd runs both inside loss.backward(), train.py:314)."""
    from frhip import _lib
    nparts, C = 4096, 512
    part = (torch.rand(nparts, 2, C, device="cuda") + 0.5)
    ref = part.double().sum(0).float()
    main = torch.cuda.current_stream()
    side = torch.cuda.Stream()
    st = K.current_stream_ptr()
    big = torch.rand(64 * 1024 * 1024, device="cuda")
    for name, want_n in (("fr_reduce_parts", 1), ("fr_bn_finalize", 0)):
        o0, o1 = torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
        copy0 = torch.empty(C, device="cuda")
        ev = torch.cuda.Event()
        ev.record(main)  # torch allocates the hipEvent_t at the first record
        if name == "fr_reduce_parts":
            l = K.call(name, part, nparts, 2, C, o0, o1, None, st)
        else:
            l = K.call(name, part, nparts, C, float(nparts), None, None, 1e-5, 0.1, None, None, None, o0, o1,
                       torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda"), st)
        l.arm(ev, st)
        torch.cuda.synchronize()
        for _ in range(4):
            big.mul_(1.0001)  # the main stream is busy: the launch below starts late
        _lib.lib.fr_arm_stop_event(l.stop_handle)
        assert l.fn(*l.args) == 0
        n = _lib.lib.fr_finish_stop_event(l.stop_stream)
        assert n == want_n, (name, n)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            copy0.copy_(o0)
        torch.cuda.synchronize()
        if name == "fr_reduce_parts":
            np.testing.assert_allclose(copy0.cpu(), ref[0].cpu(), rtol=1e-6)
        else:
            np.testing.assert_allclose(copy0.cpu(), (ref[0] / nparts).cpu(), rtol=1e-5)
    assert _lib.lib.fr_finish_stop_event(st) < 0 and b"no event armed" in _lib.lib.fr_last_error_string()
    # Launch.__call__ does the same bracket
    o0 = torch.zeros(C, device="cuda")
    ev = torch.cuda.Event()
    ev.record(main)
    l = K.call("fr_reduce_parts", part, nparts, 2, C, o0, torch.zeros(C, device="cuda"), None, st)
    l.arm(ev, st)
    l()
    side.wait_event(ev)
    with torch.cuda.stream(side):
        got = o0.clone()
    torch.cuda.synchronize()
    np.testing.assert_allclose(got.cpu(), ref[0].cpu(), rtol=1e-6)
    with pytest.raises(_lib.FrhipError):
        K.call("fr_reduce_parts", part, nparts, 2, C, o0, o0, None, st).arm(torch.cuda.Event(), st)  # never recorded: no handle
