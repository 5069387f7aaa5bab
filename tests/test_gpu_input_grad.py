"""Gradients with respect to the input images on the HIP path: the stem's data-gradient kernel (fr_stem_dgrad) and the
adjoint of pSp's bilinear resize (fr_resize_bilinear_bwd) against float64 restatements, and x.grad of whole backbones
against the reference's gradient (g15_input_grad) and the float64 oracle.  A backward that asks for input gradients leaves
the loss, the parameter gradients, the running statistics and the plan's launch lists exactly as they are without it."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from frhip import synth  # noqa: E402

from test_gpu_model import BF16_BARS, build  # noqa: E402
from test_input_grad_host import g15_inputs, oracle_input_grad  # noqa: E402
from test_oracle_golden import build_state  # noqa: E402
from oracle import irse_ref as O  # noqa: E402

BF16_TOL = 8e-3  # the bf16 bar of the kernel tests (test_gpu_kernels.BF16_TOL)


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def K():
    from frhip import _lib, ops
    _lib.self_check()
    return ops


def relerr(a, b):
    return float((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30))


def normerr(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def cos(a, b):
    return float(F.cosine_similarity(a.double().flatten(), b.double().flatten(), dim=0))


# ------------------------------------------------------------------------------------------------ the stem kernel
def stem_dgrad_ref(G, X, W, Y, co, s0, s1, M, B, H, Wd, C, Ct, Kp):
    """float64 restatement of fr_stem_dgrad: g' = G * prelu'(u); g_y = gamma*invstd*(g' - s0/M - (y-mean)*invstd*s1/M);
    gX = g_y Wp; col2im over the 3x3 taps of the im2col layout, image channels only."""
    d = lambda t: t.double().cpu()  # noqa: E731
    G, W, Y = d(G), d(W), d(Y)
    mean, invstd, scale, shift, slope, gamma = (d(co[k]) for k in ("mean", "invstd", "scale", "shift", "slope", "gamma"))
    u = Y * scale + shift
    gp = torch.where(u > 0, G, G * slope)
    gy = gamma * invstd * (gp - d(s0) / M - (Y - mean) * invstd * d(s1) / M)
    gX = (gy @ W)[:, :9 * Ct].view(B, H, Wd, 9, Ct)
    P = F.pad(gX.permute(0, 3, 4, 1, 2), (1, 1, 1, 1))  # [B][9][Ct][H+2][W+2]
    gx = torch.zeros(B, C, H, Wd, dtype=torch.float64)
    for kh in range(3):
        for kw in range(3):
            gx += P[:, kh * 3 + kw, :C, 2 - kh:2 - kh + H, 2 - kw:2 - kw + Wd]
    return gx


STEM = [(32, 3, 3, 2, 112), (64, 3, 6, 2, 112), (32, 3, 3, 1, 224), (64, 3, 6, 1, 224), (32, 3, 3, 3, 13), (64, 3, 6, 3, 13),
        (32, 3, 3, 2, 40), (64, 3, 6, 1, 130), (32, 3, 3, 1, 253)]


@pytest.mark.parametrize("train", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("Kp,C,Ct,B,S", STEM, ids=["K%d_S%d" % (s[0], s[4]) for s in STEM])
def test_stem_dgrad_matches_float64(K, Kp, C, Ct, B, S, train):
    """bf16: y recomputed from the rows (and, with Y, read) vs float64 on the same bf16-rounded X0, Wp and G.  Row bands are
    16 image rows, column segments at most 126 (K0 = 32) / 62 (K0 = 64) pixels: 13 is one band and segment smaller than both,
    40 and 130 end in a partial band, 130 (K0 = 64: 44 + 44 + 42) and 253 (K0 = 32: 85 + 85 + 83) in a partial segment, 224
    splits into equal segments.  fp32 (y read): ~1e-5."""
    st = K.current_stream_ptr()
    M = B * S * S
    tag = "sd%d_%d_%d" % (Kp, S, train)
    vec = lambda n, lo, hi: synth.uniform(86, tag + n, (64,), lo, hi).cuda()  # noqa: E731
    co = dict(mean=vec("m", -0.3, 0.3), invstd=vec("i", 0.5, 2.0), gamma=vec("ga", 0.8, 1.2), slope=vec("sl", 0.1, 0.4))
    co["scale"] = co["gamma"] * co["invstd"]
    co["shift"] = vec("b", -0.2, 0.2) - co["mean"] * co["scale"]
    if train:
        s0, s1 = vec("s0", -1, 1) * M * 0.05, vec("s1", -1, 1) * M * 0.05
    else:
        s0 = s1 = torch.zeros(64, device="cuda")
    X = synth.normal(86, tag + "x", (M, Kp)) * 0.7
    W = synth.normal(86, tag + "w", (64, Kp)) * 0.2
    G = synth.normal(86, tag + "g", (M, 64))
    args = lambda g, x, y, w, gx, dt: (g, x, y, w, co["mean"], co["invstd"], co["scale"], co["shift"], co["slope"],  # noqa: E731
                                       co["gamma"], s0, s1, 1.0 / M, gx, B, S, S, C, Ct, Kp, dt, st)
    bf = torch.bfloat16
    Xb, Wb, Gb = X.to("cuda", bf), W.to("cuda", bf), G.to("cuda", bf)
    Yb = (Xb.float() @ Wb.float().t()).to(bf)  # what the forward pass stores / the kernel recomputes (rounded once)
    want = stem_dgrad_ref(Gb, None, Wb, Yb, co, s0, s1, M, B, S, S, C, Ct, Kp)
    for x, y in ((Xb, None), (None, Yb)):
        gx = torch.full((B, C, S, S), float("nan"), device="cuda")
        K.call("fr_stem_dgrad", *args(Gb, x, y, Wb, gx, 1))()
        torch.cuda.synchronize()
        assert relerr(gx.cpu(), want) < BF16_TOL, (x is None, relerr(gx.cpu(), want))
    Xf, Wf, Gf = X.cuda(), W.cuda(), G.cuda()
    Yf = Xf @ Wf.t()
    gx = torch.full((B, C, S, S), float("nan"), device="cuda")
    K.call("fr_stem_dgrad", *args(Gf, None, Yf, Wf, gx, 0))()
    torch.cuda.synchronize()
    want = stem_dgrad_ref(Gf, None, Wf, Yf.double(), co, s0, s1, M, B, S, S, C, Ct, Kp)
    assert relerr(gx.cpu(), want) < 1e-5


# ------------------------------------------------------------------------------------------------ resize backward
def _axis_weights(n_in, n_out):
    """[n_out][n_in]: the float32 weights ATen's bilinear resize applies along one axis (the other axis kept at scale 1)."""
    eye = torch.eye(n_in).view(1, 1, n_in, n_in)
    return F.interpolate(eye, (n_out, n_in), mode="bilinear")[0, 0].double()


@pytest.mark.parametrize("hin", [128, 96, 224, 113])
def test_resize_bilinear_bwd_matches_autograd(K, hin):
    """The adjoint of fr_resize_bilinear (the sizes of test_psp_bilinear_resize_matches_torch): against float64 autograd
    through CPU F.interpolate (which computes its source coordinates in float64, the kernels in float32 as ATen's float32
    path does: 2e-5), and against the float64 transpose of the float32 operator itself (1e-6); plus a non-square case."""
    B = 2
    g = synth.normal(87, "rb%d" % hin, (B, 3, 112, 112))
    gin = torch.full((B, 3, hin, hin), float("nan"), device="cuda")
    K.call("fr_resize_bilinear_bwd", g.cuda(), gin, B * 3, hin, hin, 112, 112, K.current_stream_ptr())()
    torch.cuda.synchronize()
    x = torch.zeros(B, 3, hin, hin, dtype=torch.float64, requires_grad=True)
    (want,) = torch.autograd.grad(F.interpolate(x, 112, mode="bilinear"), [x], g.double())
    assert relerr(gin.cpu(), want) < 2e-5
    A = _axis_weights(hin, 112)
    exact = A.t() @ g.double() @ A
    assert relerr(gin.cpu(), exact) < 1e-6
    rect = synth.normal(87, "rb.rect", (2, 1, 31, 120))
    gr = torch.full((2, 1, 50, 77), float("nan"), device="cuda")
    K.call("fr_resize_bilinear_bwd", rect.cuda(), gr, 2, 50, 77, 31, 120, K.current_stream_ptr())()
    torch.cuda.synchronize()
    exact = _axis_weights(50, 31).t() @ rect.double() @ _axis_weights(77, 120)
    assert relerr(gr.cpu(), exact) < 1e-6


# ------------------------------------------------------------------------------------------------ whole backbones
def _model(kind, train, dtype=torch.float32, size=112):
    from backbone.model_irse import IR_50, IR_SE_50
    if kind == "IR_SE_50":
        m = IR_SE_50([size, size])
        synth.fill_state_dict(m.state_dict(), 15)
        m = m.cuda()
    elif kind == "IR_50" and size != 112:
        m = IR_50([size, size])
        synth.fill_state_dict(m.state_dict(), 15)
        m = m.cuda()
    else:
        m, _ = build(kind)
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
    inner = m.encoder if kind == "pSp" else m
    inner.compute_dtype = dtype
    return m.train(train), inner


def _oracle(model, x, gfeat, train, kind, resize_to=None, dtype=torch.float64):
    """dL/dx of the oracle (float64 by default) on the module's own state (synth-filled: the same weights as the fixture)."""
    prefix = "encoder." if kind == "pSp" else ""
    sd = {k: (v.detach().to(dtype).cpu() if v.is_floating_point() else v.cpu()) for k, v in model.state_dict().items()}
    sd = {k[len(prefix):] if prefix and k.startswith(prefix) else k: v for k, v in sd.items()}
    xx = x.to(dtype).cpu().requires_grad_(True)
    h = F.interpolate(xx, resize_to, mode="bilinear") if resize_to else xx
    avg = synth.uniform(15, "avg_image", (3, 112, 112)).to(dtype) if kind == "pSp" else None
    se = kind in ("IR_SE_50", "pSp")
    f = O.backbone_forward(sd, h, num_layers=50, se=se, bn_train=train, avg_image=avg)
    (gx,) = torch.autograd.grad((f * gfeat.to(dtype).cpu()).sum(), [xx])
    return gx.double()


def _input_grad(model, x, gfeat):
    x = x.cuda().detach().requires_grad_(True)
    f = model(x)
    (f * gfeat.cuda().to(f.dtype)).sum().backward()
    torch.cuda.synchronize()
    return x.grad


def test_ir50_train_input_grad_matches_reference_fixture(golden_dir):
    """fp32, train mode, g15: x.grad against the reference's fp32 gradient and the float64 oracle; the bar is the fixture's
    own fp32-vs-float64 deviation (B = 2: batch statistics of two images make this gradient ill-conditioned)."""
    g = np.load(os.path.join(golden_dir, "g15_input_grad.npz"))
    dev = float(g["ir50_train.dev.gx"])
    model, _ = _model("IR_50", True)
    x, gfeat = g15_inputs()
    gx = _input_grad(model, x, gfeat).cpu()
    _f, want = oracle_input_grad(golden_dir, "ir50_train")
    assert relerr(gx, want) < max(2 * dev, 1e-3), (relerr(gx, want), dev)
    assert relerr(gx, torch.from_numpy(g["ir50_train.gx"])) < max(3 * dev, 1e-3)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_identity_loss_frozen_eval_backbone(golden_dir, dtype):
    """The identity-loss pattern: eval mode, every parameter frozen, gradient into the images only."""
    g = np.load(os.path.join(golden_dir, "g15_input_grad.npz"))
    model, _ = _model("IR_50", False, dtype)
    for p in model.parameters():
        p.requires_grad_(False)
    stats = {k: v.clone() for k, v in model.state_dict().items() if "running" in k or "num_batches" in k}
    x, gfeat = g15_inputs()
    gx = _input_grad(model, x, gfeat).cpu()
    _f, want = oracle_input_grad(golden_dir, "ir50_eval")
    if dtype == torch.float32:
        assert relerr(gx, want) < max(3 * float(g["ir50_eval.dev.gx"]), 1e-3), relerr(gx, want)
    else:
        assert cos(gx, want) > BF16_BARS["grad_cos"] and abs(float(gx.norm() / want.norm()) - 1) < BF16_BARS["grad_norm_ratio"]
    assert all(p.grad is None for p in model.parameters())
    for k, v in model.state_dict().items():
        if k in stats:
            assert torch.equal(v, stats[k]), k


def test_bf16_ir50_train_input_grad_tracks_float64():
    """bf16, train mode, B = 64: the two-pass stem, the fused unit-0 backward (fr_stem_bwd_sums_from) and the recomputing
    data-gradient kernel, against the float64 oracle within the bf16 gradient bars."""
    model, _ = _model("IR_50", True, torch.bfloat16)
    x = synth.uniform(88, "bf.x", (64, 3, 112, 112))
    gfeat = synth.normal(88, "bf.g", (64, 512))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    gx = _input_grad(model, x, gfeat).cpu().float()
    model.load_state_dict(state)  # the oracle starts from the same running statistics (unused in train mode anyway)
    want = _oracle(model, x, gfeat, True, "IR_50")
    c, r = cos(gx, want), float(gx.norm() / want.norm())
    assert c >= BF16_BARS["grad_cos"] and abs(r - 1) <= BF16_BARS["grad_norm_ratio"], (c, r)


FP32_CASES = [("IR_SE_50", 112, None), ("IR_50", 224, None), ("pSp", 112, None), ("pSp", 128, 112)]


@pytest.mark.parametrize("kind,size,resize", FP32_CASES, ids=["irse50", "ir50_224", "psp", "psp_resize128"])
def test_fp32_input_grad_matches_oracle(kind, size, resize):
    """fp32, eval mode: squeeze-excite units, a 224 input, pSp's 6-channel stem (K0 = 64, x.grad has the 3 image channels),
    and a 128-pixel batch resized to 112 inside pSp.forward, against the float64 oracle.  The bar is the oracle's own fp32
    deviation on the same case (3x; it reaches 2.4e-3 norm-wise / 1.1e-2 max-wise at 224 and with the resize), with floors."""
    model, _ = _model(kind, False, torch.float32, size=size if resize is None else 112)
    x = synth.uniform(89, "fp.x%s%d" % (kind, size), (2, 3, size, size))
    gfeat = synth.normal(89, "fp.g", (2, 512))
    gx = _input_grad(model, x, gfeat).cpu()
    assert gx.shape == (2, 3, size, size)
    want = _oracle(model, x, gfeat, False, kind, resize_to=resize)
    own = _oracle(model, x, gfeat, False, kind, resize_to=resize, dtype=torch.float32)
    bar_norm, bar_max = max(3 * normerr(own, want), 2e-3), max(3 * relerr(own, want), 1e-2)
    assert normerr(gx, want) < bar_norm and relerr(gx, want) < bar_max, (normerr(gx, want), relerr(gx, want), bar_norm,
                                                                         bar_max)


def _step(model, x, gfeat, with_input_grad):
    x = x.cuda().detach().requires_grad_(with_input_grad)
    for p in model.parameters():
        p.grad = None
    f = model(x)
    loss = (f * gfeat.cuda()).sum()
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.clone() for n, p in model.named_parameters()}
    bufs = {n: b.clone() for n, b in model.named_buffers()}
    return float(loss), grads, bufs, x.grad


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_input_grad_has_no_side_effects(dtype):
    """A training step with x.requires_grad: bit-identical loss, parameter gradients and running statistics; one plan and
    the same launch lists across alternating calls with and without input gradients."""
    model, inner = _model("IR_50", True, dtype)
    x, gfeat = synth.uniform(90, "se.x", (4, 3, 112, 112)), synth.normal(90, "se.g", (4, 512))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    runs = []
    plans = []
    for with_grad in (False, True, False, True):
        model.load_state_dict(state)
        runs.append(_step(model, x, gfeat, with_grad))
        plan = inner._runner[0].plan
        plans.append((plan, list(plan.bwd_list), list(plan.fwd_list), list(plan.pack_list)))
    for loss, grads, bufs, gx in runs[1:]:
        assert loss == runs[0][0]
        for n, g in grads.items():
            assert torch.equal(g, runs[0][1][n]), n
        for n, b in bufs.items():
            assert torch.equal(b, runs[0][2][n]), n
    assert runs[0][3] is None and runs[2][3] is None and runs[1][3] is not None and torch.equal(runs[1][3], runs[3][3])
    p0 = plans[0]
    for p in plans[1:]:
        assert p[0] is p0[0]
        for a, b in zip(p[1:], p0[1:]):
            assert len(a) == len(b) and all(u is v for u, v in zip(a, b))


def test_input_grad_is_reproducible():
    model, _ = _model("IR_50", True, torch.bfloat16)
    x, gfeat = synth.uniform(91, "rp.x", (8, 3, 112, 112)), synth.normal(91, "rp.g", (8, 512))
    a = _input_grad(model, x, gfeat)
    b = _input_grad(model, x, gfeat)
    assert torch.equal(a, b) and float(a.abs().max()) > 0


def test_autograd_surface():
    """bf16, non-contiguous and channels-last leaves get gradients of their own dtype and layout-independent values;
    torch.autograd.grad works; a second forward before the backward still raises."""
    model, _ = _model("IR_50", False)
    base = synth.uniform(92, "as.x", (2, 3, 112, 112)).cuda()
    ref = _input_grad(model, base, torch.ones(2, 512))
    xb = base.to(torch.bfloat16).requires_grad_(True)
    model(xb).sum().backward()
    assert xb.grad.dtype == torch.bfloat16 and xb.grad.shape == xb.shape
    xt = base.transpose(2, 3).contiguous().transpose(2, 3).detach().requires_grad_(True)  # same values, strides of a transpose
    assert not xt.is_contiguous()
    model(xt).sum().backward()
    assert xt.grad.shape == xt.shape and torch.equal(xt.grad, ref)
    xc = base.to(memory_format=torch.channels_last).requires_grad_(True)
    model(xc).sum().backward()
    assert torch.equal(xc.grad.contiguous(), ref)
    x = base.clone().requires_grad_(True)
    (g,) = torch.autograd.grad(model(x).sum(), x)
    assert torch.equal(g, ref)
    f1 = model(x)
    model(base)
    with pytest.raises(RuntimeError):
        f1.sum().backward()


def test_identity_loss_alternation_reuses_one_plan():
    """Frozen eval backbone, the identity-loss pattern: forwards without gradients (real image, target) alternate with a
    forward whose input requires grad (generated image) and its backward.  After the first call with input gradients every
    call runs on that one plan (no rebuild), and x.grad is the same in every round.  A forward without gradients between a
    forward and its backward does not touch that backward's plan: the backward still works and gives the same x.grad."""
    model, inner = _model("IR_50", False, torch.bfloat16)
    for p in model.parameters():
        p.requires_grad_(False)
    runner = inner._runner[0]
    x, y, yh = (synth.uniform(93, "il." + t, (4, 3, 112, 112)).cuda() for t in ("x", "y", "yh"))
    gfeat = synth.normal(93, "il.g", (4, 512)).cuda()
    model(x)
    plan, grads = None, []
    for _ in range(3):
        fx, fy = model(x), model(y)
        assert plan is None or runner.plan is plan
        xh = yh.clone().requires_grad_(True)
        f = model(xh)
        plan = plan or runner.plan
        assert runner.plan is plan and not plan.infer
        ((f * gfeat).sum() + (f * fx).sum() * 0 + (f * fy).sum() * 0).backward()
        torch.cuda.synchronize()
        grads.append(xh.grad)
    assert model(x) is not None and runner.plan is plan
    assert all(torch.equal(g, grads[0]) for g in grads[1:]) and float(grads[0].abs().max()) > 0
    xh = yh.clone().requires_grad_(True)
    f = model(xh)
    model(x)  # the pending backward owns the plan: this forward runs elsewhere
    (f * gfeat).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(xh.grad, grads[0])


def test_input_grad_is_not_raced_by_readiness_callbacks():
    """Data-parallel hook contract: a callback that rewrites announced gradients in place on the communication stream (what
    an all-reduce does) must change neither x.grad nor any gradient the backward pass computes after the announcement.  In
    train mode the stem's data gradient reads the stem BatchNorm's parameter gradients (s0 / s1) and, in bf16, the fused
    stem-sums launch reads those of the first unit's BN1: both are announced only after those reads."""
    model, inner = _model("IR_50", True, torch.bfloat16)
    runner = inner._runner[0]
    x, gfeat = synth.uniform(94, "dp.x", (8, 3, 112, 112)).cuda(), synth.normal(94, "dp.g", (8, 512)).cuda()
    state = {k: v.clone() for k, v in model.state_dict().items()}

    def run():
        model.load_state_dict(state)
        xx = x.clone().requires_grad_(True)
        (model(xx) * gfeat).sum().backward()
        torch.cuda.synchronize()
        return xx.grad

    want = run()
    want_p = {n: p.grad.clone() for n, p in model.named_parameters()}

    def on_ready(params):
        with torch.cuda.stream(runner.plan.comm_fence()):
            for p in params:
                p.grad.mul_(3.0)

    runner.on_grads_ready = on_ready
    try:
        for _ in range(3):
            assert torch.equal(run(), want)
            bad = [n for n, p in model.named_parameters() if not torch.equal(p.grad, want_p[n] * 3.0)]
            assert not bad, bad[:5]
    finally:
        runner.on_grads_ready = None
