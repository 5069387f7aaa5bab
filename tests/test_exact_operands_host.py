"""The exact-operand helpers without a GPU (tests/exact_operands.py).

(1) The operands of every case table of test_gpu_exact_conv.py satisfy the preconditions of exactness (assert_exact_range)
    on the float64 reference: every shape with up to three images (the generator repeats eight base images channel-rolled,
    so the range of a large batch is the range of its base images).
(2) Negative controls: the comparators, fed the reference with a planted defect, fail and say where.  Each control first
    shows that the comparator passes on the unplanted reference and that the defect changes the reference (a defect that
    touches only zeros would be a test-data failure).
"""
import pytest
import torch
import torch.nn.functional as F

import exact_operands as X
import test_gpu_kernels as T

NB = 3


def _shapes():
    s = {(c[0], c[1], c[2], 1) for c in T.STRIP_CASES + T.FRAG_CASES}
    s |= {(c[0], c[0], 2 * c[1], 2) for c in T.S2_CASES} | {(c[0], c[0], 2 * c[1], 2) for c in T.S2_FRAG_CASES}
    s |= {(c[2], c[2], c[3], c[4]) for c in T.BIAS_RES_CASES}
    return sorted(s)


@pytest.mark.parametrize("cin,cout,W,stride", _shapes(), ids=["%d_%d_%d_s%d" % s for s in _shapes()])
def test_conv_operands_are_in_the_exact_range(cin, cout, W, stride):
    """Forward with the three prologues (STATS, STATS_X, BIAS_RES) and data gradient (PRELU_BWD, BNBWD): stored values
    are bf16 numbers, the per-image sums of magnitudes times four images per part row stay below 2^23."""
    ipr = 4 if W // stride <= 7 or W <= 7 else 1
    p = X.density(cin, W)
    w = X.ternary(131, "w", (cout, 9, cin), p)
    Wo = W // stride
    xres = X.ternary(131, "xin", (NB, Wo, Wo, cout), 0.5)
    for pro in ("none", "bn", "prelu"):
        x = X.activations(131, "x." + pro, (W, W, cin), p, pro, nb=NB)
        pa, pb = X.prologue_coeffs(131, "pro", cin, pro)
        acc = X.conv_forward(X.apply_prologue(x, pro, pa, pb), w, stride)
        assert float((acc != 0).double().mean()) > 0.8, "mostly zeros: the kernel's work would not be seen"
        stored, terms = X.epilogue("stats_x", acc, xres)
        X.assert_exact_range(stored=[stored], terms=terms, images_per_row=ipr, what="fwd " + pro)
        ea, eb = X.pick(157, "ea", cout, [-1.0, 0.0, 1.0, 2.0]), X.pick(157, "eb", cout, [-2.0, 0.0, 1.0])
        stored, _ = X.epilogue("bias_res", acc, xres, ea, eb)
        X.assert_exact_range(stored=[stored], what="bias_res " + pro)
    g = X.ternary(131, "g", (NB, Wo, Wo, cout), X.density(cout, W))
    gx = X.conv_dgrad(g, w, stride, W)
    aux = X.ternary(131, "aux", (NB, W, W, cin), 0.5)
    stored, terms = X.epilogue("prelu_bwd", gx, aux, X.pick(131, "slope", cin, [0.25, 0.5]))
    X.assert_exact_range(stored=[stored], terms=terms, images_per_row=ipr, quantum=0.25, term_quantum=1.0, what="prelu_bwd")
    stored, terms = X.epilogue("bnbwd", gx, aux, X.pick(131, "mean", cin, [-1.0, 0.0, 1.0]),
                               X.pick(131, "invstd", cin, [0.5, 1.0, 2.0]))
    X.assert_exact_range(stored=[stored], terms=terms, images_per_row=ipr, term_quantum=0.5, what="bnbwd")


WG = sorted({(c[0], c[1], c[2], c[3], 1, min(c[4], 32)) for c in T.WGS_CASES} |
            {(C, C, 2 * WL, "prelu", 2, 3) for C, WL in T.S2_SHAPES})


@pytest.mark.parametrize("cout,cin,W,pro,stride,B", WG, ids=["%d_%d_%d_%s_s%d_b%d" % s for s in WG])
def test_weight_gradient_operands_are_in_the_exact_range(cout, cin, W, pro, stride, B):
    """sum |g * x| of every dW element stays below 2^23 (the bound scales with the batch: checked at the case's batch up to 32,
    and the bound itself at the largest batch of the tables, 162)."""
    x = X.batch(X.activations(163, "x", (W, W, cin), X.density(cin, W), pro), B)
    g = X.batch(X.ternary(163, "g", (X.BASE_IMAGES, W // stride, W // stride, cout), X.density(cin, W)), B)
    pa, pb = X.prologue_coeffs(163, "pro", cin, pro)
    bound = X.wgrad_abs_bound(g, X.apply_prologue(x, pro, pa, pb))
    X.assert_exact_range(wgrad_abs=bound, what="wgrad")
    X.assert_exact_range(wgrad_abs=bound * (162.0 / B if W <= 14 else 1.0), what="wgrad at the largest batch")


def test_residual_sum_operands_are_in_the_exact_range():
    for C, W, Cn in sorted({(c[1], c[2], c[3]) for c in T.test_residual_sum_behind_a_squeeze_excite_unit.pytestmark[0].args[1]} |
                           {(c[1], c[2], c[3]) for c in
                            T.test_residual_sum_by_its_consumer_and_statistics_from_moments.pytestmark[0].args[1]}):
        for se in (False, True):
            p = X.density(C, W) * (0.3 if se else 0.5)
            y2, x2 = X.ternary(141, "y2", (NB, W, W, C), p).double(), X.ternary(141, "x2", (NB, W, W, C), p).double()
            a, b = X.prologue_coeffs(141, "ab", C, "bn")
            c, d = X.prologue_coeffs(141, "cd", C, "bn")
            o = y2 * a.double() + b.double()
            if se:
                o = o * X.pick(141, "gate", NB * C, [0.5, 1.0, 2.0]).double().view(NB, 1, 1, C)
            o = o + x2
            q = 0.5 if se else 1.0
            X.assert_exact_range(stored=[o], quantum=q, what="residual sum")
            acc = X.conv_forward(X.apply_prologue(o, "bn", c, d), X.ternary(141, "w1n", (Cn, 9, C), X.density(C, W)))
            X.assert_exact_range(stored=[acc], quantum=q, what="conv1 behind the residual sum")


def test_range_check_refuses_what_is_not_exact():
    ok = torch.full((1, 2, 2, 4), 3.0)
    X.assert_exact_range(stored=[ok], terms=[ok])
    for bad in (dict(stored=[ok * 100]), dict(stored=[ok + 0.5]), dict(stored=[ok * 0.5 + 128.0], quantum=0.5),
                dict(terms=[ok * 2.0 ** 21]), dict(terms=[ok * 2.0 ** 20], images_per_row=4), dict(wgrad_abs=2.0 ** 23 + 1)):
        with pytest.raises(AssertionError):
            X.assert_exact_range(**bad)


# ------------------------------------------------------------------------------------------------------------ negative controls
B, H, C, O = 3, 20, 64, 64


@pytest.fixture(scope="module")
def ref():
    p = X.density(C)
    x = X.apply_prologue(X.activations(201, "x", (H, H, C), p, "bn", nb=B), "bn", *X.prologue_coeffs(201, "pro", C, "bn"))
    w = X.ternary(201, "w", (O, 9, C), p)
    acc = X.conv_forward(x, w)
    g = X.ternary(201, "g", (B, H, H, O), p)
    return dict(x=x, w=w.double(), acc=acc, terms=X.epilogue("stats", acc)[1], dw=X.conv_wgrad(g, x))


def _tap(x, w, kh, kw, b, h, col, chans=slice(None)):
    """Contribution of tap (kh, kw), input column `col`, to output pixel (b, h, .) -- [O]."""
    r = h + kh - 1
    if r < 0 or r >= x.shape[1] or col < 0 or col >= x.shape[2]:
        return torch.zeros(w.shape[0], dtype=torch.float64)
    return w[:, kh * 3 + kw, chans] @ x[b, r, col, chans]


def _zero_pixel(r):
    bad = r["acc"].clone()
    bad[1, 7, 9] = 0.0
    return bad


def _shifted_tap_at_the_right_border(r):
    bad = r["acc"].clone()
    for b in range(B):
        for h in range(H):  # tap (1, 0) of the last column reads column H - 3 instead of H - 2
            bad[b, h, H - 1] += _tap(r["x"], r["w"], 1, 0, b, h, H - 3) - _tap(r["x"], r["w"], 1, 0, b, h, H - 2)
    return bad


def _swapped_last_rows(r):
    bad = r["acc"].clone()
    bad[0, H - 1], bad[1, H - 1] = r["acc"][1, H - 1], r["acc"][0, H - 1]
    return bad


def _dropped_k_chunk(r):
    bad = r["acc"].clone()
    bad[2, 5, 6] -= _tap(r["x"], r["w"], 2, 1, 2, 5, 6, slice(32, 64))
    return bad


OUTPUT_DEFECTS = [(_zero_pixel, "image 1, row 7, column 9", None),
                  (_shifted_tap_at_the_right_border, "column %d" % (H - 1), "border 100%"),
                  (_swapped_last_rows, "image 0, row %d" % (H - 1), "image boundary rows 100%"),
                  (_dropped_k_chunk, "image 2, row 5, column 6", None)]


@pytest.mark.parametrize("plant,where,cluster", OUTPUT_DEFECTS, ids=[d[0].__name__.strip("_") for d in OUTPUT_DEFECTS])
def test_output_comparator_catches(ref, plant, where, cluster):
    X.assert_equal_nhwc(ref["acc"].clone().to(torch.bfloat16), ref["acc"], "control")  # without the defect: equal
    bad = plant(ref)
    assert not torch.equal(bad, ref["acc"]), "the planted defect changed nothing: test data"
    with pytest.raises(AssertionError) as e:
        X.assert_equal_nhwc(bad.to(torch.bfloat16), ref["acc"], "control")
    assert where in str(e.value), str(e.value)
    assert cluster is None or cluster in str(e.value), str(e.value)


def _parts(terms, scale):
    """Part rows as a kernel with 16-pixel tiles would leave them: one row per image; `scale` multiplies one cell of 16 pixels
    x 4 channels of image 1 (0: left out, 2: added twice)."""
    rows = []
    for b in range(B):
        ts = [t[b].reshape(H * H, O).clone() for t in terms]
        if b == 1:
            for t in ts:
                t[32:48, 8:12] *= scale
        rows.append(torch.stack([t.sum(0) for t in ts], 0))
    return torch.stack(rows, 0).float()


@pytest.mark.parametrize("scale", [0.0, 2.0], ids=["cell_left_out", "cell_added_twice"])
def test_sum_comparator_catches(ref, scale):
    want = X.column_sums(ref["terms"])
    X.assert_sums_equal(_parts(ref["terms"], 1.0), want, "control")  # without the defect: equal
    cell = ref["terms"][0][1].reshape(H * H, O)[32:48, 8:12]
    assert float(cell.sum(0).abs().min()) > 0, "the cell adds nothing to some channel: test data"
    with pytest.raises(AssertionError) as e:
        X.assert_sums_equal(_parts(ref["terms"], scale), want, "control")
    assert "channels [8, 9, 10, 11]" in str(e.value), str(e.value)


def test_weight_gradient_comparator_catches_a_transposed_tap(ref):
    X.assert_equal_tensor(ref["dw"].float(), ref["dw"], "control", ("cout", "tap", "cin"))  # without the defect: equal
    bad = ref["dw"].clone()
    bad[:, 1], bad[:, 3] = ref["dw"][:, 3], ref["dw"][:, 1]  # (kh, kw) = (0, 1) <-> (1, 0)
    assert not torch.equal(bad, ref["dw"]), "the planted defect changed nothing: test data"
    with pytest.raises(AssertionError) as e:
        X.assert_equal_tensor(bad.float(), ref["dw"], "control", ("cout", "tap", "cin"))
    assert "tap [1, 3]" in str(e.value), str(e.value)


@pytest.mark.parametrize("Kp", [32, 64])
@pytest.mark.parametrize("M", [4099, 64 * 2048 + 64 * 3 + 9])
def test_stem_operands_are_in_the_exact_range(Kp, M):
    """The operands of test_gpu_exact_conv.test_stem_gemms: the stem's part rows are not tied to images, so every sum is taken
    over ALL rows -- at the largest M of the stem tests too."""
    p = 0.125 * (64.0 / Kp) ** 0.5
    x, w = X.ternary(181, "x%d" % M, (M, Kp), 1.5 * p).double(), X.ternary(181, "w", (64, Kp), p).double()
    y = x @ w.t()
    scale, shift = X.prologue_coeffs(181, "bn", 64, "bn")
    slope = X.pick(181, "slope", 64, [0.5, 1.0]).double()
    u = y * scale.double() + shift.double()
    yv, z = y.view(1, 1, M, 64), torch.where(u > 0, u, u * slope).view(1, 1, M, 64)
    X.assert_exact_range(stored=[yv], terms=[yv, yv * yv], what="stem gemm")
    X.assert_exact_range(stored=[z], terms=[z, z * z], quantum=0.5, what="stem two-pass")
    g = X.ternary(181, "g%d" % M, (M, 64), 0.5).double()
    mean, invstd = X.pick(181, "mean", 64, [-1.0, 0.0, 1.0]).double(), X.pick(181, "invstd", 64, [0.5, 1.0, 2.0]).double()
    gp = torch.where(u > 0, g, g * slope)
    terms = [t.view(1, 1, M, 64) for t in (gp, gp * ((y - mean) * invstd), torch.where(u > 0, torch.zeros_like(u), g * u))]
    X.assert_exact_range(terms=terms, term_quantum=0.25, what="stem backward sums")
    X.assert_exact_range(wgrad_abs=X.wgrad_abs_bound(g.view(1, 1, M, 64), x), what="stem wgrad")
    assert float((y != 0).double().mean()) > 0.5


# ------------------------------------------------------------------------------------------------------------ channel-wise passes
# The recipes of test_gpu_exact_elementwise.py: each asserts its own preconditions (assert_exact_range) when it is built, so
# building it at every shape of the GPU tests IS the range check; then every reference against a second formulation.

EW = X.EW_SHAPES
EW_IDS = ["%d_%d_%d_%d" % s[:4] for s in EW]
MODES = ["plain", "slope", "gate", "gate_gse"]


@pytest.mark.parametrize("B,H,W,C,nb", EW, ids=EW_IDS)
def test_batchnorm_operands_are_in_the_exact_range(B, H, W, C, nb):
    """fr_bn_apply (every residual kind, gate, slope, gate + slope, the strided identity shortcut), fr_bn_bwd_reduce (four
    forms of g') and fr_bn_bwd_apply (add kinds 0 / 1, the rows of the BatchNorm in front) at every shape of the GPU tests."""
    for res_kind in (0, 1, 2):
        for gate in (False, True):
            for slope in (False, True):
                X.bn_apply_case(B, H, W, C, res_kind, gate, slope)
    for gate in (False, True):
        for slope in (False, True):
            X.bn_apply_case(B, H, W, C, 1, gate, slope, res_stride=2)
    for mode in MODES:
        X.bn_bwd_case(B, H, W, C, mode)
        for add_kind in (0, 1):
            X.bn_bwd_apply_case(B, H, W, C, mode, add_kind, nxt=mode == "plain")
    X.stats_case(B, H, W, C)


def test_scatter_and_long_statistics_operands_are_in_the_exact_range():
    for shape in X.SCATTER_SHAPES:
        for mode in ("plain", "slope", "gate_gse"):
            X.bn_bwd_apply_case(*shape, mode=mode, add_kind=2, nxt=mode == "plain")
    X.bn_bwd_apply_case(*X.SCATTER_S3, add_kind=2, add_stride=3)
    X.stats_case(*X.STATS_LONG[:4])


def test_squeeze_excite_operands_are_in_the_exact_range():
    assert {s[1] ** 2 for s in X.SE_SQUEEZE} == set(X.SE_HW)
    for shape in X.SE_SQUEEZE:
        _, _, pooled = X.se_squeeze_case(*shape)
        assert (pooled is not None) == (shape[1] in (4, 8))
    for shape in X.SE_CHAIN:
        X.se_bwd_case(*shape)
        X.se_bwd_case(*shape, zero_w1=True)
    for shape in X.SE_REAL_HW:
        X.se_bwd_case(*shape, zero_w1=True)
    with pytest.raises(AssertionError):  # 1 / 49 is not a power of two: the full chain is refused there
        X.se_bwd_case(5, 7, 128)


def _nchw(t):
    return t.double().permute(0, 3, 1, 2)


def test_bn_apply_reference_equals_torch_modules():
    """out = prelu(batch_norm(x) * gate) + batch_norm(res[:, ::s, ::s]) with F.batch_norm in eval mode (running mean 0, variance
    + eps = 1: weight and bias ARE scale and shift), F.prelu and F.max_pool2d(1, s) -- equal, the data being exact."""
    B, H, W, C = 3, 5, 7, 64
    eps = 2.0 ** -10
    zero, one = torch.zeros(C, dtype=torch.float64), torch.full((C,), 1.0 - eps, dtype=torch.float64)
    for res_kind, gate, slope, stride in ((0, False, False, 1), (1, True, False, 1), (2, True, True, 1), (1, False, True, 2),
                                          (2, False, False, 1)):
        o, out, terms = X.bn_apply_case(B, H, W, C, res_kind, gate, slope, stride)
        v = F.batch_norm(_nchw(o["x"]), zero, one, o["scale"].double(), o["shift"].double(), False, 0.0, eps)
        if gate:
            v = v * o["se"].double().view(B, C, 1, 1)
        if slope:
            v = F.prelu(v, o["slope"].double())
        if res_kind:
            r = F.max_pool2d(_nchw(o["res"]), 1, stride)
            if res_kind == 2:
                r = F.batch_norm(r, zero, one, o["rscale"].double(), o["rshift"].double(), False, 0.0, eps)
            v = v + r
        assert torch.equal(v.permute(0, 2, 3, 1), out)
        assert torch.equal(X.column_sums(terms)[1], (v * v).sum((0, 2, 3)))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("add_kind", [0, 1, 2])
def test_bn_backward_references_equal_autograd(mode, add_kind):
    """Training-mode F.batch_norm in float64 on Gaussian data (where its statistics mean something): with the batch's own mean
    and invstd, s0 = sum g', s1 = sum g' * xhat and inv_count = 1 / rows the formulas of include/frhip.h ARE its backward --
    d beta, d gamma, d slope and gx (+ the gradient of the MaxPool2d(1, 2) shortcut) against autograd."""
    from frhip import synth
    B, H, W, C, eps = 3, 6, 10, 8, 1e-5
    rows = B * H * W
    rnd = lambda tag, shape: synth.normal(241, tag, shape).double()  # noqa: E731
    x, g = rnd("x", (B, H, W, C)).requires_grad_(True), rnd("g", (B, H, W, C))
    gamma, beta = (rnd("gamma", (C,)) + 2.0).requires_grad_(True), rnd("beta", (C,)).requires_grad_(True)
    slope = (0.25 + 0.1 * rnd("slope", (C,)).abs()).requires_grad_(True)
    se, gse = rnd("se", (B, C)).abs() + 0.5, rnd("gse", (B, C))
    u = F.batch_norm(x.permute(0, 3, 1, 2), None, None, gamma, beta, True, 0.1, eps)
    kw = {}
    if mode == "slope":
        loss = (F.prelu(u, slope) * _nchw(g)).sum()
    elif mode.startswith("gate"):
        loss = (u * se.view(B, C, 1, 1) * _nchw(g)).sum()  # the excite multiplies BN's output by the gate ...
        kw["se"] = se
        if mode == "gate_gse":
            loss = loss + (u.sum((2, 3)) * gse).sum()       # ... and the squeeze hands back gse for every pixel of the image
            kw["gse"] = gse
    else:
        loss = (u * _nchw(g)).sum()
    add = None
    if add_kind == 1:
        add = rnd("add", (B, H, W, C))
        loss = loss + (x * add).sum()
    elif add_kind == 2:
        a = rnd("add", (B, H // 2, W // 2, C))
        loss = loss + (F.max_pool2d(x.permute(0, 3, 1, 2), 1, 2) * _nchw(a)).sum()
        add = X.scatter(a, H, W, 2)
    want_gx, want_dg, want_db, want_ds = torch.autograd.grad(loss, [x, gamma, beta, slope], allow_unused=True)
    xd = x.detach()
    mean = xd.mean((0, 1, 2))
    invstd = 1.0 / torch.sqrt(xd.var((0, 1, 2), unbiased=False) + eps)
    scale = gamma.detach() * invstd
    shift = beta.detach() - mean * scale
    if mode == "slope":
        kw.update(scale=scale, shift=shift, slope=slope.detach())
    gp, st = X.bn_bwd_gprime(g, xd, **kw)
    xh = X.xhat(xd, mean, invstd)
    s = X.column_sums([gp, gp * xh, st])
    gx = X.bn_bwd_apply(gp, xh, gamma.detach(), invstd, s[0], s[1], 1.0 / rows, add)
    close = lambda a, b: torch.allclose(a, b, rtol=1e-9, atol=1e-9)  # noqa: E731  (float64 against float64)
    assert close(s[0], want_db) and close(s[1], want_dg) and close(gx, want_gx)
    if mode == "slope":
        assert close(s[2], want_ds)


def test_squeeze_excite_references_equal_autograd():
    """Stage by stage, autograd in float64: gs through the excite product, gz through a sigmoid AT the gate s (z = logit s), gh
    through the ReLU mask of `hidden`, gpooled through the mean over the image, dW1 / dW2 through the two matrices; the rows of
    BN2's sums in their closed form s*G + HW*gse, s*GX + gse*XH; fr_se_pool as F.adaptive_avg_pool2d."""
    B, H, C = 5, 4, 128
    HW = H * H
    o, r = X.se_bwd_case(B, H, C)
    d = {k: v.double() for k, v in o.items()}
    close = lambda a, b: torch.allclose(a, b, rtol=1e-12, atol=1e-12)  # noqa: E731
    gate = torch.ones(B, C, dtype=torch.float64, requires_grad=True)
    y = d["x"] * d["scale"] + d["shift"]
    (gs,) = torch.autograd.grad((d["g"] * y * gate.view(B, 1, 1, C)).sum(), gate)
    assert torch.equal(gs, r["gs"])
    z = torch.logit(d["s"]).requires_grad_(True)
    (gz,) = torch.autograd.grad((torch.sigmoid(z) * r["gs"]).sum(), z)
    assert close(gz, r["gz"])
    w1, w2 = d["w1"].clone().requires_grad_(True), d["w2"].clone().requires_grad_(True)
    ymap = torch.zeros(B, H, H, C, dtype=torch.float64, requires_grad=True)  # the map the squeeze averages
    pooled = d["pooled"] + ymap.mean((1, 2))
    pre = (pooled @ w1.t())
    pre = pre + (torch.where(d["hidden"] > 0, d["hidden"], -torch.ones_like(d["hidden"])) - pre).detach()  # relu(pre) == hidden
    pre.retain_grad()
    hid = torch.relu(pre)
    assert torch.equal(hid.detach(), d["hidden"])
    loss = ((hid @ w2.t()) * r["gz"]).sum()
    gmap, gw1, gw2 = torch.autograd.grad(loss, [ymap, w1, w2], retain_graph=True)
    (gpre,) = torch.autograd.grad(loss, pre)
    assert close(gpre, r["gh"])
    assert close(gmap, r["gpooled"].view(B, 1, 1, C).expand(B, H, H, C))
    assert close(gw2, r["dw2"])
    # the weight gradient of fc1 multiplies gh by the pooled INPUT of the recipe (ymap is zero): gh^T pooled
    assert close(gw1, r["dw1"])
    sd, gse = d["s"], r["gpooled"]
    assert torch.equal(r["parts"][:, 0], r["gs"])
    assert torch.equal(r["bn"][:, 0], sd * r["parts"][:, 1] + HW * gse)
    assert torch.equal(r["bn"][:, 1], sd * r["parts"][:, 2] + gse * r["parts"][:, 3])
    q, gs2, pooled2 = X.se_squeeze_case(3, 4, 64)
    u = F.adaptive_avg_pool2d(_nchw(q["x"]), 1).view(3, 64) * q["scale"].double() + q["shift"].double()
    assert torch.equal(u, pooled2)
    assert torch.equal(torch.einsum("bhwc,bhwc->bc", q["g"].double(), q["x"].double() * q["scale"].double() + q["shift"].double()), gs2)
    x, terms = X.stats_case(3, 5, 7, 64)
    flat = x.double().reshape(-1, 64)
    assert torch.equal(X.column_sums(terms), torch.stack([flat.sum(0), (flat * flat).sum(0)]))
    assert torch.equal(X.image_sums(terms)[:, 1], torch.einsum("bhwc,bhwc->bc", x.double(), x.double()))


def test_elementwise_comparators_catch_planted_differences():
    """One wrong row, one wrong image's gate, one even-row / odd-column hit of the strided scatter -- and a part row left unwritten
    or taken from one row too many."""
    B, H, W, C = 5, 7, 7, 128
    o, out, terms = X.bn_apply_case(B, H, W, C, 1, True, False)
    X.assert_equal_nhwc(out.to(torch.bfloat16), out, "control")
    bad = out.clone()
    bad[3, 6, 2] = 0.0  # one row of the [rows][C] tensor: row 3*49 + 6*7 + 2 never written
    assert not torch.equal(bad, out)
    with pytest.raises(AssertionError) as e:
        X.assert_equal_nhwc(bad.to(torch.bfloat16), out, "control")
    assert "image 3, row 6, column 2" in str(e.value) and "images [3]" in str(e.value), str(e.value)
    se = o["se"].clone()
    se[2] = o["se"][1]  # image 2 reads image 1's gate
    assert not torch.equal(se[2], o["se"][2])
    bad, _ = X.bn_apply(**dict(o, se=se))
    with pytest.raises(AssertionError) as e:
        X.assert_equal_nhwc(bad.to(torch.bfloat16), out, "control")
    assert "images [2]" in str(e.value) and "image 2, row 0, column 0" in str(e.value), str(e.value)
    o, gx, terms = X.bn_bwd_apply_case(3, 6, 10, 64, add_kind=2, nxt=True)
    X.assert_equal_nhwc(gx.to(torch.bfloat16), gx, "control")
    bad = gx.clone()
    bad[:, ::2, 1::2] += o["add"].double()  # hits whenever h is even: the odd columns take their left neighbour's value
    with pytest.raises(AssertionError) as e:
        X.assert_equal_nhwc(bad.to(torch.bfloat16), gx, "control")
    assert "first at (image 0, row 0, column 1, channel 0)" in str(e.value), str(e.value)
    assert "%d of" % (3 * 3 * 5 * 64) in str(e.value), str(e.value)  # every planted hit counts: add is non-zero everywhere
    want = X.column_sums(terms)
    flat = [t.reshape(-1, 64) for t in terms]
    rows = lambda lo, hi: torch.stack([t[lo:hi].sum(0) for t in flat], 0).float()  # noqa: E731
    X.assert_sums_equal(torch.stack([rows(0, 100), rows(100, 180)]), want, "control")
    for parts in (torch.stack([rows(0, 100), torch.full((2, 64), 24576.0)]),   # an idle workgroup left its sentinels
                  torch.stack([rows(0, 100), rows(99, 180)])):                 # one row counted twice
        with pytest.raises(AssertionError):
            X.assert_sums_equal(parts, want, "control")


# ------------------------------------------------------------------------------------------------------------ output-layer GEMMs
# The recipes of test_gpu_exact_output.py.  linear_case / linear_dgrad / flatten_case assert their own preconditions, so building
# them at every listed geometry is the range check.  The real-K operands are built once for all tests of this file.
import functools  # noqa: E402

from test_gpu_dropout import host_keep_mask  # noqa: E402

linear_case = functools.lru_cache(maxsize=None)(X.linear_case)


def _fwd_shapes():
    return sorted({s[:3] for s in X.LINEAR_FWD})


def test_frac_weights_sit_on_the_ties_of_the_bf16_rounding():
    """torch's cast is the specification: the list holds ties to either side and their neighbours, every value is an fp32 number,
    and truncation would get three of the six wrong."""
    w = torch.tensor(X.FRAC_POS, dtype=torch.float64)
    assert torch.equal(w.float().double(), w)
    assert X.round_bf16(w.float()).tolist() == X.FRAC_ROUNDED
    assert X.round_bf16(-w.float()).tolist() == [-v for v in X.FRAC_ROUNDED]
    trunc = (w.float().view(torch.int32) & -65536).view(torch.float32).double()
    assert int((trunc != X.round_bf16(w.float())).sum()) == 3
    assert 1.0 + 2.0 ** -8 in X.FRAC_WEIGHTS and 1.0 + 3 * 2.0 ** -8 in X.FRAC_WEIGHTS
    assert 1.0 + 2.0 ** -8 + 2.0 ** -16 in X.FRAC_WEIGHTS and -(1.0 - 2.0 ** -9 - 2.0 ** -17) in X.FRAC_WEIGHTS


def test_linear_operands_are_in_the_exact_range():
    """Every geometry of the four lists: the forward sums (with frac too: quanta of 2^-8), the data gradient as bf16 integers,
    the weight gradient; the cut of FR_EPI_SLAB covers all K steps once."""
    for B, O, K in _fwd_shapes():
        for frac in (False, True):
            c = linear_case(B, O, K, frac=frac)
            assert float((c["W"] == 0).double().mean()) == pytest.approx(0.5, abs=0.05) or K < 64
            if frac:
                assert set(c["W"].unique().tolist()) <= set(torch.tensor(X.FRAC_WEIGHTS + [0.0]).tolist())
                assert not torch.equal(c["Wq"], c["W"].double()), "the cast changes nothing: test data"
    for B, O, K in X.LINEAR_DGRAD:
        ga = X.linear_dgrad(linear_case(B, O, K))
        assert float(ga.abs().max()) >= 8 and float(ga.abs().max()) <= 256
    for B, O, K, _ in X.LINEAR_WGRAD:
        assert float(X.linear_wgrad(linear_case(B, O, K)).abs().max()) <= B
    for M, N, SC, splitk, _ in X.SLAB_GEMM:
        linear_case(M, N, SC)
        linear_case(M, N, SC, frac=True)
        cuts = X.splitk_cut(SC // 32, splitk)
        assert cuts[0][0] == 0 and cuts[-1][1] == SC and all(a[1] == b[0] for a, b in zip(cuts, cuts[1:]))
    assert [(e - b) // 32 for b, e in X.splitk_cut(7, 3)] == [2, 2, 3]
    assert X.splitk_cut(3, 1) == [(0, 96)]
    assert sum(s[:3] == X.LINEAR_REAL for s in X.LINEAR_FWD) == 2 and X.LINEAR_DGRAD.count(X.LINEAR_REAL) == 1
    assert sum(s[:3] == X.LINEAR_REAL for s in X.LINEAR_WGRAD) == 1 and sum(s[:3] == X.LINEAR_REAL for s in X.SLAB_GEMM) == 1


def test_linear_geometries_reach_the_edges_they_name():
    """Step counts per slice of the forward list against the source's loop (two steps per trip, an odd tail), row counts against
    the 256-row block and the 64-row wave; the data gradient against 128-row blocks and 32-row waves; the weight gradient's batches
    against its 32-row steps and its four tiles."""
    ksteps = [K // 32 // s for _, _, K, s in X.LINEAR_FWD if s]
    assert {1, 3, 5, 8, 49} <= set(ksteps) and any(k >= 3 and k & 1 for k in ksteps)
    assert {1, 65, 256, 257} <= {s[0] for s in X.LINEAR_FWD} and {64, 128, 512} <= {s[1] for s in X.LINEAR_FWD}
    assert all(O % 64 == 0 and K % 32 == 0 and (s is None or (K // 32) % s == 0) for _, O, K, s in X.LINEAR_FWD)
    assert {1, 33, 129, 128} <= {s[0] for s in X.LINEAR_DGRAD} and all(O % 128 == 0 and K % 128 == 0 for _, O, K in X.LINEAR_DGRAD)
    assert {1, 31, 33, 256} <= {s[0] for s in X.LINEAR_WGRAD}
    tiles = {(128 if co >= 128 else 64, (128 if sc >= 128 else 64) if co >= 128 else (64 if sc >= 64 else 32))
             for _, co, sc, _ in X.LINEAR_WGRAD}
    assert tiles == {(128, 128), (128, 64), (64, 64), (64, 32)}
    assert any(co % 64 for _, co, _, _ in X.LINEAR_WGRAD)
    assert {d for s in X.LINEAR_WGRAD for d in s[3:]} == {"bf16", "f32"} == {s[4] for s in X.SLAB_GEMM}
    assert {64, 200, 512} <= {s[1] for s in X.SLAB_GEMM} and any(s[0] % 128 for s in X.SLAB_GEMM)
    assert any(s[3] == 1 for s in X.SLAB_GEMM) and any((s[2] // 32) % s[3] for s in X.SLAB_GEMM)
    assert X.LINEAR_REAL + (49, "f32") in X.SLAB_GEMM


@pytest.mark.parametrize("B,O,K,slices", X.LINEAR_FWD_ONE_HOT)
def test_one_hot_rows_of_the_forward_reach_every_position(B, O, K, slices):
    """Between them the rows hit all 32 positions of a K step, both register slots of the forward kernel, and the first and the
    last step of the first and of the last slice; the reference holds the rounded weight in the owning slice and the bias or zero
    elsewhere."""
    picks = [X.stride_pick(K)(b) for b in range(B)]
    a = X.one_hot_rows(B, K, X.stride_pick(K))
    assert torch.equal(a.sum(1), torch.ones(B)) and all(a[b, k] == 1 for b, k in enumerate(picks))
    ksteps = K // 32 // slices
    assert {k % 32 for k in picks} == set(range(32))
    local = {(k // 32 // ksteps, k // 32 % ksteps) for k in picks}   # (slice, step within the slice)
    assert {(0, 0), (0, ksteps - 1), (slices - 1, 0), (slices - 1, ksteps - 1)} <= local
    assert {st & 1 for _, st in local} == ({0, 1} if ksteps > 1 else {0})
    W, bias = X.normal_weight(O, K), X.small_ints(271, "oh.bias", (O,))
    ref = X.one_hot_forward(W, bias, picks, slices)
    plain = (a.double() @ X.round_bf16(W).t())
    assert torch.equal(ref.sum(0).float(), (plain + bias.double()).float())   # added in float64, rounded once: fr_reduce_parts
    for s in range(slices):
        own = torch.tensor([k // (K // slices) == s for k in picks])
        assert torch.equal(ref[s][~own], (bias.double() if s == 0 else torch.zeros(O, dtype=torch.float64)).expand(int((~own).sum()), O))
    assert torch.equal(X.one_hot_forward(W, None, picks, slices).sum(0), plain)


@pytest.mark.parametrize("B,O,K", X.LINEAR_DGRAD_ONE_HOT)
def test_one_hot_rows_of_the_data_gradient_reach_every_position(B, O, K):
    """The reduction of the data gradient runs over O: all 32 positions of a step, all four ring slots, the first and last step."""
    picks = [X.stride_pick(O)(b) for b in range(B)]
    assert {o % 32 for o in picks} == set(range(32))
    steps = {o // 32 for o in picks}
    assert {0, O // 32 - 1} <= steps and {s % 4 for s in steps} == {0, 1, 2, 3}


def test_normal_weight_is_finite_and_normal():
    W = X.normal_weight(128, 256)
    assert bool(torch.isfinite(W).all()) and float(W.abs().min()) > 2.0 ** -100
    assert 0.01 < float(W.std()) < 0.6
    Wq = X.round_bf16(W)
    assert not torch.equal(Wq, W.double()) and float((Wq - W.double()).abs().max()) <= 2.0 ** -8
    assert set(X.FRAC_WEIGHTS) <= set(W.double().unique().tolist())


@pytest.mark.parametrize("frac", [False, True])
def test_linear_references_equal_torch_modules(frac):
    """nn.Linear in float64 on the bf16-rounded weight: forward (the slabs added up), and autograd's input and weight gradients."""
    B, O, K = 65, 64, 192
    c = linear_case(B, O, K, frac=frac)
    lin = torch.nn.Linear(K, O, dtype=torch.float64)
    with torch.no_grad():
        lin.weight.copy_(c["W"].to(torch.bfloat16))
        lin.bias.copy_(c["bias"])
    a = c["a"].double().requires_grad_(True)
    out = lin(a)
    for slices in (1, 2, 3):
        assert torch.equal(X.linear_forward(c, slices).sum(0), out.detach())
        assert torch.equal(X.linear_forward(c, slices, bias=False).sum(0) + c["bias"].double(), out.detach())
        assert torch.equal(X.linear_forward(c, slices)[1:], X.linear_forward(c, slices, bias=False)[1:])   # the bias: slab 0 only
    assert torch.equal(X.linear_forward(c, cuts=X.splitk_cut(K // 32, 4)).sum(0), out.detach())
    ga, gw = torch.autograd.grad(out, [a, lin.weight], c["g"].double())
    assert torch.equal(X.linear_wgrad(c), gw)
    if not frac:
        assert torch.equal(X.linear_dgrad(c), ga)


def test_flatten_reference_equals_the_reference_module():
    """flatten_case against nn.Sequential(Flatten, Linear) on the NCHW tensor with the dropout mask applied by hand, for both p;
    a[b][c*HW + hw] is the BatchNorm output of pixel hw, channel c."""
    B, C, HW, O = X.FLATTEN_CASE
    for p in (0.5, 0.0):
        keep = torch.from_numpy(host_keep_mask(0x5EED, B, C, HW, p))
        assert float(keep.double().mean()) == pytest.approx(1.0 - p, abs=0.02)
        o, a, f, gy, dW = X.flatten_case(B, C, HW, O, keep, p)
        y = o["x"].double() * o["scale"].double() + o["shift"].double()             # [B, HW, C]
        assert float(a[1, 5 * HW + 7]) == float(y[1, 7, 5]) * float(keep[1, 5 * HW + 7]) / (1.0 - p)
        nchw = (y.permute(0, 2, 1).reshape(B, C, 7, 7) * keep.view(B, C, 7, 7) / (1.0 - p)).requires_grad_(True)
        mod = torch.nn.Sequential(torch.nn.Flatten(), torch.nn.Linear(C * HW, O, bias=False, dtype=torch.float64))
        with torch.no_grad():
            mod[1].weight.copy_(o["Wq"])
        out = mod(nchw)
        assert torch.equal(out.detach(), f)
        g_in, g_w = torch.autograd.grad(out, [nchw, mod[1].weight], o["g"].double())
        assert torch.equal(g_w, dW)
        assert torch.equal((g_in * keep.view(B, C, 7, 7) / (1.0 - p)).reshape(B, C, HW).permute(0, 2, 1), gy)


def test_linear_range_checks_refuse_what_is_not_exact():
    """A frac weight fed to the data-gradient recipe (ga would not be an integer), and a density at which the forward sums leave
    2^23 quanta: the same shape passes at the default density."""
    with pytest.raises(AssertionError):
        X.linear_dgrad(linear_case(65, 64, 192, frac=True))
    X.linear_case(1, 64, 50176, frac=True)
    with pytest.raises(AssertionError) as e:
        X.linear_case(1, 64, 50176, frac=True, density=1.0, wdensity=1.0)
    assert "quanta" in str(e.value), str(e.value)


def test_linear_comparators_catch_planted_differences():
    """One element of one slab, a bias added to slice 1 as well, a dropped K step, a truncated weight."""
    c = linear_case(65, 64, 192, frac=True)
    ref = X.linear_forward(c, 2)
    X.assert_equal_tensor(ref.float(), ref, "control", ("slice", "row", "feature"))
    bad = ref.clone()
    bad[1, 64, 3] += 2.0 ** -8
    with pytest.raises(AssertionError) as e:
        X.assert_equal_tensor(bad.float(), ref, "control", ("slice", "row", "feature"))
    assert "1 of" in str(e.value) and "first at (1, 64, 3)" in str(e.value), str(e.value)
    bad = ref.clone()
    bad[1] += c["bias"].double()
    assert not torch.equal(bad, ref)
    with pytest.raises(AssertionError) as e:
        X.assert_equal_tensor(bad.float(), ref, "control", ("slice", "row", "feature"))
    assert "slice [1]" in str(e.value), str(e.value)
    nz = int((c["bias"] != 0).sum())
    assert "%d of" % (65 * nz) in str(e.value), str(e.value)   # every row of every feature with a bias
    with pytest.raises(AssertionError):   # the sum of the slabs sees it too
        X.assert_equal_tensor(bad.sum(0).float(), ref.sum(0), "control")
    dropped = ref.clone()
    dropped[1] -= c["a"].double()[:, 160:192] @ c["Wq"][:, 160:192].t()   # the odd tail of ksteps = 3
    with pytest.raises(AssertionError):
        X.assert_equal_tensor(dropped.float(), ref, "control")
    trunc = (c["W"].view(torch.int32) & -65536).view(torch.float32).double()
    with pytest.raises(AssertionError):
        X.assert_equal_tensor((c["a"].double() @ trunc.t() + c["bias"].double()).float(), ref.sum(0), "control")


# ------------------------------------------------------------------------------------------------------------ margin head
# The recipe of test_gpu_exact_head.py (exact_operands.head_case) meets its conditions at every shape, its references are the
# oracle's ArcFace / CosFace and autograd's gradients, and the comparators catch five planted defects.
head_case = functools.lru_cache(maxsize=None)(X.head_case)
HEAD_IDS = ["%d_%d_%d" % s for s in X.HEAD_COL_SHAPES]


@pytest.mark.parametrize("B,N,D", X.HEAD_COL_SHAPES, ids=HEAD_IDS)
def test_head_operands_meet_their_conditions(B, N, D):
    """head_case asserts the exactness conditions itself (fp32 round trip of the whole CosFace chain, every GEMM below 2^24
    quanta, powers of two as reciprocal norms, the clearance to th).  Here: what the recipe must REACH.  Labels: the columns of
    head_label_columns where the batch has rows for them, two rows with -1 from B = 4 on.  Target cosines: -1, +1, 0, both
    neighbours of th and of 0 where the batch has the seven rows for them, every numerator at (129, 65, 32).  Density: 80 % of the
    off-label cosines are non-zero (a column permutation shows), 80 % of gx where N >= 32 and of gw where B >= 32 (with fewer rows
    than that, half the columns of a half-zero g have no term at all: (1, 4, 32) has 18 % and is there for its geometry); the
    upstream gradient is about half zeros and never zero on a label column."""
    c = head_case(B, N, D)
    lab, nnz = c["labels"], c["nnz"]
    has = lab >= 0
    cols = X.head_label_columns(N)
    assert {N - 1, 4 * ((N - 1) // 4), 0} <= set(cols) and (N <= 64 or {63, 64, 64 * (N // 64) - 1, 64 * (N // 64 - 1)} <= set(cols))
    assert N <= 4 or {3, 4} <= set(cols)
    assert int((~has).sum()) == (2 if B >= 4 else 0)
    reach = min(len(cols), int(has.sum()))
    assert set(cols[:reach]) <= set(lab[has].tolist()) and int(lab[B - 1]) == N - 1
    if B >= 32:
        assert set(cols) <= set(lab.tolist())
    tc = X.head_target_cosines(c)[has]
    num = set((tc * nnz).round().int().tolist())
    assert torch.equal(tc * nnz, (tc * nnz).round())
    if int(has.sum()) >= 3:
        assert {nnz, -nnz, 0} <= num
    if int(has.sum()) >= 7:
        assert bool(((tc > X.HEAD_TH) & (tc < -0.8)).any()) and bool((tc < X.HEAD_TH).any() and (tc[tc < X.HEAD_TH] > -1).any())
        assert bool((tc > 0).any()) and bool((tc < 0).any())
        step = 1 if D > nnz else 2   # the smallest non-zero numerator: odd ones need a place off the support
        assert {step, -step} <= num
    if (B, N, D) == (129, 65, 32):
        assert num == set(range(-16, 17))
        assert {-14, -15} <= num and -14 / 16 > X.HEAD_TH > -15 / 16
    off = torch.ones(B, N, dtype=torch.bool)
    off[has.nonzero().flatten(), lab[has]] = False
    if off.any():
        assert float((c["cos"][off] != 0).double().mean()) >= 0.8
    if N >= 32:
        assert float((c["gx"] != 0).double().mean()) >= 0.8
    if B >= 32:
        assert float((c["gw"] != 0).double().mean()) >= 0.8
    assert float((c["gw"] != 0).double().mean()) > 0.15 and float((c["gx"] != 0).double().mean()) > 0.5
    g = c["g"]
    assert bool((g[has.nonzero().flatten(), lab[has]] != 0).all())
    assert N < 32 or 0.4 < float((g == 0).double().mean()) < 0.6
    assert set(g.unique().tolist()) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
    # the geometry each shape is there for (frhip/functional.py: Np = pad32, ld = pad4, splitk = max(1, min(nk, 64, nk // 8)))
    nk = c["Np"] // 32
    want = {(1, 4, 32): (32, 4, 1), (37, 203, 64): (224, 204, 1), (129, 65, 32): (96, 68, 1), (5, 500, 32): (512, 500, 2),
            (130, 1000, 512): (1024, 1000, 4), (37, 203, 96): (224, 204, 1)}[(B, N, D)]
    assert (c["Np"], c["ld"], max(1, min(nk, 64, nk // 8))) == want


@pytest.mark.parametrize("B,N,D", [(37, 203, 64), (129, 65, 32)], ids=["37_203_64", "129_65_32"])
def test_head_references_equal_the_oracle_and_autograd(B, N, D):
    """The float64 references against code that was not written for them, on the labelled rows: the oracle's CosFace / ArcFace
    (oracle/irse_ref.py, float64) for the logits -- the two-operation fp32 values within an fp32 rounding of the float64 ones,
    the phi branch within the fp32 rounding of the constants -- and torch autograd for d phi / d cos (dphi_ref) and for the shared
    cosine backward (cosine_backward)."""
    from oracle import irse_ref as O
    c = head_case(B, N, D)
    rows = (c["labels"] >= 0).nonzero().flatten()
    lab = c["labels"][rows]
    x = c["x"][rows].double().requires_grad_(True)
    w = c["w"].double().requires_grad_(True)
    assert float((O.cosine_logits(x, w).detach() - c["cos"][rows]).abs().max()) < 1e-15
    for name, (kind, s, m, easy) in X.HEAD_CONFIGS.items():
        k = X.margin_constants(name)
        ref, bound, moved = X.margin_logits_ref(c, k)
        y = O.cosface_forward(x, w, lab, s, m) if kind == 1 else O.arcface_forward(x, w, lab, s, m, bool(easy))
        assert float((y.detach() - ref[rows]).abs().max()) < 64 * 2.0 ** -22, name
        assert float(bound.max()) < 64 * 2.0 ** -20 and bool((bound[~moved] == 0).all())
        # d logits / d cos on the label column = s * dphi
        cos = c["cos"][rows].clone().requires_grad_(True)
        tl = cos[torch.arange(len(rows)), lab]
        if kind == 1:
            phi = tl - k["cos_m"]
        else:
            full = tl * k["cos_m"] - torch.sqrt((1.0 - tl * tl).clamp(X.EPS32, 1.0)) * k["sin_m"]
            phi = torch.where(tl > 0, full, tl) if easy else torch.where(tl > k["th"], full, tl - k["mm"])
        (d_auto,) = torch.autograd.grad(phi.sum(), [cos])
        d_auto = d_auto[torch.arange(len(rows)), lab]
        for i, r in enumerate(rows.tolist()):
            d, db = X.dphi_ref(float(c["cos"][r, lab[i]]), k)
            cc = float(c["cos"][r, lab[i]])
            if abs(cc) == 1.0 or cc == 0.0:   # at the clamp autograd's subgradient is torch's choice; the kernel's mask is strict
                assert d in (1.0, k["cos_m"]) and db == 0.0
            else:
                assert abs(float(d_auto[i]) - d) < 1e-12, (name, r, cc)
    # the shared backward from CosFace's gcos: autograd through F.normalize and F.linear
    gcos = c["gcos"][rows][:, :N]
    gx, gw = torch.autograd.grad(O.cosine_logits(x, w), [x, w], gcos)
    r = X.cosine_backward(c["xn"][rows], c["inv_x"][rows], c["wn"][:N], c["inv_w"], gcos)
    assert float((gx - r["gx"]).abs().max()) <= 1e-12 * float(r["gx"].abs().max())
    assert float((gw - r["gw"]).abs().max()) <= 1e-12 * float(r["gw"].abs().max())


def test_head_clearance_check_refuses_a_cosine_on_the_threshold(monkeypatch):
    monkeypatch.setattr(X, "HEAD_TH", -14.0 / 16 + 2.0 ** -12)
    with pytest.raises(AssertionError) as e:
        X.head_case(129, 65, 32)
    assert "from th" in str(e.value), str(e.value)


SENT = 24576.0


def _forward_ok(c, k):
    ref, bound, _ = X.margin_logits_ref(c, k)
    cos_t = X.head_target_cosines(c)
    cos_t[torch.isnan(cos_t)] = SENT
    return ref.float(), cos_t.float()


def _row_with(c, pred, neighbour=True):
    """The first labelled row that `pred` accepts (neighbour: and whose label column has one to its right)."""
    for b in range(c["B"]):
        lab = int(c["labels"][b])
        if lab >= 0 and (lab + 1 < c["N"] or not neighbour) and pred(b, lab):
            return b, lab
    raise AssertionError("the recipe has no such row: test data")


@pytest.mark.parametrize("name", sorted(X.HEAD_CONFIGS))
def test_margin_comparators_catch_planted_defects(name):
    """The comparators of test_gpu_exact_head.py on the float64 reference (rounded to fp32, as a kernel's output is) with one
    defect planted at a time: the margin on column label + 1, cos_t from the neighbouring column, one non-zero in a padding column
    of gcos, dphi with the clamp mask passing at c = 1, a label -1 row with the margin applied to column 0.  Each control first
    shows that the unplanted reference passes and that the defect changes it; the failure names the element."""
    c = head_case(37, 203, 64)
    k = X.margin_constants(name)
    ref, bound, moved = X.margin_logits_ref(c, k)
    logits, cos_t = _forward_ok(c, k)
    X.check_margin_forward(logits, cos_t, c, k, SENT, "control")
    plain = (k["s"] * c["cos"]).float()

    # the margin one column off
    b, lab = _row_with(c, lambda b, lab: bool(moved[b, lab]))
    bad = logits.clone()
    bad[b, lab + 1] = plain[b, lab + 1] + (logits[b, lab] - plain[b, lab])
    bad[b, lab] = plain[b, lab]
    assert not torch.equal(bad, logits)
    with pytest.raises(AssertionError) as e:
        X.check_margin_forward(bad, cos_t, c, k, SENT, "control")
    assert "2 of" in str(e.value) and "first at (%d, %d)" % (b, lab) in str(e.value), str(e.value)

    # cos_t from the neighbouring column
    b, lab = _row_with(c, lambda b, lab: float(c["cos"][b, lab + 1]) != float(c["cos"][b, lab]))
    bad_t = cos_t.clone()
    bad_t[b] = c["cos"][b, lab + 1]
    with pytest.raises(AssertionError) as e:
        X.check_margin_forward(logits, bad_t, c, k, SENT, "control")
    assert "cos_t" in str(e.value) and "first at (%d,)" % b in str(e.value), str(e.value)

    # a row without a label: cos_t written, and the margin applied to column 0
    b = int((c["labels"] < 0).nonzero()[0])
    bad_t = cos_t.clone()
    bad_t[b] = c["cos"][b, 0]
    with pytest.raises(AssertionError) as e:
        X.check_margin_forward(logits, bad_t, c, k, SENT, "control")
    assert "cos_t" in str(e.value) and "first at (%d,)" % b in str(e.value), str(e.value)
    bad = logits.clone()
    bad[b, 0] = (c["cos"][b, 0] - 0.35) * k["s"]
    assert bad[b, 0] != logits[b, 0]
    with pytest.raises(AssertionError) as e:
        X.check_margin_forward(bad, cos_t, c, k, SENT, "control")
    assert "1 of" in str(e.value) and "first at (%d, 0)" % b in str(e.value), str(e.value)

    # the backward pass
    g, labels, Np = c["g"], c["labels"], c["Np"]
    gref, gbound = X.margin_gcos_ref(g, labels, cos_t.double(), k, Np)
    gcos = gref.float()
    X.check_margin_backward(gcos, g, labels, cos_t.double(), k, "control")
    bad = gcos.clone()
    bad[36, Np - 1] = 2.0 ** -20                                      # one non-zero in a padding column
    with pytest.raises(AssertionError) as e:
        X.check_margin_backward(bad, g, labels, cos_t.double(), k, "control")
    assert "1 of" in str(e.value) and "first at (36, %d)" % (Np - 1) in str(e.value), str(e.value)
    bad = gcos.clone()
    bad[0, Np - 3] = -0.0                                             # ... and a -0 there
    with pytest.raises(AssertionError) as e:
        X.check_margin_backward(bad, g, labels, cos_t.double(), k, "control")
    assert "not +0" in str(e.value), str(e.value)
    if k["kind"] == 0:                                                # the clamp mask passing at c = 1
        b, lab = _row_with(c, lambda b, lab: float(c["cos"][b, lab]) == 1.0, neighbour=False)
        bad = gcos.clone()
        bad[b, lab] = k["s"] * g[b, lab] * (k["cos_m"] + k["sin_m"] * 1.0 / (X.EPS32 ** 0.5))
        assert bad[b, lab] != gcos[b, lab] and float(gbound[b, lab]) == 0.0
        with pytest.raises(AssertionError) as e:
            X.check_margin_backward(bad, g, labels, cos_t.double(), k, "control")
        assert "1 of" in str(e.value) and "first at (%d, %d)" % (b, lab) in str(e.value), str(e.value)
        # one ulp beside an exact value fails, the bounded branch takes a rounding and refuses 1e-4 of the value
        b2, lab2 = _row_with(c, lambda b, lab: float(gbound[b, lab]) > 0)
        near = gcos.clone()
        near[b2, lab2] = torch.nextafter(gcos[b2, lab2], torch.tensor(1e9))
        X.check_margin_backward(near, g, labels, cos_t.double(), k, "control")
        near[b2, lab2] = gcos[b2, lab2] * (1.0 + 1e-4)
        with pytest.raises(AssertionError):
            X.check_margin_backward(near, g, labels, cos_t.double(), k, "control")
    else:                                                             # CosFace: s * g on the label column too
        b, lab = _row_with(c, lambda b, lab: True)
        bad = gcos.clone()
        bad[b, lab] = torch.nextafter(gcos[b, lab], torch.tensor(1e9))
        with pytest.raises(AssertionError) as e:
            X.check_margin_backward(bad, g, labels, cos_t.double(), k, "control")
        assert "first at (%d, %d)" % (b, lab) in str(e.value), str(e.value)
