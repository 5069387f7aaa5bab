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
