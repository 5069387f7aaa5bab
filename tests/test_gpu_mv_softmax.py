"""MV_Softmax on the HIP path (reference head/metrics.py:555-590): the reference's own vectors (g22) with the per-row target
cosine, threshold and hard count, larger sizes against a float64 host restatement, the two C entry points alone on hand-made
cosines in sentinel-filled buffers (raw cosines beyond +-1 pass unclamped, value and gradient), the pipeline (no
device-to-host copy and no ATen GEMM in the forward pass, bit-reproducible, label errors, the empty batch, the attributes
read at call time), and train.py end to end including a bit-for-bit resume, in both forms.

The float64 restatement is the head's own host path (plain PyTorch, pinned to g22 by test_mv_softmax_host.py) run on a
float64 copy of the module.  The batches are the constructed ones of tests/mv_softmax_data.py: rows without a hard negative,
rows with planted ones, rows with 0 < gt < margin and rows in the ``gt <= 0`` branch, none of them near a decision boundary."""
import copy
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_support as HS
import mv_softmax_data as MD
from frhip import synth
from head_support import Guarded, float64_reference, maxrel, relerr, run

pytestmark = pytest.mark.gpu

CASES = ("rand_am", "rand_arc", "built_am", "built_arc", "built_am_m05", "built_arc_m05")
D = 512
FORMS = [pytest.param(True, id="am"), pytest.param(False, id="arc")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g22(golden_dir):
    return np.load(os.path.join(golden_dir, "g22_mv_softmax.npz"))


def make(N, k, is_am, margin=0.35, mv_weight=1.12, scale=32):
    from head.metrics import MV_Softmax
    head = MV_Softmax(D, N, is_am, margin=margin, mv_weight=mv_weight, scale=scale)
    with torch.no_grad():
        head.weight.copy_(k)
    return head


def device_rows(head, x, label):
    """(rowv [4, B] (gt, thr, final, d final / d gt), raw cosines [B, N]) of the device forward pass, on the host."""
    from frhip import functional as FRF
    mv = (head.is_am,) + ((head.margin, 0.0) if head.is_am else (head.cos_m, head.sin_m)) + (head.mv_weight,)
    with torch.no_grad():
        _, saved, _ = FRF.mv_softmax_forward(x.cuda(), head.weight.detach().cuda(), label.cuda(), head.scale, mv)
    return saved.rowv.cpu(), saved.cos[:, :head.weight.shape[1]].cpu()


def fp32_rows(x, k, label, is_am, margin):
    """gt and thr per row from fp32 cosines: the host fp32 path's values."""
    rv = MD.from_cos(torch.mm(F.normalize(x), F.normalize(k, dim=0)), label, is_am, margin)[1]
    return rv["gt"], rv["thr"]


def assert_rows(rowv, cos, x, k, label, is_am, margin, st):
    """The device's gt and thr within max(1e-6, 8 x the host fp32 path's own deviation) of the float64 ones, and the hard
    count of the device's own mask inputs (its raw cosines, through ``from_cos`` in float64, and against its own thr) equal
    to the float64 count."""
    h_gt, h_thr = fp32_rows(x, k, label, is_am, margin)
    for i, (name, host) in enumerate((("gt", h_gt), ("thr", h_thr))):
        err = float((rowv[i].double() - st[name]).abs().max())
        bar = max(1e-6, 8 * float((host.double() - st[name]).abs().max()))
        assert err < bar, (name, err, bar)
    assert torch.equal(MD.from_cos(cos.double(), label, is_am, margin)[1]["count"], st["count"])
    hot = torch.zeros_like(cos, dtype=torch.bool).scatter_(1, label.view(-1, 1), True)
    assert torch.equal(((cos > rowv[1].view(-1, 1)) & ~hot).sum(1), st["count"])


@pytest.mark.parametrize("tag", CASES)
def test_device_head_matches_the_reference(g22, tag):
    """g22: logits within the 1e-3 bar, gradients within max(5e-3, 8 x the reference's own fp32-vs-float64 deviation) of
    max|ref| per tensor and the norm of the weight gradient likewise; gt and thr against the fixture's float64 values, and
    the hard counts (see ``assert_rows``)."""
    is_am, margin = bool(g22[tag + ".is_am"]), float(g22[tag + ".margin"])
    if tag.startswith("built"):
        x, k, label, gout = MD.built(synth, tag, 8, D, 100, is_am, margin)
        MD.assert_covers(x, k, label, is_am, margin)
    else:
        x, k, label, gout = MD.random_case(synth, tag, 8, D, 100)
    assert torch.equal(label, torch.from_numpy(g22[tag + ".label"]))
    head = make(100, k, is_am, margin, float(g22[tag + ".mv_weight"]), float(g22[tag + ".scale"])).cuda()
    y, gx, gw = run(head, x.cuda(), label, gout)
    assert head.weight.is_cuda and head.weight.grad.is_cuda and list(head.state_dict()) == ["weight"]
    ref = {n: torch.from_numpy(g22[tag + "." + n]) for n in ("logits", "gx", "gw")}
    figures = {"logits": float((y - ref["logits"]).abs().max())}
    gw_kept = gw.index_select(1, torch.from_numpy(g22[tag + ".gw_index"]))
    for name, got in (("gx", gx), ("gw", gw_kept)):
        assert got.shape == ref[name].shape
        figures[name] = (maxrel(got, ref[name]), max(5e-3, 8 * float(g22[tag + ".dev." + name])))
    figures["gw_norm"] = (abs(float(gw.double().norm()) / float(g22[tag + ".gw_norm"]) - 1),
                          max(5e-3, 8 * float(g22[tag + ".dev.gw"])))
    print(tag, figures)
    assert figures["logits"] < 1e-3, (tag, figures)
    for name in ("gx", "gw", "gw_norm"):
        assert figures[name][0] < figures[name][1], (tag, name, figures)
    rowv, cos = device_rows(head, x, label)
    st = {n: torch.from_numpy(g22["%s.%s" % (tag, n)]) for n in ("gt", "thr", "count")}
    assert_rows(rowv, cos, x, k, label, is_am, margin, st)


@pytest.mark.parametrize("is_am", FORMS)
@pytest.mark.parametrize("N", [1001, 4133])
def test_larger_sizes_against_float64(N, is_am):
    """B = 64 at N = 1001 (neither a multiple of 4 nor of 32: pad columns in ld and Np) and N = 4133 (five 1024-column
    chunks with a ragged last vector), the constructed batch scaled up, against float64: logits within 1e-3, gradients
    within max(1e-3, 8 x the host fp32 run's own deviation) by norm, the row values as in ``assert_rows``."""
    B = 64
    x, k, label, gout = MD.built(synth, "big%d" % N, B, D, N, is_am, 0.35, g_std=1e-3)
    st = MD.assert_covers(x, k, label, is_am, 0.35)
    head = make(N, k, is_am)
    ry, rgx, rgw = float64_reference(head, x, label, gout)
    _, hgx, hgw = run(copy.deepcopy(head), x, label, gout)  # host fp32
    rowv, cos = device_rows(head, x, label)
    y, gx, gw = run(head.cuda(), x.cuda(), label, gout)
    figures = dict(logits=float((y - ry).abs().max()), gx=(relerr(gx, rgx), relerr(hgx, rgx)),
                   gw=(relerr(gw, rgw), relerr(hgw, rgw)))
    print(N, is_am, figures)
    assert figures["logits"] < 1e-3, figures
    for name in ("gx", "gw"):
        assert figures[name][0] < max(1e-3, 8 * figures[name][1]), (name, figures)
    assert_rows(rowv, cos, x, k, label, is_am, 0.35, st)


@pytest.mark.parametrize("is_am", FORMS)
def test_baseline_size_logits_against_float64(is_am):
    """B = 256, N = 28000 (the largest BASELINE head), forward only: logits within 1e-3 of float64, hard counts equal."""
    B, N = 256, 28000
    x, k, label, _ = MD.built(synth, "big28000", B, D, N, is_am, 0.35)
    st = MD.assert_covers(x, k, label, is_am, 0.35)
    head = make(N, k, is_am)
    with torch.no_grad():
        ry = copy.deepcopy(head).double()(x.double(), label)
        rowv, cos = device_rows(head, x, label)
        y = head.cuda()(x.cuda(), label.cuda()).cpu()
    err = float((y - ry).abs().max())
    print("logits", is_am, err, st["min_gap"])
    assert tuple(y.shape) == (B, N) and err < 1e-3
    assert_rows(rowv, cos, x, k, label, is_am, 0.35, st)


# ------------------------------------------------------------------------------------------------ C ABI, guarded


ROWS = 9
NAN_ROW = 7


def hand_made(N):
    """(raw cosines [9, N] fp32, labels [9]).  Negatives lie on the grid of multiples of 1/64 in [-0.5, 0.5] (exact in
    fp32); the target cosines are chosen so that both forms' thresholds (margin 0.35) lie between two grid values.
      row 0: label 0, gt 0.9 (thr 0.55 / 0.696): only the special values below are hard;
      row 1: label N - 1, gt 0.9: no hard negative;
      row 2: label -1, row 3: label N: no target;
      row 4: label 17, gt -0.6: the gt <= 0 branch of the arc form, gt <= margin in the AM form; every grid value hard;
      row 5: label 3, gt 0.2 (thr -0.15 / -0.148): 0 < gt < margin, where the two forms' branches disagree; hard and easy
             grid values;
      row 6: label 9, gt 0.61 (thr 0.26 / 0.301): gt > margin, the AM form's margin applied; hard and easy grid values;
      row 7: label 11, a raw target cosine of 1 + 2^-23: sqrt(1 - gt^2) is NaN in the arc form;
      row 8: label 2, gt -0.3: a third row block with three idle waves.
    Rows 0, 2, 4 and 5 carry raw negatives of 1 + 2^-23, -1 - 2^-22, exactly 1 and exactly -1 in columns 5 .. 8: the head
    never clamps, so all four keep their value and their gradient."""
    cos = torch.round(synth.uniform(MD.SEED, "hand.cos%d" % N, (ROWS, N), -0.5, 0.5) * 64) / 64
    label = torch.tensor([0, N - 1, -1, N, 17, 3, 9, 11, 2])
    for row, gt in ((0, 0.9), (1, 0.9), (4, -0.6), (5, 0.2), (6, 0.61), (7, 1 + 2.0 ** -23), (8, -0.3)):
        cos[row, label[row]] = gt
    for row in (0, 2, 4, 5):
        cos[row, 5:9] = torch.tensor([1 + 2.0 ** -23, -1 - 2.0 ** -22, 1.0, -1.0])
    assert float(cos[0, 5]) > 1.0 and float(cos[0, 6]) < -1.0 and float(cos[NAN_ROW, 11]) > 1.0
    return cos, label


@pytest.mark.parametrize("is_am", FORMS)
@pytest.mark.parametrize("N,ld", [(33, 36), (1000, 1008), (4133, 4136)])
def test_entry_points_on_hand_made_cosines(N, ld, is_am):
    """fr_mv_softmax_apply / _bwd at rows = 9 on ``hand_made``, ld > N with a hot sentinel (+12345, above every threshold)
    in the padding columns of cos, margin 0.35, w = 1.25, every output in a sentinel-filled buffer between guard bands.
    Against ``from_cos`` and its autograd in float64 on the same fp32 cosines: the row values, out / s and gcos / s within
    1e-6 (s = 1 and 64: powers of two, exact factors; |g| <= 1), 0 / +inf / 0 / 0 where there is no target, padding columns
    exactly 0, guard bands intact; NaN exactly where ``from_cos`` has it (the arc form's row with a target cosine of
    1 + 2^-23: its label column, value and gradient, and its thr / final / slope; nowhere in the AM form).  The raw
    cosines beyond +-1 come out unclamped: bit-exact values on the easy ones, a value above that of a raw 1 on the hard
    one, and the gradients s w or s on all four (a clamping kernel with a pass mask gives the bound and 0)."""
    from frhip import ops
    st = ops.current_stream_ptr()
    rows, Np = ROWS, (N + 31) // 32 * 32
    margin, w = 0.35, 1.25
    p0, p1 = (margin, 0.0) if is_am else (math.cos(margin), math.sin(margin))
    raw, label = hand_made(N)
    has = (label >= 0) & (label < N)
    c64 = raw.double().requires_grad_(True)
    ref1, rv = MD.from_cos(c64, label, is_am, margin, w, 1.0)
    gap = (raw.double() - rv["thr"].view(-1, 1)).abs()
    gap[torch.arange(rows)[has], label[has]] = 1.0
    if not is_am:
        gap[NAN_ROW] = 1.0  # its thr is NaN: nothing is hard
    count = rv["count"].tolist()
    assert float(gap.min()) >= 1e-3 and count[0] == 2 and count[1:4] == [0, 0, 0]
    assert count[4] == N - 3 and 0 < count[5] < N - 1 and 0 < count[6] < N - 1  # row 4: all but the label and the two -1s
    dfinal, = torch.autograd.grad(rv["final"].sum(), rv["gt"], retain_graph=True)
    g = synth.uniform(MD.SEED, "hand.g%d" % N, (rows, N), -1.0, 1.0)
    gref1, = torch.autograd.grad(ref1, c64, g.double())
    ref1 = ref1.detach()
    nan_out, nan_g = torch.isnan(ref1), torch.isnan(gref1)
    expect = torch.zeros(rows, N, dtype=torch.bool)
    if not is_am:
        expect[NAN_ROW, label[NAN_ROW]] = True
    assert torch.equal(nan_out, expect) and torch.equal(nan_g, expect)
    cos = torch.full((rows, ld), 12345.0, device="cuda")
    cos[:, :N] = raw.cuda()
    lab = label.cuda()
    want = torch.stack([rv["gt"], rv["thr"], rv["final"], dfinal]).detach()
    for s in (1.0, 64.0):
        rowv, out, gcos = Guarded(4, rows), Guarded(rows, ld), Guarded(rows, Np)
        ops.call("fr_mv_softmax_apply", cos, lab, rowv.t, out.t, rows, N, ld, int(is_am), p0, p1, w, s, st)()
        ops.call("fr_mv_softmax_bwd", g.cuda(), cos, lab, rowv.t, gcos.t, rows, N, ld, Np, w, s, st)()
        torch.cuda.synchronize()
        rowv.assert_guards("rowv")
        got = rowv.t.cpu().double()
        assert torch.equal(got[:, ~has], torch.tensor([[0.0], [float("inf")], [0.0], [0.0]], dtype=torch.float64).expand(4, 2))
        for i, name in enumerate(("gt", "thr", "final", "dfinal")):
            assert torch.equal(torch.isnan(got[i]), torch.isnan(want[i])), (name, got[i], want[i])
            ok = has & ~torch.isnan(want[i])
            err = float((got[i][ok] - want[i][ok]).abs().max())
            assert err <= 1e-6, (name, err, got[i], want[i])
        assert bool(torch.isnan(got[1:, NAN_ROW]).all()) != is_am and float(got[0, NAN_ROW]) == 1 + 2.0 ** -23
        for name, b, ref, nan in (("out", out, ref1, nan_out), ("gcos", gcos, gref1, nan_g)):
            b.assert_guards(name)
            val = b.t[:, :N].cpu().double() / s
            assert torch.equal(torch.isnan(val), nan), name
            err = float((val - ref)[~nan].abs().max())
            assert err < 1e-6, (name, s, err)
            assert not bool(b.t[:, N:].any()), name
        o, gc = out.t.cpu(), gcos.t.cpu()
        big, small = float(torch.tensor(1 + 2.0 ** -23)), float(torch.tensor(-1 - 2.0 ** -22))
        wt = torch.tensor(w)
        # no target: nothing is hard, every cosine passes with its own bits and gradient s
        assert [float(v) for v in o[2, 5:9]] == [big * s, small * s, s, -s]
        assert all(float(gc[2, n]) == float(g[2, n] * s) for n in range(5, 9))
        # row 0: 1 + 2^-23 and 1 are hard (w c + w - 1, above and at 1.5 for w = 1.25), the other two easy
        assert float(o[0, 5]) > float(o[0, 7]) == 1.5 * s and [float(v) for v in o[0, [6, 8]]] == [small * s, -s]
        assert float(gc[0, 5]) == float(g[0, 5] * s * wt) and float(gc[0, 7]) == float(g[0, 7] * s * wt)
        assert float(gc[0, 6]) == float(g[0, 6] * s) and float(gc[0, 8]) == float(g[0, 8] * s)
        # row 4 (thr below -0.8): -1 - 2^-22 and -1 lie below it, easy, unclamped
        assert [float(v) for v in o[4, [6, 8]]] == [small * s, -s] and float(gc[4, 6]) == float(g[4, 6] * s)
    assert bool((cos[:, N:] == 12345.0).all())


# ------------------------------------------------------------------------------------------------ the pipeline


def test_forward_waits_for_no_host_read_and_calls_no_aten_gemm(monkeypatch):
    """torch.profiler over the forward pass (labels validated by the caller, as in train.py): no device-to-host copy, no
    scalar read, no ATen GEMM, and one row kernel (``mv_softmax_apply``; no rows launch); the same over forward + backward
    with torch.mm / matmul / F.linear raising.  The profiler does see such events when they happen (a .item() and a .cpu()
    of a device value as the control)."""
    from frhip import functional as FRF
    B, N = 16, 300
    x, k, label, _ = MD.built(synth, "prof", B, D, N, True, 0.35)
    head = make(N, k, True).cuda()
    xc, lc = x.cuda().requires_grad_(True), label.cuda()
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)
    names = HS.assert_forward_stays_on_device(monkeypatch, head, xc, lc, head.weight)
    assert sum("mv_softmax_apply" in n for n in names) == 1, sorted(set(names))
    assert not any(r + "_rows" in n for n in names for r in ("npcface", "curricular", "magface", "adacos", "mv_softmax"))


@pytest.mark.parametrize("is_am", FORMS)
def test_reproducible_labels_checked_and_empty_batch(monkeypatch, is_am):
    """Bitwise equal logits, both gradients, row values and raw cosines run to run and with FRHIP_SINGLE_STREAM=1 (no side
    stream); an out-of-range label raises the reference's scatter_ error; an empty batch gives [0, N] logits and zero
    gradients."""
    B, N = 96, 7001
    x, k, label, gout = MD.built(synth, "rep", B, D, N, is_am, 0.35)
    head = make(N, k, is_am).cuda()
    xc = x.cuda()
    outs = []
    for single in ("0", "0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        outs.append(run(head, xc, label, gout) + device_rows(head, x, label))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    bad = label.clone()
    bad[3] = N
    with pytest.raises(RuntimeError, match="out of bounds for dimension 1 with size %d" % N):
        head(xc, bad.cuda())
    bad[3] = -1
    with pytest.raises(RuntimeError, match="out of bounds"):
        head(xc, bad.cuda())
    head.weight.grad = None
    xe = torch.empty(0, D, device="cuda", requires_grad=True)
    y = head(xe, torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(y.shape) == (0, N)
    y.sum().backward()
    assert head.weight.grad is not None and not bool(head.weight.grad.any())


def test_attributes_are_read_at_call_time():
    """Changing ``margin`` / ``mv_weight`` / ``scale`` on the module between calls, then ``is_am`` and ``cos_m`` / ``sin_m``
    (which the arc form reads, not ``margin``), changes the device result as it changes the host's: each within 1e-3 of
    the float64 host path, and consecutive settings differ."""
    B, N = 16, 300
    x, k, label, gout = MD.built(synth, "attr", B, D, N, True, 0.35)
    MD.assert_covers(x, k, label, True, 0.35)
    host, dev = make(N, k, True).double(), make(N, k, True).cuda()
    seen = []
    for attrs in ({}, dict(margin=0.5), dict(mv_weight=1.3), dict(scale=64.0), dict(is_am=False),
                  dict(cos_m=math.cos(0.5), sin_m=math.sin(0.5)), dict(margin=0.1)):
        for name, v in attrs.items():
            setattr(host, name, v)
            setattr(dev, name, v)
        with torch.no_grad():
            ry = host(x.double(), label)
            y = dev(x.cuda(), label.cuda()).cpu()
        assert float((y - ry).abs().max()) < 1e-3, attrs
        seen.append(y)
    for a, b in zip(seen[:-2], seen[1:-1]):
        assert float((b - a).abs().max()) > 0.1
    assert torch.equal(seen[-1], seen[-2])  # the arc form does not read ``margin``


# ------------------------------------------------------------------------------------------------ train.py


EPOCHS = 2  # of 6 steps each: the 12 steps of the sibling heads' tests


@pytest.mark.parametrize("is_am", FORMS)
def test_train_py_learns_and_resumes_bit_for_bit_with_mv_softmax(tmp_path, is_am):
    """HEAD_NAME = 'MV_Softmax' on the synthetic config (MV_IS_AM left at its default, or False): 12 steps with finite loss
    that decreases (the mean of the last three steps below the mean of the first three), the Head_* file with the key
    ``weight`` alone; and 12 steps straight == 6 steps, stop at the epoch boundary, resume for 6, bit for bit."""
    cfg = dict(HEAD_NAME="MV_Softmax") if is_am else dict(HEAD_NAME="MV_Softmax", MV_IS_AM=False)
    losses, sd, sa, _ = HS.straight_and_resumed(tmp_path, cfg, "MV_Softmax", EPOCHS)
    assert sum(losses[-3:]) < sum(losses[:3]), losses
    assert list(sd) == ["weight"] and tuple(sd["weight"].shape) == (512, 12) and bool(torch.isfinite(sd["weight"]).all())
    assert not torch.equal(sa["weight"], sd["weight"])  # the head went on moving after the resume
