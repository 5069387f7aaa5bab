"""ArcNegFace on the HIP path (reference head/metrics.py:394-433): the reference's own vectors (g24) with the per-row target
cosine, label value and branch, larger sizes against a float64 host restatement, the two C entry points alone on hand-made
cosines in sentinel-filled buffers (both sides of the fp32 threshold, raw cosines beyond +-1 unclamped, the NaN row, rows
without a target), the pipeline (no device-to-host copy and no ATen GEMM in the forward pass, one row kernel,
bit-reproducible, label errors, the empty batch, the attributes read at call time), and train.py end to end including a
bit-for-bit resume.

The float64 restatement is the head's own host path (plain PyTorch, pinned to g24 bit for bit by test_arcneg_host.py) run on
a float64 copy of the module.  The batches are the constructed ones of tests/arcneg_data.py: target cosines near 0.9, 0.3
and -0.5 on the acos branch and just below thresh on the linear one, none within 1e-3 of the boundary."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import arcneg_data as AD
import head_support as HS
from frhip import synth
from head_support import Guarded, float64_reference, maxrel, relerr, run

pytestmark = pytest.mark.gpu

CASES = ("rand", "built", "built_m03_s32")
D = 512


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g24(golden_dir):
    return np.load(os.path.join(golden_dir, "g24_arcnegface.npz"))


def make(N, w, margin=0.5, scale=64):
    from head.metrics import ArcNegFace
    head = ArcNegFace(D, N, margin=margin, scale=scale)
    with torch.no_grad():
        head.weight.copy_(w)
    return head


def device_rows(head, x, label):
    """(rowv [3, B] (gt, a, d a / d gt), raw cosines [B, N]) of the device forward pass, on the host."""
    from frhip import functional as FRF
    arc = (head.thresh, head.margin, head.mm, head.alpha, head.sigma)
    with torch.no_grad():
        _, saved, _ = FRF.arcneg_forward(x.cuda(), head.weight.detach().cuda(), label.cuda(), head.scale, arc)
    return saved.rowv.cpu(), saved.cos[:, :head.weight.shape[0]].cpu()


def fp32_rows(x, w, label, margin):
    """gt and a per row from fp32 cosines: the host fp32 path's values."""
    c = torch.mm(x / torch.norm(x, 2, 1, keepdim=True), (w / torch.norm(w, 2, 1, keepdim=True)).t())
    rv = AD.from_cos(c, label, margin)[1]
    return rv["gt"].detach(), rv["a"].detach()


def assert_rows(rowv, x, w, label, margin, st):
    """The device's gt and a within max(1e-6, 8 x the host fp32 path's own deviation) of the float64 ones, and its branch
    per row (the stored slope is exactly 1 on the linear branch; its own gt against the threshold it was given) equal to
    the float64 branch."""
    from frhip import functional as FRF
    h_gt, h_a = fp32_rows(x, w, label, margin)
    figures = {}
    for i, (name, host) in enumerate((("gt", h_gt), ("a", h_a))):
        err = float((rowv[i].double() - st[name]).abs().max())
        bar = max(1e-6, 8 * float((host.double() - st[name]).abs().max()))
        figures[name] = (err, bar)
    print("rows", figures)
    for name, (err, bar) in figures.items():
        assert err < bar, (name, err, bar)
    branch = st["branch"].bool()
    assert torch.equal(rowv[2] != 1.0, branch)
    assert torch.equal(rowv[0] > FRF.arcneg_thresh32(AD.thresh_of(margin)), branch)


@pytest.mark.parametrize("tag", CASES)
def test_device_head_matches_the_reference(g24, tag):
    """g24: logits within the 1e-3 bar, gradients within max(5e-3, 8 x the reference's own fp32-vs-float64 deviation) of
    max|ref| per tensor and the norm of the weight gradient likewise; gt and a against the fixture's float64 values and the
    branch per row equal (see ``assert_rows``)."""
    margin, scale = float(g24[tag + ".margin"]), float(g24[tag + ".scale"])
    if tag.startswith("built"):
        x, w, label, gout = AD.built(synth, tag, 8, D, 100, margin)
        AD.assert_covers(x, w, label, margin)
    else:
        x, w, label, gout = AD.random_case(synth, tag, 8, D, 100)
    assert torch.equal(label, torch.from_numpy(g24[tag + ".label"]))
    head = make(100, w, margin, int(scale)).cuda()
    y, gx, gw = run(head, x.cuda(), label, gout)
    assert head.weight.is_cuda and head.weight.grad.is_cuda and list(head.state_dict()) == ["weight"]
    ref = {n: torch.from_numpy(g24[tag + "." + n]) for n in ("logits", "gx", "gw")}
    figures = {"logits": float((y - ref["logits"]).abs().max())}
    gw_kept = gw.index_select(0, torch.from_numpy(g24[tag + ".gw_index"]))
    for name, got in (("gx", gx), ("gw", gw_kept)):
        assert got.shape == ref[name].shape
        figures[name] = (maxrel(got, ref[name]), max(5e-3, 8 * float(g24[tag + ".dev." + name])))
    figures["gw_norm"] = (abs(float(gw.double().norm()) / float(g24[tag + ".gw_norm"]) - 1),
                          max(5e-3, 8 * float(g24[tag + ".dev.gw"])))
    print(tag, figures)
    assert figures["logits"] < 1e-3, (tag, figures)
    for name in ("gx", "gw", "gw_norm"):
        assert figures[name][0] < figures[name][1], (tag, name, figures)
    rowv, _ = device_rows(head, x, label)
    st = {n: torch.from_numpy(g24["%s.%s" % (tag, n)]) for n in ("gt", "a", "branch")}
    assert_rows(rowv, x, w, label, margin, st)


@pytest.mark.parametrize("N", [1001, 4133])
def test_larger_sizes_against_float64(N):
    """B = 64 at N = 1001 (neither a multiple of 4 nor of 32: pad columns in ld and Np) and N = 4133 (five 1024-column
    chunks with a ragged last vector), the constructed batch scaled up, against float64: logits within 1e-3, gradients
    within max(1e-3, 8 x the host fp32 run's own deviation) by norm, the row values as in ``assert_rows``."""
    B = 64
    x, w, label, gout = AD.built(synth, "big%d" % N, B, D, N, g_std=1e-3)
    st = AD.assert_covers(x, w, label, 0.5)
    head = make(N, w)
    ry, rgx, rgw = float64_reference(head, x, label, gout)
    _, hgx, hgw = run(copy.deepcopy(head), x, label, gout)  # host fp32
    rowv, _ = device_rows(head, x, label)
    y, gx, gw = run(head.cuda(), x.cuda(), label, gout)
    figures = dict(logits=float((y - ry).abs().max()), gx=(relerr(gx, rgx), relerr(hgx, rgx)),
                   gw=(relerr(gw, rgw), relerr(hgw, rgw)))
    print(N, figures)
    assert figures["logits"] < 1e-3, figures
    for name in ("gx", "gw"):
        assert figures[name][0] < max(1e-3, 8 * figures[name][1]), (name, figures)
    assert_rows(rowv, x, w, label, 0.5, st)


def test_baseline_size_logits_against_float64():
    """B = 256, N = 28000 (the largest BASELINE head), forward only: logits within 1e-3 of float64, the row values as in
    ``assert_rows``."""
    B, N = 256, 28000
    x, w, label, _ = AD.built(synth, "big28000", B, D, N)
    st = AD.assert_covers(x, w, label, 0.5)
    head = make(N, w)
    with torch.no_grad():
        ry = copy.deepcopy(head).double()(x.double(), label)
        rowv, _ = device_rows(head, x, label)
        y = head.cuda()(x.cuda(), label.cuda()).cpu()
    err = float((y - ry).abs().max())
    print("logits", err, st["gap"])
    assert tuple(y.shape) == (B, N) and err < 1e-3
    assert_rows(rowv, x, w, label, 0.5, st)


# ------------------------------------------------------------------------------------------------ C ABI, guarded


ROWS = 9
NAN_ROW = 7
MARGIN = 0.5
BIG, SMALL = 1 + 2.0 ** -23, -1 - 2.0 ** -22
RAW_ROWS = (0, 2, 4, 8)


def hand_made(N, t32):
    """(raw cosines [9, N] fp32, labels [9]).  Negatives lie on the grid of multiples of 1/64 in [-0.5, 0.5] (exact in
    fp32).  ``t32`` is the fp32 threshold the kernel is given.
      row 0: label 0, gt 0.9;        row 1: label N - 1, gt 0.9: the acos branch at both ends of the row;
      row 2: label -1, row 3: label N: no target;
      row 4: label 17, gt -0.95: the linear branch;
      row 5: label 3, gt == t32: not above it, the linear branch;
      row 6: label 9, gt == the fp32 value above t32: the acos branch (a differs by about 0.117 across the boundary);
      row 7: label 11, a raw target cosine of 1 + 2^-23: acos is NaN, and with it the whole row;
      row 8: label 2, gt -0.3: a third row block with three idle waves.
    Rows 0, 2, 4 and 8 carry raw negatives of 1 + 2^-23, -1 - 2^-22, exactly 1 and exactly -1 in columns 5 .. 8: the head
    never clamps, so all four keep their value and their gradient."""
    cos = torch.round(synth.uniform(AD.SEED, "hand.cos%d" % N, (ROWS, N), -0.5, 0.5) * 64) / 64
    label = torch.tensor([0, N - 1, -1, N, 17, 3, 9, 11, 2])
    above = float(torch.nextafter(torch.tensor(t32), torch.tensor(1.0)))
    for row, gt in ((0, 0.9), (1, 0.9), (4, -0.95), (5, t32), (6, above), (7, BIG), (8, -0.3)):
        cos[row, label[row]] = gt
    for row in RAW_ROWS:
        cos[row, 5:9] = torch.tensor([BIG, SMALL, 1.0, -1.0])
    assert float(cos[0, 5]) > 1.0 and float(cos[0, 6]) < -1.0 and float(cos[NAN_ROW, 11]) > 1.0
    assert float(cos[5, 3]) == t32 < float(cos[6, 9]) == above
    return cos, label


def row_values(rv):
    """[3, rows]: gt, a and d a / d gt of a ``from_cos`` result (autograd through a)."""
    da, = torch.autograd.grad(rv["a"].sum(), rv["gt"], retain_graph=True)
    return torch.stack([rv["gt"], rv["a"], da]).detach()


@pytest.mark.parametrize("N,ld", [(33, 36), (1000, 1008), (4133, 4136)])
def test_entry_points_on_hand_made_cosines(N, ld):
    """fr_arcneg_apply / _bwd at rows = 9 on ``hand_made``, ld > N with a 12345 sentinel in the padding columns of cos,
    margin 0.5, alpha 1.2, sigma 2, every output in a sentinel-filled buffer between guard bands.  Against ``from_cos`` and
    its autograd in float64 on the same fp32 cosines (the branch taken against the double thresh, as the reference takes
    it; the kernel gets the largest fp32 not above it): the row values, out / s and gcos / s (s = 1 and 64: powers of two,
    exact factors; |g| <= 1) within max(2e-6, 8 x the deviation of the torch fp32 expression on the same cosines from
    float64) -- 2e-6 is about eight fp32 ulps at the largest magnitude, alpha * 2 + 1; 0 / 0 / 0 where there is no target,
    and there out == s * c and gcos == g * s bit for bit; padding columns exactly 0, guard bands and the sentinel intact;
    the row with a target cosine of 1 + 2^-23 NaN in every column of out and gcos, and NaN nowhere else; the raw negatives
    beyond and at +-1 with their gradient g * s * t, not 0."""
    from frhip import functional as FRF, ops
    st = ops.current_stream_ptr()
    rows, Np = ROWS, (N + 31) // 32 * 32
    thresh, mm = AD.thresh_of(MARGIN), math.sin(math.pi - MARGIN) * MARGIN
    t32 = FRF.arcneg_thresh32(thresh)
    assert t32 < thresh  # cos(pi - 0.5) rounds up to fp32: the value passed lies one ulp below the nearest
    raw, label = hand_made(N, t32)
    has = (label >= 0) & (label < N)
    c64 = raw.double().requires_grad_(True)
    ref1, rv = AD.from_cos(c64, label, MARGIN, AD.ALPHA, AD.SIGMA, 1.0)
    assert rv["branch"].tolist() == [True, True, False, False, False, False, True, True, True]
    want = row_values(rv)
    assert abs(float(want[1, 6] - want[1, 5]) - 0.1173) < 1e-3  # a across the boundary: a wrong branch shows
    g = synth.uniform(AD.SEED, "hand.g%d" % N, (rows, N), -1.0, 1.0)
    gref1, = torch.autograd.grad(ref1, c64, g.double())
    ref1 = ref1.detach()
    nan_rows = torch.zeros(rows, N, dtype=torch.bool)
    nan_rows[NAN_ROW] = True
    assert torch.equal(torch.isnan(ref1), nan_rows) and torch.equal(torch.isnan(gref1), nan_rows)
    # the torch fp32 expression on the same cosines: its deviation from float64 sets the bars
    c32 = raw.clone().requires_grad_(True)
    f1, fv = AD.from_cos(c32, label, MARGIN, AD.ALPHA, AD.SIGMA, 1.0)
    fg1, = torch.autograd.grad(f1, c32, g, retain_graph=True)
    frow = row_values(fv)
    ok_rows = ~torch.isnan(want)

    def dev(a, b, ok):
        return float((a.detach().double() - b)[ok].abs().max())

    bars = dict(out=max(2e-6, 8 * dev(f1, ref1, ~nan_rows)), gcos=max(2e-6, 8 * dev(fg1, gref1, ~nan_rows)),
                rowv=max(2e-6, 8 * dev(frow, want, ok_rows)))
    cos = torch.full((rows, ld), 12345.0, device="cuda")
    cos[:, :N] = raw.cuda()
    lab = label.cuda()
    for s in (1.0, 64.0):
        rowv, out, gcos = Guarded(3, rows), Guarded(rows, ld), Guarded(rows, Np)
        ops.call("fr_arcneg_apply", cos, lab, rowv.t, out.t, rows, N, ld, t32, MARGIN, mm, AD.ALPHA, float(AD.SIGMA), s, st)()
        ops.call("fr_arcneg_bwd", g.cuda(), cos, lab, rowv.t, gcos.t, rows, N, ld, Np, AD.ALPHA, float(AD.SIGMA), s, st)()
        torch.cuda.synchronize()
        rowv.assert_guards("rowv")
        got = rowv.t.cpu().double()
        assert torch.equal(got[:, ~has], torch.zeros(3, 2, dtype=torch.float64))
        assert torch.equal(torch.isnan(got), torch.isnan(want)), (got, want)
        assert bool(torch.isnan(got[1:, NAN_ROW]).all()) and float(got[0, NAN_ROW]) == BIG
        assert float(got[2, 4]) == 1.0 and float(got[2, 5]) == 1.0 and float(got[2, 6]) != 1.0  # the branch at the boundary
        errs = dict(rowv=float((got - want)[ok_rows].abs().max()))
        for name, b, ref in (("out", out, ref1), ("gcos", gcos, gref1)):
            b.assert_guards(name)
            val = b.t[:, :N].cpu().double() / s
            assert torch.equal(torch.isnan(val), nan_rows), name
            errs[name] = float((val - ref)[~nan_rows].abs().max())
            assert not bool(b.t[:, N:].any()), name
        print("N = %d, s = %g: errors %s, bars %s" % (N, s, errs, bars))
        for name in errs:
            assert errs[name] < bars[name], (name, s, errs, bars)
        o, gc = out.t.cpu(), gcos.t.cpu()
        # no target: t is exactly 1, every cosine passes with its own bits and gradient g * s
        for row in (2, 3):
            assert torch.equal(o[row, :N], raw[row] * s) and torch.equal(gc[row, :N], g[row] * s)
        assert [float(v) for v in o[2, 5:9]] == [BIG * s, SMALL * s, s, -s]
        # the raw negatives beyond and at +-1 of the rows with a target: gradient g * s * t, not 0 (no pass mask)
        for row in (0, 4, 8):
            t = AD.ALPHA * torch.exp(-(raw[row, 5:9].double() - want[1, row]) ** 2 / AD.SIGMA)
            assert float((gc[row, 5:9].double() / s - g[row, 5:9].double() * t).abs().max()) < bars["gcos"]
            assert bool((gc[row, 5:9] != 0).all()) and float(t.min()) > 0.05
    assert bool((cos[:, N:] == 12345.0).all())


# ------------------------------------------------------------------------------------------------ the pipeline


def test_forward_waits_for_no_host_read_and_calls_no_aten_gemm(monkeypatch):
    """torch.profiler over the forward pass (labels validated by the caller, as in train.py): no device-to-host copy, no
    scalar read, no ATen GEMM, and exactly one row kernel (``arcneg_apply``; no ``*_rows`` launch); the same over forward
    + backward with torch.mm / matmul / F.linear raising.  The profiler does see such events when they happen (a .item()
    and a .cpu() of a device value as the control)."""
    from frhip import functional as FRF
    B, N = 16, 300
    x, w, label, _ = AD.built(synth, "prof", B, D, N)
    head = make(N, w).cuda()
    xc, lc = x.cuda().requires_grad_(True), label.cuda()
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)
    names = HS.assert_forward_stays_on_device(monkeypatch, head, xc, lc, head.weight)
    assert sum("arcneg_apply" in n for n in names) == 1, sorted(set(names))
    assert not any(r + "_rows" in n for n in names
                   for r in ("npcface", "curricular", "magface", "adacos", "mv_softmax", "arcneg"))


def test_reproducible_labels_checked_and_empty_batch(monkeypatch):
    """Bitwise equal logits, both gradients, row values and raw cosines run to run and with FRHIP_SINGLE_STREAM=1 (no side
    stream); an out-of-range label raises the shared label check's error (the reference would wrap -1 to the last class);
    an empty batch gives [0, N] logits and zero gradients."""
    B, N = 96, 7001
    x, w, label, gout = AD.built(synth, "rep", B, D, N)
    head = make(N, w).cuda()
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
    assert xe.grad is not None and tuple(xe.grad.shape) == (0, D)


def test_attributes_are_read_at_call_time():
    """Changing ``margin`` (with ``thresh`` / ``mm``), ``scale``, ``alpha`` and ``sigma`` on the module between calls changes
    the device result as it changes the float64 host result: each setting within 1e-3 of the float64 host path, and
    consecutive settings differ."""
    B, N = 16, 300
    x, w, label, gout = AD.built(synth, "attr", B, D, N)
    AD.assert_covers(x, w, label, 0.5)
    assert AD.stats64(x, w, label, 0.3)["gap"] >= 1e-3  # the batch keeps clear of the second setting's threshold too
    host, dev = make(N, w).double(), make(N, w).cuda()
    seen = []
    for attrs in ({}, dict(margin=0.3, thresh=math.cos(math.pi - 0.3), mm=math.sin(math.pi - 0.3) * 0.3), dict(scale=32),
                  dict(alpha=1.0), dict(sigma=3)):
        for name, v in attrs.items():
            setattr(host, name, v)
            setattr(dev, name, v)
        with torch.no_grad():
            ry = host(x.double(), label)
            y = dev(x.cuda(), label.cuda()).cpu()
        assert float((y - ry).abs().max()) < 1e-3, attrs
        seen.append(y)
    for a, b in zip(seen[:-1], seen[1:]):
        assert float((b - a).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ train.py


EPOCHS = 2  # of 6 steps each: the 12 steps of the sibling heads' tests


def test_train_py_learns_and_resumes_bit_for_bit_with_arcnegface(tmp_path):
    """HEAD_NAME = 'ArcNegFace' on the synthetic config: 12 steps with finite loss that decreases (the mean of the last
    three steps below the mean of the first three), the Head_* file with the key ``weight`` alone, [12, 512]; and 12 steps
    straight == 6 steps, stop at the epoch boundary, resume for 6, bit for bit."""
    losses, sd, sa, _ = HS.straight_and_resumed(tmp_path, dict(HEAD_NAME="ArcNegFace"), "ArcNegFace", EPOCHS)
    assert sum(losses[-3:]) < sum(losses[:3]), losses
    assert list(sd) == ["weight"] and tuple(sd["weight"].shape) == (12, 512) and bool(torch.isfinite(sd["weight"]).all())
    assert not torch.equal(sa["weight"], sd["weight"])  # the head went on moving after the resume
