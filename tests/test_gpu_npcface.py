"""NPCFace on the HIP path (reference head/metrics.py:592-636): the reference's own vectors (g21) with the per-row mean and
count of the hard negatives, larger sizes against a float64 host restatement, the three C entry points alone on hand-made
cosines in sentinel-filled buffers, the pipeline (no device-to-host copy and no ATen GEMM in the forward pass,
bit-reproducible, label errors, the empty batch, the attributes read at call time), and train.py end to end including a
bit-for-bit resume.

The float64 restatement is the head's own host path (plain PyTorch, pinned to g21 by test_npcface_host.py) run on a float64
copy of the module.  The batches are the constructed ones of tests/npcface_data.py: rows in the ``gt <= 0`` branch, rows
without a hard negative and rows with planted ones, none of them near a decision boundary."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_support as HS
import npcface_data as ND
from frhip import synth
from head_support import Guarded, float64_reference, maxrel, relerr, run

pytestmark = pytest.mark.gpu

CASES = ("rand", "built", "built_m03", "built_t12")
ATTRS = ("m0", "m1", "t", "a")
D = 512


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g21(golden_dir):
    return np.load(os.path.join(golden_dir, "g21_npcface.npz"))


def make(N, k, margin=0.5, scale=64, **attrs):
    from head.metrics import NPCFace
    head = NPCFace(D, N, margin=margin, scale=scale)
    for name, v in attrs.items():
        setattr(head, name, v)
    with torch.no_grad():
        head.kernel.copy_(k)
    return head


def device_rows(head, x, label):
    """rowv [6, B] (gt, ctm, final, d final / d gt, avg, count) of the device forward pass, on the host."""
    from frhip import functional as FRF
    npc = (head.cos_m, head.sin_m, head.m0, head.m1, head.t, head.a)
    with torch.no_grad():
        _, saved, _ = FRF.npcface_forward(x.cuda(), head.kernel.detach().cuda(), label.cuda(), head.scale, npc)
    return saved.rowv.cpu()


def fp32_avg(x, k, label, margin):
    """avg of the hard negatives per row from fp32 cosines: the host fp32 path's value."""
    c = torch.mm(F.normalize(x), F.normalize(k, dim=0))
    return ND.from_cos(c, label, margin)[1]["avg"]


@pytest.mark.parametrize("tag", CASES)
def test_device_head_matches_the_reference(g21, tag):
    """g21: logits within the 1e-3 bar, gradients within max(5e-3, 8 x the reference's own fp32-vs-float64 deviation) of
    max|ref| per tensor and the norm of the kernel gradient likewise, avg within max(1e-6, 8 x the host fp32 path's own
    deviation from float64) of the float64 value, the counts equal."""
    x, k, label, gout = (ND.built if tag.startswith("built") else ND.random_case)(synth, tag, 8, D, 100)
    assert torch.equal(label, torch.from_numpy(g21[tag + ".label"]))
    margin = float(g21[tag + ".margin"])
    if tag.startswith("built"):
        ND.assert_covers(x, k, label, margin)
    attrs = {n: float(g21["%s.%s" % (tag, n)]) for n in ATTRS}
    head = make(100, k, margin, float(g21[tag + ".scale"]), **attrs).cuda()
    y, gx, gw = run(head, x.cuda(), label, gout)
    assert head.kernel.is_cuda and head.kernel.grad.is_cuda and list(head.state_dict()) == ["kernel"]
    ref = {n: torch.from_numpy(g21[tag + "." + n]) for n in ("logits", "gx", "gw")}
    figures = {"logits": float((y - ref["logits"]).abs().max())}
    gw_kept = gw.index_select(1, torch.from_numpy(g21[tag + ".gw_index"]))
    for name, got in (("gx", gx), ("gw", gw_kept)):
        assert got.shape == ref[name].shape
        figures[name] = (maxrel(got, ref[name]), max(5e-3, 8 * float(g21[tag + ".dev." + name])))
    figures["gw_norm"] = (abs(float(gw.double().norm()) / float(g21[tag + ".gw_norm"]) - 1),
                          max(5e-3, 8 * float(g21[tag + ".dev.gw"])))
    rowv = device_rows(head, x, label)
    avg64 = torch.from_numpy(g21[tag + ".avg"])
    figures["avg"] = (float((rowv[4].double() - avg64).abs().max()),
                      max(1e-6, 8 * float((fp32_avg(x, k, label, margin).double() - avg64).abs().max())))
    print(tag, figures)
    assert figures["logits"] < 1e-3, (tag, figures)
    for name in ("gx", "gw", "gw_norm", "avg"):
        assert figures[name][0] < figures[name][1], (tag, name, figures)
    assert torch.equal(rowv[5].long(), torch.from_numpy(g21[tag + ".count"])), (tag, rowv[5])


@pytest.mark.parametrize("N", [1001, 4133])
def test_larger_sizes_against_float64(N):
    """B = 64 at N = 1001 (neither a multiple of 4 nor of 32: pad columns) and N = 4133 (just past one 4096-column sweep of
    the 1024-thread, 4-wide row workgroup, with a ragged last vector), the constructed batch scaled up, against float64:
    logits within 1e-3, gradients within max(1e-3, 8 x the host fp32 run's own deviation) by norm, counts equal."""
    B = 64
    x, k, label, gout = ND.built(synth, "big%d" % N, B, D, N, g_std=1e-3)
    st = ND.assert_covers(x, k, label, 0.5)
    head = make(N, k)
    ry, rgx, rgw = float64_reference(head, x, label, gout)
    _, hgx, hgw = run(copy.deepcopy(head), x, label, gout)  # host fp32
    rowv = device_rows(head, x, label)
    y, gx, gw = run(head.cuda(), x.cuda(), label, gout)
    figures = dict(logits=float((y - ry).abs().max()), gx=(relerr(gx, rgx), relerr(hgx, rgx)),
                   gw=(relerr(gw, rgw), relerr(hgw, rgw)))
    print(N, figures)
    assert figures["logits"] < 1e-3, figures
    for name in ("gx", "gw"):
        assert figures[name][0] < max(1e-3, 8 * figures[name][1]), (name, figures)
    assert torch.equal(rowv[5].long(), st["count"])
    assert float((rowv[4].double() - st["avg"]).abs().max()) < max(1e-6, 8 * float(
        (fp32_avg(x, k, label, 0.5).double() - st["avg"]).abs().max()))


def test_baseline_size_logits_and_counts_against_float64():
    """B = 256, N = 28000 (the largest BASELINE head), forward only: logits within 1e-3 of float64, counts equal."""
    B, N = 256, 28000
    x, k, label, _ = ND.built(synth, "big28000", B, D, N)
    st = ND.assert_covers(x, k, label, 0.5)
    head = make(N, k)
    with torch.no_grad():
        ry = copy.deepcopy(head).double()(x.double(), label)
        rowv = device_rows(head, x, label)
        y = head.cuda()(x.cuda(), label.cuda()).cpu()
    err = float((y - ry).abs().max())
    print("logits", err)
    assert tuple(y.shape) == (B, N) and err < 1e-3
    assert torch.equal(rowv[5].long(), st["count"])


# ------------------------------------------------------------------------------------------------ C ABI, guarded


def hand_made(N):
    """(raw cosines [6, N] fp32, labels [6]).  Negatives lie on the grid of multiples of 1/64 in [-0.5, 0.5] (exact in
    fp32); the target cosines are chosen so that cos(theta + 0.5) lies between two grid values.
      row 0: label 0, gt 0.9 (ctm 0.581): only the special values below are hard;
      row 1: label N - 1, gt 0.9: no hard negative, the clamp of the count;
      row 2: label -1, row 3: label N: no target;
      row 4: label 17, gt -0.6 (ctm -0.910): the gt <= 0 branch, every grid value hard;
      row 5: label 3, gt 0.3 (ctm -0.194): hard and easy grid values.
    Rows 0, 2, 4 and 5 carry raw negatives of 1 + 2^-23, -1 - 2^-22, exactly 1 and exactly -1 in columns 5 .. 8: the first
    two clamp (value of the bound, no gradient), the last two pass gradient."""
    cos = torch.round(synth.uniform(ND.SEED, "hand.cos%d" % N, (6, N), -0.5, 0.5) * 64) / 64
    label = torch.tensor([0, N - 1, -1, N, 17, 3])
    for row, gt in ((0, 0.9), (1, 0.9), (4, -0.6), (5, 0.3)):
        cos[row, label[row]] = gt
    for row in (0, 2, 4, 5):
        cos[row, 5:9] = torch.tensor([1 + 2.0 ** -23, -1 - 2.0 ** -22, 1.0, -1.0])
    assert float(cos[0, 5]) > 1.0 and float(cos[0, 6]) < -1.0
    return cos, label


@pytest.mark.parametrize("N,ld", [(33, 36), (1000, 1008), (4133, 4136)])
def test_entry_points_on_hand_made_cosines(N, ld):
    """fr_npcface_rows / _apply / _bwd at rows = 6 (a row block with two idle waves) on ``hand_made``, ld > N with a hot
    sentinel (+12345, which would clamp to a hard 1) in the padding columns of cos, t = 1.25, a = 0.125, margin 0.5,
    m0 = 0.3, m1 = 0.3, every output in a sentinel-filled buffer between guard bands.  Against ``from_cos`` and its autograd
    in float64: the row values, out / s and gcos / s within 1e-6 (s = 1 and 64: powers of two, exact factors; |g| <= 1),
    the counts equal, +inf for ctm where there is no target, padding columns exactly 0, guard bands intact."""
    from frhip import ops
    import math
    st = ops.current_stream_ptr()
    rows, Np = 6, (N + 31) // 32 * 32
    margin, m0, m1, t, a = 0.5, 0.3, 0.3, 1.25, 0.125
    raw, label = hand_made(N)
    c64 = raw.double().requires_grad_(True)
    ref1, rv = ND.from_cos(c64, label, margin, m0, m1, t, a, 1.0)
    gap = (raw.double().clamp(-1, 1) - rv["ctm"].view(-1, 1)).abs()
    gap[torch.arange(rows)[(label >= 0) & (label < N)], label[(label >= 0) & (label < N)]] = 1.0
    assert float(gap.min()) >= 1e-3 and rv["count"].tolist()[1:4] == [0, 0, 0] and int(rv["count"][0]) == 2
    assert int(rv["count"][4]) == N - 3 and 0 < int(rv["count"][5]) < N - 1  # row 4: all but the label and the two -1s
    dfinal, = torch.autograd.grad(rv["final"].sum(), rv["gt"], retain_graph=True)
    g = synth.uniform(ND.SEED, "hand.g%d" % N, (rows, N), -1.0, 1.0)
    gref1, = torch.autograd.grad(ref1, c64, g.double())
    cos = torch.full((rows, ld), 12345.0, device="cuda")
    cos[:, :N] = raw.cuda()
    lab = label.cuda()
    rowv = Guarded(6, rows)
    ops.call("fr_npcface_rows", cos, lab, rowv.t, rows, N, ld, math.cos(margin), math.sin(margin), m0, m1, st)()
    torch.cuda.synchronize()
    rowv.assert_guards("rowv")
    got = rowv.t.cpu().double()
    has = (label >= 0) & (label < N)
    assert torch.equal(got[1][~has], torch.full((2,), float("inf"), dtype=torch.float64))
    want = torch.stack([rv["gt"], rv["ctm"], rv["final"], dfinal, rv["avg"], rv["count"].double()]).detach()
    for i, name in enumerate(("gt", "ctm", "final", "dfinal", "avg", "count")):
        rows_ = has if name == "ctm" else torch.ones_like(has)
        err = float((got[i][rows_] - want[i][rows_]).abs().max())
        assert err <= (0.0 if name == "count" else 1e-6), (name, err, got[i], want[i])
    for s in (1.0, 64.0):
        out, gcos = Guarded(rows, ld), Guarded(rows, Np)
        ops.call("fr_npcface_apply", cos, lab, rowv.t, out.t, rows, N, ld, t, a, s, st)()
        ops.call("fr_npcface_bwd", g.cuda(), cos, lab, rowv.t, gcos.t, rows, N, ld, Np, t, s, st)()
        torch.cuda.synchronize()
        for name, b, ref in (("out", out, ref1.detach()), ("gcos", gcos, gref1)):
            b.assert_guards(name)
            err = float((b.t[:, :N].cpu().double() / s - ref).abs().max())
            assert err < 1e-6, (name, s, err)
            assert not bool(b.t[:, N:].any()), name
        gc = gcos.t.cpu()
        assert float(gc[0, 5]) == 0.0 and float(gc[0, 6]) == 0.0  # clamped: no gradient
        assert float(gc[0, 7]) == float(g[0, 7] * s * torch.tensor(t)) and float(gc[0, 8]) == float(g[0, 8] * s)  # +-1 pass
        assert float(gc[2, 7]) == float(g[2, 7] * s)  # no target: nothing is hard
    assert bool((cos[:, N:] == 12345.0).all())


# ------------------------------------------------------------------------------------------------ the pipeline


def test_forward_waits_for_no_host_read_and_calls_no_aten_gemm(monkeypatch):
    """torch.profiler over the forward pass (labels validated by the caller, as in train.py): no device-to-host copy, no
    scalar read, no ATen GEMM; the same over forward + backward with torch.mm / matmul / F.linear raising.  The profiler
    does see such events when they happen (a .item() and a .cpu() of a device value as the control)."""
    from frhip import functional as FRF
    B, N = 16, 300
    x, k, label, _ = ND.built(synth, "prof", B, D, N)
    head = make(N, k).cuda()
    xc, lc = x.cuda().requires_grad_(True), label.cuda()
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)
    names = HS.assert_forward_stays_on_device(monkeypatch, head, xc, lc, head.kernel)
    assert any("npcface_rows" in n for n in names), sorted(set(names))


def test_reproducible_labels_checked_and_empty_batch(monkeypatch):
    """Bitwise equal logits, both gradients and row values run to run and with FRHIP_SINGLE_STREAM=1 (no side stream); an
    out-of-range label raises the reference's scatter_ error; an empty batch gives [0, N] logits and zero gradients."""
    B, N = 96, 7001
    x, k, label, gout = ND.built(synth, "rep", B, D, N)
    head = make(N, k).cuda()
    xc = x.cuda()
    outs = []
    for single in ("0", "0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        outs.append(run(head, xc, label, gout) + (device_rows(head, x, label),))
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
    head.kernel.grad = None
    xe = torch.empty(0, D, device="cuda", requires_grad=True)
    y = head(xe, torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(y.shape) == (0, N)
    y.sum().backward()
    assert head.kernel.grad is not None and not bool(head.kernel.grad.any())


def test_attributes_are_read_at_call_time():
    """Changing ``t`` / ``a`` (and ``m0`` / ``m1``) on the module between calls changes the device result as it changes the
    host's: each within 1e-3 of the float64 host path, and the two settings differ."""
    B, N = 16, 300
    x, k, label, gout = ND.built(synth, "attr", B, D, N)
    ND.assert_covers(x, k, label, 0.5)
    host, dev = make(N, k).double(), make(N, k).cuda()
    seen = []
    for attrs in ({}, dict(t=1.3, a=0.05), dict(m0=0.3, m1=0.35)):
        for name, v in attrs.items():
            setattr(host, name, v)
            setattr(dev, name, v)
        with torch.no_grad():
            ry = host(x.double(), label)
            y = dev(x.cuda(), label.cuda()).cpu()
        assert float((y - ry).abs().max()) < 1e-3, attrs
        seen.append(y)
    assert float((seen[1] - seen[0]).abs().max()) > 1.0 and float((seen[2] - seen[1]).abs().max()) > 0.1


# ------------------------------------------------------------------------------------------------ train.py


EPOCHS = 4  # of 6 steps each; see test_train_py_learns_and_resumes_bit_for_bit_with_npcface


def test_train_py_learns_and_resumes_bit_for_bit_with_npcface(tmp_path):
    """HEAD_NAME = 'NPCFace' on the synthetic config: 24 steps with finite loss that decreases (the mean of the last three
    steps below the mean of the first three), the Head_* file with the key ``kernel`` alone; and 24 steps straight == 6
    steps, stop at the epoch boundary, resume for 18, bit for bit.

    Why 24 steps where the sibling heads' tests take 12: at the start every negative is hard (cos(theta + margin) ~ -0.48
    lies below all cosines), so every negative logit is lifted to scale * (t c + a) ~ 13 and grows with the spread of the
    features, and the loss first rises.  Measured with this config: 29.4 31.9 30.8 31.0 31.5 28.9 32.7 32.8 34.8 34.2 33.7
    33.5 over steps 1 .. 12, then 19.5 .. 21.1 over steps 13 .. 18 and 5.6 .. 11.9 over steps 19 .. 24 (Prec@1 45 .. 60 %);
    the head's plain-PyTorch arithmetic on the device in place of the HIP path gives the same curve (33.7 at step 12), so
    the rise is the head's, not the kernels'."""
    losses, sd, sa, _ = HS.straight_and_resumed(tmp_path, dict(HEAD_NAME="NPCFace"), "NPCFace", EPOCHS)
    assert sum(losses[-3:]) < sum(losses[:3]), losses
    assert list(sd) == ["kernel"] and tuple(sd["kernel"].shape) == (512, 12) and bool(torch.isfinite(sd["kernel"]).all())
    assert not torch.equal(sa["kernel"], sd["kernel"])  # the head went on moving after the resume
