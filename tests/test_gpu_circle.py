"""CircleLoss and the FaceX-Zoo AM_Softmax on the HIP path (reference head/metrics.py:435-473 and :371-392): the reference's
own vectors (g23), larger sizes against a float64 host restatement, the C entry points alone on hand-made cosines in
sentinel-filled buffers (bit for bit against the torch fp32 expression on the same cosines), AM_Softmax against Am_softmax on
identical raw cosines, the pipeline (no device-to-host copy and no ATen GEMM in the forward pass, bit-reproducible, label
errors, the empty batch, the attributes read at call time), and train.py end to end including a bit-for-bit resume.

The float64 restatement is the heads' own host path (plain PyTorch, pinned to g23 by test_circle_host.py) run on a float64
copy of the module.  The batches are the constructed ones of tests/circle_data.py: target cosines near +0.9 and -0.3 and
planted negatives below O_n (dead), just above it and near +0.6, which random embeddings never produce."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import circle_data as CD
import head_support as HS
from frhip import synth
from head_support import Guarded, float64_reference, maxrel, relerr, run

pytestmark = pytest.mark.gpu

CASES = ("circle_rand", "circle_built", "circle_built_m04", "am_rand", "am_built", "am_built_m05")
D = 512
HEADS = [pytest.param("circle", id="CircleLoss"), pytest.param("am", id="AM_Softmax")]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g23(golden_dir):
    return np.load(os.path.join(golden_dir, "g23_circle.npz"))


def make(head, N, k, margin=None, scale=None):
    """The module of ``head`` ("circle" / "am") with the weight k; ``scale`` is CircleLoss's gamma."""
    from head.metrics import AM_Softmax, CircleLoss
    margin = CD.DEFAULTS[head][0] if margin is None else margin
    scale = CD.DEFAULTS[head][1] if scale is None else scale
    mod = CircleLoss(D, N, margin=margin, gamma=scale) if head == "circle" else AM_Softmax(D, N, margin=margin, scale=scale)
    with torch.no_grad():
        mod.weight.copy_(k)
    return mod


def logit_bar(scale):
    """The siblings' 1e-3 was set with scales up to 64; CircleLoss's gamma of 256 makes the same cosine error four times
    larger."""
    return 1e-3 * max(1.0, scale / 64.0)


@pytest.mark.parametrize("tag", CASES)
def test_device_heads_match_the_reference(g23, tag):
    """g23: logits within 1e-3 x max(1, scale / 64) absolute, gradients within max(5e-3, 8 x the reference's own
    fp32-vs-float64 deviation) of max|ref| per tensor and the norm of the weight gradient likewise; in a built CircleLoss
    case the planted dead negatives come out as exactly 0."""
    head = tag.split("_")[0]
    margin, scale = float(g23[tag + ".margin"]), float(g23[tag + ".scale"])
    if "built" in tag:
        x, k, label, gout = CD.built(synth, tag, 8, D, 100, head, margin)
        st = CD.assert_covers(x, k, label, margin)
    else:
        x, k, label, gout = CD.random_case(synth, tag, 8, D, 100)
        st = CD.stats64(x, k, label, margin)
    assert torch.equal(label, torch.from_numpy(g23[tag + ".label"])) and torch.equal(st["dead"], torch.from_numpy(g23[tag + ".dead"]))
    mod = make(head, 100, k, margin, scale).cuda()
    y, gx, gw = run(mod, x.cuda(), label, gout)
    assert mod.weight.is_cuda and mod.weight.grad.is_cuda and list(mod.state_dict()) == ["weight"]
    ref = {n: torch.from_numpy(g23[tag + "." + n]) for n in ("logits", "gx", "gw")}
    figures = {"logits": (float((y - ref["logits"]).abs().max()), logit_bar(scale))}
    gw_kept = gw.index_select(1, torch.from_numpy(g23[tag + ".gw_index"]))
    for name, got in (("gx", gx), ("gw", gw_kept)):
        assert got.shape == ref[name].shape
        figures[name] = (maxrel(got, ref[name]), max(5e-3, 8 * float(g23[tag + ".dev." + name])))
    figures["gw_norm"] = (abs(float(gw.double().norm()) / float(g23[tag + ".gw_norm"]) - 1),
                          max(5e-3, 8 * float(g23[tag + ".dev.gw"])))
    print(tag, figures)
    for name in ("logits", "gx", "gw", "gw_norm"):
        assert figures[name][0] < figures[name][1], (tag, name, figures)
    if head == "circle":
        assert ((y == 0).sum(1) == st["dead"]).all(), ((y == 0).sum(1), st["dead"])


@pytest.mark.parametrize("head", HEADS)
@pytest.mark.parametrize("N", [1001, 4133])
def test_larger_sizes_against_float64(N, head):
    """B = 64 at N = 1001 (neither a multiple of 4 nor of 32: pad columns in ld and Np) and N = 4133 (five 1024-column
    chunks with a ragged last vector), the constructed batch scaled up, against float64: logits within 1e-3 x max(1, scale /
    64), gradients within max(1e-3, 8 x the host fp32 run's own deviation) by norm."""
    B = 64
    margin, scale = CD.DEFAULTS[head]
    x, k, label, gout = CD.built(synth, "big%d" % N, B, D, N, head, margin, g_std=1e-3)
    CD.assert_covers(x, k, label, margin)
    mod = make(head, N, k)
    ry, rgx, rgw = float64_reference(mod, x, label, gout)
    _, hgx, hgw = run(copy.deepcopy(mod), x, label, gout)  # host fp32
    y, gx, gw = run(mod.cuda(), x.cuda(), label, gout)
    figures = dict(logits=float((y - ry).abs().max()), gx=(relerr(gx, rgx), relerr(hgx, rgx)),
                   gw=(relerr(gw, rgw), relerr(hgw, rgw)))
    print(N, head, figures)
    assert figures["logits"] < logit_bar(scale), figures
    for name in ("gx", "gw"):
        assert figures[name][0] < max(1e-3, 8 * figures[name][1]), (name, figures)


@pytest.mark.parametrize("head", HEADS)
def test_baseline_size_logits_against_float64(head):
    """B = 256, N = 28000 (the largest BASELINE head), forward only: logits within 1e-3 x max(1, scale / 64) of float64."""
    B, N = 256, 28000
    margin, scale = CD.DEFAULTS[head]
    x, k, label, _ = CD.built(synth, "big28000", B, D, N, head, margin)
    CD.assert_covers(x, k, label, margin)
    mod = make(head, N, k)
    with torch.no_grad():
        ry = copy.deepcopy(mod).double()(x.double(), label)
        y = mod.cuda()(x.cuda(), label.cuda()).cpu()
    err = float((y - ry).abs().max())
    print("logits", head, err)
    assert tuple(y.shape) == (B, N) and err < logit_bar(scale)


# ------------------------------------------------------------------------------------------------ C ABI, guarded


ROWS = 9  # two full row blocks of four and a third with three idle waves
NAN_ROW = 7
NO_LABEL_ROW = 2


def hand_made(N, margin):
    """(raw cosines [9, N] fp32, labels [9]).  The bulk lies on the grid of multiples of 1/64 in [-0.9, 0.9] (many below
    O_n: dead negatives); rows 0, 2, 4 and 8 carry in columns 5 .. 15 the raw values 1 + 2^-23, -1 - 2^-22, exactly 1,
    exactly -1, 1.5, -1.5, O_n (in fp32), its two fp32 neighbours, O_n - 0.2 and O_n + 0.01.  Row 2 has the label -1 (every
    column a negative), row 3 a label column holding exactly 1, row 4 one holding 1 + 2^-23 (saturated: no gradient), row 5
    one holding exactly -1, row 7 is NaN throughout, and row 8 sits in a third row block with three idle waves."""
    cos = torch.round(synth.uniform(CD.SEED, "hand.cos%d" % N, (ROWS, N), -0.9, 0.9) * 64) / 64
    label = torch.tensor([0, N - 1, -1, 20, 21, 22, 9, 11, 2])
    o_n = torch.tensor(-margin)
    special = torch.stack([torch.tensor(v) for v in (1 + 2.0 ** -23, -1 - 2.0 ** -22, 1.0, -1.0, 1.5, -1.5)]
                          + [o_n, torch.nextafter(o_n, o_n + 1), torch.nextafter(o_n, o_n - 1), o_n - 0.2, o_n + 0.01])
    for row in (0, 2, 4, 8):
        cos[row, 5:16] = special
    cos[3, 20], cos[4, 21], cos[5, 22] = 1.0, 1 + 2.0 ** -23, -1.0
    cos[NAN_ROW] = float("nan")
    assert float(cos[0, 5]) > 1.0 and float(cos[0, 6]) < -1.0 and float(cos[0, 12]) > -margin > float(cos[0, 13])
    return cos, label


def same_bits(got, want):
    """Equal values with NaN in the same places (+0 and -0 count as equal)."""
    return torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got.nan_to_num(7.0), want.nan_to_num(7.0))


@pytest.mark.parametrize("margin,gamma", [(0.25, 256.0), (0.4, 80.0)])
@pytest.mark.parametrize("N,ld", [(33, 36), (1000, 1008), (4133, 4136)])
def test_circle_entry_points_on_hand_made_cosines(N, ld, margin, gamma):
    """fr_circle_apply / fr_circle_bwd at rows = 9 on ``hand_made``, ld > N with a sentinel in the padding columns of cos,
    ldg padded to 32, every output in a sentinel-filled buffer between guard bands.  The logits equal the torch fp32
    expression (``from_cos``, pinned to the reference's lines by test_circle_host.py) on the same cosines bit for bit, NaN
    in the same places (the NaN row and nowhere else); gcos equals (g * gamma) * alpha under the clamp's pass mask bit for
    bit, at gamma 256 and at gamma 80, where g * (gamma * alpha) rounds differently (autograd's order is pinned on the CPU
    by the host test).  Exactly +-1 pass gradient, values beyond do not, O_n and everything below it are dead (0 and 0),
    its upper fp32 neighbour is alive, the row without a label has only negatives; padding columns exactly 0, guard bands
    intact."""
    from frhip import ops
    st = ops.current_stream_ptr()
    rows, Np = ROWS, (N + 31) // 32 * 32
    o_p, o_n, delta_p, delta_n = CD.circle_constants(margin)
    raw, label = hand_made(N, margin)
    g = synth.uniform(CD.SEED, "hand.g%d" % N, (rows, N), -1.0, 1.0)
    want, _, parts = CD.from_cos(raw, label, "circle", margin, gamma)
    gwant = CD.grad_from_cos(raw, label, g, "circle", margin, gamma)
    assert int(torch.isnan(want).sum()) == N and bool(torch.isnan(want[NAN_ROW]).all()) and not bool(torch.isnan(gwant).any())
    assert not bool(parts["hot"][NO_LABEL_ROW].any()) and int(parts["hot"].sum()) == rows - 1
    cos = torch.full((rows, ld), 12345.0, device="cuda")
    cos[:, :N] = raw.cuda()
    lab = label.cuda()
    out, gcos = Guarded(rows, ld), Guarded(rows, Np)
    ops.call("fr_circle_apply", cos, lab, out.t, rows, N, ld, o_p, o_n, delta_p, delta_n, gamma, st)()
    ops.call("fr_circle_bwd", g.cuda(), cos, lab, gcos.t, rows, N, ld, Np, o_p, o_n, gamma, st)()
    torch.cuda.synchronize()
    out.assert_guards("out")
    gcos.assert_guards("gcos")
    o, gc = out.t.cpu(), gcos.t.cpu()
    assert not bool(o[:, N:].any()) and not bool(gc[:, N:].any())  # padding columns: 0, NaN row included
    bad = ~((o[:, :N] == want) | (torch.isnan(o[:, :N]) & torch.isnan(want)))
    assert same_bits(o[:, :N], want), (int(bad.sum()), bad.nonzero()[:8], o[:, :N][bad][:8], want[bad][:8])
    bad = gc[:, :N] != gwant
    assert same_bits(gc[:, :N], gwant), (int(bad.sum()), bad.nonzero()[:8], gc[:, :N][bad][:8], gwant[bad][:8])
    # what the comparison above rests on, spelled out on the special columns of row 0 (a negative in every one)
    gm = torch.tensor(gamma)
    assert float(o[0, 7]) == float(o[0, 5]) == float(o[0, 9]) and float(o[0, 8]) == float(o[0, 6]) == float(o[0, 10]) == 0
    assert float(gc[0, 7]) == float((g[0, 7] * gm) * (1.0 - torch.tensor(o_n))) and float(gc[0, 7]) != 0  # exactly +1 passes
    assert not bool(gc[0, [5, 6, 9, 10]].any())  # beyond +-1: saturated
    assert not bool(o[0, [11, 13, 14]].any()) and not bool(gc[0, [11, 13, 14]].any())  # O_n and below: dead
    assert float(o[0, 12]) != 0 and float(gc[0, 12]) != 0 and float(o[0, 15]) != 0  # just above O_n: alive
    # label columns: exactly 1 passes (alpha_p = margin), 1 + 2^-23 saturates to the same logit without a gradient
    assert float(o[3, 20]) == float(o[4, 21]) != 0 and float(gc[3, 20]) != 0 and float(gc[4, 21]) == 0
    assert float(gc[5, 22]) == float((g[5, 22] * gm) * (torch.tensor(o_p) + 1.0))  # exactly -1 on a label column
    if gamma == 80.0:
        other = torch.where(parts["mask"], g * (gamma * parts["alpha"]), torch.zeros_like(g))
        assert not torch.equal(other, gwant)  # this input does tell the two orders apart
    assert bool((cos[:, N:] == 12345.0).all())


@pytest.mark.parametrize("N,ld", [(33, 36), (1000, 1008), (4133, 4136)])
def test_am_softmax_kernels_on_hand_made_cosines(N, ld):
    """The entry points AM_Softmax runs on -- Am_softmax's fr_margin_apply / fr_margin_apply_bwd with kind 3, called as
    ``am_softmax_n_forward`` calls them (no inv_x, no r_part) -- on the same hand-made cosines, buffers and guard bands:
    scale * (label ? clamp(c) - margin : clamp(c)) and (g * scale) under the pass mask, bit for bit against the torch fp32
    expression, at (0.35, 32) and (0.5, 64)."""
    from frhip import functional as FRF
    from frhip import ops
    st = ops.current_stream_ptr()
    rows, Np = ROWS, (N + 31) // 32 * 32
    raw, label = hand_made(N, 0.35)
    g = synth.uniform(CD.SEED, "hand.g%d" % N, (rows, N), -1.0, 1.0)
    cos = torch.full((rows, ld), 12345.0, device="cuda")
    cos[:, :N] = raw.cuda()
    lab = label.cuda()
    for margin, scale in ((0.35, 32.0), (0.5, 64.0)):
        want = CD.from_cos(raw, label, "am", margin, scale)[0]
        gwant = CD.grad_from_cos(raw, label, g, "am", margin, scale)
        out, gcos = Guarded(rows, ld), Guarded(rows, Np)
        ops.call("fr_margin_apply", cos, lab, None, out.t, rows, N, ld, FRF.AM_SOFTMAX, 0, margin, scale, st)()
        ops.call("fr_margin_apply_bwd", g.cuda(), cos, lab, None, gcos.t, None, rows, N, ld, Np, FRF.AM_SOFTMAX, 0, margin,
                 scale, st)()
        torch.cuda.synchronize()
        out.assert_guards("out")
        gcos.assert_guards("gcos")
        o, gc = out.t.cpu(), gcos.t.cpu()
        assert not bool(o[:, N:].any()) and not bool(gc[:, N:].any())
        assert same_bits(o[:, :N], want) and same_bits(gc[:, :N], gwant)
        assert bool(torch.isnan(o[NAN_ROW, :N]).all()) and not bool(gc[NAN_ROW].any())
        assert float(o[0, 5]) == float(o[0, 7]) == scale and float(gc[0, 7]) == float(g[0, 7] * scale) and float(gc[0, 5]) == 0


def test_am_softmax_is_am_softmax_on_normalised_embeddings():
    """AM_Softmax through its head function against Am_softmax's: handed the rows AM_Softmax normalised, Am_softmax forms
    the identical raw cosines, and then the logits, the saved cosines and the weight gradient are equal bit for bit.  The
    feature gradients differ: Am_softmax returns G = d loss / d (its input), AM_Softmax takes G back through the row
    normalisation, gx = (G - xh (xh . G)) / ||x|| (within 1e-5 of that formula in float64 on the device's own G, by norm)."""
    from frhip import functional as FRF
    B, N = 16, 300
    x, k, label, gout = CD.built(synth, "amvs", B, D, N, "am", 0.35)
    xc, kc, lc, gc = x.cuda(), k.cuda(), label.cuda(), gout.cuda()
    y_n, sv_n, cfg_n = FRF.am_softmax_n_forward(xc, kc, lc, 0.35, 32.0)
    gx_n, gw_n = FRF.am_softmax_n_backward(sv_n, cfg_n, gc, True, True)
    xn = sv_n.xn.clone()
    y_a, sv_a, cfg_a = FRF.margin_ext_forward(xn, kc, lc, FRF.AM_SOFTMAX, 0, 0.35, 32.0)
    G, gw_a = FRF.margin_ext_backward(sv_a, cfg_a, gc, True, True)
    torch.cuda.synchronize()
    assert cfg_n.kind == FRF.AM_SOFTMAX_N and cfg_a.kind == FRF.AM_SOFTMAX and sv_a.inv_x is None and sv_n.inv_x is not None
    assert torch.equal(sv_n.cos, sv_a.cos) and torch.equal(y_n, y_a) and torch.equal(gw_n, gw_a)
    assert float((gx_n - G).norm() / G.norm()) > 0.1  # not the same gradient
    xh, G64 = F.normalize(x.double()), G.double().cpu()
    want = (G64 - xh * (xh * G64).sum(1, keepdim=True)) / x.double().norm(dim=1, keepdim=True)
    err = relerr(gx_n.cpu(), want)
    print("gx against the normalisation backward of Am_softmax's G:", err)
    assert err < 1e-5
    # and the modules: the same data through both classes gives different logits (Am_softmax does not normalise x)
    from head.metrics import Am_softmax
    a = Am_softmax(D, N, None, m=0.35, s=32.0)
    with torch.no_grad():
        a.kernel.copy_(k)
    ya = a.cuda()(xc, lc)
    yn = make("am", N, k).cuda()(xc, lc)
    assert torch.equal(yn.detach(), y_n) and float((ya - yn).detach().abs().max()) > 1.0


# ------------------------------------------------------------------------------------------------ the pipeline


ROW_KERNEL = {"circle": "circle_apply", "am": "margin_apply"}


@pytest.mark.parametrize("head", HEADS)
def test_forward_waits_for_no_host_read_and_calls_no_aten_gemm(monkeypatch, head):
    """torch.profiler over the forward pass (labels validated by the caller, as in train.py): no device-to-host copy, no
    scalar read, no ATen GEMM, and one row kernel (no rows launch); the same over forward + backward with torch.mm / matmul /
    F.linear raising.  The profiler does see such events when they happen (a .item() and a .cpu() of a device value as the
    control)."""
    from frhip import functional as FRF
    B, N = 16, 300
    x, k, label, _ = CD.built(synth, "prof", B, D, N, head, CD.DEFAULTS[head][0])
    mod = make(head, N, k).cuda()
    xc, lc = x.cuda().requires_grad_(True), label.cuda()
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)
    names = HS.assert_forward_stays_on_device(monkeypatch, mod, xc, lc, mod.weight)
    assert sum(ROW_KERNEL[head] in n for n in names) == 1, sorted(set(names))
    assert not any(r + "_rows" in n for n in names for r in ("npcface", "curricular", "magface", "adacos", "mv_softmax", "circle"))


@pytest.mark.parametrize("head", HEADS)
def test_reproducible_labels_checked_and_empty_batch(monkeypatch, head):
    """Bitwise equal logits and both gradients run to run and with FRHIP_SINGLE_STREAM=1 (no side stream); an out-of-range
    label raises the reference's scatter_ error; an empty batch gives [0, N] logits and zero gradients."""
    B, N = 96, 7001
    x, k, label, gout = CD.built(synth, "rep", B, D, N, head, CD.DEFAULTS[head][0])
    mod = make(head, N, k).cuda()
    xc = x.cuda()
    outs = []
    for single in ("0", "0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        outs.append(run(mod, xc, label, gout))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    bad = label.clone()
    bad[3] = N
    with pytest.raises(RuntimeError, match="out of bounds for dimension 1 with size %d" % N):
        mod(xc, bad.cuda())
    bad[3] = -1
    with pytest.raises(RuntimeError, match="out of bounds"):
        mod(xc, bad.cuda())
    mod.weight.grad = None
    xe = torch.empty(0, D, device="cuda", requires_grad=True)
    y = mod(xe, torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(y.shape) == (0, N)
    y.sum().backward()
    assert mod.weight.grad is not None and not bool(mod.weight.grad.any())


def test_attributes_are_read_at_call_time():
    """Changing ``gamma`` / ``O_p`` / ``O_n`` / ``delta_p`` / ``delta_n`` on a CircleLoss module between calls, and
    ``margin`` / ``scale`` on an AM_Softmax module, changes the device result as it changes the host's: each within the logit
    bar of the float64 host path, and consecutive settings differ.  CircleLoss's ``margin`` is read by the constructor alone."""
    B, N = 16, 300
    for head, steps in (("circle", ({}, dict(gamma=64.0), dict(O_p=1.5), dict(O_n=-0.1), dict(delta_p=0.5), dict(delta_n=0.4),
                                    dict(margin=0.9))),
                        ("am", ({}, dict(margin=0.5), dict(scale=64.0)))):
        x, k, label, _ = CD.built(synth, "attr", B, D, N, head, CD.DEFAULTS[head][0])
        host, dev = make(head, N, k).double(), make(head, N, k).cuda()
        seen = []
        for attrs in steps:
            for name, v in attrs.items():
                setattr(host, name, v)
                setattr(dev, name, v)
            with torch.no_grad():
                ry = host(x.double(), label)
                y = dev(x.cuda(), label.cuda()).cpu()
            assert float((y - ry).abs().max()) < logit_bar(float(dev.gamma if head == "circle" else dev.scale)), (head, attrs)
            seen.append(y)
        last = len(seen) - (1 if head == "circle" else 0)
        for a, b in zip(seen[:last - 1], seen[1:last]):
            assert float((b - a).abs().max()) > 0.1
        if head == "circle":
            assert torch.equal(seen[-1], seen[-2])  # ``margin`` is not read after construction, as in the reference


# ------------------------------------------------------------------------------------------------ train.py


EPOCHS = 2  # of 6 steps each: the 12 steps of the sibling heads' tests


@pytest.mark.parametrize("name", ["CircleLoss", "AM_Softmax"])
def test_train_py_runs_and_resumes_bit_for_bit(tmp_path, name):
    """HEAD_NAME = 'CircleLoss' / 'AM_Softmax' on the synthetic config, the reference's defaults: 12 steps with finite loss
    that decreases (the mean of the last three steps below the mean of the first three), the Head_* file with the key
    ``weight`` alone; and 12 steps straight == 6 steps, stop at the epoch boundary, resume for 6, bit for bit.  The loss is
    asserted to fall because the host path falls too: the same loop with the head's forward replaced by its plain-PyTorch
    arithmetic on CPU copies of the features and the weight went from 221.6 to 134.0 with CircleLoss (the device path:
    221.6 to 133.9; gamma = 256 makes the focal loss that large) and from 14.2 to 5.06 with AM_Softmax (5.01)."""
    losses, sd, sa, _ = HS.straight_and_resumed(tmp_path, dict(HEAD_NAME=name), name, EPOCHS)
    assert sum(losses[-3:]) < sum(losses[:3]), losses
    assert list(sd) == ["weight"] and tuple(sd["weight"].shape) == (512, 12) and bool(torch.isfinite(sd["weight"]).all())
    assert not torch.equal(sa["weight"], sd["weight"])  # the head went on moving after the resume
