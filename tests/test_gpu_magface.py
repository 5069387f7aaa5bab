"""MagFace on the HIP path (reference head/metrics.py:512-553): the reference's own vectors (g19), larger sizes against a
float64 host restatement, the two radial paths of the feature gradient on their own (loss_g alone: a closed form; the
margin's dependence on the magnitude), one-sided gradients, label errors, the empty batch, bit reproducibility, no ATen GEMM
in the forward pass, sentinel-filled buffers around the row kernels, and train.py end to end including a bit-for-bit resume.

The float64 restatement is the head's own host path (plain PyTorch, pinned to g19 by test_magface_host.py) run on a float64
copy of the module.  The batches are the constructed ones of tests/magface_data.py: rows below, inside and above
[l_a, u_a], both target branches, none of them near a branch boundary or an end of the clamp."""
import copy
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_support as HS
import magface_data as MD
from frhip import synth
from head_support import SENTINEL, Guarded, maxrel, relerr

pytestmark = pytest.mark.gpu

CASES = ("rand", "built", "built_am", "built_p")
PARAMS = ("margin_am", "scale", "l_a", "u_a", "l_margin", "u_margin", "lamda")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(os.path.join(golden_dir, "g19_magface.npz"))


def make(D, N, k, **kw):
    from head.metrics import MagFace
    head = MagFace(D, N, **kw)
    with torch.no_grad():
        head.weight.copy_(k)
    return head


def run(head, x, label, gout, gg):
    """(logits, loss_g, gx, gweight) of one forward + backward of sum(logits * gout) + sum(loss_g * gg), on whatever
    device x is on; gout or gg None: that output takes no part."""
    x = x.clone().requires_grad_(True)
    head.weight.grad = None
    y, lg = head(x, label.to(x.device))
    outs = [(o, g.to(device=x.device, dtype=o.dtype)) for o, g in ((y, gout), (lg, gg)) if g is not None]
    torch.autograd.backward([o for o, _ in outs], [g for _, g in outs])
    gw = head.weight.grad
    return y.detach().cpu(), lg.detach().cpu(), x.grad.cpu(), None if gw is None else gw.cpu()


def float64_reference(head, x, label, gout, gg):
    h = copy.deepcopy(head).cpu().double()
    return run(h, x.double().cpu(), label.cpu(), None if gout is None else gout.double(), None if gg is None else gg.double())


@pytest.mark.parametrize("tag", CASES)
def test_device_head_matches_the_reference(g19, tag):
    """g19: logits and loss_g within 1e-3 absolute, gradients within max(5e-3, 8 x the reference's own fp32-vs-float64
    deviation) of max|ref| per tensor (the bars of test_device_heads_match_the_reference)."""
    x, k, label, gout, gg = (MD.built if tag.startswith("built") else MD.random_case)(synth, tag, 8, 512, 100)
    assert torch.equal(label, torch.from_numpy(g19[tag + ".label"]))
    assert torch.equal(gout, torch.from_numpy(g19[tag + ".gout"])) and torch.equal(gg, torch.from_numpy(g19[tag + ".gg"]))
    p = {n: float(g19["%s.%s" % (tag, n)]) for n in PARAMS}
    if tag.startswith("built"):
        MD.assert_covers(x, k, label, **p)
    head = make(512, 100, k, **p).cuda()
    y, lg, gx, gw = run(head, x.cuda(), label, gout, gg)
    assert head.weight.is_cuda and head.weight.grad.is_cuda and tuple(lg.shape) == (8, 1)
    ref = {n: torch.from_numpy(g19[tag + "." + n]) for n in ("logits", "loss_g", "gx", "gw")}
    for name, got in (("logits", y), ("loss_g", lg)):
        err = float((got - ref[name]).abs().max())
        print(tag, name, err)
        assert got.shape == ref[name].shape and err < 1e-3, (tag, name, err)
    gw_kept = gw.index_select(1, torch.from_numpy(g19[tag + ".gw_index"]))
    for name, got in (("gx", gx), ("gw", gw_kept)):
        bar = max(5e-3, 8 * float(g19[tag + ".dev." + name]))
        assert got.shape == ref[name].shape
        print(tag, name, maxrel(got, ref[name]), bar)
        assert maxrel(got, ref[name]) < bar, (tag, name, maxrel(got, ref[name]), bar)
    assert abs(float(gw.double().norm()) / float(g19[tag + ".gw_norm"]) - 1) < max(5e-3, 8 * float(g19[tag + ".dev.gw"]))


@pytest.mark.parametrize("N", [1000, 1001, 7000])
def test_larger_sizes_against_float64(N):
    """B = 64 at N = 1000, 1001 (neither a multiple of 4 nor of 32) and 7000, the constructed batch scaled up, against
    float64: logits and loss_g within 1e-3, gradients within max(1e-3, 8 x the host fp32 run's own deviation) by norm."""
    B, D = 64, 512
    x, k, label, gout, gg = MD.built(synth, "big%d" % N, B, D, N, g_std=1e-3)
    MD.assert_covers(x, k, label, **MD.DEFAULTS)
    head = make(D, N, k)
    ry, rlg, rgx, rgw = float64_reference(head, x, label, gout, gg)
    _, _, hgx, hgw = run(copy.deepcopy(head), x, label, gout, gg)  # host fp32
    y, lg, gx, gw = run(head.cuda(), x.cuda(), label, gout, gg)
    assert float((y - ry).abs().max()) < 1e-3 and float((lg - rlg).abs().max()) < 1e-3
    for got, host, ref in ((gx, hgx, rgx), (gw, hgw, rgw)):
        print(N, relerr(got, ref), relerr(host, ref))
        assert relerr(got, ref) < max(1e-3, 8 * relerr(host, ref)), (relerr(got, ref), relerr(host, ref))


def test_baseline_size_logits_against_float64():
    """B = 256, N = 28000 (the largest BASELINE head): logits within 1e-3 of float64."""
    B, D, N = 256, 512, 28000
    x, k, label, _, _ = MD.built(synth, "big28000", B, D, N)
    head = make(D, N, k)
    ref = copy.deepcopy(head).double()
    with torch.no_grad():
        ry, rlg = ref(x.double(), label)
        y, lg = head.cuda()(x.cuda(), label.cuda())
    assert tuple(y.shape) == (B, N) and float((y.cpu() - ry).abs().max()) < 1e-3
    assert tuple(lg.shape) == (B, 1) and float((lg.cpu() - rlg).abs().max()) < 1e-3


@pytest.fixture(scope="module")
def radial():
    """One constructed batch (B = 64, N = 1001) for the radial-path tests: inputs, the module on the device, and the
    float64 quantities the closed forms need."""
    B, D, N = 64, 512, 1001
    x, k, label, gout, gg = MD.built(synth, "radial", B, D, N)
    MD.assert_covers(x, k, label, **MD.DEFAULTS)
    nrm = x.double().norm(dim=1, keepdim=True)
    return dict(B=B, x=x, k=k, label=label, gout=gout, head=make(D, N, k).cuda(), nrm=nrm, xhat=x.double() / nrm,
                inside=((nrm >= 10) & (nrm <= 110)).view(-1))


def test_radial_path_of_loss_g_alone(radial):
    """loss = loss_g.mean(), the logits unused: the weight's gradient is exactly zero, gx[m] = inside * lamda * (1 / u_a^2 -
    1 / a^2) / B * xhat[m] within 1e-6 relative per row (float64 closed form), rows outside [l_a, u_a] exactly zero."""
    B, head = radial["B"], radial["head"]
    x = radial["x"].cuda().requires_grad_(True)
    head.weight.grad = None
    _, lg = head(x, radial["label"].cuda())
    lg.mean().backward()
    assert head.weight.grad is not None and not bool(head.weight.grad.any())
    gx = x.grad.cpu().double()
    inside = radial["inside"]
    assert 0 < int(inside.sum()) < B
    assert not bool(gx[~inside].any())
    want = 20 * (1 / 110.0 ** 2 - 1 / radial["nrm"] ** 2) / B * radial["xhat"]
    err = ((gx - want)[inside].norm(dim=1) / want[inside].norm(dim=1)).max()
    print("radial loss_g rows, max relative error", float(err))
    assert float(err) < 1e-6


def test_radial_path_of_the_margin(radial):
    """A loss on the logits only: for rows inside [l_a, u_a] the component of gx along xhat (zero for a head whose margin
    ignores the magnitude) is non-zero in the margin branch and matches float64 within max(1e-3, 8 x the host fp32 run's
    deviation) by norm; rows outside have none beyond the rounding of the projection (a 512-term fp32 dot product taken
    twice: below 2 x 512 x 2^-24 = 6e-5 of the row's gradient, bar 1e-4)."""
    head, x, label, gout = radial["head"], radial["x"], radial["label"], radial["gout"]
    _, _, rgx, _ = float64_reference(head, x, label, gout, None)
    _, _, hgx, _ = run(copy.deepcopy(head).cpu(), x, label, gout, None)
    _, _, gx, gw = run(head, x.cuda(), label, gout, None)
    assert gw is not None and bool(torch.isfinite(gw).all())
    along = lambda g: (g.double() * radial["xhat"]).sum(dim=1)  # noqa: E731
    inside = radial["inside"]
    ref, host, got = along(rgx)[inside], along(hgx)[inside], along(gx)[inside]
    st = MD.stats64(x, radial["k"], label)
    assert int((ref != 0).sum()) >= st["inside_margin_rows"] > 0
    err, herr = float((got - ref).norm() / ref.norm()), float((host - ref).norm() / ref.norm())
    print("radial margin component: device", err, "host fp32", herr)
    assert err < max(1e-3, 8 * herr)
    outside_scale = rgx[~inside].double().norm(dim=1)
    assert float((along(gx)[~inside].abs() / outside_scale).max()) < 1e-4


def test_one_sided_gradients_and_a_frozen_head(radial):
    """x only, the weight only, and the head under no_grad with x wanting a gradient: each equals the two-sided run bit for
    bit where it is computed."""
    head, label, gout = radial["head"], radial["label"].cuda(), radial["gout"].cuda()
    gg = synth.normal(MD.SEED, "onesided.gg", (radial["B"], 1)).cuda()

    def step(need_x, need_w):
        x = radial["x"].cuda().requires_grad_(need_x)
        head.weight.requires_grad_(need_w)
        head.weight.grad = None
        y, lg = head(x, label)
        torch.autograd.backward([y, lg], [gout, gg])
        return x.grad, head.weight.grad

    try:
        gx, gw = step(True, True)
        gx1, none_w = step(True, False)
        none_x, gw1 = step(False, True)
    finally:
        head.weight.requires_grad_(True)
    assert none_w is None and none_x is None
    assert torch.equal(gx, gx1) and torch.equal(gw, gw1)
    x = radial["x"].cuda().requires_grad_(True)
    with torch.no_grad():
        y, lg = head(x, label)
    assert not y.requires_grad and not lg.requires_grad


def test_labels_checked_minus_one_selects_nothing_and_empty_batch(radial):
    """An out-of-range label raises the reference's scatter_ error; label -1 handed straight to FRF.magface_forward selects
    nothing (the row is s * clamp(cos)); an empty batch gives [0, N] logits, [0, 1] loss_g and zero gradients."""
    from frhip import functional as FRF
    head, x, label = radial["head"], radial["x"].cuda(), radial["label"]
    N = head.weight.shape[1]
    bad = label.clone()
    bad[3] = N
    with pytest.raises(RuntimeError, match="out of bounds for dimension 1 with size %d" % N):
        head(x, bad.cuda())
    bad[3] = -1
    with pytest.raises(RuntimeError, match="out of bounds"):
        head(x, bad.cuda())
    w = head.weight.detach()
    y, _ = head(x, label.cuda())
    y2, lg2, saved, cfg = FRF.magface_forward(x, w, bad.cuda(), 32, 0.0, 10, 110, 0.45, 0.8, 20)
    keep = torch.arange(x.shape[0]) != 3
    assert torch.equal(y2[keep], y.detach()[keep])
    plain = (32 * saved.cos[3, :N].clamp(-1, 1)).cpu()
    assert torch.equal(y2[3].cpu(), plain)
    gx, gw = FRF.magface_backward(saved, cfg, torch.ones_like(y2), torch.ones_like(lg2), True, True)
    assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all())
    head.weight.grad = None
    xe = torch.empty(0, 512, device="cuda", requires_grad=True)
    ye, lge = head(xe, torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(ye.shape) == (0, N) and tuple(lge.shape) == (0, 1)
    (ye.sum() + lge.sum()).backward()
    assert head.weight.grad is not None and not bool(head.weight.grad.any()) and tuple(xe.grad.shape) == (0, 512)


def test_two_runs_are_bit_identical(monkeypatch):
    """Bitwise equal logits, loss_g and both gradients run to run and with FRHIP_SINGLE_STREAM=1 (no side stream)."""
    B, D, N = 64, 512, 1001
    x, k, label, gout, gg = MD.built(synth, "rep", B, D, N)
    head = make(D, N, k).cuda()
    xc = x.cuda()
    outs = []
    for single in ("0", "0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        outs.append(run(head, xc, label, gout, gg))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)


def test_forward_calls_no_aten_gemm(monkeypatch):
    """torch.profiler over the forward pass (labels validated by the caller, as in train.py): no ATen GEMM and no
    device-to-host copy; the same over forward + backward with torch.mm / matmul / F.linear raising.  The profiler does see
    such events when they happen (a torch.mm and a .cpu() as the control)."""
    from frhip import functional as FRF
    B, D, N = 16, 512, 300
    x, k, label, _, _ = MD.built(synth, "prof", B, D, N)
    head = make(D, N, k).cuda()
    xc, lc = x.cuda().requires_grad_(True), label.cuda()
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)
    head(xc, lc)  # first call: streams, allocator
    torch.cuda.synchronize()
    control = HS.profiled_names(lambda: (lc.cpu(), torch.mm(xc.detach(), head.weight.detach())))
    assert "aten::mm" in control and any("DtoH" in n for n in control), sorted(set(control))
    names = HS.profiled_names(lambda: head(xc, lc))
    bad = [n for n in names if n in HS.ATEN_GEMMS or "DtoH" in n or n.startswith("Cijk_")]
    assert not bad, sorted(set(bad))
    HS.forbid_aten_gemm(monkeypatch)
    y, lg = head(xc, lc)
    (y.sum() + lg.mean()).backward()
    torch.cuda.synchronize()
    assert torch.isfinite(xc.grad).all() and torch.isfinite(head.weight.grad).all()


# ------------------------------------------------------------------------------------------------ row kernels, guarded

def test_row_kernels_in_sentinel_filled_buffers():
    """fr_magface_rows / _apply / _bwd at rows = 6 (a row block with two idle waves), N = 1001, ld = 1004, ldg = 1024 with
    raw cosines in [-1.2, 1.2] (both ends of the clamp saturate): every entry of rowv, out [.., :N], gcos [.., :N] and r is
    written and matches the plain-PyTorch arithmetic, columns N..ld of out and N..ldg of gcos read 0 (whatever the padding
    columns of cos hold), and nothing outside the buffers is touched."""
    from frhip import ops
    rows, N, ld, ldg = 6, 1001, 1004, 1024
    s, am, l_a, u_a, l_m, u_m, lam = 32.0, 0.1, 10.0, 110.0, 0.45, 0.8, 20.0
    st = ops.current_stream_ptr()
    cos = torch.full((rows, ld), SENTINEL, device="cuda")
    cos[:, :N] = synth.uniform(MD.SEED, "guard.cos", (rows, N), -1.2, 1.2).cuda()
    label = torch.tensor([0, 1000, 517, -1, 1023, 3], device="cuda")  # first / last column, none, a padding column of gcos
    tc = torch.tensor([0.5, -0.95, 0.9, 0.0, 0.0, 1.1], device="cuda")  # margin, fallback, margin, -, -, saturated
    for m in (0, 1, 2, 5):
        cos[m, label[m]] = tc[m]
    nrm = torch.tensor([5.0, 30.0, 70.0, 109.0, 200.0, 10.5], device="cuda")
    g = synth.normal(MD.SEED, "guard.g", (rows, N)).cuda()
    glossg = synth.normal(MD.SEED, "guard.gg", (rows,)).cuda()
    rowv, out, gcos, r = Guarded(6, rows), Guarded(rows, ld), Guarded(rows, ldg), Guarded(rows)
    xd = F.normalize(synth.normal(MD.SEED, "guard.x", (rows, 20))).cuda() * nrm.view(-1, 1)
    ops.call("fr_magface_rows", xd.contiguous(), rowv.t, rows, 20, l_a, u_a, l_m, u_m, lam, st)()
    ops.call("fr_magface_apply", cos, label, rowv.t, out.t, rows, N, ld, s, am, st)()
    ops.call("fr_magface_bwd", g, glossg, cos, label, rowv.t, gcos.t, r.t, rows, N, ld, ldg, s, l_a, u_a, l_m, u_m, lam, st)()
    torch.cuda.synchronize()
    for name, b in (("rowv", rowv), ("out", out), ("gcos", gcos), ("r", r)):
        b.assert_guards(name)
        assert not bool((b.t == SENTINEL).any()), name
    assert not bool(out.t[:, N:].any()) and not bool(gcos.t[:, N:].any())
    # the same arithmetic through autograd, in float64
    nrm64 = nrm.double().cpu().requires_grad_(True)
    a = nrm64.clamp(l_a, u_a)
    m = (u_m - l_m) / (u_a - l_a) * (a - l_a) + l_m
    c_raw = cos[:, :N].double().cpu().requires_grad_(True)
    c = c_raw.clamp(-1, 1)
    lab = label.cpu()
    has = (lab >= 0) & (lab < N)
    idx = lab.clamp(0, N - 1).view(-1, 1)
    tl = c.gather(1, idx).view(-1)
    ctm = tl * torch.cos(m) - torch.sqrt((1.0 - tl * tl).clamp_min(0)) * torch.sin(m)
    final = torch.where(tl > torch.cos(np.pi - m), ctm, tl - am)
    final = torch.where(has, final, tl)
    want = c.scatter(1, idx, final.view(-1, 1)) * s
    loss_g = lam * (a / u_a ** 2 + 1 / a)
    assert float((out.t[:, :N].cpu() - want.detach()).abs().max()) < 1e-4
    assert float((rowv.t[4].cpu() - loss_g.detach()).abs().max()) < 1e-5
    assert rowv.t[5].cpu().tolist() == [0.0, 1.0, 1.0, 1.0, 0.0, 1.0]
    keep = torch.ones(rows, dtype=torch.bool)
    keep[5] = False  # a saturated target: d sqrt(1 - c^2) is infinite there in autograd; its gcos entry is checked as 0 below
    gc, gn = torch.autograd.grad([want[keep], loss_g], [c_raw, nrm64], [g.double().cpu()[keep], glossg.double().cpu()])
    got = gcos.t[:, :N].cpu().double()
    assert float((got[keep] - gc[keep]).abs().max() / gc[keep].abs().max()) < 1e-5
    assert float(got[5, 3]) == 0.0 and not bool(got[5][c_raw[5].detach().abs() > 1].any())
    assert float((r.t.cpu().double()[keep] - gn[keep]).abs().max() / gn[keep].abs().max()) < 1e-5
    assert float(r.t[0]) == 0.0 and float(r.t[4]) == 0.0


# ------------------------------------------------------------------------------------------------ train.py


def test_train_py_learns_and_resumes_bit_for_bit_with_magface(tmp_path):
    """HEAD_NAME = 'MagFace' on the synthetic config: 12 steps with finite loss that decreases (the mean of the last three
    steps below the mean of the first three), the Head_* file in the reference's layout; and 12 steps straight == 6 steps,
    stop, resume for 6, bit for bit."""
    losses, sd, _, _ = HS.straight_and_resumed(tmp_path, dict(HEAD_NAME="MagFace"), "MagFace")
    assert sum(losses[-3:]) < sum(losses[:3]), losses
    assert list(sd) == ["weight"] and tuple(sd["weight"].shape) == (512, 12) and bool(torch.isfinite(sd["weight"]).all())
