"""CurricularFace on the HIP path (reference head/metrics.py:475-510): the reference's own vectors (g18), larger sizes
against a float64 host restatement, ``t`` kept on the device (its trajectory, no device-to-host copy and no ATen GEMM in the
forward pass, bit-reproducible), label errors, the empty batch, and train.py end to end including a bit-for-bit resume.

The float64 restatement is the head's own host path (plain PyTorch, pinned to g18 by test_curricular_host.py) run on a
float64 copy of the module.  The batches are the constructed ones of tests/curricular_data.py: easy and hard negatives and
both target branches, none of them near a decision boundary."""
import copy
import os

import numpy as np
import pytest
import torch

import curricular_data as CD
import head_support as HS
from frhip import synth
from head_support import maxrel, relerr

pytestmark = pytest.mark.gpu

CASES = ("rand_t0", "built_t0", "built_t03", "built_m03")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_curricular.npz"))


def make(D, N, k, t0=0.0, **kw):
    from head.metrics import CurricularFace
    head = CurricularFace(D, N, **kw)
    with torch.no_grad():
        head.kernel.copy_(k)
        head.t.fill_(t0)
    return head


def run(head, x, label, gout):
    """(logits, gx, gkernel, t after the call) of one forward + backward, on whatever device x is on."""
    x = x.clone().requires_grad_(True)
    head.kernel.grad = None
    y = head(x, label.to(x.device))
    y.backward(gout.to(device=x.device, dtype=y.dtype))
    return y.detach().cpu(), x.grad.cpu(), head.kernel.grad.cpu(), head.t.detach().cpu().clone()


def float64_reference(head, x, label, gout):
    h = copy.deepcopy(head).cpu().double()
    return run(h, x.double().cpu(), label.cpu(), gout.double().cpu())


@pytest.mark.parametrize("tag", CASES)
def test_device_head_matches_the_reference(g18, tag):
    """g18: logits within the 1e-3 bar, gradients within max(5e-3, 8 x the reference's own fp32-vs-float64 deviation) of
    max|ref| per tensor (the bars of test_device_heads_match_the_reference), t within max(1e-6, 8 x the host fp32
    restatement's own deviation from float64) of the float64 value."""
    x, k, label, gout = (CD.built if tag.startswith("built") else CD.random_case)(synth, tag, 8, 512, 100)
    assert torch.equal(label, torch.from_numpy(g18[tag + ".label"]))
    m, s, t0 = float(g18[tag + ".m"]), float(g18[tag + ".s"]), float(g18[tag + ".t0"])
    if tag.startswith("built"):
        CD.assert_covers_both_branches(x, k, label, m)
    host = make(512, 100, k, t0, m=m, s=s)
    host(x, label)
    head = make(512, 100, k, t0, m=m, s=s).cuda()
    y, gx, gw, t = run(head, x.cuda(), label, gout)
    assert head.kernel.is_cuda and head.kernel.grad.is_cuda and head.t.is_cuda and tuple(head.t.shape) == (1,)
    ref = {n: torch.from_numpy(g18[tag + "." + n]) for n in ("logits", "gx", "gw")}
    assert float((y - ref["logits"]).abs().max()) < 1e-3
    gw_kept = gw.index_select(1, torch.from_numpy(g18[tag + ".gw_index"]))
    for name, got in (("gx", gx), ("gw", gw_kept)):
        bar = max(5e-3, 8 * float(g18[tag + ".dev." + name]))
        assert got.shape == ref[name].shape
        assert maxrel(got, ref[name]) < bar, (tag, name, maxrel(got, ref[name]), bar)
    assert abs(float(gw.double().norm()) / float(g18[tag + ".gw_norm"]) - 1) < max(5e-3, 8 * float(g18[tag + ".dev.gw"]))
    t64 = float(g18[tag + ".t64"][0])
    bar = max(1e-6, 8 * abs(float(host.t) - t64))
    assert abs(float(t) - t64) < bar, (tag, float(t), t64, bar)


@pytest.mark.parametrize("N", [1000, 1001, 7000])
def test_larger_sizes_against_float64(N):
    """B = 64 at N = 1000, 1001 (neither a multiple of 4 nor of 32) and 7000, the constructed batch scaled up, against
    float64: logits within 1e-3, gradients within max(1e-3, 8 x the host fp32 run's own deviation) by norm."""
    B, D = 64, 512
    x, k, label, gout = CD.built(synth, "big%d" % N, B, D, N, g_std=1e-3)
    CD.assert_covers_both_branches(x, k, label, 0.5)
    head = make(D, N, k, 0.25)
    ry, rgx, rgw, rt = float64_reference(head, x, label, gout)
    _, hgx, hgw, ht = run(copy.deepcopy(head), x, label, gout)  # host fp32
    y, gx, gw, t = run(head.cuda(), x.cuda(), label, gout)
    assert float((y - ry).abs().max()) < 1e-3
    for got, host, ref in ((gx, hgx, rgx), (gw, hgw, rgw)):
        assert relerr(got, ref) < max(1e-3, 8 * relerr(host, ref)), (relerr(got, ref), relerr(host, ref))
    assert abs(float(t) - float(rt)) < max(1e-6, 8 * abs(float(ht) - float(rt)))


def test_baseline_size_logits_against_float64():
    """B = 256, N = 28000 (the largest BASELINE head): logits within 1e-3 of float64."""
    B, D, N = 256, 512, 28000
    x, k, label, gout = CD.built(synth, "big28000", B, D, N)
    CD.assert_covers_both_branches(x, k, label, 0.5)
    head = make(D, N, k, 0.25)
    ref = copy.deepcopy(head).double()
    with torch.no_grad():
        ry = ref(x.double(), label)
        y = head.cuda()(x.cuda(), label.cuda()).cpu()
    assert tuple(y.shape) == (B, N) and float((y - ry).abs().max()) < 1e-3
    assert abs(float(head.t) - float(ref.t)) < 1e-6


def test_t_follows_the_restatement_over_three_calls():
    """Three consecutive forward calls on three batches (the last two under no_grad / in eval mode: the reference moves t
    on every call): t after each within max(1e-6, 8 x the host fp32 run's deviation) of the float64 run."""
    B, D, N = 16, 512, 300
    _, k, _, _ = CD.built(synth, "traj0", B, D, N)
    dev, h32 = make(D, N, k).cuda(), make(D, N, k)
    h64 = make(D, N, k).double()
    seen = []
    for step in range(3):
        # the first batch is built around k (target cosines ~0.9 and ~-0.97), the later ones are random (~0)
        x, _, label, _ = (CD.built if step == 0 else CD.random_case)(synth, "traj%d" % step, B, D, N)
        if step == 2:
            dev.eval(), h32.eval(), h64.eval()
        with torch.no_grad():
            dev(x.cuda(), label.cuda())
            h32(x, label)
            h64(x.double(), label)
        t, t32, t64 = float(dev.t), float(h32.t), float(h64.t)
        assert abs(t - t64) < max(1e-6, 8 * abs(t32 - t64)), (step, t, t32, t64)
        seen.append(t64)
    assert seen[0] != 0.0 and len(set(seen)) == 3


def test_forward_keeps_t_on_the_device_and_calls_no_aten_gemm(monkeypatch):
    """torch.profiler over the forward pass (labels validated by the caller, as in train.py): no device-to-host copy, no
    scalar read, no ATen GEMM; the same over forward + backward with torch.mm / matmul / F.linear raising.  The profiler
    does see such events when they happen (a .item() and a .cpu() of a device value as the control).  The profiled
    call moves t; the host reads it only afterwards."""
    from frhip import functional as FRF
    B, D, N = 16, 512, 300
    x, k, label, _ = CD.built(synth, "prof", B, D, N)
    head = make(D, N, k).cuda()
    xc, lc = x.cuda().requires_grad_(True), label.cuda()
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)
    seen = []

    def forward(x, lab):
        seen.append(head.t.clone())  # a device copy: the host reads it after the profiled pass
        return head(x, lab)

    HS.assert_forward_stays_on_device(monkeypatch, forward, xc, lc, head.kernel)
    ts = [float(t) for t in seen]  # before the first call, before the profiled one, after it
    assert len(ts) == 3 and ts[2] != ts[1], ts


def test_reproducible_labels_checked_and_empty_batch(monkeypatch):
    """Bitwise equal logits, both gradients and t run to run and with FRHIP_SINGLE_STREAM=1 (no side stream); an
    out-of-range label raises the reference's scatter_ error; an empty batch gives [0, N] logits, zero gradients and leaves
    t as it is."""
    B, D, N = 96, 512, 7001
    x, k, label, gout = CD.built(synth, "rep", B, D, N)
    head = make(D, N, k).cuda()
    xc = x.cuda()
    outs = []
    for single in ("0", "0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        with torch.no_grad():
            head.t.fill_(0.3)
        outs.append(run(head, xc, label, gout))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    assert float(outs[0][3]) != pytest.approx(0.3)
    bad = label.clone()
    bad[3] = N
    with pytest.raises(RuntimeError, match="out of bounds for dimension 1 with size %d" % N):
        head(xc, bad.cuda())
    bad[3] = -1
    with pytest.raises(RuntimeError, match="out of bounds"):
        head(xc, bad.cuda())
    t = head.t.clone()
    head.kernel.grad = None
    xe = torch.empty(0, D, device="cuda", requires_grad=True)
    y = head(xe, torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(y.shape) == (0, N)
    y.sum().backward()
    assert head.kernel.grad is not None and not bool(head.kernel.grad.any())
    assert torch.equal(head.t, t)


# ------------------------------------------------------------------------------------------------ train.py


def test_train_py_learns_and_resumes_bit_for_bit_with_curricularface(tmp_path):
    """HEAD_NAME = 'CurricularFace' on the synthetic config: 12 steps with finite loss that decreases (the mean of the
    last three steps below the mean of the first three), the Head_* file in the reference's layout with a t that has
    moved; and 12 steps straight == 6 steps, stop, resume for 6, bit for bit, t included (the Head_* file carries it)."""
    losses, sd, sa, _ = HS.straight_and_resumed(tmp_path, dict(HEAD_NAME="CurricularFace"), "CurricularFace")
    assert sum(losses[-3:]) < sum(losses[:3]), losses
    assert list(sd) == ["kernel", "t"] and tuple(sd["kernel"].shape) == (512, 12) and tuple(sd["t"].shape) == (1,)
    assert bool(torch.isfinite(sd["kernel"]).all()) and float(sd["t"]) != 0.0
    assert float(sa["t"]) != float(sd["t"])  # t went on moving after the resume
