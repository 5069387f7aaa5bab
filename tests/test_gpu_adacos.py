"""AdaCos on the HIP path (reference head/metrics.py:336-369): the reference's own vectors (g20) including the three-call
trajectory of the scale, larger sizes against a float64 host restatement on both sides of min(pi/4, theta_med), the scale
kept on the device (no device-to-host copy and no ATen GEMM in the forward pass, bit-reproducible), one-sided gradients,
label errors, the empty batch, the three C entry points in sentinel-filled buffers, and train.py end to end including a
bit-for-bit resume.

The float64 restatement is the head's own host path (plain PyTorch, pinned to g20 by test_adacos_host.py) run on a float64
copy of the module.  The batches are those of tests/adacos_data.py.

Bars: logits within 1e-3 absolute (the project's fp32 logits bar); gradients by norm within max(1e-3, 8 x the host fp32
run's own deviation from float64); the scale within max(1e-6, 8 x the host fp32 deviation) RELATIVE to the float64 value
(1e-6 is about 8 ulp of fp32; the factor 8 is the convention of test_gpu_curricular.py)."""
import copy
import math
import os

import numpy as np
import pytest
import torch

import adacos_data as AD
import head_support as HS
from frhip import synth
from head_support import SENTINEL, Guarded, relerr

pytestmark = pytest.mark.gpu

D = 512


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_adacos.npz"))


def make(N, W):
    from head.metrics import AdaCos
    head = AdaCos(D, N)
    with torch.no_grad():
        head.W.copy_(W)
    return head


def run(head, x, label, gout):
    """(logits, gx, gW, scale after the call) of one forward + backward, on whatever device x is on."""
    x = x.clone().requires_grad_(True)
    head.W.grad = None
    y = head(x, label.to(x.device))
    y.backward(gout.to(device=x.device, dtype=y.dtype))
    return y.detach().cpu(), x.grad.cpu(), head.W.grad.cpu(), head.scale.detach().cpu().clone()


def srel(got, ref):
    return abs(float(got) / float(ref) - 1)


def check_against(dev, host, ref, what):
    """The three bars of the module docstring: (logits, gx, gW, scale) of the device run, of the host fp32 run and of the
    float64 run."""
    figures = dict(logits=float((dev[0] - ref[0]).abs().max()), gx=(relerr(dev[1], ref[1]), relerr(host[1], ref[1])),
                   gw=(relerr(dev[2], ref[2]), relerr(host[2], ref[2])), scale=(srel(dev[3], ref[3]), srel(host[3], ref[3])))
    print(what, figures)
    assert figures["logits"] < 1e-3, (what, figures)
    for k in ("gx", "gw"):
        assert figures[k][0] < max(1e-3, 8 * figures[k][1]), (what, k, figures)
    assert figures["scale"][0] < max(1e-6, 8 * figures["scale"][1]), (what, figures)


@pytest.mark.parametrize("tag", AD.CASES)
def test_device_head_matches_the_reference(g20, tag):
    """g20, every case: per call the logits against the reference's, the scale after the call against the reference's
    float64 run, the gradients against the float64 host run.  The trajectory's last call runs in eval mode under no_grad,
    and the scale still moves."""
    calls = AD.batches(synth, tag, D, 100)
    W = calls[0][1][1]
    dev, h32, h64 = make(100, W).cuda(), make(100, W), make(100, W).double()
    for i, (name, (x, _, label, gout), branch, mid_gap) in enumerate(calls):
        assert torch.equal(label, torch.from_numpy(g20[name + ".label"]))
        AD.assert_covers(x, W, label, float(h64.scale), branch, mid_gap)
        before = dev.scale.clone()
        if tag == "traj" and i == 2:
            dev.eval(), h32.eval(), h64.eval()
            with torch.no_grad():
                y = dev(x.cuda(), label.cuda()).cpu()
                h32(x, label), h64(x.double(), label)
            assert float((y - torch.from_numpy(g20[name + ".logits"])).abs().max()) < 1e-3
        else:
            got = run(dev, x.cuda(), label, gout)
            check_against(got, run(h32, x, label, gout), run(h64, x.double(), label, gout.double()), name)
            assert float((got[0] - torch.from_numpy(g20[name + ".logits"])).abs().max()) < 1e-3
        assert dev.scale.is_cuda and tuple(dev.scale.shape) == (1,) and not torch.equal(before, dev.scale)
        s64 = float(g20[name + ".scale64"])
        bar = max(1e-6, 8 * srel(h32.scale, s64))
        assert srel(dev.scale, s64) < bar, (name, float(dev.scale), s64, bar)
    assert list(dev.state_dict()) == ["W"] and dev.W.is_cuda


@pytest.mark.parametrize("N,close,branch", [(1000, 48, "median"), (1001, 48, "median"), (7000, 48, "median"),
                                            (1001, 16, "pi4")])
def test_larger_sizes_against_float64(N, close, branch):
    """B = 64 at N = 1000, 1001 (a multiple of neither 4 nor 32) and 7000 with 3/4 of the rows built close to their class
    (the median branch), and once with 1/4 of them (the pi/4 branch), against float64."""
    B = 64
    x, W, label, gout = AD.built(synth, "big%d_%d" % (N, close), B, D, N, close)
    AD.assert_covers(x, W, label, AD.scale0(N), branch)
    head = make(N, W)
    ref = run(copy.deepcopy(head).double(), x.double(), label, gout.double())
    host = run(copy.deepcopy(head), x, label, gout)
    check_against(run(head.cuda(), x.cuda(), label, gout), host, ref, "N=%d close=%d" % (N, close))


def test_baseline_size_logits_and_scale_against_float64():
    """B = 256, N = 28000 (the largest BASELINE head), 3/4 of the rows close: logits within 1e-3 of float64, the scale
    within max(1e-6, 8 x the host fp32 deviation) relative."""
    B, N = 256, 28000
    x, W, label, _ = AD.built(synth, "big28000", B, D, N, 192)
    AD.assert_covers(x, W, label, AD.scale0(N), "median")
    head = make(N, W)
    ref, h32 = copy.deepcopy(head).double(), copy.deepcopy(head)
    with torch.no_grad():
        ry = ref(x.double(), label)
        h32(x, label)
        y = head.cuda()(x.cuda(), label.cuda()).cpu()
    figures = (float((y - ry).abs().max()), srel(head.scale, ref.scale), srel(h32.scale, ref.scale))
    print("B=256 N=28000", figures)
    assert tuple(y.shape) == (B, N) and figures[0] < 1e-3
    assert figures[1] < max(1e-6, 8 * figures[2]), figures


def test_one_sided_gradients_and_no_grad():
    """x without requires_grad leaves the weight gradient of the two-sided run, bit for bit; a frozen W leaves its feature
    gradient; under no_grad nothing requires a gradient.  Every call starts from the same scale."""
    B, N = 16, 300
    x, W, label, gout = AD.built(synth, "one", B, D, N, 12)
    head = make(N, W).cuda()
    s0 = head.scale.clone()
    y, gx, gw, s1 = run(head, x.cuda(), label, gout)
    head.scale.copy_(s0)
    head.W.grad = None
    head(x.cuda(), label.cuda()).backward(gout.cuda())
    assert torch.equal(head.W.grad.cpu(), gw) and torch.equal(head.scale.cpu(), s1)
    head.scale.copy_(s0)
    head.W.requires_grad_(False)
    head.W.grad = None
    xc = x.cuda().requires_grad_(True)
    head(xc, label.cuda()).backward(gout.cuda())
    assert torch.equal(xc.grad.cpu(), gx) and head.W.grad is None
    head.W.requires_grad_(True)
    with torch.no_grad():
        assert not head(xc, label.cuda()).requires_grad


def test_reproducible_labels_checked_and_empty_batch(monkeypatch):
    """Bitwise equal logits, both gradients and scale for two identical calls from the same state, and with
    FRHIP_SINGLE_STREAM=1 (no side stream); with CHECK_LABELS on an out-of-range label raises the reference's scatter_
    error; an empty batch gives [0, N] logits, zero gradients and leaves the scale as it is."""
    from frhip import functional as FRF
    B, N = 64, 1001
    x, W, label, gout = AD.built(synth, "rep", B, D, N, 48)
    head = make(N, W).cuda()
    xc = x.cuda()
    outs = []
    for single in ("0", "0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        with torch.no_grad():
            head.scale.fill_(9.5)
        outs.append(run(head, xc, label, gout))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    assert float(outs[0][3]) != pytest.approx(9.5)
    assert FRF.CHECK_LABELS
    bad = label.clone()
    bad[3] = N
    with pytest.raises(RuntimeError, match="out of bounds for dimension 1 with size %d" % N):
        head(xc, bad.cuda())
    bad[3] = -1
    with pytest.raises(RuntimeError, match="out of bounds"):
        head(xc, bad.cuda())
    s = head.scale.clone()
    head.W.grad = None
    xe = torch.empty(0, D, device="cuda", requires_grad=True)
    y = head(xe, torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(y.shape) == (0, N)
    y.sum().backward()
    assert head.W.grad is not None and not bool(head.W.grad.any())
    assert torch.equal(head.scale, s)
    with pytest.raises(ValueError, match="scale must be"):
        FRF.adacos_head(xc, head.W, label.cuda(), torch.ones(1, device="cuda", dtype=torch.float64))


def test_forward_keeps_the_scale_on_the_device_and_calls_no_aten_gemm(monkeypatch):
    """torch.profiler over the forward pass (labels validated by the caller, as in train.py): no device-to-host copy, no
    scalar read, no ATen GEMM; the same over forward + backward with torch.mm / matmul / F.linear raising.  The profiler
    does see such events when they happen (a .item() and a .cpu() of a device value as the control).  The profiled
    call moves the scale; the host reads it only afterwards."""
    from frhip import functional as FRF
    B, N = 16, 300
    x, W, label, _ = AD.built(synth, "prof", B, D, N, 12)
    head = make(N, W).cuda()
    xc, lc = x.cuda().requires_grad_(True), label.cuda()
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)
    seen = []

    def forward(x, lab):
        seen.append(head.scale.clone())  # a device copy: the host reads it after the profiled pass
        return head(x, lab)

    HS.assert_forward_stays_on_device(monkeypatch, forward, xc, lc, head.W)
    scales = [float(v) for v in seen]  # before the first call, before the profiled one, after it
    assert len(scales) == 3 and scales[2] != scales[1], scales


# ------------------------------------------------------------------------------------------------ C ABI, guarded


@pytest.mark.parametrize("N", [33, 1000, 1001])
def test_rows_kernel_in_sentinel_filled_buffers(N):
    """fr_adacos_rows at rows = 1, 4, 5 with labels on column 0, column N - 1, -1 and N, raw cosines in [-1.1, 1.1] (no
    clamp enters the sum) and sentinels in the padding columns of cos: rowv[0] within 1e-6 relative of the float64 sum
    (|scale * cos| <= 8: the fp32 product's rounding is 4.8e-7 relative inside exp, expf 1.2e-7, the final rounding
    6e-8), rowv[1] the raw target cosine bit for bit or exactly the marker 2.0, and nothing around rowv is written."""
    from frhip import ops
    st = ops.current_stream_ptr()
    ld = (N + 3) // 4 * 4
    scale = torch.tensor([7.25], device="cuda")
    for rows in (1, 4, 5):
        cos = torch.full((rows, ld), SENTINEL, device="cuda")
        cos[:, :N] = synth.uniform(AD.SEED, "rows.cos%d" % rows, (rows, N), -1.1, 1.1).cuda()
        label = torch.tensor([0, N - 1, -1, N, 17][:rows] if rows > 1 else [N - 1], device="cuda")
        rowv = Guarded(2, rows)
        ops.call("fr_adacos_rows", cos, label, scale, rowv.t, rows, N, ld, st)()
        torch.cuda.synchronize()
        rowv.assert_guards("rowv")
        assert float(scale) == float(torch.tensor(7.25))  # read only
        c = cos[:, :N].cpu()
        lab = label.cpu()
        has = (lab >= 0) & (lab < N)
        e = torch.exp(7.25 * c.double())
        e[has, lab[has]] = 0.0
        want = e.sum(1)
        got = rowv.t.cpu()
        assert float((got[0].double() / want - 1).abs().max()) < 1e-6, (rows, N, got[0], want)
        target = torch.where(has, c.gather(1, lab.clamp(0, N - 1).view(-1, 1)).view(-1), torch.tensor(2.0))
        assert torch.equal(got[1], target), (rows, N, got[1], target)


def scale_reference(rowv, old):
    """The float64 formula with torch.median over the rows that have a target."""
    r0, tc = rowv[0].double(), rowv[1]
    tc = tc[tc != 2.0].double()
    if tc.numel() == 0:
        return None
    th = torch.median(torch.acos(tc.clamp(-1 + 1e-7, 1 - 1e-7)))
    return float(torch.log(r0.sum() / r0.numel()) / torch.cos(torch.clamp(th, max=math.pi / 4)))


@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 255, 256, 257, 1000])
def test_scale_kernel_on_hand_made_rows(rows):
    """fr_adacos_scale on hand-made rowv: distinct target cosines on the median side and on the pi/4 side, ties (cosines
    from a grid of 7 values), marker rows mixed in, and all rows marked, where the scale stays bit for bit.  The kernel
    works in double from fp32 inputs and rounds once: within 2e-7 relative of the float64 formula."""
    from frhip import ops
    st = ops.current_stream_ptr()
    sums = synth.uniform(AD.SEED, "scale.sums%d" % rows, (rows,), 50.0, 150.0)
    variants = {
        "median": synth.uniform(AD.SEED, "scale.a%d" % rows, (rows,), 0.75, 0.99),
        "pi4": synth.uniform(AD.SEED, "scale.b%d" % rows, (rows,), -0.5, 0.5),
        "ties": 0.75 + 0.03 * torch.floor(synth.uniform(AD.SEED, "scale.c%d" % rows, (rows,), 0.0, 7.0)),
    }
    mixed = synth.uniform(AD.SEED, "scale.d%d" % rows, (rows,), 0.75, 0.99)
    mixed[::3] = 2.0
    variants["markers"] = mixed
    variants["all_marked"] = torch.full((rows,), 2.0)
    for name, tc in variants.items():
        rowv = torch.stack([sums, tc]).contiguous()
        scale = Guarded(1)
        scale.t.fill_(6.25)
        ops.call("fr_adacos_scale", rowv.cuda(), rows, scale.t, st)()
        torch.cuda.synchronize()
        scale.assert_guards(name)
        want = scale_reference(rowv, 6.25)
        if want is None:
            assert float(scale.t) == 6.25, (name, rows, float(scale.t))
        else:
            assert srel(scale.t, want) < 2e-7, (name, rows, float(scale.t), want)


@pytest.mark.parametrize("N", [1000, 1001])
def test_apply_kernel_forward_and_backward_use(N):
    """fr_adacos_apply as the forward pass uses it (src = raw cosines with pitch ld, sentinels in its padding columns, out
    with pitch ld) and as the backward pass does (src = g [rows][N] contiguous, out = gcos with pitch Np = 1024), rows = 6
    (a row block with two idle waves): exactly scale * src in fp32, padding columns exactly 0, guard bands intact."""
    from frhip import ops
    st = ops.current_stream_ptr()
    rows, ld, Np = 6, (N + 3) // 4 * 4, 1024
    scale = torch.tensor([5.28091], device="cuda")
    cos = torch.full((rows, ld), SENTINEL, device="cuda")
    cos[:, :N] = synth.uniform(AD.SEED, "apply.cos", (rows, N), -1.1, 1.1).cuda()
    g = synth.normal(AD.SEED, "apply.g", (rows, N)).cuda()
    out, gcos = Guarded(rows, ld), Guarded(rows, Np)
    ops.call("fr_adacos_apply", cos, scale, out.t, rows, N, ld, ld, st)()
    ops.call("fr_adacos_apply", g, scale, gcos.t, rows, N, N, Np, st)()
    torch.cuda.synchronize()
    for name, b, src in (("out", out, cos[:, :N]), ("gcos", gcos, g)):
        b.assert_guards(name)
        assert torch.equal(b.t[:, :N], scale * src), name
        assert not bool(b.t[:, N:].any()), name


# ------------------------------------------------------------------------------------------------ train.py


def test_train_py_runs_and_resumes_bit_for_bit_with_adacos(tmp_path):
    """HEAD_NAME = 'AdaCos' on the synthetic config: 12 steps with finite loss, the Head_* file with the key W alone and the
    State_* file with a ``head_scale`` that has moved; and 12 steps straight == 6 steps, stop, resume for 6, bit for bit,
    the scale included (the State_* file carries it).  SHARDED_HEAD=True raises before anything is built."""
    cfg = dict(HEAD_NAME="AdaCos")
    _, sd, _, (a_dir, b1_dir, b2_dir) = HS.straight_and_resumed(tmp_path, cfg, "AdaCos")
    assert list(sd) == ["W"] and tuple(sd["W"].shape) == (12, 512) and bool(torch.isfinite(sd["W"]).all())
    state1 = torch.load(HS.ckpt(b1_dir, "State_AdaCos_Epoch_1_Batch_6_"), map_location="cpu")
    s_mid = state1["head_scale"]
    assert isinstance(s_mid, float) and math.isfinite(s_mid) and abs(s_mid - AD.scale0(12)) > 1e-3
    ea = torch.load(HS.ckpt(a_dir, "State_AdaCos_Epoch_2_Batch_12_"), map_location="cpu")
    eb = torch.load(HS.ckpt(b2_dir, "State_AdaCos_Epoch_2_Batch_12_"), map_location="cpu")
    assert ea["head_scale"] == eb["head_scale"] and ea["head_scale"] != s_mid  # bit for bit, and it went on moving
    out = HS.run_train(tmp_path, "sharded", dict(cfg, SHARDED_HEAD=True), ok=False)
    assert out.returncode != 0 and "NotImplementedError" in out.stderr and "AdaCos" in out.stderr
    assert "Number of Training Classes" not in out.stdout and not os.path.exists(tmp_path / "sharded")
