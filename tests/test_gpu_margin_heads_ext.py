"""SphereFace / Am_softmax on the HIP path (reference head/metrics.py:200-333): the reference's own vectors (g14), BASELINE
head sizes against a float64 host restatement, Am_softmax's clamp mask, no ATen GEMM, reproducibility, label errors, the
empty batch, and train.py end to end including a bit-for-bit resume through SphereFace's lambda schedule.

The float64 restatement is the head's own host path (plain PyTorch, pinned to g14 by test_margin_heads_ext_host.py) run on
a float64 copy of the module."""
import copy
import os
import re

import numpy as np
import pytest
import torch

import head_support as HS
from frhip import synth
from head_support import float64_reference, maxrel, relerr, run

pytestmark = pytest.mark.gpu

CASES = ("sphere_m4_it1", "sphere_m4_it10000", "sphere_m2_it10000", "am_unit", "am_small")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def inputs_of(g, tag, B=8, D=512, N=100):
    """(x, weight, label, gout) of a g14 case, regenerated from synth (make_golden_heads.inputs_of)."""
    x = synth.normal(14, tag + ".x", (B, D), std=float(g[tag + ".x_std"]))
    if tag.startswith("sphere"):
        w = synth.uniform(14, tag + ".w", (N, D), -0.1, 0.1)
    else:
        w = synth.uniform(14, tag + ".k", (D, N), -1.0, 1.0)
    label = synth.labels(14, tag + ".y", B, N)
    assert torch.equal(label, torch.from_numpy(g[tag + ".label"]))
    return x, w, label, synth.normal(14, tag + ".g", (B, N))


def param_of(head):
    return head.weight if hasattr(head, "weight") else head.kernel


def make(kind, D, N, w, it=10000, **kw):
    from head.metrics import Am_softmax, SphereFace
    head = SphereFace(D, N, None, **kw) if kind == "sphere" else Am_softmax(D, N, None, **kw)
    if kind == "sphere":
        head.iter = it - 1
    with torch.no_grad():
        param_of(head).copy_(w)
    return head


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(os.path.join(golden_dir, "g14_sphere_am.npz"))


@pytest.mark.parametrize("tag", CASES)
def test_device_heads_match_the_reference(g14, tag):
    """g14: logits within the 1e-3 bar, gradients within max(5e-3, 8 x the reference's own fp32-vs-float64 deviation) of
    max|ref| per tensor."""
    kind = "sphere" if tag.startswith("sphere") else "am"
    kw = dict(m=int(g14[tag + ".m"])) if kind == "sphere" else dict(m=float(g14[tag + ".m"]), s=float(g14[tag + ".s"]))
    x, w, label, gout = inputs_of(g14, tag)
    head = make(kind, 512, 100, w, it=int(g14.get(tag + ".iter", 1)), **kw).cuda()
    y, gx, gw = run(head, x.cuda(), label, gout)
    assert param_of(head).is_cuda and param_of(head).grad.is_cuda
    if kind == "sphere":
        assert head.iter == int(g14[tag + ".iter"]) and head.lamb == float(g14[tag + ".lamb"])
    ref = {k: torch.from_numpy(g14[tag + "." + k]) for k in ("logits", "gx", "gw")}
    assert float((y - ref["logits"]).abs().max()) < 1e-3
    # the file keeps gw at every label class and every 20th class (rows of [N, D] / columns of [D, N]) and its whole norm
    gw_kept = gw.index_select(0 if kind == "sphere" else 1, torch.from_numpy(g14[tag + ".gw_index"]))
    for name, got in (("gx", gx), ("gw", gw_kept)):
        bar = max(5e-3, 8 * float(g14[tag + ".dev." + name]))
        assert got.shape == ref[name].shape
        assert maxrel(got, ref[name]) < bar, (tag, name, maxrel(got, ref[name]), bar)
    assert abs(float(gw.double().norm()) / float(g14[tag + ".gw_norm"]) - 1) < max(5e-3, 8 * float(g14[tag + ".dev.gw"]))


@pytest.mark.parametrize("N", [7000, 7001, 28000])
@pytest.mark.parametrize("kind", ["sphere", "am"])
def test_baseline_head_sizes_against_float64(kind, N):
    """B = 256 at the BASELINE class counts (7001: neither a multiple of 4 nor of 32), against float64.  Gradient bar:
    max(1e-3, 8 x the host fp32 run's own deviation from float64).  With Am_softmax's unit-variance embeddings ~30 % of the
    cosines saturate, and the few within fp32 rounding of +-1 take the clamp mask either way in ANY fp32 run (~1e-3 of the
    gradient norm at N = 7000)."""
    B, D = 256, 512
    tag = "%s%d" % (kind, N)
    x = synth.normal(41, tag + ".x", (B, D))
    w = synth.uniform(41, tag + ".w", (N, D), -0.1, 0.1) if kind == "sphere" else \
        synth.uniform(41, tag + ".k", (D, N), -1.0, 1.0)
    label = synth.labels(41, tag + ".y", B, N)
    gout = synth.normal(41, tag + ".g", (B, N), std=1e-3)
    head = make(kind, D, N, w)
    ry, rgx, rgw = float64_reference(head, x, label, gout)
    _, hgx, hgw = run(copy.deepcopy(head), x, label, gout)  # host fp32
    y, gx, gw = run(head.cuda(), x.cuda(), label, gout)
    assert float((y - ry).abs().max()) < 1e-3
    for got, host, ref in ((gx, hgx, rgx), (gw, hgw, rgw)):
        assert relerr(got, ref) < max(1e-3, 8 * relerr(host, ref)), (relerr(got, ref), relerr(host, ref))


def test_am_softmax_clamp_mask_is_exercised():
    """Unit-variance embeddings saturate >= 10 % of the cosines; the gradients match the restatement, and differ from
    what an unmasked backward pass would give."""
    B, D, N = 64, 512, 1000
    x = synth.normal(42, "sat.x", (B, D))
    k = synth.uniform(42, "sat.k", (D, N), -1.0, 1.0)
    label = synth.labels(42, "sat.y", B, N)
    gout = synth.normal(42, "sat.g", (B, N))
    kn = k.double() / k.double().norm(2, 0, True)
    cos = x.double() @ kn
    assert float((cos.abs() > 1).double().mean()) >= 0.10
    head = make("am", D, N, k)
    _, rgx, rgk = float64_reference(head, x, label, gout)
    y, gx, gk = run(head.cuda(), x.cuda(), label, gout)
    assert relerr(gx, rgx) < 1e-3 and relerr(gk, rgk) < 1e-3
    # without the mask: gx = s g K^T (normalised), far from the reference
    assert relerr(30.0 * gout.double() @ kn.t(), rgx) > 0.1
    # saturated logits are exactly +-s (after the label margin)
    sat = cos.abs() > 1 + 1e-4
    hot = torch.zeros(B, N, dtype=torch.bool).scatter_(1, label.view(-1, 1), True)
    want = torch.sign(cos) * 30.0 - hot * 0.35 * 30.0
    assert torch.allclose(y.double()[sat], want[sat], atol=1e-4)


def test_no_aten_gemm_on_the_device_path(monkeypatch):
    """Forward + backward of both heads on device with torch.mm / matmul / F.linear / Tensor.mm / Tensor.__matmul__
    raising: the cosine GEMMs are the project's own kernels."""
    B, D, N = 16, 512, 300
    heads = [make("sphere", D, N, synth.uniform(43, "mm.w", (N, D), -0.1, 0.1)).cuda(),
             make("am", D, N, synth.uniform(43, "mm.k", (D, N))).cuda()]
    x = synth.normal(43, "mm.x", (B, D)).cuda()
    label = synth.labels(43, "mm.y", B, N).cuda()
    HS.forbid_aten_gemm(monkeypatch)
    for head in heads:
        xx = x.clone().requires_grad_(True)
        y = head(xx, label)
        y.backward(torch.ones_like(y))
        torch.cuda.synchronize()
        assert torch.isfinite(xx.grad).all() and torch.isfinite(param_of(head).grad).all()


@pytest.mark.parametrize("kind", ["sphere", "am"])
def test_reproducible_labels_checked_and_empty_batch(kind, monkeypatch):
    """Bitwise equal logits and gradients run to run and with FRHIP_SINGLE_STREAM=1 (no side stream); an out-of-range
    label raises the reference's scatter_ error; an empty batch gives [0, N] logits and zero gradients."""
    B, D, N = 96, 512, 7001
    w = synth.uniform(44, "rep.w", (N, D), -0.1, 0.1) if kind == "sphere" else synth.uniform(44, "rep.k", (D, N))
    x = synth.normal(44, "rep.x", (B, D)).cuda()
    label = synth.labels(44, "rep.y", B, N)
    gout = synth.normal(44, "rep.g", (B, N))
    head = make(kind, D, N, w).cuda()
    outs = []
    for single in ("0", "0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        if kind == "sphere":
            head.iter = 9999
        outs.append(run(head, x, label, gout))
    for o in outs[1:]:
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b)
    bad = label.clone()
    bad[3] = N
    with pytest.raises(RuntimeError, match="out of bounds for dimension 1 with size %d" % N):
        head(x, bad.cuda())
    it = getattr(head, "iter", None)
    param_of(head).grad = None
    xe = torch.empty(0, D, device="cuda", requires_grad=True)
    y = head(xe, torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(y.shape) == (0, N)
    y.sum().backward()
    assert param_of(head).grad is not None and not bool(param_of(head).grad.any())
    if it is not None:
        assert head.iter == it + 1  # every forward call counts, as in the reference


# ------------------------------------------------------------------------------------------------ train.py


@pytest.mark.parametrize("name,key,shape", [("SphereFace", "weight", (12, 512)), ("Am_softmax", "kernel", (512, 12))])
def test_train_py_runs_with_the_head(tmp_path, name, key, shape):
    """HEAD_NAME = SphereFace / Am_softmax on the synthetic config: finite loss, precision reported, checkpoint in the
    reference's layout."""
    d, out = HS.run_train(tmp_path, name, dict(HEAD_NAME=name), max_steps=3)
    losses = [float(m.group(1)) for m in re.finditer(r"Training Loss ([0-9.eE+-]+|nan|inf) \(", out)]
    assert losses and all(np.isfinite(losses)), out[-2000:]
    assert "Prec@1" in out and "nan" not in out.lower()
    sd = torch.load(HS.ckpt(d, "Head_%s_Epoch_1_Batch_3_" % name), map_location="cpu")
    assert list(sd) == [key] and tuple(sd[key].shape) == shape and bool(torch.isfinite(sd[key]).all())


def test_resume_continues_bit_for_bit_with_sphereface(tmp_path):
    """test_gpu_model.py::test_resume_continues_bit_for_bit with HEAD_NAME = 'SphereFace': 12 steps straight == 6 steps,
    stop, resume for 6.  SphereFace's lambda follows its forward counter, which the State_* file carries (head_iter)."""
    r = HS.resumed(tmp_path, dict(HEAD_NAME="SphereFace"), "SphereFace")
    assert "Training Loss" in r.a_log and "nan" not in r.a_log.lower()
    assert torch.load(HS.ckpt(r.b1_dir, "State_SphereFace_Epoch_1_Batch_6_"))["head_iter"] == 6
    sa = torch.load(HS.ckpt(r.a_dir, "State_SphereFace_Epoch_2_Batch_12_"))
    sb = torch.load(HS.ckpt(r.b2_dir, "State_SphereFace_Epoch_2_Batch_12_"))
    assert sa["head_iter"] == sb["head_iter"] == 12
