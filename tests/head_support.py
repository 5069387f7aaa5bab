"""Scaffolding shared by the margin-head GPU tests (test_gpu_curricular / _magface / _adacos / _npcface / _mv_softmax /
_circle / _margin_heads_ext / _sharded_heads_ext and the train.py tests of test_gpu_model.py).

What belongs here is what is identical from head to head: the guarded buffers around a C entry point, the profiler and
``boom`` harness of the "no host read, no ATen GEMM" tests, one forward + backward of a head with a single parameter, the
train.py child process and the straight / stop / resume / compare skeleton of the resume tests.  What does not: a head's
reference arithmetic (tests/*_data.py and the *_host.py tests) and every tolerance -- a bar is stated by the test that
asserts it.  A head whose ``run`` returns more than (logits, gx, gweight) keeps its own; nothing here takes a flag for it.

This is a plain module, not a test module: pytest does not rewrite its ``assert`` statements, so every one of them carries
the values a reader needs in its message."""
import copy
import os
import re
import subprocess
import sys
import types

import numpy as np
import torch
import torch.nn.functional as F

PRODUCT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stylegan-for-facerec_amd")

# ------------------------------------------------------------------------------------------------ C ABI, guarded

SENTINEL = -12345.0
BAND = 4096  # floats on either side of a buffer (a multiple of 4: the interior keeps its 16-byte alignment)


class Guarded(object):
    """A sentinel-filled buffer of ``shape`` between two sentinel-filled guard bands."""

    def __init__(self, *shape, device="cuda"):
        n = int(np.prod(shape))
        self.flat = torch.full((2 * BAND + n,), SENTINEL, device=device)
        self.t = self.flat[BAND:BAND + n].view(*shape)

    def assert_guards(self, what):
        front, back = self.flat[:BAND] != SENTINEL, self.flat[-BAND:] != SENTINEL
        assert not bool(front.any()) and not bool(back.any()), (
            what, "guard band written: floats before / after the buffer", int(front.sum()), int(back.sum()))


# ------------------------------------------------------------------------------------------------ figures


def maxrel(got, ref):
    return float((got.double() - ref.double()).abs().max() / ref.double().abs().max())


def relerr(got, ref):
    return float((got.double() - ref.double()).norm() / ref.double().norm())


# ------------------------------------------------------------------------------------------------ one step of a head


def run(head, x, label, gout):
    """(logits, gx, gparameter) of one forward + backward of a head with exactly one parameter, on whatever device x is
    on."""
    (p,) = head.parameters()
    x = x.clone().requires_grad_(True)
    p.grad = None
    y = head(x, label.to(x.device))
    y.backward(gout.to(device=x.device, dtype=y.dtype))
    return y.detach().cpu(), x.grad.cpu(), p.grad.cpu()


def float64_reference(head, x, label, gout):
    """``run`` of the head's host path in float64, on a copy of the module."""
    h = copy.deepcopy(head).cpu().double()
    return run(h, x.double().cpu(), label.cpu(), gout.double().cpu())


# ------------------------------------------------------------------------------------------------ the pipeline

HOST_READS = ("aten::item", "aten::_local_scalar_dense")
ATEN_GEMMS = ("aten::mm", "aten::addmm", "aten::matmul", "aten::bmm", "aten::linear")


def profiled_names(fn):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return [e.name for e in prof.events()]


def forbid_aten_gemm(monkeypatch):
    """torch.mm / matmul / F.linear / Tensor.mm / Tensor.__matmul__ raise from here to the end of the test."""

    def boom(*a, **kw):
        raise AssertionError("ATen GEMM called on the HIP path")

    for mod, name in ((torch, "mm"), (torch, "matmul"), (F, "linear"), (torch.Tensor, "mm"), (torch.Tensor, "__matmul__")):
        monkeypatch.setattr(mod, name, boom)


def assert_forward_stays_on_device(monkeypatch, head, xc, lc, param):
    """The common body of the "no host read, no ATen GEMM" tests, for a ``head`` (a module, or a callable around one) that
    returns the logits alone: a first call (streams, allocator); the control -- the profiler does see a ``.item()``, a
    ``.cpu()`` and a ``torch.mm`` of device values; the profiled forward pass, which shows no scalar read, no
    device-to-host copy, no ATen GEMM and no Tensile kernel; forward + backward with the ATen GEMMs raising; finite
    gradients in ``xc`` and ``param``.  Returns the event names of the profiled forward pass."""
    head(xc, lc)  # first call: streams, allocator
    torch.cuda.synchronize()
    one = torch.ones(1, device=xc.device)
    control = profiled_names(lambda: (one.item(), one.cpu(), torch.mm(xc.detach(), xc.detach().t())))
    assert any(n in HOST_READS for n in control) and any("DtoH" in n for n in control), ("control", sorted(set(control)))
    assert "aten::mm" in control, ("control", sorted(set(control)))
    names = profiled_names(lambda: head(xc, lc))
    bad = [n for n in names if n in HOST_READS or n in ATEN_GEMMS or "DtoH" in n or n.startswith("Cijk_")]
    assert not bad, ("forward pass", sorted(set(bad)))
    forbid_aten_gemm(monkeypatch)
    y = head(xc, lc)
    y.backward(torch.ones_like(y))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(xc.grad).all()) and bool(torch.isfinite(param.grad).all()), (
        "non-finite gradient entries in x / the parameter",
        int((~torch.isfinite(xc.grad)).sum()), int((~torch.isfinite(param.grad)).sum()))
    return names


# ------------------------------------------------------------------------------------------------ train.py


def child(cmd, cwd, env, limit):
    """A child process under its own ``timeout`` and a subprocess limit just above it."""
    return subprocess.run(["timeout", "-k", "10", str(limit)] + cmd, cwd=cwd, env=env, capture_output=True, text=True,
                          timeout=limit + 30)


def run_train(tmp, tag, extra_cfg, max_steps=0, epochs=2, ok=True, limit=900):
    """train.py on the synthetic config (12 identities x 10 images, batches of 20: 6 steps an epoch) with ``extra_cfg``
    laid over it, writing to tmp / tag: (model directory, stdout).  ``ok=False`` returns the finished process instead,
    whatever its exit status."""
    env = dict(os.environ, PYTHONPATH=PRODUCT)
    argv = ["train.py", "--config", "configs/config_synthetic_smoke.py", "--synthetic", "12x10"]
    if max_steps:
        argv += ["--max-steps", str(max_steps)]
    model_dir = tmp / tag
    cfg_patch = ("import configs.config_synthetic_smoke as c; c.configurations[1].update(BATCH_SIZE=20, NUM_EPOCH=%d, "
                 "MODEL_ROOT=r'%s', LOG_ROOT=r'%s', **%r)" % (epochs, model_dir, tmp / "log", extra_cfg))
    code = "import sys, runpy; sys.argv=%r; %s; runpy.run_path('train.py', run_name='__main__')" % (argv, cfg_patch)
    out = child([sys.executable, "-c", code], PRODUCT, env, limit)
    if not ok:
        return out
    assert out.returncode == 0, "train.py run %r exited %d\n%s" % (
        tag, out.returncode, out.stdout[-2000:] + out.stderr[-2000:])
    return model_dir, out.stdout


def ckpt(model_dir, prefix):
    """The one file of ``model_dir`` whose name starts with ``prefix``."""
    hits = sorted(f for f in os.listdir(model_dir) if f.startswith(prefix))
    assert len(hits) == 1, (prefix, os.listdir(model_dir))
    return os.path.join(model_dir, hits[0])


def resume_cfg(cfg, model_dir, head_name, batch=6):
    """``cfg`` with the four *_RESUME_ROOT keys pointing at the epoch-1 files ``model_dir`` holds for ``batch``."""
    tag = "Epoch_1_Batch_%d_" % batch
    return dict(cfg, BACKBONE_RESUME_ROOT=ckpt(model_dir, "Backbone_IR_50_ReStyle_" + tag),
                HEAD_RESUME_ROOT=ckpt(model_dir, "Head_%s_%s" % (head_name, tag)),
                OPTIMIZER_RESUME_ROOT=ckpt(model_dir, "Optimizer_%s_%s" % (head_name, tag)),
                STATE_RESUME_ROOT=ckpt(model_dir, "State_%s_%s" % (head_name, tag)))


def assert_same_state(sa, sb, what):
    """Two state dicts with the same keys in the same order and every tensor equal bit for bit."""
    assert list(sa.keys()) == list(sb.keys()), (what, list(sa.keys()), list(sb.keys()))
    for key in sa:
        assert torch.equal(sa[key], sb[key]), (what, key, float((sa[key].double() - sb[key].double()).abs().max()))


def assert_same_checkpoints(a_dir, b_dir, head_name, last):
    """The Backbone_* and Head_* files of the two runs at ``last`` ("Epoch_E_Batch_B_") equal key by key and bit for bit,
    and every momentum buffer of the Optimizer_* files.  Returns (a's Head_* state dict, the two Optimizer_* dicts)."""
    for prefix in ("Backbone_IR_50_ReStyle_" + last, "Head_%s_%s" % (head_name, last)):
        sa = torch.load(ckpt(a_dir, prefix), map_location="cpu")
        sb = torch.load(ckpt(b_dir, prefix), map_location="cpu")
        assert_same_state(sa, sb, prefix)
    oa = torch.load(ckpt(a_dir, "Optimizer_%s_%s" % (head_name, last)), map_location="cpu")
    ob = torch.load(ckpt(b_dir, "Optimizer_%s_%s" % (head_name, last)), map_location="cpu")
    for key in oa["state"]:
        ma, mb = oa["state"][key]["momentum_buffer"], ob["state"][key]["momentum_buffer"]
        assert torch.equal(ma, mb), ("momentum_buffer", key, float((ma.double() - mb.double()).abs().max()))
    return sa, oa, ob


def resumed(tmp_path, cfg, head_name, epochs=2):
    """``epochs`` epochs straight ("straight"), 6 steps and stop ("first"), resume from those files to the end ("second"),
    and the end states of "straight" and "second" compared with ``assert_same_checkpoints``.  Returns a namespace: ``a_log``
    (the straight run's), ``sd_mid`` / ``sd_final`` (the Head_* state dict after 6 steps and at the end), ``a_dir`` /
    ``b1_dir`` / ``b2_dir`` (the three model directories), ``oa`` / ``ob`` (the two final Optimizer_* dicts)."""
    a_dir, a_log = run_train(tmp_path, "straight", cfg, epochs=epochs)
    b1_dir, _ = run_train(tmp_path, "first", cfg, max_steps=6, epochs=epochs)
    sd_mid = torch.load(ckpt(b1_dir, "Head_%s_Epoch_1_Batch_6_" % head_name), map_location="cpu")
    b2_dir, log = run_train(tmp_path, "second", resume_cfg(cfg, b1_dir, head_name), epochs=epochs)
    assert "Resuming at epoch 1 batch 6" in log and "Loading Optimizer Checkpoint" in log, log[-2000:]
    sd_final, oa, ob = assert_same_checkpoints(a_dir, b2_dir, head_name, "Epoch_%d_Batch_%d_" % (epochs, 6 * epochs))
    return types.SimpleNamespace(a_log=a_log, sd_mid=sd_mid, sd_final=sd_final, a_dir=a_dir, b1_dir=b1_dir, b2_dir=b2_dir,
                                 oa=oa, ob=ob)


def straight_and_resumed(tmp_path, cfg, head_name, epochs=2):
    """The skeleton of the "resumes bit for bit" tests of the replicated heads: ``resumed``, and of the straight run 6
    finite losses an epoch, a reported Prec@1 and no ``nan`` in the log.  Returns (the losses per step, the mid-run Head_*
    state dict, the final one, the three model directories)."""
    r = resumed(tmp_path, cfg, head_name, epochs)
    losses = [float(m.group(1)) for m in re.finditer(r"Training Loss ([0-9.eE+-]+|nan|inf) \(", r.a_log)]
    print("losses per step:", cfg, losses)
    assert len(losses) == 6 * epochs and all(np.isfinite(losses)), "%s\n%s" % (losses, r.a_log[-2000:])
    assert "Prec@1" in r.a_log and "nan" not in r.a_log.lower(), r.a_log[-2000:]
    return losses, r.sd_mid, r.sd_final, (r.a_dir, r.b1_dir, r.b2_dir)
