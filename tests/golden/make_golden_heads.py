#!/usr/bin/env python3
"""Generate tests/golden/g14_sphere_am.npz: the reference's SphereFace and Am_softmax heads (head/metrics.py:200-333) on CPU.

Runs only in the build container, like make_golden.py (whose import-only stand-ins and reference imports it reuses).
Inputs come from the repo's counter-based generator (stylegan-for-facerec_amd/frhip/synth.py): B = 8, D = 512, N = 100.
The file holds no inputs: ``inputs_of`` regenerates them from synth (the tests do the same), the file keeps the labels and
the scalars (m, iter, lambda, the embeddings' std) as a check.  Per case it holds the reference's fp32 logits and gx in full,
and the weight gradient gw at the classes ``gw_index`` (every label plus every 20th class: rows of SphereFace's [N, D]
``weight`` gradient, columns of Am_softmax's [D, N] ``kernel`` gradient) together with the float64 norm of the whole of it
(``gw_norm``); and per tensor the reference's own fp32-vs-float64 deviation ``dev.*`` = max|t32 - t64| / max|t64| over the
whole tensor (the float64 run is the same module in double precision).

    python tests/golden/make_golden_heads.py        # writes next to this file

Cases:
  sphere_m4_it1      SphereFace m = 4, first forward (iter 1, lambda ~ 893)
  sphere_m4_it10000  SphereFace m = 4 at iter 10000 (lambda = LambdaMin = 5: the margin is visible)
  sphere_m2_it10000  SphereFace m = 2 at iter 10000
  am_unit            Am_softmax, unit-variance embeddings (||x|| ~ 22: many cosines clamp at +-1)
  am_small           Am_softmax, embeddings of norm ~ 0.45 (no cosine clamps)
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py

B, D, N = 8, 512, 100
SEED = 14


def _run(head, x, label, gout, param):
    x = x.clone().requires_grad_(True)
    y = head(x, label)
    gx, gw = torch.autograd.grad(y, [x, param], gout.to(y.dtype))
    return y, gx, gw


def inputs_of(synth, tag, x_std=1.0):
    """(x [B, D], weight, label [B], gout [B, N]) of a case; the weight is SphereFace's ``weight`` [N, D] or
    Am_softmax's ``kernel`` [D, N]."""
    x = synth.normal(SEED, tag + ".x", (B, D), std=x_std)
    if tag.startswith("sphere"):
        w = synth.uniform(SEED, tag + ".w", (N, D), -0.1, 0.1)
    else:
        w = synth.uniform(SEED, tag + ".k", (D, N), -1.0, 1.0)
    return x, w, synth.labels(SEED, tag + ".y", B, N), synth.normal(SEED, tag + ".g", (B, N))


def sphere_case(out, tag, m, it):
    x, w, label, gout = inputs_of(MG.synth, tag)
    res = {}
    for dt in (torch.float32, torch.float64):
        head = MG.ref_heads.SphereFace(D, N, None, m=m)
        with torch.no_grad():
            head.weight.data = w.clone().to(dt)
        head.iter = it - 1  # the forward call increments it to `it`
        res[dt] = _run(head, x.to(dt), label, gout, head.weight)
        assert head.iter == it
    out[tag + ".lamb"] = np.array(head.lamb)
    _store(out, tag, label, res, 0, m=m, iter=it, x_std=1.0)


def am_case(out, tag, std):
    x, k, label, gout = inputs_of(MG.synth, tag, std)
    res = {}
    for dt in (torch.float32, torch.float64):
        head = MG.ref_heads.Am_softmax(D, N, None)
        with torch.no_grad():
            head.kernel.data = k.clone().to(dt)
        res[dt] = _run(head, x.to(dt), label, gout, head.kernel)
    kn = k / k.norm(2, 0, True)
    out[tag + ".saturated"] = np.array(float(((x @ kn).abs() > 1).float().mean()))
    _store(out, tag, label, res, 1, m=0.35, s=30.0, x_std=std)


def _store(out, tag, label, res, class_dim, **scalars):
    out[tag + ".label"] = MG.npy(label)
    for k, v in scalars.items():
        out["%s.%s" % (tag, k)] = np.array(v)
    y32, gx32, gw32 = res[torch.float32]
    y64, gx64, gw64 = res[torch.float64]
    idx = torch.tensor(sorted(set(label.tolist()) | set(range(0, N, 20))))
    out[tag + ".logits"] = MG.npy(y32)
    out[tag + ".gx"] = MG.npy(gx32)
    out[tag + ".gw_index"] = MG.npy(idx)
    out[tag + ".gw"] = MG.npy(gw32.index_select(class_dim, idx))
    out[tag + ".gw_norm"] = np.array(float(gw32.detach().double().norm()))
    for name, a, b in (("logits", y32, y64), ("gx", gx32, gx64), ("gw", gw32, gw64)):
        a, b = a.detach().double(), b.detach()
        out["%s.dev.%s" % (tag, name)] = np.array(float((a - b).abs().max() / b.abs().max()))


def g14_sphere_am():
    out = {}
    sphere_case(out, "sphere_m4_it1", 4, 1)
    sphere_case(out, "sphere_m4_it10000", 4, 10000)
    sphere_case(out, "sphere_m2_it10000", 2, 10000)
    am_case(out, "am_unit", 1.0)
    am_case(out, "am_small", 0.02)
    for k in sorted(out):
        if ".dev." in k or k.endswith((".saturated", ".lamb")):
            print("%-32s %.3e" % (k, float(out[k])))
    MG.save("g14_sphere_am", **out)


if __name__ == "__main__":
    g14_sphere_am()
