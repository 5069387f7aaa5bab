#!/usr/bin/env python3
"""Generate tests/golden/g15_input_grad.npz: the reference's gradient with respect to the input images (backbone/model_irse.py,
backbone/restyle_psp.py) on CPU.

Runs only in the build container, like make_golden.py (whose import-only stand-ins, reference imports and synth weights,
``full_model``, it reuses).  Per case: B = 2 images x = synth.uniform(15, "g15.x"), the loss sum(features * gfeat) with
gfeat = synth.normal(15, "g15.g", [2, 512]); the file keeps the reference's fp32 ``gx`` and ``features``, the float64 norm
of its float64 gradient (``gx_norm64``) and its own fp32-vs-float64 deviation ``dev.gx`` = max|gx32 - gx64| / max|gx64|
(the float64 run is the same module in double precision).  The inputs are regenerated from synth by the tests.

    python tests/golden/make_golden_input_grad.py        # writes next to this file

Cases:
  ir50_train   IR-50, train mode (batch statistics in every BatchNorm)
  ir50_eval    IR-50, eval mode (running statistics: the identity-loss use of a frozen recognizer)
  psp_train    pSp IR-SE-50 with the average image concatenated to the stem input (6-channel stem), train mode
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as MG  # noqa: E402  -- stubs + the reference's backbone modules

B = 2
SEED = 15
CASES = {"ir50_train": ("ir50", True), "ir50_eval": ("ir50", False), "psp_train": ("psp", True)}


def inputs_of(synth):
    return synth.uniform(SEED, "g15.x", (B, 3, 112, 112)), synth.normal(SEED, "g15.g", (B, 512))


def run_case(out, tag):
    kind, train = CASES[tag]
    x, gfeat = inputs_of(MG.synth)
    res = {}
    for dt in (torch.float32, torch.float64):
        model, _prefix, avg = MG.full_model(kind)
        model = model.to(dt).train(train)
        if avg is not None:
            model.avg_image = avg.to(dt)
        xx = x.to(dt).requires_grad_(True)
        feats = model(xx)
        (gx,) = torch.autograd.grad((feats * gfeat.to(dt)).sum(), [xx])
        res[dt] = feats.detach(), gx
    f32, gx32 = res[torch.float32]
    _f64, gx64 = res[torch.float64]
    out[tag + ".features"] = MG.npy(f32)
    out[tag + ".gx"] = MG.npy(gx32)
    out[tag + ".gx_norm64"] = np.array(float(gx64.norm()))
    out[tag + ".dev.gx"] = np.array(float((gx32.double() - gx64).abs().max() / gx64.abs().max()))


def g15_input_grad():
    out = {}
    for tag in CASES:
        run_case(out, tag)
    for k in sorted(out):
        if ".dev." in k:
            print("%-24s %.3e" % (k, float(out[k])))
    MG.save("g15_input_grad", **out)


if __name__ == "__main__":
    g15_input_grad()
