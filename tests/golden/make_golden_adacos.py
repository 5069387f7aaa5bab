#!/usr/bin/env python3
"""Generate tests/golden/g20_adacos.npz: the reference's AdaCos head (head/metrics.py:336-369) on CPU.

Runs only in the build container, like make_golden_magface.py (whose import-only stand-ins and reference imports it reuses
through make_golden.py).  Inputs come from the repo's counter-based generator through tests/adacos_data.py, which the tests
import too: D = 512, N = 100.  The file holds no inputs, only the labels and the upstream gradient as a check.  Per call it
holds the reference's fp32 logits and gx in full, the weight gradient gW at the rows ``gw_index`` (every label plus every
20th class) with the float64 norm of the whole of it (``gw_norm``), the scale after the call from the fp32 run (``scale``)
and from the float64 run (``scale64``: the same module in double precision), and per tensor the reference's own
fp32-vs-float64 deviation ``dev.*`` = max|t32 - t64| / max|t64|.  The gradients are those of sum(logits * gout).

    python tests/golden/make_golden_adacos.py        # writes next to this file

Cases:
  rand        B = 8, random rows: the median angle is near pi/2, the pi/4 branch
  built_even  B = 8, six rows at 0.2 .. 0.7 rad from their class direction and two random ones: lower median 0.5, upper 0.6
  built_odd   B = 7, five such rows and two random ones
  traj.0-2    three consecutive calls of one head on three built batches (one W): the second and third call use the moved
              scale inside exp; gradients are kept for the middle call only
The maker asserts adacos_data.assert_covers on every case.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import adacos_data as AD  # noqa: E402

D, N = 512, 100
NO_GRADS = ("traj.0", "traj.2")  # the trajectory keeps the gradients of its middle call only (file size)


def case(out, tag):
    calls = AD.batches(MG.synth, tag)
    res = {}
    for dt in (torch.float32, torch.float64):
        head = MG.ref_heads.AdaCos(D, N)
        if dt == torch.float64:
            head = head.double()
        with torch.no_grad():
            head.W.data = calls[0][1][1].clone().to(dt)
        for name, (x, W, label, gout), branch, mid_gap in calls:
            old = float(head.scale)
            xx = x.clone().to(dt).requires_grad_(True)
            y = head(xx, label)
            gx, gw = torch.autograd.grad(y, [xx, head.W], gout.to(dt))
            res[name, dt] = (y, gx, gw, torch.as_tensor(float(head.scale), dtype=torch.float64))
            if dt == torch.float64:
                st = AD.assert_covers(x, W, label, old, branch, mid_gap)
                assert abs(st["scale"] / float(head.scale) - 1) < 1e-12, (st, float(head.scale))
                for k in ("theta_med", "upper_med", "b_avg"):
                    out["%s.%s" % (name, k)] = np.array(st[k])
    for name, (x, W, label, gout), _, _ in calls:
        y32, gx32, gw32, s32 = res[name, torch.float32]
        y64, gx64, gw64, s64 = res[name, torch.float64]
        idx = torch.tensor(sorted(set(label.tolist()) | set(range(0, N, 20))))
        out[name + ".label"] = MG.npy(label)
        out[name + ".gout"] = MG.npy(gout)
        out[name + ".logits"] = MG.npy(y32)
        if name not in NO_GRADS:
            out[name + ".gx"] = MG.npy(gx32)
            out[name + ".gw_index"] = MG.npy(idx)
            out[name + ".gw"] = MG.npy(gw32.index_select(0, idx))
            out[name + ".gw_norm"] = np.array(float(gw32.detach().double().norm()))
        out[name + ".scale"] = np.array(float(s32))
        out[name + ".scale64"] = np.array(float(s64))
        for k, a, b in (("logits", y32, y64), ("gx", gx32, gx64), ("gw", gw32, gw64), ("scale", s32, s64)):
            if name in NO_GRADS and k in ("gx", "gw"):
                continue
            a, b = a.detach().double(), b.detach()
            out["%s.dev.%s" % (name, k)] = np.array(float((a - b).abs().max() / b.abs().max()))


def g20_adacos():
    out = {}
    for tag in ("rand", "built_even", "built_odd", "traj"):
        case(out, tag)
    for k in sorted(out):
        if np.ndim(out[k]) == 0:
            print("%-32s %s" % (k, out[k]))
    MG.save("g20_adacos", **out)


if __name__ == "__main__":
    g20_adacos()
