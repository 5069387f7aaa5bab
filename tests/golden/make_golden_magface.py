#!/usr/bin/env python3
"""Generate tests/golden/g19_magface.npz: the reference's MagFace head (head/metrics.py:512-553) on CPU.

Runs only in the build container, like make_golden_curricular.py (whose import-only stand-ins and reference imports it
reuses through make_golden.py).  Inputs come from the repo's counter-based generator through tests/magface_data.py, which
the tests import too: B = 8, D = 512, N = 100.  The file holds no inputs, only the labels and the parameters as a check.
Per case it holds the reference's fp32 logits, loss_g (the second output, lamda included) and gx in full, the weight
gradient gw at the columns ``gw_index`` (every label plus every 20th class) with the float64 norm of the whole of it
(``gw_norm``), and per tensor the reference's own fp32-vs-float64 deviation ``dev.*`` = max|t32 - t64| / max|t64| (the
float64 run is the same module in double precision).  The gradients are those of sum(logits * gout) + sum(loss_g * gg)
with gout, gg from magface_data (both outputs take part).

    python tests/golden/make_golden_magface.py        # writes next to this file

Cases:
  rand       random embeddings and weight: every norm inside [l_a, u_a], every target in the margin branch
  built      the constructed batch of magface_data.built (three norm regimes, both target branches), default parameters
  built_am   the same construction, margin_am = 0.1
  built_p    the same construction, scale = 64, l_margin = 0.3, u_margin = 0.6, lamda = 35
The maker asserts magface_data.assert_covers on every built case.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import magface_data as MD  # noqa: E402

B, D, N = 8, 512, 100
CASES = (("rand", {}), ("built", {}), ("built_am", dict(margin_am=0.1)),
         ("built_p", dict(scale=64, l_margin=0.3, u_margin=0.6, lamda=35)))


def case(out, tag, over):
    p = MD.params(**over)
    x, k, label, gout, gg = (MD.built if tag.startswith("built") else MD.random_case)(MG.synth, tag, B, D, N)
    res = {}
    for dt in (torch.float32, torch.float64):
        head = MG.ref_heads.MagFace(D, N, **p)
        with torch.no_grad():
            head.weight.data = k.clone().to(dt)
        xx = x.clone().to(dt).requires_grad_(True)
        y, lg = head(xx, label)
        gx, gw = torch.autograd.grad([y, lg], [xx, head.weight], [gout.to(dt), gg.to(dt)])
        res[dt] = (y, lg, gx, gw)
    st = MD.assert_covers(x, k, label, **p) if tag.startswith("built") else MD.stats64(x, k, label, **p)
    out[tag + ".label"] = MG.npy(label)
    for name, v in list(p.items()) + list(st.items()):
        out["%s.%s" % (tag, name)] = np.array(v)
    y32, lg32, gx32, gw32 = res[torch.float32]
    y64, lg64, gx64, gw64 = res[torch.float64]
    idx = torch.tensor(sorted(set(label.tolist()) | set(range(0, N, 20))))
    out[tag + ".logits"] = MG.npy(y32)
    out[tag + ".loss_g"] = MG.npy(lg32)
    out[tag + ".gx"] = MG.npy(gx32)
    out[tag + ".gw_index"] = MG.npy(idx)
    out[tag + ".gw"] = MG.npy(gw32.index_select(1, idx))
    out[tag + ".gw_norm"] = np.array(float(gw32.detach().double().norm()))
    out[tag + ".gout"] = MG.npy(gout)
    out[tag + ".gg"] = MG.npy(gg)
    for name, a, b in (("logits", y32, y64), ("loss_g", lg32, lg64), ("gx", gx32, gx64), ("gw", gw32, gw64)):
        a, b = a.detach().double(), b.detach()
        out["%s.dev.%s" % (tag, name)] = np.array(float((a - b).abs().max() / b.abs().max()))


def g19_magface():
    out = {}
    for tag, over in CASES:
        case(out, tag, over)
    for k in sorted(out):
        if np.ndim(out[k]) == 0:
            print("%-32s %s" % (k, out[k]))
    MG.save("g19_magface", **out)


if __name__ == "__main__":
    g19_magface()
