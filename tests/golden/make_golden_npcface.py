#!/usr/bin/env python3
"""Generate tests/golden/g21_npcface.npz: the reference's NPCFace head (head/metrics.py:592-636) on CPU.

Runs only in the build container, like make_golden_curricular.py (whose import-only stand-ins and reference imports it
reuses through make_golden.py).  The reference builds its hard mask with ``.type(torch.FloatTensor).cuda()`` (:622);
``torch.Tensor.cuda`` is patched to the identity while its module runs, and restored afterwards.  Inputs come from the repo's
counter-based generator through tests/npcface_data.py, which the tests import too: B = 8, D = 512, N = 100.  The file holds
no inputs, only the labels and the scalars (margin, scale, m0, m1, t, a) as a check.  Per case it holds the reference's fp32
logits and gx in full, the kernel gradient gw at the columns ``gw_index`` (every label plus every 20th class) with the
float64 norm of the whole of it (``gw_norm``), per tensor the reference's own fp32-vs-float64 deviation ``dev.*`` =
max|t32 - t64| / max|t64| (the float64 run is the same module in double precision), and per row ``avg`` and ``count`` of the
hard negatives in float64 (npcface_data.stats64; the reference keeps neither).

    python tests/golden/make_golden_npcface.py        # writes next to this file

Cases:
  rand        random embeddings and kernel: every negative is hard, avg ~ 0
  built       the constructed batch of npcface_data.built (the three kinds of row), margin 0.5
  built_m03   the same construction, margin 0.3
  built_t12   the same construction, t = 1.2, a = 0.1, m0 = 0.3, m1 = 0.3 set on the module
The maker calls npcface_data.assert_covers on every built case.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import npcface_data as ND  # noqa: E402

B, D, N = 8, 512, 100
CASES = (("rand", 0.5, {}), ("built", 0.5, {}), ("built_m03", 0.3, {}),
         ("built_t12", 0.5, dict(t=1.2, a=0.1, m0=0.3, m1=0.3)))


def inputs_of(tag):
    return (ND.built if tag.startswith("built") else ND.random_case)(MG.synth, tag, B, D, N)


def case(out, tag, margin, attrs):
    x, k, label, gout = inputs_of(tag)
    res = {}
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **kw: self
    try:
        for dt in (torch.float32, torch.float64):
            head = MG.ref_heads.NPCFace(D, N, margin=margin)
            for name, v in attrs.items():
                setattr(head, name, v)
            with torch.no_grad():
                head.kernel.data = k.clone().to(dt)
            xx = x.clone().to(dt).requires_grad_(True)
            y = head(xx, label)
            gx, gw = torch.autograd.grad(y, [xx, head.kernel], gout.to(dt))
            res[dt] = (y, gx, gw)
    finally:
        torch.Tensor.cuda = real_cuda
    st = ND.assert_covers(x, k, label, margin) if tag.startswith("built") else ND.stats64(x, k, label, margin)
    out[tag + ".label"] = MG.npy(label)
    for name, v in (("margin", margin), ("scale", float(head.scale)), ("m0", head.m0), ("m1", head.m1), ("t", head.t),
                    ("a", head.a), ("rows_negative", st["negative"]), ("rows_none", st["none"]),
                    ("rows_some", st["some"]), ("max_abs_c", st["max_abs_c"]), ("min_gap", st["min_gap"])):
        out["%s.%s" % (tag, name)] = np.array(v)
    out[tag + ".avg"] = MG.npy(st["avg"])
    out[tag + ".count"] = MG.npy(st["count"])
    y32, gx32, gw32 = res[torch.float32]
    y64, gx64, gw64 = res[torch.float64]
    idx = torch.tensor(sorted(set(label.tolist()) | set(range(0, N, 20))))
    out[tag + ".logits"] = MG.npy(y32)
    out[tag + ".gx"] = MG.npy(gx32)
    out[tag + ".gw_index"] = MG.npy(idx)
    out[tag + ".gw"] = MG.npy(gw32.index_select(1, idx))
    out[tag + ".gw_norm"] = np.array(float(gw32.detach().double().norm()))
    for name, a, b in (("logits", y32, y64), ("gx", gx32, gx64), ("gw", gw32, gw64)):
        a, b = a.detach().double(), b.detach()
        out["%s.dev.%s" % (tag, name)] = np.array(float((a - b).abs().max() / b.abs().max()))


def g21_npcface():
    out = {}
    for tag, margin, attrs in CASES:
        case(out, tag, margin, attrs)
    for k in sorted(out):
        if ".dev." in k or k.endswith((".rows_negative", ".rows_none", ".rows_some", ".max_abs_c", ".min_gap", ".avg", ".count")):
            print("%-32s %s" % (k, out[k]))
    MG.save("g21_npcface", **out)


if __name__ == "__main__":
    g21_npcface()
