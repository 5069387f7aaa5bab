#!/usr/bin/env python3
"""Generate tests/golden/g23_circle.npz: the reference's CircleLoss (head/metrics.py:435-473) and AM_Softmax (:371-392) heads
on CPU.

Runs only in the build container, like make_golden_mv_softmax.py (whose import-only stand-ins and reference imports it
reuses through make_golden.py).  The reference's classes run unpatched, backward included (torch warns that indexing with
uint8 masks is deprecated; the results are those of bool masks).  Inputs come from the repo's counter-based generator through
tests/circle_data.py, which the tests import too: B = 8, D = 512, N = 100.  The file holds no inputs, only the labels and the
scalars (margin, and gamma or scale as ``scale``) as a check.  Per case it holds the reference's fp32 logits and gx in full,
the weight gradient gw at the columns ``gw_index`` (the labels of rows 0 .. 3, one row of each kind, plus in a built case the
columns of row 1's two smallest cosines: its planted dead and barely alive negatives) with the float64 norm of the whole of
it (``gw_norm``), per tensor the reference's own fp32-vs-float64 deviation ``dev.*`` = max|t32 - t64| / max|t64| (the float64
run is the same module in double precision), and per row the target cosine ``gt`` and the number ``dead`` of negatives at or
below -margin in float64 (circle_data.stats64; CircleLoss's dead negatives).

    python tests/golden/make_golden_circle.py        # writes next to this file

Cases:
  circle_rand, am_rand                random embeddings and weight: no negative is dead
  circle_built, am_built              the constructed batch of circle_data.built, the heads' defaults
  circle_built_m04                    the same construction, margin 0.4, gamma 80 (not a power of two)
  am_built_m05                        the same construction, margin 0.5, scale 64
The maker calls circle_data.assert_covers on every built case.
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import circle_data as CD  # noqa: E402

B, D, N = 8, 512, 100
CASES = (("circle_rand", "circle", {}), ("circle_built", "circle", {}),
         ("circle_built_m04", "circle", dict(margin=0.4, gamma=80)),
         ("am_rand", "am", {}), ("am_built", "am", {}), ("am_built_m05", "am", dict(margin=0.5, scale=64)))


def inputs_of(tag, head, margin):
    if "built" in tag:
        return CD.built(MG.synth, tag, B, D, N, head, margin)
    return CD.random_case(MG.synth, tag, B, D, N)


def case(out, tag, head, kw):
    margin = kw.get("margin", CD.DEFAULTS[head][0])
    x, k, label, gout = inputs_of(tag, head, margin)
    cls = MG.ref_heads.CircleLoss if head == "circle" else MG.ref_heads.AM_Softmax
    res = {}
    for dt in (torch.float32, torch.float64):
        mod = cls(D, N, **kw)
        with torch.no_grad():
            mod.weight.data = k.clone().to(dt)
        xx = x.clone().to(dt).requires_grad_(True)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            y = mod(xx, label)
            gx, gw = torch.autograd.grad(y, [xx, mod.weight], gout.to(dt))
        res[dt] = (y, gx, gw)
    assert mod.margin == margin
    st = CD.assert_covers(x, k, label, margin) if "built" in tag else CD.stats64(x, k, label, margin)
    out[tag + ".label"] = MG.npy(label)
    for name, v in (("margin", mod.margin), ("scale", float(mod.gamma if head == "circle" else mod.scale)),
                    ("max_abs_c", st["max_abs_c"])):
        out["%s.%s" % (tag, name)] = np.array(v)
    for name in ("gt", "dead"):
        out["%s.%s" % (tag, name)] = MG.npy(st[name])
    y32, gx32, gw32 = res[torch.float32]
    y64, gx64, gw64 = res[torch.float64]
    c1 = CD.cosines64(x[1:2], k)[0]
    low = c1.argsort()
    idx = torch.tensor(sorted(set(label[:4].tolist()) | ({int(low[0]), int(low[1])} if "built" in tag else set())))
    out[tag + ".logits"] = MG.npy(y32)
    out[tag + ".gx"] = MG.npy(gx32)
    out[tag + ".gw_index"] = MG.npy(idx)
    out[tag + ".gw"] = MG.npy(gw32.index_select(1, idx))
    out[tag + ".gw_norm"] = np.array(float(gw32.detach().double().norm()))
    for name, a, b in (("logits", y32, y64), ("gx", gx32, gx64), ("gw", gw32, gw64)):
        a, b = a.detach().double(), b.detach()
        out["%s.dev.%s" % (tag, name)] = np.array(float((a - b).abs().max() / b.abs().max()))


def g23_circle():
    out = {}
    for tag, head, kw in CASES:
        case(out, tag, head, kw)
    for k in sorted(out):
        if ".dev." in k or k.endswith((".max_abs_c", ".dead", ".gt", ".scale", ".margin")):
            print("%-32s %s" % (k, out[k]))
    MG.save("g23_circle", **out)


if __name__ == "__main__":
    g23_circle()
