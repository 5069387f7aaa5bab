#!/usr/bin/env python3
"""Generate tests/golden/g22_mv_softmax.npz: the reference's MV_Softmax head (head/metrics.py:555-590) on CPU.

Runs only in the build container, like make_golden_npcface.py (whose import-only stand-ins and reference imports it
reuses through make_golden.py).  The reference's class runs unpatched, backward included.  Inputs come from the repo's
counter-based generator through tests/mv_softmax_data.py, which the tests import too: B = 8, D = 512, N = 100.  The file
holds no inputs, only the labels and the scalars (is_am, margin, mv_weight, scale) as a check.  Per case it holds the
reference's fp32 logits and gx in full, the weight gradient gw at the columns ``gw_index`` (the labels of rows 0 .. 3, one
row of each kind, plus in a built case the columns of row 1's largest and third-largest non-target cosine: its planted
negatives at thr + 0.10, hard, and thr - 0.05, easy; so few columns keep the file below g20 / g21 with six cases) with the
float64 norm of the whole of it (``gw_norm``), per tensor the reference's own fp32-vs-float64 deviation
``dev.*`` = max|t32 - t64| / max|t64| (the float64 run is the same module in double precision), per row the target cosine
``gt``, the threshold ``thr`` and the number of hard negatives ``count`` in float64 (mv_softmax_data.stats64; the reference
keeps none of them), and the number of rows of each kind.

    python tests/golden/make_golden_mv_softmax.py        # writes next to this file

Cases:
  rand_am, rand_arc              random embeddings and weight: every negative is hard
  built_am, built_arc            the constructed batch of mv_softmax_data.built (the four kinds of row), margin 0.35
  built_am_m05, built_arc_m05    the same construction, margin 0.5, mv_weight 1.3, scale 64
The maker calls mv_softmax_data.assert_covers on every built case.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import mv_softmax_data as MD  # noqa: E402

B, D, N = 8, 512, 100
CASES = (("rand_am", True, {}), ("rand_arc", False, {}), ("built_am", True, {}), ("built_arc", False, {}),
         ("built_am_m05", True, dict(margin=0.5, mv_weight=1.3, scale=64)),
         ("built_arc_m05", False, dict(margin=0.5, mv_weight=1.3, scale=64)))


def inputs_of(tag, is_am, margin):
    if tag.startswith("built"):
        return MD.built(MG.synth, tag, B, D, N, is_am, margin)
    return MD.random_case(MG.synth, tag, B, D, N)


def case(out, tag, is_am, kw):
    margin = kw.get("margin", 0.35)
    x, k, label, gout = inputs_of(tag, is_am, margin)
    res = {}
    for dt in (torch.float32, torch.float64):
        head = MG.ref_heads.MV_Softmax(D, N, is_am, **kw)
        with torch.no_grad():
            head.weight.data = k.clone().to(dt)
        xx = x.clone().to(dt).requires_grad_(True)
        y = head(xx, label)
        gx, gw = torch.autograd.grad(y, [xx, head.weight], gout.to(dt))
        res[dt] = (y, gx, gw)
    st = MD.assert_covers(x, k, label, is_am, margin) if tag.startswith("built") else MD.stats64(x, k, label, is_am, margin)
    out[tag + ".label"] = MG.npy(label)
    for name, v in (("is_am", int(is_am)), ("margin", head.margin), ("mv_weight", head.mv_weight),
                    ("scale", float(head.scale)), ("max_abs_c", st["max_abs_c"]), ("min_gap", st["min_gap"]),
                    ("gt_gap", st["gt_gap"])) + tuple(("rows_" + n, st[n]) for n in MD.KINDS):
        out["%s.%s" % (tag, name)] = np.array(v)
    for name in ("gt", "thr", "count"):
        out["%s.%s" % (tag, name)] = MG.npy(st[name])
    y32, gx32, gw32 = res[torch.float32]
    y64, gx64, gw64 = res[torch.float64]
    c1 = torch.nn.functional.normalize(x[1:2].double()) @ torch.nn.functional.normalize(k.double(), dim=0)
    c1[0, label[1]] = -2.0
    top = c1[0].argsort(descending=True)
    idx = torch.tensor(sorted(set(label[:4].tolist()) | ({int(top[0]), int(top[2])} if tag.startswith("built") else set())))
    out[tag + ".logits"] = MG.npy(y32)
    out[tag + ".gx"] = MG.npy(gx32)
    out[tag + ".gw_index"] = MG.npy(idx)
    out[tag + ".gw"] = MG.npy(gw32.index_select(1, idx))
    out[tag + ".gw_norm"] = np.array(float(gw32.detach().double().norm()))
    for name, a, b in (("logits", y32, y64), ("gx", gx32, gx64), ("gw", gw32, gw64)):
        a, b = a.detach().double(), b.detach()
        out["%s.dev.%s" % (tag, name)] = np.array(float((a - b).abs().max() / b.abs().max()))


def g22_mv_softmax():
    out = {}
    for tag, is_am, kw in CASES:
        case(out, tag, is_am, kw)
    for k in sorted(out):
        if ".dev." in k or ".rows_" in k or k.endswith((".max_abs_c", ".min_gap", ".gt_gap", ".count")):
            print("%-32s %s" % (k, out[k]))
    MG.save("g22_mv_softmax", **out)


if __name__ == "__main__":
    g22_mv_softmax()
