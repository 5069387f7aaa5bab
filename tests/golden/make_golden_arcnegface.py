#!/usr/bin/env python3
"""Generate tests/golden/g24_arcnegface.npz: the reference's ArcNegFace head (head/metrics.py:394-433) on CPU.

Runs only in the build container, like make_golden_mv_softmax.py (whose import-only stand-ins and reference imports it
reuses through make_golden.py).  The reference's class runs unpatched -- its loop over the rows, backward included.  Inputs
come from the repo's counter-based generator through tests/arcneg_data.py, which the tests import too: B = 8, D = 512,
N = 100.  The file holds no inputs, only the labels and the scalars (margin, scale, alpha, sigma, thresh, mm) as a check.
Per case it holds the reference's fp32 logits and gx in full, the weight gradient gw at the rows ``gw_index`` (the labels of
rows 0 .. 3, one row of each kind, and the two lowest classes that are nobody's label: every class takes gradient through
t) with the float64 norm of the whole of it (``gw_norm``), per tensor the reference's own fp32-vs-float64 deviation
``dev.*`` = max|t32 - t64| / max|t64| (the float64 run is the same module in double precision), and per row the target cosine
``gt``, the label column's value ``a`` and the ``branch`` (1: acos) in float64 (arcneg_data.stats64; the reference keeps
none of them).

    python tests/golden/make_golden_arcnegface.py        # writes next to this file

Cases:
  rand             random embeddings and weight: every row on the acos branch
  built            the constructed batch of arcneg_data.built: target cosines near 0.9, 0.3 and -0.5, and two rows below
                   thresh, near -0.95
  built_m03_s32    the same construction at margin 0.3, scale 32 (thresh -0.955: its two linear rows lie near -0.97)
The maker calls arcneg_data.assert_covers on every built case.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import arcneg_data as AD  # noqa: E402

B, D, N = 8, 512, 100
CASES = (("rand", {}), ("built", {}), ("built_m03_s32", dict(margin=0.3, scale=32)))


def inputs_of(tag, margin):
    if tag.startswith("built"):
        return AD.built(MG.synth, tag, B, D, N, margin)
    return AD.random_case(MG.synth, tag, B, D, N)


def case(out, tag, kw):
    margin = kw.get("margin", 0.5)
    x, w, label, gout = inputs_of(tag, margin)
    res = {}
    for dt in (torch.float32, torch.float64):
        head = MG.ref_heads.ArcNegFace(D, N, **kw)
        with torch.no_grad():
            head.weight.data = w.clone().to(dt)
        xx = x.clone().to(dt).requires_grad_(True)
        y = head(xx, label)
        gx, gw = torch.autograd.grad(y, [xx, head.weight], gout.to(dt))
        res[dt] = (y, gx, gw)
    st = AD.assert_covers(x, w, label, margin) if tag.startswith("built") else AD.stats64(x, w, label, margin)
    out[tag + ".label"] = MG.npy(label)
    for name, v in (("margin", head.margin), ("scale", float(head.scale)), ("alpha", head.alpha), ("sigma", float(head.sigma)),
                    ("thresh", head.thresh), ("mm", head.mm), ("gap", st["gap"]), ("max_abs_gt", st["max_abs_gt"])):
        out["%s.%s" % (tag, name)] = np.array(v)
    out[tag + ".gt"] = MG.npy(st["gt"])
    out[tag + ".a"] = MG.npy(st["a"])
    out[tag + ".branch"] = MG.npy(st["branch"].to(torch.uint8))
    y32, gx32, gw32 = res[torch.float32]
    y64, gx64, gw64 = res[torch.float64]
    taken = set(label.tolist())
    idx = torch.tensor(sorted(set(label[:4].tolist()) | set([j for j in range(N) if j not in taken][:2])))
    out[tag + ".logits"] = MG.npy(y32)
    out[tag + ".gx"] = MG.npy(gx32)
    out[tag + ".gw_index"] = MG.npy(idx)
    out[tag + ".gw"] = MG.npy(gw32.index_select(0, idx))
    out[tag + ".gw_norm"] = np.array(float(gw32.detach().double().norm()))
    for name, a, b in (("logits", y32, y64), ("gx", gx32, gx64), ("gw", gw32, gw64)):
        a, b = a.detach().double(), b.detach()
        out["%s.dev.%s" % (tag, name)] = np.array(float((a - b).abs().max() / b.abs().max()))


def g24_arcnegface():
    out = {}
    for tag, kw in CASES:
        case(out, tag, kw)
    for k in sorted(out):
        if ".dev." in k or k.endswith((".gap", ".max_abs_gt", ".branch", ".gt")):
            print("%-32s %s" % (k, out[k]))
    MG.save("g24_arcnegface", **out)


if __name__ == "__main__":
    g24_arcnegface()
