#!/usr/bin/env python3
"""Generate tests/golden/g18_curricular.npz: the reference's CurricularFace head (head/metrics.py:475-510) on CPU.

Runs only in the build container, like make_golden_heads.py (whose import-only stand-ins and reference imports it reuses
through make_golden.py).  Inputs come from the repo's counter-based generator through tests/curricular_data.py, which the
tests import too: B = 8, D = 512, N = 100.  The file holds no inputs, only the labels and the scalars (m, s, t before the
call) as a check.  Per case it holds the reference's fp32 logits and gx in full, the kernel gradient gw at the columns
``gw_index`` (every label plus every 20th class) with the float64 norm of the whole of it (``gw_norm``), ``t`` after the call
(fp32, and ``t64`` from the float64 run), and per tensor the reference's own fp32-vs-float64 deviation ``dev.*`` =
max|t32 - t64| / max|t64| (the float64 run is the same module in double precision).

    python tests/golden/make_golden_curricular.py        # writes next to this file

Cases:
  rand_t0     random embeddings and kernel, t = 0 (a first call): every negative is hard
  built_t0    the constructed batch of curricular_data.built (easy and hard negatives, both target branches), t = 0
  built_t03   the same construction, t preset to 0.3 (a later call)
  built_m03   the same construction, m = 0.3, t preset to 0.1
The maker asserts on the float64 run of every built case that 10 % .. 90 % of the non-target entries are hard, that both
target branches occur and that |tl| <= 0.99.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import curricular_data as CD  # noqa: E402

B, D, N = 8, 512, 100
CASES = (("rand_t0", 0.5, 0.0), ("built_t0", 0.5, 0.0), ("built_t03", 0.5, 0.3), ("built_m03", 0.3, 0.1))


def inputs_of(tag):
    return (CD.built if tag.startswith("built") else CD.random_case)(MG.synth, tag, B, D, N)


def case(out, tag, m, t0):
    x, k, label, gout = inputs_of(tag)
    res = {}
    for dt in (torch.float32, torch.float64):
        head = MG.ref_heads.CurricularFace(D, N, m=m)
        with torch.no_grad():
            head.kernel.data = k.clone().to(dt)
            head.t = torch.full((1,), t0, dtype=dt)
        xx = x.clone().to(dt).requires_grad_(True)
        y = head(xx, label)
        gx, gw = torch.autograd.grad(y, [xx, head.kernel], gout.to(dt))
        res[dt] = (y, gx, gw, head.t.detach().reshape(1))
    frac, first, second, tmax = CD.stats64(x, k, label, m)
    if tag.startswith("built"):
        CD.assert_covers_both_branches(x, k, label, m)
    out[tag + ".label"] = MG.npy(label)
    for name, v in (("m", m), ("s", 64.0), ("t0", t0), ("hard_fraction", frac), ("rows_first_branch", first),
                    ("rows_second_branch", second), ("max_abs_tl", tmax)):
        out["%s.%s" % (tag, name)] = np.array(v)
    y32, gx32, gw32, t32 = res[torch.float32]
    y64, gx64, gw64, t64 = res[torch.float64]
    idx = torch.tensor(sorted(set(label.tolist()) | set(range(0, N, 20))))
    out[tag + ".logits"] = MG.npy(y32)
    out[tag + ".gx"] = MG.npy(gx32)
    out[tag + ".gw_index"] = MG.npy(idx)
    out[tag + ".gw"] = MG.npy(gw32.index_select(1, idx))
    out[tag + ".gw_norm"] = np.array(float(gw32.detach().double().norm()))
    out[tag + ".t"] = MG.npy(t32)
    out[tag + ".t64"] = MG.npy(t64)
    for name, a, b in (("logits", y32, y64), ("gx", gx32, gx64), ("gw", gw32, gw64), ("t", t32, t64)):
        a, b = a.detach().double(), b.detach()
        out["%s.dev.%s" % (tag, name)] = np.array(float((a - b).abs().max() / b.abs().max()))


def g18_curricular():
    out = {}
    for tag, m, t0 in CASES:
        case(out, tag, m, t0)
    for k in sorted(out):
        if ".dev." in k or k.endswith((".hard_fraction", ".rows_first_branch", ".rows_second_branch", ".max_abs_tl", ".t")):
            print("%-32s %s" % (k, out[k]))
    MG.save("g18_curricular", **out)


if __name__ == "__main__":
    g18_curricular()
