#!/usr/bin/env python3
"""Generate tests/golden/g25_softmax.npz: the reference's Softmax head (head/metrics.py:12-63) under nn.CrossEntropyLoss(),
the pair its train.py builds for HEAD_NAME / LOSS_NAME 'Softmax' (train.py:237-238, :300-302), on CPU.

Runs only in the build container, like make_golden_arcnegface.py (whose import-only stand-ins and reference imports it
reuses through make_golden.py).  The reference's class runs unpatched, as ``Softmax(512, N, None)``; its constructor calls
``nn.init.zero_``, a name this torch no longer has, so the maker lends it ``nn.init.zeros_`` for the call.  Inputs come
from the repo's counter-based generator through tests/softmax_data.py, which the tests import too; the file holds no
inputs, only the labels as a check.  Cases (B, N) = (6, 37) and (8, 100).  Per case it holds the reference's fp32 logits,
loss, gx and gbias in full, the weight gradient gw at the rows ``gw_index`` (softmax_data.gw_rows) with the float64 norm of the whole of
it (``gw_norm``), and the spread of the logits (``logit_absmax``).

    python tests/golden/make_golden_softmax.py        # writes next to this file
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import softmax_data as SD  # noqa: E402


def case(out, B, N):
    tag = SD.tag_of(B, N)
    x, w, b, label = SD.case(MG.synth, B, N)
    if not hasattr(torch.nn.init, "zero_"):
        torch.nn.init.zero_ = torch.nn.init.zeros_
    head = MG.ref_heads.Softmax(SD.D, N, None)
    with torch.no_grad():
        head.weight.copy_(w)
        head.bias.copy_(b)
    xx = x.clone().requires_grad_(True)
    y = head(xx)
    loss = torch.nn.CrossEntropyLoss()(y, label)
    gx, gw, gb = torch.autograd.grad(loss, [xx, head.weight, head.bias])
    assert int(label[0]) == 0 and int(label[-1]) == N - 1 and float(b.abs().min()) > 0
    idx = SD.gw_rows(label, N)
    out[tag + ".label"] = MG.npy(label)
    out[tag + ".logits"] = MG.npy(y)
    out[tag + ".loss"] = MG.npy(loss)
    out[tag + ".gx"] = MG.npy(gx)
    out[tag + ".gb"] = MG.npy(gb)
    out[tag + ".gw_index"] = MG.npy(idx)
    out[tag + ".gw"] = MG.npy(gw.index_select(0, idx))
    out[tag + ".gw_norm"] = np.array(float(gw.detach().double().norm()))
    out[tag + ".logit_absmax"] = np.array(float(y.detach().abs().max()))
    print("%-16s loss %.6f  |logit| max %.3f" % (tag, float(loss), float(y.detach().abs().max())))


def g25_softmax():
    out = {}
    for B, N in SD.CASES:
        case(out, B, N)
    MG.save("g25_softmax", **out)


if __name__ == "__main__":
    g25_softmax()
