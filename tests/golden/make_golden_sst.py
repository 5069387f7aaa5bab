#!/usr/bin/env python3
"""Generate tests/golden/g27_sst_prototype.npz: the reference's SST_Prototype head (head/metrics.py:638-708) on CPU.

Runs only in the build container, like make_golden_npcface.py (whose import-only stand-ins and reference imports it reuses
through make_golden.py).  The reference moves its label with ``.cuda()`` (:696); ``torch.Tensor.cuda`` is patched to the
identity while its module runs, and restored afterwards.  The reference's module also calls ``random.random()`` (:703)
without importing ``random``; the maker puts the standard module into its namespace for the run.  Inputs come from the repo's counter-based generator through
tests/sst_data.py, which the tests import too: B = 8, D = 512, Q = 32, scale 30; the queue is set from the generator and
``random.seed(COIN_SEED)`` fixes the coin.  The file holds no inputs.

    python tests/golden/make_golden_sst.py        # writes next to this file

Per loss type (``softmax``; ``am_softmax``, margin 0.35; ``arc_softmax``, margin 0.5) a trajectory of 5 calls at index 0, 8,
16, 24 and 0 again, so the window wraps and overwrites; the maker asserts that both coin outcomes occur in each.  Per call
``<loss>.<k>.``: ``out1`` / ``out2`` / ``label``, ``coin`` (1: the queue took g1) and ``index`` after the call, ``label_list``
and the sorted ``id_set``, ``gp1`` / ``gp2`` for the generated upstream gradients, ``window`` (the written columns of the
queue, [D, B]) and ``queue_norm`` (the float64 norm of the whole queue), and per tensor the reference's own
fp32-vs-float64 deviation ``dev.*`` = max|t32 - t64| / max|t64| (the float64 run is the same module in double precision).
The maker calls sst_data.assert_covers on every call's inputs.
"""
import os
import random
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stubs + the reference's head/metrics.py
import sst_data as SD  # noqa: E402

B, D, Q, CALLS = 8, 512, 32, 5
COIN_SEED = 27


def trajectory(out, loss_type, margin):
    queue0 = SD.initial_queue(MG.synth, "g27", D, Q)
    res = {}
    real_cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **kw: self
    had_random = hasattr(MG.ref_heads, "random")
    MG.ref_heads.random = random
    try:
        for dt in (torch.float32, torch.float64):
            head = MG.ref_heads.SST_Prototype(D, Q, scale=SD.SCALE, loss_type=loss_type, margin=margin)
            head.queue = queue0.clone()
            head = head.to(dt)
            random.seed(COIN_SEED)
            for k in range(CALLS):
                p1, g2, p2, g1, ids, go1, go2 = SD.step(MG.synth, "g27." + loss_type, k, B, D, Q, queue0)
                SD.assert_covers(p1, g2, p2, g1)
                index = head.index
                a1, a2 = p1.clone().to(dt).requires_grad_(True), p2.clone().to(dt).requires_grad_(True)
                o1, o2, label, id_set = head(a1, g2.to(dt), a2, g1.to(dt), ids)
                gp1, gp2 = torch.autograd.grad((o1 * go1.to(dt)).sum() + (o2 * go2.to(dt)).sum(), [a1, a2])
                window = head.queue[:, index:index + B].clone()
                is_g1 = torch.equal(window, F.normalize(g1.to(dt)).t())
                assert is_g1 or torch.equal(window, F.normalize(g2.to(dt)).t())
                res[dt, k] = dict(out1=o1, out2=o2, gp1=gp1, gp2=gp2, label=label, coin=int(is_g1), index=head.index,
                                  label_list=list(head.label_list), id_set=sorted(id_set), window=window,
                                  queue_norm=float(head.queue.double().norm()))
    finally:
        torch.Tensor.cuda = real_cuda
        if not had_random:
            del MG.ref_heads.random
    coins = [res[torch.float32, k]["coin"] for k in range(CALLS)]
    assert set(coins) == {0, 1}, coins
    assert coins == [res[torch.float64, k]["coin"] for k in range(CALLS)]
    for k in range(CALLS):
        r32, r64 = res[torch.float32, k], res[torch.float64, k]
        pre = "%s.%d." % (loss_type, k)
        for name in ("out1", "out2", "gp1", "gp2", "window"):
            out[pre + name] = MG.npy(r32[name])
        out[pre + "label"] = MG.npy(r32["label"])
        for name in ("coin", "index", "queue_norm"):
            out[pre + name] = np.array(r32[name])
        out[pre + "label_list"] = np.array(r32["label_list"], dtype=np.int64)
        out[pre + "id_set"] = np.array(r32["id_set"], dtype=np.int64)
        for name in ("out1", "out2", "gp1", "gp2"):
            a, b = r32[name].detach().double(), r64[name].detach()
            out[pre + "dev." + name] = np.array(float((a - b).abs().max() / b.abs().max()))
    out[loss_type + ".margin"] = np.array(margin)
    out[loss_type + ".coins"] = np.array(coins)


def g27_sst_prototype():
    out = {}
    for loss_type, margin in SD.LOSS_TYPES:
        trajectory(out, loss_type, margin)
    for k in sorted(out):
        if ".dev." in k or k.endswith((".coins", ".index")):
            print("%-32s %s" % (k, out[k]))
    MG.save("g27_sst_prototype", **out)


if __name__ == "__main__":
    g27_sst_prototype()
