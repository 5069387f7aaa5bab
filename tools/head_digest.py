#!/usr/bin/env python3
"""Digest of the heads, the class-sharded head and the losses on the HIP path: per case one SHA-1 over everything the case
produced in two consecutive forward + backward calls.  Two trees that print the same lines compute bit-identical heads
(profiles/head_pipeline_refactor.txt, profiles/head_rows_refactor.txt).  Only public modules are used, so the same file
runs in either tree.

    python tools/head_digest.py

Heads: every head of head/metrics.py, built as tools/head_time.py builds them (both MV_Softmax forms, ArcFace with and
without easy_margin): the logits (MagFace: and loss_g, with gradients for both), x.grad, the gradient of every parameter
(Softmax: the bias too) and the head's one-float buffer after each call (CurricularFace's t, AdaCos's scale).
ShardedMarginLoss at world size 1 for the six heads it serves, with loss="Focal" and loss="Softmax": the loss, both
precisions, x.grad and the gradient of every parameter.  FocalLoss, CrossEntropyLoss and accuracy on contiguous logits and on
the [B, N] view of a [B, pad(N, 4)] store: the loss, both precisions, the gradient of the logits.

Cases: (B, N) = (8, 100), (5, 1001), (96, 7001), D = 512; the heads with gradients wanted by both inputs, by x only, by the
parameters only; FRHIP_SINGLE_STREAM 0 and 1.  Inputs come from frhip.synth with fixed seeds.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stylegan-for-facerec_amd"), ROOT]
import torch  # noqa: E402
from frhip import sharded_head, synth  # noqa: E402
from head import metrics as H  # noqa: E402
from loss.focal import FocalLoss  # noqa: E402
from loss.softmax import CrossEntropyLoss  # noqa: E402
from util.utils import accuracy  # noqa: E402

D = 512
SHAPES = ((8, 100), (5, 1001), (96, 7001))
HEADS = ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace", "ArcFace_easy", "MagFace", "AdaCos", "NPCFace",
         "MV_Softmax", "MV_Softmax-arc", "CircleLoss", "AM_Softmax", "ArcNegFace", "Softmax")
ZOO = ("CurricularFace", "MagFace", "AdaCos", "NPCFace", "CircleLoss", "AM_Softmax", "ArcNegFace")  # no device_id
SHARDED = ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace", "Softmax")
NEEDS = (("both", True, True), ("x", True, False), ("w", False, True))


def make(name, N):
    if name in ("MV_Softmax", "MV_Softmax-arc"):  # the additive-margin form, or the ArcFace-style one
        head = H.MV_Softmax(D, N, name == "MV_Softmax")
    elif name == "ArcFace_easy":
        head = H.ArcFace(D, N, None, easy_margin=True)
    else:
        head = getattr(H, name)(D, N) if name in ZOO else getattr(H, name)(D, N, None)
    params = list(head.parameters())  # one parameter; the Softmax head's bias is a second
    with torch.no_grad():
        for i, p in enumerate(params):
            p.copy_(synth.uniform(71, "%s.%d.w%s" % (name, N, i or ""), tuple(p.shape), -0.1, 0.1))
    return head.cuda(), list(head.parameters())


def sha(tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(b"-" if t is None else t.detach().float().cpu().numpy().tobytes())
    return h.hexdigest()


def batch(B, N, x_std=0.04):
    x = synth.normal(71, "x.%d" % B, (B, D), std=x_std).cuda()
    return x, synth.labels(71, "y.%d.%d" % (B, N), B, N).cuda()


def head_case(name, B, N, need_x, need_w):
    head, params = make(name, N)
    x, label = batch(B, N, 1.0 if name == "MagFace" else 0.04)  # MagFace: ||x|| inside [l_a, u_a], the radial terms live
    x.requires_grad_(need_x)
    g = [synth.normal(71, "g.%d.%d" % (B, N), (B, N)).cuda(), torch.full((B, 1), 1.0 / B).cuda()]
    for p in params:
        p.requires_grad_(need_w)
    out = []
    for _ in range(2):
        x.grad = None
        for p in params:
            p.grad = None
        y = head(x, label)
        y = y if isinstance(y, tuple) else (y,)
        torch.autograd.backward(y, g[:len(y)])
        out += list(y) + [x.grad] + [p.grad for p in params] + [getattr(head, "t", None), getattr(head, "scale", None)]
    return sha(t for t in out if t is None or torch.is_tensor(t))


def sharded_case(name, loss, B, N):
    shape = (N, D) if sharded_head.CLASS_DIM[name] == 0 else (D, N)
    kw = {"full_bias": synth.uniform(71, "%s.%d.w1" % (name, N), (N,), -0.1, 0.1)} if name == "Softmax" else {}
    crit = sharded_head.ShardedMarginLoss(D, N, name, full_weight=synth.uniform(71, "%s.%d.w" % (name, N), shape, -0.1, 0.1),
                                          loss=loss, **kw).cuda()
    x, label = batch(B, N)
    x.requires_grad_(True)
    params = list(crit.parameters())
    out = []
    for _ in range(2):
        x.grad = None
        for p in params:
            p.grad = None
        loss_v, prec1, prec5 = crit(x, label)
        loss_v.backward()
        out += [loss_v, prec1, prec5, x.grad] + [p.grad for p in params] + [getattr(crit, "t", None)]
    return sha(out)


def loss_case(crit, B, N, view):
    ld = (N + 3) // 4 * 4 if view else N
    store = torch.zeros(B, ld)
    store[:, :N] = synth.normal(71, "z.%d.%d" % (B, N), (B, N), std=4.0)
    store = store.cuda().requires_grad_(True)
    label = synth.labels(71, "y.%d.%d" % (B, N), B, N).cuda()
    out = []
    for _ in range(2):
        store.grad = None
        z = store[:, :N] if view else store
        loss_v = crit(z, label)
        loss_v = loss_v[0] if isinstance(loss_v, tuple) else loss_v  # FocalLoss returns (loss, None)
        loss_v.backward()
        out += [loss_v, store.grad] + list(accuracy(z.detach(), label, topk=(1, 5)))
    return sha(out)


def line(single, name, B, N, tag, digest):
    print("HEADDIGEST single_stream=%s %-14s B=%-3d N=%-5d grads=%-4s %s" % (single, name, B, N, tag, digest), flush=True)


for single in ("0", "1"):
    os.environ["FRHIP_SINGLE_STREAM"] = single
    for B, N in SHAPES:
        for name in HEADS:
            for tag, need_x, need_w in NEEDS:
                line(single, name, B, N, tag, head_case(name, B, N, need_x, need_w))
        for name in SHARDED:
            for loss in ("Focal", "Softmax"):
                line(single, "Sharded%s/%s" % (name, loss), B, N, "both", sharded_case(name, loss, B, N))
        for name, crit in (("FocalLoss", FocalLoss()), ("CrossEntropyLoss", CrossEntropyLoss())):
            for view in (False, True):
                line(single, "%s/%s" % (name, "view" if view else "contiguous"), B, N, "z", loss_case(crit, B, N, view))
