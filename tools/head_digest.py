#!/usr/bin/env python3
"""Digest of the five margin heads on the HIP path: per case one SHA-1 over the logits, x.grad, the weight / kernel
gradient and (CurricularFace) t of two consecutive forward + backward calls.  Two trees that print the same lines compute
bit-identical heads (profiles/head_pipeline_refactor.txt).

    python tools/head_digest.py

Cases: every head at (B, N) = (8, 100), (5, 1001), (96, 7001), D = 512; gradients wanted by both inputs, by x only, by the
weight only; FRHIP_SINGLE_STREAM 0 and 1; ArcFace with easy_margin; ShardedMarginLoss at world size 1 (loss and both
gradients).  Inputs come from frhip.synth with fixed seeds.
"""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stylegan-for-facerec_amd"), ROOT]
import torch  # noqa: E402
from frhip import synth  # noqa: E402
from frhip.sharded_head import ShardedMarginLoss  # noqa: E402
from head import metrics as H  # noqa: E402

D = 512
SHAPES = ((8, 100), (5, 1001), (96, 7001))
HEADS = ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace", "ArcFace_easy")
NEEDS = (("both", True, True), ("x", True, False), ("w", False, True))


def make(name, N):
    if name == "CurricularFace":
        head = H.CurricularFace(D, N)  # FaceX-Zoo heads take no device_id
    elif name == "ArcFace_easy":
        head = H.ArcFace(D, N, None, easy_margin=True)
    else:
        head = getattr(H, name)(D, N, None)
    p = list(head.parameters())[0]
    with torch.no_grad():
        p.copy_(synth.uniform(71, "%s.%d.w" % (name, N), tuple(p.shape), -0.1, 0.1))
    return head.cuda(), list(head.parameters())[0]


def sha(tensors):
    h = hashlib.sha1()
    for t in tensors:
        h.update(b"-" if t is None else t.detach().float().cpu().numpy().tobytes())
    return h.hexdigest()


def head_case(name, B, N, need_x, need_w):
    head, p = make(name, N)
    x = synth.normal(71, "x.%d" % B, (B, D), std=0.04).cuda().requires_grad_(need_x)
    label = synth.labels(71, "y.%d.%d" % (B, N), B, N).cuda()
    g = synth.normal(71, "g.%d.%d" % (B, N), (B, N)).cuda()
    p.requires_grad_(need_w)
    out = []
    for _ in range(2):
        x.grad = p.grad = None
        y = head(x, label)
        y.backward(g)
        out += [y, x.grad, p.grad, getattr(head, "t", None)]
    return sha(out)


def sharded_case(name, B, N):
    crit = ShardedMarginLoss(D, N, name, full_weight=synth.uniform(71, "%s.%d.w" % (name, N), (N, D), -0.1, 0.1)).cuda()
    x = synth.normal(71, "x.%d" % B, (B, D), std=0.04).cuda().requires_grad_(True)
    label = synth.labels(71, "y.%d.%d" % (B, N), B, N).cuda()
    out = []
    for _ in range(2):
        x.grad = crit.weight.grad = None
        loss, prec1, prec5 = crit(x, label)
        loss.backward()
        out += [loss, prec1, prec5, x.grad, crit.weight.grad]
    return sha(out)


for single in ("0", "1"):
    os.environ["FRHIP_SINGLE_STREAM"] = single
    for B, N in SHAPES:
        for name in HEADS:
            for tag, need_x, need_w in NEEDS:
                print("HEADDIGEST single_stream=%s %-14s B=%-3d N=%-5d grads=%-4s %s"
                      % (single, name, B, N, tag, head_case(name, B, N, need_x, need_w)))
        for name in ("ArcFace", "CosFace"):
            print("HEADDIGEST single_stream=%s %-14s B=%-3d N=%-5d grads=both %s"
                  % (single, "Sharded" + name, B, N, sharded_case(name, B, N)))
