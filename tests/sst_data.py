"""Inputs for the SST_Prototype tests and for tests/golden/make_golden_sst.py (which imports this file, so the fixture and the
tests cannot build different data), the float64 statistics both assert on, and ``from_cos``, the head's arithmetic from given
cosines (for the tests of the C entry points).

SST_Prototype (reference head/metrics.py:638-708) scores the probe rows p1 against a queue whose window [index, index + B)
holds the gallery rows g2 of the same identities, and p2 against the same queue with g1 there; row i's label is the window
column i.  ``step`` builds one call's inputs.  Identity i of a call has a direction u_i; its gallery views are u_i plus a
little noise; p1_i lies at the planted cosine ``planted(i, k)`` in [0.2, 0.95] from g2_i and p2_i at ``planted(i + 4, k)``
from g1_i.  By i % 4 the rest of a probe row leans on something else, which plants a high negative:
  1: the gallery row of identity i + 1 of the same call, a negative inside the window;
  2: column ``(7 i + 3) % Q`` of the initial queue, a negative outside it wherever that column has not been replaced yet.
Nothing depends on the evolving queue, so the host path, the device path and the fixture's maker see the same inputs.  No
target cosine comes within 1e-3 of +-1: the derivative of ``arc_softmax`` has its poles there.
"""
import math

import numpy as np
import torch

SEED = 27
LOSS_TYPES = (("softmax", 0.0), ("am_softmax", 0.35), ("arc_softmax", 0.5))
SCALE = 30.0


def initial_queue(synth, tag, D, Q):
    """[D, Q] float32, columns of norm 1: normalised in float64, rounded once."""
    q = synth.normal(SEED, tag + ".queue", (D, Q)).double()
    return (q / q.norm(dim=0, keepdim=True)).float()


def planted(i, k):
    """The target cosine planted in row i of call k: 0.2 .. 0.95; at most 0.7 in the rows that lean on a negative (i % 4 in
    (1, 2)), which leaves the negative a cosine above 0.6."""
    if i % 4 in (1, 2):
        return (0.22, 0.45, 0.7)[(i // 4 + k) % 3] - 0.01 * (i % 2)
    return (0.22, 0.45, 0.7, 0.95)[(i // 2 + k) % 4] - 0.01 * ((i // 4) % 3)


def _at_cosine(g, lean, v, c, lean_w):
    """A row at cosine c from the direction g, the remainder split between ``lean`` (weight lean_w) and the noise v."""
    u = g / g.norm()
    o = lean_w * lean / lean.norm() + (1 - lean_w) * v / v.norm()
    o = o - (o @ u) * u
    return c * u + math.sqrt(1 - c * c) * o / o.norm()


def step(synth, tag, k, B, D, Q, queue0):
    """(p1, g2, p2, g1, ids, gout1, gout2) of call k: fp32 [B, D] embeddings, int64 ids [B] (1000 k + 7 i: distinct over a
    trajectory), fp32 upstream gradients [B, Q] of the two outputs.  ``queue0`` is ``initial_queue``'s tensor."""
    name = "%s.%d" % (tag, k)
    u = synth.normal(SEED, name + ".u", (B, D)).double()
    g1 = u + 0.05 * synth.normal(SEED, name + ".n1", (B, D)).double()
    g2 = u + 0.05 * synth.normal(SEED, name + ".n2", (B, D)).double()
    v1 = synth.normal(SEED, name + ".v1", (B, D)).double()
    v2 = synth.normal(SEED, name + ".v2", (B, D)).double()
    p1 = torch.empty(B, D, dtype=torch.float64)
    p2 = torch.empty(B, D, dtype=torch.float64)
    q0 = queue0.double()
    for i in range(B):
        if i % 4 == 1:
            lean1, lean2, w = g2[(i + 1) % B], g1[(i + 1) % B], 0.7
        elif i % 4 == 2:
            lean1 = lean2 = q0[:, (7 * i + 3) % Q]
            w = 0.7
        else:
            lean1, lean2, w = v1[i], v2[i], 0.0
        # the head normalises the rows: any positive row scale
        p1[i] = (0.5 + i % 5) * _at_cosine(g2[i], lean1, v1[i], planted(i, k), w)
        p2[i] = (0.5 + (i + 2) % 5) * _at_cosine(g1[i], lean2, v2[i], planted(i + 4, k), w)
    ids = torch.arange(B, dtype=torch.int64) * 7 + 1000 * k
    gout1 = synth.normal(SEED, name + ".go1", (B, Q))
    gout2 = synth.normal(SEED, name + ".go2", (B, Q))
    return p1.float(), (1.5 * g2).float(), p2.float(), (0.75 * g1).float(), ids, gout1, gout2


def window_cos64(p, g):
    """Float64 cosines [B, B] of the probe rows against the gallery rows."""
    p, g = p.double(), g.double()
    return (p / p.norm(dim=1, keepdim=True)) @ (g / g.norm(dim=1, keepdim=True)).t()


def assert_covers(p1, g2, p2, g1):
    """Every target cosine lies in [0.2, 0.95] (so none within 1e-3 of +-1) and, where the batch has the rows that plant
    one (B >= 3), a negative inside the window reaches 0.4.  Returns the statistics."""
    st = {}
    for name, p, g in (("1", p1, g2), ("2", p2, g1)):
        c = window_cos64(p, g)
        t = c.diag()
        off = c - torch.diag_embed(t)
        st["t" + name] = t
        st["neg" + name] = float(off.max())
        assert float(t.min()) >= 0.2 - 1e-6 and float(t.max()) <= 0.95 + 1e-6, (name, t)
        assert float((1 - t.abs()).min()) >= 1e-3, (name, t)
        if p.shape[0] >= 3:
            assert st["neg" + name] >= 0.4, (name, st["neg" + name])
    return st


def sqrt_rn(t):
    """The correctly rounded square root of a host tensor (numpy's; not differentiable).  ``torch.sqrt`` of float32 host
    tensors is a vectorised approximation that is an ulp off in about 6 elements of 1000, so a bit-for-bit statement of
    "every operation rounded to fp32 on its own" takes its root here."""
    with np.errstate(invalid="ignore"):
        return torch.from_numpy(np.sqrt(t.detach().numpy()))


def from_cos(c, label, loss_type, margin, scale, sqrt=torch.sqrt):
    """The head's logits from cosines [rows, Q] that already have the window substituted, in c's dtype and in the reference's
    operation order (head/metrics.py:654-666, :701-702); differentiable in ``c``.  Margin scalars are rounded to c's dtype
    as torch rounds a Python scalar.  ``sqrt``: the square root to use (``sqrt_rn`` for a bit-for-bit fp32 statement)."""
    c = c.clamp(-1, 1)
    at = label.view(-1, 1)
    if loss_type == "am_softmax":
        c = c.scatter(1, at, c.gather(1, at) - margin)
    elif loss_type == "arc_softmax":
        gt = c.gather(1, at)
        sin_theta = sqrt(1.0 - torch.pow(gt, 2))
        c = c.scatter(1, at, gt * math.cos(margin) - sin_theta * math.sin(margin))
    return c * scale


def reference64(queue, index, p1, g2, p2, g1, loss_type, margin, scale, gout1, gout2):
    """(output1, output2, gp1, gp2) in float64 from float32 inputs: the head's arithmetic restated on its own."""
    B = p1.shape[0]
    q = queue.double()
    label = torch.arange(B) + index
    outs, grads = [], []
    for p, g, go in ((p1, g2, gout1), (p2, g1, gout2)):
        p = p.double().clone().requires_grad_(True)
        gn = torch.nn.functional.normalize(g.double())
        qq = torch.cat([q[:, :index], gn.t(), q[:, index + B:]], 1)
        out = from_cos(torch.nn.functional.normalize(p) @ qq, label, loss_type, margin, scale)
        (gp,) = torch.autograd.grad(out, p, go.double())
        outs.append(out.detach())
        grads.append(gp)
    return outs[0], outs[1], grads[0], grads[1]
