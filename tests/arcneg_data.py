"""Inputs for the ArcNegFace tests and for tests/golden/make_golden_arcnegface.py (which imports this file, so the fixture and
the tests cannot build different data), the float64 statistics both assert on, and ``from_cos``, the head's arithmetic from a
given raw cosine matrix (for the tests of the C entry points).

ArcNegFace (reference head/metrics.py:394-433) puts ``a = cos(acos(gt) + margin)`` on the label column where the row's target
cosine ``gt`` lies above ``thresh = cos(pi - margin)`` and ``gt - mm`` where it does not, and turns every other column into
``t c + t - 1`` with ``t = alpha exp(-(c - a)^2 / sigma)`` a constant of the graph.  Random embeddings have gt ~ 0: the acos
branch alone.  ``built`` plants the target cosines, by i % 4:
  0: gt 0.9;   1: gt 0.3;   2: gt -0.5: the acos branch at three angles;
  3: gt just below ``thresh`` (-0.9476 / -0.9526 at margin 0.5, near -0.95; -0.97 / -0.975 at a margin below 0.43, whose
     thresh lies lower): the linear branch.
No target cosine comes within 1e-3 of ``thresh`` or beyond +-0.98, so fp32 and float64 runs take the same branches and stay
away from the poles of acos' derivative.
"""
import math

import torch

SEED = 24
ALPHA, SIGMA = 1.2, 2


def thresh_of(margin):
    return math.cos(math.pi - margin)


def cos64(x, w):
    """The float64 cosines of x [B, D] against the rows of w [N, D]."""
    x, w = x.double(), w.double()
    return (x / x.norm(dim=1, keepdim=True)) @ (w / w.norm(dim=1, keepdim=True)).t()


def random_case(synth, tag, B, D, N):
    """(x, weight [N, D], label, gout): plain random data, every row on the acos branch (gt ~ N(0, 1/D))."""
    x = synth.normal(SEED, tag + ".x", (B, D))
    w = synth.normal(SEED, tag + ".w", (N, D), std=0.01)
    label = synth.labels(SEED, tag + ".y", B, N)
    return x, w, label, synth.normal(SEED, tag + ".g", (B, N))


def planted(i, margin):
    """The target cosine planted in row i."""
    if i % 4 == 3:
        return max(thresh_of(margin) - 0.07, -0.97) - 0.005 * ((i // 4) % 2)
    return (0.9, 0.3, -0.5)[i % 4] + 0.01 * ((i // 4) % 3)


def built(synth, tag, B, D, N, margin=0.5, g_std=1.0):
    """(x, weight [N, D], label, gout) of the constructed case: row i lies at the cosine ``planted(i, margin)`` from its
    class's weight row.  The labels are distinct where N allows (a drawn label that an earlier row has moves on to the next
    free class)."""
    w = synth.normal(SEED, tag + ".w", (N, D), std=0.01)
    label = synth.labels(SEED, tag + ".y", B, N)
    seen = set()
    for i in range(B):
        while N >= B and int(label[i]) in seen:
            label[i] = (int(label[i]) + 1) % N
        seen.add(int(label[i]))
    v = synth.normal(SEED, tag + ".v", (B, D)).double()
    x = torch.empty(B, D, dtype=torch.float64)
    for i in range(B):
        u = w[label[i]].double()
        u = u / u.norm()
        o = v[i] - (v[i] @ u) * u
        g = planted(i, margin)
        x[i] = (0.5 + i % 5) * (g * u + math.sqrt(1 - g * g) * o / o.norm())  # the head normalises the rows
    return x.float(), w, label, synth.normal(SEED, tag + ".g", (B, N), std=g_std)


def from_cos(cos, label, margin=0.5, alpha=ALPHA, sigma=SIGMA, scale=64.0, thresh=None):
    """(logits, row values) of the head from a raw cosine matrix [B, N] in cos's dtype, differentiable in ``cos``; nothing is
    clamped.  The branch is taken as the reference takes it: the value of gt, as a double, against the double ``thresh``
    (cos(pi - margin) unless given).  t, the a inside it and the branch are constants of the graph.  A row whose label lies
    outside [0, N) has no target: gt = a = 0, t = 1 (the reference's initial values) and its logits are scale * c.  Row
    values, [B] each: gt, a (a function of gt in the graph), branch (bool: the acos branch)."""
    c = cos
    N = c.shape[1]
    thresh = thresh_of(margin) if thresh is None else thresh
    mm = math.sin(math.pi - margin) * margin
    has = (label >= 0) & (label < N)
    at = label.clamp(0, N - 1).view(-1, 1)
    hot = torch.zeros_like(c, dtype=torch.bool).scatter_(1, at, True) & has.view(-1, 1)
    zero = torch.zeros_like(c[:, 0])
    gt = torch.where(has, c.gather(1, at).view(-1), zero)
    branch = has & (gt.detach().double() > thresh)
    arc = torch.cos(torch.acos(torch.where(branch, gt, zero)) + margin)  # the other rows: acos' derivative stays finite
    a = torch.where(has, torch.where(branch, arc, gt - mm), zero)
    t = (alpha * torch.exp(-torch.pow(c - a.view(-1, 1), 2) / sigma)).detach()
    body = torch.where(has.view(-1, 1), t * c + t - 1, c)
    out = torch.where(hot, a.view(-1, 1), body) * scale
    return out, dict(gt=gt, a=a, branch=branch)


def stats64(x, w, label, margin):
    """Float64 row values of one call: gt, a and the branch per row, and the smallest |gt - thresh| and largest |gt|."""
    _, rv = from_cos(cos64(x, w), label, margin)
    gt = rv["gt"]
    return dict(gt=gt, a=rv["a"], branch=rv["branch"], gap=float((gt - thresh_of(margin)).abs().min()),
                max_abs_gt=float(gt.abs().max()))


def assert_covers(x, w, label, margin):
    """Both branches occur, every target cosine is at least 1e-3 from ``thresh`` (no fp32 run can sit on the boundary) and
    at most 0.98 in magnitude.  Returns the statistics."""
    st = stats64(x, w, label, margin)
    assert bool(st["branch"].any()) and not bool(st["branch"].all()), st["branch"]
    assert st["gap"] >= 1e-3, st["gap"]
    assert st["max_abs_gt"] <= 0.98, st["max_abs_gt"]
    return st
