"""Inputs for the CircleLoss / AM_Softmax tests and for tests/golden/make_golden_circle.py (which imports this file, so the
fixture and the tests cannot build different data), the float64 statistics both assert on, and ``from_cos``, the two heads'
arithmetic and its derivative from a given raw cosine matrix (for the tests of the C entry points).

Both heads (reference head/metrics.py:435-473 and :371-392) are element-wise on the clamped cosines c between normalised
embeddings and normalised weight columns.  CircleLoss: gamma * alpha_p * (c - delta_p) on the label column, gamma * alpha_n *
(c - delta_n) off it, alpha_p = max(O_p - c, 0) and alpha_n = max(c - O_n, 0) detached, O_n = -margin.  Random 512-dimensional
embeddings have |c| ~ 0.05: no negative comes near O_n = -0.25 and the ``clamp_min`` never acts.  ``built`` is the
construction of tests/mv_softmax_data.py with four kinds of row, by i % 4:
  0: near its own class column (target cosine 0.86 .. 0.94), nothing planted;
  1: the same, and three weight columns (classes that are nobody's label) are moved to a cosine of O_n - 0.10 (a dead
     negative: logit 0, gradient 0), O_n + 0.05 (barely alive) and +0.6 (a strong negative) with that row;
  2: target cosine -0.30 / -0.32 (a far-off positive: alpha_p above 1.5);
  3: target cosine 0.04 / 0.06, as on random data.
The logit and its slope are continuous at c = O_n, so nothing has to keep a distance from the hinge.  AM_Softmax takes the
same batch (O_n = -margin places the planted columns; the head has no hinge).
"""
import math

import torch

SEED = 23
HEADS = ("circle", "am")
DEFAULTS = {"circle": (0.25, 256.0), "am": (0.35, 32.0)}  # (margin, gamma) and (margin, scale)


def cosines64(x, k):
    return torch.nn.functional.normalize(x.double()) @ torch.nn.functional.normalize(k.double(), dim=0)


def random_case(synth, tag, B, D, N):
    """(x, weight [D, N], label, gout): plain random data; no cosine comes near O_n."""
    x = synth.normal(SEED, tag + ".x", (B, D))
    k = synth.normal(SEED, tag + ".k", (D, N), std=0.01)
    label = synth.labels(SEED, tag + ".y", B, N)
    return x, k, label, synth.normal(SEED, tag + ".g", (B, N))


PLANTED = (-0.10, 0.05)  # offsets from O_n of the dead and of the barely alive planted negative
STRONG = 0.6             # the cosine of the third


def built(synth, tag, B, D, N, head, margin, g_std=1.0):
    """(x, weight [D, N], label, gout) of the constructed case; needs N >= 4 * B + 1.  ``head`` is "circle" or "am"; both
    get the same construction around O_n = -margin.  The labels are distinct (a drawn label that an earlier row has moves on
    to the next free class)."""
    assert head in HEADS and N >= 4 * B + 1
    o_n = -margin
    k = synth.normal(SEED, tag + ".k", (D, N), std=0.01).double()
    label = synth.labels(SEED, tag + ".y", B, N)
    seen = set()
    for i in range(B):
        while int(label[i]) in seen:
            label[i] = (int(label[i]) + 1) % N
        seen.add(int(label[i]))
    v = synth.normal(SEED, tag + ".v", (B, D)).double()
    r = synth.normal(SEED, tag + ".r", (B, 3, D)).double()
    pool = [j for j in range(N) if j not in seen]
    x = torch.empty(B, D, dtype=torch.float64)

    def unit_orthogonal(a, u):
        a = a - (a @ u) * u
        return a / a.norm()

    for i in range(B):
        u = k[:, label[i]] / k[:, label[i]].norm()
        if i % 4 == 3:
            a = 0.04 + 0.02 * ((i // 4) % 2)
        elif i % 4 == 2:
            a = -0.30 - 0.02 * ((i // 4) % 2)
        else:
            a = 0.86 + 0.08 * ((i * 5) % 8) / 7.0
        xh = a * u + math.sqrt(1 - a * a) * unit_orthogonal(v[i], u)
        x[i] = (0.5 + i % 5) * xh  # the heads normalise the rows
        if i % 4 == 1:
            for q, c in enumerate((o_n + PLANTED[0], o_n + PLANTED[1], STRONG)):
                j = pool[3 * i + q]
                k[:, j] = k[:, j].norm() * (c * xh + math.sqrt(1 - c * c) * unit_orthogonal(r[i, q], xh))
    return x.float(), k.float(), label, synth.normal(SEED, tag + ".g", (B, N), std=g_std)


def circle_constants(margin):
    """(O_p, O_n, delta_p, delta_n) as the reference's constructor forms them (:446-449), Python floats."""
    return 1 + margin, -margin, 1 - margin, margin


def from_cos(cos, label, head, margin=None, scale=None):
    """(out, d out / d cos, parts) of a head from a raw cosine matrix [B, N], in cos's dtype and in the reference's
    operation order (clamp; O_p - c, clamp_min, c - delta_p, the product, then * gamma; AM_Softmax: c - margin, * scale), the
    constants rounded to cos's dtype as torch rounds a Python scalar.  ``scale`` is CircleLoss's gamma.  d out / d cos is
    gamma * alpha (AM_Softmax: scale) where -1 <= cos <= 1, the closed interval on which torch.clamp passes gradient, else
    0 -- a NaN cosine too.  A row whose label lies outside [0, N) has no label column: every column is a negative.
    ``parts``: alpha (CircleLoss; ones for AM_Softmax), mask (the clamp's pass mask) and hot (the label columns)."""
    assert head in HEADS
    margin = DEFAULTS[head][0] if margin is None else margin
    scale = DEFAULTS[head][1] if scale is None else scale
    N = cos.shape[1]
    has = (label >= 0) & (label < N)
    hot = torch.zeros_like(cos, dtype=torch.bool).scatter_(1, label.clamp(0, N - 1).view(-1, 1), True) & has.view(-1, 1)
    c = cos.clamp(-1, 1)
    mask = (cos >= -1) & (cos <= 1)
    if head == "circle":
        o_p, o_n, delta_p, delta_n = circle_constants(margin)
        alpha = torch.where(hot, torch.clamp_min(o_p - c, min=0.), torch.clamp_min(c - o_n, min=0.))
        out = torch.where(hot, alpha * (c - delta_p), alpha * (c - delta_n)) * scale
    else:
        alpha = torch.ones_like(c)
        out = torch.where(hot, c - margin, c) * scale
    dout = torch.where(mask, alpha * scale, torch.zeros_like(c))
    return out, dout, dict(alpha=alpha, mask=mask, hot=hot)


def grad_from_cos(cos, label, g, head, margin=None, scale=None):
    """d loss / d cos for the upstream gradient g in autograd's operation order: (g * scale) * alpha, then the clamp's mask
    (a select: 0 where the clamp saturated or the cosine is NaN)."""
    scale = DEFAULTS[head][1] if scale is None else scale
    parts = from_cos(cos, label, head, margin, scale)[2]
    return torch.where(parts["mask"], (g * scale) * parts["alpha"], torch.zeros_like(g))


def stats64(x, k, label, margin):
    """Float64 statistics of one call: per row the target cosine ``gt`` and the number ``dead`` of negatives at or below
    O_n = -margin (CircleLoss's dead negatives), max |c|, and the rows that carry the three planted negatives (one below
    O_n - 0.05, one inside (O_n, O_n + 0.1), one within 0.02 of +0.6)."""
    c = cosines64(x, k)
    o_n = -margin
    hot = torch.zeros_like(c, dtype=torch.bool).scatter_(1, label.view(-1, 1), True)
    neg = ~hot
    gt = c.gather(1, label.view(-1, 1)).view(-1)
    planted = ((neg & (c < o_n - 0.05)).any(1) & (neg & (c > o_n) & (c < o_n + 0.1)).any(1)
               & (neg & ((c - STRONG).abs() < 0.02)).any(1))
    return dict(gt=gt, dead=(neg & (c <= o_n)).sum(1), max_abs_c=float(c.abs().max()), planted=planted,
                high=int(((gt > 0.85) & (gt < 0.95)).sum()), low=int(((gt > -0.35) & (gt < -0.25)).sum()))


def assert_covers(x, k, label, margin):
    """In float64: a row with a target cosine near +0.9 and one near -0.3, a row with the three planted negatives (dead,
    barely alive, near +0.6), and max |c| < 0.99 over the whole batch.  Returns the statistics."""
    st = stats64(x, k, label, margin)
    assert st["high"] > 0 and st["low"] > 0, st
    assert bool(st["planted"].any()), st
    assert int(st["dead"].sum()) > 0, st
    assert st["max_abs_c"] < 0.99, st["max_abs_c"]
    return st
