"""Inputs for the MV_Softmax tests and for tests/golden/make_golden_mv_softmax.py (which imports this file, so the fixture and
the tests cannot build different data), the float64 statistics both assert on, and ``from_cos``, the head's arithmetic from a
given raw cosine matrix (for the tests of the C entry points).

MV_Softmax (reference head/metrics.py:555-590) lifts the negatives above a per-row threshold ``thr`` to ``w c + w - 1`` and
puts a margin on the label column; ``thr`` and the label column's value depend on the row's target cosine ``gt`` alone, by one
of two rules (``is_am``: thr = gt - margin, the margin applied where gt > margin; otherwise thr = cos(theta + margin), applied
where gt > 0).  Random embeddings have gt ~ 0 and make every negative hard.  ``built`` is the construction of
tests/npcface_data.py with four kinds of row, by i % 4:
  0: near its own class column (gt 0.86 .. 0.94), nothing planted: the ordinary negatives (|c| < 0.3) lie below thr, no
     negative is hard;
  1: the same, and three weight columns (classes that are nobody's label) are moved to a cosine of thr + 0.05, thr + 0.10 and
     thr - 0.05 with that row: two hard negatives, and one easy negative well above the bulk;
  2: gt = 0.04 / 0.06, so 0 < gt < margin: the AM form's ``gt > margin`` and the arc form's ``gt > 0`` disagree here, and
     every negative is hard;
  3: near the NEGATIVE of its class column (gt = -0.97 / -0.98): the ``gt <= 0`` branch, and every negative is hard.
No cosine comes near a decision boundary (c == thr, gt == 0, gt == margin), so fp32 and float64 runs take the same branches.
"""
import math

import torch

SEED = 22


def target_cos64(x, k, label):
    c = torch.nn.functional.normalize(x.double()) @ torch.nn.functional.normalize(k.double(), dim=0)
    return c.gather(1, label.view(-1, 1)).view(-1)


def random_case(synth, tag, B, D, N):
    """(x, weight [D, N], label, gout): plain random data, every negative hard.  The data are those of the first of the
    tags ``tag``, ``tag.1``, ``tag.2`` .. on which every target cosine has |gt| >= 1e-3 (the ``gt > 0`` branch must not hang
    on fp32 rounding; a random target cosine is ~N(0, 1/D))."""
    for n in range(64):
        tg = tag + (".%d" % n if n else "")
        x = synth.normal(SEED, tg + ".x", (B, D))
        k = synth.normal(SEED, tg + ".k", (D, N), std=0.01)
        label = synth.labels(SEED, tg + ".y", B, N)
        if float(target_cos64(x, k, label).abs().min()) >= 1e-3:
            break
    assert float(target_cos64(x, k, label).abs().min()) >= 1e-3, tag
    return x, k, label, synth.normal(SEED, tg + ".g", (B, N))


def threshold(gt, is_am, margin):
    """thr of a target cosine (a Python float), in double."""
    if is_am:
        return gt - margin
    return gt * math.cos(margin) - math.sqrt(1 - gt * gt) * math.sin(margin)


def built(synth, tag, B, D, N, is_am, margin, g_std=1.0):
    """(x, weight [D, N], label, gout) of the constructed case; needs N >= 4 * B + 1.  The labels are distinct (a drawn
    label that an earlier row has moves on to the next free class): two rows near one class column would see each other's
    planted columns at a cosine near their own thr."""
    assert N >= 4 * B + 1
    k = synth.normal(SEED, tag + ".k", (D, N), std=0.01).double()
    label = synth.labels(SEED, tag + ".y", B, N)
    seen = set()
    for i in range(B):
        while int(label[i]) in seen:
            label[i] = (int(label[i]) + 1) % N
        seen.add(int(label[i]))
    v = synth.normal(SEED, tag + ".v", (B, D)).double()
    r = synth.normal(SEED, tag + ".r", (B, 3, D)).double()
    taken = set(label.tolist())
    pool = [j for j in range(N) if j not in taken]
    x = torch.empty(B, D, dtype=torch.float64)

    def unit_orthogonal(a, u):
        a = a - (a @ u) * u
        return a / a.norm()

    for i in range(B):
        u = k[:, label[i]] / k[:, label[i]].norm()
        if i % 4 == 3:
            a = -0.97 - 0.01 * ((i // 4) % 2)
        elif i % 4 == 2:
            a = 0.04 + 0.02 * ((i // 4) % 2)
        else:
            a = 0.86 + 0.08 * ((i * 5) % 8) / 7.0
        xh = a * u + math.sqrt(1 - a * a) * unit_orthogonal(v[i], u)
        x[i] = (0.5 + i % 5) * xh  # the head normalises the rows
        if i % 4 == 1:
            thr = threshold(a, is_am, margin)
            for q, c in enumerate((thr + 0.05, thr + 0.10, thr - 0.05)):
                j = pool[3 * i + q]
                k[:, j] = k[:, j].norm() * (c * xh + math.sqrt(1 - c * c) * unit_orthogonal(r[i, q], xh))
    return x.float(), k.float(), label, synth.normal(SEED, tag + ".g", (B, N), std=g_std)


def from_cos(cos, label, is_am, margin=0.35, w=1.12, s=32.0, cos_m=None, sin_m=None):
    """(logits, row values) of the head from a raw cosine matrix [B, N] in cos's dtype, differentiable in ``cos``; nothing
    is clamped.  ``cos_m`` / ``sin_m`` default to those of ``margin`` (the arc form reads them, not ``margin``).  A row whose
    label lies outside [0, N) has no target: gt = 0, thr = +inf, final = 0, nothing in it is hard and no column is selected.
    Row values, [B] each: gt, thr (detached), final (a function of gt in the graph), count (int64, hard negatives with the
    label column left out)."""
    c = cos
    N = c.shape[1]
    cos_m = math.cos(margin) if cos_m is None else cos_m
    sin_m = math.sin(margin) if sin_m is None else sin_m
    has = (label >= 0) & (label < N)
    at = label.clamp(0, N - 1).view(-1, 1)
    hot = torch.zeros_like(c, dtype=torch.bool).scatter_(1, at, True) & has.view(-1, 1)
    zero = torch.zeros_like(c[:, 0])
    gt = torch.where(has, c.gather(1, at).view(-1), zero)
    if is_am:
        thr = gt - margin
        final = torch.where(gt > margin, gt - margin, gt)
    else:
        thr = gt * cos_m - torch.sqrt(1.0 - gt * gt) * sin_m
        final = torch.where(gt > 0, thr, gt)
    thr = torch.where(has, thr, torch.full_like(gt, float("inf"))).detach()
    final = torch.where(has, final, zero)
    hard = c > thr.view(-1, 1)  # NaN thr: nothing is hard
    out = torch.where(hot, final.view(-1, 1), torch.where(hard, w * c + w - 1.0, c)) * s
    return out, dict(gt=gt, thr=thr, final=final, count=(hard & ~hot).sum(1))


def stats64(x, k, label, is_am, margin):
    """Float64 statistics of one call: per row gt, thr and the hard count, the number of rows of each kind (``none``: gt >
    0.5 and no hard negative; ``planted``: gt > 0.5 and exactly two; ``small``: 0 < gt < margin and every negative hard;
    ``negative``: gt <= 0 and every negative hard), max |c|, the smallest distance of a non-target entry from its row's thr
    and the smallest distance of a gt from 0 and from ``margin``."""
    c = torch.nn.functional.normalize(x.double()) @ torch.nn.functional.normalize(k.double(), dim=0)
    _, rv = from_cos(c, label, is_am, margin)
    B, N = c.shape
    hot = torch.zeros_like(c, dtype=torch.bool).scatter_(1, label.view(-1, 1), True)
    gap = (c - rv["thr"].view(-1, 1)).abs().masked_fill(hot, float("inf"))
    gt, count = rv["gt"], rv["count"]
    return dict(gt=gt, thr=rv["thr"], count=count, none=int(((gt > 0.5) & (count == 0)).sum()),
                planted=int(((gt > 0.5) & (count == 2)).sum()),
                small=int(((gt > 0) & (gt < margin) & (count == N - 1)).sum()),
                negative=int(((gt <= 0) & (count == N - 1)).sum()), max_abs_c=float(c.abs().max()),
                min_gap=float(gap.min()), gt_gap=float(torch.minimum(gt.abs(), (gt - margin).abs()).min()))


KINDS = ("none", "planted", "small", "negative")


def assert_covers(x, k, label, is_am, margin):
    """All four kinds of row occur and between them make up the batch, max |c| <= 0.99, every non-target entry is at least
    1e-3 from its row's thr, and every gt is at least 0.03 from 0 and from ``margin``.  Returns the statistics."""
    st = stats64(x, k, label, is_am, margin)
    assert all(st[n] > 0 for n in KINDS) and sum(st[n] for n in KINDS) == x.shape[0], st
    assert st["max_abs_c"] <= 0.99, st["max_abs_c"]
    assert st["min_gap"] >= 1e-3, st["min_gap"]
    assert st["gt_gap"] >= 0.03, st["gt_gap"]
    return st
