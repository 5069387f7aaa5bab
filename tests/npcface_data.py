"""Inputs for the NPCFace tests and for tests/golden/make_golden_npcface.py (which imports this file, so the fixture and the
tests cannot build different data), the float64 statistics both assert on, and ``from_cos``, the head's arithmetic from a
given raw cosine matrix (for the tests of the C entry points).

NPCFace's margin on the label column is ``m0 + m1 * avg`` with ``avg`` the mean of the row's hard negatives (the cosines
above cos(theta_target + margin), label column excluded) and the count clamped at 1.  Random embeddings make every negative
hard and every ``avg`` ~0, so the margin never leaves ``m0``.  ``built`` is the construction of tests/curricular_data.py
with one change, and gives three kinds of row:
  * rows i with i % 4 == 3 lie near the NEGATIVE of their class column (target cosine -0.97 / -0.98): the ``gt <= 0``
    branch, and every negative of such a row is hard;
  * rows with i % 4 == 0 lie near their own class column (target cosine 0.86..0.94, cos(theta + margin) ~ 0.58) and get no
    planted column (the change): their ordinary negatives (|c| < 0.3) are easy, count = 0, the clamp of the count to 1;
  * the other rows lie near their class column too, and three kernel columns per such row (classes that are nobody's
    label) are moved to a cosine of 0.70 / 0.78 / 0.86 with that row: count = 3, avg ~ 0.78, a margin far from ``m0``.
No cosine comes near a decision boundary (c == ctm, gt == 0) or the clamp, so fp32 and float64 runs take the same branches.
"""
import math

import torch

SEED = 21


def target_cos64(x, k, label):
    c = torch.nn.functional.normalize(x.double()) @ torch.nn.functional.normalize(k.double(), dim=0)
    return c.gather(1, label.view(-1, 1)).view(-1)


def random_case(synth, tag, B, D, N):
    """(x, kernel [D, N], label, gout): plain random data, every negative hard.  The data are those of the first of the
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


def built(synth, tag, B, D, N, g_std=1.0):
    """(x, kernel [D, N], label, gout) of the constructed case; needs N >= 4 * B + 1."""
    assert N >= 4 * B + 1
    k = synth.normal(SEED, tag + ".k", (D, N), std=0.01).double()
    label = synth.labels(SEED, tag + ".y", B, N)
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
        else:
            a = 0.86 + 0.08 * ((i * 5) % 8) / 7.0
        xh = a * u + math.sqrt(1 - a * a) * unit_orthogonal(v[i], u)
        x[i] = (0.5 + i % 5) * xh  # the head normalises the rows
        if i % 4 in (1, 2):
            for q, c in enumerate((0.70, 0.78, 0.86)):
                j = pool[3 * i + q]
                k[:, j] = k[:, j].norm() * (c * xh + math.sqrt(1 - c * c) * unit_orthogonal(r[i, q], xh))
    return x.float(), k.float(), label, synth.normal(SEED, tag + ".g", (B, N), std=g_std)


def from_cos(cos, label, margin=0.5, m0=0.40, m1=0.20, t=1.10, a=0.20, s=64.0):
    """(logits, row values) of the head from a raw cosine matrix [B, N] in cos's dtype, differentiable in ``cos``.  A row
    whose label lies outside [0, N) has no target: gt = 0, ctm = +inf, nothing in it is hard and no column is selected.
    Row values, [B] each: gt, ctm, final (a function of gt in the graph), avg, count (int64)."""
    c = cos.clamp(-1, 1)
    N = c.shape[1]
    has = (label >= 0) & (label < N)
    at = label.clamp(0, N - 1).view(-1, 1)
    hot = torch.zeros_like(c, dtype=torch.bool).scatter_(1, at, True) & has.view(-1, 1)
    gt = torch.where(has, c.gather(1, at).view(-1), torch.zeros_like(c[:, 0]))
    sin_theta = torch.sqrt(1.0 - gt * gt)
    inf = torch.full_like(gt, float("inf"))
    ctm = torch.where(has, gt * math.cos(margin) - sin_theta * math.sin(margin), inf).detach()
    hard = (c > ctm.view(-1, 1)) & ~hot
    count = hard.sum(1)
    avg = (torch.where(hard, c, torch.zeros_like(c)).sum(1) / count.clamp(min=1)).detach()
    newm = m0 + m1 * avg
    final = torch.where(gt > 0, gt * torch.cos(newm) - sin_theta * torch.sin(newm), gt)
    out = torch.where(hot, final.view(-1, 1), torch.where(c > ctm.view(-1, 1), t * c + a, c)) * s
    return out, dict(gt=gt, ctm=ctm, final=final, avg=avg, count=count)


def stats64(x, k, label, margin):
    """Float64 statistics of one call: per row gt, count and avg, the number of rows of each kind (``negative``: gt <= 0
    and every negative hard; ``none``: gt > 0 and no hard negative; ``some``: gt > 0 and at least one), max |c| and the
    smallest distance of a non-target entry from its row's ctm."""
    c = torch.nn.functional.normalize(x.double()) @ torch.nn.functional.normalize(k.double(), dim=0)
    _, rv = from_cos(c, label, margin)
    B, N = c.shape
    hot = torch.zeros_like(c, dtype=torch.bool).scatter_(1, label.view(-1, 1), True)
    gap = (c - rv["ctm"].view(-1, 1)).abs().masked_fill(hot, float("inf"))
    gt, count = rv["gt"], rv["count"]
    return dict(gt=gt, count=count, avg=rv["avg"], negative=int(((gt <= 0) & (count == N - 1)).sum()),
                none=int(((gt > 0) & (count == 0)).sum()), some=int(((gt > 0) & (count > 0)).sum()),
                max_abs_c=float(c.abs().max()), min_gap=float(gap.min()))


def assert_covers(x, k, label, margin):
    """Each of the three kinds of row occurs, 0.05 <= |gt| <= 0.99, max |c| <= 0.99, and every non-target entry is at least
    1e-3 from its row's cos(theta + margin).  Returns the statistics."""
    st = stats64(x, k, label, margin)
    assert st["negative"] > 0 and st["none"] > 0 and st["some"] > 0, st
    assert 0.05 <= float(st["gt"].abs().min()) and float(st["gt"].abs().max()) <= 0.99, st["gt"]
    assert st["max_abs_c"] <= 0.99, st["max_abs_c"]
    assert st["min_gap"] >= 1e-3, st["min_gap"]
    return st
