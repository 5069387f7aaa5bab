"""Inputs for the CurricularFace tests and for tests/golden/make_golden_curricular.py (which imports this file, so the
fixture and the tests cannot build different data), and the float64 statistics both assert on.

Random embeddings make every negative "hard": their cosines are ~0 +- 0.05 while cos(theta_target + m) ~ -0.48 at a target
cosine of ~0.  ``built`` therefore constructs the batch:
  * rows i with i % 4 != 3 lie near their own class column: target cosine 0.86..0.94, cos(theta + m) ~ 0.58, so their
    ordinary negatives (|c| < 0.3) are easy;
  * three kernel columns per such row (classes that are nobody's label) are moved to a cosine of 0.70 / 0.78 / 0.86 with
    that row: hard negatives among easy ones;
  * rows with i % 4 == 3 lie near the NEGATIVE of their class column (target cosine -0.97 / -0.98, below cos(pi - m) for
    m = 0.5 and m = 0.3): the ``tl - mm`` branch, and every negative of such a row is hard.
All target cosines stay within |tl| <= 0.99, and no cosine comes near a decision boundary (c == ctm, tl == threshold) or the
clamp, so fp32 and float64 runs take the same branches.
"""
import math

import torch

SEED = 18


def random_case(synth, tag, B, D, N):
    """(x, kernel [D, N], label, gout): plain random data, every negative hard."""
    x = synth.normal(SEED, tag + ".x", (B, D))
    k = synth.normal(SEED, tag + ".k", (D, N), std=0.01)
    return x, k, synth.labels(SEED, tag + ".y", B, N), synth.normal(SEED, tag + ".g", (B, N))


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
        if i % 4 != 3:
            for q, c in enumerate((0.70, 0.78, 0.86)):
                j = pool[3 * i + q]
                k[:, j] = k[:, j].norm() * (c * xh + math.sqrt(1 - c * c) * unit_orthogonal(r[i, q], xh))
    return x.float(), k.float(), label, synth.normal(SEED, tag + ".g", (B, N), std=g_std)


def stats64(x, k, label, m):
    """(fraction of the non-target entries that are hard, number of rows in the cos(theta + m) branch, number in the
    tl - mm branch, max |tl|) in float64."""
    xn = torch.nn.functional.normalize(x.double())
    kn = torch.nn.functional.normalize(k.double(), dim=0)
    c = (xn @ kn).clamp(-1, 1)
    tl = c.gather(1, label.view(-1, 1))
    ctm = tl * math.cos(m) - torch.sqrt(1 - tl * tl) * math.sin(m)
    hard = c > ctm
    hard.scatter_(1, label.view(-1, 1), False)
    first = int((tl > math.cos(math.pi - m)).sum())
    return float(hard.double().sum() / (c.numel() - c.shape[0])), first, c.shape[0] - first, float(tl.abs().max())


def assert_covers_both_branches(x, k, label, m):
    frac, first, second, tmax = stats64(x, k, label, m)
    assert 0.10 <= frac <= 0.90, frac
    assert first > 0 and second > 0, (first, second)
    assert tmax <= 0.99, tmax
    return frac, first, second, tmax
