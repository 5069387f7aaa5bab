"""Inputs for the MagFace tests and for tests/golden/make_golden_magface.py (which imports this file, so the fixture and the
tests cannot build different data), and the float64 statistics both assert on.

Random embeddings have norms of ~sqrt(D) (inside [l_a, u_a] at D = 512) and target cosines of ~0 (the margin branch), so
they reach neither the clamp of the magnitude nor the ``c - margin_am`` branch.  ``built`` therefore constructs the batch:
  * rows with i % 4 != 3 cycle through the three norm regimes (i % 3: 0.6 / 0.9 l_a, inside at 20 / 50 / 80 % of the way
    from l_a to u_a, 1.2 / 1.5 u_a) and lie at a target cosine of -0.5 .. 0.9 with their class column: above
    cos(pi - m(a)) <= -0.69 for every margin in use, the cos(theta + m(a)) branch;
  * rows with i % 4 == 3 lie near the NEGATIVE of their class column (target cosine -0.97): the ``c - margin_am`` branch.
    Their norms alternate between 80 % of the way from l_a to u_a and 1.3 u_a, where m(a) >= 0.54 for both parameter sets
    of the fixture and cos(pi - m(a)) >= -0.86 is well away from -0.97 (at m = 0.3 the boundary, -0.955, is not);
  * every other column is an ordinary negative (|cosine| < 0.3).
No target cosine lies within 0.05 of its row's branch boundary, none has |c| > 0.99 and no norm lies within 1 % of l_a or
u_a, so fp32 and float64 runs take the same branches and the same side of the clamp.
"""
import math

import torch

SEED = 19
DEFAULTS = dict(margin_am=0.0, scale=32, l_a=10, u_a=110, l_margin=0.45, u_margin=0.8, lamda=20)


def params(**kw):
    return dict(DEFAULTS, **kw)


def random_case(synth, tag, B, D, N):
    """(x, weight [D, N], label, gout [B, N], gg [B, 1]): plain random data, every row inside and in the margin branch."""
    x = synth.normal(SEED, tag + ".x", (B, D))
    k = synth.normal(SEED, tag + ".k", (D, N), std=0.01)
    return (x, k, synth.labels(SEED, tag + ".y", B, N), synth.normal(SEED, tag + ".g", (B, N)),
            synth.normal(SEED, tag + ".gg", (B, 1)))


def built(synth, tag, B, D, N, g_std=1.0, l_a=10, u_a=110, **_unused):
    """(x, weight [D, N], label, gout [B, N], gg [B, 1]) of the constructed case."""
    k = synth.normal(SEED, tag + ".k", (D, N), std=0.01).double()
    label = synth.labels(SEED, tag + ".y", B, N)
    v = synth.normal(SEED, tag + ".v", (B, D)).double()
    x = torch.empty(B, D, dtype=torch.float64)
    for i in range(B):
        u = k[:, label[i]] / k[:, label[i]].norm()
        if i % 4 == 3:
            c = -0.97
            nrm = (l_a + 0.8 * (u_a - l_a)) if (i // 4) % 2 else 1.3 * u_a
        else:
            c = -0.5 + 1.4 * ((i * 5) % 8) / 7.0
            j = i // 3
            nrm = ((0.6 + 0.3 * (j % 2)) * l_a, l_a + (0.2 + 0.3 * (j % 3)) * (u_a - l_a), (1.2 + 0.3 * (j % 2)) * u_a)[i % 3]
        w = v[i] - (v[i] @ u) * u
        x[i] = nrm * (c * u + math.sqrt(1 - c * c) * w / w.norm())
    return (x.float(), k.float(), label, synth.normal(SEED, tag + ".g", (B, N), std=g_std),
            synth.normal(SEED, tag + ".gg", (B, 1)))


def stats64(x, k, label, l_a=10, u_a=110, l_margin=0.45, u_margin=0.8, **_unused):
    """Float64 statistics of a batch: rows below / inside / above [l_a, u_a], rows in the margin branch and in the fallback
    branch, inside rows in the margin branch, and the safety margins (smallest distance of a target cosine from its branch
    boundary, largest |target cosine|, smallest relative distance of a norm from l_a or u_a, largest |negative cosine|)."""
    x, k = x.double(), k.double()
    nrm = x.norm(dim=1)
    a = nrm.clamp(l_a, u_a)
    m = (u_margin - l_margin) / (u_a - l_a) * (a - l_a) + l_margin
    c = (torch.nn.functional.normalize(x) @ torch.nn.functional.normalize(k, dim=0)).clamp(-1, 1)
    tl = c.gather(1, label.view(-1, 1)).view(-1)
    first = tl > torch.cos(math.pi - m)
    inside = (nrm >= l_a) & (nrm <= u_a)
    neg = c.scatter(1, label.view(-1, 1), 0.0)
    return dict(below=int((nrm < l_a).sum()), inside=int(inside.sum()), above=int((nrm > u_a).sum()),
                margin_rows=int(first.sum()), fallback_rows=int((~first).sum()), inside_margin_rows=int((inside & first).sum()),
                boundary_gap=float((tl - torch.cos(math.pi - m)).abs().min()), max_abs_tl=float(tl.abs().max()),
                norm_gap=float(torch.minimum((nrm / l_a - 1).abs(), (nrm / u_a - 1).abs()).min()),
                max_abs_neg=float(neg.abs().max()))


def assert_covers(x, k, label, **p):
    """The coverage and the safety margins ``built`` promises; returns the statistics."""
    st = stats64(x, k, label, **p)
    assert st["below"] > 0 and st["inside"] > 0 and st["above"] > 0, st
    assert st["margin_rows"] > 0 and st["fallback_rows"] > 0 and st["inside_margin_rows"] > 0, st
    assert st["boundary_gap"] >= 0.05 and st["max_abs_tl"] <= 0.99 and st["norm_gap"] >= 0.01, st
    assert st["max_abs_neg"] < 0.3, st  # ordinary negatives
    return st
