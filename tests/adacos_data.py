"""Inputs for the AdaCos tests and for tests/golden/make_golden_adacos.py (which imports this file, so the fixture and the
tests cannot build different data), and the float64 statistics both assert on.

AdaCos moves its scale by ``log(B_avg) / cos(min(pi/4, median(theta_target)))``.  Random embeddings have target angles near
pi/2, so they only ever take the pi/4 side of the ``min``.  ``built`` therefore constructs the batch: W = 0.05 * randn
[N, D], distinct labels, and ``n_close`` rows placed at the angles ``linspace(0.2, 0.7, n_close)`` from their class
direction (norms 5 .. 11); the other rows are random (angle ~1.55).  The close rows sit at shuffled row indices, so the
order statistic is not the row order.  With B = 8 and six close rows the ascending angles are 0.2 .. 0.7, ~1.55, ~1.55: the
lower median is 0.5, the upper 0.6, both below pi/4 -- a head that takes the upper median, or the mean of the two, or the
mean of per-rank medians, is told apart.
"""
import math

import torch

SEED = 20


def distinct_labels(synth, tag, B, N):
    """B distinct labels in [0, N): a seeded start and the stride 37 (coprime to every N in use)."""
    assert B <= N and N % 37 != 0
    start = int(synth.labels(SEED, tag + ".y", 1, N)[0])
    return (start + 37 * torch.arange(B, dtype=torch.int64)) % N


def random_case(synth, tag, B, D, N, w_tag=None):
    """(x, W [N, D], label, gout [B, N]): plain random data; every target angle is near pi/2."""
    x = synth.normal(SEED, tag + ".x", (B, D))
    W = synth.normal(SEED, (w_tag or tag) + ".W", (N, D), std=0.05)
    return x, W, synth.labels(SEED, tag + ".y", B, N), synth.normal(SEED, tag + ".g", (B, N))


def built(synth, tag, B, D, N, n_close, w_tag=None):
    """(x, W [N, D], label, gout [B, N]) of the constructed case: ``n_close`` rows at linspace(0.2, 0.7, n_close) rad from
    their class direction, the rest random."""
    W = synth.normal(SEED, (w_tag or tag) + ".W", (N, D), std=0.05).double()
    label = distinct_labels(synth, tag, B, N)
    v = synth.normal(SEED, tag + ".v", (B, D)).double()
    slot = torch.argsort(synth.uniform(SEED, tag + ".perm", (B,)))  # row i takes the slot[i]-th angle
    ang = torch.linspace(0.2, 0.7, n_close, dtype=torch.float64)
    x = torch.empty(B, D, dtype=torch.float64)
    for i in range(B):
        k = int(slot[i])
        if k >= n_close:
            x[i] = v[i]
            continue
        u = W[label[i]] / W[label[i]].norm()
        w = v[i] - (v[i] @ u) * u
        x[i] = (5.0 + k % 7) * (math.cos(ang[k]) * u + math.sin(ang[k]) * w / w.norm())
    return x.float(), W.float(), label, synth.normal(SEED, tag + ".g", (B, N))


CASES = ("rand", "built_even", "built_odd", "traj")


def batches(synth, tag, D=512, N=100):
    """[(name, (x, W, label, gout), branch, mid_gap)]: the calls of a fixture case, in order."""
    if tag == "rand":
        return [(tag, random_case(synth, tag, 8, D, N), "pi4", False)]
    if tag == "built_even":
        return [(tag, built(synth, tag, 8, D, N, 6), "median", True)]
    if tag == "built_odd":
        return [(tag, built(synth, tag, 7, D, N, 5), "median", False)]
    assert tag == "traj"
    return [("traj.%d" % i, built(synth, "traj.%d" % i, 8, D, N, 6, w_tag="traj"), "median", True) for i in range(3)]


def scale0(N):
    return math.sqrt(2) * math.log(N - 1)


def stats64(x, W, label, scale_old):
    """Float64 statistics of one AdaCos call from ``scale_old``: B_avg, the ascending target angles, the lower median, the
    two middle angles' distance (even counts; inf for odd ones), the branch of the ``min`` and the new scale."""
    x, W = x.double(), W.double()
    c = torch.nn.functional.normalize(x) @ torch.nn.functional.normalize(W).t()
    B = c.shape[0]
    hot = torch.zeros_like(c).scatter_(1, label.view(-1, 1), 1.0).bool()
    b_avg = float(torch.exp(float(scale_old) * c).masked_fill(hot, 0.0).sum() / B)
    th = torch.sort(torch.acos(c[hot].clamp(-1 + 1e-7, 1 - 1e-7))).values
    med = float(th[(B - 1) // 2])
    assert med == float(torch.median(th))
    gap = float(th[B // 2] - th[(B - 1) // 2]) if B % 2 == 0 else float("inf")
    return dict(b_avg=b_avg, theta_med=med, upper_med=float(th[B // 2]), mid_gap=gap,
                branch="median" if med < math.pi / 4 else "pi4",
                scale=math.log(b_avg) / math.cos(min(math.pi / 4, med)), max_exp_arg=float(scale_old) * float(c.max()))


def assert_covers(x, W, label, scale_old, branch, mid_gap=False):
    """The branch of ``min(pi/4, theta_med)`` the case is built for, at least 0.05 rad away from the other; ``mid_gap``:
    the two middle angles of an even batch are at least 0.05 rad apart, both on the median side (lower and upper median
    give different scales).  exp stays far from fp32 overflow.  Returns the statistics."""
    st = stats64(x, W, label, scale_old)
    assert st["branch"] == branch, st
    assert abs(st["theta_med"] - math.pi / 4) >= 0.05, st
    if mid_gap:
        assert x.shape[0] % 2 == 0 and st["mid_gap"] >= 0.05 and st["upper_med"] < math.pi / 4 - 0.05, st
    assert st["max_exp_arg"] < 60, st
    return st
