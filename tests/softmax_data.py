"""Inputs for the Softmax-head / cross-entropy tests and for tests/golden/make_golden_softmax.py (which imports this file, so
the fixture and the tests cannot build different data).

The Softmax head (reference head/metrics.py:12-63) is ``F.linear(x, weight, bias)``; the loss of LOSS_NAME 'Softmax' is
``nn.CrossEntropyLoss()`` on its logits.  x is uniform in [-1, 1); the weight is N(0, 0.2^2), so a logit is a sum of 512
products of standard deviation 0.2 / sqrt(3): about 2.6, and the largest of a few hundred lies near +-8; the bias is uniform
in [-1, 1) -- never zero, which would hide a missing bias.  One label is 0 and one is N - 1.
"""
import torch

SEED = 25
D = 512
CASES = ((6, 37), (8, 100))
W_STD = 0.2


def tag_of(B, N):
    return "sm_b%d_n%d" % (B, N)


def case(synth, B, N, d=D):
    """(x [B, d], weight [N, d], bias [N], label [B])."""
    tag = tag_of(B, N)
    x = synth.uniform(SEED, tag + ".x", (B, d))
    w = synth.normal(SEED, tag + ".w", (N, d), std=W_STD)
    b = synth.uniform(SEED, tag + ".b", (N,))
    label = synth.labels(SEED, tag + ".y", B, N)
    label[0], label[B - 1] = 0, N - 1
    return x, w, b, label


def gw_rows(label, N):
    """The rows of the weight gradient the fixture keeps: the labels of rows 0 .. 3 and the two lowest classes that are
    nobody's label (every class takes gradient through the softmax)."""
    taken = set(label.tolist())
    return torch.tensor(sorted(set(label[:4].tolist()) | set([j for j in range(N) if j not in taken][:2])))


def col_sums_in_row_order(g):
    """((g[0] + g[1]) + g[2]) + ... in the dtype of g: what fr_col_sums computes, as a torch loop."""
    acc = g[0].clone()
    for m in range(1, g.shape[0]):
        acc = acc + g[m]
    return acc
