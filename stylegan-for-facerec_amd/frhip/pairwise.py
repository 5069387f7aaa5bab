"""Threshold tallies over all pairwise cosine scores of one set of embeddings (``fr_pair_counts``).

The RB-WebFace protocol (rb-webface/scripts/test_RB_Webface.py) needs, per ethnic group and per threshold, two integers:
how many impostor pairs score ABOVE the threshold (``calc_FMR``) and how many genuine pairs score BELOW it (``calc_FNMR``).
The reference forms the full M x M float64 cosine matrix on the host once per threshold; here one pass over the upper
triangle on the f32-input MFMA tallies every threshold at once and only the counts leave the chip.

    counts, pairs_seen = pair_counts(emb, thresholds)            # all pairs i < j,            score > t
    counts, pairs_seen = pair_counts(emb, thresholds, group=5)   # pairs inside a group of 5,  score < t

Scores are fp32 (the reference's are float64): a score within 2**-13 of a threshold may fall on the other side, see
DESIGN.md section 7a for the bound.  A row of norm zero has NaN scores in the reference (scipy's cosine); here its row is
set to NaN after the normalisation, so its pairs are in ``pairs_seen`` and in no tally as well.
"""
import numpy as np
import torch

from . import ops
from ._lib import FR_F32, FrhipError, lib

MAX_T = 32  # thresholds per launch (fr_pair_counts)


def pairs_in(m, group=None):
    """Number of pairs the tallies run over: M (M - 1) / 2, or the pairs inside consecutive groups of ``group`` rows (a
    short last group has the pairs it has)."""
    m = int(m)
    if group is None:
        return m * (m - 1) // 2
    g = int(group)
    full, rest = divmod(m, g)
    return full * (g * (g - 1) // 2) + rest * (rest - 1) // 2


def pair_counts(emb, thresholds, group=None):
    """``emb``: fp32 [M, D] on a ROCm device (rows need not be normalised).  ``thresholds``: sequence / array / tensor of T
    values.  Returns ``(counts, pairs_seen)``: int64 [T] on the device and a Python int.  Nothing here waits for the GPU;
    the caller synchronises when it reads ``counts``."""
    if not isinstance(emb, torch.Tensor) or not emb.is_cuda:
        raise FrhipError("frhip.pair_counts: expected a ROCm device tensor -- the HIP path has no CPU fallback")
    if emb.dim() != 2 or emb.dtype != torch.float32:
        raise FrhipError("frhip.pair_counts: expected fp32 [M, D], got %s %s" % (emb.dtype, tuple(emb.shape)))
    M, D = emb.shape
    mode = 0 if group is None else 1
    g = 0 if group is None else int(group)
    parts = int(lib.fr_pair_counts_parts(M, mode, g))
    if parts < 0:
        msg = lib.fr_last_error_string()
        raise FrhipError("frhip.pair_counts: %s" % (msg.decode() if msg else "unsupported argument"))
    dev = emb.device
    st = ops.current_stream_ptr()
    if isinstance(thresholds, torch.Tensor):
        thr = thresholds.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    else:
        thr = torch.from_numpy(np.asarray(thresholds, dtype=np.float64).astype(np.float32).reshape(-1))
        thr = thr.pin_memory().to(dev, non_blocking=True)
    T = thr.numel()
    if T < 1:
        raise FrhipError("frhip.pair_counts: at least one threshold")
    x = emb.contiguous()
    xn = torch.empty(M, D, device=dev)
    inv = torch.empty(M, device=dev)
    ops.call("fr_row_normalize", x, xn, None, inv, M, M, D, 0, FR_F32, st)()
    # fr_row_normalize leaves a zero row zero (inv = 1 / eps = 1e12); the reference divides 0 by 0 there
    xn.masked_fill_(~(inv < 1e11).unsqueeze(1), float("nan"))
    counts = torch.empty(T, dtype=torch.int64, device=dev)
    partials = torch.empty(parts * min(T, MAX_T), dtype=torch.int32, device=dev)  # uint32 to the kernel
    for t0 in range(0, T, MAX_T):
        n = min(MAX_T, T - t0)
        ops.call("fr_pair_counts", xn, D, M, D, thr[t0:t0 + n], n, mode, g, partials, counts[t0:t0 + n], st)()
    return counts, pairs_in(M, group)
