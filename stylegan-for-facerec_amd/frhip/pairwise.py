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

The exact threshold at a chosen FPR is one order statistic of the impostor scores, found without storing them by a
three-pass radix select over histograms of the scores' integer keys (``fr_pair_hist``, the same fp32 scores bit for bit):

    hist, pairs_seen = pair_histogram(emb, key_lo, shift, bins)  # int64 [bins + 2]: below, the bins, above the window
    t, count_above = score_at_rank(emb, k)                       # the (k + 1)-th largest score, and how many exceed it
    t, achieved_fmr = threshold_at_fmr(emb, 1e-4)                # k = floor(fmr * pairs_seen)
"""
import math

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


def _unit_rows(emb, who, parts_fn, group):
    """The checks and the normalisation the entry points share: (xn fp32 [M, D] with NaN rows for zero rows, mode, g,
    rows of partials)."""
    if not isinstance(emb, torch.Tensor) or not emb.is_cuda:
        raise FrhipError("frhip.%s: expected a ROCm device tensor -- the HIP path has no CPU fallback" % who)
    if emb.dim() != 2 or emb.dtype != torch.float32:
        raise FrhipError("frhip.%s: expected fp32 [M, D], got %s %s" % (who, emb.dtype, tuple(emb.shape)))
    M, D = emb.shape
    mode = 0 if group is None else 1
    g = 0 if group is None else int(group)
    parts = int(parts_fn(M, mode, g))
    if parts < 0:
        msg = lib.fr_last_error_string()
        raise FrhipError("frhip.%s: %s" % (who, msg.decode() if msg else "unsupported argument"))
    x = emb.contiguous()
    xn = torch.empty(M, D, device=emb.device)
    inv = torch.empty(M, device=emb.device)
    ops.call("fr_row_normalize", x, xn, None, inv, M, M, D, 0, FR_F32, ops.current_stream_ptr())()
    # fr_row_normalize leaves a zero row zero (inv = 1 / eps = 1e12); the reference divides 0 by 0 there
    xn.masked_fill_(~(inv < 1e11).unsqueeze(1), float("nan"))
    return xn, mode, g, parts


def pair_counts(emb, thresholds, group=None):
    """``emb``: fp32 [M, D] on a ROCm device (rows need not be normalised).  ``thresholds``: sequence / array / tensor of T
    values.  Returns ``(counts, pairs_seen)``: int64 [T] on the device and a Python int.  Nothing here waits for the GPU;
    the caller synchronises when it reads ``counts``."""
    xn, mode, g, parts = _unit_rows(emb, "pair_counts", lib.fr_pair_counts_parts, group)
    M, D = xn.shape
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
    counts = torch.empty(T, dtype=torch.int64, device=dev)
    partials = torch.empty(parts * min(T, MAX_T), dtype=torch.int32, device=dev)  # uint32 to the kernel
    for t0 in range(0, T, MAX_T):
        n = min(MAX_T, T - t0)
        ops.call("fr_pair_counts", xn, D, M, D, thr[t0:t0 + n], n, mode, g, partials, counts[t0:t0 + n], st)()
    return counts, pairs_in(M, group)


# ---- score keys: an order-preserving map of the fp32 scores onto uint32 (pure host helpers; csrc/pair_hist.hip has the
# same three lines)
_SIGN = np.uint32(0x80000000)
KEY_NEG_INF, KEY_POS_INF = 0x007FFFFF, 0xFF800000  # keys outside [KEY_NEG_INF, KEY_POS_INF] belong to NaN bit patterns
SELECT_PASSES = ((21, 2048), (10, 2048), (0, 1024))  # (shift, bins): the 32 key bits split 11 / 11 / 10
MAX_BINS, MAX_SHIFT = 2048, 21


def score_key(scores):
    """float32 array -> uint32 keys with s1 < s2 <=> key1 < key2; -0 and +0 share a key.  Not meant for NaN (the kernel
    never keys one)."""
    s = np.ascontiguousarray(scores, dtype=np.float32)
    u = np.where(s == 0, np.uint32(0), s.view(np.uint32))
    return np.where(u & _SIGN, ~u, u | _SIGN).astype(np.uint32)


def key_score(keys):
    """The inverse of ``score_key``: uint32 keys -> float32."""
    k = np.ascontiguousarray(keys, dtype=np.uint32)
    return np.where(k & _SIGN, k & ~_SIGN, ~k).astype(np.uint32).view(np.float32)


def bin_edges(key_lo, shift, bins):
    """float32 [bins + 1]: edge b is the float whose key is ``key_lo + (b << shift)``, so bin b holds exactly the scores
    with ``edges[b] <= s < edges[b + 1]``.  An edge key below the key of -inf reads -inf and one above the key of +inf
    (2**32 included) reads +inf: no score lies beyond them."""
    k = int(key_lo) + (np.arange(int(bins) + 1, dtype=np.int64) << int(shift))
    return key_score(np.clip(k, KEY_NEG_INF, KEY_POS_INF).astype(np.uint32))


def pair_histogram(emb, key_lo, shift, bins, group=None):
    """Histogram of the pair scores of ``emb`` (fp32 [M, D] on a ROCm device; rows and NaN convention as for
    ``pair_counts``) by key: slot 0 counts the pairs whose key is below ``key_lo``, slot 1 + b those of bin b (width
    ``1 << shift`` keys, ``bins`` of them), slot ``bins + 1`` those above the window.  Returns ``(hist, pairs_seen)``: int64
    [bins + 2] on the device and a Python int; NaN scores are in ``pairs_seen`` and in no slot.  Does not synchronise."""
    xn, mode, g, parts = _unit_rows(emb, "pair_histogram", lib.fr_pair_hist_parts, group)
    return _hist_unit(xn, mode, g, parts, key_lo, shift, bins), pairs_in(xn.shape[0], group)


def _hist_unit(xn, mode, g, parts, key_lo, shift, bins):
    M, D = xn.shape
    key_lo, shift, bins = int(key_lo), int(shift), int(bins)
    if not 0 <= key_lo < 2 ** 32:
        raise FrhipError("frhip.pair_histogram: key_lo must fit 32 bits")
    hist = torch.empty(max(bins, 0) + 2, dtype=torch.int64, device=xn.device)
    partials = torch.empty(parts * (max(bins, 0) + 2), dtype=torch.int32, device=xn.device)  # uint32 to the kernel
    ops.call("fr_pair_hist", xn, D, M, D, key_lo, shift, bins, mode, g, partials, hist, ops.current_stream_ptr())()
    return hist


def select_rank(hist_fn, k):
    """The three-pass descent on its own.  ``hist_fn(key_lo, shift, bins)`` returns the int64 [bins + 2] histogram of the
    scores as an array; returns ``(score, count_above)``: the (k + 1)-th largest score as np.float32 and the number of
    scores strictly greater.  Each pass picks, counting from the top, the bin that holds rank k and the next pass
    histograms that bin alone; the overflow slot carries the count above it."""
    k = int(k)
    key_lo, above = 0, 0
    for n, (shift, bins) in enumerate(SELECT_PASSES):
        h = np.asarray(hist_fn(key_lo, shift, bins), dtype=np.int64)
        if h.shape != (bins + 2,):
            raise FrhipError("frhip.score_at_rank: a histogram of %d slots, expected %d" % (h.size, bins + 2))
        if n == 0:
            total = int(h.sum())
            if not 0 <= k < total:
                raise FrhipError("frhip.score_at_rank: rank k = %d, but there are %d pairs with a score" % (k, total))
        elif int(h[bins + 1]) != above or int(h[1:bins + 1].sum()) != inside:
            raise FrhipError("frhip.score_at_rank: pass %d sees %d scores above and %d inside the bin pass %d chose; expected "
                             "%d and %d" % (n + 1, int(h[bins + 1]), int(h[1:bins + 1].sum()), n, above, inside))
        ge = above + np.cumsum(h[1:bins + 1][::-1])[::-1]  # ge[b] = scores in bin b or above it
        b = int(np.nonzero(ge > k)[0][-1])                 # the highest bin with more than k scores at or above it
        above = int(ge[b] - h[1 + b])
        inside = int(h[1 + b])
        key_lo += b << shift
    return key_score(np.array([key_lo], np.uint32))[0], above


def scores_at_ranks(emb, ks, group=None):
    """``score_at_rank`` for several ranks: the rows are normalised once and a histogram is computed once per window, so
    the first pass (and every later pass two ranks share) is not repeated.  Returns a list of ``(score, count_above)``."""
    xn, mode, g, parts = _unit_rows(emb, "score_at_rank", lib.fr_pair_hist_parts, group)
    done = {}

    def hist(key_lo, shift, bins):
        if (key_lo, shift, bins) not in done:
            done[key_lo, shift, bins] = _hist_unit(xn, mode, g, parts, key_lo, shift, bins).cpu().numpy()
        return done[key_lo, shift, bins]

    return [select_rank(hist, k) for k in ks]


def score_at_rank(emb, k, group=None):
    """The exact (k + 1)-th largest pair score of ``emb`` (k = 0: the largest), as np.float32, and ``count_above``, the
    number of scores strictly greater than it (<= k; less where the score is tied).  Three ``fr_pair_hist`` passes, one
    read-back each; the scores are never stored.  Raises if k is not smaller than the number of non-NaN pairs."""
    return scores_at_ranks(emb, [k], group)[0]


def thresholds_at_fmr(emb, fmrs):
    """``threshold_at_fmr`` for several FMRs, sharing the normalisation and the common passes."""
    seen = pairs_in(emb.shape[0])
    ranks = scores_at_ranks(emb, [int(math.floor(float(f) * seen)) for f in fmrs])
    return [(t, above / seen) for t, above in ranks]


def threshold_at_fmr(emb, fmr):
    """``(threshold, achieved_fmr)``: the smallest score t with at most k = floor(fmr * pairs_seen) impostor pairs above
    it, where pairs_seen = M (M - 1) / 2 is the denominator of ``pair_counts``' rates, and achieved_fmr = (number of
    scores > t) / pairs_seen <= fmr: what ``calc_FMR(emb, t)`` returns."""
    return thresholds_at_fmr(emb, [fmr])[0]
