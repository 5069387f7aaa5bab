"""numpy statement of the score-key histogram (fr_pair_hist) and of the order statistic the radix select must return.
Written for this repository; numpy only.  The key map is written differently from frhip/pairwise.py's on purpose.

    keys = score_key_ref(scores)                      # uint32, s1 < s2 <=> key1 < key2, -0 and +0 share a key
    hist = hist_ref(scores, key_lo, shift, bins)      # int64 [bins + 2]: below the window, the bins, above; NaN nowhere
    s    = pair_scores(E, group=None)                 # float64 cosines of the pairs i < j (same group), NaN for a zero row
    t, count_above = score_at_rank_ref(scores, k)     # (k + 1)-th largest by np.partition, and #{ s > t }
"""
import numpy as np

import pair_counts_ref as R


def score_key_ref(scores):
    s = np.array(scores, dtype=np.float32, copy=True).reshape(-1)
    s[s == 0] = 0.0  # -0 -> +0
    i = s.view(np.int32).astype(np.int64)
    # negative floats: all 32 bits flipped; the others: the sign bit set
    return np.where(i < 0, (~i) & 0xFFFFFFFF, i | 0x80000000).astype(np.uint32)


def hist_ref(scores, key_lo, shift, bins):
    s = np.asarray(scores, dtype=np.float32).reshape(-1)
    keys = score_key_ref(s[~np.isnan(s)]).astype(np.int64)
    lo, width = int(key_lo), 1 << int(shift)
    hist = np.zeros(bins + 2, np.int64)
    hist[0] = (keys < lo).sum()
    hist[bins + 1] = (keys >= lo + bins * width).sum()
    inside = keys[(keys >= lo) & (keys < lo + bins * width)]
    hist[1:bins + 1] = np.bincount((inside - lo) // width, minlength=bins)
    return hist


def pair_scores(E, group=None):
    """float64 cosines (scipy's: NaN for a zero row) of the pairs the tallies run over, as one flat array."""
    E = np.asarray(E, dtype=np.float64)
    nrm = np.sqrt((E * E).sum(1))
    S = R.cosine_block(E, nrm, E, nrm)
    i, j = np.triu_indices(E.shape[0], 1)
    if group is not None:
        same = (i // group) == (j // group)
        i, j = i[same], j[same]
    return S[i, j]


def score_at_rank_ref(scores, k):
    s = np.asarray(scores).reshape(-1)
    s = s[~np.isnan(s)]
    assert 0 <= k < s.size
    t = np.partition(s, s.size - 1 - k)[s.size - 1 - k]
    return t, int((s > t).sum())


def count_above(scores, t):
    """c64(t): scores strictly above t (NaN never)."""
    s = np.asarray(scores).reshape(-1)
    return int((s[~np.isnan(s)] > t).sum())
