"""Host-side checks of the exact-threshold radix select: the score-key map and the bin edges of frhip/pairwise.py against
their definitions, the three-pass descent (``select_rank``) run over the numpy histogram of tests/pair_hist_ref.py in
place of the kernel, negative controls that show the descent test sees the mistakes a histogram kernel can make, the
fp32 bracket of tests/test_gpu_pair_hist.py on the CPU, and the C ABI of the two new entry points."""
import ctypes

import numpy as np
import pytest

import pair_counts_ref as R
import pair_hist_ref as H

WINDOWS = ((0, 21, 2048), (0xBD800000, 10, 2048), (0x42000000, 10, 2048), (0xBD812345, 0, 1024), (0x7FFFFE00, 0, 1024),
           (0x7FF00000, 10, 2048), (0xFFE00000, 10, 2048), (0x3F800000, 21, 7))


def _sweep():
    rng = np.random.default_rng(1604)
    tiny = np.float32(1e-45)
    parts = [np.array([-np.inf, -3.4028235e38, -1.0, -0.0, 0.0, 1.0, 3.4028235e38, np.inf], np.float32),
             np.array([-tiny, tiny, -2 * tiny, 2 * tiny, -1.1754942e-38, 1.1754942e-38, -1.17549435e-38, 1.17549435e-38], np.float32),
             rng.standard_normal(4000).astype(np.float32) * np.float32(0.05),
             (rng.standard_normal(500) * 1e-41).astype(np.float32),  # subnormals
             rng.uniform(-1, 1, 2000).astype(np.float32)]
    s = np.concatenate(parts)
    with np.errstate(over="ignore"):  # the neighbours of the largest finite values are the infinities
        s = np.concatenate([s, np.nextafter(s, np.float32(np.inf)), np.nextafter(s, np.float32(-np.inf))])  # one ulp apart
    return s[~np.isnan(s)]


def test_key_map_is_monotone_and_invertible():
    from frhip.pairwise import key_score, score_key
    s = np.unique(_sweep())  # sorted, -0 == +0 merged by value
    k = score_key(s)
    assert k.dtype == np.uint32 and np.array_equal(k, H.score_key_ref(s))
    assert np.all(np.diff(k.astype(np.int64)) > 0)  # strictly increasing with the score
    back = key_score(k)
    assert back.dtype == np.float32 and np.array_equal(back, s)
    z = score_key(np.array([-0.0, 0.0], np.float32))
    assert z[0] == z[1] == 0x80000000 and not np.signbit(key_score(z)).any()
    assert score_key(np.array([1.0], np.float32))[0] == 0xBF800000 and score_key(np.array([-1.0], np.float32))[0] == 0x407FFFFF
    one = np.float32(1.0)
    assert score_key(np.array([np.nextafter(one, np.float32(2))]))[0] == 0xBF800001
    assert score_key(np.array([-np.inf, np.inf], np.float32)).tolist() == [0x007FFFFF, 0xFF800000]
    # shapes pass through
    assert score_key(np.zeros((3, 2), np.float32)).shape == (3, 2)


@pytest.mark.parametrize("key_lo,shift,bins", WINDOWS)
def test_bin_edges_against_the_definition(key_lo, shift, bins):
    from frhip.pairwise import bin_edges, score_key
    e = bin_edges(key_lo, shift, bins)
    assert e.dtype == np.float32 and e.shape == (bins + 1,)
    ek = key_lo + (np.arange(bins + 1, dtype=np.int64) << shift)
    finite = (ek >= 0x007FFFFF) & (ek <= 0xFF800000)  # keys of -inf .. +inf
    # 0x7FFFFFFF would be the key of -0, which shares +0's key 0x80000000: no score has it, its edge reads -0.0 (== +0)
    real = finite & (ek != 0x7FFFFFFF)
    assert np.array_equal(score_key(e[real]).astype(np.int64), ek[real])
    assert np.all(e[ek < 0x007FFFFF] == -np.inf) and np.all(e[ek > 0xFF800000] == np.inf)
    assert np.all(np.diff(e[real]) > 0)
    # every float at or above edge b and below edge b + 1 is in bin b: the edge itself, its upper neighbour, and the
    # lower neighbour of the next edge; the lower neighbour of edge b is in bin b - 1 (or below the window)
    with np.errstate(over="ignore"):
        up = np.nextafter(e, np.float32(np.inf))
        dn = np.nextafter(e, np.float32(-np.inf))
    for b in range(bins):
        if not (real[b] and finite[b + 1]):
            continue
        inside = [e[b], dn[b + 1]] + ([up[b]] if up[b] < e[b + 1] else [])
        h = H.hist_ref(np.array(inside, np.float32), key_lo, shift, bins)
        assert h[1 + b] == len(inside) and h.sum() == len(inside), (b, inside)
        if np.isfinite(dn[b]):
            h = H.hist_ref(np.array([dn[b]], np.float32), key_lo, shift, bins)
            # slot b = bin b - 1, or slot 0 = below the window; below +0 the unused key of -0 is skipped
            assert h[max(b - 1, 0) if (ek[b] == 0x80000000 and shift == 0) else b] == 1, b
    if finite[bins] and np.isfinite(e[bins]):
        assert H.hist_ref(np.array([e[bins]], np.float32), key_lo, shift, bins)[bins + 1] == 1


def test_hist_ref_window_semantics():
    s = np.array([-1.0, -0.0, 0.0, 0.5, 0.5, 1.0, np.nan, 2.0], np.float32)
    lo = 0x80000000  # the key of 0
    h = H.hist_ref(s, lo, 21, 508)  # 0 .. below 1.0: 508 bins of 2**21 keys
    assert h[0] == 1 and h[1] == 2 and h[-1] == 2 and h.sum() == 7
    assert h[1 + ((0xBF000000 - lo) >> 21)] == 2


def _lattice_scores():
    g16 = R.load_golden()
    E = R.lattice_rows(g16["lattice_pos"], g16["lattice_sign"])
    s = H.pair_scores(E)
    assert np.array_equal(s * 16, np.rint(s * 16))  # multiples of 1/16: exact in fp32
    return s.astype(np.float32)


def _random_scores(n=200000, nans=0):
    rng = np.random.default_rng(1605)
    s = (rng.standard_normal(n) * 0.044).astype(np.float32)
    if nans:
        s[rng.choice(n, nans, replace=False)] = np.nan
    return s


def _ranks(s):
    n = int((~np.isnan(s)).sum())
    return sorted({0, 1, 2, 17, n // 10000, n // 1000, n // 100, n // 2, n - 2, n - 1})


CASES = {"random": _random_scores, "ties": _lattice_scores, "nans": lambda: _random_scores(50000, 777)}


@pytest.mark.parametrize("case", sorted(CASES))
def test_three_pass_descent_equals_partition(case):
    from frhip.pairwise import SELECT_PASSES, select_rank
    assert SELECT_PASSES == ((21, 2048), (10, 2048), (0, 1024))
    s = CASES[case]()
    calls = []

    def hist(key_lo, shift, bins):
        calls.append((shift, bins))
        return H.hist_ref(s, key_lo, shift, bins)

    for k in _ranks(s):
        del calls[:]
        t, above = select_rank(hist, k)
        want, want_above = H.score_at_rank_ref(s, k)
        assert isinstance(t, np.float32) and t == want and above == want_above, (case, k, t, want, above, want_above)
        assert above <= k < above + int((s == t).sum())
        assert calls == [(21, 2048), (10, 2048), (0, 1024)]  # exactly three passes, 11 / 11 / 10 bits
    if case == "ties":
        assert any(H.score_at_rank_ref(s, k)[1] < k for k in _ranks(s))  # a tie really is among the tested ranks


def test_rank_out_of_range_raises():
    from frhip._lib import FrhipError
    from frhip.pairwise import select_rank
    s = _random_scores(1000, 10)
    hist = lambda key_lo, shift, bins: H.hist_ref(s, key_lo, shift, bins)  # noqa: E731
    assert select_rank(hist, 989)[0] == np.nanmin(s)
    for k in (990, 1000, -1):
        with pytest.raises(FrhipError):
            select_rank(hist, k)


# ---- negative controls: each mistake a histogram kernel can make changes an answer of the descent test (or trips the
# descent's own consistency check)
def _drops_overflow(s, key_lo, shift, bins):
    h = H.hist_ref(s, key_lo, shift, bins)
    h[bins + 1] = 0
    return h


def _edge_value_in_the_lower_bin(s, key_lo, shift, bins):
    """bins ( lo, hi ] instead of [ lo, hi ): a score exactly on an edge lands one bin too low."""
    s = np.asarray(s, np.float32)
    keys = H.score_key_ref(s[~np.isnan(s)]).astype(np.int64) - 1
    h = np.zeros(bins + 2, np.int64)
    d = keys - int(key_lo)
    slot = np.where(d < 0, 0, np.minimum(d >> shift, bins) + 1)
    np.add.at(h, slot, 1)
    return h


def _counts_nan(s, key_lo, shift, bins):
    """keys the NaNs by their bit pattern like any other score."""
    s = np.asarray(s, np.float32)
    h = H.hist_ref(s, key_lo, shift, bins)
    u = s[np.isnan(s)].view(np.uint32).astype(np.int64)
    keys = np.where(u & 0x80000000, (~u) & 0xFFFFFFFF, u | 0x80000000)
    d = keys - int(key_lo)
    np.add.at(h, np.where(d < 0, 0, np.minimum(d >> shift, bins) + 1), 1)
    return h


def _descent_passes(s, hist_fn):
    from frhip._lib import FrhipError
    from frhip.pairwise import select_rank
    for k in _ranks(s):
        try:
            got = select_rank(lambda lo, sh, nb: hist_fn(s, lo, sh, nb), k)
        except (FrhipError, IndexError):
            return False
        if got != H.score_at_rank_ref(s, k):
            return False
    return True


def test_negative_controls():
    rnd, ties, nans = CASES["random"](), CASES["ties"](), CASES["nans"]()
    assert _descent_passes(rnd, H.hist_ref) and _descent_passes(ties, H.hist_ref) and _descent_passes(nans, H.hist_ref)
    assert not _descent_passes(rnd, _drops_overflow)
    assert not _descent_passes(ties, _drops_overflow)
    assert not _descent_passes(ties, _edge_value_in_the_lower_bin)  # every lattice score lies on an edge of passes 1 and 2
    assert not _descent_passes(rnd, _edge_value_in_the_lower_bin)
    assert not _descent_passes(nans, _counts_nan)
    assert _descent_passes(rnd, _counts_nan)  # no NaN, no difference: the control is about NaN only


def test_fp32_order_statistic_falls_inside_the_bracket():
    """The bound of tests/test_gpu_pair_hist.py on the CPU.  Every fp32 score is within e < 6.3e-5 of its float64 value
    (DESIGN.md 7a), so the (k + 1)-th largest fp32 score t* is within e of the (k + 1)-th largest float64 score t64, and
    with d = 2**-13 > e:  c64(t* + d) <= c64(t64) <= k  and  c64(t* - d) >= c64(t64 - (d - e)) > k."""
    from frhip.pairwise import select_rank
    g16 = R.load_golden()
    X = R.random_rows(int(g16["random_seed"]), R.RANDOM_M)
    s64 = H.pair_scores(X)
    Xn = (X / np.sqrt((X * X).sum(1, dtype=np.float32))[:, None].astype(np.float32)).astype(np.float32)
    S = Xn @ Xn.T
    s32 = S[np.triu_indices(R.RANDOM_M, 1)]
    assert s32.dtype == np.float32
    for k in (0, 49, 499, 4995, 49950, 249750):
        t64, _ = H.score_at_rank_ref(s64, k)
        assert H.count_above(s64, t64 + R.DELTA) <= k < H.count_above(s64, t64 - R.DELTA)  # the reference alone
        t, above = select_rank(lambda lo, sh, nb: H.hist_ref(s32, lo, sh, nb), k)
        assert abs(float(t) - t64) < R.DELTA
        assert H.count_above(s64, float(t) + R.DELTA) <= k < H.count_above(s64, float(t) - R.DELTA)
        # and the bracket is not vacuous: it spans at most 0.25 % of the pairs (as for the tallies)
        assert H.count_above(s64, float(t) - R.DELTA) - H.count_above(s64, float(t) + R.DELTA) <= 0.0025 * s64.size


# ---- C ABI
def test_pair_hist_entries_are_declared_and_exported():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fr_pair_hist", "fr_pair_hist_parts"):
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.protos["fr_pair_hist"][2] == ["E", "ldE", "M", "D", "key_lo", "shift", "NB", "mode", "group", "partials",
                                              "hist", "stream"]
    assert _lib.protos["fr_pair_hist"][1][4] is ctypes.c_uint32
    assert _lib.protos["fr_pair_hist_parts"][2] == ["M", "mode", "group"]
    assert _lib.lib.fr_abi_version() == 7


def test_pair_hist_parts_is_the_tile_count_capped_at_the_resident_grid():
    from frhip import _lib
    lib = _lib.lib
    for m in (2, 5, 128, 129, 600, 1000, 4992, 5121, 16421, 65536):
        assert lib.fr_pair_hist_parts(m, 0, 0) == min(768, lib.fr_pair_counts_parts(m, 0, 0))
        for g in (2, 5, 16):
            assert lib.fr_pair_hist_parts(m, 1, g) == min(768, lib.fr_pair_counts_parts(m, 1, g))
    assert lib.fr_pair_hist_parts(600, 0, 0) == 15 and lib.fr_pair_hist_parts(65536, 0, 0) == 768
    # one workgroup must see fewer than 2**32 pairs: 768 workgroups x 262 143 tiles of 16 384
    assert lib.fr_pair_hist_parts(2_500_000, 0, 0) == 768
    assert lib.fr_pair_hist_parts(2_600_000, 0, 0) < 0 and b"2^32" in lib.fr_last_error_string()


def test_pair_hist_refuses_bad_arguments_without_a_gpu():
    from frhip import _lib
    lib = _lib.lib
    buf = (ctypes.c_float * 64)()  # never read: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    base = p.value + (-p.value) % 16  # a 16-byte aligned address inside buf
    ok = dict(E=base, M=16, D=8, ldE=8, key_lo=0, shift=21, NB=2048, mode=0, group=0)
    for bad, word in ((dict(mode=2), b"mode"), (dict(mode=-1), b"mode"), (dict(mode=1, group=1), b"group"),
                      (dict(mode=1, group=17), b"group"), (dict(NB=0), b"NB"), (dict(NB=2049), b"NB"), (dict(shift=22), b"shift"),
                      (dict(shift=-1), b"shift"), (dict(key_lo=1), b"window"), (dict(key_lo=0xFFFFFC01, shift=0, NB=1024), b"window"),
                      (dict(key_lo=0x80000000, shift=21, NB=1025), b"window"), (dict(E=base + 4), b"aligned"),
                      (dict(M=1), b"M"), (dict(D=6, ldE=6), b"D"), (dict(ldE=4), b"ldE"), (dict(E=None), b"required")):
        a = dict(ok, **bad)
        rc = lib.fr_pair_hist(a["E"], a["ldE"], a["M"], a["D"], a["key_lo"], a["shift"], a["NB"], a["mode"], a["group"], p, p,
                              None)
        assert rc < 0, a
        assert word in lib.fr_last_error_string(), (a, lib.fr_last_error_string())
    assert lib.fr_pair_hist_parts(1, 0, 0) < 0 and lib.fr_pair_hist_parts(16, 2, 0) < 0
    assert lib.fr_pair_hist_parts(16, 1, 1) < 0 and b"fr_pair_hist" in lib.fr_last_error_string()
    # the shared shape check still speaks for fr_pair_counts under its own name
    assert lib.fr_pair_counts_parts(16, 1, 1) < 0 and b"fr_pair_counts" in lib.fr_last_error_string()


def test_host_tensor_is_refused():
    import torch
    from frhip import _lib
    from frhip.pairwise import pair_histogram, score_at_rank, threshold_at_fmr
    with pytest.raises(_lib.FrhipError):
        pair_histogram(torch.zeros(8, 8), 0, 21, 2048)
    with pytest.raises(_lib.FrhipError):
        score_at_rank(torch.zeros(8, 8), 0)
    with pytest.raises(_lib.FrhipError):
        threshold_at_fmr(torch.zeros(8, 8), 1e-2)
