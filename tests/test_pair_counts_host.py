"""Host-side checks of the RB-WebFace pair tallies: the float64 statement tests/pair_counts_ref.py against the reference's
own calc_FMR / calc_FNMR (g16_rbwebface, tests/golden/make_golden_rbwebface.py), negative controls that show the fixture
sees the mistakes a kernel can make, the fp32 bracket on the CPU, and the C ABI of the two new entry points."""
import ctypes

import numpy as np
import pytest

import pair_counts_ref as R


@pytest.fixture(scope="module")
def g16():
    return R.load_golden()


@pytest.fixture(scope="module")
def lattice(g16):
    return R.lattice_rows(g16["lattice_pos"], g16["lattice_sign"])


def _rates(E, thr, group=None):
    c, seen = R.pair_counts_ref(E, thr, group)
    return c / seen, c, seen


def test_fixture_inputs_regenerate(g16, lattice):
    pos, sign = R.lattice_draw()
    assert np.array_equal(pos, g16["lattice_pos"]) and np.array_equal(sign, g16["lattice_sign"])
    assert lattice.shape == (R.LATTICE_M, R.LATTICE_D)
    assert np.all((lattice.astype(np.float64) ** 2).sum(1) == 1.0)
    X = R.random_rows(int(g16["random_seed"]), R.RANDOM_M)
    assert R.checksum(X) == g16["random_crc32"]
    assert int(g16["group"]) == R.GROUP


def test_ref_reproduces_the_reference_on_the_lattice(g16, lattice):
    for thr, fmr, fnmr in ((g16["lattice_thr"], g16["lattice_fmr"], g16["lattice_fnmr"]),
                           (g16["lattice_thr_on"], g16["lattice_fmr_on"], g16["lattice_fnmr_on"])):
        r0, _c, seen0 = _rates(lattice, thr)
        r1, _c, seen1 = _rates(lattice, thr, R.GROUP)
        assert seen0 == 600 * 599 // 2 and seen1 == 120 * 10
        assert np.array_equal(r0, fmr) and np.array_equal(r1, fnmr)
    # every threshold between lattice points separates something, and the curves span the whole range
    assert np.all(np.diff(g16["lattice_fmr"]) <= 0) and g16["lattice_fmr"][0] > 0.9999 and g16["lattice_fmr"][-1] == 0
    assert g16["lattice_fnmr"][0] == 0 and g16["lattice_fnmr"][-1] == 1
    # strictness: a score ON the threshold k / 16 is in neither tally, so "> k / 16" is "> (k + 0.5) / 16" (a ">=" would
    # give the tally of (k - 0.5) / 16, which differs) and "< k / 16" is "< (k - 0.5) / 16"
    assert np.array_equal(g16["lattice_fmr_on"], g16["lattice_fmr"])
    assert np.all(g16["lattice_fmr_on"][1:-1] != g16["lattice_fmr"][:-2])
    assert np.array_equal(g16["lattice_fnmr_on"][1:], g16["lattice_fnmr"][:-1])
    assert not np.array_equal(g16["lattice_fnmr_on"], g16["lattice_fnmr"])


def test_ref_reproduces_the_reference_on_the_random_set(g16):
    X = R.random_rows(int(g16["random_seed"]), R.RANDOM_M)
    r0, _c, _s = _rates(X, g16["random_thr"])
    r1, _c, _s = _rates(X, g16["random_thr"], R.GROUP)
    assert np.array_equal(r0, g16["random_fmr"]) and np.array_equal(r1, g16["random_fnmr"])


def test_ragged_last_group_and_zero_row():
    pos, sign = R.lattice_draw(13)
    E = R.lattice_rows(pos, sign)
    _c, seen = R.pair_counts_ref(E, [0.0], R.GROUP)
    assert seen == 10 + 10 + 3  # 5 + 5 + 3 rows
    E[4] = 0
    c, seen = R.pair_counts_ref(E, [-2.0])
    assert seen == 78 and c[0] == 78 - 12  # the zero row's 12 pairs are NaN: seen, never counted
    c, seen = R.pair_counts_ref(E, [2.0], R.GROUP)
    assert seen == 23 and c[0] == 23 - 4


# ---- negative controls: each mistake changes at least one stored tally of the lattice set
def _scores(E):
    E = E.astype(np.float64)
    return E @ E.T


def _golden_counts(g16):
    return (np.rint(g16["lattice_fmr"] * (600 * 599 // 2)).astype(np.int64),
            np.rint(g16["lattice_fnmr"] * 1200).astype(np.int64),
            np.rint(g16["lattice_fmr_on"] * (600 * 599 // 2)).astype(np.int64))


def test_negative_controls(g16, lattice):
    S = _scores(lattice)
    thr, thr_on = g16["lattice_thr"], g16["lattice_thr_on"]
    fmr_c, fnmr_c, fmr_on_c = _golden_counts(g16)
    iu = np.triu_indices(600, 1)
    above = lambda s, t: np.array([(s > x).sum() for x in t], np.int64)  # noqa: E731
    assert np.array_equal(above(S[iu], thr), fmr_c)  # the control itself is right
    # counting the diagonal
    assert not np.array_equal(above(S[np.triu_indices(600, 0)], thr), fmr_c)
    # counting both triangles
    assert not np.array_equal(above(S[~np.eye(600, dtype=bool)], thr), fmr_c)
    # >= for >
    assert not np.array_equal(np.array([(S[iu] >= x).sum() for x in thr_on], np.int64), fmr_on_c)
    # a group size off by one, either way
    for g in (4, 6):
        c, _seen = R.pair_counts_ref(lattice, thr, g)
        assert not np.array_equal(c, fnmr_c)
    # dropping the last partial tile (600 = 4 * 128 + 88): rows and columns from 512 on
    keep = (iu[0] < 512) & (iu[1] < 512)
    assert not np.array_equal(above(S[iu][keep], thr), fmr_c)
    c, _seen = R.pair_counts_ref(lattice[:512], thr, R.GROUP)
    assert not np.array_equal(c, fnmr_c)


def test_fp32_scores_fall_inside_the_bracket(g16):
    """The bound of tests/test_gpu_pair_counts.py on the CPU: fp32-normalised rows, numpy float32 matmul."""
    X = R.random_rows(int(g16["random_seed"]), R.RANDOM_M)
    thr = g16["random_thr"]
    Xn = (X / np.sqrt((X * X).sum(1, dtype=np.float32))[:, None].astype(np.float32)).astype(np.float32)
    S = Xn @ Xn.T
    assert S.dtype == np.float32
    t32 = thr.astype(np.float32)
    iu = np.triu_indices(R.RANDOM_M, 1)
    got0 = np.array([(S[iu] > t).sum() for t in t32], np.int64)
    lo, seen = R.pair_counts_ref(X, thr + R.DELTA)
    hi, _ = R.pair_counts_ref(X, thr - R.DELTA)
    assert np.all(lo <= got0) and np.all(got0 <= hi)
    assert np.all(hi - lo <= 0.0025 * seen)
    same = (iu[0] // R.GROUP) == (iu[1] // R.GROUP)
    got1 = np.array([(S[iu][same] < t).sum() for t in t32], np.int64)
    lo, _ = R.pair_counts_ref(X, thr - R.DELTA, R.GROUP)
    hi, _ = R.pair_counts_ref(X, thr + R.DELTA, R.GROUP)
    assert np.all(lo <= got1) and np.all(got1 <= hi)


# ---- C ABI
def _parts_mode0(m):
    nt = (m + 127) // 128
    return nt * (nt + 1) // 2


def _parts_mode1(m, g):
    nt = (m + 127) // 128
    return nt + sum(1 for k in range(1, nt) if (k * 128) % g)


def test_pair_count_entries_are_declared_and_exported():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("fr_pair_counts", "fr_pair_counts_parts"):
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.protos["fr_pair_counts"][2] == ["E", "ldE", "M", "D", "thr", "T", "mode", "group", "partials", "counts",
                                                "stream"]
    assert _lib.lib.fr_abi_version() == 7


def test_pair_counts_parts_is_the_triangular_tile_count():
    from frhip import _lib
    lib = _lib.lib
    for m in (2, 5, 128, 129, 600, 1000, 16421, 65536):
        assert lib.fr_pair_counts_parts(m, 0, 0) == _parts_mode0(m)
        for g in (2, 3, 5, 6, 7, 12, 16):
            assert lib.fr_pair_counts_parts(m, 1, g) == _parts_mode1(m, g), (m, g)
    assert lib.fr_pair_counts_parts(65536, 0, 0) == 131328


def test_pair_counts_refuses_bad_arguments_without_a_gpu():
    from frhip import _lib
    lib = _lib.lib
    buf = (ctypes.c_float * 64)()  # never read: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    ok = dict(M=16, D=8, T=4, mode=0, group=0)
    for bad, word in ((dict(T=0), b"T"), (dict(T=33), b"T"), (dict(M=1), b"M"), (dict(D=6), b"D"), (dict(mode=2), b"mode"),
                      (dict(mode=1, group=1), b"group"), (dict(mode=1, group=17), b"group")):
        a = dict(ok, **bad)
        rc = lib.fr_pair_counts(p, a["D"], a["M"], a["D"], p, a["T"], a["mode"], a["group"], p, p, None)
        assert rc < 0, a
        assert word in lib.fr_last_error_string(), (a, lib.fr_last_error_string())
    assert lib.fr_pair_counts_parts(1, 0, 0) < 0 and lib.fr_pair_counts_parts(16, 2, 0) < 0
    assert lib.fr_pair_counts_parts(16, 1, 1) < 0


def test_pairs_in_matches_the_reference_count():
    from frhip.pairwise import pairs_in
    assert pairs_in(600) == 179700 and pairs_in(600, 5) == 1200 and pairs_in(13, 5) == 23 and pairs_in(2) == 1
    assert pairs_in(65536) == 2147450880


def test_host_tensor_is_refused():
    import torch
    from frhip import _lib
    from frhip.pairwise import pair_counts
    with pytest.raises(_lib.FrhipError):
        pair_counts(torch.zeros(8, 8), [0.0])
