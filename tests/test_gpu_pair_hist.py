"""GPU checks of fr_pair_hist (frhip.pairwise.pair_histogram), of the radix select built on it (score_at_rank,
threshold_at_fmr) and of rb-webface/scripts/exact_RB_Webface.py, the RB-WebFace driver with --exact_fpr.

Exact against the existing kernel.  fr_pair_hist and fr_pair_counts form their scores in one main loop
(csrc/pair_tile.h), so on ANY rows the number of scores at or above bin edge b -- the histogram's suffix sum, the slot
above the window included -- must EQUAL the mode-0 tally "score > the fp32 value just below edge b", and the number of
scores below edge b (the prefix sum) the mode-1 tally "score < edge b": at every edge, no bracket.

Exact against float64 on the lattice set of g16_rbwebface (scores are multiples of 1/16, exact in fp32 in any order).

Bracket on fp32 rounding (random unit rows, D = 512), d = 2**-13 as for the tallies (tests/test_gpu_pair_counts.py has the
derivation: every fp32 score is within e < 6.3e-5 of its float64 value).  The (k + 1)-th largest of values that each moved
by at most e moved by at most e, so with t64 the float64 order statistic |t* - t64| <= e < d and, c64(x) being the float64
count of scores above x:  c64(t* + d) <= c64(t64) <= k  and  c64(t* - d) >= c64(t64 - (d - e)) > k.  Both hold for the
reference alone whatever M and seed are (t64 itself lies above t64 - d, with the k scores above it);
tests/test_pair_hist_host.py checks that, and that the bracket spans at most 0.25 % of the pairs, on the CPU.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import pair_counts_ref as R
import pair_hist_ref as H

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(REPO, "stylegan-for-facerec_amd", "rb-webface", "scripts")
KEY_NEG_INF, KEY_POS_INF = 0x007FFFFF, 0xFF800000


@pytest.fixture(scope="module")
def g16():
    return R.load_golden()


@pytest.fixture(scope="module")
def lattice(g16):
    return R.lattice_rows(g16["lattice_pos"], g16["lattice_sign"])


def _script(name):
    spec = importlib.util.spec_from_file_location("rb_webface_" + name[:-3], os.path.join(SCRIPTS, name))  # the directory name has a hyphen
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def driver():
    return _script("test_RB_Webface.py")  # the reference's driver, unchanged


@pytest.fixture(scope="module")
def exact():
    return _script("exact_RB_Webface.py")  # the same evaluation with --exact_fpr


def _dev(E):
    return E if isinstance(E, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(E)).cuda()


def _hist(E, key_lo, shift, bins, group=None):
    from frhip.pairwise import pair_histogram
    h, seen = pair_histogram(_dev(E), key_lo, shift, bins, group)
    assert h.dtype == torch.int64 and h.is_cuda and h.shape == (bins + 2,)
    return h.cpu().numpy(), seen


def _counts(E, thr, group=None):
    from frhip.pairwise import pair_counts
    return pair_counts(_dev(E), thr, group)[0].cpu().numpy()


def _key_float(keys):
    """The fp32 value of each key, -inf / +inf beyond the keys of the infinities."""
    from frhip.pairwise import key_score
    return key_score(np.clip(keys, KEY_NEG_INF, KEY_POS_INF).astype(np.uint32))


def _check_against_pair_counts(E, key_lo, shift, bins, group):
    h, seen = _hist(E, key_lo, shift, bins, group)
    ek = key_lo + (np.arange(bins + 1, dtype=np.int64) << shift)
    if group is None:
        # score >= edge  <=>  key >= ek  <=>  key > ek - 1  <=>  score > float(ek - 1) = nextafter(edge, -inf).  The key
        # below +0's (0x7FFFFFFF) is the unused key of -0: nextafter(+0, -inf) is the float of 0x7FFFFFFE.
        below = np.where(ek - 1 == 0x7FFFFFFF, 0x7FFFFFFE, ek - 1)
        thr = _key_float(below)
        got = np.cumsum(h[::-1])[::-1][1:]  # suffix sums from slot 1 + b on: bins b .. and the slot above the window
    else:
        thr = _key_float(ek)
        got = np.cumsum(h)[:-1]             # prefix sums up to slot b: below the window and bins .. b - 1
    want = _counts(E, thr, group)
    bad = np.nonzero(got != want)[0]
    print("M %d D %d group %s key_lo %08x shift %d bins %d: %d of %d slots occupied, %d edges differ"
          % (E.shape[0], E.shape[1], group, key_lo, shift, bins, int((h > 0).sum()), bins + 2, bad.size))
    assert bad.size == 0, (bad[:8], got[bad[:8]], want[bad[:8]], thr[bad[:8]])
    return h, seen


def _rows(m, d, seed):
    """Unnormalised fp32 rows with a zero row; the scale differs from row to row."""
    from frhip import synth
    x = synth.normal(seed, "pair_hist.rows", (m, d)).numpy()
    x *= (1.0 + np.arange(m, dtype=np.float32) % 5)[:, None]
    x[m // 3] = 0
    return x


def _windows(E, group):
    """(key_lo, shift, bins) of the three passes: the whole key range, then the windows a select descends through for a
    rank in the upper tail and for the median, then windows that no select would choose (unaligned, around zero)."""
    from frhip.pairwise import select_rank
    out = []
    total = int(_hist(E, 0, 21, 2048, group)[0].sum())

    def spy(key_lo, shift, bins):
        out.append((key_lo, shift, bins))
        return _hist(E, key_lo, shift, bins, group)[0]

    for k in (total // 100, total // 2):
        select_rank(spy, k)
    out += [(0xBD812345, 10, 2048), (0x7FFFFE00, 0, 1024), (0x7FF00000, 10, 2048), (0xBE000000, 21, 100), (0x80000000, 21, 1024)]
    return sorted(set(out))


@pytest.mark.parametrize("m,d", [(1003, 512), (333, 20)])
@pytest.mark.parametrize("group", [None, 2, 5, 16])
def test_equals_pair_counts_at_every_edge(m, d, group):
    E = _rows(m, d, 1606)
    wins = _windows(E, group)
    assert {w[1] for w in wins} == {21, 10, 0}
    from frhip.pairwise import pairs_in
    zero_pairs = (m - 1) if group is None else (min(m, (m // 3) // group * group + group) - (m // 3) // group * group - 1)
    for key_lo, shift, bins in wins:
        h, seen = _check_against_pair_counts(E, key_lo, shift, bins, group)
        assert seen == pairs_in(m, group)
        assert int(h.sum()) + zero_pairs == seen  # every pair is in one slot, but the NaN pairs of the zero row


def test_equals_pair_counts_with_persistent_workgroups():
    """41 x 41 tiles of the triangle = 861 > the 768 workgroups of the grid: some walk two tiles; ragged M."""
    E = _rows(5205, 20, 1607)
    for key_lo, shift, bins in ((0, 21, 2048), (0xBE000000, 10, 2048)):
        h, seen = _check_against_pair_counts(E, key_lo, shift, bins, None)
        assert int(h.sum()) + 5204 == seen


def test_lattice_equals_float64_exactly(lattice):
    from frhip.pairwise import score_at_rank
    for group in (None, R.GROUP):
        s = H.pair_scores(lattice, group).astype(np.float32)
        for key_lo, shift, bins in ((0, 21, 2048), (0xBD800000, 10, 2048), (0x80000000, 0, 1024), (0xBE800000, 0, 1024),
                                    (0x80000000, 21, 1024), (0x41000000, 21, 1500)):
            h, seen = _hist(lattice, key_lo, shift, bins, group)
            assert seen == s.size and np.array_equal(h, H.hist_ref(s, key_lo, shift, bins)), (group, key_lo, shift)
        n = s.size
        for k in sorted({0, 1, 5, n // 1000, n // 100, n // 10, n // 2, n - 2, n - 1}):
            t, above = score_at_rank(_dev(lattice), k, group)
            assert (t, above) == H.score_at_rank_ref(s, k), (group, k)
            assert isinstance(t, np.float32)


def test_leading_rows_and_a_zero_row(lattice):
    for m in (599, 257, 129, 128, 6, 2):
        E = lattice[:m].copy()
        if m > 5:
            E[4] = 0
        for group in (None, 3):
            s = H.pair_scores(E, group).astype(np.float32)
            h, seen = _hist(E, 0, 21, 2048, group)
            assert seen == s.size and np.array_equal(h, H.hist_ref(s, 0, 21, 2048)), (m, group)
            assert h[0] == 0 and h[-1] == 0 and h.sum() == (~np.isnan(s)).sum()


def test_rank_beyond_the_pairs_raises(lattice):
    from frhip._lib import FrhipError
    from frhip.pairwise import pair_histogram, score_at_rank
    E = lattice[:10].copy()
    E[0] = 0
    x = _dev(E)
    t, above = score_at_rank(x, 35)  # 36 pairs have a score, 9 are NaN
    assert t == np.nanmin(H.pair_scores(E)).astype(np.float32)
    with pytest.raises(FrhipError):
        score_at_rank(x, 36)
    with pytest.raises(FrhipError):
        pair_histogram(x, 1, 21, 2048)  # the window passes 2**32
    with pytest.raises(FrhipError):
        pair_histogram(x, 0, 22, 512)
    with pytest.raises(FrhipError):
        pair_histogram(torch.zeros(8, 6, device="cuda"), 0, 21, 2048)


def test_bracket_on_the_golden_random_set(g16):
    from frhip.pairwise import pairs_in, score_at_rank, threshold_at_fmr
    X = R.random_rows(int(g16["random_seed"]), R.RANDOM_M)
    assert R.checksum(X) == g16["random_crc32"]
    s64 = H.pair_scores(X)
    xd = _dev(X)
    for k in (0, 49, 499, 4995, 49950, 249750):
        t64, _ = H.score_at_rank_ref(s64, k)
        t, above = score_at_rank(xd, k)
        lo, hi = H.count_above(s64, float(t) + R.DELTA), H.count_above(s64, float(t) - R.DELTA)
        print("k %6d  t* %.9g  t64 %.9g  count_above %d  c64(t* + d) %d  c64(t* - d) %d" % (k, t, t64, above, lo, hi))
        assert lo <= k < hi
        assert above <= k
    t, fmr = threshold_at_fmr(xd, 1e-2)
    t2, above = score_at_rank(xd, 4995)
    assert pairs_in(R.RANDOM_M) == 499500 and t == t2 and fmr == above / 499500 and fmr <= 1e-2
    # genuine pairs (mode 1): the same select over the pairs inside groups of 5
    s64 = H.pair_scores(X, R.GROUP)
    for k in (0, 20, 1000, 1999):
        t, above = score_at_rank(xd, k, group=R.GROUP)
        assert H.count_above(s64, float(t) + R.DELTA) <= k < H.count_above(s64, float(t) - R.DELTA) and above <= k


def test_self_consistency_and_repeatability_at_16421_rows():
    """129 x 129 tiles of the triangle = 8 385: every workgroup of the grid walks 10 or 11 of them."""
    from frhip.pairwise import pair_histogram, pairs_in, score_at_rank, threshold_at_fmr
    X = R.random_rows(R.BIG_SEED, R.BIG_M)
    xd = _dev(X)
    seen = pairs_in(R.BIG_M)
    for fpr in (1e-3, 1e-4, 0.5):
        k = int(fpr * seen)
        t, above = score_at_rank(xd, k)
        c = _counts(xd, np.array([t, np.nextafter(t, np.float32(-np.inf))], np.float32))
        print("FPR %g  k %d  t* %.9g  count_above %d  pair_counts(t*) %d  pair_counts(below t*) %d" % (fpr, k, t, above, c[0], c[1]))
        assert c[0] == above <= k < c[1]
        assert threshold_at_fmr(xd, fpr) == (t, above / seen)
    k = pairs_in(R.BIG_M, R.GROUP) // 10
    t, above = score_at_rank(xd, k, group=R.GROUP)
    # mode 1 tallies score < thr: the scores above t* are those not below the next float
    total = int(_hist(xd, 0, 21, 2048, R.GROUP)[0].sum())
    c = _counts(xd, np.array([np.nextafter(t, np.float32(np.inf)), t], np.float32), R.GROUP)
    assert total - c[0] == above <= k < total - c[1]
    for key_lo, shift, bins, group in ((0, 21, 2048, None), (0xBE200000, 10, 2048, None), (0xBE275400, 0, 1024, None),
                                       (0, 21, 2048, R.GROUP)):
        a, _ = pair_histogram(xd, key_lo, shift, bins, group)
        b, _ = pair_histogram(xd, key_lo, shift, bins, group)
        assert torch.equal(a, b)
        assert int(a.sum()) == pairs_in(R.BIG_M, group)


# ---- the driver
def _write_tree(tmp_path, n_pos=15, n_neg=24):
    """Small JPEGs (two sizes, so one batch is mixed) and the eight list files (as in tests/test_gpu_pair_counts.py)."""
    from PIL import Image
    from frhip import synth
    data = tmp_path / "images"
    lists = tmp_path / "lists"
    data.mkdir()
    lists.mkdir()
    names = {}
    for gi, grp in enumerate(("African", "Asian", "Caucasian", "Indian")):
        for kind, n in (("pos", n_pos), ("neg", n_neg)):
            rel = []
            for k in range(n):
                side = 112 if (k % 7) else 120
                lo = synth.uniform(40 + gi, "%s.%s.%d" % (grp, kind, k), (8, 8, 3), 0.0, 255.0).numpy().astype(np.uint8)
                img = Image.fromarray(lo).resize((side, side), Image.BILINEAR)
                name = "%s_%s_%02d.jpg" % (grp, kind, k)
                img.save(str(data / name), quality=95)
                rel.append(name)
            (lists / ("%s_pairs_samples_%s.txt" % (kind, grp))).write_text("\n".join(rel) + "\n")
            names[(grp, kind)] = rel
    return str(data), str(lists), names


def _reference_lines(driver, ckpt, embs, thr):
    """What the reference's driver prints from the checkpoint line on, rebuilt from the same tallies."""
    lines = ["Loading Backbone Checkpoint '{}'".format(ckpt)]
    for grp in ("African", "Asian", "Caucasian", "Indian"):
        lines += ["calculating embeddings for positive names", "calculating embeddings for negative names"]
        fmr, fnmr = driver.group_rates(embs[(grp, "pos")], embs[(grp, "neg")], thr, 5)
        for t, a, b in zip(thr, list(fnmr), list(fmr)):
            lines.append("threshold %s fnmr %s fmr %s" % (t, a, b))
        lines += ["=" * 20, "Group  %s" % grp,
                  "TPR@FPR=1e-3 %s" % (1 - np.interp(1e-3, list(fmr)[::-1], list(fnmr)[::-1])),
                  "TPR@FPR=1e-4 %s" % (1 - np.interp(1e-4, list(fmr)[::-1], list(fnmr)[::-1])), ""]
    return lines


def test_driver_exact_fpr_end_to_end(tmp_path, driver, exact, capsys):
    from frhip import synth
    import configs.config_synthetic_smoke as smoke_cfg
    from train import build_backbone

    data, lists, names = _write_tree(tmp_path)
    config = smoke_cfg.__file__
    model = build_backbone(smoke_cfg.configurations[1])
    synth.fill_state_dict(model.state_dict(), 21)
    ckpt = str(tmp_path / "Backbone_test.pth")
    torch.save(model.state_dict(), ckpt)
    backbone = driver.initialize_model(config, ckpt)
    embs = {key: driver.calc_embeddings(backbone, rel, data, batch_size=10, num_workers=0) for key, rel in names.items()}
    capsys.readouterr()

    # the reference's driver: its lines, nothing else
    thr = np.linspace(0.5, 1.01, 18)  # FMR 1 at one end (the smoke backbone's embeddings lie close together), 0 at the other
    plain = driver.evaluate_model(config, ckpt, data, lists, gpu_batch_size=10, thresholds=thr, num_workers=0)
    out_plain = capsys.readouterr().out
    plain_lines = out_plain.splitlines()
    assert plain_lines[0] == "initializing model..."
    start = plain_lines.index("Loading Backbone Checkpoint '{}'".format(ckpt))  # the backbone builder's own lines come before
    assert plain_lines[start:] == _reference_lines(driver, ckpt, embs, thr)
    assert not any(ln.startswith(("exact ", "warning")) for ln in plain_lines)

    # the new script without the flag: the same output, line for line
    no_flag = exact.evaluate_model(config, ckpt, data, lists, gpu_batch_size=10, thresholds=thr, num_workers=0)
    assert capsys.readouterr().out == out_plain
    assert no_flag == plain + ({},)

    # with it: the driver's output first, then per group a block "Group  <name>", one exact line, a blank line; this
    # grid's FMR values span 1e-2, so no warning
    with_flag = exact.evaluate_model(config, ckpt, data, lists, cpu_batch_size=1000, cpu_n_jobs=2, gpu_batch_size=10,
                                     thresholds=thr, num_workers=0, exact_fpr=[1e-2])
    out = capsys.readouterr().out
    assert with_flag[:2] == plain and list(with_flag[2]) == list(plain[0])
    assert out.startswith(out_plain)
    tail = out[len(out_plain):].splitlines()
    assert len(tail) == 12 and tail[0::3] == ["Group  %s" % g for g in plain[0]] and tail[2::3] == [""] * 4
    extra = tail[1::3]
    for ln, grp in zip(extra, ("African", "Asian", "Caucasian", "Indian")):
        w = ln.split()
        assert w[:2] == ["exact", "TPR@FPR=0.01"] and w[3] == "threshold" and w[5] == "fmr"
        tpr, t, fmr = float(w[2]), float(w[4]), float(w[6])
        s_neg = H.pair_scores(embs[(grp, "neg")].cpu().numpy())
        s_pos = H.pair_scores(embs[(grp, "pos")].cpu().numpy(), 5)
        assert s_neg.size == 276 and s_pos.size == 30
        k = int(np.floor(1e-2 * 276))
        t64, _ = H.score_at_rank_ref(s_neg, k)
        print(grp, "threshold %.9g (float64 %.9g)  fmr %.6g  tpr %.6g" % (t, t64, fmr, tpr))
        assert abs(t - t64) < R.DELTA
        assert H.count_above(s_neg, t + R.DELTA) <= k < H.count_above(s_neg, t - R.DELTA)
        assert H.count_above(s_neg, t + R.DELTA) / 276 <= fmr <= min(k, H.count_above(s_neg, t - R.DELTA)) / 276
        below = lambda x: int((s_pos < x).sum())  # noqa: E731
        assert 1 - below(t + R.DELTA) / 30 <= tpr <= 1 - below(t - R.DELTA) / 30
        assert [(1e-2, t, fmr, tpr)] == exact.exact_rates(embs[(grp, "pos")], embs[(grp, "neg")], [1e-2], 5) == with_flag[2][grp]

    # a grid placed away from the target: no cosine reaches it, all its FMR values are 0, the reference's number is a clamp,
    # and the driver says so
    far = np.linspace(1.5, 2.0, 5)
    exact.evaluate_model(config, ckpt, data, lists, gpu_batch_size=10, thresholds=far, num_workers=0, exact_fpr=[1e-2])
    out = capsys.readouterr().out
    assert out.count("warning: FPR=0.01 lies outside the FMR range") == 4
    assert len([ln for ln in out.splitlines() if ln.startswith("exact ")]) == 4
    # several FPRs share the normalisation and the first pass, and give what one call each gives
    from frhip.pairwise import threshold_at_fmr, thresholds_at_fmr
    neg = embs[("Asian", "neg")]
    assert thresholds_at_fmr(neg, [1e-2, 0.1, 1e-2]) == [threshold_at_fmr(neg, f) for f in (1e-2, 0.1, 1e-2)]
