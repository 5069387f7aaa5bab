"""GPU checks of frhip.pairwise.pair_counts (fr_pair_counts) and of the RB-WebFace driver built on it.

Exact part: the lattice set of g16_rbwebface (scores are multiples of 1/16, exact in fp32 in any summation order), so the
kernel's tallies must equal the reference's integers.

Bracket on fp32 rounding (random unit rows, D = 512).  With c64(t) the float64 tally at threshold t, mode 0 must satisfy
c64(t + d) <= gpu(t) <= c64(t - d) and mode 1 the mirror image, d = 2**-13.  Derivation: a score is a sum of 512 products
accumulated in fp32 (the f32-input MFMA is a k-ordered fmaf chain), error at most gamma_512 = 512 * 2**-24 = 3.05e-5 times
sum |a_i b_i| <= 1 (Cauchy-Schwarz on unit rows); the fp32 normalisation of each row is off by at most about half of that,
two rows: 3.2e-5; the fp32 cast of a threshold: 3e-8.  Total below 6.3e-5; d = 1.22e-4 is twice that.  Two-sided, no case
left out.  So that the bracket cannot be vacuous, c64(t - d) - c64(t + d) must be at most 0.25 % of pairs_seen at every
threshold (thresholds in [-0.1, 0.1], the densest part of the score distribution: about 0.22 % measured).  That width
assertion is made wherever 0.25 % of pairs_seen is more than sampling noise: the genuine pairs of the 1 000-row golden set
are 2 000, 0.25 % of them is 5 pairs against an expected width of 4.4 +- 2.1 (the float64 width there is 9 pairs, whatever the
code under test does), so for that one case only the bracket itself is asserted; the 16 421-row genuine case (32 840 pairs)
carries the width assertion.
"""
import importlib.util
import os

import numpy as np
import pytest
import torch

import pair_counts_ref as R

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DRIVER = os.path.join(REPO, "stylegan-for-facerec_amd", "rb-webface", "scripts", "test_RB_Webface.py")


@pytest.fixture(scope="module")
def g16():
    return R.load_golden()


@pytest.fixture(scope="module")
def lattice(g16):
    return R.lattice_rows(g16["lattice_pos"], g16["lattice_sign"])


@pytest.fixture(scope="module")
def driver():
    spec = importlib.util.spec_from_file_location("rb_webface_driver", DRIVER)  # the directory name has a hyphen
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _gpu(E, thr, group=None):
    from frhip.pairwise import pair_counts
    c, seen = pair_counts(torch.from_numpy(np.ascontiguousarray(E)).cuda(), thr, group)
    assert c.dtype == torch.int64 and c.is_cuda
    return c.cpu().numpy(), seen


def test_lattice_equals_the_reference_exactly(g16, lattice):
    for thr, fmr, fnmr in ((g16["lattice_thr"], g16["lattice_fmr"], g16["lattice_fnmr"]),
                           (g16["lattice_thr_on"], g16["lattice_fmr_on"], g16["lattice_fnmr_on"])):  # ties are not counted
        c0, seen0 = _gpu(lattice, thr)
        c1, seen1 = _gpu(lattice, thr, R.GROUP)
        print("mode 0", c0.tolist(), seen0, "\nmode 1", c1.tolist(), seen1)
        assert seen0 == 179700 and seen1 == 1200
        assert np.array_equal(c0 / seen0, fmr) and np.array_equal(c1 / seen1, fnmr)


@pytest.mark.parametrize("m", [599, 257, 130, 129, 128, 6, 5, 2])
def test_leading_rows(g16, lattice, m):
    thr = g16["lattice_thr"]
    for group in (None, R.GROUP, 3, 16):
        want, seen = R.pair_counts_ref(lattice[:m], thr, group)
        got, gseen = _gpu(lattice[:m], thr, group)
        assert gseen == seen
        assert np.array_equal(got, want), (m, group, got.tolist(), want.tolist())


@pytest.mark.parametrize("T", [1, 17, 32, 33, 70])
def test_threshold_counts_and_the_split(lattice, T):
    thr = (np.arange(T) % 17 - 8 + 0.5) / 16.0 if T > 1 else np.array([0.5 / 16])
    for group in (None, R.GROUP):
        want, _ = R.pair_counts_ref(lattice, thr, group)
        got, _ = _gpu(lattice, thr, group)
        assert got.shape == (T,) and np.array_equal(got, want)


def test_row_pitch_scaling_and_other_widths(g16):
    """Unnormalised rows are normalised by the wrapper; D = 64, 100 (a partial k-chunk of the kernel's 32) and 2048."""
    pos, sign = g16["lattice_pos"], g16["lattice_sign"]
    thr = g16["lattice_thr"]
    for d in (64, 100, 2048):
        E = R.lattice_rows(pos[:300], sign[:300], d) * np.float32(4.0)
        want, _ = R.pair_counts_ref(E, thr)
        got, _ = _gpu(E, thr)
        assert np.array_equal(got, want), d
    from frhip import _lib
    from frhip.pairwise import pair_counts
    with pytest.raises(_lib.FrhipError):
        pair_counts(torch.zeros(8, 6, device="cuda"), [0.0])
    with pytest.raises(_lib.FrhipError):
        pair_counts(torch.zeros(1, 8, device="cuda"), [0.0])


def test_zero_row_is_seen_and_never_counted(lattice):
    E = lattice[:300].copy()
    E[7] = 0
    E[299] = 0
    for group, thr in ((None, [-2.0, 0.0, 2.0]), (R.GROUP, [-2.0, 0.0, 2.0])):
        want, seen = R.pair_counts_ref(E, thr, group)
        got, gseen = _gpu(E, thr, group)
        assert gseen == seen and np.array_equal(got, want)
    got, seen = _gpu(E, [-2.0])
    assert seen == 300 * 299 // 2 and got[0] == 298 * 297 // 2


def _bracket(X, thr, group, width):
    lo, seen = R.pair_counts_ref(X, thr + R.DELTA if group is None else thr - R.DELTA, group)
    hi, _ = R.pair_counts_ref(X, thr - R.DELTA if group is None else thr + R.DELTA, group)
    mid, _ = R.pair_counts_ref(X, thr, group)
    got, gseen = _gpu(X, thr, group)
    print("M %d group %s pairs %d\n  gpu    %s\n  c64    %s\n  lo     %s\n  hi     %s\n  width/pairs max %.4f %%"
          % (X.shape[0], group, seen, got.tolist(), mid.tolist(), lo.tolist(), hi.tolist(), 100.0 * (hi - lo).max() / seen))
    assert gseen == seen
    assert np.all(lo <= got) and np.all(got <= hi)
    if width:
        assert np.all(hi - lo <= 0.0025 * seen)
    return got


def test_bracket_on_the_golden_random_set(g16):
    X = R.random_rows(int(g16["random_seed"]), R.RANDOM_M)
    assert R.checksum(X) == g16["random_crc32"]
    thr = g16["random_thr"]
    # the float64 statement is the reference's on this set (tests/test_pair_counts_host.py pins all 20 rates)
    c, seen = R.pair_counts_ref(X, thr)
    assert np.array_equal(c / seen, g16["random_fmr"])
    _bracket(X, thr, None, width=True)
    _bracket(X, thr, R.GROUP, width=False)  # 2 000 pairs: see the module docstring


def test_bracket_determinism_and_memory_at_16421_rows():
    from frhip.pairwise import pair_counts
    X = R.random_rows(R.BIG_SEED, R.BIG_M)
    thr = np.linspace(-0.1, 0.1, 20)
    _bracket(X, thr, None, width=True)
    _bracket(X, thr, R.GROUP, width=True)
    xd = torch.from_numpy(X).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    a, _ = pair_counts(xd, thr)
    b, _ = pair_counts(xd, thr)
    a1, _ = pair_counts(xd, thr, R.GROUP)
    b1, _ = pair_counts(xd, thr, R.GROUP)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    print("peak device memory of the counting calls: %.1f MB (M x M x 4 = %.1f MB)" % (peak / 1e6, R.BIG_M ** 2 * 4 / 1e6))
    assert torch.equal(a, b) and torch.equal(a1, b1)
    assert peak < R.BIG_M * R.BIG_M * 4


def test_driver_rates_on_the_lattice(g16, lattice, driver):
    for src in (lattice, torch.from_numpy(lattice).cuda()):
        for i in (0, 5, 8, 12, 16):
            t = float(g16["lattice_thr"][i])
            assert driver.calc_FMR(src, t, n_jobs=1, batch_size=200) == g16["lattice_fmr"][i]
            assert driver.calc_FNMR(src, t, 5) == g16["lattice_fnmr"][i]
            t = float(g16["lattice_thr_on"][i])
            assert driver.calc_FMR(src, t) == g16["lattice_fmr_on"][i]
            assert driver.calc_FNMR(src, t, n_names_per_grp=5) == g16["lattice_fnmr_on"][i]


def _write_tree(tmp_path, n_pos=15, n_neg=24):
    """Small JPEGs (two sizes, so one batch is mixed) and the eight list files."""
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


def test_driver_end_to_end(tmp_path, driver, capsys):
    from PIL import Image
    from frhip import synth
    from util.utils import _from_uint8, l2_norm
    import configs.config_synthetic_smoke as smoke_cfg
    from train import build_backbone

    data, lists, names = _write_tree(tmp_path)
    config = smoke_cfg.__file__
    model = build_backbone(smoke_cfg.configurations[1])
    synth.fill_state_dict(model.state_dict(), 21)
    ckpt = str(tmp_path / "Backbone_test.pth")
    torch.save(model.state_dict(), ckpt)

    thr = np.linspace(-0.2, 0.9, 12)
    tpr3, tpr4 = driver.evaluate_model(config, ckpt, data, lists, gpu_batch_size=10, thresholds=thr, num_workers=0)
    out = capsys.readouterr().out
    assert sorted(tpr3) == sorted(tpr4) == ["African", "Asian", "Caucasian", "Indian"]
    assert out.count("TPR@FPR=1e-3") == 4 and out.count("TPR@FPR=1e-4") == 4

    backbone = driver.initialize_model(config, ckpt)
    for grp in tpr3:
        embs = {}
        for kind in ("pos", "neg"):
            emb = driver.calc_embeddings(backbone, names[(grp, kind)], data, batch_size=10, num_workers=0)
            assert emb.is_cuda and emb.shape == (len(names[(grp, kind)]), 512)
            # the same decoded images through the existing eval path, in the driver's batches: the reference's host transform
            # (PIL resize + centre crop, ToTensor / Normalize of util.utils), the backbone, l2_norm -- the same kernels on
            # the same input bits, so the same embeddings
            want = []
            with torch.no_grad():
                for k in range(0, len(names[(grp, kind)]), 10):
                    u8 = []
                    for n in names[(grp, kind)][k:k + 10]:
                        img = Image.open(os.path.join(data, n)).convert("RGB").resize((128, 128), Image.BILINEAR)
                        u8.append(torch.from_numpy(np.asarray(img.crop((8, 8, 120, 120))).copy()).permute(2, 0, 1))
                    want.append(l2_norm(backbone(_from_uint8(torch.stack(u8)).cuda()).float()))
            want = torch.cat(want)
            print(grp, kind, "max |emb - eval path| = %.3g" % float((emb - want).abs().max()))
            assert torch.equal(emb, want)
            embs[kind] = emb
        fmr, fnmr = driver.group_rates(embs["pos"], embs["neg"], thr, 5)
        E_neg, E_pos = embs["neg"].cpu().numpy(), embs["pos"].cpu().numpy()
        lo, seen = R.pair_counts_ref(E_neg, thr + R.DELTA)
        hi, _ = R.pair_counts_ref(E_neg, thr - R.DELTA)
        assert np.all(lo / seen <= fmr) and np.all(fmr <= hi / seen)
        lo, seen = R.pair_counts_ref(E_pos, thr - R.DELTA, 5)
        hi, _ = R.pair_counts_ref(E_pos, thr + R.DELTA, 5)
        assert np.all(lo / seen <= fnmr) and np.all(fnmr <= hi / seen)
        assert tpr3[grp] == 1 - np.interp(1e-3, list(fmr)[::-1], list(fnmr)[::-1])
        assert tpr4[grp] == 1 - np.interp(1e-4, list(fmr)[::-1], list(fnmr)[::-1])
