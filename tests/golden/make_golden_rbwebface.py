#!/usr/bin/env python3
"""Generate tests/golden/g16_rbwebface.npz: the reference's own calc_FMR / calc_FNMR
(rb-webface/scripts/test_RB_Webface.py:153-233) on the CPU, on two generated input sets.

Runs only in the build container, like make_golden.py (whose import-only stand-ins it reuses; the reference script also
imports skimage and torchvision.datasets without using them, so those get empty stand-ins here).  The script's directory
name has a hyphen, so it is loaded by file path.  The inputs are not stored in bulk: tests/pair_counts_ref.py regenerates
them (the tests do the same).

    python tests/golden/make_golden_rbwebface.py        # writes next to this file

Lattice set (exact): 600 rows of 16 non-zeros +-0.25 among the first 64 of 512 columns -- unit norm, every score a
  multiple of 1/16.  Stored: the positions and signs, thresholds (k + 0.5) / 16 between the lattice points and k / 16 ON
  them (k = -8 .. 8), and the reference's FMR (batch_size = 200) and FNMR (5 rows per person) at both.
Random set (bracketed): 1000 unit-norm fp32 rows by seed (stored: seed and CRC-32), 20 thresholds in [-0.1, 0.1] where
  their scores live, the reference's float64 rates.
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as MG  # noqa: E402  -- stand-ins for torchvision, imageio, ...
import pair_counts_ref as R  # noqa: E402


def load_reference_script():
    for name in ("skimage", "skimage.transform", "torchvision.datasets"):
        if name not in sys.modules:
            sys.modules[name] = types.ModuleType(name)
    sys.modules["torchvision"].datasets = sys.modules["torchvision.datasets"]
    sys.modules["skimage"].transform = sys.modules["skimage.transform"]
    path = os.path.join(MG.REF, "rb-webface", "scripts", "test_RB_Webface.py")
    spec = importlib.util.spec_from_file_location("ref_rb_webface", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def rates(ref, E, thresholds, batch_size):
    E = np.asarray(E, np.float64)
    fmr = np.array([ref.calc_FMR(E, t, n_jobs=1, batch_size=batch_size) for t in thresholds], np.float64)
    fnmr = np.array([ref.calc_FNMR(E, t, R.GROUP) for t in thresholds], np.float64)
    return fmr, fnmr


def main():
    ref = load_reference_script()
    out = {}

    pos, sign = R.lattice_draw()
    E = R.lattice_rows(pos, sign)
    assert np.all((E.astype(np.float64) ** 2).sum(1) == 1.0)
    k = np.arange(-8, 9, dtype=np.float64)
    thr_mid, thr_on = (k + 0.5) / 16.0, k / 16.0
    out["lattice_pos"], out["lattice_sign"] = pos, sign
    out["lattice_thr"], out["lattice_thr_on"] = thr_mid, thr_on
    out["lattice_fmr"], out["lattice_fnmr"] = rates(ref, E, thr_mid, 200)
    out["lattice_fmr_on"], out["lattice_fnmr_on"] = rates(ref, E, thr_on, 200)
    # the reference against a plain float64 upper-triangle count
    S = E.astype(np.float64) @ E.astype(np.float64).T
    iu = np.triu_indices(E.shape[0], 1)
    for t, r in zip(thr_mid, out["lattice_fmr"]):
        assert r == (S[iu] > t).sum() / iu[0].size
    print("lattice FMR  %.6g .. %.6g   FNMR %.6g .. %.6g" % (out["lattice_fmr"].max(), out["lattice_fmr"].min(),
                                                           out["lattice_fnmr"].min(), out["lattice_fnmr"].max()))

    X = R.random_rows(R.RANDOM_SEED, R.RANDOM_M)
    thr = np.linspace(-0.1, 0.1, 20)
    out["random_seed"] = np.int64(R.RANDOM_SEED)
    out["random_crc32"] = R.checksum(X)
    out["random_thr"] = thr
    out["random_fmr"], out["random_fnmr"] = rates(ref, X, thr, 200)
    out["group"] = np.int64(R.GROUP)

    np.savez_compressed(R.GOLDEN, **out)
    print("wrote %s (%d bytes)" % (R.GOLDEN, os.path.getsize(R.GOLDEN)))


if __name__ == "__main__":
    main()
