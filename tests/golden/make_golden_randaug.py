#!/usr/bin/env python3
"""Generate tests/golden/g28_randaugment.npz: the reference's Rand_Augment (data_processing/randaugment.py) on the
installed Pillow, on CPU.

Runs only in the build container, like its siblings (the reference is absent on the GPU box).  The reference's class runs
unpatched, with two loans from the maker: ``np.int = int`` (its ``ranges`` table uses the alias numpy 2 dropped) and an
import-only stand-in for matplotlib where that is not installed.  ``random.choice`` is replaced by a recorded sign
sequence while an operation runs, so the file holds the sign every output was made with.

Contents: ``transforms`` (the 13 names in order), ``numbers`` (default Numbers), ``max_magnitude``, ``ranges.<name>`` for
the 14 tables, two 16x12 RGB inputs (``in.random``; ``in.lowrange``, values 90..153), ``single.<input>.<op>`` uint8
[10 magnitudes, 2 signs (-1, +1), 16, 12, 3] for each served operation, and three chains of six served operations:
``chain.<i>.ops`` (names), ``.mags`` (magnitude indices), ``.signs``, ``.input`` (name) and ``.out``.

    python tests/golden/make_golden_randaug.py        # writes next to this file
"""
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = "/root/reference"
sys.path.insert(0, os.path.dirname(HERE))
from randaug_ref import SERVED, SIGNED  # noqa: E402
H, W = 16, 12


def reference_class():
    np.int = int
    try:
        import matplotlib.pyplot  # noqa: F401
    except Exception:  # noqa: BLE001 -- import-only stand-in: the class never plots
        mpl = types.ModuleType("matplotlib")
        mpl.pyplot = types.ModuleType("matplotlib.pyplot")
        sys.modules["matplotlib"], sys.modules["matplotlib.pyplot"] = mpl, mpl.pyplot
    sys.path.insert(0, REF)
    from data_processing.randaugment import Rand_Augment
    return Rand_Augment


class Signs(object):
    """Stands in for ``random.choice`` while one operation runs: hands out the recorded signs in order."""

    def __init__(self, signs):
        self.signs, self.taken = list(signs), 0

    def __call__(self, seq):
        assert list(seq) == [-1, 1], seq
        s = self.signs[self.taken]
        self.taken += 1
        return s


def with_signs(signs, fn):
    real, fake = random.choice, Signs(signs)
    random.choice = fake
    try:
        return fn(), fake.taken
    finally:
        random.choice = real


def g28_randaugment():
    ra = reference_class()()
    rng = np.random.RandomState(28)
    inputs = {"random": rng.randint(0, 256, (H, W, 3)).astype(np.uint8),
              "lowrange": rng.randint(90, 154, (H, W, 3)).astype(np.uint8)}
    out = {"transforms": np.array(ra.transforms), "numbers": np.array(ra.Numbers),
           "max_magnitude": np.array(ra.max_Magnitude)}
    for name, table in ra.ranges.items():
        out["ranges." + name] = np.asarray(table)
    for key, img in inputs.items():
        out["in." + key] = img
        for op in SERVED:
            res = np.empty((10, 2, H, W, 3), np.uint8)
            for m in range(10):
                for j, sign in enumerate((-1, 1)):
                    res[m, j], _ = with_signs([sign], lambda: ra.test_single_operation(img, op, m))
            out["single.%s.%s" % (key, op)] = res
    chains = [("random", ["color", "contrast", "translateX", "translateY", "autocontrast", "solarize"]),
              ("lowrange", ["brightness", "autocontrast", "contrast", "contrast", "posterize", "invert"]),
              ("random", ["translateY", "contrast", "equalize", "color", "brightness", "autocontrast"])]
    for i, (key, ops) in enumerate(chains):
        mags = rng.randint(1, 10, len(ops))
        signs = rng.choice([-1, 1], len(ops))
        plan = list(zip(ops, mags))
        ra.rand_augment = lambda plan=plan: plan  # the chain runs through the reference's __call__
        ra.Numbers = len(ops)
        res, taken = with_signs(list(signs) * 2, lambda: ra(inputs[key]))
        # a sign is consumed only by the operations that draw one: record the sign each step actually got
        got, at = [], 0
        for op in ops:
            if op in SIGNED:
                got.append(int((list(signs) * 2)[at]))
                at += 1
            else:
                got.append(0)
        assert at == taken, (at, taken)
        out["chain.%d.ops" % i] = np.array(ops)
        out["chain.%d.mags" % i] = np.asarray(mags, np.int64)
        out["chain.%d.signs" % i] = np.asarray(got, np.int64)
        out["chain.%d.input" % i] = np.array(key)
        out["chain.%d.out" % i] = res
    path = os.path.join(HERE, "g28_randaugment.npz")
    np.savez_compressed(path, **out)
    print("wrote %s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    g28_randaugment()
