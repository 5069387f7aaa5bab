#!/usr/bin/env python3
"""Time the radix select behind the exact threshold at a chosen FPR: fr_pair_hist and frhip.pairwise.score_at_rank.

    python tools/pair_select_time.py [--reps 20] [--sizes 8192 32768 65536]

One process, one GPU, HIP events, D = 512, unit-norm Gaussian rows from frhip/synth.py (impostor cosines: sigma = 0.044, the
concentrated case for the histogram's LDS adds).  Per M, after 3 warm-up calls, ``--reps`` calls are timed one by one and
median, minimum and maximum are printed for

* one fr_pair_hist call (tile kernel + the sum of the partials) at each of the three passes of the select, with the windows
  score_at_rank descends through for the rank of FPR = 1e-4: shift 21 / 2048 bins, shift 10 / 2048 bins, shift 0 / 1024 bins;
* the whole score_at_rank (row normalisation, three passes, three read-backs), timed on the host clock around a
  synchronising call;
* fr_pair_counts at T = 20 and T = 1 on the same rows: the yardstick, measured in the same run.

A tool, not a yardstick: nothing reads its output.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))

from frhip import ops, pairwise, synth  # noqa: E402
from frhip._lib import lib  # noqa: E402

D = 512


def rows(m):
    """(x, xn): the Gaussian rows and what score_at_rank makes of them before its first pass."""
    x = synth.normal(1603, "pair_counts_time.rows", (m, D)).cuda()
    return x, pairwise._unit_rows(x, "pair_select_time", lib.fr_pair_hist_parts, None)[0]


def timed(launch, reps):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def hist_launch(xn, key_lo, shift, bins):
    m = xn.shape[0]
    parts = lib.fr_pair_hist_parts(m, 0, 0)
    partials = torch.empty(parts * (bins + 2), dtype=torch.int32, device="cuda")
    hist = torch.empty(bins + 2, dtype=torch.int64, device="cuda")
    return ops.call("fr_pair_hist", xn, D, m, D, key_lo, shift, bins, 0, 0, partials, hist, ops.current_stream_ptr()), hist


def counts_launch(xn, thr):
    m, T = xn.shape[0], thr.numel()
    partials = torch.empty(lib.fr_pair_counts_parts(m, 0, 0) * T, dtype=torch.int32, device="cuda")
    counts = torch.empty(T, dtype=torch.int64, device="cuda")
    return ops.call("fr_pair_counts", xn, D, m, D, thr, T, 0, 0, partials, counts, ops.current_stream_ptr())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 32768, 65536])
    ap.add_argument("--fpr", type=float, default=1e-4)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pair_select_time.py needs a GPU"
    print("device: %s   D = %d   reps = %d (after 3 warm-up calls)   library: %s"
          % (torch.cuda.get_device_name(0), D, args.reps, os.environ.get("FRHIP_LIB", "libfrhip.so")))
    thr20 = torch.linspace(0.3, 0.6, 20, device="cuda")
    for m in args.sizes:
        x, xn = rows(m)
        pairs = m * (m - 1) // 2
        k = int(args.fpr * pairs)
        yard = {}
        for tag, thr in (("T=20", thr20), ("T=1", thr20[:1].clone())):
            yard[tag] = timed(counts_launch(xn, thr), args.reps)
            print("M = %6d  fr_pair_counts %-28s median %8.3f ms  (min %8.3f  max %8.3f)" % ((m, tag) + yard[tag]))
        # the windows of the select for rank k, found by the select itself
        windows = []

        def spy(key_lo, shift, bins):
            windows.append((key_lo, shift, bins))
            launch, hist = hist_launch(xn, key_lo, shift, bins)
            launch()
            return hist.cpu().numpy()

        t, above = pairwise.select_rank(spy, k)
        for key_lo, shift, bins in windows:
            launch, hist = hist_launch(xn, key_lo, shift, bins)
            med, lo, hi = timed(launch, args.reps)
            h = hist.cpu().numpy()
            print("M = %6d  fr_pair_hist   shift %2d bins %4d key_lo %08x  median %8.3f ms  (min %8.3f  max %8.3f)  %.2f x counts T=20"
                  "   [%d of %d bins occupied; the fullest slot, below / above the window included, holds %.1f %% of the pairs]"
                  % (m, shift, bins, key_lo, med, lo, hi, med / yard["T=20"][0], int((h[1:-1] > 0).sum()), bins,
                     100.0 * h.max() / pairs))
        wall = []
        for _ in range(3 + args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            t2, above2 = pairwise.score_at_rank(x, k)
            wall.append((time.perf_counter() - t0) * 1e3)
        wall = wall[3:]
        assert t2 == t and above2 == above
        print("M = %6d  score_at_rank  k = %d (FPR %g): t = %.9g, %d scores above   median %8.3f ms  (min %8.3f  max %8.3f), host clock"
              % (m, k, args.fpr, t, above, statistics.median(wall), min(wall), max(wall)))
        del x, xn


if __name__ == "__main__":
    main()
