#!/usr/bin/env python3
"""Time fr_pair_counts (RB-WebFace impostor tallies, mode 0) on one GPU and the host procedure it replaces.

    python tools/pair_counts_time.py [--reps 20] [--host-m 8192]

GPU: HIP-event time of one fr_pair_counts call (tile kernel + the sum of the partials; the row normalisation is done once,
outside the timed window) at M = 8 192, 32 768, 65 536, D = 512 on unit-norm rows from frhip/synth.py, T = 20 and T = 1
(the difference is what the threshold comparisons of the epilogue cost).  After 3 warm-up calls, ``--reps`` calls are timed
one by one; median, minimum and maximum are printed, with pairs/s and TFLOP/s (2 D flops per pair) against the 157.3 TFLOP/s
f32 matrix peak of the MI355X.  Mode 1 (genuine pairs, 5 rows per person) is timed at M = 65 536 for the record.
Host: the reference's procedure for ONE threshold -- float64 scipy ``cdist(chunk, all, 'cosine')`` per chunk of 1 024 rows,
upper-trapezoid mask, count -- in 16 joblib workers, at M = ``--host-m``.  The reference repeats it for each of 20 thresholds.
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

from frhip import ops, synth  # noqa: E402
from frhip._lib import FR_F32, lib  # noqa: E402

PEAK_TFLOPS = 157.3
D = 512


def unit_rows(m):
    x = synth.normal(1603, "pair_counts_time.rows", (m, D)).cuda()
    xn = torch.empty_like(x)
    inv = torch.empty(m, device="cuda")
    ops.call("fr_row_normalize", x, xn, None, inv, m, m, D, 0, FR_F32, ops.current_stream_ptr())()
    return xn


def time_gpu(xn, thr, mode, group, reps):
    m = xn.shape[0]
    T = thr.numel()
    parts = lib.fr_pair_counts_parts(m, mode, group)
    partials = torch.empty(parts * T, dtype=torch.int32, device="cuda")
    counts = torch.empty(T, dtype=torch.int64, device="cuda")
    launch = ops.call("fr_pair_counts", xn, D, m, D, thr, T, mode, group, partials, counts, ops.current_stream_ptr())
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
    return statistics.median(ms), min(ms), max(ms), counts.cpu()


def host_chunk(E, i, batch, t):
    from scipy.spatial.distance import cdist
    S = 1 - cdist(E[i:i + batch], E, metric="cosine")
    rows = np.arange(S.shape[0])[:, None] + i
    s = S[np.arange(S.shape[1])[None, :] > rows]
    return int((s > t).sum()), s.size


def time_host(m, t, jobs=16, batch=1024):
    from joblib import Parallel, delayed
    E = synth.normal(1603, "pair_counts_time.rows", (m, D)).numpy().astype(np.float64)
    t0 = time.perf_counter()
    res = Parallel(n_jobs=jobs)(delayed(host_chunk)(E, i, batch, t) for i in range(0, m, batch))
    dt = time.perf_counter() - t0
    return dt, sum(r[0] for r in res), sum(r[1] for r in res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-m", type=int, default=8192)
    ap.add_argument("--sizes", type=int, nargs="+", default=[8192, 32768, 65536])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pair_counts_time.py needs a GPU"
    print("device: %s   D = %d   reps = %d (after 3 warm-up calls)   peak f32 matrix = %.1f TFLOP/s"
          % (torch.cuda.get_device_name(0), D, args.reps, PEAK_TFLOPS))
    thr20 = torch.linspace(0.3, 0.6, 20, device="cuda")
    thr_lo = torch.linspace(-0.1, 0.1, 20, device="cuda")
    for m in args.sizes:
        xn = unit_rows(m)
        pairs = m * (m - 1) // 2
        for tag, thr in (("T=20", thr20), ("T=1 ", thr20[:1].clone()), ("T=20 thresholds in [-0.1, 0.1]", thr_lo)):
            med, lo, hi, _c = time_gpu(xn, thr, 0, 0, args.reps)
            print("mode 0  M = %6d  %-32s median %8.3f ms  (min %8.3f  max %8.3f)  %7.2f G pairs/s  %6.1f TFLOP/s = %4.1f %% of peak"
                  % (m, tag, med, lo, hi, pairs / med / 1e6, 2 * D * pairs / med / 1e9, 100 * 2 * D * pairs / med / 1e9 / PEAK_TFLOPS))
        if m == args.sizes[-1]:
            med, lo, hi, _c = time_gpu(xn, thr20, 1, 5, args.reps)
            print("mode 1  M = %6d  T=20 group=5                       median %8.3f ms  (min %8.3f  max %8.3f)" % (m, med, lo, hi))
        if m == args.host_m:
            _med, _lo, _hi, c = time_gpu(xn, thr_lo[10:11].clone(), 0, 0, 1)
            t = float(thr_lo[10])
            dt, cnt, seen = time_host(m, t)
            print("host    M = %6d  one threshold, float64 cdist in 16 workers: %8.3f s  (count %d of %d pairs; GPU fp32 count %d)"
                  % (m, dt, cnt, seen, int(c[0])))
        del xn


if __name__ == "__main__":
    main()
