"""Time forward + backward of the class-sharded ArcFace head (world size 1) with class sampling at rates 1.0 / 0.5 / 0.1,
alternating the rates in one process as tools/sharded_head_time.py does: `rounds` x (`steps` steps per rate), event-timed
after a warm-up of all three.  Prints per N and rate the median and the spread (min .. max) of the rounds' ms per step and
the ratio of the median to that of rate 1.0 of the same run (profiles/class_sample_b256.txt).  Nothing else is a baseline:
a rate is compared with rate 1.0 of the same tree in the same process.

    python tools/class_sample_time.py [--batch 256] [--classes 28000 1000000] [--steps 20] [--rounds 5]

The kernel times of the selection launches come from one `rocprofv3 --kernel-trace --stats` run of this script on its own
(`--classes 28000 --rounds 1` keeps the trace small); no counters in that run.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stylegan-for-facerec_amd"), ROOT]
import torch  # noqa: E402
from frhip import functional as FRF  # noqa: E402
from frhip import synth  # noqa: E402
from frhip.sharded_head import ShardedMarginLoss  # noqa: E402

RATES = (1.0, 0.5, 0.1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, nargs="+", default=[28000, 1000000])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B, D = a.batch, 512
    FRF.CHECK_LABELS = False  # as train.py: no host sync per call
    for N in a.classes:
        x = synth.normal(7, "cst.x", (B, D)).cuda()
        y = synth.labels(7, "cst.y", B, N).cuda()
        full = torch.empty(N, D).uniform_(-0.1, 0.1, generator=torch.Generator().manual_seed(7))
        crits = {r: ShardedMarginLoss(D, N, "ArcFace", full_weight=full, sample_rate=r, sample_seed=7).cuda() for r in RATES}
        del full

        def step(rate):
            crit = crits[rate]
            xx = x.detach().requires_grad_(True)
            crit.weight.grad = None
            loss, _p1, _p5 = crit(xx, y)
            loss.backward()

        def window(rate):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(rate)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps

        for _ in range(2):
            for r in RATES:
                step(r)
        torch.cuda.synchronize()
        res = {r: [] for r in RATES}
        for _ in range(a.rounds):
            for r in RATES:
                res[r].append(window(r))
        base = statistics.median(res[1.0])
        for r in RATES:
            v = res[r]
            print("CLASSSAMPLETIME ArcFace B=%d N=%d rate %.1f (n_s %7d)  median %.3f ms/step  spread %.3f .. %.3f  "
                  "%.3f x rate 1.0  (%d rounds x %d steps)" % (B, N, r, crits[r].n_s, statistics.median(v), min(v), max(v),
                                                               statistics.median(v) / base, a.rounds, a.steps), flush=True)
        del crits
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
