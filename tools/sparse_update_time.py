"""Time a whole training step of the class-sharded ArcFace head (world size 1) under class sampling -- zero_grad + forward +
backward + optimizer.step() with frhip.optim.SGD (momentum 0.9, weight decay 5e-4) -- with the default dense update and
with ``sparse_update=True``, modelled on tools/class_sample_time.py: per N and rate the two variants alternate in one
process, `rounds` x (`steps` steps per variant), event-timed after a warm-up of both.  Prints per case the median and the
spread (min .. max) of the rounds' ms per step, the ratio of the sparse median to the dense median OF THE SAME RUN, and
torch.cuda.max_memory_allocated() of each variant (profiles/sparse_update_b256.txt).  The dense variant is the baseline:
the code path the option leaves untouched, in the same tree and the same process.

    python tools/sparse_update_time.py [--batch 256] [--classes 28000 1000000] [--rates 0.5 0.1] [--steps 20] [--rounds 5]

The variants are built, measured and freed one pair at a time.  "peak memory" of a variant is
torch.cuda.max_memory_allocated() after a reset_peak_memory_stats() right before the variant is built, less what was
allocated at that moment (the inputs, and the dense variant while the sparse one is built): the variant's own weight,
momentum buffer, gradient (dense variant) and activations over its build and three warm-up steps.
The fr_sgd_rows kernel time comes from one `rocprofv3 --kernel-trace --stats` run of this script on its own
(`--rounds 1 --steps 10` keeps the trace small); no counters in that run.
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
from frhip.optim import SGD  # noqa: E402
from frhip.sharded_head import ShardedMarginLoss  # noqa: E402

VARIANTS = ("dense", "sparse")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, nargs="+", default=[28000, 1000000])
    ap.add_argument("--rates", type=float, nargs="+", default=[0.5, 0.1])
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B, D = a.batch, 512
    FRF.CHECK_LABELS = False  # as train.py: no host sync per call
    for N in a.classes:
        x = synth.normal(7, "sut.x", (B, D)).cuda()
        y = synth.labels(7, "sut.y", B, N).cuda()
        full = torch.empty(N, D).uniform_(-0.1, 0.1, generator=torch.Generator().manual_seed(7))
        for rate in a.rates:
            crits, opts, peak = {}, {}, {}

            def step(v):  # the order of train.py: forward, zero_grad, backward, step
                crit, opt = crits[v], opts[v]
                xx = x.detach().requires_grad_(True)
                loss, _p1, _p5 = crit(xx, y)
                opt.zero_grad()
                loss.backward()
                opt.step()

            def window(v):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    step(v)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / a.steps

            for v in VARIANTS:  # build + warm up one variant at a time: its peak is its own
                torch.cuda.synchronize()
                before = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                crits[v] = ShardedMarginLoss(D, N, "ArcFace", full_weight=full, sample_rate=rate, sample_seed=7,
                                             sparse_update=(v == "sparse")).cuda()
                opts[v] = SGD([{"params": [crits[v].weight], "weight_decay": 5e-4}], lr=0.1, momentum=0.9)
                for _ in range(3):
                    step(v)
                torch.cuda.synchronize()
                peak[v] = torch.cuda.max_memory_allocated() - before
            res = {v: [] for v in VARIANTS}
            for _ in range(a.rounds):
                for v in VARIANTS:
                    res[v].append(window(v))
            base = statistics.median(res["dense"])
            for v in VARIANTS:
                t = res[v]
                print("SPARSEUPDATETIME ArcFace B=%d N=%d rate %.1f (n_s %7d) %-6s  median %.3f ms/step  spread %.3f .. %.3f  "
                      "%.3f x dense  peak memory %.1f MB  (%d rounds x %d steps)" % (
                          B, N, rate, crits[v].n_s, v, statistics.median(t), min(t), max(t), statistics.median(t) / base,
                          peak[v] / 2.0 ** 20, a.rounds, a.steps), flush=True)
            del crits, opts
            torch.cuda.empty_cache()
        del full


if __name__ == "__main__":
    main()
