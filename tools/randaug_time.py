#!/usr/bin/env python3
"""Measure fr_randaug_u8 (RandAugment on the GPU input pipeline) on the GPU.

B = 256 images of 112x112, K = 6 operations per image drawn by GpuRandAugment from the served set, against fr_augment_u8 (the
resize / crop / flip / normalise launch that follows it) on the same batch.  The two alternate in one process; every round
times a run of launches of each with device events.  Reported: the median and the spread of the rounds and of the per-round
ratio, the share of a training step, and where the time goes: the same launch with six identity steps (the read, the write
and the launch itself) and with six steps of one operation each.

    python tools/randaug_time.py [--out FILE] [--rounds 9] [--launches 2000] [--step-ms 13.4]

Needs a GPU: there is no host fallback, and a time taken elsewhere would say nothing."""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from frhip import ops  # noqa: E402
from frhip.input_pipeline import RANDAUG_CODE, RANDAUG_RANGES, SERVED, GpuRandAugment, GpuTrainTransform  # noqa: E402

B, SIDE, K, SEED = 256, 112, 6, 900
LINES = []


def say(text=""):
    print(text, flush=True)
    LINES.append(text)


def spread(values, unit, scale=1.0):
    v = sorted(x * scale for x in values)
    return "median %.2f %s (min %.2f, max %.2f, %d rounds)" % (statistics.median(v), unit, v[0], v[-1], len(v))


def timed(launch, launches):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(launches):
        launch()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / launches * 1e3  # us per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--launches", type=int, default=2000)
    ap.add_argument("--step-ms", type=float, default=13.4, help="the training step the share is taken of")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("randaug_time: needs a GPU")
    say("# tools/randaug_time.py on %s, torch %s" % (torch.cuda.get_device_name(0), torch.__version__))
    dev = torch.device("cuda")
    gen = torch.Generator().manual_seed(SEED)
    tf, ra = GpuTrainTransform(SIDE), GpuRandAugment(num=K)
    u8 = torch.randint(0, 256, (B, SIDE, SIDE, 3), dtype=torch.uint8, device=dev)
    crop, flip = tf.draw(B, gen)
    crop, flip = crop.to(dev), flip.to(dev)
    op, par = ra.draw(B, gen, (SIDE, SIDE))
    xtab, ytab, lut, kx, ky = tf.tables(dev, SIDE, SIDE)
    staged, out = torch.empty_like(u8), torch.empty(B, 3, SIDE, SIDE, device=dev)
    stream = ops.current_stream_ptr()

    def randaug(op_host, par_host):
        o, p = op_host.to(dev), par_host.to(dev)
        return ops.call("fr_randaug_u8", u8, None, None, o, p, staged, None, B, B, int(o.shape[1]), SIDE, SIDE, stream)

    policy = randaug(op, par)
    sibling = ops.call("fr_augment_u8", u8, xtab, ytab, crop, flip, lut, out, B, SIDE, SIDE, tf.big, tf.big, SIDE, kx, ky,
                       stream)
    for _ in range(20):
        policy()
        sibling()
    torch.cuda.synchronize()
    first = staged.clone()
    policy()
    torch.cuda.synchronize()
    if not torch.equal(first, staged):
        sys.exit("randaug_time: two launches on the same inputs disagree")

    tr, ts = [], []
    for r in range(args.rounds):
        a, b = (policy, sibling) if r % 2 == 0 else (sibling, policy)
        ta, tb = timed(a, args.launches), timed(b, args.launches)
        tr.append(ta if r % 2 == 0 else tb)
        ts.append(tb if r % 2 == 0 else ta)
    med = statistics.median(tr)
    traffic = 2 * B * SIDE * SIDE * 3
    say("B = %d, %dx%d, K = %d operations per image drawn from the served set; %d launches per round, device events"
        % (B, SIDE, SIDE, K, args.launches))
    say("    fr_randaug_u8        : %s" % spread(tr, "us"))
    say("    fr_augment_u8        : %s   (the launch that follows it, on the same batch)" % spread(ts, "us"))
    say("    ratio randaug/augment: %s" % spread([a / b for a, b in zip(tr, ts)], "x"))
    say("    share of a %.1f ms step: %.2f %%" % (args.step_ms, med / (args.step_ms * 1e3) * 100))
    say("    traffic              : %.1f MB per batch (read once, written once) -> %.0f GB/s at the median"
        % (traffic / 1e6, traffic / med / 1e3))
    say("    two launches on the same inputs give the same bytes")
    say()
    say("where the time goes: the same launch with K = %d steps of one kind in every image (median of %d rounds of %d)"
        % (K, min(args.rounds, 5), args.launches // 4))
    kinds = [("identity (read, write, launch)", "equalize")] + [(n, n) for n in SERVED if n != "equalize"]
    floor = None
    for label, name in kinds:
        code = RANDAUG_CODE[name]
        values = np.full((B, K), float(np.asarray(RANDAUG_RANGES[name])[9]))
        p = GpuRandAugment.parameters(np.full((B, K), code), values, np.ones((B, K)), SIDE, SIDE)
        launch = randaug(torch.full((B, K), code, dtype=torch.uint8), torch.from_numpy(p))
        launch()
        torch.cuda.synchronize()
        t = statistics.median(timed(launch, args.launches // 4) for _ in range(min(args.rounds, 5)))
        floor = t if floor is None else floor
        say("    %-32s %7.2f us   %+6.2f us per step over the identity" % (label, t, (t - floor) / K))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
