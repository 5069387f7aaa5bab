"""Time forward + backward of the SST_Prototype head (B = 256 identities, two views: 512 probe rows against a queue of Q
columns) beside the AM_Softmax head at N = Q classes on 256 rows, alternating the two in one process: `rounds` x (`steps`
steps per head), event-timed after a warm-up of both.  The AM_Softmax head runs half the cosine rows, but also normalises
and repacks its [512, N] weight and forms a weight gradient; SST_Prototype does neither.  Prints per head the median and
the spread (min .. max) of the rounds' ms per step and the ratio of the medians (profiles/sst_prototype_b256_q16384.txt).

    python tools/sst_time.py [--batch 256] [--queue 16384] [--steps 20] [--rounds 5]

The kernel-time breakdown comes from one `rocprofv3 --kernel-trace --stats` run of this script on its own (`--rounds 1`
keeps the trace small); no counters in that run.
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
from head.metrics import AM_Softmax, SST_Prototype  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--queue", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B, Q, D = a.batch, a.queue, 512
    if not torch.cuda.is_available():
        raise SystemExit("tools/sst_time.py measures on a GPU; none is available")
    FRF.CHECK_LABELS = False  # as train.py: no host sync per call
    p = synth.normal(7, "sst.p", (2 * B, D)).cuda()
    g = (p + 0.3 * synth.normal(7, "sst.g", (2 * B, D)).cuda()).detach()
    ids = torch.arange(B, dtype=torch.int64).cuda()
    sst = SST_Prototype(D, Q, loss_type="am_softmax", margin=0.35).cuda()
    am = AM_Softmax(D, Q).cuda()
    y = synth.labels(7, "sst.y", B, Q).cuda()
    g1 = torch.ones(B, Q, device="cuda")

    def step_sst():
        x = p.detach().requires_grad_(True)
        o1, o2, _label, _ids = sst(x[:B], g[B:], x[B:], g[:B], ids)
        torch.autograd.backward([o1, o2], [g1, g1])

    def step_am():
        x = p[:B].detach().requires_grad_(True)
        am.weight.grad = None
        am(x, y).backward(g1)

    steps = {"SST_Prototype": step_sst, "AM_Softmax": step_am}

    def window(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    for _ in range(3):
        for fn in steps.values():
            fn()
    torch.cuda.synchronize()
    res = {name: [] for name in steps}
    for _ in range(a.rounds):
        for name, fn in steps.items():
            res[name].append(window(fn))
    for name, v in res.items():
        print("SSTTIME %-13s B=%d %s=%d  median %.3f ms/step  spread %.3f .. %.3f  (%d rounds x %d steps)"
              % (name, B, "Q" if name == "SST_Prototype" else "N", Q, statistics.median(v), min(v), max(v), a.rounds,
                 a.steps), flush=True)
    print("SSTTIME ratio SST_Prototype / AM_Softmax  %.3f" % (statistics.median(res["SST_Prototype"])
                                                               / statistics.median(res["AM_Softmax"])), flush=True)


if __name__ == "__main__":
    main()
