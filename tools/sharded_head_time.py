"""Time forward + backward of the class-sharded SphereFace, Am_softmax and CurricularFace heads (world size 1) beside their
replicated heads + FocalLoss + accuracy, alternating the two in one process as tools/input_grad_time.py does: `rounds` x
(`steps` steps replicated, `steps` steps sharded), event-timed after a warm-up of both.  Prints per head and variant the
median and the spread (min .. max) of the rounds' ms per step (profiles/sharded_heads_ext_b256_n28000.txt).

    python tools/sharded_head_time.py [--batch 256] [--classes 28000] [--steps 20] [--rounds 5]
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
from head import metrics as H  # noqa: E402
from loss.focal import FocalLoss  # noqa: E402
from util.utils import accuracy  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--classes", type=int, default=28000)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    B, N, D = a.batch, a.classes, 512
    FRF.CHECK_LABELS = False  # as train.py: no host sync per call
    x = synth.normal(7, "sht.x", (B, D)).cuda()
    y = synth.labels(7, "sht.y", B, N).cuda()
    focal = FocalLoss()
    for name in ("SphereFace", "Am_softmax", "CurricularFace"):
        head = (H.CurricularFace(D, N) if name == "CurricularFace" else getattr(H, name)(D, N, None)).cuda()
        crit = ShardedMarginLoss.from_head(head).cuda()
        p = list(head.parameters())[0]

        def step(sharded):
            xx = x.detach().requires_grad_(True)
            if sharded:
                crit.weight.grad = None
                loss, _p1, _p5 = crit(xx, y)
            else:
                p.grad = None
                logits = head(xx, y)
                loss = focal(logits, y)[0]
                accuracy(logits.data, y, topk=(1, 5))
            loss.backward()

        def window(sharded):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                step(sharded)
            e1.record()
            torch.cuda.synchronize()
            return e0.elapsed_time(e1) / a.steps

        for w in (False, True, False, True):
            step(w)
        torch.cuda.synchronize()
        res = {False: [], True: []}
        for _ in range(a.rounds):
            for w in (False, True):
                res[w].append(window(w))
        for w in (False, True):
            v = res[w]
            print("SHARDEDHEADTIME %-14s B=%d N=%d %-22s median %.3f ms/step  spread %.3f .. %.3f  (%d rounds x %d steps)"
                  % (name, B, N, "sharded, world 1" if w else "replicated+focal+acc", statistics.median(v), min(v), max(v),
                     a.rounds, a.steps))


if __name__ == "__main__":
    main()
