"""Time a backbone step (forward + backward, every parameter training) with and without gradients with respect to the
input images, alternating the two in one process: `rounds` x (`steps` steps without, `steps` steps with), event-timed
after a warm-up of both.  Prints per variant the median and the spread (min .. max) of the rounds' ms per step, and the
median extra cost.  Run it under `rocprofv3 --kernel-trace --stats -- ...` for the kernel times
(profiles/input_grad_*.txt); --size other than 112 makes pSp resize its input (fr_resize_bilinear and its adjoint).

    python tools/input_grad_time.py --model {IR_50|pSp} [--batch 256] [--dtype bf16] [--steps 10] [--rounds 5] [--size 112]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stylegan-for-facerec_amd"), ROOT]
import torch  # noqa: E402
from frhip import synth  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="IR_50", choices=["IR_50", "pSp"])
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--dtype", default="bf16", choices=["bf16", "f32"])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--size", type=int, default=112)
    a = ap.parse_args()
    if a.model == "IR_50":
        from backbone.model_irse import IR_50
        model = IR_50([112, 112])
        inner = model
    else:
        from backbone.restyle_psp import pSp
        model = pSp(size=112, checkpoint_path=None, avg_image=synth.uniform(15, "avg_image", (3, 112, 112)),
                    include_dropout=False)
        inner = model.encoder
    synth.fill_state_dict(model.state_dict(), 15)
    inner.compute_dtype = torch.bfloat16 if a.dtype == "bf16" else torch.float32
    model = model.cuda().train()
    x = synth.uniform(7, "igt.x", (a.batch, 3, a.size, a.size)).cuda()
    g = synth.normal(7, "igt.g", (a.batch, 512)).cuda()
    params = list(model.parameters())

    def step(with_grad):
        xx = x.detach().requires_grad_(with_grad)
        for p in params:
            p.grad = None
        (model(xx) * g).sum().backward()

    def window(with_grad):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            step(with_grad)
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
    extra = [b - c for c, b in zip(res[False], res[True])]
    tag = "%s bs%d %s size %d" % (a.model, a.batch, a.dtype, a.size)
    for w in (False, True):
        v = res[w]
        print("INPUTGRAD %s %-18s median %.3f ms/step  spread %.3f .. %.3f  (%d rounds x %d steps)"
              % (tag, "with x.grad" if w else "without", statistics.median(v), min(v), max(v), a.rounds, a.steps))
    print("INPUTGRAD %s extra per step: median %+.3f ms  spread %+.3f .. %+.3f" % (tag, statistics.median(extra), min(extra),
                                                                                  max(extra)))


if __name__ == "__main__":
    main()
