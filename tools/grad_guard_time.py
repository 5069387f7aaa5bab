"""Time ``zero_grad`` + ``step`` of frhip.optim.SGD (momentum 0.9, weight decay 2e-3 off the batch-norm tensors) over the
parameter set of IR-50, its gradients in one arena, with the gradient guard off, in measure-only mode and with clipping, modelled on
tools/sparse_update_time.py: the variants alternate in one process, `rounds` x (`steps` steps per variant), event-timed
after a warm-up of all.  Prints per variant the median and the spread (min .. max) of the rounds' us per step and the ratio
to the "off" median OF THE SAME RUN, then fr_grad_sumsq on its own against its floor of 4 bytes per element at the
achievable HBM rate DESIGN.md uses (6.3 TB/s) and fr_grad_guard on its own (profiles/grad_guard_ir50.txt).

    python tools/grad_guard_time.py [--model IR_50] [--steps 50] [--rounds 7]

"off" is ``optimizer.step()``: the code path the guard leaves untouched.  For the unguarded step of a commit without the
guard on the same box, run this file against that commit's tree (``GRAD_GUARD_TIME_TREE=<its root>``): only the "off" line
is printed there, and it is the one to compare.
"""
import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.environ.get("GRAD_GUARD_TIME_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "stylegan-for-facerec_amd"), ROOT]
import torch  # noqa: E402
from backbone import model_irse  # noqa: E402
from frhip import _lib, ops  # noqa: E402
from frhip.optim import SGD  # noqa: E402
from util.utils import separate_irse_bn_paras  # noqa: E402

HBM_ACHIEVABLE = 6.3e12  # bytes/s, DESIGN.md section 2
VARIANTS = ("off", "measure", "clip")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="IR_50")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    have_guard = hasattr(_lib.lib, "fr_grad_sumsq")  # a parent library times the "off" variant alone
    model = getattr(model_irse, a.model)([112, 112]).cuda()
    # the gradients are views of one arena in the parameters' own memory layout, packed back to back, as the engine leaves
    # them: zero_grad is one fill, and a tensor starts wherever the one before it ended
    n_elem = sum(p.numel() for p in model.parameters())
    arena = torch.empty(n_elem, device="cuda").normal_(0.0, 1e-3, generator=torch.Generator(device="cuda").manual_seed(7))
    arena._frhip_grad_arena = True
    at = 0
    for p in model.parameters():
        p.grad = arena.as_strided(p.shape, p.stride(), at)
        at += p.numel()
    bn, wo = separate_irse_bn_paras(model)
    opts, guards = {}, {}
    for v in VARIANTS if have_guard else VARIANTS[:1]:
        opts[v] = SGD([{"params": wo, "weight_decay": 2e-3}, {"params": bn}], lr=1e-6, momentum=0.9)
        if v != "off":
            from frhip.optim import GradGuard
            guards[v] = GradGuard(model.parameters(), max_norm=1.0 if v == "clip" else None, skip_nonfinite=v == "clip")

    def step(v):
        opts[v].zero_grad()
        if v == "off":
            opts[v].step()
        else:
            guards[v].measure()
            opts[v].step(guard=guards[v])

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / n  # us per call

    for v in opts:
        for _ in range(3):
            step(v)
    torch.cuda.synchronize()
    res = {v: [] for v in opts}
    for _ in range(a.rounds):
        for v in opts:
            res[v].append(timed(lambda: step(v), a.steps))
    base = statistics.median(res["off"])
    tensors = sum(1 for _ in model.parameters())
    for v, t in res.items():
        print("GRADGUARDTIME %s (%d tensors, %.1f M elements) %-8s median %.1f us/step  spread %.1f .. %.1f  %.3f x off  "
              "+%.1f us  (%d rounds x %d steps)" % (a.model, tensors, n_elem / 1e6, v, statistics.median(t), min(t), max(t),
                                                    statistics.median(t) / base, statistics.median(t) - base, a.rounds,
                                                    a.steps), flush=True)
    if not have_guard:
        return
    g = guards["clip"]
    raw, ch, n, parts = g._table
    table = ctypes.cast(ctypes.c_void_p(raw.data_ptr()), ctypes.POINTER(_lib.FrGradTensor))
    st = ops.current_stream_ptr()
    sumsq = ops.Launch("fr_grad_sumsq", [table, ctypes.c_void_p(ch.data_ptr()), n, ops.ptr(parts), st])
    fin = ops.Launch("fr_grad_guard", [ops.ptr(parts), n, 1.0, 1, ops.ptr(g.ctl), ops.ptr(g.skipped), st])
    floor = 4.0 * n_elem / HBM_ACHIEVABLE * 1e6
    for name, launch in (("fr_grad_sumsq", sumsq), ("fr_grad_guard", fin)):
        t = [timed(launch, a.steps) for _ in range(a.rounds)]
        tail = ("  floor %.1f us (4 B/element at %.1f TB/s): %.2f x floor, %.2f TB/s" % (
            floor, HBM_ACHIEVABLE / 1e12, statistics.median(t) / floor, 4.0 * n_elem / statistics.median(t) / 1e6)
            if name == "fr_grad_sumsq" else "  (%d parts, one workgroup)" % n)
        print("GRADGUARDTIME %s %-14s back to back: median %.1f us/call  spread %.1f .. %.1f%s" % (
            a.model, name, statistics.median(t), min(t), max(t), tail), flush=True)


if __name__ == "__main__":
    main()
