"""Worker for tests/test_gpu_softmax.py::test_two_ranks_sharing_one_gpu (torch.distributed.run, two ranks on GPU 0, ``gloo``
collectives on device tensors), modelled on tests/shard_ext_worker.py.  Each rank feeds its own features / labels to the
class-sharded Softmax head, and to the class-sharded ArcFace, under ``loss="Softmax"`` (HIP kernels) for two steps; the
expected values are the REPLICATED HIP head + CrossEntropyLoss over the concatenated batch with the full parameters on the
same GPU, and the host expression (fp32, CPU) on the same numbers.  N = 1001 splits unevenly (501 / 500)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))
sys.path.insert(0, HERE)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def rel(a, b):
    return float((a - b).norm() / b.norm())


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from frhip import synth
    from frhip.sharded_head import ShardedMarginLoss, class_range
    from head import metrics as H
    from loss.softmax import CrossEntropyLoss
    from oracle import irse_ref as O
    from util.utils import accuracy
    N, B, D = 1001, 12, 512
    lo, hi = class_range(N, world, rank)
    for name in ("Softmax", "ArcFace"):
        full = synth.normal(31, "shardsm.w." + name, (N, D), std=0.2 if name == "Softmax" else 0.01)
        bias = synth.uniform(31, "shardsm.b", (N,)) if name == "Softmax" else None
        xs = [synth.uniform(40 + r, "shardsm.x", (B, D), -1.0, 1.0) for r in range(world)]
        labs = [synth.labels(40 + r, "shardsm.y", B, N) for r in range(world)]
        labs[0][0], labs[-1][-1] = 0, N - 1
        crit = ShardedMarginLoss(D, N, name, loss="Softmax", full_weight=full, full_bias=bias).cuda()
        head = H.Softmax(D, N, None) if name == "Softmax" else H.ArcFace(D, N, None)
        with torch.no_grad():
            head.weight.copy_(full)
            if bias is not None:
                head.bias.copy_(bias)
        head = head.cuda()
        pairs = list(zip(crit.parameters(), head.parameters()))
        assert len(pairs) == (2 if name == "Softmax" else 1)
        yc = torch.cat(labs)
        for step in range(2):
            x = xs[rank].cuda().requires_grad_(True)
            crit.zero_grad()
            head.zero_grad()
            loss, p1, p5 = crit(x, labs[rank].cuda())
            loss.backward()
            # replicated head over the concatenated batch (HIP)
            xc = torch.cat(xs).cuda().requires_grad_(True)
            logits = head(xc, yc.cuda())
            rloss = CrossEntropyLoss()(logits, yc.cuda())
            rloss.backward()
            e1, e5 = accuracy(logits.detach(), yc.cuda(), topk=(1, 5))
            tag = (name, "step", step)
            assert abs(float(loss.detach()) - float(rloss)) <= 2e-6 * max(1.0, abs(float(rloss))), tag + (
                float(loss.detach()), float(rloss))
            assert float(p1) == float(e1) and float(p5) == float(e5), tag + (float(p1), float(e1), float(p5), float(e5))
            gx_e = xc.grad[rank * B:(rank + 1) * B] * world
            assert rel(x.grad, gx_e) < 1e-5, tag + ("gx", rel(x.grad, gx_e))
            for pc, ph in pairs:
                assert rel(pc.grad, ph.grad[lo:hi]) < 1e-5, tag + ("g" + str(tuple(pc.shape)), rel(pc.grad, ph.grad[lo:hi]))
                assert rel(crit.gather_full(pc.grad), ph.grad) < 1e-5, tag + ("gathered",)
            # the host expression on the same numbers (fp32 CPU): the 1e-3 bar of the north star, gradients norm-wise
            xo = torch.cat(xs).clone().requires_grad_(True)
            hw = full.clone().requires_grad_(True)
            if name == "Softmax":
                hb = bias.clone().requires_grad_(True)
                lo_ = F.cross_entropy(F.linear(xo, hw, hb), yc)
                host = torch.autograd.grad(lo_, [xo, hw, hb])
            else:
                lo_ = F.cross_entropy(O.arcface_forward(xo, hw, yc, s=64.0, m=0.5, easy_margin=False), yc)
                host = torch.autograd.grad(lo_, [xo, hw])
            assert abs(float(loss.detach()) - float(lo_)) < 1e-3, tag + (float(loss.detach()), float(lo_))
            assert rel(x.grad.cpu() / world, host[0][rank * B:(rank + 1) * B]) < 1e-3, tag + ("host gx",)
            for (pc, _), want in zip(pairs, host[1:]):
                assert rel(pc.grad.cpu(), want[lo:hi]) < 1e-3, tag + ("host g" + str(tuple(pc.shape)),)
            both = [torch.zeros_like(loss.detach()) for _ in range(world)]
            dist.all_gather(both, loss.detach().clone())
            assert all(torch.equal(both[0], t) for t in both), tag
        assert torch.equal(crit.gather_weight().cpu(), full)
        if name == "Softmax":
            assert torch.equal(crit.gather_bias().cpu(), bias)
    dist.barrier()
    if rank == 0:
        print("SHARD_SOFTMAX_WORKER_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except Exception:  # noqa: BLE001 -- the launcher's summary hides the traceback
        import traceback
        print("SHARD_SOFTMAX_WORKER_FAILED\n" + traceback.format_exc(), flush=True)
        raise
