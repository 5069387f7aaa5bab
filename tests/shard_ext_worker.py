"""Worker for tests/test_gpu_sharded_heads_ext.py::test_two_ranks_sharing_one_gpu (torch.distributed.run, two ranks on GPU
0, ``gloo`` collectives on device tensors), modelled on tests/shard_worker.py.  Each rank feeds its own features / labels to
the class-sharded SphereFace, Am_softmax and CurricularFace (HIP kernels) for two consecutive steps; the expected values are
the REPLICATED HIP head + focal loss over the concatenated batch with the full parameter on the same GPU, and the head's
host path (fp32, CPU) on the same numbers."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))
sys.path.insert(0, HERE)

import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def rel(a, b):
    return float((a - b).norm() / b.norm())


def main():
    torch.cuda.set_device(0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    from frhip import synth
    from frhip.sharded_head import ShardedMarginLoss, class_range
    from head import metrics as H
    from loss.focal import FocalLoss
    from util.utils import accuracy
    from oracle import irse_ref as O
    import curricular_data as CD
    N, B, D = 1001, 12, 512
    for name in ("SphereFace", "Am_softmax", "CurricularFace"):
        cdim = 0 if name == "SphereFace" else 1
        if name == "CurricularFace":  # both label branches, hard and easy negatives
            xa, full, ya, _ = CD.built(synth, "shardext", world * B, D, N)
            CD.assert_covers_both_branches(xa, full, ya, 0.5)
            xs, labs = list(xa.split(B)), list(ya.split(B))
        else:
            full = synth.uniform(31, "shardext.w." + name, (N, D) if cdim == 0 else (D, N), -0.1, 0.1)
            xs = [synth.uniform(40 + r, "shardext.x", (B, D), -1.0, 1.0) for r in range(world)]
            labs = [synth.labels(40 + r, "shardext.y", B, N) for r in range(world)]
            labs[0][0], labs[-1][-1] = 0, N - 1
        crit = ShardedMarginLoss(D, N, name, gamma=2.0, full_weight=full).cuda()
        lo, hi = class_range(N, world, rank)
        shard = (lambda t: t[lo:hi]) if cdim == 0 else (lambda t: t[:, lo:hi])
        make = (lambda: H.CurricularFace(D, N)) if name == "CurricularFace" else (lambda: getattr(H, name)(D, N, None))
        head, host = make().cuda(), make()
        for h in (head, host):
            with torch.no_grad():
                list(h.parameters())[0].copy_(full)
        p, ph = list(head.parameters())[0], list(host.parameters())[0]
        yc = torch.cat(labs)
        for step in range(2):
            x = xs[rank].cuda().requires_grad_(True)
            crit.weight.grad = p.grad = ph.grad = None
            loss, p1, p5 = crit(x, labs[rank].cuda())
            loss.backward()
            # replicated head over the concatenated batch (HIP)
            xc = torch.cat(xs).cuda().requires_grad_(True)
            logits = head(xc, yc.cuda())
            floss, _ = FocalLoss()(logits, yc.cuda())
            floss.backward()
            e1, e5 = accuracy(logits.detach(), yc.cuda(), topk=(1, 5))
            tag = (name, "step", step)
            assert abs(float(loss.detach()) - float(floss)) <= 2e-6 * max(1.0, abs(float(floss))), tag + (
                float(loss.detach()), float(floss))
            assert float(p1) == float(e1) and float(p5) == float(e5), tag + (float(p1), float(e1), float(p5), float(e5))
            gx_e = xc.grad[rank * B:(rank + 1) * B] * world
            assert rel(x.grad, gx_e) < 1e-5, tag + ("gx", rel(x.grad, gx_e))
            assert rel(crit.weight.grad, shard(p.grad)) < 1e-5, tag + ("gw", rel(crit.weight.grad, shard(p.grad)))
            # the head's host path on the same numbers (fp32 CPU): the 1e-3 bar of the north star, gradients norm-wise
            xo = torch.cat(xs).clone().requires_grad_(True)
            lo_ = O.focal_loss(host(xo, yc), yc, 2)
            ogx, ogw = torch.autograd.grad(lo_, [xo, ph])
            assert abs(float(loss.detach()) - float(lo_)) < 1e-3, tag + (float(loss.detach()), float(lo_))
            assert rel(x.grad.cpu() / world, ogx[rank * B:(rank + 1) * B]) < 1e-3, tag + ("host gx",)
            assert rel(crit.weight.grad.cpu(), shard(ogw)) < 1e-3, tag + ("host gw",)
            # identical loss (and t) bits on every rank; the ragged gather restores the full parameter
            for v in (loss.detach(),) + ((crit.t,) if name == "CurricularFace" else ()):
                both = [torch.zeros_like(v) for _ in range(world)]
                dist.all_gather(both, v.clone())
                assert all(torch.equal(both[0], t) for t in both), tag
            if name == "CurricularFace":
                assert float(crit.t) != 0.0 and abs(float(crit.t) - float(host.t)) < 1e-6
            if name == "SphereFace":
                assert crit.iter == head.iter == step + 1
        assert torch.equal(crit.gather_weight().cpu(), full)
    dist.barrier()
    if rank == 0:
        print("SHARD_EXT_WORKER_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except Exception:  # noqa: BLE001 -- the launcher's summary hides the traceback
        import traceback
        print("SHARD_EXT_WORKER_FAILED\n" + traceback.format_exc(), flush=True)
        raise
