"""Worker for tests/test_gpu_class_sample.py::test_two_ranks_sharing_one_gpu (torch.distributed.run, two ranks on GPU 0,
``gloo`` collectives on device tensors unless FRHIP_SHARD_BACKEND says otherwise), modelled on tests/shard_ext_worker.py.
Each rank feeds its own features / labels to the class-sharded ArcFace with sample_rate 0.25 (HIP kernels) for two
consecutive steps.  Expected values: the float64 restatement of the full head on the concatenated batch, restricted to the
union of the classes the two ranks select (class_sample_ref.restricted_step, the selection restated in numpy); bars:
|d loss| < 1e-3, relative gradient error < 1e-3 (tests/test_gpu_sharded_heads_ext.py).  The unselected gradient rows are
exactly 0 and the loss bits are the same on both ranks."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402


def rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def main():
    torch.cuda.set_device(0)
    dist.init_process_group(os.environ.get("FRHIP_SHARD_BACKEND", "gloo"))
    rank, world = dist.get_rank(), dist.get_world_size()
    import class_sample_ref as CS
    from frhip import synth
    from frhip.sharded_head import ShardedMarginLoss, class_range, sampled_classes
    N, B, D, RATE, SEED = 1001, 12, 512, 0.25, 77
    full = synth.uniform(31, "shardsample.w", (N, D), -0.1, 0.1)
    xs = [synth.uniform(40 + r, "shardsample.x", (B, D), -1.0, 1.0) for r in range(world)]
    labs = [synth.labels(40 + r, "shardsample.y", B, N) for r in range(world)]
    labs[0][0], labs[-1][-1] = 0, N - 1
    crit = ShardedMarginLoss(D, N, "ArcFace", gamma=2.0, full_weight=full, sample_rate=RATE, sample_seed=SEED).cuda()
    lo, hi = class_range(N, world, rank)
    n = hi - lo
    yc = torch.cat(labs)
    for step in range(2):
        x = xs[rank].cuda().requires_grad_(True)
        crit.weight.grad = None
        loss, _p1, _p5 = crit(x, labs[rank].cuda())
        loss.backward()
        cols, mine = [], None
        for r in range(world):
            rlo, rhi = class_range(N, world, r)
            local = torch.where((yc >= rlo) & (yc < rhi), yc - rlo, torch.full_like(yc, -1)).numpy()
            idx, _, _ = CS.select(local, rhi - rlo, sampled_classes(RATE, rhi - rlo), CS.salt(SEED, step), rlo)
            if r == rank:
                mine = (len(cols), idx)
            cols += [rlo + int(c) for c in idx]
        e_loss, e_gx, e_gw, _ = CS.restricted_step("ArcFace", full, None, torch.cat(xs), yc, cols, step, "Focal", 2.0)
        at, idx = mine
        sel = torch.from_numpy(idx.astype(np.int64))
        gw = crit.weight.grad.cpu()
        unsel = torch.ones(n, dtype=torch.bool)
        unsel[sel] = False
        tag = ("rank", rank, "step", step)
        print("rank %d step %d: loss %.6f expected %.6f  gx %.2e  gw %.2e" % (
            rank, step, float(loss.detach()), float(e_loss), rel(x.grad.cpu() / world, e_gx[rank * B:(rank + 1) * B]),
            rel(gw[sel], e_gw[at:at + idx.shape[0]])), flush=True)
        assert abs(float(loss.detach()) - float(e_loss)) < 1e-3, tag + (float(loss.detach()), float(e_loss))
        assert rel(x.grad.cpu() / world, e_gx[rank * B:(rank + 1) * B]) < 1e-3, tag + ("gx",)
        assert rel(gw[sel], e_gw[at:at + idx.shape[0]]) < 1e-3, tag + ("gw",)
        assert bool((gw[unsel] == 0).all()) and int(unsel.sum()) == n - idx.shape[0], tag + ("unselected rows",)
        both = [torch.zeros_like(loss.detach()) for _ in range(world)]
        dist.all_gather(both, loss.detach().clone())
        assert all(torch.equal(both[0], t) for t in both), tag
    assert crit.sample_step == 2 and torch.equal(crit.gather_weight().cpu(), full)
    dist.barrier()
    if rank == 0:
        print("SHARD_SAMPLE_WORKER_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except Exception:  # noqa: BLE001 -- the launcher's summary hides the traceback
        import traceback
        print("SHARD_SAMPLE_WORKER_FAILED\n" + traceback.format_exc(), flush=True)
        raise
