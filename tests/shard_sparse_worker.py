"""Worker for tests/test_gpu_sparse_update.py::test_two_ranks_sharing_one_gpu (torch.distributed.run, two ranks on GPU 0,
``gloo`` collectives on device tensors unless FRHIP_SHARD_BACKEND says otherwise), modelled on tests/shard_sample_worker.py.
Each rank runs the class-sharded ArcFace (N = 193, so the shards are ragged: 97 and 96 classes) at sample_rate 0.25 on the HIP
kernels for two training steps, twice: as it is, and with ``sparse_update=True``, each under its own frhip.optim.SGD
(momentum 0.9, weight decay 1e-2).  Bit for bit on every rank:

    step 1 (zero momentum)   selected rows of weight and momentum: the two variants agree; unselected rows of the sparse
                             variant: the initial weight, zero momentum
    both steps               the sparse variant's weight and momentum are the restatement (tests/sparse_update_ref.py) driven
                             by the restated selection (tests/class_sample_ref.py) and the row gradients it left;
                             ``weight.grad`` stays None; both variants and both ranks see the same loss bits"""
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


def bits(t):
    return t.detach().cpu().numpy().view(np.int32)


def main():
    torch.cuda.set_device(0)
    dist.init_process_group(os.environ.get("FRHIP_SHARD_BACKEND", "gloo"))
    rank, world = dist.get_rank(), dist.get_world_size()
    import class_sample_ref as CS
    import sparse_update_ref as SU
    from frhip import synth
    from frhip.optim import SGD
    from frhip.sharded_head import ShardedMarginLoss, class_range, sampled_classes
    N, B, D, RATE, SEED, LR, MOM, WD = 193, 12, 512, 0.25, 77, 0.1, 0.9, 1e-2
    full = synth.uniform(31, "shardsparse.w", (N, D), -0.1, 0.1)
    lo, hi = class_range(N, world, rank)
    n = hi - lo
    n_s = sampled_classes(RATE, n)
    make = lambda **kw: ShardedMarginLoss(D, N, "ArcFace", gamma=2.0, full_weight=full, sample_rate=RATE, sample_seed=SEED,  # noqa: E731
                                          **kw).cuda()
    dense, sparse = make(), make(sparse_update=True)
    opts = {c: SGD([{"params": [c.weight], "weight_decay": WD}], lr=LR, momentum=MOM) for c in (dense, sparse)}
    p_ref, buf_ref = full[lo:hi].numpy().copy(), np.zeros((n, D), dtype=np.float32)
    for step in range(2):
        xs = [synth.uniform(40 + r + 10 * step, "shardsparse.x", (B, D), -1.0, 1.0) for r in range(world)]
        labs = [synth.labels(40 + r + 10 * step, "shardsparse.y", B, N) for r in range(world)]
        labs[0][0], labs[-1][-1] = 0, N - 1
        yc = torch.cat(labs)
        local = torch.where((yc >= lo) & (yc < hi), yc - lo, torch.full_like(yc, -1)).numpy()
        idx, _, _ = CS.select(local, n, n_s, CS.salt(SEED, step), lo)
        sel = torch.from_numpy(idx.astype(np.int64)).cuda()
        unsel = torch.ones(n, dtype=torch.bool, device="cuda")
        unsel[sel] = False
        tag = ("rank", rank, "step", step)
        losses = {}
        for crit in (dense, sparse):
            x = xs[rank].cuda().requires_grad_(True)
            loss, _p1, _p5 = crit(x, labs[rank].cuda())
            opts[crit].zero_grad()
            loss.backward()
            if crit is sparse:
                assert crit.weight.grad is None, tag + ("a dense gradient was formed",)
                got_idx, rows = crit.weight._frhip_row_grad
                assert np.array_equal(got_idx.cpu().numpy(), idx), tag + ("idx",)
                if step == 0:  # the same weights still: the rows are the dense variant's gradient rows
                    assert torch.equal(rows, dense.weight.grad[sel]), tag + ("rows != dense grad[idx]",)
                p_ref, buf_ref = SU.sgd_rows_ref(p_ref, buf_ref, rows.cpu().numpy(), idx, WD, MOM, LR)
            opts[crit].step()
            losses[crit] = loss.detach()
        torch.cuda.synchronize()
        assert torch.equal(losses[dense], losses[sparse]) or step > 0, tag  # after step 1 the two weights differ by design
        ws, bs = sparse.weight.detach(), opts[sparse].state[sparse.weight]["momentum_buffer"]
        assert sparse.weight.grad is None and sparse.weight._frhip_row_grad is None, tag
        assert np.array_equal(bits(ws), p_ref.view(np.int32)), tag + ("weight != restatement", int((bits(ws) != p_ref.view(np.int32)).sum()))
        assert np.array_equal(bits(bs), buf_ref.view(np.int32)), tag + ("momentum != restatement",)
        if step == 0:
            wd_, bd = dense.weight.detach(), opts[dense].state[dense.weight]["momentum_buffer"]
            assert np.array_equal(bits(ws[sel]), bits(wd_[sel])) and np.array_equal(bits(bs[sel]), bits(bd[sel])), tag
            assert np.array_equal(bits(ws[unsel]), bits(full[lo:hi].cuda()[unsel])) and not bool(bs[unsel].any()), tag
            assert not np.array_equal(bits(wd_[unsel]), bits(ws[unsel])), tag + ("the dense variant decays the unselected rows",)
        both = [torch.zeros_like(losses[sparse]) for _ in range(world)]
        dist.all_gather(both, losses[sparse].clone())
        assert all(torch.equal(both[0], t) for t in both), tag
    assert sparse.sample_step == 2
    dist.barrier()
    if rank == 0:
        print("SHARD_SPARSE_WORKER_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except Exception:  # noqa: BLE001 -- the launcher's summary hides the traceback
        import traceback
        print("SHARD_SPARSE_WORKER_FAILED\n" + traceback.format_exc(), flush=True)
        raise
