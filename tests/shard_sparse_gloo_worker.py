"""Worker for tests/test_sparse_update_host.py::test_two_ranks_over_gloo_leave_row_gradients (torch.distributed.run, two
ranks on the CPU over ``gloo``, the oracle-backed stand-in kernels of tests/shard_ref*.py with the numpy class selection of
tests/class_sample_ref.py), written like tests/shard_sample_worker.py.  Every rank runs the sampled class-sharded head
twice over the same two steps, once as it is (the dense gradient of the shard's shape) and once with
``sparse_update=True``, for ArcFace / Focal and for Softmax / Softmax (weight and bias).  All comparisons are bit for bit:
the same stand-ins compute both variants, and the only difference is the scatter that the sparse variant leaves out.

    sparse variant     weight.grad (bias.grad) is None; ``_frhip_row_grad`` = (idx, rows) with idx the restated selection of
                       this rank and rows == the dense variant's grad[idx]; scatter_rows is never called
    dense variant      grad is exactly 0 outside idx
    both               the same loss bits and the same feature gradient; after a plain SGD step on each (the rows for the
                       sparse variant, the whole shard for the dense one: no decay, no momentum, where the two coincide) the
                       same weight bits, step after step"""
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

N, B, D, RATE, SEED, LR = 101, 5, 64, 0.4, 5, 0.05


def main():
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    import class_sample_ref as CS
    from frhip.sharded_head import ShardedMarginLoss, class_range, sampled_classes
    from shard_ref_ext import ExtOracleKernels
    from shard_ref_softmax import SoftmaxOracleKernels

    class Kernels(ExtOracleKernels, SoftmaxOracleKernels):
        pass

    lo, hi = class_range(N, world, rank)
    n = hi - lo
    for name, loss_name in (("ArcFace", "Focal"), ("Softmax", "Softmax")):
        g = torch.Generator().manual_seed(11)
        full = torch.randn(N, D, generator=g) * 0.3
        bias = torch.randn(N, generator=g) * 0.1 if name == "Softmax" else None
        Kd, Ks = CS.sampling_kernels(Kernels), CS.sampling_kernels(Kernels)
        make = lambda K, **kw: ShardedMarginLoss(D, N, name, full_weight=full, full_bias=bias, kernels=K, loss=loss_name,  # noqa: E731
                                                 sample_rate=RATE, sample_seed=SEED, **kw)
        dense, sparse = make(Kd), make(Ks, sparse_update=True)
        assert sparse.sparse_update and not dense.sparse_update
        params = ["weight"] + (["bias"] if bias is not None else [])
        for step in range(2):
            labs = [torch.randint(0, N, (B,), generator=g) for _ in range(world)]
            labs[0][0], labs[-1][0] = 0, N - 1
            xs = [torch.randn(B, D, generator=g) for _ in range(world)]
            lab_all = torch.cat(labs)
            local = torch.where((lab_all >= lo) & (lab_all < hi), lab_all - lo, torch.full_like(lab_all, -1)).numpy()
            idx, _, _ = CS.select(local, n, sampled_classes(RATE, n), CS.salt(SEED, step), lo)
            sel = torch.from_numpy(idx.astype(np.int64))
            unsel = torch.ones(n, dtype=torch.bool)
            unsel[sel] = False
            out = {}
            for crit in (dense, sparse):
                x = xs[rank].clone().requires_grad_(True)
                for k in params:
                    getattr(crit, k).grad = None
                loss, _p1, _p5 = crit(x, labs[rank])
                loss.backward()
                out[crit] = (loss.detach(), x.grad)
            tag = (name, "rank", rank, "step", step)
            assert torch.equal(out[dense][0], out[sparse][0]) and torch.equal(out[dense][1], out[sparse][1]), tag
            for k in params:
                pd, ps = getattr(dense, k), getattr(sparse, k)
                assert ps.grad is None, tag + (k, "the sparse variant formed a dense gradient")
                assert getattr(pd, "_frhip_row_grad", None) is None, tag + (k, "the dense variant left a row gradient")
                got_idx, rows = ps._frhip_row_grad
                assert got_idx.dtype == torch.int32 and np.array_equal(got_idx.numpy(), idx), tag + (k, "idx")
                assert tuple(rows.shape) == (idx.shape[0],) + tuple(pd.shape[1:]), tag + (k, tuple(rows.shape))
                assert torch.equal(rows, pd.grad[sel]), tag + (k, "rows != dense grad[idx]")
                assert bool((pd.grad[unsel] == 0).all()) and int(unsel.sum()) == n - idx.shape[0], tag + (k, "zeros")
                with torch.no_grad():  # what an optimizer without decay and momentum does with either form
                    pd -= LR * pd.grad
                    ps[sel] -= LR * rows
                ps._frhip_row_grad = None
                assert torch.equal(pd.detach(), ps.detach()), tag + (k, "weights after the step")
        assert Ks.calls["scatter_rows"] == 0 and Ks.calls["sample_classes"] == 2, Ks.calls
        assert Kd.calls["scatter_rows"] == 2 * len(params), Kd.calls
        assert torch.equal(dense.gather_weight(), sparse.gather_weight())  # collective
    dist.barrier()
    if rank == 0:
        print("SHARD_SPARSE_GLOO_WORKER_OK")
    dist.destroy_process_group()


if __name__ == "__main__":
    try:
        main()
    except Exception:  # noqa: BLE001 -- the launcher's summary hides the traceback
        import traceback
        print("SHARD_SPARSE_GLOO_WORKER_FAILED\n" + traceback.format_exc(), flush=True)
        raise
