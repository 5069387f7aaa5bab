"""CurricularFace with ``process_group`` set, world 2 over ``gloo`` on the host path: the batch mean of the target cosines
is averaged over the ranks before it enters ``t``, so both ranks end with the ``t`` of ONE head over the concatenated batch
(what the reference's nn.DataParallel shows its single head), and each rank's logits are that head's rows."""
import os
import socket
import sys

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (HERE, REPO, os.path.join(REPO, "stylegan-for-facerec_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import curricular_data as CD
        from frhip import synth
        from head.metrics import CurricularFace
        B, D, N = 6, 64, 80  # per-rank batch; the single head sees world * B rows
        # rows 3, 7, 11 of the built batch have target cosines near -1: one in the first half, two in the second
        x, k, label, _ = CD.built(synth, "gloo", world * B, D, N)

        def head_with(t0, group):
            h = CurricularFace(D, N)
            with torch.no_grad():
                h.kernel.copy_(k)
                h.t.fill_(t0)
            h.process_group = group
            return h

        one, mine, alone = head_with(0.2, None), head_with(0.2, dist.group.WORLD), head_with(0.2, None)
        rows = slice(rank * B, (rank + 1) * B)
        for _ in range(2):  # t carries over from call to call
            want = one(x, label)
            got = mine(x[rows], label[rows])
            alone(x[rows], label[rows])
            # the mean of two equal-sized halves' means against the mean of the whole: one fp32 rounding apart at most
            assert abs(float(mine.t) - float(one.t)) <= 2e-7 * abs(float(one.t)), (float(mine.t), float(one.t))
            # logits: cosines from GEMMs of different heights (a few fp32 roundings, 64 * (t + 2c) <= 150 times that each)
            torch.testing.assert_close(got, want[rows], rtol=0, atol=1e-4)
        ts = [torch.zeros(1) for _ in range(world)]
        dist.all_gather(ts, mine.t)
        assert all(torch.equal(ts[0], t) for t in ts)  # the same bits on every rank
        # the halves differ, so a head without the group ends somewhere else
        assert abs(float(alone.t) - float(one.t)) > 1e-3, (float(alone.t), float(one.t))
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_t_of_one_head_over_the_global_batch():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
    for rank, msg in res:
        assert msg == "ok", "rank %d: %s" % (rank, msg)
