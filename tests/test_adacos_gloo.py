"""AdaCos with ``process_group`` set, world 2 over ``gloo`` on the host path: each rank all-gathers its [2, B] row sums and
target cosines and reduces the gathered rows in rank order, so both ranks end with the scale of ONE head over the
concatenated batch (what the reference's nn.DataParallel shows its single head): B_avg over world * B rows and the median of
all ranks' target angles -- not the mean of the two local medians, nor of the two local scales."""
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

# the two-rank scale against the single head's: the same 8 x 100 terms added per row and then over the rows instead of in
# one sweep, a few fp32 roundings of a sum of ~800 positive terms; log() halves their relative weight again
BAR = 1e-6


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
        import math
        import adacos_data as AD
        from frhip import synth
        from head.metrics import AdaCos
        D, N = 512, 100
        (_, (x, W, label, _), branch, mid_gap), = AD.batches(synth, "built_even", D, N)
        B = x.shape[0] // world  # 4 rows per rank; the single head sees all 8
        # even rows to rank 0, odd rows to rank 1: local lower medians 0.6 and 0.3 rad, global 0.5 (the contiguous halves
        # have 0.4 and 0.6, whose mean happens to be the global one)
        order = torch.arange(world * B).view(B, world).t().reshape(-1)
        x, label = x[order], label[order]
        st = AD.assert_covers(x, W, label, AD.scale0(N), branch, mid_gap)

        def head_with(group):
            h = AdaCos(D, N)
            with torch.no_grad():
                h.W.copy_(W)
            h.process_group = group
            return h

        one, mine, alone = head_with(None), head_with(dist.group.WORLD), head_with(None)
        rows = slice(rank * B, (rank + 1) * B)
        for _ in range(2):  # the scale carries over from call to call
            want = one(x, label)
            got = mine(x[rows], label[rows])
            assert abs(float(mine.scale) / float(one.scale) - 1) <= BAR, (float(mine.scale), float(one.scale))
            # logits: the scale within BAR and cosines from GEMMs of different heights (a few fp32 roundings)
            torch.testing.assert_close(got, want[rows], rtol=0, atol=1e-4)
        assert abs(float(AdaCos(D, N).scale) - AD.scale0(N)) < 1e-6
        first = head_with(dist.group.WORLD)
        first(x[rows], label[rows])
        assert abs(float(first.scale) / st["scale"] - 1) <= BAR  # the global lower median (0.5 rad), float64 statistics
        alone(x[rows], label[rows])  # each half on its own, from the same initial scale
        ss = [torch.zeros(1) for _ in range(world)]
        dist.all_gather(ss, mine.scale)
        assert all(torch.equal(ss[0], s) for s in ss)  # the same bits on every rank
        # the stand-in: the mean of the two local scales (local medians, local B_avg) misses the bar
        local = [torch.zeros(1) for _ in range(world)]
        dist.all_gather(local, alone.scale)
        averaged = float(sum(local) / world)
        assert abs(averaged / st["scale"] - 1) > 100 * BAR, (averaged, st["scale"])
        # and so does the global B_avg with the mean of the two local medians
        c = torch.nn.functional.normalize(x.double()) @ torch.nn.functional.normalize(W.double()).t()
        th = torch.acos(c.gather(1, label.view(-1, 1)).view(-1).clamp(-1 + 1e-7, 1 - 1e-7))
        mean_med = sum(float(torch.median(th[r * B:(r + 1) * B])) for r in range(world)) / world
        wrong = math.log(st["b_avg"]) / math.cos(min(math.pi / 4, mean_med))
        assert abs(wrong / st["scale"] - 1) > 100 * BAR, (wrong, st["scale"], mean_med)
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


def test_two_ranks_hold_the_scale_of_one_head_over_the_global_batch():
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
