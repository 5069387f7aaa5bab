"""The class-sharded Softmax head and ``loss="Softmax"`` (frhip/sharded_head.py) on the CPU at world size 2 over ``gloo``: the
whole choreography with tests/shard_ref_softmax.py standing in for the HIP kernels.

Expected values: one process on the concatenated batch with the full parameters -- ``head.metrics.Softmax`` (its host path,
F.linear, pinned to the reference by g25) or the oracle's ArcFace, then ``F.cross_entropy`` and ``oracle.irse_ref
.topk_accuracy``; gradients by autograd.  N = 33 splits unevenly (17 / 16), N = 100 evenly.

Bars (those of tests/test_sharded_head_gloo.py): loss 1e-5 relative, precision equal, x.grad / world, the weight-shard and
the bias-shard gradients rtol 1e-4 / atol 1e-6, the loss bits equal on all ranks; the gathered gradients of the weight and
the bias meet the same bar against the full ones.

Negative controls: every rank adding the FIRST hi - lo entries of the full bias misses the loss bar; a focal slope left in
the backward pass meets the loss bar and misses the gradient bars."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (HERE, REPO, os.path.join(REPO, "stylegan-for-facerec_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

D, B, WORLD = 64, 5, 2


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _labels(g, N):
    """Per-rank labels: class 0 and class N - 1 forced, and on every rank a row whose label the other rank owns."""
    from frhip.sharded_head import class_range
    labs = [torch.randint(0, N, (B,), generator=g) for _ in range(WORLD)]
    for r in range(WORLD):
        lo, hi = class_range(N, WORLD, (r + 1) % WORLD)
        labs[r][-1] = lo + (hi - lo) // 2
    labs[0][0], labs[-1][0] = 0, N - 1
    return labs


def _loss_ok(loss, e_loss):
    return abs(float(loss) - float(e_loss)) < 1e-5 * max(1.0, abs(float(e_loss)))


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-4, atol=1e-6)


def _all_equal_bits(t):
    got = [torch.zeros_like(t) for _ in range(WORLD)]
    dist.all_gather(got, t.detach().clone())
    return all(torch.equal(got[0], v) for v in got)


def _expected(name, full_w, full_b, xs, labs):
    """(loss, gx, gw, gb or None, prec@1, prec@5) of one process on the concatenated batch."""
    from oracle import irse_ref as O
    x = torch.cat(xs).clone().requires_grad_(True)
    lab = torch.cat(labs)
    w = full_w.clone().requires_grad_(True)
    if name == "Softmax":
        from head.metrics import Softmax
        head = Softmax(D, full_w.shape[0], None)
        with torch.no_grad():
            head.weight.copy_(full_w)
            head.bias.copy_(full_b)
        logits = head(x, lab)
        loss = F.cross_entropy(logits, lab)
        gx, gw, gb = torch.autograd.grad(loss, [x, head.weight, head.bias])
    else:
        logits = O.arcface_forward(x, w, lab, s=64.0, m=0.5, easy_margin=False)
        loss = F.cross_entropy(logits, lab)
        (gx, gw), gb = torch.autograd.grad(loss, [x, w]), None
    p1, p5 = O.topk_accuracy(logits.detach(), lab)
    return loss.detach(), gx, gw, gb, float(p1), float(p5)


def _run(name, rank, N, kernels=None, wrong_bias=False):
    """Two steps of one head under loss "Softmax" on this rank: per step (ok_loss, ok_prec, ok_gx, ok_gw, ok_gb)."""
    from frhip.sharded_head import ShardedMarginLoss, class_range
    from shard_ref_softmax import SoftmaxOracleKernels
    g = torch.Generator().manual_seed(25)
    full_w = torch.randn(N, D, generator=g) * 0.3
    full_b = torch.rand(N, generator=g) * 2 - 1 if name == "Softmax" else None
    crit = ShardedMarginLoss(D, N, name, loss="Softmax", full_weight=full_w, full_bias=full_b,
                             kernels=kernels or SoftmaxOracleKernels())
    lo, hi = class_range(N, WORLD, rank)
    assert (crit.lo, crit.hi) == (lo, hi) and tuple(crit.weight.shape) == (hi - lo, D)
    assert torch.equal(crit.gather_weight(), full_w)
    if name == "Softmax":
        assert tuple(crit.bias.shape) == (hi - lo,) and torch.equal(crit.bias.detach(), full_b[lo:hi])
        assert torch.equal(crit.gather_bias(), full_b)
        assert torch.equal(crit.gather_full(crit.slice_full(full_b)), full_b)
        if wrong_bias:
            with torch.no_grad():
                crit.bias.copy_(full_b[:hi - lo])
    res = []
    for _ in range(2):
        labs = _labels(g, N)
        xs = [torch.randn(B, D, generator=g) for _ in range(WORLD)]
        x = xs[rank].clone().requires_grad_(True)
        crit.zero_grad()
        loss, p1, p5 = crit(x, labs[rank])
        loss.backward()
        e_loss, e_gx, e_gw, e_gb, e_p1, e_p5 = _expected(name, full_w, full_b, xs, labs)
        ok_gb = True
        if name == "Softmax":
            ok_gb = _close(crit.bias.grad, e_gb[lo:hi]) and _close(crit.gather_full(crit.bias.grad), e_gb)
        print("%s N %d rank %d: loss %.8f expected %.8f  max|dgx| %.3e  max|dgw| %.3e" % (
            name, N, rank, float(loss.detach()), float(e_loss),
            float((x.grad / WORLD - e_gx[rank * B:(rank + 1) * B]).abs().max()),
            float((crit.weight.grad - e_gw[lo:hi]).abs().max())))
        res.append((_loss_ok(loss.detach(), e_loss),
                    float(p1) == pytest.approx(e_p1) and float(p5) == pytest.approx(e_p5),
                    _close(x.grad / WORLD, e_gx[rank * B:(rank + 1) * B]),
                    _close(crit.weight.grad, e_gw[lo:hi]) and _close(crit.gather_full(crit.weight.grad), e_gw), ok_gb))
        assert _all_equal_bits(loss)
    return res


def _missed(flags):
    """Asked of the ranks together: a bar missed on any rank counts."""
    missed = torch.tensor([float(not all(flags))])
    dist.all_reduce(missed)
    return float(missed) > 0


def _worker(rank, port, N, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=WORLD)
    try:
        from shard_ref_softmax import FocalSlopeKernels
        for name in ("Softmax", "ArcFace"):
            for step, oks in enumerate(_run(name, rank, N)):
                assert all(oks), (name, "step", step, "loss / precision / gx / gw / gbias", oks)
        bad = _run("Softmax", rank, N, wrong_bias=True)
        assert _missed([ok[0] for ok in bad]), "the first hi - lo entries of the bias on every rank still met the loss bar"
        bad = _run("Softmax", rank, N, kernels=FocalSlopeKernels())
        assert not _missed([ok[0] for ok in bad]), "the focal slope changes the backward pass only"
        for i, what in ((2, "x.grad"), (3, "weight"), (4, "bias")):
            assert _missed([ok[i] for ok in bad]), "a focal slope in the backward pass still met the %s bar" % what
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("n_classes", [33, 100])
def test_sharded_softmax_matches_one_process_on_the_whole_batch(n_classes):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, port, n_classes, q)) for r in range(WORLD)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
    for rank, msg in res:
        assert msg == "ok", "rank %d: %s" % (rank, msg)
