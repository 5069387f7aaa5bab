"""Class-sharded SphereFace, Am_softmax and CurricularFace (frhip/sharded_head.py) on the CPU at world size 2 and 3 over
``gloo``: the whole choreography -- the all-gathers, the statistics exchange, CurricularFace's [Bg] all-reduce of the target
cosines, SphereFace's [Bg, 1] reduce-scatter of the radial sums, the column-wise ragged gather of a [D, N] kernel -- with
tests/shard_ref_ext.py standing in for the HIP kernels.

Expected values: the host (plain PyTorch) paths of ``head.metrics.SphereFace`` / ``Am_softmax`` / ``CurricularFace`` (pinned
to the reference by g14 / g18) on the concatenated batch with the full parameter, then ``oracle.irse_ref.focal_loss`` and
``topk_accuracy``; gradients by autograd.  Two consecutive steps per case: from t = 0 a hard negative is c * c, so only the
second step sees a non-zero t, and SphereFace's lambda moves between the steps.

Bars (those of tests/test_sharded_head_gloo.py): loss 1e-5 relative, precision equal, x.grad / world and the shard gradient
rtol 1e-4 / atol 1e-6, loss and t bits equal on all ranks, t within 1e-6 of the reference head's.

Negative controls: CurricularFace with cos(theta_target + m) from the local target cosines only misses the loss bar;
SphereFace without the exchange of r misses the x.grad bar."""
import math
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))

D, GAMMA = 64, 2.0
HEADS = ("SphereFace", "Am_softmax", "CurricularFace")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _unit(v):
    return v / v.norm()


def _labels(g, world, B, N):
    """Per-rank labels: class 0 and class N - 1 forced, and on every rank a row whose label another rank owns."""
    from frhip.sharded_head import class_range
    labs = [torch.randint(0, N, (B,), generator=g) for _ in range(world)]
    for r in range(world):
        lo, hi = class_range(N, world, (r + 1) % world)
        labs[r][-1] = lo + (hi - lo) // 2  # lives on the next rank
    labs[0][0], labs[-1][0] = 0, N - 1
    for r in range(world):
        lo, hi = class_range(N, world, r)
        assert ((labs[r] < lo) | (labs[r] >= hi)).any()
    return labs


def _built_x(g, k, label):
    """Rows for CurricularFace against a fixed kernel k [D, N] (the construction of tests/curricular_data.py with the labels
    given): rows i % 4 != 3 have a target cosine of 0.62 .. 0.71, so cos(theta + m) ~ 0.2 and their ordinary negatives are
    mostly easy, and a cosine of ~0.5 with one other class: a hard negative; rows i % 4 == 3 lie near the negative of their
    class column (target cosine -0.97: the tl - mm branch, every negative hard)."""
    N = k.shape[1]
    kd = k.double()
    x = torch.empty(label.shape[0], k.shape[0], dtype=torch.float64)
    for i, lab in enumerate(label.tolist()):
        u = _unit(kd[:, lab])
        v = torch.randn(k.shape[0], generator=g, dtype=torch.float64)
        if i % 4 == 3:
            a, c = -0.97, 0.0
        else:
            a, c = 0.62 + 0.01 * i, 0.5
        other = _unit(kd[:, (lab + 1 + i) % N] - (kd[:, (lab + 1 + i) % N] @ u) * u)
        rest = v - (v @ u) * u
        rest = _unit(rest - (rest @ other) * other)
        x[i] = (0.5 + i % 5) * (a * u + c * other + math.sqrt(1 - a * a - c * c) * rest)
    return x.float()


def _reference_head(name, N, full):
    from head import metrics as H
    head = H.CurricularFace(D, N) if name == "CurricularFace" else getattr(H, name)(D, N, None)
    p = head.kernel if hasattr(head, "kernel") else head.weight
    with torch.no_grad():
        p.copy_(full)
    return head, p


def _expected(head, p, xs, labs):
    """One step of the host head over the concatenated batch; the head keeps its t / iter for the next step."""
    from oracle import irse_ref as O
    x = torch.cat(xs).clone().requires_grad_(True)
    lab = torch.cat(labs)
    p.grad = None
    logits = head(x, lab)
    loss = O.focal_loss(logits, lab, GAMMA)
    gx, gp = torch.autograd.grad(loss, [x, p])
    p1, p5 = O.topk_accuracy(logits.detach(), lab)
    return loss.detach(), gx, gp, float(p1), float(p5)


def _loss_ok(loss, e_loss):
    return abs(float(loss) - float(e_loss)) < 1e-5 * max(1.0, abs(float(e_loss)))


def _close(a, b):
    return torch.allclose(a, b, rtol=1e-4, atol=1e-6)


def _all_equal_bits(t, world):
    got = [torch.zeros_like(t) for _ in range(world)]
    dist.all_gather(got, t.detach().clone())
    return all(torch.equal(got[0], v) for v in got)


def _steps(g, name, world, B, N, full):
    """Two steps of per-rank (features, labels)."""
    out = []
    for _ in range(2):
        labs = _labels(g, world, B, N)
        if name == "CurricularFace":
            xa = _built_x(g, full, torch.cat(labs))
            xs = list(xa.split(B))
        else:
            xs = [torch.randn(B, D, generator=g) for _ in range(world)]
        out.append((xs, labs))
    return out


def _run_head(name, rank, world, B, N, kernels=None, drop_r=False):
    """Both steps of one head on this rank; returns per step (ok_loss, ok_prec, ok_gx, ok_gw) and runs the exact checks."""
    from frhip.sharded_head import ShardedMarginLoss, class_range
    from shard_ref_ext import ExtOracleKernels
    import curricular_data as CD
    g = torch.Generator().manual_seed(11)
    cdim = 0 if name == "SphereFace" else 1
    full = torch.randn((N, D) if cdim == 0 else (D, N), generator=g) * 0.3
    crit = ShardedMarginLoss(D, N, name, gamma=GAMMA, full_weight=full, kernels=kernels or ExtOracleKernels())
    lo, hi = class_range(N, world, rank)
    assert (crit.lo, crit.hi, crit.class_dim) == (lo, hi, cdim)
    assert tuple(crit.weight.shape) == ((hi - lo, D) if cdim == 0 else (D, hi - lo))
    assert torch.equal(crit.gather_weight(), full)
    if drop_r:  # SphereFace's r stays local: the [Bg, 1] exchange is skipped
        real = crit.comm.reduce_scatter_rows
        n_local = lambda t: t[rank * B:(rank + 1) * B].contiguous()  # noqa: E731
        crit.comm.reduce_scatter_rows = lambda t: n_local(t) if t.shape[1] == 1 else real(t)
    head, p = _reference_head(name, N, full)
    res = []
    for xs, labs in _steps(g, name, world, B, N, full):
        if name == "CurricularFace":
            CD.assert_covers_both_branches(torch.cat(xs), full, torch.cat(labs), crit.m)
        x = xs[rank].clone().requires_grad_(True)
        crit.weight.grad = None
        loss, p1, p5 = crit(x, labs[rank])
        loss.backward()
        e_loss, e_gx, e_gp, e_p1, e_p5 = _expected(head, p, xs, labs)
        e_shard = e_gp[lo:hi] if cdim == 0 else e_gp[:, lo:hi]
        print("%s world %d N %d rank %d: loss %.8f expected %.8f  max|dgx| %.3e  max|dgw| %.3e" % (
            name, world, N, rank, float(loss.detach()), float(e_loss),
            float((x.grad / world - e_gx[rank * B:(rank + 1) * B]).abs().max()),
            float((crit.weight.grad - e_shard).abs().max())))
        res.append((_loss_ok(loss.detach(), e_loss),
                    float(p1) == pytest.approx(e_p1) and float(p5) == pytest.approx(e_p5),
                    _close(x.grad / world, e_gx[rank * B:(rank + 1) * B]), _close(crit.weight.grad, e_shard)))
        assert _all_equal_bits(loss, world)  # combined in rank order: the same bits everywhere
        if name == "CurricularFace" and kernels is None:
            assert _all_equal_bits(crit.t, world)
            assert abs(float(crit.t) - float(head.t)) <= 1e-6, (float(crit.t), float(head.t))
        if name == "SphereFace":
            assert crit.iter == head.iter and crit.lamb == head.lamb
    if name == "CurricularFace" and kernels is None:
        assert float(crit.t) != 0.0
    return res


def _worker(rank, world, port, B, N, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from shard_ref_ext import LocalTargetKernels
        for name in HEADS:
            for step, oks in enumerate(_run_head(name, rank, world, B, N)):
                assert all(oks), (name, "step", step, "loss / precision / gx / gw", oks)
        # negative controls: the ranks are asked together, a bar missed on any rank counts
        bad = _run_head("CurricularFace", rank, world, B, N, kernels=LocalTargetKernels())
        missed = torch.tensor([float(not all(ok[0] for ok in bad))])
        dist.all_reduce(missed)
        assert float(missed) > 0, "local-only target cosines still met the loss bar"
        bad = _run_head("SphereFace", rank, world, B, N, drop_r=True)
        missed = torch.tensor([float(not all(ok[2] for ok in bad))])
        dist.all_reduce(missed)
        assert float(missed) > 0, "dropping the exchange of r still met the x.grad bar"
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,B,n_classes", [(2, 5, 101), (3, 2, 20)])
def test_sharded_ext_heads_match_full_batch_heads(world, B, n_classes):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, B, n_classes, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=240) for _ in procs]
    for p in procs:
        p.join(60)
    for rank, msg in res:
        assert msg == "ok", "rank %d: %s" % (rank, msg)
