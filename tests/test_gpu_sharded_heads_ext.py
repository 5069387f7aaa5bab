"""Class-sharded SphereFace, Am_softmax and CurricularFace on the GPU (frhip/sharded_head.py): the three new kernels against
torch, label -1 in the apply kernels, the one-rank module against the replicated HIP heads and their host paths, two ranks
sharing GPU 0, and train.py with SHARDED_HEAD=True for each head."""
import math
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

import curricular_data as CD  # noqa: E402
import head_support as HS  # noqa: E402
from frhip import ops, synth  # noqa: E402
from head_support import ckpt as _ckpt  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SHAPES = [(7, 33, 36), (64, 1001, 1004), (5, 1, 4)]
HEADS = ("SphereFace", "Am_softmax", "CurricularFace")
M = 0.5
CONSTS = (math.cos(M), math.sin(M), math.cos(math.pi - M), math.sin(math.pi - M) * M)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _cosines(rows, N, ld, tag):
    """Raw cosines [rows, ld] (padding columns 0) with a few just outside [-1, 1], so the clamp shows."""
    cos = torch.zeros(rows, ld)
    cos[:, :N] = synth.uniform(5, "shext.cos." + tag, (rows, N), -1.0, 1.0)
    flat = cos[:, :N].reshape(-1)  # a copy when ld != N
    flat[::7] = 1.0 + 1e-6
    flat[3::11] = -(1.0 + 1e-6)
    cos[:, :N] = flat.view(rows, N)
    return cos.cuda()


@pytest.mark.parametrize("rows,N,ld", SHAPES)
def test_shard_target_cos(rows, N, ld):
    _need_gpu()
    cos = _cosines(rows, N, ld, "tc")
    lab = synth.labels(6, "shext.lab", rows, N).cuda()
    lab[0], lab[1], lab[2], lab[3] = -1, 0, N - 1, N  # not owned, first, last, one past the shard
    tl = torch.full((rows,), 7.0, device="cuda")
    ops.call("fr_shard_target_cos", cos, lab, tl, rows, N, ld, ops.current_stream_ptr())()
    own = (lab >= 0) & (lab < N)
    want = torch.where(own, cos.gather(1, lab.clamp(0, N - 1)[:, None])[:, 0].clamp(-1, 1), torch.zeros(rows, device="cuda"))
    torch.testing.assert_close(tl, want, rtol=0, atol=0)
    assert bool((tl[~own] == 0).all()) and not bool(torch.signbit(tl[~own]).any())
    assert float(tl.abs().max()) <= 1.0
    if rows == 64:  # some picked cosines lay outside [-1, 1]
        assert bool((cos.gather(1, lab.clamp(0, N - 1)[:, None])[:, 0][own].abs() > 1.0).any())


@pytest.mark.parametrize("train", [1, 0])
@pytest.mark.parametrize("rows,N,ld", SHAPES)
def test_rows_from_equals_curricular_rows(rows, N, ld, train):
    """Every label local: fr_shard_target_cos + fr_curricular_rows_from give the bits of fr_curricular_rows."""
    _need_gpu()
    st = ops.current_stream_ptr()
    cos = _cosines(rows, N, ld, "rf")
    lab = synth.labels(7, "shext.lab2", rows, N).cuda()
    lab[0], lab[rows - 1] = 0, N - 1
    rowv_a, rowv_b = torch.empty(4, rows, device="cuda"), torch.empty(4, rows, device="cuda")
    mean_a, mean_b = torch.empty(1, device="cuda"), torch.empty(1, device="cuda")
    t_a, t_b = torch.full((1,), 0.3, device="cuda"), torch.full((1,), 0.3, device="cuda")
    ops.call("fr_curricular_rows", cos, lab, rowv_a, mean_a, t_a, rows, N, ld, *CONSTS, train, st)()
    tl = torch.empty(rows, device="cuda")
    ops.call("fr_shard_target_cos", cos, lab, tl, rows, N, ld, st)()
    ops.call("fr_curricular_rows_from", tl, rowv_b, mean_b, t_b, rows, *CONSTS, train, st)()
    assert torch.equal(rowv_a, rowv_b) and torch.equal(mean_a, mean_b) and torch.equal(t_a, t_b)
    assert (float(t_a) != float(torch.tensor(0.3))) == bool(train)
    assert bool(torch.isfinite(rowv_a).all())


@pytest.mark.parametrize("nparts", [1, 2, 5])
@pytest.mark.parametrize("rows", [7, 64, 300])
def test_shard_sum_parts(rows, nparts):
    _need_gpu()
    r_part = synth.normal(8, "shext.rpart.%d" % nparts, (rows, nparts)).cuda()
    r = torch.full((rows, 1), 7.0, device="cuda")
    ops.call("fr_shard_sum_parts", r_part, nparts, r, rows, ops.current_stream_ptr())()
    want = torch.zeros(rows, device="cuda")
    for p in range(nparts):  # fp32, in part order: what fr_normalize_bwd_radial does
        want = want + r_part[:, p]
    torch.testing.assert_close(r[:, 0], want, rtol=0, atol=0)


@pytest.mark.parametrize("rows,N,ld", SHAPES)
def test_label_minus_one_selects_no_column(rows, N, ld):
    """fr_margin_apply / fr_curricular_apply and their backward kernels with label -1: the row is the one a labelled run
    gives outside its label column, and at that column the plain (unlabelled) value."""
    _need_gpu()
    st = ops.current_stream_ptr()
    cos = _cosines(rows, N, ld, "m1")
    none = torch.full((rows,), -1, dtype=torch.long, device="cuda")
    dummy = synth.labels(9, "shext.dummy", rows, N).cuda()
    keep = torch.ones(rows, N, dtype=torch.bool, device="cuda").scatter_(1, dummy[:, None], False)
    inv_x = (synth.uniform(9, "shext.inv", (rows,), 0.5, 2.0)).cuda()
    g = synth.normal(9, "shext.g", (rows, N)).cuda()
    ldg = (N + 31) // 32 * 32
    parts = int(ops.lib.fr_margin_apply_parts(ldg))

    def fwd_bwd(label, kind):
        out = torch.empty(rows, ld, device="cuda")
        gcos = torch.empty(rows, ldg, device="cuda")
        if kind == 4:
            rowv = torch.stack([torch.full((rows,), 0.4), torch.full((rows,), 0.1), torch.full((rows,), -0.2),
                                torch.ones(rows)]).cuda()
            t = torch.full((1,), 0.3, device="cuda")
            ops.call("fr_curricular_apply", cos, label, rowv, t, out, rows, N, ld, 64.0, st)()
            ops.call("fr_curricular_bwd", g, cos, label, rowv, t, gcos, rows, N, ld, ldg, CONSTS[0], CONSTS[1], 64.0, st)()
        else:
            mi, p0, p1 = (4, 6.0, 0.0) if kind == 2 else (0, 0.35, 30.0)
            r_part = torch.empty(rows, parts, device="cuda") if kind == 2 else None
            ops.call("fr_margin_apply", cos, label, inv_x, out, rows, N, ld, kind, mi, p0, p1, st)()
            ops.call("fr_margin_apply_bwd", g, cos, label, inv_x, gcos, r_part, rows, N, ld, ldg, kind, mi, p0, p1, st)()
        return out, gcos

    c = cos[:, :N].clamp(-1, 1)
    passes = ((cos[:, :N] >= -1) & (cos[:, :N] <= 1)).float()
    plain = {2: (c / inv_x[:, None], g / inv_x[:, None] * passes), 3: (c * 30.0, g * 30.0 * passes),
             4: (torch.where(c > 0.1, c * (0.3 + c), c) * 64.0,
                 g * 64.0 * torch.where(c > 0.1, 0.3 + 2 * c, torch.ones_like(c)) * passes)}
    for kind in (2, 3, 4):
        out_n, gcos_n = fwd_bwd(none, kind)
        out_d, gcos_d = fwd_bwd(dummy, kind)
        assert torch.equal(out_n[:, :N][keep], out_d[:, :N][keep]), kind
        assert torch.equal(gcos_n[:, :N][keep], gcos_d[:, :N][keep]), kind
        assert not bool(out_n[:, N:].any()) and not bool(gcos_n[:, N:].any())
        # the whole row, the dummy column included, is the unlabelled value
        torch.testing.assert_close(out_n[:, :N], plain[kind][0], rtol=2e-6, atol=1e-6)
        torch.testing.assert_close(gcos_n[:, :N], plain[kind][1], rtol=2e-6, atol=1e-6)
        assert not torch.equal(out_n[:, :N], out_d[:, :N])  # the labelled run did touch its column


def _case(name, N, B):
    D = 512
    if name == "CurricularFace":
        x, full, y, _ = CD.built(synth, "sh1ext.%d" % N, B, D, N)
        CD.assert_covers_both_branches(x, full, y, 0.5)
    else:
        full = synth.uniform(11, "sh1ext.w." + name, (N, D) if name == "SphereFace" else (D, N), -0.1, 0.1)
        x = synth.uniform(12, "sh1ext.x", (B, D), -1.0, 1.0)
        y = synth.labels(13, "sh1ext.y", B, N)
        y[0], y[1] = 0, N - 1
    return x, full, y


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("N,B", [(100, 8), (1001, 16), (7000, 64)])
@pytest.mark.parametrize("name", HEADS)
def test_one_rank_equals_replicated_head(name, N, B):
    """Without a process group the sharded module is the whole head: over two steps loss, accuracy, both gradients (and
    CurricularFace's t, bit for bit) equal the replicated HIP head + FocalLoss + accuracy, and the head's host path on
    the CPU within the north-star bar."""
    _need_gpu()
    from frhip.sharded_head import ShardedMarginLoss
    from head import metrics as H
    from loss.focal import FocalLoss
    from util.utils import accuracy
    from oracle import irse_ref as O
    D = 512
    x0, full, y = _case(name, N, B)
    make = (lambda: H.CurricularFace(D, N)) if name == "CurricularFace" else (lambda: getattr(H, name)(D, N, None))
    head, host = make(), make()
    for h in (head, host):
        with torch.no_grad():
            list(h.parameters())[0].copy_(full)
    head = head.cuda()
    p, ph = list(head.parameters())[0], list(host.parameters())[0]
    crit = ShardedMarginLoss.from_head(head, gamma=2.0).cuda()
    assert (crit.lo, crit.hi) == (0, N) and crit.grad_scale == 1.0 and crit.weight.shape == p.shape
    for step in range(2):
        crit.weight.grad = p.grad = None
        x = x0.cuda().requires_grad_(True)
        loss, p1, p5 = crit(x, y.cuda())
        loss.backward()
        xr = x0.cuda().requires_grad_(True)
        logits = head(xr, y.cuda())
        floss, _ = FocalLoss()(logits, y.cuda())
        floss.backward()
        e1, e5 = accuracy(logits.detach(), y.cuda(), topk=(1, 5))
        print("%s N %d B %d step %d: loss %.8f replicated %.8f  gx %.2e  gw %.2e" % (
            name, N, B, step, float(loss.detach()), float(floss), _rel(x.grad, xr.grad), _rel(crit.weight.grad, p.grad)))
        assert abs(float(loss.detach()) - float(floss)) <= 2e-6 * max(1.0, abs(float(floss)))
        assert float(p1) == float(e1) and float(p5) == float(e5)
        assert _rel(x.grad, xr.grad) <= 1e-5 and _rel(crit.weight.grad, p.grad) <= 1e-5
        if name == "CurricularFace":
            assert torch.equal(crit.t, head.t) and float(crit.t) != 0.0
        if name == "SphereFace":
            assert crit.iter == head.iter == step + 1 and crit.lamb == head.lamb
        xo = x0.clone().requires_grad_(True)
        lo = O.focal_loss(host(xo, y), y, 2)
        ogx, ogw = torch.autograd.grad(lo, [xo, ph])
        assert abs(float(loss.detach()) - float(lo)) < 1e-3
        assert _rel(x.grad.cpu(), ogx) < 1e-3 and _rel(crit.weight.grad.cpu(), ogw) < 1e-3
    with pytest.raises(RuntimeError):
        crit(x.detach(), torch.full((B,), N, device="cuda"))
    with pytest.raises(Exception):
        crit(x0, y)  # host tensors: no CPU fallback


def test_eval_mode_leaves_t_alone():
    _need_gpu()
    from frhip.sharded_head import ShardedMarginLoss
    x, full, y = _case("CurricularFace", 100, 8)
    crit = ShardedMarginLoss(512, 100, "CurricularFace", full_weight=full).cuda()
    crit.t.fill_(0.2)
    crit.eval()
    with torch.no_grad():
        crit(x.cuda(), y.cuda())
    assert float(crit.t) == float(torch.tensor(0.2))
    crit.train()
    crit(x.cuda(), y.cuda())
    assert float(crit.t) != float(torch.tensor(0.2))


def test_two_ranks_sharing_one_gpu():
    _need_gpu()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29583", os.path.join(HERE, "shard_ext_worker.py")]
    out = HS.child(cmd, REPO, env, 300)
    assert out.returncode == 0 and "SHARD_EXT_WORKER_OK" in out.stdout, out.stdout[-4000:] + out.stderr[-1500:]


# ------------------------------------------------------------------------------------------------ train.py


def _sharded_train(tmp, tag, extra_cfg, max_steps=0):
    model_dir, stdout = HS.run_train(tmp, tag, dict(extra_cfg, SHARDED_HEAD=True), max_steps=max_steps, limit=300)
    assert "Training Loss" in stdout and "nan" not in stdout.lower()
    return model_dir, stdout


def _check_head_file(path, name):
    """Exactly the replicated head's keys and shapes, all values finite."""
    from head import metrics as H
    ref = H.CurricularFace(512, 12) if name == "CurricularFace" else getattr(H, name)(512, 12, None)
    sd = torch.load(path, map_location="cpu")
    want = ref.state_dict()
    assert list(sd) == list(want), (list(sd), list(want))
    for k in want:
        assert tuple(sd[k].shape) == tuple(want[k].shape) and bool(torch.isfinite(sd[k]).all()), k
    return sd


def test_train_py_am_softmax(tmp_path):
    _need_gpu()
    d, _ = _sharded_train(tmp_path, "am", dict(HEAD_NAME="Am_softmax"), max_steps=3)
    sd = _check_head_file(_ckpt(d, "Head_Am_softmax_Epoch_1_Batch_3_"), "Am_softmax")
    assert list(sd) == ["kernel"] and tuple(sd["kernel"].shape) == (512, 12)
    osd = torch.load(_ckpt(d, "Optimizer_Am_softmax_Epoch_1_Batch_3_"), map_location="cpu")
    assert (512, 12) in [tuple(v["momentum_buffer"].shape) for v in osd["state"].values()]


def test_train_py_sphereface_resume_restores_iter(tmp_path):
    _need_gpu()
    d, _ = _sharded_train(tmp_path, "first", dict(HEAD_NAME="SphereFace"), max_steps=6)
    sd = _check_head_file(_ckpt(d, "Head_SphereFace_Epoch_1_Batch_6_"), "SphereFace")
    assert list(sd) == ["weight"] and tuple(sd["weight"].shape) == (12, 512)
    assert torch.load(_ckpt(d, "State_SphereFace_Epoch_1_Batch_6_"))["head_iter"] == 6
    d2, log = _sharded_train(tmp_path, "second", HS.resume_cfg(dict(HEAD_NAME="SphereFace"), d, "SphereFace"))
    assert "Resuming at epoch 1 batch 6" in log
    assert torch.load(_ckpt(d2, "State_SphereFace_Epoch_2_Batch_12_"))["head_iter"] == 12


def test_train_py_curricularface_resume_continues_bit_for_bit(tmp_path):
    """The pattern of test_gpu_model.py::test_resume_continues_bit_for_bit with the class-sharded CurricularFace: 12 steps
    straight == 6 steps, stop, resume for 6 -- backbone, kernel, t and momentum."""
    _need_gpu()
    cfg = dict(HEAD_NAME="CurricularFace")
    a_dir, _ = _sharded_train(tmp_path, "straight", cfg)
    b1_dir, _ = _sharded_train(tmp_path, "first", cfg, max_steps=6)
    sd = _check_head_file(_ckpt(b1_dir, "Head_CurricularFace_Epoch_1_Batch_6_"), "CurricularFace")
    assert sorted(sd) == ["kernel", "t"] and tuple(sd["kernel"].shape) == (512, 12) and float(sd["t"]) != 0.0
    b2_dir, log = _sharded_train(tmp_path, "second", HS.resume_cfg(cfg, b1_dir, "CurricularFace"))
    assert "Resuming at epoch 1 batch 6" in log and "Loading Optimizer Checkpoint" in log
    HS.assert_same_checkpoints(a_dir, b2_dir, "CurricularFace", "Epoch_2_Batch_12_")
