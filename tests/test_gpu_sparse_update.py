"""The row-sparse SGD update of the sampled class-sharded head on the GPU (``ShardedMarginLoss(sparse_update=True)``,
``frhip.optim.SGD``, fr_sgd_rows in csrc/head_loss_optim.hip; config key SHARDED_HEAD_SPARSE_UPDATE).  Every comparison is
bit for bit (int32 views: -0.0 and +0.0 differ, NaN equals itself).

fr_sgd_rows: in sentinel-guarded buffers against fr_sgd_step (through ``frhip.optim.SGD``) on a copy of the gathered rows,
and against the np.float32 restatement (tests/sparse_update_ref.py: three single-rounding fused multiply-adds, which is what
the shared device function compiles to); unselected rows, the gradient rows and the guard bands keep their bits.

The head: one step against the default (dense) variant, what the profiler sees of it, three steps where the two semantics
coincide (no decay, no momentum) and three where they do not (against the restatement driven by the restated selection of
tests/class_sample_ref.py), the cases that stay on the dense path, two ranks sharing GPU 0, and train.py with a bit-for-bit
resume on the 120-identity synthetic set of tests/test_gpu_class_sample.py."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import class_sample_ref as CS  # noqa: E402
import head_support as HS  # noqa: E402
import sparse_update_ref as SU  # noqa: E402
from frhip import ops, synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
D = 512


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def bits(t):
    t = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t, dtype=np.float32)
    return np.ascontiguousarray(t).view(np.int32)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ fr_sgd_rows


def _idx_sets(n, n_s):
    """Ascending, distinct index sets that hold row 0 and row n - 1 (one at a time where only one row is selected)."""
    if n_s == n:
        return [np.arange(n, dtype=np.int32)]
    if n_s == 1:
        return [np.array([0], dtype=np.int32), np.array([n - 1], dtype=np.int32)]
    inner = 1 + np.random.RandomState(n_s).permutation(n - 2)[:n_s - 2]
    return [np.sort(np.concatenate([[0, n - 1], inner])).astype(np.int32)]


def _operands(mode, n, n_s, d):
    rng = np.random.RandomState(1000 * d + n + n_s)
    if mode == "dyadic":  # nothing rounds: multiples of 1/64 and power-of-two scalars
        return SU.dyadic(rng, (n, d)), SU.dyadic(rng, (n, d)), SU.dyadic(rng, (n_s, d)), (0.25, 0.5, 0.5)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return f(n, d), f(n, d), f(n_s, d), (0.1, 0.9, 5e-4)


def _sgd_step_on_gathered(p_rows, buf_rows, g_rows, lr, momentum, wd):
    """What fr_sgd_step leaves on a copy of the gathered rows: (p, buf)."""
    from frhip.optim import SGD
    q = torch.nn.Parameter(p_rows.clone())
    q.grad = g_rows.clone()
    opt = SGD([q], lr=lr, momentum=momentum, weight_decay=wd)
    opt.state[q]["momentum_buffer"] = buf_rows.clone()
    opt.step()
    return q.detach(), opt.state[q]["momentum_buffer"]


@pytest.mark.parametrize("mode", ["random", "dyadic"])
@pytest.mark.parametrize("d", [1, 4, 6, 512])
@pytest.mark.parametrize("n,n_s", [(1, 1), (33, 1), (300, 77), (300, 300)])
def test_sgd_rows_equals_sgd_step_on_the_gathered_rows(n, n_s, d, mode):
    _need_gpu()
    p0, b0, g0, (lr, mom, wd) = _operands(mode, n, n_s, d)
    for idx in _idx_sets(n, n_s):
        assert idx.shape == (n_s,) and (idx[0] == 0 or idx[-1] == n - 1) and (n_s == 1 or (idx[0] == 0 and idx[-1] == n - 1))
        gp, gb, gg = HS.Guarded(n, d), HS.Guarded(n, d), HS.Guarded(n_s, d)
        gp.t.copy_(torch.from_numpy(p0))
        gb.t.copy_(torch.from_numpy(b0))
        gg.t.copy_(torch.from_numpy(g0))
        idx_dev = torch.from_numpy(idx).cuda()
        sel = idx_dev.long()
        want_p, want_b = _sgd_step_on_gathered(gp.t[sel], gb.t[sel], gg.t, lr, mom, wd)
        ops.call("fr_sgd_rows", gp.t, gb.t, gg.t, idx_dev, n_s, d, lr, mom, wd, ops.current_stream_ptr())()
        torch.cuda.synchronize()
        tag = (n, n_s, d, mode, int(idx[0]))
        assert same(gp.t[sel], want_p) and same(gb.t[sel], want_b), tag + (
            "selected rows != fr_sgd_step", int((bits(gp.t[sel]) != bits(want_p)).sum()), int((bits(gb.t[sel]) != bits(want_b)).sum()))
        unsel = np.ones(n, dtype=bool)
        unsel[idx] = False
        assert same(gp.t.cpu()[unsel], p0[unsel]) and same(gb.t.cpu()[unsel], b0[unsel]), tag + ("an unselected row moved",)
        assert same(gg.t, g0) and np.array_equal(idx_dev.cpu().numpy(), idx), tag + ("an input was written",)
        for g_, what in ((gp, "p"), (gb, "buf"), (gg, "g_rows")):
            g_.assert_guards(what)
        ref_p, ref_b = SU.sgd_rows_ref(p0, b0, g0, idx, wd, mom, lr)
        assert same(gp.t, ref_p) and same(gb.t, ref_b), tag + ("!= restatement", int((bits(gp.t) != bits(ref_p)).sum()))
        if mode == "dyadic":
            ref_p, ref_b = SU.sgd_rows_ref64(p0, b0, g0, idx, wd, mom, lr)
            assert same(gp.t, ref_p) and same(gb.t, ref_b), tag + ("!= float64 restatement",)
        if n_s * d >= 64:  # (fewer elements: dyadic operands may cancel to a zero step)
            assert not same(gp.t[sel], p0[idx]), tag + ("nothing moved",)


def test_sgd_rows_on_unaligned_rows_takes_the_scalar_path_to_the_same_bits():
    """D % 4 == 0 but p one float off a 16-byte boundary: 4-byte accesses, the bits of the aligned call."""
    _need_gpu()
    n, n_s, d = 33, 5, 8
    p0, b0, g0, (lr, mom, wd) = _operands("random", n, n_s, d)
    idx = _idx_sets(n, n_s)[0]
    idx_dev = torch.from_numpy(idx).cuda()
    out = []
    for off in (0, 1):
        gp, gb, gg = HS.Guarded(n * d + 1), HS.Guarded(n, d), HS.Guarded(n_s, d)
        p = gp.t[off:off + n * d].view(n, d)
        assert (p.data_ptr() % 16 == 0) == (off == 0)
        gp.t.fill_(HS.SENTINEL)
        p.copy_(torch.from_numpy(p0))
        gb.t.copy_(torch.from_numpy(b0))
        gg.t.copy_(torch.from_numpy(g0))
        ops.call("fr_sgd_rows", p, gb.t, gg.t, idx_dev, n_s, d, lr, mom, wd, ops.current_stream_ptr())()
        torch.cuda.synchronize()
        gp.assert_guards("p")
        rest = torch.cat([gp.t[:off], gp.t[off + n * d:]])
        assert bool((rest == HS.SENTINEL).all())
        out.append((p.clone(), gb.t.clone()))
    assert same(out[0][0], out[1][0]) and same(out[0][1], out[1][1])
    ref_p, ref_b = SU.sgd_rows_ref(p0, b0, g0, idx, wd, mom, lr)
    assert same(out[1][0], ref_p) and same(out[1][1], ref_b)


def test_sgd_rows_launches_nothing_without_rows():
    _need_gpu()
    gp = HS.Guarded(4, 4)
    assert ops.lib.fr_sgd_rows(ops.ptr(gp.t), ops.ptr(gp.t), ops.ptr(gp.t), ops.ptr(gp.t), 0, 4, 0.1, 0.9, 0.0,
                               ops.current_stream_ptr()) == 0
    torch.cuda.synchronize()
    assert bool((gp.flat == HS.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ the head, one rank

N2, B2, RATE2, SEED2, LR2 = 96, 8, 0.25, 21, 0.1
HEADS = [("ArcFace", "Focal"), ("Softmax", "Softmax")]


def _case(name, step=0):
    w = synth.uniform(11, "su.w." + name, (N2, D), -0.1, 0.1)
    b = synth.uniform(14, "su.b", (N2,), -0.5, 0.5) if name == "Softmax" else None
    x = synth.uniform(12 + step, "su.x", (B2, D), -1.0, 1.0)
    y = synth.labels(13 + step, "su.y", B2, N2)
    y[0], y[1], y[2] = 0, N2 - 1, y[3]
    return w, b, x, y


def _make(name, loss, momentum, wd, **kw):
    from frhip.optim import SGD
    from frhip.sharded_head import ShardedMarginLoss
    w, b, _, _ = _case(name)
    crit = ShardedMarginLoss(D, N2, name, full_weight=w, full_bias=b, loss=loss, sample_rate=RATE2, sample_seed=SEED2,
                             **kw).cuda()
    opt = SGD([{"params": list(crit.parameters()), "weight_decay": wd}], lr=LR2, momentum=momentum)
    return crit, opt


def _train_step(crit, opt, x, y):
    """The order of train.py: forward, zero_grad, backward, step.  Returns (loss, the row gradients the backward left)."""
    xc = x.cuda().requires_grad_(True)
    loss = crit(xc, y.cuda())[0]
    opt.zero_grad()
    loss.backward()
    left = {k: tuple(t.clone() for t in p._frhip_row_grad) for k, p in crit.named_parameters()
            if getattr(p, "_frhip_row_grad", None) is not None}
    opt.step()
    torch.cuda.synchronize()
    return loss.detach(), left


def _selection(y, step):
    from frhip.sharded_head import sampled_classes
    n_s = sampled_classes(RATE2, N2)
    assert n_s == 24
    idx, inv, _ = CS.select(y.numpy(), N2, n_s, CS.salt(SEED2, step), 0)
    return idx, torch.from_numpy(idx.astype(np.int64)).cuda(), torch.from_numpy(inv < 0).cuda()


@pytest.mark.parametrize("name,loss", HEADS)
def test_one_step_agrees_with_the_dense_variant_on_the_selected_rows(name, loss):
    """From zero momentum the selected rows see the same operands in both variants; the unselected rows of the sparse
    variant keep their initial bits, where the dense variant has decayed them."""
    _need_gpu()
    w0, b0, x, y = _case(name)
    dense, od = _make(name, loss, 0.9, 1e-2)
    sparse, osp = _make(name, loss, 0.9, 1e-2, sparse_update=True)
    ld, left_d = _train_step(dense, od, x, y)
    ls, left_s = _train_step(sparse, osp, x, y)
    idx, sel, unsel = _selection(y, 0)
    assert torch.equal(ld, ls) and not left_d and sorted(left_s) == sorted(k for k, _ in sparse.named_parameters())
    for (k, pd), (_, ps) in zip(dense.named_parameters(), sparse.named_parameters()):
        init = (w0 if k == "weight" else b0).cuda()
        bd, bs = od.state[pd]["momentum_buffer"], osp.state[ps]["momentum_buffer"]
        assert ps.grad is None and ps._frhip_row_grad is None and pd.grad is not None, k
        got_idx, rows = left_s[k]
        assert np.array_equal(got_idx.cpu().numpy(), idx) and same(rows, pd.grad[sel]), k
        assert tuple(bs.shape) == tuple(ps.shape) and same(ps[sel], pd[sel]) and same(bs[sel], bd[sel]), k
        assert same(ps[unsel], init[unsel]) and not bool(bs[unsel].any()), (k, "an unselected row moved")
        assert not same(ps[sel], init[sel]), (k, "the selected rows did not move")
        if k == "weight":  # the control: the dense path decays the rows the sparse one leaves alone
            assert not same(pd[unsel], init[unsel])


def test_profile_shows_no_scatter_and_no_host_copy(monkeypatch):
    _need_gpu()
    from frhip import functional as FRF
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)  # as train.py runs it: the label check is a host read of its own
    _, _, x, y = _case("Softmax")
    xc, yc = x.cuda(), y.cuda()
    seen = {}
    for tag, kw in (("dense", {}), ("sparse", dict(sparse_update=True))):
        crit, opt = _make("Softmax", "Softmax", 0.9, 1e-2, **kw)
        _train_step(crit, opt, x, y)  # first call: streams, allocator, the optimizer's tables and momentum buffers
        hold = {}

        def fwd():
            hold["loss"] = crit(xc.detach().requires_grad_(True), yc)[0]

        def bwd_step():
            opt.zero_grad()
            hold["loss"].backward()
            opt.step()

        seen[tag] = (HS.profiled_names(fwd), HS.profiled_names(bwd_step))
    cs = lambda names: sorted(set(n for n in names if "cs_" in n and "kernel" in n))  # noqa: E731
    fwd_s, bwd_s = seen["sparse"]
    assert len(cs(fwd_s)) >= 9 and any("cs_gather_kernel" in n for n in fwd_s), ("the forward pass samples", cs(fwd_s))
    assert any("cs_scatter_kernel" in n for n in seen["dense"][1]), ("control: the dense backward scatters", cs(seen["dense"][1]))
    assert not any("cs_scatter_kernel" in n for n in bwd_s), cs(bwd_s)
    assert sum("sgd_rows_kernel" in n for n in bwd_s) >= 2 and not any("sgd_rows_kernel" in n for n in seen["dense"][1])
    cell = torch.ones(1, device="cuda")
    control = HS.profiled_names(lambda: (cell.item(), cell.cpu()))
    assert any(n in HS.HOST_READS for n in control) and any("DtoH" in n for n in control), sorted(set(control))
    bad = [n for n in fwd_s + bwd_s if n in HS.HOST_READS or "DtoH" in n]
    assert not bad, ("sparse step", sorted(set(bad)))


@pytest.mark.parametrize("name,loss", HEADS)
def test_three_steps_without_decay_and_momentum_are_the_dense_steps(name, loss):
    """Where the two semantics coincide: d = g, buf = d, p -= lr d, and an unselected row of the dense path moves by
    lr * 0."""
    _need_gpu()
    dense, od = _make(name, loss, 0.0, 0.0)
    sparse, osp = _make(name, loss, 0.0, 0.0, sparse_update=True)
    for step in range(3):
        _, _, x, y = _case(name, step)
        ld, _ = _train_step(dense, od, x, y)
        ls, _ = _train_step(sparse, osp, x, y)
        assert torch.equal(ld, ls), step
        for (k, pd), (_, ps) in zip(dense.named_parameters(), sparse.named_parameters()):
            assert same(pd, ps), (k, step, int((bits(pd) != bits(ps)).sum()))
            assert ps.grad is None
    assert dense.sample_step == sparse.sample_step == 3


@pytest.mark.parametrize("name,loss", HEADS)
def test_three_steps_with_decay_and_momentum_are_the_restatement(name, loss):
    """The restatement is driven by the restated selection and by the rows the backward pass left; a dense parameter in the
    same optimizer keeps stepping, and the launch tables are built once."""
    _need_gpu()
    from frhip.optim import SGD
    mom, wd = 0.9, 1e-2
    w0, b0, _, _ = _case(name)
    sparse, _ = _make(name, loss, mom, wd, sparse_update=True)
    extra = torch.nn.Parameter(torch.ones(5, device="cuda"))
    opt = SGD([{"params": list(sparse.parameters()), "weight_decay": wd}, {"params": [extra]}], lr=LR2, momentum=mom)
    builds = []
    build = opt._build
    opt._build = lambda: (builds.append(1), build())[1]
    ref = {"weight": (w0.numpy().copy(), np.zeros((N2, D), dtype=np.float32))}
    if b0 is not None:
        ref["bias"] = (b0.numpy().copy(), np.zeros(N2, dtype=np.float32))
    drawn = []
    extra.grad = torch.ones(5, device="cuda")
    for step in range(3):
        _, _, x, y = _case(name, step)
        xc = x.cuda().requires_grad_(True)
        loss_t = sparse(xc, y.cuda())[0]
        opt.zero_grad()
        extra.grad.fill_(1.0)
        loss_t.backward()
        idx, sel, unsel = _selection(y, step)
        drawn.append(idx)
        for k, p in sparse.named_parameters():
            got_idx, rows = p._frhip_row_grad
            assert np.array_equal(got_idx.cpu().numpy(), idx), (k, step)
            ref[k] = SU.sgd_rows_ref(ref[k][0], ref[k][1], rows.cpu().numpy(), idx, wd, mom, LR2)
        opt.step()
        torch.cuda.synchronize()
        for k, p in sparse.named_parameters():
            buf = opt.state[p]["momentum_buffer"]
            assert p.grad is None and p._frhip_row_grad is None
            assert same(p, ref[k][0]) and same(buf, ref[k][1]), (
                k, step, int((bits(p) != bits(ref[k][0])).sum()), int((bits(buf) != bits(ref[k][1])).sum()))
    assert not np.array_equal(drawn[0], drawn[1]) and len(builds) == 1, (len(builds), "table builds in three steps")
    # the dense parameter of the same optimizer: three momentum steps of gradient 1, no decay in its group
    e, b = np.ones(5), np.zeros(5)
    for _ in range(3):
        b = mom * b + 1.0
        e = e - LR2 * b
    assert np.allclose(extra.detach().cpu().numpy(), e, rtol=1e-6)
    # rows never selected in the three steps kept their initial bits and a zero momentum
    never = torch.ones(N2, dtype=torch.bool)
    never[torch.from_numpy(np.concatenate(drawn).astype(np.int64))] = False
    assert int(never.sum()) > 0 and same(sparse.weight.detach().cpu()[never], w0[never])
    assert not bool(opt.state[sparse.weight]["momentum_buffer"].cpu()[never].any())
    sd = opt.state_dict()  # the state dict is what the dense path writes: one dense momentum buffer per stepped parameter
    shapes = [tuple(p.shape) for p in sparse.parameters()] + [(5,)]
    assert {i: tuple(s["momentum_buffer"].shape) for i, s in sd["state"].items()} == dict(enumerate(shapes))


def test_second_backward_and_adam_are_refused_on_the_hip_path():
    _need_gpu()
    from frhip.optim import Adam
    _, _, x, y = _case("ArcFace")
    sparse, opt = _make("ArcFace", "Focal", 0.9, 1e-2, sparse_update=True)
    sparse(x.cuda().requires_grad_(True), y.cuda())[0].backward()
    with pytest.raises(RuntimeError, match="second backward"):
        sparse(x.cuda().requires_grad_(True), y.cuda())[0].backward()
    with pytest.raises(NotImplementedError, match="sparse_update"):
        Adam(list(sparse.parameters()), lr=0.1).step()
    opt.zero_grad()
    assert sparse.weight._frhip_row_grad is None
    sparse(x.cuda().requires_grad_(True), y.cuda())[0].backward()
    opt.step()
    assert sparse.weight._frhip_row_grad is None and sparse.weight.grad is None


def test_rate_one_eval_mode_and_a_whole_shard_stay_on_the_dense_path():
    _need_gpu()
    from frhip.sharded_head import ShardedMarginLoss
    w, _, x, y = _case("ArcFace")
    make = lambda **kw: ShardedMarginLoss(D, N2, "ArcFace", full_weight=w, sample_seed=SEED2, **kw).cuda()  # noqa: E731

    def step(crit):
        xc = x.cuda().requires_grad_(True)
        loss = crit(xc, y.cuda())[0]
        loss.backward()
        return loss.detach(), xc.grad, crit.weight.grad

    base = step(make())
    for kw in (dict(sample_rate=1.0), dict(sample_rate=0.995)):
        crit = make(sparse_update=True, **kw)
        assert crit.n_s == N2
        got = step(crit)
        assert all(same(a, b) for a, b in zip(got, base)), kw
        assert getattr(crit.weight, "_frhip_row_grad", None) is None
    crit = make(sparse_update=True, sample_rate=RATE2).eval()
    got = step(crit)
    assert all(same(a, b) for a, b in zip(got, base)) and getattr(crit.weight, "_frhip_row_grad", None) is None
    assert crit.sample_step == 0


# ------------------------------------------------------------------------------------------------ two ranks


def test_two_ranks_sharing_one_gpu():
    _need_gpu()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29593", os.path.join(HERE, "shard_sparse_worker.py")]
    out = HS.child(cmd, REPO, env, 300)
    assert out.returncode == 0 and "SHARD_SPARSE_WORKER_OK" in out.stdout, out.stdout[-4000:] + out.stderr[-1500:]


# ------------------------------------------------------------------------------------------------ train.py


def _run_train_120(tmp, tag, extra_cfg, max_steps=0, epochs=2, ok=True, limit=900):
    """``head_support.run_train`` on 120 identities x 1 image, as tests/test_gpu_class_sample.py runs it: the 12-identity
    set of the other train.py tests admits no rate below 1.  Same config, the same 6 steps an epoch, 30 of 120 classes a
    step at rate 0.25."""
    env = dict(os.environ, PYTHONPATH=HS.PRODUCT)
    argv = ["train.py", "--config", "configs/config_synthetic_smoke.py", "--synthetic", "120x1"]
    if max_steps:
        argv += ["--max-steps", str(max_steps)]
    model_dir = tmp / tag
    cfg_patch = ("import configs.config_synthetic_smoke as c; c.configurations[1].update(BATCH_SIZE=20, NUM_EPOCH=%d, "
                 "MODEL_ROOT=r'%s', LOG_ROOT=r'%s', **%r)" % (epochs, model_dir, tmp / "log", extra_cfg))
    code = "import sys, runpy; sys.argv=%r; %s; runpy.run_path('train.py', run_name='__main__')" % (argv, cfg_patch)
    out = HS.child([sys.executable, "-c", code], HS.PRODUCT, env, limit)
    if not ok:
        return out
    assert out.returncode == 0, "train.py run %r exited %d\n%s" % (
        tag, out.returncode, out.stdout[-2000:] + out.stderr[-2000:])
    return model_dir, out.stdout


def test_train_py_updates_rows_and_resumes_bit_for_bit(tmp_path, monkeypatch):
    """12 steps straight == 6 steps, stop, resume for 6, with SHARDED_HEAD_SPARSE_UPDATE=True: the State_* file has no new
    key, the momentum buffer of the Optimizer_* file is the dense one.  And the option is not a no-op: the same run without
    the key ends on another weight (its unselected rows decay)."""
    _need_gpu()
    monkeypatch.setattr(HS, "run_train", _run_train_120)
    cfg = dict(HEAD_NAME="ArcFace", SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=0.25, SHARDED_HEAD_SPARSE_UPDATE=True)
    losses, sd_mid, sd_final, dirs = HS.straight_and_resumed(tmp_path, cfg, "ArcFace")
    assert list(sd_final) == ["weight"] and tuple(sd_final["weight"].shape) == (120, 512)
    assert not torch.equal(sd_mid["weight"], sd_final["weight"])
    state = torch.load(HS.ckpt(dirs[0], "State_ArcFace_Epoch_2_Batch_12_"), map_location="cpu")
    assert not any("sparse" in k.lower() for k in state), list(state)
    dense_dir, _ = _run_train_120(tmp_path, "dense", dict(cfg, SHARDED_HEAD_SPARSE_UPDATE=False))
    sd_dense = torch.load(HS.ckpt(dense_dir, "Head_ArcFace_Epoch_2_Batch_12_"), map_location="cpu")
    assert tuple(sd_dense["weight"].shape) == (120, 512) and not torch.equal(sd_dense["weight"], sd_final["weight"])


def test_train_py_refuses_the_option_without_the_sharded_head(tmp_path):
    _need_gpu()
    out = _run_train_120(tmp_path, "refused", dict(HEAD_NAME="ArcFace", SHARDED_HEAD_SPARSE_UPDATE=True), max_steps=1,
                         ok=False, limit=120)
    assert out.returncode != 0 and "SHARDED_HEAD_SPARSE_UPDATE=True needs SHARDED_HEAD=True" in out.stderr, out.stderr[-1500:]
