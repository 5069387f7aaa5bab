"""Class sampling in the class-sharded head on the GPU (frhip/sharded_head.py ``sample_rate``; csrc/class_sample.hip):
fr_class_sample bit for bit against the numpy restatement (tests/class_sample_ref.py) in sentinel-guarded buffers, twice;
fr_gather_rows / fr_scatter_rows against torch indexing; the sampled one-rank step bit for bit an unsampled step on the
gathered rows, and against a float64 restatement; rate 1.0 and a rate that keeps every class against the default path; what
the profiler sees; one SGD step; two ranks sharing GPU 0; train.py with a bit-for-bit resume.

The integer buffers are float32 ``head_support.Guarded`` buffers viewed as int32 / int64: the sentinel's bit pattern
(-12345.0f = 0xC640E400) is no value the entry point may write (every output is >= -1), so equality with the restatement
also says that every element was written.

train.py: the synthetic set of the other train.py tests (12 identities, batches of 20) admits no rate below 1 -- n_s must
be at least min(classes, rows of the batch) = 12 -- so these runs take 120 identities x 1 image: 6 steps an epoch as before,
and 30 of 120 classes a step at rate 0.25."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import class_sample_ref as CS  # noqa: E402
import head_support as HS  # noqa: E402
from frhip import ops, synth  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
D = 512


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


# ------------------------------------------------------------------------------------------------ fr_class_sample


def _labels(n, rows, tag):
    """Random labels with rows owned elsewhere (-1), labels past the shard and duplicates."""
    lab = synth.labels(3, "cs.lab." + tag, rows, n)
    if rows >= 8:
        lab[::5] = -1
        lab[1::7] = n + 2
        lab[2] = lab[3]
    return lab


def _sample(lab_dev, n, n_s, salt, class0):
    """One guarded call: (idx, inv, label_s) as numpy, the guards checked."""
    rows = lab_dev.shape[0]
    gi, gv, gl = HS.Guarded(n_s), HS.Guarded(n), HS.Guarded(2 * rows)
    idx, inv, label_s = gi.t.view(torch.int32), gv.t.view(torch.int32), gl.t.view(torch.int64)
    words = int(ops.lib.fr_class_sample_work(n))
    gw = HS.Guarded(words)
    ops.call("fr_class_sample", lab_dev, rows, n, n_s, salt, class0, idx, inv, label_s, gw.t.view(torch.int32),
             ops.current_stream_ptr())()
    torch.cuda.synchronize()
    for g, what in ((gi, "idx"), (gv, "inv"), (gl, "label_s"), (gw, "work")):
        g.assert_guards(what)
    return idx.cpu().numpy(), inv.cpu().numpy(), label_s.cpu().numpy()


CASES = [(1, 1, 3, 0, 1), (5, 5, 2, 11, 1), (257, 64, 64, 0, 1), (4133, 414, 32, 24500, 16), (70001, 7001, 512, 9, 1),
         (2 ** 20 + 3, 104858, 256, 3 * 2 ** 20, 1)]


@pytest.mark.parametrize("n,n_s,rows,class0,salts", CASES)
def test_class_sample_equals_the_restatement_bit_for_bit(n, n_s, rows, class0, salts):
    _need_gpu()
    if n == 1:
        lab = torch.tensor([0, -1, 5])
    elif n == 5:
        lab = torch.tensor([4, 0])
    elif n == 257:  # 64 distinct labels: P = n_s, no negative is drawn
        lab = torch.from_numpy(np.random.RandomState(5).permutation(n)[:rows].astype(np.int64))
    else:
        lab = _labels(n, rows, str(n))
    lab_dev = lab.cuda()
    for step in range(salts):
        salt = CS.salt(17, step)
        want = CS.select(lab.numpy(), n, n_s, salt, class0)
        for run in range(2):
            got = _sample(lab_dev, n, n_s, salt, class0)
            for g, w, what in zip(got, want, ("idx", "inv", "label_s")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (
                    what, "n %d n_s %d step %d run %d" % (n, n_s, step, run), int((g != w).sum()), g[:8], w[:8])
    if n == 257:
        assert int(CS.positives(lab.numpy(), n).sum()) == n_s
    assert torch.equal(lab_dev.cpu(), lab)  # the labels are read only


# ------------------------------------------------------------------------------------------------ gather / scatter


@pytest.mark.parametrize("d", [1, 512, 516])
@pytest.mark.parametrize("n,n_s", [(300, 300), (300, 1), (300, 77), (1, 1)])
def test_gather_and_scatter_rows_equal_torch_indexing(d, n, n_s):
    _need_gpu()
    st = ops.current_stream_ptr()
    w = synth.normal(4, "cs.w.%d" % d, (n, d)).cuda()
    idx = torch.from_numpy(np.sort(np.random.RandomState(n_s).permutation(n)[:n_s]).astype(np.int32)).cuda()
    out = HS.Guarded(n_s, d)
    ops.call("fr_gather_rows", w, idx, out.t, n_s, d, st)()
    assert torch.equal(out.t, w[idx.long()])
    out.assert_guards("gather out")
    inv = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    inv[idx.long()] = torch.arange(n_s, dtype=torch.int32, device="cuda")
    g = synth.normal(5, "cs.g.%d" % d, (n_s, d)).cuda()
    dense = HS.Guarded(n, d)
    ops.call("fr_scatter_rows", g, inv, dense.t, n, d, st)()
    want = torch.zeros(n, d, device="cuda")
    want[idx.long()] = g
    assert torch.equal(dense.t, want) and not bool(torch.signbit(dense.t[inv < 0]).any())
    dense.assert_guards("scatter out")


def test_hip_kernels_methods_take_a_bias_as_one_column():
    _need_gpu()
    from frhip.sharded_head import HipKernels
    K = HipKernels()
    b = synth.normal(6, "cs.b", (300,)).cuda()
    lab = _labels(300, 16, "bias").cuda()
    idx, inv, label_s = K.sample_classes(lab, 300, 40, CS.salt(1, 2), 600)
    want = CS.select(lab.cpu().numpy(), 300, 40, CS.salt(1, 2), 600)
    assert all(np.array_equal(a.cpu().numpy(), b_) for a, b_ in zip((idx, inv, label_s), want))
    picked = K.gather_rows(b, idx)
    assert picked.shape == (40,) and torch.equal(picked, b[idx.long()])
    back = K.scatter_rows(picked, inv, 300)
    assert back.shape == (300,) and torch.equal(back[idx.long()], picked) and int((back != 0).sum()) <= 40


# ------------------------------------------------------------------------------------------------ one rank

N1, B1, RATE1, SEED1 = 4133, 32, 0.1, 21


def _case(name):
    w = synth.uniform(11, "cs1.w." + name, (N1, D), -0.1, 0.1)
    b = synth.uniform(14, "cs1.b", (N1,), -0.5, 0.5) if name == "Softmax" else None
    x = synth.uniform(12, "cs1.x", (B1, D), -1.0, 1.0)
    y = synth.labels(13, "cs1.y", B1, N1)
    y[0], y[1], y[2] = 0, N1 - 1, y[3]
    return w, b, x, y


def _step(crit, x, y):
    for p in crit.parameters():
        p.grad = None
    xc = x.cuda().requires_grad_(True)
    loss, p1, p5 = crit(xc, y.cuda())
    loss.backward()
    return loss.detach(), xc.grad, p1, p5


@pytest.mark.parametrize("name,loss", [("ArcFace", "Focal"), ("ArcFace", "Softmax"), ("CosFace", "Focal"),
                                       ("SphereFace", "Focal"), ("Softmax", "Softmax")])
def test_sampled_step_is_the_unsampled_step_on_the_gathered_rows(name, loss):
    """Bit for bit: same kernels, same shapes.  And the float64 restatement within |d loss| < 1e-3, relative gradient error
    < 1e-3 (the bars of tests/test_gpu_sharded_heads_ext.py)."""
    _need_gpu()
    from frhip.sharded_head import ShardedMarginLoss, sampled_classes
    w, b, x, y = _case(name)
    n_s = sampled_classes(RATE1, N1)
    assert n_s == 414
    idx, inv, y_s = CS.select(y.numpy(), N1, n_s, CS.salt(SEED1, 0), 0)
    sel = torch.from_numpy(idx.astype(np.int64))
    crit = ShardedMarginLoss(D, N1, name, full_weight=w, full_bias=b, loss=loss, sample_rate=RATE1,
                             sample_seed=SEED1).cuda()
    small = ShardedMarginLoss(D, n_s, name, full_weight=w[sel], full_bias=None if b is None else b[sel], loss=loss).cuda()
    la, gxa, p1a, p5a = _step(crit, x, y)
    lb, gxb, p1b, p5b = _step(small, x, torch.from_numpy(y_s))
    assert crit.sample_step == 1
    assert torch.equal(la, lb) and torch.equal(gxa, gxb), (float(la), float(lb), HS.relerr(gxa, gxb))
    assert torch.equal(p1a, p1b) and torch.equal(p5a, p5b)
    unsel = torch.from_numpy(inv < 0)
    assert tuple(crit.weight.grad.shape) == (N1, D) and torch.equal(crit.weight.grad[sel.cuda()], small.weight.grad)
    assert bool((crit.weight.grad[unsel.cuda()] == 0).all()) and int(unsel.sum()) == N1 - n_s
    if b is not None:
        assert tuple(crit.bias.grad.shape) == (N1,) and torch.equal(crit.bias.grad[sel.cuda()], small.bias.grad)
        assert bool((crit.bias.grad[unsel.cuda()] == 0).all())
    e_loss, e_gx, e_gw, e_gb = CS.restricted_step(name, w, b, x, y, idx, 0, loss, 2.0)
    print("%s / %s: loss %.6f float64 %.6f  gx %.2e  gw %.2e" % (
        name, loss, float(la), float(e_loss), HS.relerr(gxa.cpu(), e_gx), HS.relerr(small.weight.grad.cpu(), e_gw)))
    assert abs(float(la) - float(e_loss)) < 1e-3
    assert HS.relerr(gxa.cpu(), e_gx) < 1e-3 and HS.relerr(small.weight.grad.cpu(), e_gw) < 1e-3
    if b is not None:
        assert HS.relerr(small.bias.grad.cpu(), e_gb) < 1e-3
    # the next step draws another set, and eval mode runs every class
    crit.weight.grad = None
    _step(crit, x, y)
    assert crit.sample_step == 2 and not torch.equal((crit.weight.grad.abs().sum(1) != 0).cpu(), ~unsel)
    crit.eval()
    with torch.no_grad():
        crit(x.cuda(), y.cuda())
    assert crit.sample_step == 2


def test_all_classes_at_any_rate_are_the_default_path(monkeypatch):
    """Rate 1.0 and a rate whose n_s is the whole shard give the default path's bits; under the profiler rate 1.0 launches
    none of the new kernels, and a sampled forward pass copies nothing to the host."""
    _need_gpu()
    from frhip.sharded_head import ShardedMarginLoss
    w, _, x, y = _case("ArcFace")
    make = lambda **kw: ShardedMarginLoss(D, N1, "ArcFace", full_weight=w, **kw).cuda()  # noqa: E731
    base, one, whole, part = make(), make(sample_rate=1.0), make(sample_rate=0.99999), make(sample_rate=RATE1)
    assert whole.n_s == N1 and whole.sample_rate < 1.0
    lb, gxb, _, _ = _step(base, x, y)
    for crit in (one, whole):
        la, gxa, _, _ = _step(crit, x, y)
        assert torch.equal(la, lb) and torch.equal(gxa, gxb) and torch.equal(crit.weight.grad, base.weight.grad)
    from frhip import functional as FRF
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)  # as train.py runs it: the label check is a host read of its own
    xc, yc = x.cuda(), y.cuda()
    new = lambda names: sorted(set(n for n in names if "cs_" in n and "kernel" in n))  # noqa: E731
    part(xc, yc)  # first call: streams, allocator
    torch.cuda.synchronize()
    names_part = HS.profiled_names(lambda: part(xc, yc))
    names_one = HS.profiled_names(lambda: one(xc, yc))
    assert len(new(names_part)) >= 9, ("the sampled forward pass shows the new kernels", new(names_part))
    assert any("cs_gather_kernel" in n for n in names_part)
    assert not new(names_one), ("rate 1.0 launched", new(names_one))
    cell = torch.ones(1, device="cuda")
    control = HS.profiled_names(lambda: (cell.item(), cell.cpu()))
    assert any(n in HS.HOST_READS for n in control) and any("DtoH" in n for n in control), sorted(set(control))
    bad = [n for n in names_part if n in HS.HOST_READS or "DtoH" in n]
    assert not bad, ("sampled forward pass", sorted(set(bad)))


def test_one_sgd_step_leaves_the_unselected_rows_alone():
    _need_gpu()
    from frhip.optim import SGD
    from frhip.sharded_head import ShardedMarginLoss, sampled_classes
    w, b, x, y = _case("Softmax")
    crit = ShardedMarginLoss(D, N1, "Softmax", full_weight=w, full_bias=b, loss="Softmax", sample_rate=RATE1,
                             sample_seed=SEED1).cuda()
    opt = SGD([{"params": list(crit.parameters()), "weight_decay": 0.0}], lr=0.1, momentum=0.0)
    _, inv, _ = CS.select(y.numpy(), N1, sampled_classes(RATE1, N1), CS.salt(SEED1, 0), 0)
    unsel = torch.from_numpy(inv < 0).cuda()
    opt.zero_grad()
    xc = x.cuda().requires_grad_(True)
    crit(xc, y.cuda())[0].backward()
    opt.step()
    torch.cuda.synchronize()
    w1, b1 = crit.weight.detach(), crit.bias.detach()
    assert torch.equal(w1[unsel], w.cuda()[unsel]) and torch.equal(b1[unsel], b.cuda()[unsel])
    assert bool((w1[~unsel] != w.cuda()[~unsel]).any(1).all()) and bool((b1[~unsel] != b.cuda()[~unsel]).all())


def test_hip_path_refuses_a_rate_too_small_for_the_batch():
    _need_gpu()
    from frhip.sharded_head import ShardedMarginLoss
    crit = ShardedMarginLoss(D, 200, "ArcFace", sample_rate=0.05).cuda()  # n_s = 10 < 32 rows
    with pytest.raises(ValueError, match="smallest admissible rate here is 0.16"):
        crit(torch.zeros(32, D, device="cuda"), torch.zeros(32, dtype=torch.long, device="cuda"))


# ------------------------------------------------------------------------------------------------ two ranks


def test_two_ranks_sharing_one_gpu():
    _need_gpu()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29591", os.path.join(HERE, "shard_sample_worker.py")]
    out = HS.child(cmd, REPO, env, 300)
    assert out.returncode == 0 and "SHARD_SAMPLE_WORKER_OK" in out.stdout, out.stdout[-4000:] + out.stderr[-1500:]


# ------------------------------------------------------------------------------------------------ train.py


def _run_train_120(tmp, tag, extra_cfg, max_steps=0, epochs=2, ok=True, limit=900):
    """``head_support.run_train`` on 120 identities x 1 image (see the module docstring): same config, same 6 steps an epoch."""
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


def test_train_py_samples_classes_and_resumes_bit_for_bit(tmp_path, monkeypatch):
    """train.py with SHARDED_HEAD=True and SHARDED_HEAD_SAMPLE_RATE=0.25: 12 steps straight == 6 steps, stop, resume for 6
    (the sets drawn after the resume are those of the straight run: ``sample_step`` follows the batch counter)."""
    _need_gpu()
    monkeypatch.setattr(HS, "run_train", _run_train_120)
    cfg = dict(HEAD_NAME="ArcFace", SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=0.25)
    losses, sd_mid, sd_final, dirs = HS.straight_and_resumed(tmp_path, cfg, "ArcFace")
    assert list(sd_final) == ["weight"] and tuple(sd_final["weight"].shape) == (120, 512)
    assert not torch.equal(sd_mid["weight"], sd_final["weight"])


def test_train_py_refuses_a_rate_without_the_sharded_head(tmp_path):
    _need_gpu()
    out = _run_train_120(tmp_path, "refused", dict(HEAD_NAME="ArcFace", SHARDED_HEAD_SAMPLE_RATE=0.25), max_steps=1,
                         ok=False, limit=120)
    assert out.returncode != 0 and "needs SHARDED_HEAD=True" in out.stderr, out.stderr[-1500:]
