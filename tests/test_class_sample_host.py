"""CPU checks of class sampling in the class-sharded head (frhip/sharded_head.py ``sample_rate``; fr_class_sample,
fr_gather_rows, fr_scatter_rows): the numpy restatement of the selection (tests/class_sample_ref.py) and its properties,
the uniformity of the draw, the C ABI of the four entry points and their argument checks, the module's and the driver's
validation, and the whole choreography at world size 2 and 3 over ``gloo`` with numpy stand-ins for the kernels.

Uniformity: with no positives, over 400 steps, z = (inclusion count - 400 p) / sqrt(400 p (1 - p)), p = n_s / n, has
|z| <= 5 for every class (the restatement alone gives max |z| = 3.65 on these inputs).

gloo: three heads, two optimizer steps, ragged shards.  Expected values: the head of head/metrics.py in float64 on the
concatenated batch, restricted to the union of the ranks' selected classes (class_sample_ref.restricted_step).  Bars, those
of tests/test_sharded_heads_ext_gloo.py: loss 1e-5 relative, x.grad / world and the shard gradient rtol 1e-4 / atol 1e-6;
the unselected gradient rows are exactly 0.  Negative control: a selection that drops a positive misses the loss bar."""
import ctypes
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))

import class_sample_ref as CS  # noqa: E402

ENTRIES = ("fr_class_sample_work", "fr_class_sample", "fr_gather_rows", "fr_scatter_rows")
D, GAMMA, RATE, SEED, LR = 64, 2.0, 0.4, 5, 0.05
HEADS = (("ArcFace", "Focal"), ("SphereFace", "Focal"), ("Softmax", "Softmax"))


# ------------------------------------------------------------------------------------------------ the restatement


def test_fmix32_and_salt_agree_with_the_module():
    from frhip import sharded_head as SH
    vals = [0, 1, 0xFFFFFFFF, 0x9E3779B9, 123456789]
    assert [int(v) for v in CS.fmix32(np.array(vals, dtype=np.uint32))] == [SH.fmix32(v) for v in vals]
    assert SH.fmix32(0) == 0 and SH.fmix32(1) == 0x514E28B7  # MurmurHash3's finaliser
    for seed, step in ((0, 0), (1337, 5), (0xFFFFFFFF, 3), (7, 10 ** 7)):
        assert CS.salt(seed, step) == SH.sample_salt(seed, step)
    assert SH.sampled_classes(0.1, 4133) == 414 and SH.sampled_classes(0.25, 1000) == 250
    assert SH.sampled_classes(1e-9, 10) == 1 and SH.sampled_classes(1.0, 10) == 10


@pytest.mark.parametrize("n,class0", [(28000, 0), (4133, 123456), (2 ** 20, 7)])
def test_keys_of_a_shard_are_distinct(n, class0):
    for salt in (0, CS.salt(3, 1), 0xFFFFFFFF):
        assert np.unique(CS.keys(n, class0, salt)).shape[0] == n


def _labels(n, rows, seed):
    rng = np.random.RandomState(seed)
    lab = rng.randint(0, n, size=rows).astype(np.int64)
    lab[::5] = -1  # rows owned by another rank
    lab[1::7] = n + 3  # out of range: marks nothing
    lab[2] = lab[3]  # a duplicate
    return lab


@pytest.mark.parametrize("n,n_s,rows,class0", [(1, 1, 3, 0), (5, 5, 2, 9), (257, 64, 64, 0), (4133, 414, 32, 24500),
                                                (28000, 2800, 256, 0)])
def test_selection_properties(n, n_s, rows, class0):
    lab = _labels(n, rows, 1) if n > 5 else np.zeros(rows, dtype=np.int64)
    salt = CS.salt(SEED, 0)
    idx, inv, label_s = CS.select(lab, n, n_s, salt, class0)
    assert idx.dtype == np.int32 and inv.dtype == np.int32 and label_s.dtype == np.int64
    assert idx.shape == (n_s,) and bool((np.diff(idx) > 0).all()) and idx.min() >= 0 and idx.max() < n
    pos = CS.positives(lab, n)
    assert bool((inv[pos] >= 0).all()), "a positive is missing"
    assert bool((inv[idx] == np.arange(n_s)).all()) and int((inv >= 0).sum()) == n_s
    own = (lab >= 0) & (lab < n)
    assert bool((label_s[~own] == -1).all()) and bool((idx[label_s[own]] == lab[own]).all())
    # the negatives drawn are the ones with the smallest keys
    key = CS.keys(n, class0, salt)
    drawn, left = (inv >= 0) & ~pos, (inv < 0)
    if drawn.any() and left.any():
        assert key[drawn].max() < key[left].min()
    # the same (seed, step) gives the same set, consecutive steps differ
    again = CS.select(lab, n, n_s, CS.salt(SEED, 0), class0)
    assert all(np.array_equal(a, b) for a, b in zip((idx, inv, label_s), again))
    if n_s < n and int(pos.sum()) < n_s:
        nxt = CS.select(lab, n, n_s, CS.salt(SEED, 1), class0)
        assert not np.array_equal(idx, nxt[0])


@pytest.mark.parametrize("n,rate,seed,class0", [(1000, .25, 0, 0), (1000, .25, 7, 3500), (4133, .1, 42, 24500),
                                                 (512, .5, 1, 0)])
def test_every_class_is_drawn_at_the_rate(n, rate, seed, class0):
    from frhip.sharded_head import sampled_classes
    n_s, steps = sampled_classes(rate, n), 400
    none = np.full(1, -1, dtype=np.int64)
    count, overlap, prev = np.zeros(n), [], None
    for step in range(steps):
        _, inv, _ = CS.select(none, n, n_s, CS.salt(seed, step), class0)
        sel = inv >= 0
        count += sel
        if prev is not None:
            overlap.append(float((sel & prev).sum()) / n_s)
        prev = sel
    p = n_s / float(n)
    z = (count - steps * p) / np.sqrt(steps * p * (1 - p))
    print("n %d rate %g seed %d class0 %d: max|z| %.2f  std z %.3f  mean overlap %.4f (p %.4f)" % (
        n, rate, seed, class0, np.abs(z).max(), z.std(), np.mean(overlap), p))
    assert np.abs(z).max() <= 5.0


def test_negative_controls_fail_their_checks():
    n, n_s, class0 = 4133, 414, 24500
    lab = _labels(n, 32, 1)
    salt = CS.salt(SEED, 0)
    pos = CS.positives(lab, n)
    _, inv, _ = CS.select_unforced(lab, n, n_s, salt, class0)
    assert not bool((inv[pos] >= 0).all()), "the unforced selection happened to hold every positive"
    good = CS.select(lab, n, n_s, salt, class0)[0]
    assert not np.array_equal(CS.select_local_keys(lab, n, n_s, salt, class0)[0], good)
    # without class0 two shards draw the same local set; with it they do not
    a, b = CS.select_local_keys(lab[:1] * 0 - 1, n, n_s, salt, 0)[0], CS.select_local_keys(lab[:1] * 0 - 1, n, n_s, salt, n)[0]
    assert np.array_equal(a, b)
    a, b = CS.select(lab[:1] * 0 - 1, n, n_s, salt, 0)[0], CS.select(lab[:1] * 0 - 1, n, n_s, salt, n)[0]
    assert not np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ the C ABI


def test_entries_are_declared_exported_and_prototyped():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in ENTRIES:
        assert "int %s(" % name in header, "include/frhip.h does not declare %s" % name
        assert name in _lib.protos, "no prototype for %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
        assert getattr(_lib.lib, name).argtypes == _lib.protos[name][1]
    assert _lib.protos["fr_class_sample"][2] == ["label_local", "rows", "n", "n_s", "salt", "class0", "idx", "inv", "label_s",
                                                 "work", "stream"]
    assert _lib.protos["fr_gather_rows"][2] == ["w", "idx", "out", "n_s", "D", "stream"]
    assert _lib.protos["fr_scatter_rows"][2] == ["g", "inv", "out", "n", "D", "stream"]
    assert _lib.lib.fr_abi_version() == 7


def test_entries_reject_bad_arguments_without_a_gpu():
    from frhip import _lib
    lib = _lib.lib
    buf = (ctypes.c_uint64 * 64)()  # a host address: the checks come before any launch and never follow a pointer
    p = ctypes.cast(buf, ctypes.c_void_p)

    def cs(rows, n, n_s, class0=0, ptrs=(p, p, p, p, p)):
        return lib.fr_class_sample(ptrs[0], rows, n, n_s, 1, class0, ptrs[1], ptrs[2], ptrs[3], ptrs[4], None)

    for bad in ((4, 10, 0), (4, 10, -1), (4, 10, 11), (4, 10, 3), (20, 10, 9), (0, 10, 5), (4, 0, 1)):
        assert cs(*bad) == -1 and b"fr_class_sample" in lib.fr_last_error_string(), bad
    assert cs(4, 10, 3) == -1 and b"min(n, rows)" in lib.fr_last_error_string()
    assert cs(4, 10, 5, class0=2 ** 32 - 5) == -1 and b"fr_class_sample" in lib.fr_last_error_string()
    for hole in range(5):
        ptrs = tuple(None if i == hole else p for i in range(5))
        assert cs(4, 10, 5, ptrs=ptrs) == -1 and b"fr_class_sample" in lib.fr_last_error_string(), hole
    assert lib.fr_class_sample_work(0) == -1 and b"fr_class_sample_work" in lib.fr_last_error_string()
    sizes = [lib.fr_class_sample_work(n) for n in (1, 1024, 1025, 28000, 2 ** 20 + 3)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    for name, fn in (("fr_gather_rows", lib.fr_gather_rows), ("fr_scatter_rows", lib.fr_scatter_rows)):
        for bad in ((0, 4), (-2, 4), (8, 0), (8, -1)):
            assert fn(p, p, p, bad[0], bad[1], None) == -1 and name.encode() in lib.fr_last_error_string(), (name, bad)
        for hole in range(3):
            ptrs = [None if i == hole else p for i in range(3)]
            assert fn(ptrs[0], ptrs[1], ptrs[2], 8, 4, None) == -1 and name.encode() in lib.fr_last_error_string()


# ------------------------------------------------------------------------------------------------ the module


def _all_kernels():
    from shard_ref_ext import ExtOracleKernels
    from shard_ref_softmax import SoftmaxOracleKernels

    class AllKernels(ExtOracleKernels, SoftmaxOracleKernels):
        """The stand-ins of the three heads, their arithmetic in float64: the expected values are float64, and in float32
        the stand-in's own rounding (ArcFace at s = 64: 3e-6 of the largest gradient entry) would sit above the absolute
        part of the bar.  What is under test is the choreography: selection, gather, remapped labels, scatter."""

        def logits(self, x_all, w, *a):
            return super().logits(x_all.double(), w.double(), *a)

        def ext_logits(self, x_all, w, *a):
            return super().ext_logits(x_all.double(), w.double(), *a)

        def linear_logits(self, x_all, w, bias):
            return super().linear_logits(x_all.double(), w.double(), bias.double())

    return AllKernels


def test_rate_validation_and_refused_heads():
    from frhip.sharded_head import ShardedMarginLoss
    for bad in (0.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="sample_rate"):
            ShardedMarginLoss(D, 40, "ArcFace", sample_rate=bad)
    for name in ("Am_softmax", "CurricularFace"):
        with pytest.raises(ValueError, match="column gather is not built"):
            ShardedMarginLoss(D, 40, name, sample_rate=0.5)
        ShardedMarginLoss(D, 40, name, sample_rate=1.0)  # all classes: served as before
    for name in ("ArcFace", "CosFace", "SphereFace", "Softmax"):
        crit = ShardedMarginLoss(D, 40, name, sample_rate=0.5, sample_seed=9)
        assert (crit.n_s, crit.sample_step, crit.sample_seed, crit.sample_rate) == (20, 0, 9, 0.5)
    assert ShardedMarginLoss(D, 40, "ArcFace").n_s == 40
    from head import metrics as H
    crit = ShardedMarginLoss.from_head(H.ArcFace(D, 40, None), sample_rate=0.25, sample_seed=3)
    assert (crit.n_s, crit.sample_seed) == (10, 3)


def test_too_small_a_rate_is_refused_before_any_kernel_naming_the_smallest():
    from frhip.sharded_head import ShardedMarginLoss
    K = CS.sampling_kernels(_all_kernels())
    crit = ShardedMarginLoss(D, 40, "ArcFace", kernels=K, sample_rate=0.1)  # n_s = 4 < 8 rows
    x, y = torch.randn(8, D), torch.arange(8)
    with pytest.raises(ValueError, match="smallest admissible rate here is 0.2"):
        crit(x, y)
    assert K.calls["sample_classes"] == 0
    crit.eval()
    crit(x, y)  # eval mode runs all classes at any rate
    assert sum(K.calls.values()) == 0


def test_sample_step_counts_training_forwards_and_rate_one_calls_nothing():
    from frhip.sharded_head import ShardedMarginLoss
    x, y = torch.randn(6, D), torch.tensor([0, 39, 4, 4, 17, 20])
    full = torch.randn(40, D) * 0.3
    K1 = CS.sampling_kernels(_all_kernels())
    one = ShardedMarginLoss(D, 40, "ArcFace", kernels=K1, full_weight=full, sample_rate=1.0)
    base = ShardedMarginLoss(D, 40, "ArcFace", kernels=_all_kernels()(), full_weight=full)
    for k in range(3):
        la, lb = one(x, y)[0], base(x, y)[0]
        la.backward()
        lb.backward()
        assert torch.equal(la, lb) and torch.equal(one.weight.grad, base.weight.grad)
    assert sum(K1.calls.values()) == 0 and one.sample_step == 3
    K = CS.sampling_kernels(_all_kernels())
    crit = ShardedMarginLoss(D, 40, "ArcFace", kernels=K, full_weight=full, sample_rate=0.5, sample_seed=SEED)
    crit(x, y)[0].backward()
    assert crit.sample_step == 1 and K.calls == {"sample_classes": 1, "gather_rows": 1, "scatter_rows": 1}
    idx, inv = K.drawn[0]
    want = CS.select(y.numpy(), 40, 20, CS.salt(SEED, 0), 0)
    assert np.array_equal(idx, want[0]) and np.array_equal(inv, want[1])
    unsel = torch.from_numpy(inv < 0)
    assert bool((crit.weight.grad[unsel] == 0).all()) and bool((crit.weight.grad[~unsel].abs().sum(1) > 0).all())
    crit.eval()
    crit(x, y)
    assert crit.sample_step == 1 and K.calls["sample_classes"] == 1
    crit.train()
    crit(x, y)
    assert crit.sample_step == 2 and K.calls["sample_classes"] == 2
    assert not np.array_equal(K.drawn[1][0], K.drawn[0][0])  # the next step draws another set
    crit.sample_step = 0  # what a resumed run does: the same step gives the same set
    crit(x, y)
    assert np.array_equal(K.drawn[2][0], K.drawn[0][0])
    # a rate whose n_s is the whole shard runs the unsampled path
    Kf = CS.sampling_kernels(_all_kernels())
    whole = ShardedMarginLoss(D, 40, "ArcFace", kernels=Kf, full_weight=full, sample_rate=0.99)
    assert whole.n_s == 40 and torch.equal(whole(x, y)[0], base(x, y)[0]) and sum(Kf.calls.values()) == 0


# ------------------------------------------------------------------------------------------------ the driver


def test_check_head_config_refuses_the_new_combinations_and_keeps_the_old():
    import train
    for name in ("ArcFace", "CosFace", "SphereFace", "Softmax"):
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=0.25))
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=1.0))
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD_SAMPLE_RATE=1.0))
        with pytest.raises(NotImplementedError, match="needs SHARDED_HEAD=True"):
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD_SAMPLE_RATE=0.25))
        with pytest.raises(NotImplementedError, match="needs SHARDED_HEAD=True"):
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=False, SHARDED_HEAD_SAMPLE_RATE=0.25))
        for bad in (0.0, -1.0, 1.5):
            with pytest.raises(ValueError, match="SHARDED_HEAD_SAMPLE_RATE"):
                train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=bad))
    for name in ("Am_softmax", "CurricularFace"):
        with pytest.raises(NotImplementedError, match="column gather of class sampling is not built"):
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=0.5))
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=1.0))
    # the existing refusals come first and keep their words; the heads they name are refused with or without a rate
    for table in (train.NOT_SHARDED, train.NOT_SHARDED_ROW_VALUE):
        for name, why in table.items():
            for extra in ({}, {"SHARDED_HEAD_SAMPLE_RATE": 0.5}):
                with pytest.raises(NotImplementedError) as e:
                    train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True, **extra))
                assert str(e.value) == ("SHARDED_HEAD=True with HEAD_NAME '%s': the class-sharded head does not serve %s "
                                        "(%s); run it replicated, SHARDED_HEAD=False" % (name, name, why))
            train.check_head_config(dict(HEAD_NAME=name))
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=False))
    assert sorted(train.NOT_SHARDED) == ["AM_Softmax", "AdaCos", "CircleLoss", "MV_Softmax", "MagFace", "NPCFace"]
    assert sorted(train.NOT_SHARDED_ROW_VALUE) == ["ArcNegFace"]
    src = open(train.__file__).read()
    assert 'sample_rate=cfg.get("SHARDED_HEAD_SAMPLE_RATE", 1.0)' in src and 'sample_seed=cfg["SEED"]' in src
    assert "crit.sample_step = batch" in src
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "SHARDED_HEAD_SAMPLE_RATE" in common


# ------------------------------------------------------------------------------------------------ gloo


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_labels(g, world, B, N):
    """Per-rank labels: class 0 and class N - 1 forced, and on every rank a row whose label another rank owns."""
    from frhip.sharded_head import class_range
    labs = [torch.randint(0, N, (B,), generator=g) for _ in range(world)]
    for r in range(world):
        lo, hi = class_range(N, world, (r + 1) % world)
        labs[r][-1] = lo + (hi - lo) // 2
    labs[0][0], labs[-1][0] = 0, N - 1
    return labs


def _run_head(name, loss_name, rank, world, B, N, select_fn=CS.select):
    """Two optimizer steps of one head on this rank: per step (ok_loss, ok_gx, ok_gw, ok_gb, zeros exact)."""
    from frhip.sharded_head import ShardedMarginLoss, class_range, sampled_classes
    g = torch.Generator().manual_seed(11)
    full = torch.randn(N, D, generator=g) * 0.3
    bias = torch.randn(N, generator=g) * 0.1 if name == "Softmax" else None
    K = CS.sampling_kernels(_all_kernels(), select_fn)
    crit = ShardedMarginLoss(D, N, name, gamma=GAMMA, full_weight=full, full_bias=bias, kernels=K, loss=loss_name,
                             sample_rate=RATE, sample_seed=SEED)
    lo, hi = class_range(N, world, rank)
    n = hi - lo
    assert (crit.lo, crit.hi) == (lo, hi) and crit.n_s == sampled_classes(RATE, n) < n
    full64, bias64 = full.double().clone(), None if bias is None else bias.double().clone()
    res = []
    for step in range(2):
        labs = _rank_labels(g, world, B, N)
        xs = [torch.randn(B, D, generator=g) for _ in range(world)]
        lab_all = torch.cat(labs)
        x = xs[rank].clone().requires_grad_(True)
        crit.weight.grad = None
        if bias is not None:
            crit.bias.grad = None
        loss, _p1, _p5 = crit(x, labs[rank])
        loss.backward()
        # every rank's selection, restated: the union of the selected global classes
        cols, mine = [], None
        for r in range(world):
            rlo, rhi = class_range(N, world, r)
            local = torch.where((lab_all >= rlo) & (lab_all < rhi), lab_all - rlo, torch.full_like(lab_all, -1)).numpy()
            idx, _, _ = CS.select(local, rhi - rlo, sampled_classes(RATE, rhi - rlo), CS.salt(SEED, step), rlo)
            if r == rank:
                mine = (len(cols), idx)
            cols += [rlo + int(c) for c in idx]
        e_loss, e_gx, e_gw, e_gb = CS.restricted_step(name, full64, bias64, torch.cat(xs), lab_all, cols, step, loss_name, GAMMA)
        at, idx = mine
        sel = torch.from_numpy(idx.astype(np.int64))
        e_shard = torch.zeros(n, D, dtype=torch.float64)
        e_shard[sel] = e_gw[at:at + idx.shape[0]]
        unsel = torch.ones(n, dtype=torch.bool)
        unsel[sel] = False
        close = lambda a, b: torch.allclose(a.double(), b, rtol=1e-4, atol=1e-6)  # noqa: E731
        ok_gb, zeros = True, bool((crit.weight.grad[unsel] == 0).all())
        if bias is not None:
            e_b = torch.zeros(n, dtype=torch.float64)
            e_b[sel] = e_gb[at:at + idx.shape[0]]
            ok_gb = close(crit.bias.grad, e_b)
            zeros = zeros and bool((crit.bias.grad[unsel] == 0).all())
        print("%s world %d N %d rank %d step %d: loss %.8f expected %.8f  max|dgx| %.3e of %.3e  max|dgw| %.3e of %.3e" % (
            name, world, N, rank, step, float(loss.detach()), float(e_loss),
            float((x.grad.double() / world - e_gx[rank * B:(rank + 1) * B]).abs().max()), float(e_gx.abs().max()),
            float((crit.weight.grad.double() - e_shard).abs().max()), float(e_shard.abs().max())))
        res.append((abs(float(loss.detach()) - float(e_loss)) < 1e-5 * max(1.0, abs(float(e_loss))),
                    close(x.grad / world, e_gx[rank * B:(rank + 1) * B]), close(crit.weight.grad, e_shard), ok_gb, zeros))
        with torch.no_grad():  # plain SGD on the shard and on the float64 copy of the full parameter
            crit.weight -= LR * crit.weight.grad
            full64[torch.tensor(cols)] -= LR * e_gw
            if bias is not None:
                crit.bias -= LR * crit.bias.grad
                bias64[torch.tensor(cols)] -= LR * e_gb
    gathered = crit.gather_weight()  # collective
    if select_fn is CS.select:
        assert crit.sample_step == 2 and torch.allclose(gathered.double(), full64, rtol=1e-4, atol=1e-6)
    return res


def _worker(rank, world, port, B, N, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for name, loss_name in HEADS:
            for step, oks in enumerate(_run_head(name, loss_name, rank, world, B, N)):
                assert all(oks), (name, "step", step, "loss / gx / gw / gb / exact zeros", oks)
        # negative control: the ranks are asked together, a bar missed on any rank counts
        bad = _run_head("ArcFace", "Focal", rank, world, B, N, select_fn=CS.select_dropping_a_positive)
        missed = torch.tensor([float(not all(ok[0] for ok in bad))])
        dist.all_reduce(missed)
        assert float(missed) > 0, "a selection that drops a positive still met the loss bar"
        q.put((rank, "ok"))
    except Exception as e:  # noqa: BLE001
        import traceback
        q.put((rank, traceback.format_exc() + repr(e)))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,B,n_classes", [(2, 5, 101), (3, 2, 50)])
def test_sampled_sharded_heads_match_the_restricted_full_batch_heads(world, B, n_classes):
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
