"""CPU checks of the row-sparse SGD update of the sampled class-sharded head (``ShardedMarginLoss(sparse_update=True)``,
``frhip.optim.SGD``, fr_sgd_rows, config key SHARDED_HEAD_SPARSE_UPDATE): the np.float32 restatement
(tests/sparse_update_ref.py) against the literal loop over all rows and its three negative controls; the C ABI of the entry
point and its argument checks; the module's and the driver's refusals; the hand-over of the row gradient on one rank and on
two ranks over ``gloo`` with the oracle-backed stand-in kernels; what ``zero_grad`` and ``Adam`` do with a row gradient.
Every comparison is bit for bit."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "stylegan-for-facerec_amd"))

import class_sample_ref as CS  # noqa: E402
import head_support as HS  # noqa: E402
import sparse_update_ref as SU  # noqa: E402

D = 64


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.int32), b.view(np.int32))


# ------------------------------------------------------------------------------------------------ the restatement


def test_fma32_is_one_rounding():
    """Against exact rational arithmetic, on operands chosen so that the float64 sum lands on an fp32 tie."""
    from fractions import Fraction
    rng = np.random.RandomState(0)
    a = rng.standard_normal(2000).astype(np.float32)
    b = rng.standard_normal(2000).astype(np.float32)
    c = (rng.standard_normal(2000) * 10.0 ** rng.randint(-6, 3, 2000)).astype(np.float32)
    # a * b + c = 1 + 2^-11 + 2^-24 + 2^-60: just above the tie between 1 + 2^-11 and its upper fp32 neighbour; a plain
    # float64 sum drops the 2^-60 first and the tie then goes to even, the wrong way
    a[0], b[0], c[0] = np.float32(1 + 2.0 ** -12), np.float32(1 + 2.0 ** -12), np.float32(2.0 ** -60)
    got = SU.fma32(a, b, c)
    for i in range(a.shape[0]):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))  # float(Fraction) is correctly rounded to float64; decide the fp32 neighbour exactly
        cands = sorted({np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))}, key=float)
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(np.float32(v).view(np.int32)) & 1))
        assert same_bits(got[i], best), (i, float(a[i]), float(b[i]), float(c[i]), float(got[i]), float(best))
    assert float(got[0]) == 1 + 2.0 ** -11 + 2.0 ** -23
    assert float(np.float32(np.float64(a[0]) * np.float64(b[0]) + np.float64(c[0]))) == 1 + 2.0 ** -11  # the control


def _case(seed, n=40, n_s=12, d=8, dyadic=False):
    rng = np.random.RandomState(seed)
    idx = np.sort(rng.permutation(n)[:n_s]).astype(np.int32)
    if dyadic:
        return SU.dyadic(rng, (n, d)), SU.dyadic(rng, (n, d)), SU.dyadic(rng, (n_s, d)), idx
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    return f(n, d), f(n, d), f(n_s, d), idx


@pytest.mark.parametrize("shape", [(40, 12, 8), (7, 7, 3), (5, 1, 1)])
def test_restatement_equals_the_literal_loop_and_leaves_the_other_rows(shape):
    n, n_s, d = shape
    p, buf, g, idx = _case(3, n, n_s, d)
    for wd, mom, lr in ((1e-2, 0.9, 0.1), (0.0, 0.0, 0.05), (5e-4, 0.9, 0.03)):
        a = SU.sgd_rows_ref(p, buf, g, idx, wd, mom, lr)
        b = SU.dense_loop(p, buf, g, idx, wd, mom, lr)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1])
        unsel = np.ones(n, dtype=bool)
        unsel[idx] = False
        assert same_bits(a[0][unsel], p[unsel]) and same_bits(a[1][unsel], buf[unsel])
        if n_s and (wd or mom):
            assert not same_bits(a[0][idx], p[idx])
    # one-dimensional parameters (a bias): the same rows
    a = SU.sgd_rows_ref(p[:, 0], buf[:, 0], g[:, 0], idx, 1e-2, 0.9, 0.1)
    b = SU.sgd_rows_ref(p[:, :1], buf[:, :1], g[:, :1], idx, 1e-2, 0.9, 0.1)
    assert same_bits(a[0], b[0][:, 0]) and same_bits(a[1], b[1][:, 0])


def test_dyadic_operands_agree_with_the_float64_sgd_restatement():
    p, buf, g, idx = _case(4, dyadic=True)
    for step in range(3):
        a = SU.sgd_rows_ref(p, buf, g, idx, 0.5, 0.5, 0.25)
        b = SU.sgd_rows_ref64(p, buf, g, idx, 0.5, 0.5, 0.25)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), step
        p, buf = a
    # and on random operands the float64 form is NOT the kernel's three single roundings everywhere: the fp32 form is needed
    p, buf, g, idx = _case(5, 400, 300, 64)
    a, b = SU.sgd_rows_ref(p, buf, g, idx, 1e-2, 0.9, 0.1), SU.sgd_rows_ref64(p, buf, g, idx, 1e-2, 0.9, 0.1)
    assert not same_bits(a[0], b[0])


def test_negative_controls_fail_their_checks():
    p, buf, g, idx = _case(6)
    good = SU.sgd_rows_ref(p, buf, g, idx, 1e-2, 0.9, 0.1)
    unsel = np.ones(p.shape[0], dtype=bool)
    unsel[idx] = False
    for wrong in ("decay_unselected", "momentum_unselected", "write_at_j"):
        bad = SU.dense_loop(p, buf, g, idx, 1e-2, 0.9, 0.1, wrong=wrong)
        assert not same_bits(bad[0], good[0]), wrong
        if wrong != "write_at_j":  # these two touch exactly the rows that must keep their bits, and only those
            assert same_bits(bad[0][idx], good[0][idx]) and not same_bits(bad[0][unsel], p[unsel]), wrong
    assert not np.array_equal(idx, np.arange(idx.shape[0])), "write_at_j needs an idx that is not 0 .. n_s - 1"


# ------------------------------------------------------------------------------------------------ the C ABI


def test_entry_is_declared_exported_and_prototyped():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    assert "int fr_sgd_rows(" in header and "fr_sgd_rows" in _lib.protos and hasattr(lib, "fr_sgd_rows")
    assert _lib.protos["fr_sgd_rows"][2] == ["p", "buf", "g_rows", "idx", "n_s", "D", "lr", "momentum", "wd", "stream"]
    assert _lib.lib.fr_sgd_rows.argtypes == _lib.protos["fr_sgd_rows"][1]
    assert _lib.protos["fr_sgd_rows"][1][4:9] == [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_float, ctypes.c_float]
    assert _lib.lib.fr_abi_version() == 7 and "#define FR_ABI_VERSION 7" in header


def test_entry_rejects_bad_arguments_without_a_gpu():
    from frhip import _lib
    lib = _lib.lib
    buf = (ctypes.c_uint64 * 64)()  # a host address: the checks come before any launch and never follow a pointer
    p = ctypes.cast(buf, ctypes.c_void_p)
    call = lambda ptrs, n_s, d: lib.fr_sgd_rows(ptrs[0], ptrs[1], ptrs[2], ptrs[3], n_s, d, 0.1, 0.9, 1e-2, None)  # noqa: E731
    for hole in range(4):
        ptrs = [None if i == hole else p for i in range(4)]
        assert call(ptrs, 8, 4) == -1 and b"fr_sgd_rows" in lib.fr_last_error_string(), hole
    for d in (0, -1):
        assert call([p] * 4, 8, d) == -1 and b"fr_sgd_rows: D >= 1" in lib.fr_last_error_string(), d
    for n_s in (0, -3):  # nothing selected: nothing launched, whatever the other arguments
        assert call([p] * 4, n_s, 4) == 0 and call([None] * 4, n_s, 0) == 0


# ------------------------------------------------------------------------------------------------ the module


def _kernels():
    from shard_ref_ext import ExtOracleKernels
    from shard_ref_softmax import SoftmaxOracleKernels

    class Kernels(ExtOracleKernels, SoftmaxOracleKernels):
        pass

    return CS.sampling_kernels(Kernels)


def test_constructor_takes_the_option_and_refuses_the_column_sharded_heads():
    from frhip.sharded_head import ShardedMarginLoss
    for name in ("Am_softmax", "CurricularFace"):
        with pytest.raises(ValueError, match="sparse_update=True with head %s" % name):
            ShardedMarginLoss(D, 40, name, sparse_update=True)
        with pytest.raises(ValueError, match="column gather is not built"):  # the older refusal comes first, in its words
            ShardedMarginLoss(D, 40, name, sample_rate=0.5, sparse_update=True)
        assert ShardedMarginLoss(D, 40, name).sparse_update is False
    for name in ("ArcFace", "CosFace", "SphereFace", "Softmax"):
        assert ShardedMarginLoss(D, 40, name, sample_rate=0.5, sparse_update=True).sparse_update is True
        assert ShardedMarginLoss(D, 40, name, sample_rate=0.5).sparse_update is False
    from head import metrics as H
    crit = ShardedMarginLoss.from_head(H.ArcFace(D, 40, None), sample_rate=0.25, sample_seed=3, sparse_update=True)
    assert crit.sparse_update is True and crit.n_s == 10
    with pytest.raises(ValueError, match="sparse_update=True with head Am_softmax"):
        ShardedMarginLoss.from_head(H.Am_softmax(D, 40, None), sparse_update=True)


@pytest.mark.parametrize("name,loss", [("ArcFace", "Focal"), ("Softmax", "Softmax")])
def test_backward_leaves_the_rows_and_a_second_backward_is_refused(name, loss):
    from frhip.sharded_head import ShardedMarginLoss
    g = torch.Generator().manual_seed(2)
    full, bias = torch.randn(40, D, generator=g) * 0.3, (torch.randn(40, generator=g) * 0.1 if name == "Softmax" else None)
    x, y = torch.randn(6, D, generator=g), torch.tensor([0, 39, 4, 4, 17, 20])
    Kd, Ks = _kernels(), _kernels()
    make = lambda K, **kw: ShardedMarginLoss(D, 40, name, kernels=K, full_weight=full, full_bias=bias, loss=loss,  # noqa: E731
                                             sample_seed=5, **kw)
    dense, sparse = make(Kd, sample_rate=0.5), make(Ks, sample_rate=0.5, sparse_update=True)
    xd, xs = x.clone().requires_grad_(True), x.clone().requires_grad_(True)
    ld, ls = dense(xd, y)[0], sparse(xs, y)[0]
    ld.backward()
    ls.backward()
    idx = CS.select(y.numpy(), 40, 20, CS.salt(5, 0), 0)[0]
    sel = torch.from_numpy(idx.astype(np.int64))
    assert torch.equal(ld.detach(), ls.detach()) and torch.equal(xd.grad, xs.grad)
    for k in ("weight",) + (("bias",) if bias is not None else ()):
        pd, ps = getattr(dense, k), getattr(sparse, k)
        got_idx, rows = ps._frhip_row_grad
        assert ps.grad is None and np.array_equal(got_idx.numpy(), idx) and torch.equal(rows, pd.grad[sel]), k
        assert tuple(rows.shape) == (20,) + tuple(ps.shape[1:])
        assert getattr(pd, "_frhip_row_grad", None) is None
    assert Ks.calls == {"sample_classes": 1, "gather_rows": 1 + (bias is not None), "scatter_rows": 0}
    # the row gradients of two steps belong to two index sets
    with pytest.raises(RuntimeError, match="second backward"):
        sparse(x.clone().requires_grad_(True), y)[0].backward()
    sparse.weight._frhip_row_grad = None
    if bias is not None:
        sparse.bias._frhip_row_grad = None
    sparse(x.clone().requires_grad_(True), y)[0].backward()  # consumed: the next one passes
    assert sparse.weight._frhip_row_grad is not None


def test_dense_path_runs_where_nothing_is_sampled():
    """Eval mode, rate 1.0 and a rate whose n_s is the whole shard: the default path's bits, a dense gradient, no rows."""
    from frhip.sharded_head import ShardedMarginLoss
    g = torch.Generator().manual_seed(3)
    full = torch.randn(40, D, generator=g) * 0.3
    x, y = torch.randn(6, D, generator=g), torch.tensor([0, 39, 4, 4, 17, 20])
    make = lambda **kw: ShardedMarginLoss(D, 40, "ArcFace", kernels=_kernels(), full_weight=full, **kw)  # noqa: E731

    def step(crit):
        xx = x.clone().requires_grad_(True)
        loss = crit(xx, y)[0]
        loss.backward()
        return loss.detach(), xx.grad, crit.weight.grad

    base = step(make())
    for kw in (dict(sample_rate=1.0), dict(sample_rate=0.99)):
        crit = make(sparse_update=True, **kw)
        got = step(crit)
        assert all(torch.equal(a, b) for a, b in zip(got, base)), kw
        assert getattr(crit.weight, "_frhip_row_grad", None) is None and sum(crit.kernels.calls.values()) == 0
    crit = make(sparse_update=True, sample_rate=0.5).eval()
    got = step(crit)
    assert all(torch.equal(a, b) for a, b in zip(got, base)) and getattr(crit.weight, "_frhip_row_grad", None) is None
    assert sum(crit.kernels.calls.values()) == 0 and crit.sample_step == 0


# ------------------------------------------------------------------------------------------------ the optimizers


def _param_with_rows():
    p = torch.nn.Parameter(torch.zeros(6, 4))
    p._frhip_row_grad = (torch.tensor([1, 4], dtype=torch.int32), torch.ones(2, 4))
    return p


def test_zero_grad_drops_a_pending_row_gradient():
    from frhip.optim import SGD, Adam
    for make in (lambda ps: SGD(ps, lr=0.1, momentum=0.9), lambda ps: Adam(ps, lr=0.1)):
        for set_to_none in (False, True):
            p, q = _param_with_rows(), torch.nn.Parameter(torch.zeros(3))
            q.grad = torch.ones(3)
            opt = make([p, q])
            opt.zero_grad(set_to_none=set_to_none)
            assert p._frhip_row_grad is None and p.grad is None
            assert q.grad is None if set_to_none else bool((q.grad == 0).all())


def test_adam_refuses_a_row_gradient_naming_the_option():
    from frhip.optim import Adam
    p = _param_with_rows()
    opt = Adam([p], lr=0.1)
    with pytest.raises(NotImplementedError, match="sparse_update"):
        opt.step()
    assert p._frhip_row_grad is not None and bool((p == 0).all())  # nothing was consumed, nothing moved


def test_sgd_refuses_rows_next_to_a_dense_gradient():
    from frhip import _lib
    from frhip.optim import SGD
    p = _param_with_rows()
    p.grad = torch.zeros(6, 4)
    with pytest.raises(_lib.FrhipError, match="row gradient"):
        SGD([p], lr=0.1).step()
    assert p._frhip_row_grad is not None and bool((p == 0).all())


# ------------------------------------------------------------------------------------------------ the driver


def _outcome(train, cfg):
    try:
        train.check_head_config(cfg)
        return None
    except (NotImplementedError, ValueError) as e:
        return type(e).__name__ + ": " + str(e)


def test_check_head_config_refuses_the_three_combinations_and_keeps_everything_else():
    import train
    key = "SHARDED_HEAD_SPARSE_UPDATE"
    ok = dict(HEAD_NAME="ArcFace", SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=0.25, **{key: True})
    for name in ("ArcFace", "CosFace", "SphereFace", "Softmax"):
        for opt in ({}, {"OPTIMIZER_NAME": "SGD"}):
            train.check_head_config(dict(ok, HEAD_NAME=name, **opt))
    for cfg, words in ((dict(HEAD_NAME="ArcFace", SHARDED_HEAD=False, **{key: True}), "needs SHARDED_HEAD=True"),
                       (dict(HEAD_NAME="ArcFace", **{key: True}), "needs SHARDED_HEAD=True"),
                       (dict(ok, SHARDED_HEAD_SAMPLE_RATE=1.0), "SHARDED_HEAD_SAMPLE_RATE=1.0"),
                       (dict(HEAD_NAME="ArcFace", SHARDED_HEAD=True, **{key: True}), "SHARDED_HEAD_SAMPLE_RATE=1.0"),
                       (dict(ok, OPTIMIZER_NAME="Adam"), "OPTIMIZER_NAME 'Adam'"),
                       (dict(ok, OPTIMIZER_NAME="RMSprop"), "OPTIMIZER_NAME 'RMSprop'")):
        with pytest.raises(NotImplementedError) as e:
            train.check_head_config(cfg)
        assert key in str(e.value) and words in str(e.value), (cfg, str(e.value))
    # every config of today -- heads x sharded x rate x optimizer -- keeps its outcome with the key absent or False, and a
    # config that is refused today is refused in the same words with the key set
    heads = ["ArcFace", "CosFace", "SphereFace", "Softmax", "Am_softmax", "CurricularFace", "ArcNegFace"] + sorted(train.NOT_SHARDED)
    refused, passed = 0, 0
    for name in heads:
        for sharded in ({}, {"SHARDED_HEAD": False}, {"SHARDED_HEAD": True}):
            for rate in ({}, {"SHARDED_HEAD_SAMPLE_RATE": 1.0}, {"SHARDED_HEAD_SAMPLE_RATE": 0.5}, {"SHARDED_HEAD_SAMPLE_RATE": 1.5}):
                for opt in ({}, {"OPTIMIZER_NAME": "Adam"}):
                    cfg = dict(HEAD_NAME=name, **sharded, **rate, **opt)
                    was = _outcome(train, cfg)
                    assert _outcome(train, dict(cfg, **{key: False})) == was, cfg
                    now = _outcome(train, dict(cfg, **{key: True}))
                    if was is not None:
                        refused += 1
                        assert now == was, (cfg, was, now)
                    else:
                        passed += 1
                        served = (cfg.get("SHARDED_HEAD", False) and cfg.get("SHARDED_HEAD_SAMPLE_RATE", 1.0) != 1.0
                                  and "OPTIMIZER_NAME" not in cfg)
                        assert (now is None) == served, (cfg, now)
                        assert now is None or key in now, (cfg, now)
    assert refused > 50 and passed > 50
    # the words of today's refusals, spelled out (tests/test_class_sample_host.py pins them on the parent too)
    for table in (train.NOT_SHARDED, train.NOT_SHARDED_ROW_VALUE):
        for name, why in table.items():
            assert _outcome(train, dict(HEAD_NAME=name, SHARDED_HEAD=True, **{key: True})) == (
                "NotImplementedError: SHARDED_HEAD=True with HEAD_NAME '%s': the class-sharded head does not serve %s (%s); "
                "run it replicated, SHARDED_HEAD=False" % (name, name, why))
    assert _outcome(train, dict(HEAD_NAME="ArcFace", SHARDED_HEAD_SAMPLE_RATE=0.25, **{key: True})) == (
        "NotImplementedError: SHARDED_HEAD_SAMPLE_RATE=0.25 needs SHARDED_HEAD=True: classes are sampled by the class-sharded "
        "head only")
    assert _outcome(train, dict(HEAD_NAME="Am_softmax", SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=0.5, **{key: True})) == (
        "NotImplementedError: SHARDED_HEAD_SAMPLE_RATE=0.5 with HEAD_NAME 'Am_softmax': its kernel is [D, N], sharded by "
        "columns, and the column gather of class sampling is not built; run it with SHARDED_HEAD_SAMPLE_RATE=1.0")
    assert _outcome(train, dict(HEAD_NAME="ArcFace", SHARDED_HEAD=True, SHARDED_HEAD_SAMPLE_RATE=0.0, **{key: True})) == (
        "ValueError: SHARDED_HEAD_SAMPLE_RATE must lie in (0, 1], got 0.0")
    src = open(train.__file__).read()
    assert 'sparse_update=cfg.get("SHARDED_HEAD_SPARSE_UPDATE", False)' in src
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert key in common


# ------------------------------------------------------------------------------------------------ gloo


def test_two_ranks_over_gloo_leave_row_gradients():
    env = dict(os.environ)
    env.pop("CUDA_VISIBLE_DEVICES", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29597", os.path.join(HERE, "shard_sparse_gloo_worker.py")]
    out = HS.child(cmd, REPO, env, 240)
    assert out.returncode == 0 and "SHARD_SPARSE_GLOO_WORKER_OK" in out.stdout, out.stdout[-4000:] + out.stderr[-1500:]
