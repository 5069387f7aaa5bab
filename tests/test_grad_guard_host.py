"""Host tests of the gradient guard (no GPU): the numpy restatement of tests/grad_guard_ref.py against
``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.SGD`` on CPU tensors, with negative controls that the same checks catch;
the C ABI of the five new entry points and their argument checks, which run before any launch; the driver's config keys and
the place of ``measure()`` in its loop."""
import ctypes
import inspect
import math
import re

import numpy as np
import pytest
import torch

import grad_guard_ref as G
import loss_optim_ref as R

ENTRIES = ("fr_grad_sumsq", "fr_grad_guard", "fr_sgd_step_ctl", "fr_adam_step_ctl", "fr_sgd_rows_ctl")
EPS32 = 2.0 ** -24  # half an ulp of 1 in fp32: the relative error of one rounding
SIZES = (1, 3, 255, 256, 257, 4095, 4096, 4097, 12289)


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def _grads(seed, scale=1.0):
    rng = np.random.default_rng(seed)
    return [(scale * rng.standard_normal(n)).astype(np.float32) for n in SIZES]


def _fsum_norm(grads):
    return math.sqrt(math.fsum(float(v) * float(v) for g in grads for v in g.astype(np.float64)))


# ------------------------------------------------------------------------------------------------ the checks


def check_norm(norm_of, grads):
    """Within 1 fp32 ulp of the float64 fsum norm.  The bar is derived: the restatement adds at most 2^26 doubles, a relative
    error below 2^26 * 2^-53 = 2^-27 in the sum and half of that in its root -- under a quarter of an fp32 ulp -- before
    the one rounding to fp32 (half an ulp)."""
    want = _fsum_norm(grads)
    got = float(norm_of(grads))
    assert abs(got - want) <= ulp32(want), (got, want, abs(got - want) / ulp32(want))


def torch_coef(norm32, max_norm):
    """torch's expression (torch/nn/utils/clip_grad.py) on the fp32 norm, with a true division:
    clamp(max_norm / (total_norm + 1e-6), max=1.0)."""
    t = torch.tensor(float(norm32), dtype=torch.float32)
    return torch.clamp(torch.tensor(max_norm, dtype=torch.float32) / (t + 1e-6), max=1.0).numpy()


def check_coef(ctl_of, grads, max_norm):
    ctl = ctl_of(grads, max_norm)
    want = torch_coef(ctl[0], max_norm)
    assert np.float32(ctl[1]).tobytes() == np.float32(want).tobytes(), (ctl, want, max_norm)


def _torch_clip_sgd(ps, gs, bufs, max_norm, wd, momentum, lr):
    """clip_grad_norm_ + one torch.optim.SGD step in float64 on the fp32 values: (total norm, params, buffers)."""
    params = [torch.nn.Parameter(torch.from_numpy(p).double().clone()) for p in ps]
    opt = torch.optim.SGD(params, lr=lr, momentum=momentum, weight_decay=wd)
    for q, g, b in zip(params, gs, bufs):
        q.grad = torch.from_numpy(g).double().clone()
        opt.state[q]["momentum_buffer"] = torch.from_numpy(b).double().clone()
    total = torch.nn.utils.clip_grad_norm_(params, max_norm)
    opt.step()
    return float(total), [q.detach().numpy() for q in params], [opt.state[q]["momentum_buffer"].numpy() for q in params]


def check_step(step_of, seed, max_norm, scale):
    """``step_of(ps, gs, bufs, max_norm, wd, momentum, lr) -> (ps', bufs')`` against torch in float64.  The restatement
    differs from it by the fp32 roundings of the coefficient -- the norm, the sum with 1e-6, the quotient -- and of the
    product g * c: |g' - g'64| <= 4 e |g'64| to first order, e = 2^-24; the step itself is float64 on both sides, so
    |buf - buf64| <= that and |p - p64| <= lr times that.  Bar: the bound times 1.001 for the second order, plus 1e-12 for
    float64's own roundings (the bar of tests/test_loss_optim_host.py)."""
    rng = np.random.default_rng(seed)
    gs = _grads(seed, scale)
    ps = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    bufs = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    wd, momentum, lr = 2e-3, 0.9, 0.03
    total, tp, tb = _torch_clip_sgd(ps, gs, bufs, max_norm, wd, momentum, lr)
    c64 = min(1.0, max_norm / (total + 1e-6))
    gp, gb = step_of(ps, gs, bufs, max_norm, wd, momentum, lr)
    worst = 0.0
    for t in range(len(SIZES)):
        bound = 4.004 * EPS32 * np.abs(gs[t].astype(np.float64) * c64)
        eb, ep = np.abs(gb[t] - tb[t]), np.abs(gp[t] - tp[t])
        assert (eb <= bound + 1e-12).all() and (ep <= lr * bound + 1e-12).all(), (
            t, SIZES[t], float((eb / (bound + 1e-12)).max()), float((ep / (lr * bound + 1e-12)).max()))
        worst = max(worst, float(eb.max()))
    return c64, worst


# ------------------------------------------------------------------------------------------------ the restatement


def _ref_ctl(grads, max_norm, skip=True):
    return G.ctl_ref(G.parts_ref(grads, G.pairs_of([g.size for g in grads])), max_norm, skip)


def _ref_step(ps, gs, bufs, max_norm, wd, momentum, lr, ctl_of=_ref_ctl):
    ctl = ctl_of(gs, max_norm)
    out = [G.sgd_step_ctl_ref(p, g, b, wd, momentum, lr, ctl, True) for p, g, b in zip(ps, gs, bufs)]
    return [o[0] for o in out], [o[1] for o in out]


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_norm_within_one_ulp_of_the_fsum_norm(scale):
    check_norm(lambda grads: _ref_ctl(grads, 1.0)[0], _grads(21, scale))


@pytest.mark.parametrize("max_norm", [1e-7, 0.5, 1.0, 100.0, 1e6])
def test_coefficient_is_torchs_expression(max_norm):
    for scale in (1e-3, 1.0, 1e3):
        check_coef(_ref_ctl, _grads(22, scale), max_norm)
    check_coef(_ref_ctl, [np.zeros(n, np.float32) for n in SIZES], max_norm)  # all-zero gradients: max_norm / 1e-6, clamped


def test_clipped_and_unclipped_steps_against_torch():
    """A norm above max_norm (clipped, c < 1) and one below it (c = 1: the plain step)."""
    c, worst = check_step(_ref_step, 23, 5.0, 1.0)
    assert c < 0.1 and worst > 0  # the gradients were clipped, and fp32 did round: the bound is not vacuous
    c, _ = check_step(_ref_step, 24, 5.0, 1e-3)
    assert c == 1.0


def test_measure_only_and_the_empty_set():
    g = _grads(25)
    ctl = _ref_ctl(g, None)
    assert ctl[1] == 1.0 and ctl[2] == 1.0 and ctl[3] == 0.0 and ctl[0] > 0
    assert _ref_ctl(g, 0.0)[1] == 1.0 and _ref_ctl(g, -1.0)[1] == 1.0
    assert G.ctl_ref(np.zeros(0), 5.0, True).tolist() == [0.0, 1.0, 1.0, 0.0]


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_gradients_follow_torch(bad):
    """With skipping the go flag is 0; without it the coefficient is torch's: an infinite norm gives 0, a NaN a NaN."""
    g = _grads(26)
    g[6][4095] = bad
    on, off = _ref_ctl(g, 5.0, True), _ref_ctl(g, 5.0, False)
    assert on[2] == 0.0 and off[2] == 1.0
    params = [torch.nn.Parameter(torch.zeros(v.size)) for v in g]
    for q, v in zip(params, g):
        q.grad = torch.from_numpy(v.copy())
    with torch.no_grad():
        total = torch.nn.utils.clip_grad_norm_(params, 5.0)
    if np.isnan(bad):
        assert np.isnan(off[0]) and np.isnan(off[1]) and bool(torch.isnan(total))
        assert bool(torch.isnan(params[0].grad).all())  # torch multiplies every gradient by the NaN coefficient
    else:
        assert np.isinf(off[0]) and off[1] == 0.0 and bool(torch.isinf(total))
        assert float(params[0].grad.abs().max()) == 0.0  # inf -> coefficient 0
    p, b = np.ones(4, np.float32), np.full(4, 2.0, np.float32)
    sp, sb = G.sgd_step_ctl_ref(p, np.full(4, bad, np.float32), b, 0.5, 0.5, 0.25, on, True)
    assert sp.tobytes() == p.astype(np.float64).tobytes() and sb.tobytes() == b.astype(np.float64).tobytes()


# ------------------------------------------------------------------------------------------------ negative controls


def test_a_sum_of_squares_without_the_root_is_caught():
    def no_root(grads):
        return np.float32(G.total_ref(G.parts_ref(grads, G.pairs_of([g.size for g in grads]))))

    with pytest.raises(AssertionError):
        check_norm(no_root, _grads(21))


def _ctl_no_clamp(grads, max_norm):
    ctl = _ref_ctl(grads, max_norm)
    ctl[1] = np.float32(max_norm) / np.float32(ctl[0] + np.float32(1e-6))
    return ctl


def test_a_coefficient_without_the_clamp_is_caught():
    """It scales small gradients up: the step misses torch's, and the coefficient misses torch's expression."""
    with pytest.raises(AssertionError):
        check_step(lambda *a: _ref_step(*a, ctl_of=_ctl_no_clamp), 24, 5.0, 1e-3)
    with pytest.raises(AssertionError):
        check_coef(_ctl_no_clamp, _grads(24, 1e-3), 5.0)
    check_step(lambda *a: _ref_step(*a, ctl_of=_ctl_no_clamp), 23, 5.0, 1.0)  # (above max_norm the clamp does nothing)


def test_the_missing_epsilon_is_caught_on_all_zero_gradients():
    """max_norm / 0 is inf, which the clamp turns into 1; torch's max_norm / 1e-6 is 0.1 at max_norm 1e-7."""
    def no_eps(grads, max_norm):
        ctl = _ref_ctl(grads, max_norm)
        with np.errstate(divide="ignore"):
            c = np.float32(max_norm) / np.float32(ctl[0])
        ctl[1] = np.float32(1.0) if c > 1 else c
        return ctl

    zeros = [np.zeros(n, np.float32) for n in SIZES]
    with pytest.raises(AssertionError):
        check_coef(no_eps, zeros, 1e-7)
    check_coef(_ref_ctl, zeros, 1e-7)


def test_a_skip_that_only_zeroes_the_gradient_is_caught():
    """Weight decay and momentum still move p and buf under a zeroed gradient; a skipped step keeps their bits, as a step
    that torch.cuda.amp.GradScaler does not take."""
    rng = np.random.default_rng(27)
    p, b = rng.standard_normal(257).astype(np.float32), rng.standard_normal(257).astype(np.float32)
    g = np.full(257, np.nan, np.float32)
    ctl = np.array([np.nan, np.nan, 0.0, 0.0], np.float32)

    def kept(step):
        sp, sb = step(p, g, b)
        assert np.array_equal(sp, p.astype(np.float64)) and np.array_equal(sb, b.astype(np.float64))

    kept(lambda p, g, b: G.sgd_step_ctl_ref(p, g, b, 2e-3, 0.9, 0.03, ctl, True))
    with pytest.raises(AssertionError):
        kept(lambda p, g, b: R.sgd_step_ref(p, np.zeros_like(g), b, 2e-3, 0.9, 0.03))
    sc = R.adam_scalars(1e-3, (0.9, 0.999), 1e-8, 1)
    ap, am, av = G.adam_step_ctl_ref(p, g, b, np.abs(b), sc, ctl, True)
    assert ap.tobytes() == p.tobytes() and am.tobytes() == b.tobytes() and av.tobytes() == np.abs(b).tobytes()


def test_the_order_of_a_chunk_is_the_documented_one():
    """Restated once more, element by element in python floats, on a chunk with a ragged tail."""
    x = _grads(28)[5][:1000]
    acc = [0.0] * 256
    for i, v in enumerate(x):
        acc[i % 256] = acc[i % 256] + float(v) * float(v)  # i ascending: thread i % 256 sees its elements in order
    waves = []
    for w in range(4):
        v = acc[64 * w:64 * w + 64]
        h = 32
        while h:
            v = [v[l] + v[l + h] for l in range(h)]
            h //= 2
        waves.append(v[0])
    assert G.chunk_sumsq(x) == ((waves[0] + waves[1]) + waves[2]) + waves[3]
    assert G.pairs_of((1, 4096, 4097)) == [(0, 0), (1, 0), (2, 0), (2, 1)]


# ------------------------------------------------------------------------------------------------ the C ABI


def test_entries_are_declared_exported_and_prototyped():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.protos and hasattr(lib, name), name
    assert _lib.lib.fr_abi_version() == 7  # no existing struct changed
    assert _lib.lib.fr_struct_size(10) == ctypes.sizeof(_lib.FrGradTensor) == 16
    assert [f[0] for f in _lib.FrGradTensor._fields_] == ["g", "n"]
    assert _lib.self_check()
    names = {name: _lib.protos[name][2] for name in ENTRIES}
    assert names["fr_grad_sumsq"] == ["table_dev", "chunks_dev", "nchunks", "parts", "stream"]
    assert names["fr_grad_guard"] == ["parts", "nparts", "max_norm", "skip_nonfinite", "ctl", "skipped", "stream"]
    assert names["fr_sgd_step_ctl"] == _lib.protos["fr_sgd_step"][2][:-1] + ["ctl", "use_coef", "stream"]
    assert names["fr_adam_step_ctl"] == _lib.protos["fr_adam_step"][2][:-1] + ["ctl", "use_coef", "stream"]
    assert names["fr_sgd_rows_ctl"] == _lib.protos["fr_sgd_rows"][2][:-1] + ["ctl", "stream"]


def test_entry_points_refuse_bad_arguments_and_keep_the_no_op_without_a_gpu():
    """A missing pointer with something to launch and nparts < 0 are refused before any launch (-1, the entry's name first
    in the message); nchunks <= 0 and n_s <= 0 return 0 whatever the pointers.  No call follows a pointer."""
    from frhip import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)  # a pointer that is not NULL; no call below gets as far as a launch

    def refused(name, rc):
        assert rc == -1, (name, rc)
        assert lib.fr_last_error_string().startswith(name.encode() + b":"), lib.fr_last_error_string()

    gtab = ctypes.cast(one, ctypes.POINTER(_lib.FrGradTensor))
    stab = ctypes.cast(one, ctypes.POINTER(_lib.FrSgdTensor))
    atab = ctypes.cast(one, ctypes.POINTER(_lib.FrAdamTensor))
    assert lib.fr_grad_sumsq(None, None, 0, None, None) == 0 and lib.fr_grad_sumsq(gtab, one, -2, one, None) == 0
    for args in ((None, one, 3, one), (gtab, None, 3, one), (gtab, one, 3, None)):
        refused("fr_grad_sumsq", lib.fr_grad_sumsq(*args, None))
    refused("fr_grad_guard", lib.fr_grad_guard(one, -1, 5.0, 1, one, one, None))
    refused("fr_grad_guard", lib.fr_grad_guard(None, 3, 5.0, 1, one, one, None))
    refused("fr_grad_guard", lib.fr_grad_guard(one, 3, 5.0, 1, None, one, None))
    refused("fr_grad_guard", lib.fr_grad_guard(one, 3, float("nan"), 1, one, one, None))
    assert lib.fr_sgd_step_ctl(None, None, 0, 0.03, 0.9, None, 1, None) == 0
    assert lib.fr_sgd_step_ctl(stab, one, -3, 0.03, 0.9, one, 1, None) == 0
    for args in ((None, one, 4, 0.03, 0.9, one), (stab, None, 4, 0.03, 0.9, one), (stab, one, 4, 0.03, 0.9, None)):
        refused("fr_sgd_step_ctl", lib.fr_sgd_step_ctl(*args, 1, None))
    adam = (1e-3, 0.1, 0.999, 0.001, 1e-8, 0.03)
    assert lib.fr_adam_step_ctl(None, None, 0, *adam, None, 1, None) == 0
    for args in ((None, one, 4) + adam + (one,), (atab, None, 4) + adam + (one,), (atab, one, 4) + adam + (None,)):
        refused("fr_adam_step_ctl", lib.fr_adam_step_ctl(*args, 0, None))
    assert lib.fr_sgd_rows_ctl(None, None, None, None, 0, 4, 0.1, 0.9, 0.0, None, None) == 0
    for missing in range(4):
        ptrs = [None if i == missing else one for i in range(4)]
        refused("fr_sgd_rows_ctl", lib.fr_sgd_rows_ctl(*ptrs, 2, 4, 0.1, 0.9, 0.0, one, None))
    refused("fr_sgd_rows_ctl", lib.fr_sgd_rows_ctl(one, one, one, one, 2, 4, 0.1, 0.9, 0.0, None, None))
    refused("fr_sgd_rows_ctl", lib.fr_sgd_rows_ctl(one, one, one, one, 2, 0, 0.1, 0.9, 0.0, one, None))


# ------------------------------------------------------------------------------------------------ the module, the driver


def test_grad_guard_refuses_host_parameters_and_bad_max_norm():
    from frhip import _lib
    from frhip.optim import GradGuard
    p = torch.nn.Parameter(torch.zeros(4))
    with pytest.raises(_lib.FrhipError, match="GradGuard"):
        GradGuard([p], max_norm=1.0)
    for bad in (-1.0, 0.0, float("nan"), "5", True):
        with pytest.raises(ValueError, match="max_norm"):
            GradGuard([p], max_norm=bad)
    with pytest.raises(NotImplementedError, match="norm type 2"):
        GradGuard([p], max_norm=1.0, norm_type=1.0)
    with pytest.raises(ValueError):
        GradGuard([], max_norm=1.0)


def test_config_validation():
    import train
    for absent in ({}, {"GRAD_CLIP_NORM": None}, {"SKIP_NONFINITE_STEP": False},
                   {"GRAD_CLIP_NORM": None, "SKIP_NONFINITE_STEP": False}):
        assert train.check_guard_config(absent) is None  # no guard is built
    assert train.check_guard_config({"GRAD_CLIP_NORM": 5}) == (5.0, False)
    assert train.check_guard_config({"GRAD_CLIP_NORM": 0.5, "SKIP_NONFINITE_STEP": True}) == (0.5, True)
    assert train.check_guard_config({"SKIP_NONFINITE_STEP": True}) == (None, True)
    for bad in (0, 0.0, -1.0, float("nan"), "5.0", True):
        with pytest.raises(ValueError, match="GRAD_CLIP_NORM"):
            train.check_guard_config({"GRAD_CLIP_NORM": bad})
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="SKIP_NONFINITE_STEP"):
            train.check_guard_config({"SKIP_NONFINITE_STEP": bad})
    import os
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "GRAD_CLIP_NORM=None" in common and "SKIP_NONFINITE_STEP=False" in common
    from configs._common import stage3
    assert train.check_guard_config(stage3("x")) is None  # the shipped defaults are off


def test_main_measures_between_synchronize_and_step():
    import train
    src = inspect.getsource(train.main)
    sync = src.index("BACKBONE.synchronize()")
    measure = src.index("guard.measure()")
    step = src.index("optimizer.step(guard=guard)")
    assert sync < measure < step
    assert not re.search(r"\S", src[measure + len("guard.measure()"):step])  # nothing between the two
    assert "check_guard_config(cfg)" in src and src.index("check_head_config(cfg)") < src.index("check_guard_config(cfg)")
    assert src.count("optimizer.step()") == 1 and "if guard is None:" in src  # the loop without a guard is today's
    assert 'run_state["grad_guard"] = guard.state_dict()' in src
