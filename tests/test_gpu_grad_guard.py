"""The gradient guard on the GPU: fr_grad_sumsq / fr_grad_guard bit for bit against the numpy restatement of
tests/grad_guard_ref.py in a sentinel-banded arena, non-finite gradients, the three _ctl step entries against the entries
they extend, ``frhip.optim.GradGuard`` with ``SGD``, one IR-50 training step, and train.py end to end with a resume.

Sizes: 1, 3, 255, 256, 257 (the 256 threads of a workgroup), 4095, 4096, 4097 (the chunk) and 12289 (three chunks and one
element) -- the smallest that cross every boundary of the kernels."""
import ctypes
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_guard_ref as G  # noqa: E402
import head_support as HS  # noqa: E402
import loss_optim_ref as R  # noqa: E402
from frhip import _lib, ops, synth  # noqa: E402

SIZES = (1, 3, 255, 256, 257, 4095, 4096, 4097, 12289)
GAP = 67  # sentinel floats between neighbours: odd, so the offsets run through every residue modulo 4
SENTINEL = HS.SENTINEL
WD = tuple(float(np.float32(w / 250)) for w in (0.5, 0.25, 0.125, 0.0, 0.5, 0.125, 0.25, 0.5, 0.25))  # per tensor


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def bits(a):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and np.array_equal(a, b)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


class Arena(object):
    """``names`` x SIZES float32 tensors carved from ONE guarded buffer, a GAP of sentinels in front of each, at offsets
    that are multiples of 4 bytes and never of 16."""

    def __init__(self, names):
        self.names = names
        self.off, at = {}, 0
        for name in names:
            for t, n in enumerate(SIZES):
                at += GAP
                if at % 4 == 0:
                    at += 1
                self.off[name, t] = (at, n)
                at += n
        self.g = HS.Guarded(at + GAP)
        self.base = self.g.t.data_ptr()
        assert self.base % 16 == 0 and all(o % 4 for o, _ in self.off.values())
        self.host = np.full(at + GAP, SENTINEL, dtype=np.float32)

    def fill(self, values):
        """values[name, t] -> the arena, uploaded."""
        for (name, t), v in values.items():
            if name in self.names:
                o, n = self.off[name, t]
                self.host[o:o + n] = v
        self.g.t.copy_(torch.from_numpy(self.host))
        return self

    def ptr(self, name, t):
        return self.base + 4 * self.off[name, t][0]

    def download(self, what):
        """The tensors as numpy after asserting the guards; the gaps between the tensors must hold the sentinel."""
        torch.cuda.synchronize()
        self.g.assert_guards(what)
        got = self.g.t.cpu().numpy()
        inside = np.zeros(got.shape, dtype=bool)
        for o, n in self.off.values():
            inside[o:o + n] = True
        assert (got[~inside] == np.float32(SENTINEL)).all(), (what, "a band between two tensors was written",
                                                               int((got[~inside] != np.float32(SENTINEL)).sum()))
        return {key: got[o:o + n].copy() for key, (o, n) in self.off.items()}


class Banded(object):
    """A buffer of ``n`` elements of ``dtype`` between two bands of ``fill``."""
    BAND = 64

    def __init__(self, n, dtype, fill):
        self.fill = fill
        self.flat = torch.full((2 * self.BAND + n,), fill, dtype=dtype, device="cuda")
        self.t = self.flat[self.BAND:self.BAND + n]

    def assert_bands(self, what):
        assert bool((self.flat[:self.BAND] == self.fill).all()) and bool((self.flat[self.BAND + self.t.numel():] == self.fill).all()), (
            what, "band written")


def device_table(struct, records):
    arr = (struct * len(records))()
    for i, rec in enumerate(records):
        for key, value in rec.items():
            setattr(arr[i], key, value)
    raw = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).cuda()
    return raw, ctypes.cast(ctypes.c_void_p(raw.data_ptr()), ctypes.POINTER(struct))


def shuffled_pairs(seed):
    assert _lib.lib.fr_sgd_chunk_elems() == G.CHUNK == 4096  # SIZES straddle it
    pairs = G.pairs_of(SIZES)
    order = np.random.default_rng(seed).permutation(len(pairs))
    assert not np.array_equal(order, np.arange(len(pairs)))
    return [pairs[i] for i in order]


def run_guard(grads, pairs, max_norm, skip, skipped0=(0, 0), what="guard"):
    """fr_grad_sumsq + fr_grad_guard over ``grads[t]`` in a banded arena: (parts float64, ctl float32 [4], skipped int32 [2])
    after checking that the gradients and every band are untouched."""
    arena = Arena(("g",)).fill({("g", t): g for t, g in enumerate(grads)})
    raw, table = device_table(_lib.FrGradTensor, [dict(g=arena.ptr("g", t), n=n) for t, n in enumerate(SIZES)])
    chunks = dev(np.array(pairs, dtype=np.int32).reshape(-1))
    parts = Banded(len(pairs), torch.float64, -7.0)
    ctl = Banded(4, torch.float32, SENTINEL)
    skipped = Banded(2, torch.int32, -99)
    skipped.t.copy_(torch.tensor(skipped0, dtype=torch.int32))
    st = ops.current_stream_ptr()
    ops.Launch("fr_grad_sumsq", [table, ctypes.c_void_p(chunks.data_ptr()), len(pairs), ops.ptr(parts.t), st])()
    ops.Launch("fr_grad_guard", [ops.ptr(parts.t), len(pairs), float(max_norm), int(skip), ops.ptr(ctl.t),
                                 ops.ptr(skipped.t), st])()
    got = arena.download(what)
    for t, g in enumerate(grads):
        assert same(got["g", t], g), (what, "a gradient was written", t)
    for b in (parts, ctl, skipped):
        b.assert_bands(what)
    return parts.t.cpu().numpy(), ctl.t.cpu().numpy(), skipped.t.cpu().numpy()


# ------------------------------------------------------------------------------------------------ fr_grad_sumsq, fr_grad_guard


@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e3])
def test_sumsq_and_guard_bit_for_bit_on_random_operands(scale):
    """Every part, the norm and the coefficient have the bits of the restatement; a second run has the bits of the first."""
    rng = np.random.default_rng(31)
    grads = [(scale * rng.standard_normal(n)).astype(np.float32) for n in SIZES]
    pairs = shuffled_pairs(32)
    max_norm = 5.0 * scale
    parts, ctl, skipped = run_guard(grads, pairs, max_norm, 1)
    want_parts = G.parts_ref(grads, pairs)
    assert same(parts, want_parts), ("parts", int((bits(parts) != bits(want_parts)).sum()), parts[:4], want_parts[:4])
    want = G.ctl_ref(want_parts, max_norm, True)
    assert same(ctl, want), (ctl, want)
    assert 0 < ctl[1] < 1 and ctl[2] == 1.0 and skipped.tolist() == [0, 1]
    parts2, ctl2, _ = run_guard(grads, pairs, max_norm, 1)
    assert same(parts, parts2) and same(ctl, ctl2), "two runs differ"
    # another order of the chunk list permutes the parts and changes none
    other = shuffled_pairs(33)
    parts3, _, _ = run_guard(grads, other, max_norm, 1)
    assert {p: v for p, v in zip(pairs, bits(parts))} == {p: v for p, v in zip(other, bits(parts3))}
    # measure only
    _, ctl4, _ = run_guard(grads, pairs, 0.0, 1)
    assert same(ctl4, G.ctl_ref(want_parts, None, True)) and ctl4[1] == 1.0 and ctl4[0] == ctl[0]


@pytest.mark.parametrize("where", ["first", "last", "boundary", "boundary-1"])
def test_sumsq_counts_every_element_once_on_exact_operands(where):
    """Integers in [-8, 8] and one planted 2^(10 + t) per tensor t at its first, last, chunk-boundary (4096) or
    chunk-boundary-minus-one element: every square and every sum is an integer below 2^53, exact in any order, and the
    planted squares 4^(10 + t) are distinct bits above everything else -- a missed or doubly counted element shows in the
    part and in the total itself."""
    rng = np.random.default_rng(34)
    grads = [rng.integers(-8, 9, size=n).astype(np.float32) for n in SIZES]
    for t, g in enumerate(grads):
        at = {"first": 0, "last": g.size - 1, "boundary": 4096, "boundary-1": 4095}[where]
        if at < g.size:
            g[at] = 2.0 ** (10 + t)
    pairs = shuffled_pairs(35)
    parts, ctl, _ = run_guard(grads, pairs, 0.0, 1, what=where)
    exact = [sum(int(v) ** 2 for v in grads[t][c * 4096:(c + 1) * 4096]) for t, c in pairs]
    assert [int(v) for v in parts] == exact and all(float(int(v)) == v for v in parts), (where, parts, exact)
    total = sum(exact)
    assert total == sum(int(v) ** 2 for g in grads for v in g) and total < 2 ** 53
    assert same(ctl, np.array([np.sqrt(np.float64(total)), 1.0, 1.0, 0.0], dtype=np.float32)), (where, ctl, total)
    assert same(parts, G.parts_ref(grads, pairs))


@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_gradients(bad):
    """One non-finite value at index 0, at 4095 / 4096 of a multi-chunk tensor and at the last element of the last tensor.
    Skipping on: go 0, skipped[0] + 1.  Skipping off: go 1 and torch's coefficient -- inf gives 0, NaN gives NaN."""
    rng = np.random.default_rng(36)
    clean = [rng.standard_normal(n).astype(np.float32) for n in SIZES]
    pairs = shuffled_pairs(37)
    last = len(SIZES) - 1
    for t, at in ((0, 0), (last, 4095), (last, 4096), (last, SIZES[last] - 1)):
        grads = [g.copy() for g in clean]
        grads[t][at] = bad
        _, on, skipped_on = run_guard(grads, pairs, 5.0, 1, skipped0=(3, 10), what="skip on")
        _, off, skipped_off = run_guard(grads, pairs, 5.0, 0, skipped0=(3, 10), what="skip off")
        tag = (bad, t, at, on, off)
        assert on[2] == 0.0 and on[3] == 0.0 and skipped_on.tolist() == [4, 11], tag
        assert off[2] == 1.0 and skipped_off.tolist() == [3, 11], tag
        if np.isnan(bad):
            assert np.isnan(off[0]) and np.isnan(off[1]), tag
        else:
            assert off[0] == np.inf and off[1] == 0.0, tag
        assert same(on[:2], off[:2]) or np.isnan(bad), tag
    _, ok, skipped = run_guard(clean, pairs, 5.0, 1, skipped0=(3, 10))
    assert ok[2] == 1.0 and skipped.tolist() == [3, 11]


def test_guard_without_parts_and_without_counters():
    """nparts == 0 (nothing had a gradient) gives {0, 1, 1, 0}, with parts NULL; skipped may be NULL."""
    ctl = Banded(4, torch.float32, SENTINEL)
    skipped = Banded(2, torch.int32, -99)
    skipped.t.zero_()
    st = ops.current_stream_ptr()
    ops.Launch("fr_grad_guard", [None, 0, 5.0, 1, ops.ptr(ctl.t), ops.ptr(skipped.t), st])()
    torch.cuda.synchronize()
    assert ctl.t.tolist() == [0.0, 1.0, 1.0, 0.0] and skipped.t.tolist() == [0, 1]
    ctl.t.fill_(SENTINEL)
    ops.Launch("fr_grad_guard", [None, 0, 0.0, 0, ops.ptr(ctl.t), None, st])()
    torch.cuda.synchronize()
    assert ctl.t.tolist() == [0.0, 1.0, 1.0, 0.0] and skipped.t.tolist() == [0, 1]
    ctl.assert_bands("ctl")
    skipped.assert_bands("skipped")


# ------------------------------------------------------------------------------------------------ fr_sgd_step_ctl

COEF = 0.3  # rounds in fp32 and in every product with a gradient


def _ctl(norm, coef, go):
    return dev(np.array([norm, coef, go, 0.0], dtype=np.float32))


def _sgd_run(start, entry, ctl=None, use_coef=0, lr=0.03, momentum=0.9, seed=41):
    arena = Arena(("p", "g", "buf")).fill(start)
    raw, table = device_table(_lib.FrSgdTensor, [dict(p=arena.ptr("p", t), g=arena.ptr("g", t), buf=arena.ptr("buf", t), n=n,
                                                      wd=WD[t]) for t, n in enumerate(SIZES)])
    pairs = shuffled_pairs(seed)
    chunks = dev(np.array(pairs, dtype=np.int32).reshape(-1))
    args = [table, ctypes.c_void_p(chunks.data_ptr()), len(pairs), lr, momentum]
    if entry == "fr_sgd_step_ctl":
        args += [ops.ptr(ctl), use_coef]
    ops.Launch(entry, args + [ops.current_stream_ptr()])()
    got = arena.download(entry)
    for t in range(len(SIZES)):
        assert same(got["g", t], start["g", t]), (entry, "g was written", t)
    return got


def _same_tensors(a, b, names, what):
    for name in names:
        for t in range(len(SIZES)):
            diff = int((bits(a[name, t]) != bits(b[name, t])).sum())
            assert diff == 0, (what, name, t, SIZES[t], diff)


def test_sgd_step_ctl():
    rng = np.random.default_rng(42)
    start = {(name, t): rng.standard_normal(n).astype(np.float32) for name in ("p", "g", "buf") for t, n in enumerate(SIZES)}
    plain = _sgd_run(start, "fr_sgd_step")
    assert not same(plain["p", 8], start["p", 8])
    # coefficient 1: bit for bit fr_sgd_step
    _same_tensors(_sgd_run(start, "fr_sgd_step_ctl", _ctl(7.0, 1.0, 1.0), 1), plain, ("p", "buf"), "coefficient 1")
    # a coefficient below 1: the gradients scaled in place in fp32, then fr_sgd_step
    scaled = dict(start)
    for t in range(len(SIZES)):
        scaled["g", t] = start["g", t] * np.float32(COEF)
    want = _sgd_run(scaled, "fr_sgd_step")
    got = _sgd_run(start, "fr_sgd_step_ctl", _ctl(7.0, COEF, 1.0), 1)
    _same_tensors(got, want, ("p", "buf"), "coefficient %r" % COEF)
    assert not same(got["p", 8], plain["p", 8])
    # use_coef = 0 ignores the coefficient
    _same_tensors(_sgd_run(start, "fr_sgd_step_ctl", _ctl(7.0, COEF, 1.0), 0), plain, ("p", "buf"), "use_coef 0")
    # go 0: nothing moves, whatever the coefficient
    for coef in (COEF, np.nan):
        _same_tensors(_sgd_run(start, "fr_sgd_step_ctl", _ctl(np.inf, coef, 0.0), 1), start, ("p", "buf"), "go 0")


# ------------------------------------------------------------------------------------------------ fr_adam_step_ctl


@pytest.mark.parametrize("case", ["coefficient 1", "coefficient below 1", "use_coef 0", "go 0"])
def test_adam_step_ctl_three_steps(case):
    """p, m and v after each of three steps are bit for bit the np.float32 restatement on g * ctl[1] (or on g), and keep
    their bits on a skipped step; with coefficient 1 they are also the bits fr_adam_step leaves."""
    coef, use_coef, go = {"coefficient 1": (1.0, 1, 1.0), "coefficient below 1": (COEF, 1, 1.0),
                          "use_coef 0": (COEF, 0, 1.0), "go 0": (COEF, 1, 0.0)}[case]
    ctl_host = np.array([7.0, coef, go, 0.0], dtype=np.float32)
    ctl = dev(ctl_host)
    rng = np.random.default_rng(43)
    state = {}
    for t, n in enumerate(SIZES):
        state["p", t] = rng.standard_normal(n).astype(np.float32)
        state["m", t] = (0.1 * rng.standard_normal(n)).astype(np.float32)
        state["v", t] = (0.01 * rng.standard_normal(n) ** 2).astype(np.float32)
    pairs = shuffled_pairs(44)
    chunks = dev(np.array(pairs, dtype=np.int32).reshape(-1))
    lr, betas, eps = 1e-3, (0.9, 0.999), 1e-8
    for step, scale in enumerate((1e-3, 1.0, 1e3), 1):
        for t, n in enumerate(SIZES):
            state["g", t] = (scale * rng.standard_normal(n)).astype(np.float32)
        sc = R.adam_scalars(lr, betas, eps, step)
        scalars = [float(sc[key]) for key in ("step_size", "w1", "beta2", "w2", "eps", "bc2_sqrt")]
        results = []
        for entry in ("fr_adam_step_ctl",) + (("fr_adam_step",) if case == "coefficient 1" else ()):
            arena = Arena(("p", "g", "m", "v")).fill(state)
            raw, table = device_table(_lib.FrAdamTensor, [dict(p=arena.ptr("p", t), g=arena.ptr("g", t), m=arena.ptr("m", t),
                                                               v=arena.ptr("v", t), n=n) for t, n in enumerate(SIZES)])
            tail = [ops.ptr(ctl), use_coef] if entry == "fr_adam_step_ctl" else []
            ops.Launch(entry, [table, ctypes.c_void_p(chunks.data_ptr()), len(pairs)] + scalars + tail +
                       [ops.current_stream_ptr()])()
            results.append(arena.download("%s, step %d" % (entry, step)))
        got = results[0]
        if len(results) == 2:
            _same_tensors(got, results[1], ("p", "m", "v"), "fr_adam_step")
        for t in range(len(SIZES)):
            p, m, v = G.adam_step_ctl_ref(state["p", t], state["g", t], state["m", t], state["v", t], sc, ctl_host, use_coef)
            for name, want in (("p", p), ("m", m), ("v", v)):
                diff = int((bits(got[name, t]) != bits(want)).sum())
                assert diff == 0, (case, step, name, t, SIZES[t], diff, "elements differ from the fp32 restatement")
            assert same(got["g", t], state["g", t])
            if go == 0.0:
                assert same(p, state["p", t]) and same(m, state["m", t])
            else:
                assert not same(p, state["p", t]) or SIZES[t] == 1
            state["p", t], state["m", t], state["v", t] = p, m, v


# ------------------------------------------------------------------------------------------------ fr_sgd_rows_ctl


def _idx_sets(n, n_s):
    """The row sets of tests/test_gpu_sparse_update.py: ascending, distinct, holding row 0 and row n - 1."""
    if n_s == n:
        return [np.arange(n, dtype=np.int32)]
    if n_s == 1:
        return [np.array([0], dtype=np.int32), np.array([n - 1], dtype=np.int32)]
    inner = 1 + np.random.RandomState(n_s).permutation(n - 2)[:n_s - 2]
    return [np.sort(np.concatenate([[0, n - 1], inner])).astype(np.int32)]


@pytest.mark.parametrize("d", [1, 4, 6, 512])
@pytest.mark.parametrize("n,n_s", [(1, 1), (33, 1), (300, 77), (300, 300)])
def test_sgd_rows_ctl(n, n_s, d):
    """go 1: the bits of fr_sgd_rows whatever the coefficient (the head is not clipped); go 0: p, buf and the bands keep
    their bits."""
    rng = np.random.RandomState(1000 * d + n + n_s)
    f = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    p0, b0, g0 = f(n, d), f(n, d), f(n_s, d)
    lr, mom, wd = 0.1, 0.9, 5e-4
    for idx in _idx_sets(n, n_s):
        idx_dev = dev(idx)

        def run(entry, ctl=None):
            gp, gb, gg = HS.Guarded(n, d), HS.Guarded(n, d), HS.Guarded(n_s, d)
            gp.t.copy_(torch.from_numpy(p0))
            gb.t.copy_(torch.from_numpy(b0))
            gg.t.copy_(torch.from_numpy(g0))
            tail = [ctl] if ctl is not None else []
            ops.call(entry, gp.t, gb.t, gg.t, idx_dev, n_s, d, lr, mom, wd, *(tail + [ops.current_stream_ptr()]))()
            torch.cuda.synchronize()
            for g_, what in ((gp, "p"), (gb, "buf"), (gg, "g_rows")):
                g_.assert_guards(what)
            assert same(gg.t, g0) and np.array_equal(idx_dev.cpu().numpy(), idx), "an input was written"
            return gp.t.cpu().numpy(), gb.t.cpu().numpy()

        plain = run("fr_sgd_rows")
        assert not same(plain[0], p0)
        for coef in (1.0, COEF):
            got = run("fr_sgd_rows_ctl", _ctl(7.0, coef, 1.0))
            assert same(got[0], plain[0]) and same(got[1], plain[1]), (n, n_s, d, coef, "!= fr_sgd_rows")
        got = run("fr_sgd_rows_ctl", _ctl(np.nan, np.nan, 0.0))
        assert same(got[0], p0) and same(got[1], b0), (n, n_s, d, "a skipped step moved a row")


# ------------------------------------------------------------------------------------------------ GradGuard with SGD

MOD_SIZES = (5, 300, 4097, 9000, 64)  # the last one is the "head": in the optimizer, outside the guard
LR, MOM, WDM = 0.05, 0.9, 1e-2


def _module_params(seed):
    rng = np.random.default_rng(seed)
    return [torch.nn.Parameter(dev(rng.standard_normal(n).astype(np.float32))) for n in MOD_SIZES]


def _module_grads(step, poison=False):
    rng = np.random.default_rng(100 + step)
    grads = [rng.standard_normal(n).astype(np.float32) for n in MOD_SIZES]
    if poison:
        grads[2][4096] = np.nan
    return grads


def _make_sgd(params):
    from frhip.optim import SGD
    # group 0 holds body tensors and the head (it splits under a guard), group 1 the "batch-norm" tensors
    return SGD([{"params": [params[0], params[2], params[4]], "weight_decay": WDM}, {"params": [params[1], params[3]]}],
               lr=LR, momentum=MOM)


def _set_grads(params, grads):
    for p, g in zip(params, grads):
        if p.grad is None:
            p.grad = dev(g)
        else:
            p.grad.copy_(torch.from_numpy(g))


def _state(params, opt):
    return [p.detach().clone() for p in params], [opt.state[p]["momentum_buffer"].clone() for p in params]


def test_grad_guard_with_sgd_three_steps_and_a_poisoned_one():
    """Three steps under GradGuard(max_norm) equal, bit for bit, the unguarded optimizer fed with the gradients the
    restatement scales (fp32 g * c, c from ctl_ref; the head unscaled) -- fr_sgd_step_ctl is "scale, then fr_sgd_step".
    Second run: the gradient of step 2 holds a NaN; weights and momentum keep their step-1 bits, step 3 proceeds, the
    counters read 1 of 3.  .grad is never written."""
    from frhip.optim import GradGuard
    max_norm = 20.0
    for poison in (False, True):
        params, ref_params = _module_params(51), _module_params(51)
        opt, ref_opt = _make_sgd(params), _make_sgd(ref_params)
        guard = GradGuard(params[:4], max_norm=max_norm, skip_nonfinite=True)
        for step in range(3):
            grads = _module_grads(step, poison and step == 1)
            _set_grads(params, grads)
            before = _state(params, opt) if step else None
            ctl = guard.measure()
            opt.step(guard=guard)
            torch.cuda.synchronize()
            want = G.ctl_ref(G.parts_ref(grads[:4], G.pairs_of(MOD_SIZES[:4])), max_norm, True)
            got = ctl.cpu().numpy()
            assert same(got[2:], want[2:]) and (same(got, want) or np.isnan(want[0])), (step, got, want)
            for p, g in zip(params, grads):
                assert same(p.grad, g), "a gradient was written"
            if want[2] == 0.0:
                assert poison and step == 1
                after = _state(params, opt)
                for a, b in zip(before[0] + before[1], after[0] + after[1]):
                    assert same(a, b), "a skipped step moved a weight or a momentum buffer"
                continue
            assert 0 < want[1] < 1  # these gradients are clipped
            _set_grads(ref_params, [G.scaled(g, want, t < 4) for t, g in enumerate(grads)])
            ref_opt.step()
            torch.cuda.synchronize()
            for t, (a, b) in enumerate(zip(params, ref_params)):
                assert same(a, b), (poison, step, t, "weights")
                assert same(opt.state[a]["momentum_buffer"], ref_opt.state[b]["momentum_buffer"]), (poison, step, t, "momentum")
        assert guard.state_dict() == {"skipped": 1 if poison else 0, "steps": 3}
    guard.load_state_dict({"skipped": 4, "steps": 9})
    assert guard.skipped.tolist() == [4, 9] and guard.state_dict() == {"skipped": 4, "steps": 9}


@pytest.mark.parametrize("max_norm", [1e30, None])
def test_a_norm_below_max_norm_gives_the_unguarded_bits(max_norm):
    from frhip.optim import GradGuard
    params, ref_params = _module_params(52), _module_params(52)
    opt, ref_opt = _make_sgd(params), _make_sgd(ref_params)
    guard = GradGuard(params[:4], max_norm=max_norm, skip_nonfinite=max_norm is not None)
    for step in range(2):
        grads = _module_grads(step)
        _set_grads(params, grads)
        _set_grads(ref_params, grads)
        guard.measure()
        opt.step(guard=guard)
        ref_opt.step()
    torch.cuda.synchronize()
    assert guard.ctl[1].item() == 1.0 and guard.ctl[2].item() == 1.0
    for a, b in zip(params, ref_params):
        assert same(a, b) and same(opt.state[a]["momentum_buffer"], ref_opt.state[b]["momentum_buffer"])


def test_step_with_a_guard_that_did_not_measure_raises():
    from frhip.optim import Adam, GradGuard
    params = _module_params(53)
    _set_grads(params, _module_grads(0))
    opt = _make_sgd(params)
    guard = GradGuard(params[:4], max_norm=1.0)
    before = [p.detach().clone() for p in params]
    with pytest.raises(_lib.FrhipError, match="measure"):
        opt.step(guard=guard)
    guard.measure()
    opt.step(guard=guard)
    with pytest.raises(_lib.FrhipError, match="measure"):  # one step per measure()
        opt.step(guard=guard)
    with pytest.raises(_lib.FrhipError, match="measure"):
        Adam(params, lr=1e-3).step(guard=guard)
    torch.cuda.synchronize()
    assert not same(params[0], before[0])


def test_adam_with_a_guard_skips_and_clips():
    """Adam under the guard: a poisoned step keeps p, exp_avg and exp_avg_sq (the host step counter advances all the same),
    a clean one is the restatement on the scaled gradient."""
    from frhip.optim import Adam, GradGuard
    params = _module_params(54)
    opt = Adam([{"params": params}], lr=1e-3)
    guard = GradGuard(params[:4], max_norm=20.0)
    host = [p.detach().cpu().numpy() for p in params]
    m = [np.zeros(n, np.float32) for n in MOD_SIZES]
    v = [np.zeros(n, np.float32) for n in MOD_SIZES]
    for step in range(3):
        grads = _module_grads(step, step == 1)
        _set_grads(params, grads)
        guard.measure()
        opt.step(guard=guard)
        torch.cuda.synchronize()
        want = G.ctl_ref(G.parts_ref(grads[:4], G.pairs_of(MOD_SIZES[:4])), 20.0, True)
        sc = R.adam_scalars(1e-3, (0.9, 0.999), 1e-8, step + 1)
        for t, p in enumerate(params):
            host[t], m[t], v[t] = G.adam_step_ctl_ref(host[t], grads[t], m[t], v[t], sc, want, t < 4)
            assert same(p, host[t]) and same(opt.state[p]["exp_avg"], m[t]) and same(opt.state[p]["exp_avg_sq"], v[t]), (step, t)
            assert float(opt.state[p]["step"]) == step + 1
    assert guard.state_dict() == {"skipped": 1, "steps": 3}


def test_profile_shows_two_more_launches_and_no_host_copy():
    """measure() + step(guard=...) against the unguarded step under the profiler: no scalar read, no device-to-host copy;
    two launches more (fr_grad_sumsq, fr_grad_guard) plus one for group 0, which splits into body and head."""
    from frhip.optim import GradGuard
    counts = {}
    for tag in ("plain", "guarded"):
        params = _module_params(55)
        _set_grads(params, _module_grads(0))
        opt = _make_sgd(params)
        guard = GradGuard(params[:4], max_norm=20.0) if tag == "guarded" else None

        def step():
            if guard is None:
                opt.step()
            else:
                guard.measure()
                opt.step(guard=guard)

        step()  # first call: the tables, the momentum buffers
        torch.cuda.synchronize()
        names = HS.profiled_names(step)
        bad = [n for n in names if n in HS.HOST_READS or "DtoH" in n or "HtoD" in n]
        assert not bad, (tag, sorted(set(bad)))
        counts[tag] = {k: sum(k in n for n in names) for k in ("sgd_kernel", "sgd_ctl_kernel", "grad_sumsq_kernel",
                                                               "grad_guard_kernel")}
    cell = torch.ones(1, device="cuda")
    control = HS.profiled_names(lambda: (cell.item(), cell.cpu()))
    assert any(n in HS.HOST_READS for n in control) and any("DtoH" in n for n in control), sorted(set(control))
    per_launch = counts["plain"]["sgd_kernel"] // 2  # events the profiler lists per kernel launch: two groups, two launches
    assert per_launch >= 1 and counts["plain"] == dict(sgd_kernel=2 * per_launch, sgd_ctl_kernel=0, grad_sumsq_kernel=0,
                                                       grad_guard_kernel=0), counts
    assert counts["guarded"] == dict(sgd_kernel=0, sgd_ctl_kernel=3 * per_launch, grad_sumsq_kernel=per_launch,
                                     grad_guard_kernel=per_launch), counts


# ------------------------------------------------------------------------------------------------ one IR-50 step

B50, N50 = 8, 100


def _ir50_step(max_norm, guarded):
    """One training step of IR-50 + ArcFace + focal loss at batch 8 from seeded weights, as __graft_entry__.smoke builds it:
    (named backbone parameters, head weight, initial values, the guard or None)."""
    from backbone.model_irse import IR_50
    from frhip.optim import SGD, GradGuard
    from head.metrics import ArcFace
    from loss.focal import FocalLoss
    from util.utils import separate_irse_bn_paras
    model = IR_50([112, 112])
    synth.fill_state_dict(model.state_dict(), 15)
    model.output_layer[1].p = 0.0
    x = synth.uniform(3, "gg.x", (B50, 3, 112, 112))
    label = synth.labels(3, "gg.y", B50, N50)
    model = model.cuda().train()
    head = ArcFace(512, N50, None).cuda()
    with torch.no_grad():
        head.weight.copy_(synth.uniform(3, "gg.w", (N50, 512), -0.1, 0.1))
    init = {k: p.detach().clone() for k, p in model.named_parameters()}
    bn, wo = separate_irse_bn_paras(model)
    opt = SGD([{"params": wo + list(head.parameters()), "weight_decay": 2e-3}, {"params": bn}], lr=0.03, momentum=0.9)
    guard = GradGuard(model.parameters(), max_norm=max_norm) if guarded else None
    loss, _ = FocalLoss()(head(model(x.cuda()), label.cuda()), label.cuda())
    opt.zero_grad()
    loss.backward()
    if guard is None:
        opt.step()
    else:
        guard.measure()
        opt.step(guard=guard)
    torch.cuda.synchronize()
    return model, head, init, guard


def test_one_ir50_step_under_the_guard():
    """max_norm 1e30: every parameter has the bits of the unguarded step.  max_norm = half the measured norm: the control
    word has the bits of the restatement over all backbone gradients (more than 10 000 chunks), sampled backbone tensors
    have moved as the unguarded optimizer moves them on the fp32-scaled gradient, and the head has moved exactly as
    unguarded."""
    from frhip.optim import SGD
    plain_model, plain_head, _, _ = _ir50_step(None, False)
    model, head, _, guard = _ir50_step(1e30, True)
    norm = float(guard.ctl[0])
    assert guard.ctl.tolist()[1:] == [1.0, 1.0, 0.0] and np.isfinite(norm) and norm > 0
    for (k, a), (_, b) in zip(plain_model.named_parameters(), model.named_parameters()):
        assert same(a, b), (k, "max_norm 1e30 != unguarded")
    assert same(plain_head.weight, head.weight)
    half = norm / 2
    model, head, init, guard = _ir50_step(half, True)
    named = list(model.named_parameters())
    # the kernel reads a gradient in storage order (the conv weights are channels-last): take the elements that way
    grads = [p.grad.detach().as_strided((p.numel(),), (1,)).cpu().numpy() for _, p in named]
    want = G.ctl_ref(G.parts_ref(grads, G.pairs_of([g.size for g in grads])), half, True)
    got = guard.ctl.cpu().numpy()
    assert same(got, want), (got, want)
    assert abs(float(got[0]) - norm) <= np.spacing(np.float32(norm)) and 0.49 < got[1] < 0.51
    assert same(plain_head.weight, head.weight), "the head is not clipped"
    from util.utils import separate_irse_bn_paras
    decay = {id(p) for p in separate_irse_bn_paras(model)[1]}  # group 0 of the step: weight decay 2e-3
    moved = 0
    for i in sorted(set([0, 1, 2, len(named) // 2, len(named) // 2 + 1, len(named) - 2, len(named) - 1])):
        k, p = named[i]
        q = torch.nn.Parameter(init[k].clone())
        q.grad = p.grad * guard.ctl[1]  # fp32, one rounding: the gradient scaled in place
        SGD([q], lr=0.03, momentum=0.9, weight_decay=2e-3 if id(p) in decay else 0.0).step()
        torch.cuda.synchronize()
        assert same(p, q), (k, "!= the unguarded step on the scaled gradient")
        moved += int(not same(p, init[k]))
        assert not same(p, dict(plain_model.named_parameters())[k]) or not bool(p.grad.any()), (k, "not clipped")
    assert moved >= 5


# ------------------------------------------------------------------------------------------------ train.py


def test_train_py_with_both_keys_trains_logs_and_resumes_bit_for_bit(tmp_path):
    """12 steps straight == 6 steps, stop, resume for 6 with GRAD_CLIP_NORM and SKIP_NONFINITE_STEP set; the display line
    carries the norm and the counts; the State_* file carries the counters and the resumed run ends on the straight run's."""
    cfg = dict(HEAD_NAME="ArcFace", GRAD_CLIP_NORM=1.0, SKIP_NONFINITE_STEP=True)
    r = HS.resumed(tmp_path, cfg, "ArcFace")
    lines = re.findall(r"Training Loss [^\n]*\tGrad Norm ([0-9.eE+-]+|nan|inf)\tSkipped (\d+)/(\d+)", r.a_log)
    assert len(lines) == 12, r.a_log[-3000:]  # 6 steps an epoch: a display line every step
    assert all(np.isfinite(float(n)) and float(n) > 0 for n, _, _ in lines), lines
    assert [int(s) for _, s, _ in lines] == [0] * 12 and [int(t) for _, _, t in lines] == list(range(1, 13)), lines
    mid = torch.load(HS.ckpt(r.b1_dir, "State_ArcFace_Epoch_1_Batch_6_"), map_location="cpu")
    assert mid["grad_guard"] == {"skipped": 0, "steps": 6}
    for d in (r.a_dir, r.b2_dir):
        state = torch.load(HS.ckpt(d, "State_ArcFace_Epoch_2_Batch_12_"), map_location="cpu")
        assert state["grad_guard"] == {"skipped": 0, "steps": 12}, state["grad_guard"]


def test_train_py_without_the_keys_writes_no_guard_state(tmp_path):
    model_dir, log = HS.run_train(tmp_path, "plain", dict(HEAD_NAME="ArcFace"), max_steps=1, epochs=1, limit=300)
    state = torch.load(HS.ckpt(model_dir, "State_ArcFace_Epoch_1_Batch_1_"), map_location="cpu")
    assert "grad_guard" not in state and "Grad Norm" not in log and "Skipped" not in log, (list(state), log[-1000:])


def test_train_py_refuses_a_bad_clip_norm(tmp_path):
    out = HS.run_train(tmp_path, "refused", dict(HEAD_NAME="ArcFace", GRAD_CLIP_NORM=0), max_steps=1, ok=False, limit=120)
    assert out.returncode != 0 and "GRAD_CLIP_NORM must be None or a number greater than 0" in out.stderr, out.stderr[-1500:]
