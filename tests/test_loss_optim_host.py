"""CPU checks of the restatements in tests/loss_optim_ref.py, which the GPU tests of tests/test_gpu_loss_optim.py hold the
loss, accuracy and optimiser kernels to: each against torch on the host (``F.cross_entropy`` and autograd through the line
of loss/focal.py, ``torch.topk``, ``torch.optim.SGD`` / ``Adam``), five deliberately wrong variants that must each miss a
stated check, and the argument checks of the seven entry points, which run before any launch.

Adam: torch's host kernels do NOT have the restatement's bits.  ATen's vectorised CPU ``lerp`` and ``addcmul`` contract
``m + w1 (g - m)`` and ``v beta2 + (w2 g) g`` into fused multiply-adds (measured here over three steps of 12289 elements: a
quarter of the elements of exp_avg and exp_avg_sq differ in the last bit from step 2 on, a few dozen of p; step 1, where
m = v = 0, agrees in both moments), while the kernel's ``_rn`` intrinsics round every operation on its own, which is what
the restatement states.  So the comparison with torch is within that gap, with bounds from the roundings involved
(``test_adam_restatement_against_torch_on_the_host``); the device is held to the restatement bit for bit."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_optim_ref as R

ENTRIES = ("fr_ce_rows", "fr_rank_rows", "fr_topk_precision", "fr_focal_finalize", "fr_focal_bwd", "fr_sgd_step",
           "fr_adam_step")
EPS32 = 2.0 ** -24  # half an ulp of 1 in fp32: the relative error of one rounding


def _gauss(seed, rows, N, std=3.0):
    rng = np.random.default_rng(seed)
    return (std * rng.standard_normal((rows, N))).astype(np.float32), rng.integers(0, N, size=rows)


# ------------------------------------------------------------------------------------------------ rows


@pytest.mark.parametrize("rows,N", [(5, 1), (7, 33), (16, 1001)])
def test_rows_against_f_cross_entropy(rows, N):
    z, y = _gauss(1, rows, N)
    lse, ce, rank = R.rows_ref(z, y)
    zt, yt = torch.from_numpy(z).double(), torch.from_numpy(y)
    np.testing.assert_allclose(lse, torch.logsumexp(zt, 1).numpy(), rtol=1e-14, atol=1e-14)
    np.testing.assert_allclose(ce, F.cross_entropy(zt, yt, reduction="none").numpy(), rtol=1e-12, atol=1e-13)
    # distinct logits: the rank is the label's place in the descending order
    order = torch.argsort(zt, 1, descending=True)
    place = (order == yt[:, None]).nonzero()[:, 1].numpy()
    assert np.array_equal(rank, place)


def test_rank_rules_for_ties_nan_and_missing_labels():
    """The cases of the rank rule one by one, and that ``>=`` in place of ``>`` (negative control) fails the tie cases."""
    nan = np.nan
    z = np.array([[2.0, 2.0, 2.0, 2.0],     # all equal: rank 0
                  [1.0, 5.0, 5.0, 5.0],     # the label (1) tied with two others at the top: rank 0
                  [9.0, 5.0, 5.0, 5.0],     # the same tie below one larger column: rank 1
                  [3.0, 1.0, 2.0, 0.0],     # label -1
                  [3.0, 1.0, 2.0, 0.0],     # label N
                  [nan, nan, nan, nan],     # all NaN
                  [7.0, nan, 1.0, 0.0],     # NaN off the label, the label (0) the largest finite value
                  [7.0, nan, 1.0, 0.0]],    # the label is the NaN column
                 dtype=np.float32)
    y = np.array([2, 1, 1, -1, 4, 0, 0, 1])
    lse, ce, rank = R.rows_ref(z, y)
    assert rank.tolist() == [0, 0, 1, 4, 4, 4, 1, 4]
    assert ce[3] == lse[3] and ce[4] == lse[4] and np.isnan(ce[5:]).all()
    # torch.topk agrees about NaN: it comes first, so the finite label of row 6 is not the top-1 prediction
    zt = torch.from_numpy(z)
    assert int(torch.topk(zt[6], 1).indices) == 1 and int(torch.topk(zt[7], 1).indices) == 1
    # and the reference's accuracy (util/utils.py:343-358: topk, pred.eq(target)) counts rows 3..5 as misses at every k
    pred = torch.topk(zt, 4, 1).indices
    hit = pred.eq(torch.from_numpy(y)[:, None])
    assert not bool(hit[3].any()) and not bool(hit[4].any()) and rank[5] >= 4
    # negative control: counting >= puts the label behind its ties
    zl = z[np.arange(8), np.clip(y, 0, 3)]
    wrong = (z >= zl[:, None]).sum(1)
    assert wrong[0] != rank[0] and wrong[1] != rank[1] and wrong[2] != rank[2]


def test_confident_logits_span_the_stated_range():
    """The confident regime of the GPU test, every case of it, built on the host: the label leads, every logit is s * cos
    with |cos| < 1, and the float64 ce lies within about 1e-3 .. 1e-1 (not lower: there S = 1 + ce rounds to 1 in fp32).
    N = 1 has no other column: its ce is 0."""
    spans = []
    for rows, N, _ in R.CE_CASES:
        for regime in R.REGIMES[1:]:
            z, y = R.ce_case(rows, N, regime)
            _, ce, rank = R.rows_ref(z, y)
            assert (rank == 0).all() and np.abs(z).max() < float(regime[1:]), (rows, N, regime)
            if N == 1:
                assert (ce == 0).all()
                continue
            assert 0.9e-3 < ce.min() and ce.max() < 1.1e-1, (rows, N, regime, ce.min(), ce.max())
            spans.append(ce.max() / ce.min())
    assert max(spans) > 30 and np.median(spans) > 5, spans  # the cases together cover the range


# ------------------------------------------------------------------------------------------------ finalize, gradient


def _focal_torch(z, y, gamma):
    """loss/focal.py:17-21 of the reference, in float64: logp = CE(input, target); p = exp(-logp);
    ((1 - p) ** gamma * logp).mean()."""
    logp = F.cross_entropy(z, y)
    p = torch.exp(-logp)
    return ((1 - p) ** gamma * logp).mean()


@pytest.mark.parametrize("gamma", [None, 0.0, 0.5, 1.0, 2.0, 3.5])
def test_finalize_and_gradient_against_autograd(gamma):
    z, y = _gauss(2, 19, 333)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    yt = torch.from_numpy(y)
    loss = F.cross_entropy(zt, yt) if gamma is None else _focal_torch(zt, yt, gamma)
    (g,) = torch.autograd.grad(loss, [zt])
    _, ce, rank = R.rows_ref(z, y)
    s = R.finalize_ref(ce, rank, gamma)
    assert abs(s["loss"] / float(loss.detach()) - 1) < 1e-12
    assert abs(s["mean"] / float(F.cross_entropy(zt.detach(), yt)) - 1) < 1e-12
    got = R.grad_ref(z, y, s["slope"] / 19)
    np.testing.assert_allclose(got, g.numpy(), rtol=1e-9, atol=1e-15)
    if gamma is None:
        assert s["slope"] == 1.0 and s["loss"] == s["mean"]
    # precision@1 / @5 as the reference's accuracy() on distinct logits
    pred = torch.topk(zt.detach(), 5, 1).indices.eq(yt[:, None])
    assert s["prec1"] == np.float32(100.0 * int(pred[:, :1].sum()) / 19)
    assert s["prec5"] == np.float32(100.0 * int(pred.sum()) / 19)


@pytest.mark.parametrize("gamma", [0.5, 1.0, 2.0, 3.5])
def test_focal_slope_without_its_first_term_misses_autograd(gamma):
    """Negative control: the slope (1 - p)^gamma alone, without gamma (1 - p)^(gamma - 1) p l, misses the gradient
    check of ``test_finalize_and_gradient_against_autograd`` (rtol 1e-9) by orders of magnitude."""
    z, y = _gauss(2, 19, 333)
    zt = torch.from_numpy(z).double().requires_grad_(True)
    (g,) = torch.autograd.grad(_focal_torch(zt, torch.from_numpy(y), gamma), [zt])
    _, ce, rank = R.rows_ref(z, y)
    l = R.finalize_ref(ce, rank, gamma)["mean"]
    wrong = (1.0 - np.exp(-l)) ** gamma
    miss = np.abs(R.grad_ref(z, y, wrong / 19) - g.numpy()).max() / np.abs(g.numpy()).max()
    assert miss > 1e-4, miss


def test_gradient_of_a_row_without_a_label_is_k_softmax():
    z, _ = _gauss(4, 3, 9)
    g = R.grad_ref(z, np.array([-1, 9, 2]), 0.37)
    sm = torch.softmax(torch.from_numpy(z).double(), 1).numpy()
    np.testing.assert_allclose(g[:2], 0.37 * sm[:2], rtol=1e-12)
    assert abs(g[2].sum()) < 1e-15 and abs(g[0].sum() - 0.37) < 1e-15


@pytest.mark.parametrize("rows", [1, 255, 256, 257, 1000])
def test_topk_against_the_reference_line(rows):
    """``(rank < k).float().sum().mul_(100.0 / n)`` (util/utils.py:343-358 as util.utils.accuracy states it on ranks), bit
    for bit, a k of 0 and a k above every rank included."""
    rng = np.random.default_rng(rows)
    rank = rng.integers(0, 12, size=rows)
    ks = (0, 1, 3, 5, 10, 1000)
    got = R.topk_ref(rank, ks, 100.0 / rows)
    rt = torch.from_numpy(rank)
    want = [float((rt < k).float().sum().mul_(100.0 / rows)) for k in ks]
    assert got.dtype == np.float32 and [float(v) for v in got] == want
    assert got[0] == 0.0 and got[-1] == np.float32(rows) * np.float32(100.0 / rows)


# ------------------------------------------------------------------------------------------------ SGD


def _sgd_torch(p, g, buf, wd, momentum, lr):
    pt = torch.nn.Parameter(torch.from_numpy(p).double().clone())
    opt = torch.optim.SGD([pt], lr=lr, momentum=momentum, weight_decay=wd)
    opt.state[pt]["momentum_buffer"] = torch.from_numpy(buf).double().clone()
    pt.grad = torch.from_numpy(g).double().clone()
    opt.step()
    return pt.detach().numpy(), opt.state[pt]["momentum_buffer"].numpy()


def test_sgd_restatement_against_torch_and_two_wrong_variants():
    """One step of torch.optim.SGD in float64 on a tensor with a momentum buffer.  Negative controls, each far outside the
    1e-12 bar: the weight decay of the neighbouring tensor; momentum applied after the learning rate (buf = momentum buf +
    lr d, p -= buf: the other convention, equal only while lr never changes and the buffer was built with it)."""
    rng = np.random.default_rng(5)
    p, g, buf = (rng.standard_normal(4097) for _ in range(3))
    wd, other_wd, momentum, lr = 2e-3, 5e-4, 0.9, 0.03
    tp, tb = _sgd_torch(p, g, buf, wd, momentum, lr)
    rp, rb = R.sgd_step_ref(p, g, buf, wd, momentum, lr)
    bar = 1e-12
    np.testing.assert_allclose(rp, tp, rtol=bar, atol=bar)
    np.testing.assert_allclose(rb, tb, rtol=bar, atol=bar)
    wp, _ = R.sgd_step_ref(p, g, buf, other_wd, momentum, lr)
    assert np.abs(wp - tp).max() > 1e-6
    late = momentum * buf + lr * (g + wd * p)
    assert np.abs((p - late) - tp).max() > 1e-3


# ------------------------------------------------------------------------------------------------ Adam


def _adam_runs(steps=3, n=12289, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, eps_inside=False):
    """(torch host single-tensor Adam, the restatement) over ``steps`` steps with gradients scaled 1e-3, 1, 1e3: per step
    (p, m, v) of each and the operands the bounds need."""
    gen = np.random.default_rng(9)
    p0 = gen.standard_normal(n).astype(np.float32)
    pt = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([pt], lr=lr, betas=betas, eps=eps, foreach=False)
    rp, rm, rv = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    out = []
    for step, scale in enumerate((1e-3, 1.0, 1e3)[:steps], 1):
        g = (scale * gen.standard_normal(n)).astype(np.float32)
        pt.grad = torch.from_numpy(g.copy())
        opt.step()
        sc = R.adam_scalars(lr, betas, eps, step)
        m_prev = rm
        if eps_inside:  # the wrong variant: sqrt(v / bc2 + eps) in place of sqrt(v) / bc2_sqrt + eps
            m = rm + sc["w1"] * (g - rm)
            v = rv * sc["beta2"] + (sc["w2"] * g) * g
            rp = rp + ((-sc["step_size"]) * m) / np.sqrt(v / (sc["bc2_sqrt"] * sc["bc2_sqrt"]) + sc["eps"])
            rm, rv = m, v
        else:
            rp, rm, rv = R.adam_step_ref(rp, g, rm, rv, sc)
        st = opt.state[pt]
        out.append(dict(tp=pt.detach().numpy().copy(), tm=st["exp_avg"].numpy().copy(), tv=st["exp_avg_sq"].numpy().copy(),
                        rp=rp, rm=rm, rv=rv, g=g, m_prev=m_prev, sc=sc))
    return out


def _adam_gaps(runs, lr=1e-3):
    """Per step, the largest of |difference| / bound over the elements, for m, v and p (<= 1: within the bound).

    m: both sides round m + w1 (g - m) from operands that differ by the previous step's gap; one evaluation with and one
    without the intermediate roundings differ by at most 3 roundings of terms no larger than max(|m|, |g|), and the
    earlier gap comes in scaled by 0.9: bound 8 eps max(|m_prev|, |g|).  v: three roundings of positive terms, the earlier
    gap scaled by 0.999: 8 eps v.  p: one rounding of p on either side, plus the step, lr-sized (|m| / denom is at most
    about sqrt(step) / (1 - beta1^step) < 7 here), with the relative gaps of m and v and its own four roundings, less than
    64 eps together: 2 eps |p| + 7 * 64 eps lr."""
    worst = []
    for r in runs:
        bm = 8 * EPS32 * np.maximum(np.abs(r["m_prev"]), np.abs(r["g"]))
        bv = 8 * EPS32 * r["rv"]
        bp = 2 * EPS32 * np.abs(r["rp"]) + 7 * 64 * EPS32 * lr
        worst.append((float((np.abs(r["tm"].astype(np.float64) - r["rm"]) / bm).max()),
                      float((np.abs(r["tv"].astype(np.float64) - r["rv"]) / bv).max()),
                      float((np.abs(r["tp"].astype(np.float64) - r["rp"]) / bp).max())))
    return worst


def test_adam_restatement_against_torch_on_the_host():
    """Three steps of torch.optim.Adam (host, single-tensor path).  Not bit for bit (module docstring): the moments of step
    1 are, everything else is within the bounds of ``_adam_gaps``, and the count of differing elements is printed."""
    runs = _adam_runs()
    for i, r in enumerate(runs):
        print("adam host step %d: elements that differ from torch in m / v / p: %d / %d / %d of %d" % (
            i + 1, int((r["tm"] != r["rm"]).sum()), int((r["tv"] != r["rv"]).sum()), int((r["tp"] != r["rp"]).sum()),
            r["rp"].size))
    assert np.array_equal(runs[0]["tm"], runs[0]["rm"]) and np.array_equal(runs[0]["tv"], runs[0]["rv"])
    gaps = _adam_gaps(runs)
    print("adam host |difference| / bound per step (m, v, p):", gaps)
    assert all(max(g) <= 1.0 for g in gaps), gaps


def test_adam_with_eps_inside_the_square_root_misses_torch():
    """Negative control: sqrt(v_hat + eps) misses the p bound of ``_adam_gaps`` at the step whose gradients are 1e-3 (there
    sqrt(v_hat) is about 1e-3 and sqrt(v_hat + 1e-8) is 0.5 percent above it)."""
    gaps = _adam_gaps(_adam_runs(eps_inside=True))
    assert gaps[0][2] > 10.0, gaps


def test_adam_scalars_are_what_the_optimizer_passes():
    """frhip.optim.Adam.step: step_size = lr / (1 - b1^step), bc2_sqrt = (1 - b2^step)^0.5 in host doubles, and
    float(1 - b1), float(b2), float(1 - b2), float(eps); ctypes rounds each to a C float as np.float32 does."""
    import inspect
    from frhip.optim import Adam
    src = inspect.getsource(Adam.step)
    for text in ('step_size = group["lr"] / (1.0 - b1 ** step)', "bc2_sqrt = (1.0 - b2 ** step) ** 0.5",
                 'float(step_size), float(1.0 - b1),', 'float(b2), float(1.0 - b2), float(group["eps"]), float(bc2_sqrt)'):
        assert text in src, text
    sc = R.adam_scalars(1e-3, (0.9, 0.999), 1e-8, 3)
    for key, want in (("step_size", 1e-3 / (1.0 - 0.9 ** 3)), ("w1", 1.0 - 0.9), ("beta2", 0.999), ("w2", 1.0 - 0.999),
                      ("eps", 1e-8), ("bc2_sqrt", (1.0 - 0.999 ** 3) ** 0.5)):
        assert sc[key].dtype == np.float32 and float(sc[key]) == ctypes.c_float(want).value, key


# ------------------------------------------------------------------------------------------------ the C ABI


def test_entries_are_declared_and_the_abi_version_stays():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert name in _lib.protos and hasattr(lib, name), name
    assert _lib.lib.fr_abi_version() == 7  # no struct changed
    assert _lib.protos["fr_ce_rows"][2] == ["logits", "label", "lse", "ce", "rank", "rows", "N", "ld", "stream"]
    assert _lib.protos["fr_focal_bwd"][2] == ["logits", "label", "lse", "scalars", "gup", "grad", "rows", "N", "ld", "stream"]


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    """rows <= 0, N <= 0, ld < N and missing pointers are refused before any launch: -1, the entry's name first in the
    message.  fr_sgd_step / fr_adam_step keep nchunks <= 0 as a silent no-op (whatever the pointers) and refuse a missing
    table or chunk list once there is something to launch."""
    from frhip import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)  # a pointer that is not NULL; no call below gets as far as a launch

    def refused(name, rc):
        assert rc == -1, (name, rc)
        assert lib.fr_last_error_string().startswith(name.encode() + b":"), lib.fr_last_error_string()

    def ce_rows(rows, n, ld, z=one, y=one, lse=one, ce=one, rank=one):
        return lib.fr_ce_rows(z, y, lse, ce, rank, rows, n, ld, None)

    for rc in (ce_rows(0, 33, 36), ce_rows(-1, 33, 36), ce_rows(7, 0, 36), ce_rows(7, -5, 36), ce_rows(7, 33, 32),
               ce_rows(7, 33, 36, z=None), ce_rows(7, 33, 36, y=None), ce_rows(7, 33, 36, lse=None),
               ce_rows(7, 33, 36, ce=None), ce_rows(7, 33, 36, rank=None)):
        refused("fr_ce_rows", rc)

    def rank_rows(rows, n, ld, z=one, y=one, rank=one):
        return lib.fr_rank_rows(z, y, rank, rows, n, ld, None)

    for rc in (rank_rows(0, 33, 36), rank_rows(-1, 33, 36), rank_rows(7, 0, 36), rank_rows(7, 33, 32),
               rank_rows(7, 33, 36, z=None), rank_rows(7, 33, 36, y=None), rank_rows(7, 33, 36, rank=None)):
        refused("fr_rank_rows", rc)

    def finalize(rows, ce=one, rank=one, sc=one):
        return lib.fr_focal_finalize(ce, rank, rows, 2.0, sc, None)

    for rc in (finalize(0), finalize(-1), finalize(8, ce=None), finalize(8, rank=None), finalize(8, sc=None)):
        refused("fr_focal_finalize", rc)

    def bwd(rows, n, ld, z=one, y=one, lse=one, sc=one, gup=one, grad=one):
        return lib.fr_focal_bwd(z, y, lse, sc, gup, grad, rows, n, ld, None)

    for rc in (bwd(0, 33, 36), bwd(-1, 33, 36), bwd(7, 0, 36), bwd(7, 33, 32), bwd(7, 33, 36, z=None),
               bwd(7, 33, 36, y=None), bwd(7, 33, 36, lse=None), bwd(7, 33, 36, sc=None), bwd(7, 33, 36, gup=None),
               bwd(7, 33, 36, grad=None)):
        refused("fr_focal_bwd", rc)

    # fr_topk_precision keeps the check it had
    refused("fr_topk_precision", lib.fr_topk_precision(one, 8, 0, 1, 5, 0, 0, 12.5, one, None))
    refused("fr_topk_precision", lib.fr_topk_precision(one, 8, 5, 1, 5, 0, 0, 12.5, one, None))
    refused("fr_topk_precision", lib.fr_topk_precision(one, -1, 2, 1, 5, 0, 0, 12.5, one, None))

    sgd_table = ctypes.cast(one, ctypes.POINTER(_lib.FrSgdTensor))
    adam_table = ctypes.cast(one, ctypes.POINTER(_lib.FrAdamTensor))
    assert lib.fr_sgd_step(None, None, 0, 0.03, 0.9, None) == 0 and lib.fr_sgd_step(sgd_table, one, -3, 0.03, 0.9, None) == 0
    refused("fr_sgd_step", lib.fr_sgd_step(None, one, 4, 0.03, 0.9, None))
    refused("fr_sgd_step", lib.fr_sgd_step(sgd_table, None, 4, 0.03, 0.9, None))
    adam = (1e-3, 0.1, 0.999, 0.001, 1e-8, 0.03)
    assert lib.fr_adam_step(None, None, 0, *adam, None) == 0 and lib.fr_adam_step(adam_table, one, -3, *adam, None) == 0
    refused("fr_adam_step", lib.fr_adam_step(None, one, 4, *adam, None))
    refused("fr_adam_step", lib.fr_adam_step(adam_table, None, 4, *adam, None))

