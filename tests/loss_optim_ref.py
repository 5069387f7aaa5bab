"""numpy statement of what the loss, accuracy and optimiser entry points of frhip/csrc/head_loss_optim.hip compute
(fr_ce_rows, fr_rank_rows, fr_topk_precision, fr_focal_finalize / fr_ce_finalize, fr_focal_bwd, fr_sgd_step, fr_adam_step).
Written for this repository; numpy only.  Everything is float64 except where an entry point's contract is a sequence of
fp32 roundings (precision@k, the Adam step): those are restated in np.float32, operation by operation.

    lse, ce, rank = rows_ref(z, label)                  # float64, float64, int64 [rows]
    s = finalize_ref(ce, rank, gamma)                   # dict: loss, slope, prec1, prec5, mean (gamma None: plain CE)
    g = grad_ref(z, label, k)                           # float64 k (softmax - onehot); k = gup * slope / rows
    out = topk_ref(rank, ks, scale)                     # float32 [len(ks)]: float32(count) * float32(scale)
    p, buf = sgd_step_ref(p, g, buf, wd, momentum, lr)  # float64
    sc = adam_scalars(lr, betas, eps, step)             # the six fp32 scalars frhip.optim.Adam passes
    p, m, v = adam_step_ref(p, g, m, v, sc)             # float32, the kernel's operation order

The rank rule: rank[m] = #{n < N: not (z[m][n] <= zl)}, zl = z[m][label[m]], or NaN when the label
lies outside [0, N).  On finite data that is the count of columns strictly above the label, so a tie does not count
against it; a NaN column counts as above the label (torch.topk's order), and a NaN or missing label logit gives rank N:
such a row is never a hit, as the reference's pred.eq(target) finds no match for it.  The ce of a row without a label is
its lse."""
import numpy as np


def rows_ref(z, label):
    z = np.asarray(z, dtype=np.float64)
    label = np.asarray(label, dtype=np.int64)
    rows, N = z.shape
    has = (label >= 0) & (label < N)
    zl = np.where(has, z[np.arange(rows), np.where(has, label, 0)], np.nan)
    with np.errstate(invalid="ignore", over="ignore"):
        mx = z.max(1)
        lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
        ce = np.where(has, lse - zl, lse)
        rank = (~(z <= zl[:, None])).sum(1)
    return lse, ce, rank.astype(np.int64)


def focal_head(l, gamma):
    """(loss, slope) of loss/focal.py:17-21 at the mean cross entropy l: (1 - p)^gamma l and its derivative
    gamma (1 - p)^(gamma - 1) p l + (1 - p)^gamma, p = exp(-l); gamma None is nn.CrossEntropyLoss(): (l, 1)."""
    l = float(l)
    if gamma is None:
        return l, 1.0
    p = np.exp(-l)
    omp = 1.0 - p
    return omp ** gamma * l, gamma * omp ** (gamma - 1.0) * p * l + omp ** gamma


def precision_percent(count, rows):
    """100.0f * float(count) / rows as the finalize kernels round it: one fp32 product, one fp32 quotient."""
    return np.float32(np.float32(100.0) * np.float32(count)) / np.float32(rows)


def finalize_ref(ce, rank, gamma):
    ce = np.asarray(ce, dtype=np.float64)
    rank = np.asarray(rank)
    rows = ce.shape[0]
    mean = ce.sum() / rows
    loss, slope = focal_head(mean, gamma)
    return dict(loss=loss, slope=slope, mean=mean, prec1=precision_percent(int((rank < 1).sum()), rows),
                prec5=precision_percent(int((rank < 5).sum()), rows))


def grad_ref(z, label, k):
    z = np.asarray(z, dtype=np.float64)
    label = np.asarray(label, dtype=np.int64)
    rows, N = z.shape
    mx = z.max(1, keepdims=True)
    e = np.exp(z - mx)
    g = e / e.sum(1, keepdims=True)
    has = (label >= 0) & (label < N)
    g[np.arange(rows)[has], label[has]] -= 1.0
    return float(k) * g


def topk_ref(rank, ks, scale):
    rank = np.asarray(rank)
    return np.array([np.float32(int((rank < k).sum())) * np.float32(scale) for k in ks], dtype=np.float32)


def sgd_step_ref(p, g, buf, wd, momentum, lr):
    """torch.optim.SGD's update with coupled weight decay, dampening 0: d = g + wd p; buf = momentum buf + d; p -= lr buf."""
    p, g, buf = (np.asarray(a, dtype=np.float64) for a in (p, g, buf))
    d = g + float(wd) * p
    b = float(momentum) * buf + d
    return p - float(lr) * b, b


def adam_scalars(lr, betas, eps, step):
    """(step_size, w1, beta2, w2, eps, bc2_sqrt): host doubles as torch/optim/adam.py derives them, each rounded to fp32
    once where it crosses the C ABI."""
    b1, b2 = betas
    f = np.float32
    return dict(step_size=f(lr / (1.0 - b1 ** step)), w1=f(1.0 - b1), beta2=f(b2), w2=f(1.0 - b2), eps=f(eps),
                bc2_sqrt=f((1.0 - b2 ** step) ** 0.5))


def adam_step_ref(p, g, m, v, sc):
    """One update in np.float32, every operation rounded on its own: lerp (m + w1 (g - m)); mul + addcmul
    (v beta2 + (w2 g) g); sqrt(v) / bc2_sqrt + eps; addcdiv (p + (-step_size m) / denom)."""
    p, g, m, v = (np.asarray(a, dtype=np.float32) for a in (p, g, m, v))
    assert all(np.asarray(x).dtype == np.float32 for x in sc.values())
    m = m + sc["w1"] * (g - m)
    v = v * sc["beta2"] + (sc["w2"] * g) * g
    denom = np.sqrt(v) / sc["bc2_sqrt"] + sc["eps"]
    p = p + ((-sc["step_size"]) * m) / denom
    assert p.dtype == m.dtype == v.dtype == np.float32
    return p, m, v


# ------------------------------------------------------------------------------------------------ test data


def pitched(z, ld, fill):
    """[rows, ld] float32 with z in the first columns and ``fill`` in the padding."""
    z = np.asarray(z, dtype=np.float32)
    out = np.full((z.shape[0], ld), fill, dtype=np.float32)
    out[:, :z.shape[1]] = z
    return out


CE_CASES = [(5, 1, 4), (7, 33, 36), (3, 255, 256), (3, 256, 256), (3, 257, 260), (16, 1001, 1004), (4, 28000, 28000)]
REGIMES = ("gauss3", "s30", "s64")
PAD = 1e30  # in the padding columns [N, ld): large and finite, so a kernel that read one would show it in every output


def ce_case(rows, N, regime):
    """(z float32 [rows, N], label int64 [rows]) of one case: Gaussian logits of std 3 with uniform labels, or confident
    logits at s = 30 / 64 (``confident_logits``)."""
    rng = np.random.default_rng([rows, N, REGIMES.index(regime)])
    if regime == "gauss3":
        return (3.0 * rng.standard_normal((rows, N))).astype(np.float32), rng.integers(0, N, size=rows)
    return confident_logits(rng, rows, N, float(regime[1:]))


def special_rows(N):
    """(z float32 [r, N], label, name per row): the rows of the rank rule that N has room for."""
    rng = np.random.default_rng(N)
    base = (3.0 * rng.standard_normal(N)).astype(np.float32)
    rows, label, names = [], [], []

    def add(name, row, lab):
        rows.append(np.asarray(row, dtype=np.float32))
        label.append(lab)
        names.append(name)

    add("all equal", np.full(N, 1.5), N // 2)
    add("label 0", base, 0)
    add("label N-1", base, N - 1)
    add("label -1", base, -1)
    add("label N", base, N)
    add("all NaN", np.full(N, np.nan), N // 2)
    if N >= 2:
        r = base.copy()
        r[N - 1] = np.nan
        add("NaN off the label", r, 0)
        r = base.copy()
        r[0] = np.nan
        add("NaN label logit", r, 0)
    if N >= 3:
        r = base.copy()
        r[[0, N // 2, N - 1]] = np.sort(base)[N // 2]  # three columns share the median: columns above them remain
        add("label tied with two others", r, N // 2)
        r = base.copy()
        r[[0, N // 2, N - 1]] = base.max() + 1.0
        add("label tied with two others at the top", r, N - 1)
    return np.stack(rows), np.array(label, dtype=np.int64), names


def confident_logits(rng, rows, N, s, ce_lo=1e-3, ce_hi=1e-1):
    """fp32 logits s * cos with the label leading, and their labels: the other columns' cosines are uniform in
    [-0.25, 0.25], and the label's cosine is set so that the row's float64 cross entropy is log-uniform in about
    [ce_lo, ce_hi]: ce = log1p(R exp(-zl)), R = sum of exp over the other columns, so zl = log R - log expm1(ce)."""
    label = rng.integers(0, N, size=rows)
    z = (s * rng.uniform(-0.25, 0.25, size=(rows, N))).astype(np.float32)
    want = np.exp(rng.uniform(np.log(ce_lo), np.log(ce_hi), size=rows))
    if N == 1:
        return z, label
    zz = z.astype(np.float64)
    zz[np.arange(rows), label] = -np.inf
    mx = zz.max(1)
    logR = mx + np.log(np.exp(zz - mx[:, None]).sum(1))
    z[np.arange(rows), label] = (logR - np.log(np.expm1(want))).astype(np.float32)
    return z, label
