"""numpy statement of the gradient guard (fr_grad_sumsq, fr_grad_guard and the three _ctl step entries of
frhip/csrc/head_loss_optim.hip; ``frhip.optim.GradGuard``).  Written for this repository; numpy only.

    parts = parts_ref(tensors, pairs)                   # float64 [len(pairs)], the order include/frhip.h documents
    total = total_ref(parts)                            # float64, the same tree over the parts
    ctl = ctl_ref(parts, max_norm, skip_nonfinite)      # float32 [4]: norm, coefficient, go flag, 0
    p, buf = sgd_step_ctl_ref(p, g, buf, wd, momentum, lr, ctl, use_coef)
    p, m, v = adam_step_ctl_ref(p, g, m, v, sc, ctl, use_coef)

The order of a sum is part of its bits.  A chunk of L <= 4096 elements: thread t of 256 adds the squares of elements t,
t + 256, ... in ascending order (an absent element is +0.0, which changes no bit of a sum of squares); the 64 values of a
wave fold in halves, v[l] += v[l + h] for h = 32 .. 1; the four waves' sums are added in wave order.  The total of the parts
runs the same way with thread t taking parts t, t + 256, ... ."""
import numpy as np

import loss_optim_ref as R

CHUNK = 4096
THREADS = 256


def _threads_then_tree(values):
    """float64 ``values`` in index order -> their sum in the kernels' order."""
    values = np.asarray(values, dtype=np.float64)
    rows = max(1, -(-values.size // THREADS))
    padded = np.zeros(rows * THREADS, dtype=np.float64)
    padded[:values.size] = values
    with np.errstate(invalid="ignore", over="ignore"):
        acc = np.zeros(THREADS, dtype=np.float64)
        for row in padded.reshape(rows, THREADS):  # thread t: element t of every row, rows ascending
            acc = acc + row
        waves = []
        for w in range(THREADS // 64):
            v = acc[64 * w:64 * w + 64].copy()
            h = 32
            while h:
                v = v[:h] + v[h:2 * h]
                h //= 2
            waves.append(v[0])
        return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def chunk_sumsq(x):
    """Sum of squares of one chunk (fp32 values, at most CHUNK of them) in double, in the kernel's order."""
    x = np.asarray(x, dtype=np.float32)
    assert x.ndim == 1 and x.size <= CHUNK
    with np.errstate(invalid="ignore", over="ignore"):
        x64 = x.astype(np.float64)
        return _threads_then_tree(x64 * x64)  # the square of an fp32 value is exact in double


def pairs_of(sizes):
    """The (tensor, chunk) pairs of tensors of these sizes, in table order."""
    return [(t, c) for t, n in enumerate(sizes) for c in range(-(-n // CHUNK))]


def parts_ref(tensors, pairs):
    return np.array([chunk_sumsq(np.asarray(tensors[t], dtype=np.float32).reshape(-1)[c * CHUNK:(c + 1) * CHUNK])
                     for t, c in pairs], dtype=np.float64)


def total_ref(parts):
    return _threads_then_tree(np.asarray(parts, dtype=np.float64))


def ctl_ref(parts, max_norm, skip_nonfinite):
    """float32 [4]: (float)sqrt(total); c = max_norm / (norm + 1e-6f) clamped at 1, every operation rounded to fp32 (1 when
    max_norm is None or <= 0); the go flag; 0."""
    f = np.float32
    total = total_ref(parts)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        norm = f(np.sqrt(np.float64(total)))
        coef = f(1.0)
        if max_norm is not None and max_norm > 0:
            c = f(max_norm) / f(norm + f(1e-6))
            coef = f(1.0) if c > f(1.0) else f(c)
    go = f(0.0) if (skip_nonfinite and not np.isfinite(total)) else f(1.0)
    return np.array([norm, coef, go, 0.0], dtype=np.float32)


def scaled(g, ctl, use_coef):
    """The gradient a _ctl step takes: g * ctl[1] rounded to fp32 on its own when use_coef, else g."""
    g = np.asarray(g, dtype=np.float32)
    if not use_coef:
        return g
    with np.errstate(invalid="ignore", over="ignore"):
        out = g * np.float32(ctl[1])
    assert out.dtype == np.float32
    return out


def sgd_step_ctl_ref(p, g, buf, wd, momentum, lr, ctl, use_coef):
    """fr_sgd_step_ctl: nothing moves when the go flag is 0; else loss_optim_ref.sgd_step_ref (float64) on the scaled
    fp32 gradient."""
    if float(ctl[2]) == 0.0:
        return np.asarray(p, dtype=np.float64), np.asarray(buf, dtype=np.float64)
    return R.sgd_step_ref(p, scaled(g, ctl, use_coef), buf, wd, momentum, lr)


def adam_step_ctl_ref(p, g, m, v, sc, ctl, use_coef):
    """fr_adam_step_ctl: p, m, v keep their bits when the go flag is 0; else loss_optim_ref.adam_step_ref (np.float32) on
    the scaled gradient."""
    if float(ctl[2]) == 0.0:
        return tuple(np.asarray(a, dtype=np.float32) for a in (p, m, v))
    return R.adam_step_ref(p, scaled(g, ctl, use_coef), m, v, sc)

