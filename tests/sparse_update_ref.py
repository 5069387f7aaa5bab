"""np.float32 statement of the row-sparse SGD update of the sampled class-sharded head (fr_sgd_rows; frhip/optim.py
``SGD._step_rows``): the lazy update of Partial-FC v1.

    for j < n_s, r = idx[j]:   d = g_rows[j] + wd p[r];   buf[r] = momentum buf[r] + d;   p[r] -= lr buf[r]

Rows that are not in ``idx`` keep their weight and momentum bits: no weight decay, no momentum step.

Roundings.  The kernel shares its per-element function with the dense fr_sgd_step: d and buf are ``fmaf`` by the source, and
the compiler contracts ``p - lr * buf`` into a third fused multiply-add, fma(-lr, buf, p) (the one ``v_fma_f32`` with a
negated operand in the kernel's listing).  Each of the three is therefore ONE fp32 rounding of an exact a * b + c, and
``fma32`` restates that: the product of two fp32 values is exact in float64 (48 bits), the float64 sum is made
round-to-odd with the error term of Knuth's TwoSum, and a round-to-odd float64 (53 >= 24 + 2 bits) rounds to fp32 as the
exact value does.  On dyadic operands nothing rounds at all and the float64 statement of tests/loss_optim_ref.py
(``sgd_step_ref``), rounded to fp32, gives the same bits; ``sgd_rows_ref64`` is that form.

Test infrastructure only.  ``dense_loop`` is the literal loop over all n rows; its ``wrong`` forms are wrong on purpose
(negative controls)."""
import numpy as np

from loss_optim_ref import sgd_step_ref


def fma32(a, b, c):
    """fp32(a * b + c) with one rounding, element-wise on np.float32 operands."""
    a, b, c = (np.asarray(v, dtype=np.float32).astype(np.float64) for v in (a, b, c))
    prod = a * b  # exact
    s = prod + c
    bb = s - prod
    err = (prod - (s - bb)) + (c - bb)  # TwoSum: prod + c = s + err exactly
    bits = np.asarray(s).view(np.int64)
    fix = (err != 0) & ((bits & 1) == 0) & np.isfinite(s)  # inexact and even: the odd neighbour lies towards err
    toward = np.where(err > 0, np.inf, -np.inf)
    s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def sgd_rows_ref(p, buf, g_rows, idx, wd, momentum, lr):
    """(p, buf) after the update, as new np.float32 arrays of the dense shape; p / buf [n, D] or [n], g_rows [n_s, D] or
    [n_s], idx [n_s] distinct."""
    p, buf = np.array(p, dtype=np.float32), np.array(buf, dtype=np.float32)
    g = np.asarray(g_rows, dtype=np.float32)
    sel = np.asarray(idx, dtype=np.int64)
    wd, momentum, lr = np.float32(wd), np.float32(momentum), np.float32(lr)
    d = fma32(wd, p[sel], g)
    b = fma32(momentum, buf[sel], d)
    pn = fma32(-lr, b, p[sel])
    buf[sel] = b
    p[sel] = pn
    return p, buf


def sgd_rows_ref64(p, buf, g_rows, idx, wd, momentum, lr):
    """The same through the float64 ``sgd_step_ref`` of tests/loss_optim_ref.py on the gathered rows, rounded to fp32 once
    at the end: the kernel's bits where no operation rounds (dyadic operands)."""
    p, buf = np.array(p, dtype=np.float32), np.array(buf, dtype=np.float32)
    sel = np.asarray(idx, dtype=np.int64)
    pn, b = sgd_step_ref(p[sel], np.asarray(g_rows, dtype=np.float32), buf[sel], np.float32(wd), np.float32(momentum),
                         np.float32(lr))
    p[sel], buf[sel] = pn.astype(np.float32), b.astype(np.float32)
    return p, buf


def dense_loop(p, buf, g_rows, idx, wd, momentum, lr, wrong=None):
    """The literal loop over all n rows.  ``wrong``: None, or a negative control --
    "decay_unselected"     an unselected row takes the step with a zero gradient and zero momentum factor (it decays)
    "momentum_unselected"  an unselected row takes the step with a zero gradient and no decay (its momentum moves it)
    "write_at_j"           row j is updated in place of row idx[j]"""
    p, buf = np.array(p, dtype=np.float32), np.array(buf, dtype=np.float32)
    g = np.asarray(g_rows, dtype=np.float32)
    n = p.shape[0]
    where = {int(r): j for j, r in enumerate(np.asarray(idx))}
    if wrong == "write_at_j":
        where = {j: j for j in range(len(where))}
    zero = np.zeros_like(p[0])
    wd, momentum, lr = np.float32(wd), np.float32(momentum), np.float32(lr)
    for r in range(n):
        if r in where:
            grad, w, m = g[where[r]], wd, momentum
        elif wrong == "decay_unselected":
            grad, w, m = zero, wd, np.float32(0)
        elif wrong == "momentum_unselected":
            grad, w, m = zero, np.float32(0), momentum
        else:
            continue
        d = fma32(w, p[r], grad)
        b = fma32(m, buf[r], d)
        p[r] = fma32(-lr, b, p[r])
        buf[r] = b
    return p, buf


def dyadic(rng, shape, scale=1.0 / 64):
    """Multiples of ``scale`` in [-32, 32] * scale: with power-of-two lr / momentum / wd every product and sum of the update
    is exact in fp32."""
    return (rng.randint(-32, 33, size=shape) * scale).astype(np.float32)
