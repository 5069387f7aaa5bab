"""autograd.Function wrappers over the HIP kernels for the margin head, the focal loss and top-k accuracy.

These are what ``head/metrics.py``, ``loss/focal.py`` and ``util/utils.py`` call.  Inputs must be ROCm device
tensors; a host tensor raises (no CPU fallback -- the CPU restatement is ``oracle/``, test-only).
The head always computes in fp32 (FR_F32): it is <0.3 % of the step's FLOPs and the 1e-3 logits bar of
BASELINE.json is an fp32 bar (bf16 operands drift the logits by ~0.2).
"""
import math
import os

import torch

from . import ops
from ._lib import FR_F32
from .engine import _side_stream


def _head_side_stream(dev):
    """The device's weight-gradient stream (engine.py: one per device), or None: FRHIP_SINGLE_STREAM=1."""
    if os.environ.get("FRHIP_SINGLE_STREAM", "0") != "0":
        return None
    return _side_stream(dev, 1)


def _pad(n, m):
    return (n + m - 1) // m * m


def margin_forward(x, weight, label, kind, s, m, easy_margin):
    """logits = s * where(j == label, phi(cos), cos) for fp32 device tensors.  Returns (logits, saved, cfg) for
    ``margin_backward``.  A label outside [0, N) selects nothing in its row (the class-sharded head passes -1 for rows
    whose label lives on another rank)."""
    B, D = x.shape
    N = weight.shape[0]
    dev = x.device
    st = ops.current_stream_ptr()
    x = x.contiguous().float()
    w = weight.contiguous().float()
    label = label.contiguous().long()
    Np = _pad(N, 32)
    xn = torch.empty(B, D, device=dev)
    inv_x = torch.empty(B, device=dev)
    wn = torch.empty(Np, D, device=dev)
    wt = torch.empty(D, Np, device=dev)
    inv_w = torch.empty(N, device=dev)
    ops.call("fr_row_normalize", x, xn, None, inv_x, B, B, D, 0, FR_F32, st)()
    ops.call("fr_row_normalize", w, wn, wt, inv_w, N, Np, D, Np, FR_F32, st)()
    ld = _pad(N, 4)  # 16-byte row pitch for the GEMM's vector stores; [B, N] is a view when N is not a multiple of 4
    store = torch.empty(B, ld, device=dev)
    logits = store if ld == N else store[:, :N]
    cos_t = torch.zeros(B, device=dev)
    if kind == 0:
        cos_m, sin_m = math.cos(m), math.sin(m)
        th, mm = math.cos(math.pi - m), math.sin(math.pi - m) * m
    else:
        cos_m, sin_m, th, mm = m, 0.0, 0.0, 0.0
    ops.conv(st, FR_F32, src=xn, w=wn, out=logits, B=B, RH=1, RW=1, SH=1, SW=1, SC=D, N=N, KH=1, KW=1, stride=1,
             pad=0, mode=0, lda=D, ldc=ld, pro=0, epi=ops.EPI_MARGIN, out_f32=1, margin_kind=kind,
             easy_margin=int(bool(easy_margin)), cos_m=cos_m, sin_m=sin_m, th=th, mm=mm, scale=float(s),
             label=label, cos_t=cos_t)()
    saved = (x, w, label, xn, wt, inv_x, inv_w, cos_t)
    cfg = (kind, float(s), cos_m, sin_m, th, int(bool(easy_margin)), Np)
    return logits, saved, cfg


def margin_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gw) of ``margin_forward``.  ``raw_x_grad``: return G = d loss / d normalize(x) instead of gx (the
    class-sharded head sums G over ranks before it goes through the normalisation backward, which is linear in G)."""
    x, w, label, xn, wt, inv_x, inv_w, cos_t = saved
    kind, s, cos_m, sin_m, th, easy, Np = cfg
    B, D = x.shape
    N = w.shape[0]
    dev = x.device
    st = ops.current_stream_ptr()
    g = g.contiguous().float()
    gcos = torch.empty(B, Np, device=dev)
    ops.call("fr_margin_bwd", g, label, cos_t, gcos, B, N, Np, kind, easy, cos_m, sin_m, th, s, FR_F32, st)()
    gx = gw = None
    # Round 6: the two halves (three launches each, 55 us each at 7000 classes, neither fills the chip) run side by side: the
    # weight's on the weight-gradient stream, which is idle until the backbone's backward pass starts.  Every buffer is
    # allocated on the calling stream, which waits for the side stream before this function returns.
    side = _head_side_stream(dev) if (need_x and need_w) else None
    if side is not None:
        main = torch.cuda.current_stream(dev)
        N4 = _pad(N, 4)
        GW = torch.empty(N4, D, device=dev)
        gw = torch.empty(N, D, device=dev)
        side.wait_stream(main)
        sp = ops.stream_ptr(side)
        ops.call("fr_fill_rows", GW, None, N4, D, sp)()
        ops.wgrad(sp, FR_F32, g=gcos, src=xn, dw=GW, B=B, GH=1, GW=1, Cout=N4, SH=1, SW=1, SC=D, KH=1, KW=1,
                  stride=1, pad=0, ldg=Np, lda=D, pro=0, nsplit=1)()
        ops.call("fr_normalize_bwd", GW, w, inv_w, gw, N, D, sp)()
        need_w = False
    if need_x:
        Gx = torch.empty(B, D, device=dev)
        nk = Np // 32
        splitk = max(1, min(nk, 64, nk // 8))
        slab = torch.empty(splitk, B, D, device=dev)  # K slices to slabs, added in a fixed order (reproducible)
        ops.conv(st, FR_F32, src=gcos, w=wt, out=slab, B=B, RH=1, RW=1, SH=1, SW=1, SC=Np, N=D, KH=1, KW=1,
                 stride=1, pad=0, mode=0, lda=Np, ldc=D, pro=0, epi=ops.EPI_SLAB, out_f32=1, splitk=splitk)()
        ops.call("fr_reduce_parts", slab, splitk, 1, B * D, Gx, None, None, st)()
        if raw_x_grad:
            gx = Gx
        else:
            gx = torch.empty(B, D, device=dev)
            ops.call("fr_normalize_bwd", Gx, x, inv_x, gx, B, D, st)()
    if need_w:
        N4 = _pad(N, 4)  # the weight-gradient GEMM wants 16-byte channel counts; gcos columns >= N are zero
        GW = torch.zeros(N4, D, device=dev)
        ops.wgrad(st, FR_F32, g=gcos, src=xn, dw=GW, B=B, GH=1, GW=1, Cout=N4, SH=1, SW=1, SC=D, KH=1, KW=1,
                  stride=1, pad=0, ldg=Np, lda=D, pro=0, nsplit=1)()
        gw = torch.empty(N, D, device=dev)
        ops.call("fr_normalize_bwd", GW, w, inv_w, gw, N, D, st)()
    if side is not None:
        main.wait_stream(side)
    return gx, gw


class MarginHeadFn(torch.autograd.Function):
    """logits = s * where(j == label, phi(cos), cos),  cos = normalize(x) . normalize(W)^T

    head/metrics.py:97-140 (ArcFace: phi = cos(theta+m) with the cos>th fallback / easy margin) and
    :164-191 (CosFace: phi = cos - m).  Backward per SURVEY.md App. D.
    """

    @staticmethod
    def forward(ctx, x, weight, label, kind, s, m, easy_margin):
        logits, saved, cfg = margin_forward(x, weight, label, kind, s, m, easy_margin)
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(label)
        return logits

    @staticmethod
    def backward(ctx, g):
        gx, gw = margin_backward(ctx.saved_tensors, ctx.cfg, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw, None, None, None, None, None


SPHEREFACE, AM_SOFTMAX = 2, 3  # margin kinds of fr_margin_apply


def margin_ext_forward(x, weight, label, kind, mi, p0, p1):
    """SphereFace (kind 2: ``weight`` [N, D], mi = m, p0 = 1 + lambda) or Am_softmax (kind 3: ``weight`` is the [D, N]
    kernel, p0 = m, p1 = s) logits for fp32 device tensors.  The GEMM stores the raw cosines; fr_margin_apply turns them
    into logits, and the backward pass reads them again for its clamp mask.  Returns (logits, saved, cfg)."""
    B, D = x.shape
    N = weight.shape[0] if kind == SPHEREFACE else weight.shape[1]
    dev = x.device
    st = ops.current_stream_ptr()
    x = x.contiguous().float()
    w = weight.contiguous().float()
    label = label.contiguous().long()
    Np = _pad(N, 32)
    wn = torch.empty(Np, D, device=dev)  # GEMM B operand, rows >= N zero
    wt = torch.empty(D, Np, device=dev)  # its transpose, the B operand of the data gradient
    inv_w = torch.empty(N, device=dev)
    if kind == SPHEREFACE:
        xn = torch.empty(B, D, device=dev)
        inv_x = torch.empty(B, device=dev)
        ops.call("fr_row_normalize", x, xn, None, inv_x, B, B, D, 0, FR_F32, st)()
        ops.call("fr_row_normalize", w, wn, wt, inv_w, N, Np, D, Np, FR_F32, st)()
    else:  # the embeddings are not normalised (head/metrics.py:302-304)
        xn, inv_x = x, None
        ops.call("fr_col_normalize", w, wn, wt, inv_w, D, N, Np, st)()
    ld = _pad(N, 4)
    cos = torch.empty(B, ld, device=dev)
    ops.conv(st, FR_F32, src=xn, w=wn, out=cos, B=B, RH=1, RW=1, SH=1, SW=1, SC=D, N=N, KH=1, KW=1, stride=1, pad=0,
             mode=0, lda=D, ldc=ld, pro=0, epi=ops.EPI_STORE, out_f32=1)()
    store = torch.empty(B, ld, device=dev)
    ops.call("fr_margin_apply", cos, label, inv_x, store, B, N, ld, kind, int(mi), float(p0), float(p1), st)()
    logits = store if ld == N else store[:, :N]
    saved = (x, w, label, xn, wn, wt, inv_x, inv_w, cos)
    cfg = (kind, int(mi), float(p0), float(p1), Np, ld)
    return logits, saved, cfg


def margin_ext_backward(saved, cfg, g, need_x, need_w):
    """(gx, gweight) of ``margin_ext_forward``; gweight has the weight's own layout ([D, N] for Am_softmax)."""
    x, w, label, xn, wn, wt, inv_x, inv_w, cos = saved
    kind, mi, p0, p1, Np, ld = cfg
    B, D = x.shape
    N = w.shape[0] if kind == SPHEREFACE else w.shape[1]
    dev = x.device
    st = ops.current_stream_ptr()
    g = g.contiguous().float()
    gcos = torch.empty(B, Np, device=dev)
    nparts = int(ops.lib.fr_margin_apply_parts(Np))
    r_part = torch.empty(B, nparts, device=dev) if kind == SPHEREFACE else None
    ops.call("fr_margin_apply_bwd", g, cos, label, inv_x, gcos, r_part, B, N, ld, Np, kind, mi, p0, p1, st)()
    N4 = _pad(N, 4)  # the weight-gradient GEMM wants 16-byte channel counts; gcos columns >= N are zero

    def weight_grad(stream, GW):
        ops.wgrad(stream, FR_F32, g=gcos, src=xn, dw=GW, B=B, GH=1, GW=1, Cout=N4, SH=1, SW=1, SC=D, KH=1, KW=1,
                  stride=1, pad=0, ldg=Np, lda=D, pro=0, nsplit=1)()
        gw = torch.empty_like(w)
        if kind == SPHEREFACE:
            ops.call("fr_normalize_bwd", GW, w, inv_w, gw, N, D, stream)()
        else:
            ops.call("fr_col_normalize_bwd", GW, wn, inv_w, gw, D, N, stream)()
        return gw

    gx = gw = None
    # the weight's half on the weight-gradient stream, as margin_backward does
    side = _head_side_stream(dev) if (need_x and need_w) else None
    if side is not None:
        main = torch.cuda.current_stream(dev)
        GW = torch.empty(N4, D, device=dev)
        side.wait_stream(main)
        sp = ops.stream_ptr(side)
        ops.call("fr_fill_rows", GW, None, N4, D, sp)()
        gw = weight_grad(sp, GW)
        need_w = False
    if need_x:
        Gx = torch.empty(B, D, device=dev)
        nk = Np // 32
        splitk = max(1, min(nk, 64, nk // 8))
        slab = torch.empty(splitk, B, D, device=dev)  # K slices to slabs, added in a fixed order (reproducible)
        ops.conv(st, FR_F32, src=gcos, w=wt, out=slab, B=B, RH=1, RW=1, SH=1, SW=1, SC=Np, N=D, KH=1, KW=1,
                 stride=1, pad=0, mode=0, lda=Np, ldc=D, pro=0, epi=ops.EPI_SLAB, out_f32=1, splitk=splitk)()
        if kind == SPHEREFACE:
            ops.call("fr_reduce_parts", slab, splitk, 1, B * D, Gx, None, None, st)()
            gx = torch.empty(B, D, device=dev)
            ops.call("fr_normalize_bwd_radial", Gx, x, inv_x, r_part, nparts, gx, B, D, st)()
        else:
            gx = Gx
            ops.call("fr_reduce_parts", slab, splitk, 1, B * D, gx, None, None, st)()
    if need_w:
        gw = weight_grad(st, torch.zeros(N4, D, device=dev))
    if side is not None:
        main.wait_stream(side)
    return gx, gw


class MarginExtHeadFn(torch.autograd.Function):
    """SphereFace (head/metrics.py:236-268) and Am_softmax (:302-331) on the HIP path; see ``margin_ext_forward``."""

    @staticmethod
    def forward(ctx, x, weight, label, kind, mi, p0, p1):
        logits, saved, cfg = margin_ext_forward(x, weight, label, kind, mi, p0, p1)
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(label)
        return logits

    @staticmethod
    def backward(ctx, g):
        gx, gw = margin_ext_backward(ctx.saved_tensors, ctx.cfg, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw, None, None, None, None, None


def curricular_forward(x, kernel, label, t, s, m, group=None):
    """CurricularFace logits (head/metrics.py:490-510) for fp32 device tensors; ``kernel`` is [D, N], ``t`` the module's
    one-float device buffer, updated in place before it is used (no host read).  ``group``: the batch mean of the target
    cosines is averaged over that process group first (equal batch sizes on every rank), so every rank holds the ``t`` of one
    head over the global batch.  Returns (logits, saved, cfg) for ``curricular_backward``."""
    B, D = x.shape
    N = kernel.shape[1]
    dev = x.device
    st = ops.current_stream_ptr()
    x = x.contiguous().float()
    w = kernel.contiguous().float()
    label = label.contiguous().long()
    Np = _pad(N, 32)
    xn = torch.empty(B, D, device=dev)
    inv_x = torch.empty(B, device=dev)
    wn = torch.empty(Np, D, device=dev)  # GEMM B operand, rows >= N zero
    wt = torch.empty(D, Np, device=dev)  # its transpose, the B operand of the data gradient
    inv_w = torch.empty(N, device=dev)
    ops.call("fr_row_normalize", x, xn, None, inv_x, B, B, D, 0, FR_F32, st)()
    ops.call("fr_col_normalize", w, wn, wt, inv_w, D, N, Np, st)()
    ld = _pad(N, 4)
    cos = torch.empty(B, ld, device=dev)
    ops.conv(st, FR_F32, src=xn, w=wn, out=cos, B=B, RH=1, RW=1, SH=1, SW=1, SC=D, N=N, KH=1, KW=1, stride=1, pad=0,
             mode=0, lda=D, ldc=ld, pro=0, epi=ops.EPI_STORE, out_f32=1)()
    cos_m, sin_m = math.cos(m), math.sin(m)
    th, mm = math.cos(math.pi - m), math.sin(math.pi - m) * m
    rowv = torch.empty(4, B, device=dev)  # tl, ctm, final, branch flag
    mean = torch.empty(1, device=dev)
    ops.call("fr_curricular_rows", cos, label, rowv, mean, t, B, N, ld, cos_m, sin_m, th, mm, int(group is None), st)()
    if group is not None:
        import torch.distributed as dist
        dist.all_reduce(mean, group=group)  # one float, stays on the device
        ops.call("fr_curricular_ema", t, mean, 1.0 / dist.get_world_size(group), st)()
    store = torch.empty(B, ld, device=dev)
    ops.call("fr_curricular_apply", cos, label, rowv, t, store, B, N, ld, float(s), st)()
    logits = store if ld == N else store[:, :N]
    # the backward pass needs the t this forward call used: the buffer moves on with the next call
    saved = (x, w, label, xn, wn, wt, inv_x, inv_w, cos, rowv, t.clone())
    cfg = (float(s), cos_m, sin_m, Np, ld)
    return logits, saved, cfg


def curricular_backward(saved, cfg, g, need_x, need_w):
    """(gx, gkernel) of ``curricular_forward``; gkernel is [D, N].  The GEMMs of ``margin_ext_backward``, between
    fr_curricular_bwd and the two normalisation backwards."""
    x, w, label, xn, wn, wt, inv_x, inv_w, cos, rowv, t = saved
    s, cos_m, sin_m, Np, ld = cfg
    B, D = x.shape
    N = w.shape[1]
    dev = x.device
    st = ops.current_stream_ptr()
    g = g.contiguous().float()
    gcos = torch.empty(B, Np, device=dev)
    ops.call("fr_curricular_bwd", g, cos, label, rowv, t, gcos, B, N, ld, Np, cos_m, sin_m, s, st)()
    N4 = _pad(N, 4)  # the weight-gradient GEMM wants 16-byte channel counts; gcos columns >= N are zero

    def weight_grad(stream, GW):
        ops.wgrad(stream, FR_F32, g=gcos, src=xn, dw=GW, B=B, GH=1, GW=1, Cout=N4, SH=1, SW=1, SC=D, KH=1, KW=1,
                  stride=1, pad=0, ldg=Np, lda=D, pro=0, nsplit=1)()
        gw = torch.empty_like(w)
        ops.call("fr_col_normalize_bwd", GW, wn, inv_w, gw, D, N, stream)()
        return gw

    gx = gw = None
    # the weight's half on the weight-gradient stream, as margin_backward does
    side = _head_side_stream(dev) if (need_x and need_w) else None
    if side is not None:
        main = torch.cuda.current_stream(dev)
        GW = torch.empty(N4, D, device=dev)
        side.wait_stream(main)
        sp = ops.stream_ptr(side)
        ops.call("fr_fill_rows", GW, None, N4, D, sp)()
        gw = weight_grad(sp, GW)
        need_w = False
    if need_x:
        Gx = torch.empty(B, D, device=dev)
        nk = Np // 32
        splitk = max(1, min(nk, 64, nk // 8))
        slab = torch.empty(splitk, B, D, device=dev)  # K slices to slabs, added in a fixed order (reproducible)
        ops.conv(st, FR_F32, src=gcos, w=wt, out=slab, B=B, RH=1, RW=1, SH=1, SW=1, SC=Np, N=D, KH=1, KW=1,
                 stride=1, pad=0, mode=0, lda=Np, ldc=D, pro=0, epi=ops.EPI_SLAB, out_f32=1, splitk=splitk)()
        ops.call("fr_reduce_parts", slab, splitk, 1, B * D, Gx, None, None, st)()
        gx = torch.empty(B, D, device=dev)
        ops.call("fr_normalize_bwd", Gx, x, inv_x, gx, B, D, st)()
    if need_w:
        gw = weight_grad(st, torch.zeros(N4, D, device=dev))
    if side is not None:
        main.wait_stream(side)
    return gx, gw


class CurricularHeadFn(torch.autograd.Function):
    """CurricularFace (head/metrics.py:475-510) on the HIP path; see ``curricular_forward``."""

    @staticmethod
    def forward(ctx, x, kernel, label, t, s, m, group):
        logits, saved, cfg = curricular_forward(x, kernel, label, t, s, m, group)
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(label)
        return logits

    @staticmethod
    def backward(ctx, g):
        gx, gw = curricular_backward(ctx.saved_tensors, ctx.cfg, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw, None, None, None, None, None


CHECK_LABELS = True  # host-side range check of the labels (one device sync per call); loops with validated data clear it


def _check_labels(label, n):
    if CHECK_LABELS and (label.min() < 0 or label.max() >= n):  # reference: RuntimeError from scatter_ (metrics.py:134)
        raise RuntimeError("index %d is out of bounds for dimension 1 with size %d" % (int(label.max()), n))


def margin_head(x, weight, label, kind, s, m, easy_margin=False):
    if x.shape[0] == 0:  # the reference returns empty logits (F.linear / scatter_ on zero rows); nothing to launch
        ops.ptr(x)  # host tensors still fail loudly
        return x.new_zeros((0, weight.shape[0]), dtype=torch.float32) + 0.0 * (x.sum() + weight.sum())
    _check_labels(label, weight.shape[0])
    return MarginHeadFn.apply(x, weight, label, kind, s, m, easy_margin)


def margin_ext_head(x, weight, label, kind, mi, p0, p1):
    """SphereFace (kind 2) / Am_softmax (kind 3) logits; the empty batch and label check of ``margin_head``."""
    n = weight.shape[0] if kind == SPHEREFACE else weight.shape[1]
    if x.shape[0] == 0:
        ops.ptr(x)
        return x.new_zeros((0, n), dtype=torch.float32) + 0.0 * (x.sum() + weight.sum())
    _check_labels(label, n)
    return MarginExtHeadFn.apply(x, weight, label, kind, mi, p0, p1)


def curricular_head(x, kernel, label, t, s, m, group=None):
    """CurricularFace logits; the empty batch and label check of ``margin_head``.  ``t`` (float32 [1] on x's device) is
    updated in place; an empty batch leaves it as it is (the reference's mean over no rows turns it into NaN for good)."""
    n = kernel.shape[1]
    if x.shape[0] == 0:
        ops.ptr(x)
        return x.new_zeros((0, n), dtype=torch.float32) + 0.0 * (x.sum() + kernel.sum())
    _check_labels(label, n)
    if t.dtype != torch.float32 or t.numel() != 1 or t.device != x.device or not t.is_contiguous():
        raise ValueError("curricular_head: t must be a contiguous float32 tensor of one element on %s" % (x.device,))
    return CurricularHeadFn.apply(x, kernel, label, t, s, m, group)


class FocalLossFn(torch.autograd.Function):
    """loss = (1 - exp(-l))^gamma * l,  l = mean_i CE(logits_i, y_i)   -- loss/focal.py:17-21."""

    @staticmethod
    def forward(ctx, logits, target, gamma):
        B, N = logits.shape
        dev = logits.device
        st = ops.current_stream_ptr()
        logits = logits.contiguous().float()
        target = target.contiguous().long()
        lse = torch.empty(B, device=dev)
        ce = torch.empty(B, device=dev)
        rank = torch.empty(B, device=dev, dtype=torch.int32)
        scalars = torch.empty(8, device=dev)
        ops.call("fr_ce_rows", logits, target, lse, ce, rank, B, N, N, st)()
        ops.call("fr_focal_finalize", ce, rank, B, float(gamma), scalars, st)()
        ctx.save_for_backward(logits, target, lse, scalars)
        return scalars[0].clone()

    @staticmethod
    def backward(ctx, gup):
        logits, target, lse, scalars = ctx.saved_tensors
        B, N = logits.shape
        st = ops.current_stream_ptr()
        grad = torch.empty_like(logits)
        gup = gup.contiguous().float().reshape(1)
        ops.call("fr_focal_bwd", logits, target, lse, scalars, gup, grad, B, N, N, st)()
        return grad, None, None


def focal_loss(logits, target, gamma=2.0):
    if logits.shape[0] == 0:  # mean cross entropy of no rows is NaN in the reference (loss/focal.py:18)
        ops.ptr(logits)
        return logits.sum() * float("nan")
    return FocalLossFn.apply(logits, target, gamma)


def topk_precision(rank, topk):
    """[precision@k in percent for k in topk] from the label ranks (device float32 [len(topk)]); the arithmetic of
    ``(rank < k).float().sum().mul_(100.0 / n)`` (reference util/utils.py:343-358) in one launch."""
    ks = [int(k) for k in topk] + [0] * (4 - len(topk))
    out = torch.empty(len(topk), device=rank.device, dtype=torch.float32)
    ops.call("fr_topk_precision", rank, rank.numel(), len(topk), ks[0], ks[1], ks[2], ks[3], 100.0 / rank.numel(), out,
             ops.current_stream_ptr())()
    return out


def topk_ranks(logits, target):
    """rank[m] = number of classes scoring strictly above the label's logit (device int32 [B])."""
    B, N = logits.shape
    if B == 0:
        ops.ptr(logits)
        return torch.empty(0, device=logits.device, dtype=torch.int32)
    st = ops.current_stream_ptr()
    logits = logits.contiguous().float()
    rank = torch.empty(B, device=logits.device, dtype=torch.int32)
    ops.call("fr_rank_rows", logits, target.contiguous().long(), rank, B, N, N, st)()
    return rank
