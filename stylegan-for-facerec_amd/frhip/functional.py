"""autograd.Function wrappers over the HIP kernels for the heads (the margin heads, the plain Softmax head and the queue head
SST_Prototype), the focal
loss, the plain cross entropy and top-k accuracy.

These are what ``head/metrics.py``, ``loss/focal.py``, ``loss/softmax.py`` and ``util/utils.py`` call.  Inputs must be
ROCm device tensors; a host tensor raises (no CPU fallback -- the CPU restatement is ``oracle/``, test-only).
The head always computes in fp32 (FR_F32): it is <0.3 % of the step's FLOPs and the 1e-3 logits bar of
BASELINE.json is an fp32 bar (bf16 operands drift the logits by ~0.2).
"""
import collections
import math
import os
import struct

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


# One cosine-head pipeline under the heads.  Forward: ``_cosine_front`` (``_cosine_operands``: normalised operands; the
# cosine GEMM, ``_raw_cosines``; the logit store) or ArcFace / CosFace's fused margin epilogue, then the head's row kernels.
# Backward: the head's gcos kernel (``_gcos_backward``), then ``_cosine_backward`` (both GEMMs and the normalisation
# backwards).
(ARCFACE, COSFACE, SPHEREFACE, AM_SOFTMAX, CURRICULAR, MAGFACE, ADACOS, NPCFACE, MV_SOFTMAX, CIRCLE, AM_SOFTMAX_N, ARCNEG,
 SOFTMAX) = range(13)
# 0..3: the kernels' margin kinds.  AM_SOFTMAX_N is the FaceX-Zoo AM_Softmax (normalised embeddings) on the kernels' kind 3.
# SOFTMAX is the plain linear head with a bias: no cosines, the same three GEMMs on operands that are not normalised.

# The operand layout of each head, read by both directions: norm_x (the rows of x are normalised; Am_softmax's are not,
# head/metrics.py:302-304) and col_weight (the weight is a [D, N] kernel normalised by columns, not [N, D] by rows).
_OPERANDS = {ARCFACE: (True, False), COSFACE: (True, False), SPHEREFACE: (True, False), AM_SOFTMAX: (False, True),
             CURRICULAR: (True, True), MAGFACE: (True, True), ADACOS: (True, False), NPCFACE: (True, True),
             MV_SOFTMAX: (True, True), CIRCLE: (True, True), AM_SOFTMAX_N: (True, True), ARCNEG: (True, False),
             SOFTMAX: (False, False)}

# What a forward call keeps for its backward call; a head leaves what it does not use at None.  xn / wn [Np, D] / wt
# [D, Np] are the GEMM operands (xn is x itself for Am_softmax), inv_x / inv_w the reciprocal norms, cos_t the target
# cosines of the fused epilogue, cos the raw cosines [B, ld], rowv and t CurricularFace's row values and the t it used
# (rowv: MagFace's and NPCFace's six row values and MV_Softmax's four too; t: the scale an AdaCos call used).  HeadCfg.mag:
# MagFace's (margin_am, l_a, u_a, l_margin, u_margin, lamda); HeadCfg.p0 / p1: NPCFace's t / a; p0: MV_Softmax's mv_weight;
# p0 / p1 / s: CircleLoss's O_p / O_n / gamma; p0 / p1: AM_Softmax's margin / scale, as Am_softmax's; p0 / p1 / s: ArcNegFace's
# alpha / sigma / scale (rowv: its three row values).
HeadSaved = collections.namedtuple("HeadSaved", "x w label xn wn wt inv_x inv_w cos_t cos rowv t", defaults=(None,) * 12)
HeadCfg = collections.namedtuple("HeadCfg", "kind Np ld s cos_m sin_m th easy mi p0 p1 mag", defaults=(None,) * 9)


def _cosine_operands(kind, x, weight, label):
    """fp32 copies and the normalised GEMM operands of a head of ``kind`` (``_OPERANDS``): rows of x, and rows of an [N, D]
    weight or columns of a [D, N] kernel.  Returns (HeadSaved with x .. inv_w set, N, Np, ld)."""
    norm_x, col_weight = _OPERANDS[kind]
    B, D = x.shape
    N = weight.shape[1] if col_weight else weight.shape[0]
    dev = x.device
    st = ops.current_stream_ptr()
    x = x.contiguous().float()
    w = weight.contiguous().float()
    label = label.contiguous().long()
    Np = _pad(N, 32)
    wn = torch.empty(Np, D, device=dev)  # GEMM B operand, rows >= N zero
    wt = torch.empty(D, Np, device=dev)  # its transpose, the B operand of the data gradient
    inv_w = torch.empty(N, device=dev)
    if norm_x:
        xn = torch.empty(B, D, device=dev)
        inv_x = torch.empty(B, device=dev)
        ops.call("fr_row_normalize", x, xn, None, inv_x, B, B, D, 0, FR_F32, st)()
    else:  # Am_softmax: the embeddings are not normalised (head/metrics.py:302-304)
        xn, inv_x = x, None
    if col_weight:
        ops.call("fr_col_normalize", w, wn, wt, inv_w, D, N, Np, st)()
    else:
        ops.call("fr_row_normalize", w, wn, wt, inv_w, N, Np, D, Np, FR_F32, st)()
    # ld: 16-byte row pitch for the GEMM's vector stores; [B, N] is a view when N is not a multiple of 4
    return HeadSaved(x, w, label, xn, wn, wt, inv_x, inv_w), N, Np, _pad(N, 4)


def _cosine_gemm(sv, out, N, ld, epi, **epilogue):
    B, D = sv.xn.shape
    ops.conv(ops.current_stream_ptr(), FR_F32, src=sv.xn, w=sv.wn, out=out, B=B, RH=1, RW=1, SH=1, SW=1, SC=D, N=N, KH=1,
             KW=1, stride=1, pad=0, mode=0, lda=D, ldc=ld, pro=0, epi=epi, out_f32=1, **epilogue)()


def _raw_cosines(sv, N, ld):
    """cos [B, ld]: the GEMM stores the raw cosines; a row kernel turns them into logits, and the backward pass reads them
    again for its clamp mask."""
    cos = torch.empty(sv.x.shape[0], ld, device=sv.x.device)
    _cosine_gemm(sv, cos, N, ld, ops.EPI_STORE)
    return cos


def _logit_store(sv, N, ld):
    """(store [B, ld], its logits view [B, N])."""
    store = torch.empty(sv.x.shape[0], ld, device=sv.x.device)
    return store, (store if ld == N else store[:, :N])


def _cosine_front(kind, x, weight, label):
    """The forward front of a head whose row kernels work on the raw cosines: (HeadSaved with x .. inv_w and cos set, N,
    Np, ld, the logit store [B, ld], its logits view [B, N])."""
    sv, N, Np, ld = _cosine_operands(kind, x, weight, label)
    sv = sv._replace(cos=_raw_cosines(sv, N, ld))
    return (sv, N, Np, ld) + _logit_store(sv, N, ld)


def _cosine_backward(sv, cfg, gcos, need_x, need_w, raw_x_grad=False, r_part=None):
    """(gx, gw) from gcos = d loss / d cos [B, cfg.Np] (columns >= N zero): the weight-gradient GEMM, the split-K
    data-gradient GEMM and the normalisation backwards.  gx goes through the backward of the row normalisation, with the
    radial term of a row scale where ``r_part`` is given (SphereFace, MagFace); the reduced G itself is the result where x
    was not normalised (``_OPERANDS``: Am_softmax, Softmax) and under ``raw_x_grad`` (the class-sharded head).  gw has the
    weight's own layout; for the Softmax head (an [N, D] weight that is not normalised, ``sv.inv_w`` None) it is the GEMM's
    result itself, its first N rows.

    Round 6: the two halves (three launches each, 55 us each at 7000 classes, neither fills the chip) run side by side when
    both are wanted: the weight's on the weight-gradient stream, which is idle until the backbone's backward pass starts.
    Every buffer is allocated on the calling stream, which waits for the side stream before this function returns."""
    norm_x, col_weight = _OPERANDS[cfg.kind]
    norm_w, Np = cfg.kind != SOFTMAX, cfg.Np
    B, D = sv.xn.shape
    N = sv.inv_w.shape[0] if norm_w else sv.w.shape[0]
    dev = sv.x.device
    st = ops.current_stream_ptr()
    gx = gw = None
    if need_w:
        N4 = _pad(N, 4)  # the weight-gradient GEMM wants 16-byte channel counts; gcos columns >= N are zero
        GW = torch.empty(N4, D, device=dev)
        gw = torch.empty_like(sv.w) if norm_w else GW[:N]

    def weight_half(stream):
        ops.call("fr_fill_rows", GW, None, N4, D, stream)()
        ops.wgrad(stream, FR_F32, g=gcos, src=sv.xn, dw=GW, B=B, GH=1, GW=1, Cout=N4, SH=1, SW=1, SC=D, KH=1, KW=1,
                  stride=1, pad=0, ldg=Np, lda=D, pro=0, nsplit=1)()
        if norm_w and col_weight:
            ops.call("fr_col_normalize_bwd", GW, sv.wn, sv.inv_w, gw, D, N, stream)()
        elif norm_w:
            ops.call("fr_normalize_bwd", GW, sv.w, sv.inv_w, gw, N, D, stream)()

    side = _head_side_stream(dev) if (need_x and need_w) else None
    if side is not None:
        main = torch.cuda.current_stream(dev)
        side.wait_stream(main)
        weight_half(ops.stream_ptr(side))
    if need_x:
        G = torch.empty(B, D, device=dev)
        nk = Np // 32
        splitk = max(1, min(nk, 64, nk // 8))
        slab = torch.empty(splitk, B, D, device=dev)  # K slices to slabs, added in a fixed order (reproducible)
        ops.conv(st, FR_F32, src=gcos, w=sv.wt, out=slab, B=B, RH=1, RW=1, SH=1, SW=1, SC=Np, N=D, KH=1, KW=1,
                 stride=1, pad=0, mode=0, lda=Np, ldc=D, pro=0, epi=ops.EPI_SLAB, out_f32=1, splitk=splitk)()
        ops.call("fr_reduce_parts", slab, splitk, 1, B * D, G, None, None, st)()
        if raw_x_grad or not norm_x:
            gx = G
        else:
            gx = torch.empty(B, D, device=dev)
            if r_part is not None:
                ops.call("fr_normalize_bwd_radial", G, sv.x, sv.inv_x, r_part, r_part.shape[1], gx, B, D, st)()
            else:
                ops.call("fr_normalize_bwd", G, sv.x, sv.inv_x, gx, B, D, st)()
    if need_w and side is None:
        weight_half(st)
    if side is not None:
        main.wait_stream(side)
    return gx, gw


def _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, launch):
    """The backward body of a head that is one gcos kernel in front of ``_cosine_backward``: ``launch(g, gcos, B, N, st)``
    is the head's one launch, from the fp32 contiguous upstream gradient into gcos [B, cfg.Np].  ``raw_x_grad``: return G =
    d loss / d normalize(x) instead of gx (the class-sharded head sums G over ranks before it goes through the normalisation
    backward, which is linear in G)."""
    B, N = saved.x.shape[0], saved.inv_w.shape[0]
    gcos = torch.empty(B, cfg.Np, device=saved.x.device)
    launch(g.contiguous().float(), gcos, B, N, ops.current_stream_ptr())
    return _cosine_backward(saved, cfg, gcos, need_x, need_w, raw_x_grad)


def margin_forward(x, weight, label, kind, s, m, easy_margin):
    """ArcFace (kind 0) / CosFace (kind 1): logits = s * where(j == label, phi(cos), cos) for fp32 device tensors, the
    margin in the GEMM's epilogue.  Returns (logits, saved, cfg) for ``margin_backward``.  A label outside [0, N) selects
    nothing in its row (the class-sharded head passes -1 for rows whose label lives on another rank)."""
    sv, N, Np, ld = _cosine_operands(kind, x, weight, label)
    _, logits = _logit_store(sv, N, ld)
    cos_t = torch.zeros(x.shape[0], device=x.device)
    if kind == ARCFACE:
        cos_m, sin_m = math.cos(m), math.sin(m)
        th, mm = math.cos(math.pi - m), math.sin(math.pi - m) * m
    else:
        cos_m, sin_m, th, mm = m, 0.0, 0.0, 0.0
    easy = int(bool(easy_margin))
    _cosine_gemm(sv, logits, N, ld, ops.EPI_MARGIN, margin_kind=kind, easy_margin=easy, cos_m=cos_m, sin_m=sin_m, th=th,
                 mm=mm, scale=float(s), label=sv.label, cos_t=cos_t)
    cfg = HeadCfg(kind, Np, ld, s=float(s), cos_m=cos_m, sin_m=sin_m, th=th, easy=easy)
    return logits, sv._replace(wn=None, cos_t=cos_t), cfg


def margin_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gw) of ``margin_forward``.  ``raw_x_grad``: return G = d loss / d normalize(x) instead of gx (the
    class-sharded head sums G over ranks before it goes through the normalisation backward, which is linear in G)."""
    return _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, lambda g, gcos, B, N, st: ops.call(
        "fr_margin_bwd", g, saved.label, saved.cos_t, gcos, B, N, cfg.Np, cfg.kind, cfg.easy, cfg.cos_m, cfg.sin_m, cfg.th,
        cfg.s, FR_F32, st)())


def margin_ext_forward(x, weight, label, kind, mi, p0, p1):
    """SphereFace (kind 2: ``weight`` [N, D], mi = m, p0 = 1 + lambda) or Am_softmax (kind 3: ``weight`` is the [D, N]
    kernel, p0 = m, p1 = s) logits for fp32 device tensors: fr_margin_apply on the raw cosines.  Returns (logits, saved,
    cfg) for ``margin_ext_backward``."""
    sv, N, Np, ld, store, logits = _cosine_front(kind, x, weight, label)
    ops.call("fr_margin_apply", sv.cos, sv.label, sv.inv_x, store, x.shape[0], N, ld, kind, int(mi), float(p0), float(p1),
             ops.current_stream_ptr())()
    return logits, sv, HeadCfg(kind, Np, ld, mi=int(mi), p0=float(p0), p1=float(p1))


def margin_ext_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gweight) of ``margin_ext_forward``; gweight has the weight's own layout ([D, N] for Am_softmax).
    ``raw_x_grad``: (G, gweight, r_part) instead, G = d loss / d xn before the normalisation backward and r_part
    SphereFace's [B, parts] radial sums (None for Am_softmax): the class-sharded head sums both over the ranks first, as
    with ``raw_x_grad`` of ``margin_backward``."""
    sphere = cfg.kind == SPHEREFACE
    B, N = saved.x.shape[0], saved.inv_w.shape[0]
    dev = saved.x.device
    gcos = torch.empty(B, cfg.Np, device=dev)
    r_part = torch.empty(B, int(ops.lib.fr_margin_apply_parts(cfg.Np)), device=dev) if sphere else None
    ops.call("fr_margin_apply_bwd", g.contiguous().float(), saved.cos, saved.label, saved.inv_x, gcos, r_part, B, N, cfg.ld,
             cfg.Np, cfg.kind, cfg.mi, cfg.p0, cfg.p1, ops.current_stream_ptr())()
    if raw_x_grad:
        return _cosine_backward(saved, cfg, gcos, need_x, need_w, raw_x_grad=True) + (r_part,)
    return _cosine_backward(saved, cfg, gcos, need_x, need_w, r_part=r_part)


def curricular_forward(x, kernel, label, t, s, m, group=None, target_cos=None, train=True):
    """CurricularFace logits (head/metrics.py:490-510) for fp32 device tensors; ``kernel`` is [D, N], ``t`` the module's
    one-float device buffer, updated in place before it is used (no host read).  ``group``: the batch mean of the target
    cosines is averaged over that process group first (equal batch sizes on every rank), so every rank holds the ``t`` of one
    head over the global batch.  ``target_cos``: a hook ``(cos, label, N, ld) -> tl [B]`` called on the raw cosines in place
    of the gather of the target cosines (the class-sharded head: a row's label may live on another rank; the hook exchanges
    them); the row values and ``t`` (moved only if ``train``) then come from its result.  Returns (logits, saved, cfg) for
    ``curricular_backward``."""
    sv, N, Np, ld, store, logits = _cosine_front(CURRICULAR, x, kernel, label)
    B = x.shape[0]
    st = ops.current_stream_ptr()
    cos_m, sin_m = math.cos(m), math.sin(m)
    th, mm = math.cos(math.pi - m), math.sin(math.pi - m) * m
    rowv = torch.empty(4, B, device=x.device)  # tl, ctm, final, branch flag
    mean = torch.empty(1, device=x.device)
    if target_cos is not None:
        tl = target_cos(sv.cos, sv.label, N, ld)
        ops.call("fr_curricular_rows_from", tl, rowv, mean, t, B, cos_m, sin_m, th, mm, int(bool(train)), st)()
    else:
        ops.call("fr_curricular_rows", sv.cos, sv.label, rowv, mean, t, B, N, ld, cos_m, sin_m, th, mm, int(group is None),
                 st)()
    if group is not None and target_cos is None:
        import torch.distributed as dist
        dist.all_reduce(mean, group=group)  # one float, stays on the device
        ops.call("fr_curricular_ema", t, mean, 1.0 / dist.get_world_size(group), st)()
    ops.call("fr_curricular_apply", sv.cos, sv.label, rowv, t, store, B, N, ld, float(s), st)()
    # the backward pass needs the t this forward call used: the buffer moves on with the next call
    saved = sv._replace(rowv=rowv, t=t.clone())
    return logits, saved, HeadCfg(CURRICULAR, Np, ld, s=float(s), cos_m=cos_m, sin_m=sin_m)


def curricular_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gkernel) of ``curricular_forward``; gkernel is [D, N].  ``raw_x_grad``: as in ``margin_backward``."""
    return _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, lambda g, gcos, B, N, st: ops.call(
        "fr_curricular_bwd", g, saved.cos, saved.label, saved.rowv, saved.t, gcos, B, N, cfg.ld, cfg.Np, cfg.cos_m, cfg.sin_m,
        cfg.s, st)())


def magface_forward(x, kernel, label, s, margin_am, l_a, u_a, l_margin, u_margin, lamda):
    """MagFace (head/metrics.py:512-553) for fp32 device tensors; ``kernel`` is [D, N].  Returns (logits [B, N], loss_g
    [B, 1] = lamda * (a / u_a^2 + 1 / a) with a = clamp(||x||, l_a, u_a), saved, cfg) for ``magface_backward``.  The row
    kernel takes the norms from x itself.  A label outside [0, N) selects nothing in its row."""
    sv, N, Np, ld, store, logits = _cosine_front(MAGFACE, x, kernel, label)
    B = x.shape[0]
    st = ops.current_stream_ptr()
    mag = tuple(float(v) for v in (margin_am, l_a, u_a, l_margin, u_margin, lamda))
    rowv = torch.empty(6, B, device=x.device)  # a, cos_m, sin_m, min_cos, loss_g, inside
    ops.call("fr_magface_rows", sv.x, rowv, B, x.shape[1], *mag[1:], st)()
    ops.call("fr_magface_apply", sv.cos, sv.label, rowv, store, B, N, ld, float(s), mag[0], st)()
    return logits, rowv[4].clone().view(B, 1), sv._replace(rowv=rowv), HeadCfg(MAGFACE, Np, ld, s=float(s), mag=mag)


def magface_backward(saved, cfg, g, glossg, need_x, need_w):
    """(gx, gkernel) of ``magface_forward`` from the upstream gradients of the logits and of loss_g; either may be None
    (zeros).  gx leaves the tangent plane of normalize(x): the radial scalar r [B] of fr_magface_bwd (the margin's and
    loss_g's dependence on ||x||) goes through fr_normalize_bwd_radial."""
    B, N = saved.x.shape[0], saved.inv_w.shape[0]
    dev = saved.x.device
    g = torch.zeros(B, N, device=dev) if g is None else g.contiguous().float()
    if glossg is not None:
        glossg = glossg.contiguous().float()
    gcos = torch.empty(B, cfg.Np, device=dev)
    r = torch.empty(B, device=dev)
    ops.call("fr_magface_bwd", g, glossg, saved.cos, saved.label, saved.rowv, gcos, r, B, N, cfg.ld, cfg.Np, cfg.s,
             *cfg.mag[1:], ops.current_stream_ptr())()
    return _cosine_backward(saved, cfg, gcos, need_x, need_w, r_part=r.view(B, 1))


def adacos_forward(x, weight, label, scale, group=None):
    """AdaCos logits (head/metrics.py:351-369) for fp32 device tensors; ``weight`` is [N, D], ``scale`` the module's
    one-float device buffer.  It is read and written by kernels only, through its pointer (no host read): the row kernel
    takes the row sums of exp(scale_old * cos) and the target cosines, the scale kernel moves the buffer in place, and the
    logits are the NEW scale times the unclamped cosines.  ``group``: every rank all-gathers the [2, B] row values and
    reduces the gathered rows in rank order, so every rank holds the bits of the scale of one head over the concatenated
    batch (equal batch sizes on every rank).  Returns (logits, saved, cfg) for ``adacos_backward``."""
    sv, N, Np, ld, store, logits = _cosine_front(ADACOS, x, weight, label)
    B = x.shape[0]
    st = ops.current_stream_ptr()
    rowv = torch.empty(2, B, device=x.device)  # sum of exp(scale * cos) off the label column, raw target cosine
    ops.call("fr_adacos_rows", sv.cos, sv.label, scale, rowv, B, N, ld, st)()
    rows = B
    if group is not None:
        import torch.distributed as dist
        world = dist.get_world_size(group)
        every = torch.empty(world, 2, B, device=x.device)
        dist.all_gather_into_tensor(every, rowv, group=group)
        rowv, rows = every.permute(1, 0, 2).reshape(2, world * B), world * B  # [2][world * B], ranks in order
    ops.call("fr_adacos_scale", rowv, rows, scale, st)()
    ops.call("fr_adacos_apply", sv.cos, scale, store, B, N, ld, ld, st)()
    # the backward pass needs the scale this forward call used: the buffer moves on with the next call
    return logits, sv._replace(t=scale.clone()), HeadCfg(ADACOS, Np, ld)


def adacos_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gweight) of ``adacos_forward``: the scale is a constant of the graph and the cosines are not clamped, so gcos =
    scale_used * g (columns N .. Np zero).  ``raw_x_grad``: as in ``margin_backward``."""
    return _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, lambda g, gcos, B, N, st: ops.call(
        "fr_adacos_apply", g, saved.t, gcos, B, N, N, cfg.Np, st)())


def npcface_forward(x, kernel, label, s, npc):
    """NPCFace logits (head/metrics.py:612-636) for fp32 device tensors; ``kernel`` is [D, N], ``npc`` the head's (cos_m,
    sin_m, m0, m1, t, a), the attributes its forward pass reads.  A row kernel takes per row the target cosine,
    cos(theta + m), the mean and the count of the hard negatives (the clamped cosines above cos(theta + m), label column
    excluded; the sum in a fixed order) and from them the label column's value at the margin m0 + m1 * mean; a row kernel
    re-weights the hard negatives to t * c + a.  Nothing waits on the host.  A label outside [0, N) selects nothing and
    makes nothing hard in its row.  Returns (logits, saved, cfg) for ``npcface_backward``."""
    sv, N, Np, ld, store, logits = _cosine_front(NPCFACE, x, kernel, label)
    B = x.shape[0]
    st = ops.current_stream_ptr()
    cos_m, sin_m, m0, m1, t, a = (float(v) for v in npc)
    rowv = torch.empty(6, B, device=x.device)  # gt, ctm, final, d final / d gt, avg, count
    ops.call("fr_npcface_rows", sv.cos, sv.label, rowv, B, N, ld, cos_m, sin_m, m0, m1, st)()
    ops.call("fr_npcface_apply", sv.cos, sv.label, rowv, store, B, N, ld, t, a, float(s), st)()
    return logits, sv._replace(rowv=rowv), HeadCfg(NPCFACE, Np, ld, s=float(s), p0=t, p1=a)


def npcface_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gkernel) of ``npcface_forward``; gkernel is [D, N].  The margin m0 + m1 * mean, the hard mask and the branch are
    constants of the graph (:621 no_grad).  ``raw_x_grad``: as in ``margin_backward``."""
    return _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, lambda g, gcos, B, N, st: ops.call(
        "fr_npcface_bwd", g, saved.cos, saved.label, saved.rowv, gcos, B, N, cfg.ld, cfg.Np, cfg.p0, cfg.s, st)())


def mv_softmax_forward(x, weight, label, s, mv):
    """MV_Softmax logits (head/metrics.py:571-590) for fp32 device tensors; ``weight`` is [D, N], ``mv`` the head's (is_am,
    p0, p1, w): p0 = margin with ``is_am``, (p0, p1) = (cos_m, sin_m) without, w = mv_weight.  The row values depend on the
    target cosine alone, so one row kernel does it all: every wave reads its row's target cosine, derives thr and the label
    column's value, re-weights the hard negatives (c > thr) to w * c + w - 1, and leaves rowv [4, B] (gt, thr, final,
    d final / d gt) for the backward pass.  The cosines are never clamped.  Nothing waits on the host.  A label outside
    [0, N) selects nothing and makes nothing hard in its row.  Returns (logits, saved, cfg) for ``mv_softmax_backward``."""
    sv, N, Np, ld, store, logits = _cosine_front(MV_SOFTMAX, x, weight, label)
    B = x.shape[0]
    is_am, p0, p1, w = bool(mv[0]), float(mv[1]), float(mv[2]), float(mv[3])
    rowv = torch.empty(4, B, device=x.device)  # gt, thr, final, d final / d gt
    ops.call("fr_mv_softmax_apply", sv.cos, sv.label, rowv, store, B, N, ld, int(is_am), p0, p1, w, float(s),
             ops.current_stream_ptr())()
    return logits, sv._replace(rowv=rowv), HeadCfg(MV_SOFTMAX, Np, ld, s=float(s), p0=w)


def mv_softmax_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gweight) of ``mv_softmax_forward``; gweight is [D, N].  The hard mask and the branch of the label column are
    comparisons and take no gradient; no cosine is masked out (the head never clamps).  ``raw_x_grad``: as in
    ``margin_backward``."""
    return _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, lambda g, gcos, B, N, st: ops.call(
        "fr_mv_softmax_bwd", g, saved.cos, saved.label, saved.rowv, gcos, B, N, cfg.ld, cfg.Np, cfg.p0, cfg.s, st)())


def circle_forward(x, weight, label, circle):
    """CircleLoss logits (head/metrics.py:451-473, the classification form) for fp32 device tensors; ``weight`` is [D, N],
    ``circle`` the head's (O_p, O_n, delta_p, delta_n, gamma).  Element-wise on the clamped cosines: one row kernel, no row
    values, nothing waits on the host.  A label outside [0, N) makes every column of its row a negative.  Returns (logits,
    saved, cfg) for ``circle_backward``."""
    sv, N, Np, ld, store, logits = _cosine_front(CIRCLE, x, weight, label)
    o_p, o_n, delta_p, delta_n, gamma = (float(v) for v in circle)
    ops.call("fr_circle_apply", sv.cos, sv.label, store, x.shape[0], N, ld, o_p, o_n, delta_p, delta_n, gamma,
             ops.current_stream_ptr())()
    return logits, sv, HeadCfg(CIRCLE, Np, ld, s=gamma, p0=o_p, p1=o_n)


def circle_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gweight) of ``circle_forward``; gweight is [D, N].  alpha is a constant of the graph (:463-464 detach), so gcos =
    g * gamma * alpha inside the clamp, alpha recomputed from the saved raw cosines.  ``raw_x_grad``: as in
    ``margin_backward``."""
    return _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, lambda g, gcos, B, N, st: ops.call(
        "fr_circle_bwd", g, saved.cos, saved.label, gcos, B, N, cfg.ld, cfg.Np, cfg.p0, cfg.p1, cfg.s, st)())


def am_softmax_n_forward(x, weight, label, m, s):
    """The FaceX-Zoo AM_Softmax logits (head/metrics.py:380-392) for fp32 device tensors; ``weight`` is [D, N].  It is
    Am_softmax's arithmetic (fr_margin_apply kind 3: s * (label ? clamp(c) - m : clamp(c))) on the cosines of NORMALISED
    embeddings.  Returns (logits, saved, cfg) for ``am_softmax_n_backward``."""
    sv, N, Np, ld, store, logits = _cosine_front(AM_SOFTMAX_N, x, weight, label)
    ops.call("fr_margin_apply", sv.cos, sv.label, None, store, x.shape[0], N, ld, AM_SOFTMAX, 0, float(m), float(s),
             ops.current_stream_ptr())()
    return logits, sv, HeadCfg(AM_SOFTMAX_N, Np, ld, mi=0, p0=float(m), p1=float(s))


def am_softmax_n_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gweight) of ``am_softmax_n_forward``; gweight is [D, N].  Unlike Am_softmax's, gx goes back through the row
    normalisation.  ``raw_x_grad``: as in ``margin_backward``."""
    return _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, lambda g, gcos, B, N, st: ops.call(
        "fr_margin_apply_bwd", g, saved.cos, saved.label, None, gcos, None, B, N, cfg.ld, cfg.Np, AM_SOFTMAX, 0, cfg.p0,
        cfg.p1, st)())


def arcneg_thresh32(thresh):
    """The largest fp32 value not above the double ``thresh``.  The reference compares the fp32 target cosine with the
    double cos(pi - margin) (head/metrics.py:427); for every fp32 ``gt``, ``gt > thresh`` in double and ``gt >`` this value in
    fp32 decide alike."""
    t32 = struct.unpack("f", struct.pack("f", float(thresh)))[0]  # rounded to nearest, on the host: no tensor is involved
    if t32 > float(thresh):  # one ulp down: the integer before it in the order of the bit patterns, by sign
        bits = struct.unpack("I", struct.pack("f", t32))[0]
        bits = bits - 1 if t32 > 0 else (0x80000001 if t32 == 0 else bits + 1)
        t32 = struct.unpack("f", struct.pack("I", bits))[0]
    return t32


def arcneg_forward(x, weight, label, s, arc):
    """ArcNegFace logits (head/metrics.py:413-433) for fp32 device tensors; ``weight`` is [N, D], ``arc`` the head's
    (thresh, margin, mm, alpha, sigma).  The reference's loop over the rows, with two host reads per row, is one row kernel:
    every wave reads its row's target cosine gt, derives a (cos(acos(gt) + margin) where gt > thresh, else gt - mm) and
    d a / d gt, writes s * a on the label column and s * (t c + t - 1), t = alpha * exp(-(c - a)^2 / sigma), off it, and
    leaves rowv [3, B] (gt, a, d a / d gt) for the backward pass.  The cosines are never clamped.  Nothing waits on the
    host.  A label outside [0, N) leaves its row at s * c.  Returns (logits, saved, cfg) for ``arcneg_backward``."""
    sv, N, Np, ld, store, logits = _cosine_front(ARCNEG, x, weight, label)
    B = x.shape[0]
    thresh, margin, mm, alpha, sigma = (float(v) for v in arc)
    rowv = torch.empty(3, B, device=x.device)  # gt, a, d a / d gt
    ops.call("fr_arcneg_apply", sv.cos, sv.label, rowv, store, B, N, ld, arcneg_thresh32(thresh), margin, mm, alpha, sigma,
             float(s), ops.current_stream_ptr())()
    return logits, sv._replace(rowv=rowv), HeadCfg(ARCNEG, Np, ld, s=float(s), p0=alpha, p1=sigma)


def arcneg_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gweight) of ``arcneg_forward``; gweight is [N, D].  t and the branch are constants of the graph (:431-432); t is
    recomputed from the saved raw cosines and the row's a; no cosine is masked out (the head never clamps).
    ``raw_x_grad``: as in ``margin_backward``."""
    return _gcos_backward(saved, cfg, g, need_x, need_w, raw_x_grad, lambda g, gcos, B, N, st: ops.call(
        "fr_arcneg_bwd", g, saved.cos, saved.label, saved.rowv, gcos, B, N, cfg.ld, cfg.Np, cfg.p0, cfg.p1, cfg.s, st)())


SST_KINDS = {"am_softmax": 1, "arc_softmax": 2}  # fr_sst_apply's kind; every other loss_type is 0 (head/metrics.py:657-666)

# What an SST_Prototype forward call keeps: x [2B, D] the stacked probe rows, inv_x their reciprocal norms, cos [2B, Q] the
# raw cosines against the whole queue, cw [2B, Rp] those against the stacked gallery rows, gt [D, Rp] the transposed
# normalised gallery rows (Rp = pad(2B, 32), columns >= 2B zero).  SSTCfg.gen: the owner's generation at the call.
SSTSaved = collections.namedtuple("SSTSaved", "x inv_x cos cw gt")
SSTCfg = collections.namedtuple("SSTCfg", "B Q Rp index kind p0 p1 s gen")


def sst_margin(loss_type, margin):
    """(kind, p0, p1) of fr_sst_apply for a head's ``loss_type`` / ``margin``."""
    kind = SST_KINDS.get(loss_type, 0)
    if kind == 2:
        return kind, math.cos(margin), math.sin(margin)
    return kind, (float(margin) if kind == 1 else 0.0), 0.0


def _sst_gemm(st, src, w, out, rows, K, N, ldc, epi=ops.EPI_STORE, splitk=0):
    ops.conv(st, FR_F32, src=src, w=w, out=out, B=rows, RH=1, RW=1, SH=1, SW=1, SC=K, N=N, KH=1, KW=1, stride=1, pad=0,
             mode=0, lda=K, ldc=ldc, pro=0, epi=epi, out_f32=1, splitk=splitk)()


def sst_forward(p, g, ids, q, qt, labels, index, take_g1, kind, p0, p1, s, gen=0):
    """SST_Prototype logits (head/metrics.py:689-708) for fp32 device tensors.  ``p`` [2B, D] is the stacked probe views
    [p1; p2], ``g`` [2B, D] the stacked gallery views [g2; g1] in the order the probe rows meet them, ``ids`` int64 [B];
    ``q`` [D, Q], ``qt`` [Q, D] and ``labels`` [Q] are the module's queue in both layouts and its label buffer, ``index`` the
    window's first column.  Two fr_row_normalize launches (the stacked probes, the stacked galleries, which also leaves
    their transpose), fr_sst_enqueue with the view the coin chose (``take_g1``), the FR_EPI_STORE GEMM of the 2B rows
    against ``qt``, one more against the 2B gallery rows (its two diagonal blocks are p1n . g2n^T and p2n . g1n^T), and
    fr_sst_apply, which takes the window columns from that block.  The queue is neither cloned, normalised nor repacked,
    and nothing waits on the host.  Returns (out [2B, Q]: output1 over output2, saved, cfg) for ``sst_backward``."""
    ops.ptr(p)  # host tensors fail loudly, before anything asks for a device
    R, D = p.shape
    B, Q = R // 2, q.shape[1]
    dev = p.device
    st = ops.current_stream_ptr()
    p = p.contiguous().float()
    g = g.contiguous().float()
    Rp = _pad(R, 32)
    xn = torch.empty(R, D, device=dev)
    inv_x = torch.empty(R, device=dev)
    ops.call("fr_row_normalize", p, xn, None, inv_x, R, R, D, 0, FR_F32, st)()
    gn = torch.empty(Rp, D, device=dev)  # rows >= 2B zero
    gt = torch.empty(D, Rp, device=dev)
    inv_g = torch.empty(R, device=dev)
    ops.call("fr_row_normalize", g, gn, gt, inv_g, R, Rp, D, Rp, FR_F32, st)()
    ops.call("fr_sst_enqueue", gn[B:R] if take_g1 else gn[:B], ids, qt, q, labels, int(index), B, D, Q, st)()
    cos = torch.empty(R, Q, device=dev)
    _sst_gemm(st, xn, qt, cos, R, D, Q, Q)
    cw = torch.empty(R, Rp, device=dev)
    _sst_gemm(st, xn, gn, cw, R, D, R, Rp)
    out = torch.empty(R, Q, device=dev)
    ops.call("fr_sst_apply", cos, cw, out, R, B, Q, Q, Rp, int(index), kind, float(p0), float(p1), float(s), st)()
    return out, SSTSaved(p, inv_x, cos, cw, gt), SSTCfg(B, Q, Rp, int(index), kind, float(p0), float(p1), float(s), gen)


def sst_backward(saved, cfg, g, q):
    """gx [2B, D] of ``sst_forward``: fr_sst_bwd, the split-K data-gradient GEMM of gcos against ``q`` (the queue itself;
    gcos is zero in the window, so the live window's content does not enter), the window's contribution gwin . [g2n; g1n]
    as further slabs, fr_reduce_parts over all slabs in a fixed order, fr_normalize_bwd.  Nothing flows to the gallery rows
    or the queue: no weight-gradient GEMM."""
    R, D = saved.x.shape
    Q, Rp = cfg.Q, cfg.Rp
    dev = saved.x.device
    st = ops.current_stream_ptr()
    gcos = torch.empty(R, Q, device=dev)
    gwin = torch.empty(R, Rp, device=dev)
    ops.call("fr_sst_bwd", g.contiguous().float(), saved.cos, saved.cw, gcos, gwin, R, cfg.B, Q, Q, Q, Rp, cfg.index,
             cfg.kind, cfg.p0, cfg.p1, cfg.s, st)()
    nk = Q // 32
    splitk = max(1, min(nk, 64, nk // 8))
    # the window's GEMM is a handful of workgroups whose time is the length of their K loop (54 us at K = 512 in one
    # slice, profiles/sst_prototype_b256_q16384.txt): slices of four K steps, eight at the most
    wsplit = max(1, min(8, Rp // 128))
    slab = torch.empty(splitk + wsplit, R, D, device=dev)  # K slices and the window's slabs, added in a fixed order
    _sst_gemm(st, gcos, q, slab, R, Q, D, D, ops.EPI_SLAB, splitk)
    _sst_gemm(st, gwin, saved.gt, slab[splitk:], R, Rp, D, D, ops.EPI_SLAB, wsplit)
    G = torch.empty(R, D, device=dev)
    ops.call("fr_reduce_parts", slab, splitk + wsplit, 1, R * D, G, None, None, st)()
    gx = torch.empty(R, D, device=dev)
    ops.call("fr_normalize_bwd", G, saved.x, saved.inv_x, gx, R, D, st)()
    return gx


class SSTHeadFn(torch.autograd.Function):
    """SST_Prototype (head/metrics.py:638-708) on the HIP path; see ``sst_forward``.  ``owner`` is the module: its
    ``_generation`` counts forward calls, and a backward call behind a later forward call raises, since that call overwrote
    another window of the queue this one's data gradient reads."""

    @staticmethod
    def forward(ctx, p, g, ids, q, qt, labels, index, take_g1, kind, p0, p1, s, owner):
        out, saved, cfg = sst_forward(p, g, ids, q, qt, labels, index, take_g1, kind, p0, p1, s, owner._generation)
        ctx.save_for_backward(*saved)
        ctx.cfg, ctx.q, ctx.owner = cfg, q, owner  # q: written through its pointer on every call, so not a saved tensor
        ctx.set_materialize_grads(False)
        # two outputs, not one that the caller slices: the backward of a slice fills and adds a whole [2B, Q] matrix
        return out[:cfg.B], out[cfg.B:]

    @staticmethod
    def backward(ctx, g1, g2):
        if ctx.owner._generation != ctx.cfg.gen:
            raise RuntimeError("SST_Prototype: backward() after a later forward call of the same module -- the queue holds "
                               "one step at a time (%d forward calls since)" % (ctx.owner._generation - ctx.cfg.gen))
        gx = None
        if ctx.needs_input_grad[0] and (g1 is not None or g2 is not None):
            saved = SSTSaved(*ctx.saved_tensors)
            halves = [saved.cos.new_zeros(ctx.cfg.B, ctx.cfg.Q) if h is None else h.float() for h in (g1, g2)]
            g = torch.cat(halves)
            gx = sst_backward(saved, ctx.cfg, g, ctx.q)
        return (gx,) + (None,) * 12


def _row_pitch(t):
    """Floats between the rows of a [B, N] tensor whose rows are dense (one row: its stride says nothing)."""
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def softmax_linear_forward(x, weight, bias):
    """Softmax head logits (head/metrics.py:33, F.linear(x, weight, bias)) for fp32 device tensors; ``weight`` is [N, D],
    ``bias`` [N].  fr_pack_rows lays out the weight as the GEMM's operands ([Np, D], its transpose, the bias with zeros
    behind it) and the fp32 GEMM of the cosine heads adds the bias in its epilogue, once, to the accumulated dot product: no
    pass over [B, N] besides the GEMM's own store.  The GEMM runs over ld = pad(N, 4) columns (zero weight rows, zero bias),
    so the padding columns of the store are written as 0.  Nothing is normalised and nothing waits on the host.  Returns
    (logits, saved, cfg) for ``softmax_linear_backward``."""
    B, D = x.shape
    N = weight.shape[0]
    dev = x.device
    x = x.contiguous().float()
    w = weight.contiguous().float()
    Np, ld = _pad(N, 32), _pad(N, 4)
    wp = torch.empty(Np, D, device=dev)
    wt = torch.empty(D, Np, device=dev)
    bp = torch.empty(Np, device=dev)
    ops.call("fr_pack_rows", w, bias.contiguous().float(), wp, wt, bp, N, Np, D, Np, ops.current_stream_ptr())()
    sv = HeadSaved(x=x, w=w, xn=x, wn=wp, wt=wt)
    store, logits = _logit_store(sv, N, ld)
    _cosine_gemm(sv, store, ld, ld, ops.EPI_STORE, bias=bp)
    return logits, sv._replace(wn=None), HeadCfg(SOFTMAX, Np, ld)


def softmax_linear_backward(saved, cfg, g, need_x, need_w, raw_x_grad=False):
    """(gx, gweight, gbias) of ``softmax_linear_forward``: gx = g W (split-K, the slices added in a fixed order), gweight =
    g^T x, gbias[n] = ((g[0, n] + g[1, n]) + g[2, n]) + ... (fr_col_sums: fp32, the rows in order); ``need_w`` asks for
    both parameter gradients.  ``raw_x_grad`` means what it means elsewhere; nothing is normalised here, so G is gx."""
    B, N = saved.x.shape[0], saved.w.shape[0]
    dev = saved.x.device
    st = ops.current_stream_ptr()
    g = g.float()
    if g.stride(1) != 1 or g.stride(0) < N:  # rows at any pitch are read where they lie (the loss leaves them at ld)
        g = g.contiguous()
    ldg = _row_pitch(g)
    gb = None
    if need_w:
        gb = torch.empty(N, device=dev)
        ops.call("fr_col_sums", g, B, N, ldg, gb, st)()
    gp = torch.empty(B, cfg.Np, device=dev)  # the pitch both gradient GEMMs read, columns N .. Np zero
    ops.call("fr_pad_cols", g, gp, B, N, ldg, cfg.Np, st)()
    return _cosine_backward(saved, cfg, gp, need_x, need_w) + (gb,)


class SoftmaxHeadFn(torch.autograd.Function):
    """logits = x W^T + b (head/metrics.py:12-63) on the HIP path; see ``softmax_linear_forward``."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        logits, saved, cfg = softmax_linear_forward(x, weight, bias)
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg
        return logits

    @staticmethod
    def backward(ctx, g):
        need = ctx.needs_input_grad
        gx, gw, gb = softmax_linear_backward(HeadSaved(*ctx.saved_tensors), ctx.cfg, g, need[0], need[1] or need[2])
        return gx, (gw if need[1] else None), (gb if need[2] else None)


def softmax_head(x, weight, bias):
    """Softmax head logits; the empty batch of ``margin_head`` ([0, N] logits; host tensors still raise)."""
    ops.ptr(x)  # host tensors fail loudly, before anything asks for a device
    if x.shape[0] == 0:
        return x.new_zeros((0, weight.shape[0]), dtype=torch.float32) + 0.0 * (x.sum() + weight.sum() + bias.sum())
    return SoftmaxHeadFn.apply(x, weight, bias)


def _head_fn(name, fwd, bwd, doc):
    """The autograd.Function of a head from its forward / backward pair; it takes the forward function's arguments (x,
    weight, label and up to four head-specific values)."""

    def forward(ctx, x, weight, label, *args):
        logits, saved, cfg = fwd(x, weight, label, *args)
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg
        ctx.mark_non_differentiable(label)
        return logits

    def backward(ctx, g):
        gx, gw = bwd(HeadSaved(*ctx.saved_tensors), ctx.cfg, g, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return gx, gw, None, None, None, None, None

    return type(name, (torch.autograd.Function,),
                {"forward": staticmethod(forward), "backward": staticmethod(backward), "__doc__": doc})


def _head_fn2(name, fwd, bwd, doc):
    """``_head_fn`` for a head with a second output (MagFace's loss_g): ``fwd`` returns (logits, second, saved, cfg), ``bwd``
    takes both upstream gradients, None where an output took no part in the loss."""

    def forward(ctx, x, weight, label, *args):
        logits, second, saved, cfg = fwd(x, weight, label, *args)
        ctx.save_for_backward(*saved)
        ctx.cfg = cfg
        ctx.nargs = len(args)
        ctx.mark_non_differentiable(label)
        ctx.set_materialize_grads(False)
        return logits, second

    def backward(ctx, g, g2):
        gx = gw = None
        if g is not None or g2 is not None:
            gx, gw = bwd(HeadSaved(*ctx.saved_tensors), ctx.cfg, g, g2, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        return (gx, gw, None) + (None,) * ctx.nargs

    return type(name, (torch.autograd.Function,),
                {"forward": staticmethod(forward), "backward": staticmethod(backward), "__doc__": doc})


MarginHeadFn = _head_fn("MarginHeadFn", margin_forward, margin_backward, """
    logits = s * where(j == label, phi(cos), cos),  cos = normalize(x) . normalize(W)^T

    head/metrics.py:97-140 (ArcFace: phi = cos(theta+m) with the cos>th fallback / easy margin) and
    :164-191 (CosFace: phi = cos - m).  Backward per SURVEY.md App. D.""")
MarginExtHeadFn = _head_fn("MarginExtHeadFn", margin_ext_forward, margin_ext_backward, """
    SphereFace (head/metrics.py:236-268) and Am_softmax (:302-331) on the HIP path; see ``margin_ext_forward``.""")
CurricularHeadFn = _head_fn("CurricularHeadFn", curricular_forward, curricular_backward, """
    CurricularFace (head/metrics.py:475-510) on the HIP path; see ``curricular_forward``.""")

AdaCosHeadFn = _head_fn("AdaCosHeadFn", adacos_forward, adacos_backward, """
    AdaCos (head/metrics.py:336-369) on the HIP path; see ``adacos_forward``.""")

NPCFaceHeadFn = _head_fn("NPCFaceHeadFn", npcface_forward, npcface_backward, """
    NPCFace (head/metrics.py:592-636) on the HIP path; see ``npcface_forward``.""")

MVSoftmaxHeadFn = _head_fn("MVSoftmaxHeadFn", mv_softmax_forward, mv_softmax_backward, """
    MV_Softmax (head/metrics.py:555-590) on the HIP path; see ``mv_softmax_forward``.""")

CircleHeadFn = _head_fn("CircleHeadFn", circle_forward, circle_backward, """
    CircleLoss (head/metrics.py:435-473) on the HIP path; see ``circle_forward``.""")

AMSoftmaxNHeadFn = _head_fn("AMSoftmaxNHeadFn", am_softmax_n_forward, am_softmax_n_backward, """
    The FaceX-Zoo AM_Softmax (head/metrics.py:371-392) on the HIP path; see ``am_softmax_n_forward``.""")

ArcNegHeadFn = _head_fn("ArcNegHeadFn", arcneg_forward, arcneg_backward, """
    ArcNegFace (head/metrics.py:394-433) on the HIP path; see ``arcneg_forward``.""")

MagFaceHeadFn = _head_fn2("MagFaceHeadFn", magface_forward, magface_backward, """
    MagFace (head/metrics.py:512-553) on the HIP path: (logits, loss_g); see ``magface_forward``.""")

CHECK_LABELS = True  # host-side range check of the labels (one device sync per call); loops with validated data clear it


def _check_labels(label, n):
    if CHECK_LABELS and (label.min() < 0 or label.max() >= n):  # reference: RuntimeError from scatter_ (metrics.py:134)
        raise RuntimeError("index %d is out of bounds for dimension 1 with size %d" % (int(label.max()), n))


def _head_entry(fn, n, x, weight, label, *args, buf=None):
    """What every head does around its Function: empty batch, label check, the one-float device buffer of a head that has
    one, ``buf`` = (the head function's name, the buffer's argument name, the tensor): CurricularFace's ``t``, AdaCos's
    ``scale``."""
    if x.shape[0] == 0:  # the reference returns empty logits (F.linear / scatter_ on zero rows); nothing to launch
        ops.ptr(x)  # host tensors still fail loudly
        return x.new_zeros((0, n), dtype=torch.float32) + 0.0 * (x.sum() + weight.sum())
    _check_labels(label, n)
    t = None if buf is None else buf[2]
    if t is not None and (t.dtype != torch.float32 or t.numel() != 1 or t.device != x.device or not t.is_contiguous()):
        raise ValueError("%s: %s must be a contiguous float32 tensor of one element on %s" % (buf[:2] + (x.device,)))
    return fn.apply(x, weight, label, *args)


def margin_head(x, weight, label, kind, s, m, easy_margin=False):
    return _head_entry(MarginHeadFn, weight.shape[0], x, weight, label, kind, s, m, easy_margin)


def margin_ext_head(x, weight, label, kind, mi, p0, p1):
    """SphereFace (kind 2) / Am_softmax (kind 3) logits; the empty batch and label check of ``margin_head``."""
    n = weight.shape[0] if kind == SPHEREFACE else weight.shape[1]
    return _head_entry(MarginExtHeadFn, n, x, weight, label, kind, mi, p0, p1)


def curricular_head(x, kernel, label, t, s, m, group=None):
    """CurricularFace logits; the empty batch and label check of ``margin_head``.  ``t`` (float32 [1] on x's device) is
    updated in place; an empty batch leaves it as it is (the reference's mean over no rows turns it into NaN for good)."""
    return _head_entry(CurricularHeadFn, kernel.shape[1], x, kernel, label, t, s, m, group,
                       buf=("curricular_head", "t", t))


def adacos_head(x, W, label, scale, group=None):
    """AdaCos logits; the empty batch and label check of ``margin_head``.  ``scale`` (float32 [1] on x's device) is updated
    in place on every call; an empty batch leaves it as it is (the reference divides by zero rows there)."""
    return _head_entry(AdaCosHeadFn, W.shape[0], x, W, label, scale, group, buf=("adacos_head", "scale", scale))


def npcface_head(x, kernel, label, s, cos_m, sin_m, m0, m1, t, a):
    """NPCFace logits; the empty batch and label check of ``margin_head``."""
    return _head_entry(NPCFaceHeadFn, kernel.shape[1], x, kernel, label, s, (cos_m, sin_m, m0, m1, t, a))


def mv_softmax_head(x, weight, label, s, is_am, p0, p1, w):
    """MV_Softmax logits; the empty batch and label check of ``margin_head``.  p0 = margin with ``is_am``, (p0, p1) =
    (cos_m, sin_m) without; w = mv_weight."""
    return _head_entry(MVSoftmaxHeadFn, weight.shape[1], x, weight, label, s, (is_am, p0, p1, w))


def circle_head(x, weight, label, o_p, o_n, delta_p, delta_n, gamma):
    """CircleLoss logits; the empty batch and label check of ``margin_head``."""
    return _head_entry(CircleHeadFn, weight.shape[1], x, weight, label, (o_p, o_n, delta_p, delta_n, gamma))


def am_softmax_n_head(x, weight, label, m, s):
    """The FaceX-Zoo AM_Softmax logits; the empty batch and label check of ``margin_head``."""
    return _head_entry(AMSoftmaxNHeadFn, weight.shape[1], x, weight, label, m, s)


def arcneg_head(x, weight, label, s, thresh, margin, mm, alpha, sigma):
    """ArcNegFace logits; the empty batch and label check of ``margin_head``.  ``weight`` is [N, D]."""
    return _head_entry(ArcNegHeadFn, weight.shape[0], x, weight, label, s, (thresh, margin, mm, alpha, sigma))


def magface_head(x, kernel, label, s, margin_am, l_a, u_a, l_margin, u_margin, lamda):
    """MagFace (logits [B, N], loss_g [B, 1]); the empty batch and label check of ``margin_head``."""
    out = _head_entry(MagFaceHeadFn, kernel.shape[1], x, kernel, label, s, margin_am, l_a, u_a, l_margin, u_margin, lamda)
    if torch.is_tensor(out):  # the empty batch: [0, N] logits, and no rows of loss_g either
        return out, out[:, :1]
    return out


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


class CrossEntropyFn(torch.autograd.Function):
    """loss = mean_i CE(logits_i, y_i)   -- nn.CrossEntropyLoss() as the reference's LOSS_NAME 'Softmax' builds it
    (train.py:237-238, :300-302).  ``FocalLossFn`` with fr_ce_finalize in place of fr_focal_finalize: the slope it leaves is
    exactly 1, and fr_focal_bwd is the backward kernel unchanged.  Logits that are the [B, N] view of a head's [B, ld] store
    are read at that pitch, and the gradient is laid out alike: no copy of [B, N] on either side."""

    @staticmethod
    def forward(ctx, logits, target):
        B, N = logits.shape
        dev = logits.device
        st = ops.current_stream_ptr()
        logits = logits.float()
        if logits.stride(1) != 1 or logits.stride(0) < N:
            logits = logits.contiguous()
        ld = _row_pitch(logits)
        target = target.contiguous().long()
        lse = torch.empty(B, device=dev)
        ce = torch.empty(B, device=dev)
        rank = torch.empty(B, device=dev, dtype=torch.int32)
        scalars = torch.empty(8, device=dev)
        ops.call("fr_ce_rows", logits, target, lse, ce, rank, B, N, ld, st)()
        ops.call("fr_ce_finalize", ce, rank, B, scalars, st)()
        ctx.save_for_backward(logits, target, lse, scalars)
        return scalars[0].clone()

    @staticmethod
    def backward(ctx, gup):
        logits, target, lse, scalars = ctx.saved_tensors
        B, N = logits.shape
        ld = _row_pitch(logits)
        store = torch.empty(B, ld, device=logits.device)
        gup = gup.contiguous().float().reshape(1)
        ops.call("fr_focal_bwd", logits, target, lse, scalars, gup, store, B, N, ld, ops.current_stream_ptr())()
        return (store if ld == N else store[:, :N]), None


def cross_entropy(logits, target):
    """Batch-mean cross entropy of fp32 device logits.  An empty batch gives NaN, as ``focal_loss`` (the reference's mean
    over no rows); the labels are range-checked under ``CHECK_LABELS``."""
    ops.ptr(logits)  # host tensors fail loudly, before the label check reads anything
    if logits.shape[0] == 0:
        return logits.sum() * float("nan")
    _check_labels(target, logits.shape[1])
    return CrossEntropyFn.apply(logits, target)


def topk_precision(rank, topk):
    """[precision@k in percent for k in topk] from the label ranks (device float32 [len(topk)]); the arithmetic of
    ``(rank < k).float().sum().mul_(100.0 / n)`` (reference util/utils.py:343-358) in one launch."""
    ks = [int(k) for k in topk] + [0] * (4 - len(topk))
    out = torch.empty(len(topk), device=rank.device, dtype=torch.float32)
    ops.call("fr_topk_precision", rank, rank.numel(), len(topk), ks[0], ks[1], ks[2], ks[3], 100.0 / rank.numel(), out,
             ops.current_stream_ptr())()
    return out


def topk_ranks(logits, target):
    """rank[m] = number of classes n with not (z[m][n] <= z[m][label]) (device int32 [B]): those scoring strictly above the
    label's logit, every NaN, and all N of them when the label's logit is NaN or the label lies outside [0, N)."""
    B, N = logits.shape
    if B == 0:
        ops.ptr(logits)
        return torch.empty(0, device=logits.device, dtype=torch.int32)
    st = ops.current_stream_ptr()
    logits = logits.contiguous().float()
    rank = torch.empty(B, device=logits.device, dtype=torch.int32)
    ops.call("fr_rank_rows", logits, target.contiguous().long(), rank, B, N, N, st)()
    return rank
