"""Class-sharded margin head + focal loss: one process per GPU, every rank owns a contiguous range of the classes.

SURVEY.md 8(f) rank 1.  The reference's way to spread a large head is the class-dimension split of
head/metrics.py:104-113 (ArcFace) / :170-179 (CosFace): ONE process chunks ``weight`` over ``device_id`` GPUs, copies
the features to each of them and concatenates the logit chunks back on GPU 0.  The process-per-GPU form of the same
math, with nothing of size [B, N] ever crossing xGMI:

  forward   all-gather features [B,512] and labels -> every rank has the global batch (Bg = world * B rows)
            local logits [Bg, N/world] = margin head on the rank's classes (same HIP kernels as the replicated head;
            rows whose label lives elsewhere select nothing)
            per-row (max, sum exp, label logit) -> ONE all-gather of [3, Bg] floats -> combined in rank order
            -> log-sum-exp, cross entropy; top-k rank of the label = sum over ranks of "local logits above it"
            focal loss on the GLOBAL batch mean, as the reference computes it (one head over the whole DataParallel batch)
  backward  d logits locally (softmax with the global lse) -> weight-shard gradient complete on its owner (NO all-reduce
            of the N x 512 gradient: 57 MB at N = 28 000) and feature gradients summed by reduce-scatter ([Bg,512] in,
            the rank's own [B,512] out) before the normalisation backward.

Against the replicated head this removes the largest gradient bucket from the all-reduce, 1 - 1/world of the head's
weight / momentum / logit memory and FLOPs per GPU, and makes the loss the global-batch focal loss (the replicated
data-parallel step weights each rank's batch-mean separately).

SphereFace, Am_softmax and CurricularFace run the same choreography with one difference each:
  Am_softmax      a [D, N] kernel, sharded by COLUMNS (``class_dim`` 1); x is not normalised, so the reduce-scattered G is gx
  SphereFace      every logit of a row carries ||x||: the radial part of gx is a sum over ALL classes, so its per-row
                  scalar r is summed per shard (fr_shard_sum_parts) and reduce-scattered as [Bg, 1] next to G; lambda
                  follows ``iter``, one per forward call, as in head/metrics.py
  CurricularFace  [D, N] kernel by columns; the target cosine of a row decides which negatives of EVERY shard are hard, so
                  the shards' target cosines (fr_shard_target_cos: 0 where the label lives elsewhere) are all-reduced
                  ([Bg] floats, exact: one owner per label) before the row values; ``t`` then moves by the mean over the
                  global batch, identically on every rank, in a device buffer
Both extra exchanges are [Bg]-sized.

``loss="Softmax"`` (any head): the plain batch-mean cross entropy of the global batch, nn.CrossEntropyLoss() as the
reference's LOSS_NAME 'Softmax' builds it.  The choreography is the same up to the last step, where fr_ce_finalize stands in
for fr_focal_finalize; the slope it leaves is exactly 1, so the backward pass is unchanged.

Head ``Softmax`` (head/metrics.py:12-63, a linear layer with a bias): ``weight`` [N, D] sharded by rows, and a second
parameter ``bias`` [N] sharded alike.  The local logits are x_all W_shard^T + bias_shard; x is not normalised and the
labels play no part in them.  G = g W_shard, reduce-scattered, is gx itself; the gradients of the weight shard and of the
bias shard (the column sums of g over the global batch, the rows in order) are complete on their owner.

Class sampling (``sample_rate`` < 1; Partial-FC, An et al. 2021/22; the reference has no counterpart): in training mode
every rank runs the step above on n_s = ceil(sample_rate * shard size) of its classes -- the classes of its shard that occur
in the global batch, and the non-positive classes with the smallest keys fmix32(global class ^ salt(seed, step)) up to n_s
(fr_class_sample; ``sample_salt``).  The selected weight rows (and bias entries) are gathered, the labels remapped, and
everything from the logits to the two gradient GEMMs sees N = n_s; the gradient rows are scattered back into a dense
gradient of the shard's shape whose other rows are exactly 0.  The optimizer is untouched: an unselected row sees a zero
gradient, so weight decay and momentum still act on it, as under torch.optim.SGD with Partial-FC v2.  The softmax
denominator, the loss and prec@1/@5 then run over the selected classes of all ranks; prec@k is an upper estimate (the label
competes with fewer classes).  Row-sharded heads only (ArcFace, CosFace, SphereFace, Softmax); eval mode runs all classes.

Row-sparse update (``sparse_update=True``, off by default; the lazy update of Partial-FC v1): in a sampled training step
nothing of the shard's shape is formed after the logits either.  The backward pass skips the scatter, returns no gradient
for the weight (and the bias) and leaves ``param._frhip_row_grad = (idx, rows)`` on the parameter: the [n_s, D] output of
the weight-gradient GEMM (the [n_s] column sums for the bias) and the class indices.  ``frhip.optim.SGD.step`` applies
d = rows[j] + wd p[r]; buf[r] = momentum buf[r] + d; p[r] -= lr buf[r] to the rows r = idx[j] in one launch (fr_sgd_rows, the
expression and roundings of the dense step) and clears the attribute.  Rows that were not selected keep their weight and
momentum bits: they see NO weight decay and NO momentum step while unselected, where the dense path above decays them and
moves them along their momentum every step.  That difference is why this is an option; with weight decay 0 and momentum 0
the two coincide bit for bit.  Eval mode, rate 1.0 and a rate whose n_s is the whole shard run the dense path unchanged.

The device arithmetic sits behind ``HipKernels`` (the only implementation in the package: HIP through the C ABI; no
CPU fallback).  tests/ substitutes an oracle-backed stand-in to run the collective choreography at world_size 2 on
``gloo``.
"""
import math

import torch
import torch.distributed as dist
import torch.nn as nn
from torch.nn import Parameter

from . import functional as FRF
from . import ops

KINDS = {"ArcFace": FRF.ARCFACE, "CosFace": FRF.COSFACE, "SphereFace": FRF.SPHEREFACE, "Am_softmax": FRF.AM_SOFTMAX,
         "CurricularFace": FRF.CURRICULAR}
# Consulted after KINDS: the head that is no margin head, a linear layer with a bias (two parameters).
LINEAR_KINDS = {"Softmax": FRF.SOFTMAX}
# the dimension of the parameter that runs over the classes: ``weight`` [N, D] or ``kernel`` [D, N] (head/metrics.py)
CLASS_DIM = {"ArcFace": 0, "CosFace": 0, "SphereFace": 0, "Am_softmax": 1, "CurricularFace": 1, "Softmax": 0}
# (s, m) of each head's own constructor (head/metrics.py); SphereFace has no s, Softmax neither
DEFAULTS = {"ArcFace": (64.0, 0.50), "CosFace": (64.0, 0.50), "SphereFace": (0.0, 4), "Am_softmax": (30.0, 0.35),
            "CurricularFace": (64.0, 0.5), "Softmax": (0.0, 0.0)}
LOSSES = ("Focal", "Softmax")


def class_range(num_classes, world, rank):
    """[lo, hi) of the classes rank ``rank`` owns: contiguous, the first ``num_classes % world`` ranks hold one more."""
    if not 0 <= rank < world:
        raise ValueError("class_range: rank %d outside world of %d" % (rank, world))
    if num_classes < world:
        raise ValueError("class_range: %d classes cannot be split over %d ranks" % (num_classes, world))
    base, rem = divmod(num_classes, world)
    lo = rank * base + min(rank, rem)
    return lo, lo + base + (1 if rank < rem else 0)


def localize_labels(label_all, lo, hi):
    """label - lo where this rank owns the label, -1 elsewhere."""
    own = (label_all >= lo) & (label_all < hi)
    return torch.where(own, label_all - lo, torch.full_like(label_all, -1))


def fmix32(h):
    """The 32-bit finaliser of MurmurHash3, a bijection on uint32 (the key of fr_class_sample)."""
    h &= 0xFFFFFFFF
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & 0xFFFFFFFF
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & 0xFFFFFFFF
    return h ^ (h >> 16)


def sample_salt(seed, step):
    """The salt of training step ``step``: fmix32(seed + 0x9E3779B9 * step) mod 2**32, a host int."""
    return fmix32((int(seed) + 0x9E3779B9 * int(step)) & 0xFFFFFFFF)


def sampled_classes(rate, n):
    """n_s = ceil(rate * n) of a shard of n classes."""
    return min(n, max(1, int(math.ceil(rate * n))))


class Comm(object):
    """The four exchanges of the sharded head; identity when there is one rank."""

    def __init__(self, group=None):
        self.group = group
        self.on = dist.is_available() and dist.is_initialized()
        self.world = dist.get_world_size(group) if self.on else 1
        self.rank = dist.get_rank(group) if self.on else 0
        self.native = self.on and dist.get_backend(group) == "nccl"  # RCCL: reduce-scatter available

    def all_gather(self, t):
        """[n, ...] per rank -> [world * n, ...] in rank order."""
        if not self.on:
            return t
        t = t.contiguous()
        out = t.new_empty((self.world * t.shape[0],) + tuple(t.shape[1:]))
        dist.all_gather_into_tensor(out, t, group=self.group)
        return out

    def reduce_scatter_rows(self, t):
        """[world * n, D] per rank -> sum over ranks of this rank's [n, D] row block."""
        if not self.on:
            return t
        n = t.shape[0] // self.world
        if self.native:
            out = t.new_empty((n,) + tuple(t.shape[1:]))
            dist.reduce_scatter_tensor(out, t.contiguous(), op=dist.ReduceOp.SUM, group=self.group)
            return out
        dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)  # gloo has no reduce-scatter
        return t[self.rank * n:(self.rank + 1) * n].contiguous()

    def all_reduce_sum(self, t):
        if self.on:
            dist.all_reduce(t, op=dist.ReduceOp.SUM, group=self.group)
        return t

    def gather_ragged_rows(self, t, sizes):
        """Row blocks of different heights (the weight shards) -> the stacked tensor on every rank."""
        if not self.on:
            return t
        top = max(sizes)
        pad = t.new_zeros((top,) + tuple(t.shape[1:]))
        pad[:t.shape[0]] = t
        out = self.all_gather(pad).view((self.world, top) + tuple(t.shape[1:]))
        return torch.cat([out[r, :sizes[r]] for r in range(self.world)], 0)


class HipKernels(object):
    """Device arithmetic of the sharded head on the HIP kernels (current stream).  Host tensors raise in ``ops``."""

    def logits(self, x_all, w, label_local, kind, s, m, easy_margin):
        return FRF.margin_forward(x_all, w, label_local, kind, s, m, easy_margin)

    def row_stats(self, logits, label_local):
        rows, n = logits.shape
        stats = torch.empty(3, rows, device=logits.device)
        ops.call("fr_shard_row_stats", logits, label_local, stats, rows, n, logits.stride(0),
                 ops.current_stream_ptr())()
        return stats

    def combine(self, stats_all, world, rows):
        dev = stats_all.device
        lse, ce, tl = (torch.empty(rows, device=dev) for _ in range(3))
        ops.call("fr_shard_combine", stats_all, world, rows, lse, ce, tl, ops.current_stream_ptr())()
        return lse, ce, tl

    def shard_rank(self, logits, tlogit):
        rows, n = logits.shape
        rank = torch.empty(rows, device=logits.device, dtype=torch.int32)
        ops.call("fr_shard_rank_rows", logits, tlogit, rank, rows, n, logits.stride(0), ops.current_stream_ptr())()
        return rank

    def focal(self, ce, rank, gamma):
        scalars = torch.empty(8, device=ce.device)
        ops.call("fr_focal_finalize", ce, rank, ce.shape[0], float(gamma), scalars, ops.current_stream_ptr())()
        return scalars

    def ce(self, ce, rank):
        """``focal`` for loss "Softmax": the batch-mean cross entropy, slope exactly 1."""
        scalars = torch.empty(8, device=ce.device)
        ops.call("fr_ce_finalize", ce, rank, ce.shape[0], scalars, ops.current_stream_ptr())()
        return scalars

    def dlogits(self, logits, label_local, lse, scalars, gup):
        rows, n = logits.shape
        ld = logits.stride(0)  # the logits keep a 16-byte row pitch; the gradient uses the same one
        store = torch.empty(rows, ld, device=logits.device)
        gup = gup.contiguous().float().reshape(1)
        ops.call("fr_focal_bwd", logits, label_local, lse, scalars, gup, store, rows, n, ld,
                 ops.current_stream_ptr())()
        return store if ld == n else store[:, :n]

    def head_bwd(self, saved, cfg, g, need_x, need_w):
        """(G = d loss / d normalize(x_all) from this rank's classes, gradient of the weight shard)."""
        return FRF.margin_backward(saved, cfg, g, need_x, need_w, raw_x_grad=True)

    def normalize_bwd(self, G, x, inv_x):
        gx = torch.empty_like(G)
        ops.call("fr_normalize_bwd", G, x, inv_x, gx, G.shape[0], G.shape[1], ops.current_stream_ptr())()
        return gx

    # SphereFace / Am_softmax / CurricularFace
    def ext_logits(self, x_all, w, label_local, kind, mi, p0, p1):
        return FRF.margin_ext_forward(x_all, w, label_local, kind, mi, p0, p1)

    def target_cos(self, cos, label_local, n, ld):
        """This shard's target cosines [rows]: exactly 0 where another rank owns the label."""
        rows = cos.shape[0]
        tl = torch.empty(rows, device=cos.device)
        ops.call("fr_shard_target_cos", cos, label_local, tl, rows, n, ld, ops.current_stream_ptr())()
        return tl

    def curricular_logits(self, x_all, w, label_local, t, s, m, exchange, train):
        """``exchange``: the shard's target cosines -> those of the global batch (the sum over the ranks); the row values
        and ``t`` (in place, on the device) follow from them by fr_curricular_rows_from inside ``curricular_forward``."""
        return FRF.curricular_forward(x_all, w, label_local, t, s, m,
                                      target_cos=lambda cos, lab, n, ld: exchange(self.target_cos(cos, lab, n, ld)),
                                      train=train)

    def ext_bwd(self, saved, cfg, g, need_x, need_w):
        """(G, gradient of the shard, SphereFace's r_part [rows, parts] or None)."""
        if cfg.kind == FRF.CURRICULAR:
            return FRF.curricular_backward(saved, cfg, g, need_x, need_w, raw_x_grad=True) + (None,)
        return FRF.margin_ext_backward(saved, cfg, g, need_x, need_w, raw_x_grad=True)

    # Softmax
    def linear_logits(self, x_all, w, bias):
        return FRF.softmax_linear_forward(x_all, w, bias)

    def linear_bwd(self, saved, cfg, g, need_x, need_w):
        """(G = g W_shard, gradient of the weight shard, gradient of the bias shard)."""
        return FRF.softmax_linear_backward(saved, cfg, g, need_x, need_w, raw_x_grad=True)

    # class sampling
    def sample_classes(self, label_local, n, n_s, salt, class0):
        """(idx [n_s] int32 ascending, inv [n] int32, label_s [rows] int64) of fr_class_sample; nothing is read back."""
        dev, rows = label_local.device, label_local.shape[0]
        idx = torch.empty(n_s, device=dev, dtype=torch.int32)
        inv = torch.empty(n, device=dev, dtype=torch.int32)
        label_s = torch.empty(rows, device=dev, dtype=torch.int64)
        work = torch.empty(int(ops.lib.fr_class_sample_work(n)), device=dev, dtype=torch.int32)
        ops.call("fr_class_sample", label_local.contiguous(), rows, n, n_s, salt, class0, idx, inv, label_s, work,
                 ops.current_stream_ptr())()
        return idx, inv, label_s

    def gather_rows(self, w, idx):
        """w[idx]: the selected rows of a [n, D] parameter, or the selected entries of a [n] bias."""
        w = w.contiguous()
        out = torch.empty((idx.shape[0],) + tuple(w.shape[1:]), device=w.device)
        ops.call("fr_gather_rows", w, idx, out, idx.shape[0], w.shape[1] if w.dim() == 2 else 1,
                 ops.current_stream_ptr())()
        return out

    def scatter_rows(self, g, inv, n):
        """The dense [n, ...] gradient: row c = g[inv[c]] where inv[c] >= 0, else exactly 0."""
        g = g.contiguous()
        out = torch.empty((n,) + tuple(g.shape[1:]), device=g.device)
        ops.call("fr_scatter_rows", g, inv, out, n, g.shape[1] if g.dim() == 2 else 1, ops.current_stream_ptr())()
        return out

    def sum_r(self, r_part):
        """[rows, 1]: the row's parts added in the order fr_normalize_bwd_radial adds them."""
        rows, nparts = r_part.shape
        r = torch.empty(rows, 1, device=r_part.device)
        ops.call("fr_shard_sum_parts", r_part, nparts, r, rows, ops.current_stream_ptr())()
        return r

    def normalize_bwd_radial(self, G, x, inv_x, r):
        gx = torch.empty_like(G)
        ops.call("fr_normalize_bwd_radial", G, x, inv_x, r, 1, gx, G.shape[0], G.shape[1], ops.current_stream_ptr())()
        return gx


def _leave_row_grad(param, idx, rows):
    """``param._frhip_row_grad = (idx, rows)``: the gradient of the rows ``idx`` of ``param`` and nothing else, for
    ``frhip.optim.SGD.step`` to consume.  Row gradients of two backward passes belong to different index sets and cannot be
    added, so a pending one is an error."""
    if param is None or rows is None:
        return
    if getattr(param, "_frhip_row_grad", None) is not None:
        raise RuntimeError("ShardedMarginLoss(sparse_update=True): a second backward pass before the optimizer consumed the "
                           "row gradient of the first; row gradients of different class samples cannot be added -- call "
                           "optimizer.step() (or zero_grad()) after every backward pass")
    param._frhip_row_grad = (idx, rows)


class ShardedHeadLossFn(torch.autograd.Function):
    """(loss, prec@1, prec@5) of the global batch from this rank's features, labels and weight shard."""

    @staticmethod
    def forward(ctx, x, w, label, head, bias):
        K, C = head.kernels, head.comm
        B = x.shape[0]
        x_loc = x.detach().contiguous().float()
        x_all = C.all_gather(x_loc)
        lab_all = C.all_gather(label.contiguous().long())
        rows = x_all.shape[0]
        lab_loc = localize_labels(lab_all, head.lo, head.hi)
        ctx.sample = ctx.row_idx = None
        if head.step_salt is not None:  # class sampling: from here on the shard is its n_s selected classes
            n = head.hi - head.lo
            idx, inv, lab_loc = K.sample_classes(lab_loc, n, head.n_s, head.step_salt, head.lo)
            w = K.gather_rows(w.detach(), idx)
            if bias is not None:
                bias = K.gather_rows(bias.detach(), idx)
            ctx.sample = (inv, n)
            if head.sparse_update:  # row-sparse update: ``backward`` hands the optimizer the gathered rows and idx
                ctx.row_idx = idx
        if head.kind in (FRF.ARCFACE, FRF.COSFACE):
            logits, saved, cfg = K.logits(x_all, w.detach(), lab_loc, head.kind, head.s, head.m, head.easy_margin)
        elif head.kind == FRF.SPHEREFACE:
            logits, saved, cfg = K.ext_logits(x_all, w.detach(), lab_loc, head.kind, head.m, 1 + head.lamb, 0.0)
        elif head.kind == FRF.AM_SOFTMAX:
            logits, saved, cfg = K.ext_logits(x_all, w.detach(), lab_loc, head.kind, 0, head.m, head.s)
        elif head.kind == FRF.SOFTMAX:
            logits, saved, cfg = K.linear_logits(x_all, w.detach(), bias.detach())
        else:  # one [Bg] all-reduce: every rank gets every row's target cosine, and with them the same t
            logits, saved, cfg = K.curricular_logits(x_all, w.detach(), lab_loc, head.t, head.s, head.m, C.all_reduce_sum,
                                                     head.training)
        stats_all = C.all_gather(K.row_stats(logits, lab_loc).view(1, 3, rows))
        lse, ce, tlogit = K.combine(stats_all, C.world, rows)
        rank = C.all_reduce_sum(K.shard_rank(logits, tlogit))
        scalars = K.focal(ce, rank, head.gamma) if head.loss == "Focal" else K.ce(ce, rank)
        ctx.head, ctx.saved, ctx.cfg = head, saved, cfg
        ctx.rows_of_rank = (C.rank * B, (C.rank + 1) * B)
        ctx.save_for_backward(logits, lab_loc, lse, scalars, x_loc)
        loss, prec1, prec5 = scalars[0].clone(), scalars[2].clone(), scalars[3].clone()
        ctx.mark_non_differentiable(prec1, prec5)
        return loss, prec1, prec5

    @staticmethod
    def backward(ctx, gloss, _g1, _g5):
        head = ctx.head
        K, C = head.kernels, head.comm
        logits, lab_loc, lse, scalars, x_loc = ctx.saved_tensors
        grad = K.dlogits(logits, lab_loc, lse, scalars, gloss)
        r_part = gb = None
        if head.kind in (FRF.ARCFACE, FRF.COSFACE):
            G_all, gw = K.head_bwd(ctx.saved, ctx.cfg, grad, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        elif head.kind == FRF.SOFTMAX:
            G_all, gw, gb = K.linear_bwd(ctx.saved, ctx.cfg, grad, ctx.needs_input_grad[0],
                                         ctx.needs_input_grad[1] or ctx.needs_input_grad[4])
        else:
            G_all, gw, r_part = K.ext_bwd(ctx.saved, ctx.cfg, grad, ctx.needs_input_grad[0], ctx.needs_input_grad[1])
        if ctx.row_idx is not None:  # row-sparse update: the rows stay gathered, no [n, D] gradient is ever formed
            _leave_row_grad(head.weight, ctx.row_idx, gw)
            _leave_row_grad(getattr(head, "bias", None), ctx.row_idx, gb)
            gw = gb = None
        elif ctx.sample is not None:  # back to the shard's shape: the selected rows, exact zeros elsewhere
            inv, n = ctx.sample
            gw = None if gw is None else K.scatter_rows(gw, inv, n)
            gb = None if gb is None else K.scatter_rows(gb, inv, n)
        gx = None
        if G_all is not None:
            G = C.reduce_scatter_rows(G_all)
            lo, hi = ctx.rows_of_rank
            if head.kind in (FRF.AM_SOFTMAX, FRF.SOFTMAX):  # x is not normalised: G is the gradient
                gx = G
            else:
                inv_x = ctx.saved.inv_x[lo:hi].contiguous()
                if head.kind == FRF.SPHEREFACE:  # the radial term sums over all classes: one more [Bg, 1] exchange
                    r = C.reduce_scatter_rows(K.sum_r(r_part))
                    gx = K.normalize_bwd_radial(G, x_loc, inv_x, r)
                else:
                    gx = K.normalize_bwd(G, x_loc, inv_x)
            if head.grad_scale != 1.0:
                gx = gx * head.grad_scale
        return gx, gw, None, None, gb


class ShardedMarginLoss(nn.Module):
    """A head + FocalLoss (or the plain cross entropy) + accuracy, the class dimension sharded over the ranks of ``group``.

        crit = ShardedMarginLoss(512, 28000, "ArcFace", s=64.0, m=0.5, gamma=2)      # after init_process_group
        loss, prec1, prec5 = crit(features, labels)                                   # per-rank features / labels
        loss.backward()                        # crit.weight.grad is final (no all-reduce), features get their gradient

    ``head``: ArcFace, CosFace, SphereFace, Am_softmax, CurricularFace or Softmax; ``s`` / ``m`` default to that head's own
    (head/metrics.py; SphereFace takes ``m`` only, ``easy_margin`` is ArcFace's, Softmax takes neither).  ``loss``: "Focal"
    (``gamma``) or "Softmax", the batch-mean cross entropy of the global batch.

    ``weight`` is this rank's slice of the head's parameter in the head's own layout, ``class_dim`` telling which dimension
    runs over the classes: [hi - lo, in_features] of ``weight`` (ArcFace, CosFace, SphereFace: ``class_dim`` 0) or
    [in_features, hi - lo] of ``kernel`` (Am_softmax, CurricularFace: ``class_dim`` 1).  It is the slice of the tensor the
    replicated head would have drawn from the same RNG state (``full_weight`` given: of that tensor), so the two are
    interchangeable; ``gather_weight()`` returns the reference's parameter (checkpoint key ``weight`` / ``kernel``), and
    ``gather_full`` / ``slice_full`` do the same for any tensor of the parameter's shape (momentum buffers).
    CurricularFace keeps the reference's ``t`` as a one-float buffer (identical on every rank), SphereFace its forward
    counter ``iter``.  Softmax has a second parameter, ``bias``: this rank's [hi - lo] slice of the head's (``full_bias``
    given: of that tensor, else zeros as the head draws it); ``slice_full`` / ``gather_full`` take one-dimensional tensors
    too, and ``gather_bias()`` returns the reference's ``bias``.

    The loss is the focal loss of the GLOBAL batch (head/metrics.py + loss/focal.py applied to the concatenated batch,
    what the reference's single head sees under nn.DataParallel).  ``average_over_ranks=True`` (default) scales the
    feature gradient by the world size so that a backbone whose gradients are AVERAGED over ranks
    (frhip.parallel.DataParallel) ends up with the gradient of that global loss.

    ``sample_rate`` in (0, 1] (row-sharded heads: ArcFace, CosFace, SphereFace, Softmax): below 1, a training step runs on
    n_s = ceil(sample_rate * (hi - lo)) of this rank's classes, every class of the global batch among them, drawn anew each
    step from (``sample_seed``, ``sample_step``); n_s must be at least min(hi - lo, rows of the global batch).  The
    gradients keep the shard's shape, with exact zeros in the unselected rows: the optimizer is untouched, so weight decay
    and momentum still act on those rows, as under torch.optim.SGD with Partial-FC v2.  The softmax denominator, the loss
    and prec@1 / prec@5 run over the selected classes of all ranks, which makes prec@k an upper estimate.  ``sample_step``
    is a host int that counts the training forwards; set it to the step counter when a run is resumed.  In eval mode, and
    at rate 1.0, all classes run on the unsampled path.

    ``sparse_update=True`` (row-sharded heads; acts in a sampled training step only): the lazy update of Partial-FC v1.
    ``backward`` forms no gradient of the shard's shape: ``weight.grad`` (and ``bias.grad``) stay None and the parameter
    carries ``_frhip_row_grad = (idx [n_s] int32, rows [n_s, in_features])`` (``rows`` [n_s] for the bias) until
    ``frhip.optim.SGD.step()`` has applied it to exactly those rows of the parameter and of its momentum buffer, or
    ``zero_grad()`` has dropped it.  Unselected rows keep their weight and momentum bits -- no weight decay and no momentum
    step while unselected, unlike the default path.  A second ``backward`` before the optimizer consumed the first raises
    RuntimeError; ``frhip.optim.Adam`` refuses a row gradient.
    """

    def __init__(self, in_features, out_features, head="ArcFace", s=None, m=None, easy_margin=False, gamma=2.0,
                 group=None, full_weight=None, average_over_ranks=True, kernels=None, loss="Focal", full_bias=None,
                 sample_rate=1.0, sample_seed=0, sparse_update=False):
        super().__init__()
        if not 0.0 < sample_rate <= 1.0:
            raise ValueError("ShardedMarginLoss: sample_rate must lie in (0, 1], got %r" % (sample_rate,))
        if sample_rate < 1.0 and CLASS_DIM.get(head) == 1:
            raise ValueError("ShardedMarginLoss: sample_rate < 1 with head %s: its kernel is [D, N], sharded by columns, and "
                             "the column gather is not built; class sampling serves ArcFace, CosFace, SphereFace and "
                             "Softmax" % head)
        if sparse_update and CLASS_DIM.get(head) == 1:
            raise ValueError("ShardedMarginLoss: sparse_update=True with head %s: its kernel is [D, N], sharded by columns, "
                             "and class sampling does not serve it; the row-sparse update serves ArcFace, CosFace, "
                             "SphereFace and Softmax" % head)
        self.sparse_update = bool(sparse_update)
        if head not in KINDS and head not in LINEAR_KINDS:
            raise ValueError("ShardedMarginLoss: head must be one of %s, got %r"
                             % (", ".join(list(KINDS) + list(LINEAR_KINDS)), head))
        if loss not in LOSSES:
            raise ValueError("ShardedMarginLoss: loss must be one of %s, got %r" % (", ".join(LOSSES), loss))
        self.loss = loss
        self.in_features, self.out_features = in_features, out_features
        self.head_name, self.kind, self.class_dim = head, KINDS.get(head, LINEAR_KINDS.get(head)), CLASS_DIM[head]
        s = DEFAULTS[head][0] if s is None else s
        m = DEFAULTS[head][1] if m is None else m
        self.s, self.easy_margin, self.gamma = float(s), bool(easy_margin), float(gamma)
        self.m = int(m) if self.kind == FRF.SPHEREFACE else float(m)
        self.comm = Comm(group)
        self.kernels = kernels if kernels is not None else HipKernels()
        self.lo, self.hi = class_range(out_features, self.comm.world, self.comm.rank)
        self.grad_scale = float(self.comm.world) if average_over_ranks else 1.0
        # class sampling: n_s of this rank's classes run in a training step; ``sample_step`` counts the training forwards
        # (a host int: the step of the salt) and ``step_salt`` is the salt of the forward in flight, None when all classes run
        self.sample_rate, self.sample_seed, self.sample_step = float(sample_rate), int(sample_seed), 0
        self.n_s = self.hi - self.lo if sample_rate == 1.0 else sampled_classes(self.sample_rate, self.hi - self.lo)
        self.step_salt = None
        self.full_shape = (out_features, in_features) if self.class_dim == 0 else (in_features, out_features)
        if full_weight is None:  # the draw of the replicated head (head/metrics.py), from the same RNG state
            full_weight = torch.empty(self.full_shape)
            if self.kind == FRF.AM_SOFTMAX:
                full_weight.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
            elif self.kind == FRF.CURRICULAR:
                nn.init.normal_(full_weight, std=0.01)
            else:
                nn.init.xavier_uniform_(full_weight)
        if tuple(full_weight.shape) != self.full_shape:
            raise ValueError("ShardedMarginLoss: full_weight must be [%d, %d]" % self.full_shape)
        self.weight = Parameter(self.slice_full(full_weight.detach()).float())
        if self.kind == FRF.SOFTMAX:
            if full_bias is None:
                full_bias = torch.zeros(out_features)
            if tuple(full_bias.shape) != (out_features,):
                raise ValueError("ShardedMarginLoss: full_bias must be [%d]" % out_features)
            self.bias = Parameter(self.slice_full(full_bias.detach()).float())
        if self.kind == FRF.CURRICULAR:
            self.register_buffer("t", torch.zeros(1))
        if self.kind == FRF.SPHEREFACE:  # the lambda schedule of head/metrics.py SphereFace
            self.base, self.lambda_gamma, self.power, self.LambdaMin, self.iter = 1000.0, 0.12, 1, 5.0, 0

    @classmethod
    def from_head(cls, head, gamma=2.0, group=None, **kw):
        """Shard an existing head of head/metrics.py (same parameter on every rank); CurricularFace's ``t``,
        SphereFace's ``iter`` and Softmax's ``bias`` come along."""
        name = head.__class__.__name__
        full = head.kernel if hasattr(head, "kernel") else head.weight
        dims = (full.shape[0], full.shape[1]) if CLASS_DIM.get(name, 0) == 1 else (full.shape[1], full.shape[0])
        if name == "Softmax":
            kw = dict(kw, full_bias=head.bias.detach().cpu())
        crit = cls(dims[0], dims[1], name, s=getattr(head, "s", None), m=getattr(head, "m", None),
                   easy_margin=getattr(head, "easy_margin", False), gamma=gamma, group=group,
                   full_weight=full.detach().cpu(), **kw)
        if hasattr(crit, "t"):
            crit.t.copy_(head.t.detach().cpu())
        if hasattr(crit, "iter"):
            crit.iter = head.iter
        return crit

    def shard_sizes(self):
        return [hi - lo for lo, hi in (class_range(self.out_features, self.comm.world, r)
                                       for r in range(self.comm.world))]

    def slice_full(self, full):
        """This rank's class range of a tensor of the full parameter's shape, or of the bias's [N] (a copy)."""
        return (full[self.lo:self.hi] if self.class_dim == 0 or full.dim() == 1 else full[:, self.lo:self.hi]).clone()

    def gather_full(self, part):
        """Inverse of ``slice_full`` on every rank (collective).  Column shards travel transposed: the ragged gather stacks
        row blocks."""
        if self.class_dim == 0 or part.dim() == 1:
            return self.comm.gather_ragged_rows(part, self.shard_sizes())
        return self.comm.gather_ragged_rows(part.t().contiguous(), self.shard_sizes()).t().contiguous()

    def gather_weight(self):
        """The full parameter on every rank (checkpoints keep the reference's layout)."""
        return self.gather_full(self.weight.detach())

    def gather_bias(self):
        """Softmax: the full ``bias`` on every rank (collective)."""
        return self.gather_full(self.bias.detach())

    def load_full_weight(self, full_weight, full_bias=None):
        with torch.no_grad():
            self.weight.copy_(self.slice_full(full_weight))
            if full_bias is not None:
                self.bias.copy_(self.slice_full(full_bias))

    def forward(self, input, label):
        if self.weight.device != input.device:
            self.to(input.device)
        label = label.to(input.device)
        if FRF.CHECK_LABELS and (label.min() < 0 or label.max() >= self.out_features):  # metrics.py:134 (scatter_)
            raise RuntimeError("index %d is out of bounds for dimension 1 with size %d"
                               % (int(label.max()), self.out_features))
        if self.kind == FRF.SPHEREFACE:  # head/metrics.py:238-239: every forward call counts
            self.iter += 1
            self.lamb = max(self.LambdaMin, self.base * (1 + self.lambda_gamma * self.iter) ** (-1 * self.power))
        self.step_salt = None
        if self.training:
            n, rows = self.hi - self.lo, input.shape[0] * self.comm.world
            if self.n_s < n:
                if self.n_s < min(n, rows):  # every class of the batch must fit: P <= n_s without reading the device
                    raise ValueError("ShardedMarginLoss: sample_rate %g keeps %d of this rank's %d classes, fewer than the "
                                     "%d a global batch of %d rows can hold; the smallest admissible rate here is %g"
                                     % (self.sample_rate, self.n_s, n, min(n, rows), rows, min(n, rows) / float(n)))
                self.step_salt = sample_salt(self.sample_seed, self.sample_step)
            self.sample_step += 1
        return ShardedHeadLossFn.apply(input, self.weight, label, self, getattr(self, "bias", None))

    def __repr__(self):
        return "ShardedMarginLoss(%s, in_features = %d, classes [%d, %d) of %d, s = %s, m = %s, %s)" % (
            self.head_name, self.in_features, self.lo, self.hi, self.out_features, self.s, self.m,
            "gamma = %s" % self.gamma if self.loss == "Focal" else "loss = Softmax")
