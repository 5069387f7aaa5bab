"""Margin-softmax heads with the reference's import path, constructor signatures and state-dict keys.

    from head.metrics import ArcFace, CosFace, SphereFace, Am_softmax        (reference train.py:9)
    from head.metrics import CurricularFace, MagFace, AdaCos, NPCFace        (reference head/metrics.py:475, :512, :336, :592)
    from head.metrics import MV_Softmax                                      (reference head/metrics.py:555)
    from head.metrics import CircleLoss, AM_Softmax                          (reference head/metrics.py:435, :371)
    from head.metrics import ArcNegFace                                      (reference head/metrics.py:394)
    from head.metrics import Softmax                                         (reference head/metrics.py:12)
    from head.metrics import SST_Prototype                                   (reference head/metrics.py:638)

The four heads the reference driver can select (``HEAD_NAME``, train.py:56,178-182) and ``CurricularFace`` / ``MagFace`` /
``AdaCos`` / ``NPCFace`` / ``MV_Softmax`` / ``CircleLoss`` / ``AM_Softmax`` / ``ArcNegFace`` (eight of the FaceX-Zoo heads of the reference's
head/metrics.py that its driver never names; train.py here accepts them) run on the HIP kernels when their input is a device tensor:
  * ``ArcFace`` / ``CosFace`` (the two heads the shipped configs and BASELINE.json name): row normalise -> MFMA cosine
    GEMM with the margin / label-select / scale epilogue -> closed-form backward;
  * ``SphereFace`` / ``Am_softmax``: the same cosine GEMM stores the raw cosines, a row kernel applies the clamp and the
    margin (SphereFace: Chebyshev phi, lambda blend, times ||x||; Am_softmax: c - m on the label, times s), and the
    backward pass reads the raw cosines again for the clamp mask.  Am_softmax normalises the columns of its [in, out]
    ``kernel`` (no eps) and not the embeddings;
  * ``CurricularFace``: rows and ``kernel`` columns normalised, raw cosines from the same GEMM; one workgroup takes the
    per-row target cosine, cos(theta + m), the label column's value and the batch mean, and moves the buffer ``t`` on the
    device (no host read in the step); a row kernel re-weights the negatives above their row's cos(theta + m) by
    ``t + c``; the backward pass treats ``t``, that mask and the branch choice as constants;
  * ``MagFace``: rows and ``weight`` columns normalised, raw cosines from the same GEMM; a row kernel turns each embedding's
    norm into its clamped magnitude a, the margin m(a) (cos, sin, cos(pi - m)), the regulariser ``loss_g`` and the clamp's
    mask; a row kernel applies the per-row margin on the label column.  It returns ``(logits, lamda * loss_g)``.  The
    backward pass adds a radial term r * xhat to the feature gradient: the margin and ``loss_g`` both depend on ||x||;
  * ``AdaCos``: rows of x and of ``W`` normalised, raw cosines from the same GEMM; no margin and no hyper-parameter.  A row
    kernel takes each row's sum of exp(scale * cos) off its label column and its target cosine, one workgroup turns them
    into B_avg and the lower median of the target angles and moves the buffer ``scale`` on the device (no host read in the
    step), and a row kernel multiplies the unclamped cosines by the new scale; the backward pass treats it as a constant;
  * ``NPCFace``: rows and ``kernel`` columns normalised, raw cosines from the same GEMM; one workgroup per row takes the
    target cosine, cos(theta + margin) and, in one more pass over the row, the mean and the count of the hard negatives
    (the cosines above cos(theta + margin), label column excluded; summed in a fixed order), and from them the label
    column's value at the margin ``m0 + m1 * mean``; a row kernel re-weights the hard negatives to ``t * c + a``; the
    backward pass treats that margin, the mask and the ``gt > 0`` branch as constants.  No state besides ``kernel``;
  * ``MV_Softmax``: rows and ``weight`` columns normalised, raw cosines from the same GEMM, never clamped.  One row kernel:
    every wave reads its row's target cosine ``gt``, derives the threshold (``gt - margin`` with ``is_am``, else
    cos(theta + margin)) and the label column's value, and re-weights the hard negatives (the cosines above the threshold)
    to ``mv_weight * c + mv_weight - 1``; the backward pass treats the mask and the branch as constants and masks no
    cosine out.  No state besides ``weight``;
  * ``CircleLoss`` (the classification form): rows and ``weight`` columns normalised, raw cosines from the same GEMM, clamped
    to [-1, 1].  One row kernel, element-wise: ``gamma * alpha_p * (c - delta_p)`` on the label column, ``gamma * alpha_n *
    (c - delta_n)`` off it, with ``alpha_p = max(O_p - c, 0)`` and ``alpha_n = max(c - O_n, 0)`` constants of the graph: a
    negative at or below ``O_n`` has logit 0 and gradient 0.  The kernels keep the reference's fp32 operation order, so on
    the same cosines they give its bits.  No state besides ``weight``;
  * ``AM_Softmax`` (the FaceX-Zoo additive-margin head; not ``Am_softmax``): ``Am_softmax``'s row kernels on the cosines of
    NORMALISED embeddings, parameter ``weight``, margin 0.35 and scale 32 by default, and a feature gradient that goes back
    through the row normalisation.  No state besides ``weight``;
  * ``ArcNegFace``: rows of x and of the [num_class, feat_dim] ``weight`` normalised (no eps), raw cosines from the same
    GEMM, never clamped.  One row kernel: every wave reads its row's target cosine ``gt``, derives ``a`` (cos(theta +
    margin) where ``gt > thresh``, else ``gt - mm``) and writes ``scale * a`` on the label column and ``scale * (t c + t -
    1)``, ``t = alpha * exp(-(c - a)^2 / sigma)``, off it; the backward pass recomputes ``t`` and treats it and the branch
    as constants.  No state besides ``weight``.
  * ``Softmax`` (the plain classification head, ``F.linear(x, weight, bias)``): nothing is normalised.  One kernel lays out
    the weight and the bias as the GEMM's operands, the same fp32 GEMM adds the bias in its epilogue, once, to the
    accumulated dot product; the backward pass is the two gradient GEMMs of the cosine heads without their normalisation
    backwards, and a column-sum kernel that adds the bias gradient over the rows in order.  On host tensors it is
    ``F.linear``.  Parameters ``weight`` and ``bias``.
  * ``SST_Prototype`` (semi-siamese training): no parameter; the class matrix is the buffer ``queue`` of normalised gallery
    embeddings, kept on the device in both GEMM layouts.  Per call: the two stacked probe views and the two stacked gallery
    views are normalised (two launches), one launch writes the chosen gallery view into B columns of both copies of the
    queue and its ids into the label buffer, the same fp32 GEMM gives the raw cosines of the 2B rows against the whole queue
    and, in a small second launch, against the gallery rows that stand in the window; one row kernel clamps, takes the
    window columns from the small GEMM, applies the label column's margin (``am_softmax`` / ``arc_softmax``) and the scale in
    the reference's fp32 operation order.  The queue is never cloned, normalised or repacked, nothing waits on the host, and
    the backward pass is one row kernel, the split-K data-gradient GEMM against ``queue`` itself plus a few slabs for the
    window, and the row normalisation's backward: nothing flows to the gallery rows or the queue.  On host tensors it is the
    reference's arithmetic written out of place.
On host tensors ``SphereFace`` / ``Am_softmax`` / ``CurricularFace`` / ``MagFace`` / ``AdaCos`` / ``NPCFace`` / ``MV_Softmax`` /
``CircleLoss`` / ``AM_Softmax`` / ``ArcNegFace`` run the reference's plain-PyTorch arithmetic (the
restatement the tests compare with); ``ArcFace`` / ``CosFace`` refuse host tensors.  ``SphereFace.iter`` counts forward
calls on either path, as in the reference; train.py carries it across a resume in the State_* file.  ``CurricularFace.t``
is a buffer: the Head_* file carries it.  ``AdaCos.scale`` is a non-persistent buffer (the reference's Head_* files have the
key ``W`` alone): train.py carries it in the State_* file.

Differences from the reference that a caller can observe:
  * ``device_id`` is accepted for signature compatibility but the class-dimension ``.cuda(i)`` split of
    head/metrics.py:104-113 is not reproduced: one process drives one GPU and the whole weight lives there
    (data parallelism is one process per GPU over RCCL, see frhip/parallel.py).
  * the reference's ArcFace allocates its one-hot on ``'cuda'`` unconditionally (metrics.py:133) and takes an
    optional ``onehot_vec``; here the label select happens inside the GEMM epilogue (bit-exact equivalent of
    the blend for finite values), ``onehot_vec`` is accepted and ignored.
  * ``CurricularFace`` on the device path divides the kernel's columns by their norm without the eps = 1e-12 of the
    reference's ``F.normalize(kernel, dim=0)``: a column of norm below 1e-12 is out of contract.  A target cosine of
    exactly +-1 makes the reference's own gradient infinite (sin_m * tl / sqrt(1 - tl^2)); nothing is done about it here
    either.  An empty batch leaves ``t`` as it is (the reference's mean over no rows makes it NaN for good).
  * ``MagFace`` on the device path: the same two limits (no eps on the ``weight`` columns, a target cosine of exactly +-1).
    The label select is a ``where`` on the label column, so negatives at a cosine of exactly +-1 get a finite gradient
    (the reference's sqrt(1 - c^2) over the whole matrix makes theirs NaN).
  * ``AdaCos.scale`` is a one-element float tensor (a non-persistent buffer) from construction on; the reference starts
    with a Python float and turns it into a 0-dim tensor on the first call.  ``float(head.scale)`` works on both.  ``.double()``
    converts the fp32 initial value, so a float64 copy starts 3e-8 (relative) from the reference's.  An empty
    batch leaves ``scale`` as it is, where the reference divides by zero rows.  Limits as in the reference: a ``W`` row of
    norm below 1e-12 is out of contract, ``scale * cos`` above about 88 overflows exp in fp32, and ``num_classes < 3`` is
    degenerate (the initial scale is 0 or -inf).
  * ``NPCFace`` on the device path: the same two limits as ``CurricularFace`` (no eps on the ``kernel`` columns: a column of
    norm below 1e-12 is out of contract; a target cosine of exactly +-1 makes the reference's own gradient infinite, and
    nothing is done about it here either).  The reference builds its hard mask with ``.cuda()`` (:622) and so runs on no
    other device; the host path here leaves that call out and is otherwise its arithmetic.
  * ``MV_Softmax``: the host path is the reference's arithmetic out of place (the reference writes into its cosine matrix).
    Limits, followed as in the reference: on the device path a ``weight`` column of norm below 1e-12 is out of contract (no
    eps); with ``is_am`` false a target cosine of exactly +-1 makes the reference's own gradient infinite, and a target
    cosine beyond +-1 by rounding (the head never clamps) makes sqrt(1 - gt^2) and with it the threshold NaN: then no
    negative of the row is hard, the label column is NaN where ``gt > 1`` and keeps ``gt`` where ``gt < -1`` (gradient 1 on
    the device path).  The device path computes the same expressions unguarded.
  * ``CircleLoss`` / ``AM_Softmax``: the host path is the reference's arithmetic out of place (the reference writes into a
    copy of its cosine matrix through uint8 masks); on the device path a ``weight`` column of norm below 1e-12 is out of
    contract (no eps), as with the siblings.  A NaN cosine gives a NaN logit and gradient 0 on both paths (torch.clamp
    lets NaN through and passes no gradient there).
  * ``ArcNegFace``: the reference fills its logits in a Python loop over the rows with two ``.item()`` host reads per row;
    here neither path has a per-row loop or a host read, and the host path is a vectorised, out-of-place restatement that
    gives the reference's fp32 logits bit for bit.  A label outside [0, N) raises through the shared label check on both
    paths, where the reference's Python indexing would wrap -1 to the last class.  A ``weight`` row or an embedding of norm
    below 1e-12 is out of contract (no eps, as in the reference).  The cosines are never clamped, as in the reference: a raw
    target cosine above 1 by rounding (1 + 2^-23) makes acos NaN, and with it ``a``, every ``t`` of the row and so the
    whole row of logits and gradients; a target cosine of exactly +1 makes the reference's own gradient infinite, and
    nothing is done about it here either; a raw negative beyond +-1 keeps its value and its gradient ``scale * t``.
  * ``SST_Prototype``: ``label`` is an int64 tensor of shape [B] on the embeddings' device, also for B = 1 (the reference's
    ``squeeze`` makes it 0-dim there) and without the reference's unconditional ``.cuda()`` (:696).  ``label_list`` is a
    property that reads the buffer ``labels`` (int64, non-persistent) on demand, and on the device path the fourth returned
    value is a ``collections.abc.Set`` over a device clone of it that materialises on first use; it compares equal to the
    reference's ``set``.  A window that would run past the queue (``index + B > queue_size``) raises ``RuntimeError`` on
    both paths before any state is touched and before the coin is drawn, where the reference raises at its slice
    assignment after it has computed the logits.  The device path needs ``queue_size % 32 == 0`` (``NotImplementedError``
    otherwise; the host path serves any size) and fp32.  A backward call behind a later forward call of the same module
    raises: the queue holds one step at a time.  The host path replaces ``queue`` by a new tensor on every call instead of
    writing into it.  With ``arc_softmax`` a target cosine of exactly +-1 makes the reference's own gradient infinite, and
    nothing is done about it here either.  ``queue_state()`` / ``load_queue_state()`` are additions for a driver's state
    file; the state dict stays the reference's (``queue`` alone).
"""
import collections.abc
import math
import random

import torch
import torch.distributed as dist
import torch.nn as nn
import torch.nn.functional as F
from torch.nn import Parameter

from frhip import functional as FRF


def _beside(module, param, input):
    """The reference keeps HEAD on the host and copies W every step (train.py never calls HEAD.to); here the module is
    moved once, next to the features."""
    if param.device != input.device:
        module.to(input.device)


class _MarginHead(nn.Module):
    _kind = 0

    def __init__(self, in_features, out_features, device_id, s, m):
        super().__init__()
        self.in_features = in_features
        self.out_features = out_features
        self.device_id = device_id
        self.s = s
        self.m = m
        self.weight = Parameter(torch.empty(out_features, in_features))
        nn.init.xavier_uniform_(self.weight)  # metrics.py:87-88 / :163-164

    def _logits(self, input, label, easy_margin=False):
        _beside(self, self.weight, input)
        return FRF.margin_head(input, self.weight, label.to(input.device), self._kind, self.s, self.m, easy_margin)

    def __repr__(self):
        return "%s(in_features = %d, out_features = %d, s = %s, m = %s)" % (
            self.__class__.__name__, self.in_features, self.out_features, self.s, self.m)


class Softmax(nn.Module):
    """The plain classification head, a linear layer with a bias (reference head/metrics.py:12-63): HIP kernels on device
    tensors, ``F.linear`` on the host.  The reference's ``forward(x)`` cannot be called by its own train.py, which passes the
    labels too (train.py:300); they are accepted and ignored."""

    def __init__(self, in_features, out_features, device_id):
        super().__init__()
        self.in_features, self.out_features, self.device_id = in_features, out_features, device_id
        self.weight = Parameter(torch.empty(out_features, in_features))
        self.bias = Parameter(torch.empty(out_features))
        nn.init.xavier_uniform_(self.weight)  # metrics.py:28-29
        nn.init.zeros_(self.bias)

    def forward(self, x, label=None):
        if x.is_cuda:
            _beside(self, self.weight, x)
            return FRF.softmax_head(x, self.weight, self.bias)
        return F.linear(x, self.weight.to(x.device), self.bias.to(x.device))

    def __repr__(self):
        return "Softmax(in_features = %d, out_features = %d)" % (self.in_features, self.out_features)


class ArcFace(_MarginHead):
    """cos(theta + m) margin -- reference head/metrics.py:66-140."""
    _kind = 0

    def __init__(self, in_features, out_features, device_id, s=64.0, m=0.50, easy_margin=False):
        super().__init__(in_features, out_features, device_id, s, m)
        self.easy_margin = easy_margin
        self.cos_m = math.cos(m)
        self.sin_m = math.sin(m)
        self.th = math.cos(math.pi - m)
        self.mm = math.sin(math.pi - m) * m
        self.eps = 1e-10

    def forward(self, input, label, onehot_vec=None):
        return self._logits(input, label, self.easy_margin)


class CosFace(_MarginHead):
    """cos(theta) - m margin, default m = 0.50 as in the reference (head/metrics.py:143-191, :155)."""
    _kind = 1

    def __init__(self, in_features, out_features, device_id, s=64.0, m=0.50):
        super().__init__(in_features, out_features, device_id, s, m)

    def forward(self, input, label):
        return self._logits(input, label)


class SphereFace(nn.Module):
    """cos(m*theta) head (reference head/metrics.py:200-277): HIP kernels on device tensors, plain PyTorch on the host."""

    def __init__(self, in_features, out_features, device_id, m=4):
        super().__init__()
        self.in_features, self.out_features, self.device_id, self.m = in_features, out_features, device_id, m
        self.base, self.gamma, self.power, self.LambdaMin, self.iter = 1000.0, 0.12, 1, 5.0, 0
        self.weight = Parameter(torch.empty(out_features, in_features))
        nn.init.xavier_uniform_(self.weight)

    @staticmethod
    def _cheb(m, c):
        return {0: lambda x: x ** 0, 1: lambda x: x, 2: lambda x: 2 * x ** 2 - 1, 3: lambda x: 4 * x ** 3 - 3 * x,
                4: lambda x: 8 * x ** 4 - 8 * x ** 2 + 1, 5: lambda x: 16 * x ** 5 - 20 * x ** 3 + 5 * x}[m](c)

    def forward(self, input, label):
        self.iter += 1
        self.lamb = max(self.LambdaMin, self.base * (1 + self.gamma * self.iter) ** (-1 * self.power))
        if input.is_cuda:
            _beside(self, self.weight, input)
            return FRF.margin_ext_head(input, self.weight, label.to(input.device), FRF.SPHEREFACE, self.m,
                                       1 + self.lamb, 0.0)
        w = self.weight.to(input.device)
        c = F.linear(F.normalize(input), F.normalize(w)).clamp(-1, 1)
        k = (self.m * c.detach().acos() / 3.14159265).floor()
        phi = ((-1.0) ** k) * self._cheb(self.m, c) - 2 * k
        hot = torch.zeros_like(c).scatter_(1, label.view(-1, 1), 1)
        out = hot * (phi - c) / (1 + self.lamb) + c
        return out * input.norm(2, 1).view(-1, 1)


class Am_softmax(nn.Module):
    """Additive-margin softmax with a [in, out] ``kernel`` (reference head/metrics.py:287-333): HIP kernels on device
    tensors, plain PyTorch on the host."""

    def __init__(self, in_features, out_features, device_id, m=0.35, s=30.0):
        super().__init__()
        self.in_features, self.out_features, self.device_id, self.m, self.s = in_features, out_features, device_id, m, s
        self.kernel = Parameter(torch.empty(in_features, out_features))
        self.kernel.data.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)

    def forward(self, embbedings, label):
        if embbedings.is_cuda:
            _beside(self, self.kernel, embbedings)
            return FRF.margin_ext_head(embbedings, self.kernel, label.to(embbedings.device), FRF.AM_SOFTMAX, 0,
                                       self.m, self.s)
        kn = self.kernel.to(embbedings.device)
        c = torch.mm(embbedings, kn / kn.norm(2, 0, True)).clamp(-1, 1)
        hot = torch.zeros_like(c).scatter_(1, label.view(-1, 1), 1).bool()
        return torch.where(hot, c - self.m, c) * self.s


class CurricularFace(nn.Module):
    """CurricularFace (reference head/metrics.py:475-510): HIP kernels on device tensors, plain PyTorch on the host.

    ``t`` moves on every forward call, training or not, as in the reference, and the updated value is the one the call uses.
    ``process_group``: the reference's nn.DataParallel shows one head the global batch; with one replica per rank, set this
    to the ranks' group and the batch mean of the target cosines is averaged over it before it enters ``t`` (one float, a
    device tensor on the device path), so every rank holds the ``t`` of a single head over the concatenated batch.  That
    takes equal batch sizes on every rank (DROP_LAST).  Limits: see the module docstring (kernel columns of norm below
    1e-12; target cosines of exactly +-1)."""

    def __init__(self, feat_dim, num_class, m=0.5, s=64.):
        super().__init__()
        self.m, self.s = m, s
        self.cos_m, self.sin_m = math.cos(m), math.sin(m)
        self.threshold = math.cos(math.pi - m)
        self.mm = math.sin(math.pi - m) * m
        self.kernel = Parameter(torch.empty(feat_dim, num_class))
        self.register_buffer('t', torch.zeros(1))
        nn.init.normal_(self.kernel, std=0.01)
        self.process_group = None

    def forward(self, feats, labels):
        if feats.is_cuda:
            _beside(self, self.kernel, feats)
            return FRF.curricular_head(feats, self.kernel, labels.to(feats.device), self.t, self.s, self.m,
                                       self.process_group)
        kernel = self.kernel.to(feats.device)
        c = torch.mm(F.normalize(feats), F.normalize(kernel, dim=0)).clamp(-1, 1)
        at = labels.view(-1, 1).long()
        tl = c.gather(1, at)
        ctm = tl * self.cos_m - torch.sqrt(1.0 - torch.pow(tl, 2)) * self.sin_m  # cos(theta_target + m)
        final = torch.where(tl > self.threshold, ctm, tl - self.mm)
        if tl.numel():
            with torch.no_grad():
                mean = tl.mean()
                if self.process_group is not None:
                    dist.all_reduce(mean, group=self.process_group)
                    mean = mean / dist.get_world_size(self.process_group)
                self.t = mean * 0.01 + (1 - 0.01) * self.t
        hard = (c > ctm).detach()
        out = torch.where(hard, c * (self.t + c), c).scatter(1, at, final)
        return out * self.s


class MagFace(nn.Module):
    """MagFace (reference head/metrics.py:512-553): HIP kernels on device tensors, plain PyTorch on the host.

    Returns ``(logits, lamda * loss_g)``, loss_g [B, 1] = a / u_a^2 + 1 / a with a = clamp(||x||, l_a, u_a); the margin on
    the label column is m(a), linear from l_margin at l_a to u_margin at u_a.  train.py adds ``loss_g.mean()`` to the loss."""

    def __init__(self, feat_dim, num_class, margin_am=0.0, scale=32, l_a=10, u_a=110, l_margin=0.45, u_margin=0.8, lamda=20):
        super().__init__()
        self.weight = Parameter(torch.empty(feat_dim, num_class))
        self.weight.data.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
        self.margin_am, self.scale, self.l_a, self.u_a = margin_am, scale, l_a, u_a
        self.l_margin, self.u_margin, self.lamda = l_margin, u_margin, lamda

    def calc_margin(self, x):
        return (self.u_margin - self.l_margin) / (self.u_a - self.l_a) * (x - self.l_a) + self.l_margin

    def forward(self, feats, labels):
        if feats.is_cuda:
            _beside(self, self.weight, feats)
            return FRF.magface_head(feats, self.weight, labels.to(feats.device), self.scale, self.margin_am, self.l_a,
                                    self.u_a, self.l_margin, self.u_margin, self.lamda)
        weight = self.weight.to(feats.device)
        a = torch.norm(feats, dim=1, keepdim=True).clamp(self.l_a, self.u_a)
        m = self.calc_margin(a)
        loss_g = 1 / (self.u_a ** 2) * a + 1 / a
        c = torch.mm(F.normalize(feats), F.normalize(weight, dim=0)).clamp(-1, 1)
        at = labels.view(-1, 1).long()
        tl = c.gather(1, at)
        ctm = tl * torch.cos(m) - torch.sqrt(1.0 - torch.pow(tl, 2)) * torch.sin(m)  # cos(theta_target + m(a))
        final = torch.where(tl > torch.cos(math.pi - m), ctm, tl - self.margin_am)
        return c.scatter(1, at, final) * self.scale, self.lamda * loss_g


class AdaCos(nn.Module):
    """AdaCos (reference head/metrics.py:336-369): HIP kernels on device tensors, plain PyTorch on the host.

    No margin and no hyper-parameter: ``scale <- log(B_avg) / cos(min(pi/4, median(theta_target)))`` with ``B_avg = (1/B)
    sum_i sum_{j != y_i} exp(scale_old * cos_ij)`` on every forward call -- training mode, eval mode and under no_grad, as in
    the reference -- and the logits are the new scale times the unclamped cosines.  ``torch.median`` of an even count is the
    LOWER of the two middle values.  ``scale`` is a non-persistent one-float buffer: it follows ``.to()`` / ``.double()``
    and stays out of the state dict, whose only key is ``W``.
    ``process_group``: as on ``CurricularFace``, set it to the ranks' group and the statistics are those of one head over the
    concatenated batch of all ranks (B_avg over world * B rows, the median over all ranks' target angles): each rank
    all-gathers a [2, B] tensor of per-row sums and target cosines and reduces the gathered rows in rank order, so every rank
    holds the same bits.  That takes equal batch sizes on every rank (DROP_LAST).
    Limits, none worked around: a ``W`` row of norm below 1e-12 is out of contract; ``scale_old * cos`` above about 88
    overflows exp in fp32, exactly as in the reference; ``num_classes < 3`` is degenerate (the initial scale is 0 or -inf);
    an empty batch, or (device path) one in which no row has a label in [0, N), leaves ``scale`` unchanged where the
    reference raises or produces NaN."""

    def __init__(self, feat_dim, num_classes):
        super().__init__()
        s0 = math.sqrt(2) * math.log(num_classes - 1) if num_classes > 1 else float("-inf")
        self.register_buffer("scale", torch.full((1,), s0), persistent=False)
        self.W = Parameter(torch.empty(num_classes, feat_dim))
        nn.init.xavier_uniform_(self.W)
        self.process_group = None

    def forward(self, feats, labels):
        if feats.is_cuda:
            _beside(self, self.W, feats)
            return FRF.adacos_head(feats, self.W, labels.to(feats.device), self.scale, self.process_group)
        logits = F.linear(F.normalize(feats), F.normalize(self.W.to(feats.device)))
        if logits.shape[0]:
            with torch.no_grad():
                one_hot = torch.zeros_like(logits).scatter_(1, labels.view(-1, 1).long(), 1)
                e = torch.where(one_hot < 1, torch.exp(self.scale * logits), torch.zeros_like(logits))
                tc = logits[one_hot == 1]
                if self.process_group is None:
                    b_avg = torch.sum(e) / logits.size(0)
                else:  # one head over the concatenated batch: gather (row sums, target cosines), reduce in rank order
                    mine = torch.stack([e.sum(1), tc])
                    every = [torch.empty_like(mine) for _ in range(dist.get_world_size(self.process_group))]
                    dist.all_gather(every, mine, group=self.process_group)
                    every = torch.cat(every, 1)
                    b_avg, tc = torch.sum(every[0]) / every.shape[1], every[1]
                theta_med = torch.median(torch.acos(torch.clamp(tc, -1.0 + 1e-7, 1.0 - 1e-7)))
                new = torch.log(b_avg) / torch.cos(torch.min(math.pi / 4 * torch.ones_like(theta_med), theta_med))
                self.scale = new.to(self.scale.dtype).view(1)
        return self.scale * logits


class NPCFace(nn.Module):
    """NPCFace (reference head/metrics.py:592-636): HIP kernels on device tensors, plain PyTorch on the host.

    The margin on the label column follows the row's hard negatives: ``newm = m0 + m1 * mean(c | c > cos(theta + margin),
    label column excluded)``, with the count clamped at 1, so a row without hard negatives gets ``m0``.  Hard negatives
    become ``t * c + a``.  ``newm``, the mask and the ``gt > 0`` branch take no gradient.  The constants are plain
    attributes read on every call (``cos_m`` / ``sin_m``, not ``margin``, as in the reference); the state dict holds the key
    ``kernel`` alone.  Limits: see the module docstring (kernel columns of norm below 1e-12; target cosines of exactly +-1)."""

    def __init__(self, feat_dim=512, num_class=86876, margin=0.5, scale=64):
        super().__init__()
        self.kernel = Parameter(torch.empty(feat_dim, num_class))
        self.kernel.data.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
        self.margin, self.scale = margin, scale
        self.cos_m, self.sin_m = math.cos(margin), math.sin(margin)
        self.m0, self.m1, self.t, self.a = 0.40, 0.20, 1.10, 0.20
        self.cos_m0, self.sin_m0 = math.cos(self.m0), math.sin(self.m0)
        self.num_class = num_class

    def forward(self, x, label):
        if x.is_cuda:
            _beside(self, self.kernel, x)
            return FRF.npcface_head(x, self.kernel, label.to(x.device), self.scale, self.cos_m, self.sin_m, self.m0,
                                    self.m1, self.t, self.a)
        kernel = self.kernel.to(x.device)
        c = torch.mm(F.normalize(x), F.normalize(kernel, dim=0)).clamp(-1, 1)
        at = label.view(-1, 1).long()
        gt = c.gather(1, at)
        sin_theta = torch.sqrt(1.0 - torch.pow(gt, 2))
        ctm = gt * self.cos_m - sin_theta * self.sin_m  # cos(theta_target + margin)
        with torch.no_grad():
            hard = (c > ctm).to(c.dtype).scatter_(1, at, 0)
            sum_hard = torch.where(hard > 0, c, torch.zeros_like(c)).sum(1, keepdim=True)
            newm = self.m0 + self.m1 * (sum_hard / hard.sum(1, keepdim=True).clamp(1, self.num_class))
            cos_newm, sin_newm = torch.cos(newm), torch.sin(newm)
        final = torch.where(gt > 0, gt * cos_newm - sin_theta * sin_newm, gt)
        out = torch.where(c > ctm, self.t * c + self.a, c).scatter(1, at, final)
        return out * self.scale


class MV_Softmax(nn.Module):
    """MV_Softmax, "Mis-classified Vector Guided Softmax" (reference head/metrics.py:555-590): HIP kernels on device tensors,
    plain PyTorch on the host.

    With ``gt`` a row's target cosine: ``is_am`` true gives the threshold ``gt - margin`` and the label column
    ``gt - margin`` where ``gt > margin`` (else ``gt``); ``is_am`` false gives cos(theta + margin) from ``cos_m`` /
    ``sin_m`` (not from ``margin``) for both, the label column where ``gt > 0`` (else ``gt``).  Negatives above the threshold
    become ``mv_weight * c + mv_weight - 1``; the mask and the branch take no gradient, and no cosine is clamped.  All
    attributes are plain and read on every call (``threshold`` and ``mm`` are the reference's, unused there too); the state
    dict holds the key ``weight`` alone.  Limits: see the module docstring."""

    def __init__(self, feat_dim, num_class, is_am, margin=0.35, mv_weight=1.12, scale=32):
        super().__init__()
        self.weight = Parameter(torch.empty(feat_dim, num_class))
        self.weight.data.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
        self.margin = margin
        self.mv_weight = mv_weight
        self.scale = scale
        self.is_am = is_am
        self.cos_m = math.cos(margin)
        self.sin_m = math.sin(margin)
        self.threshold = math.cos(math.pi - margin)
        self.mm = self.sin_m * margin

    def forward(self, x, label):
        if x.is_cuda:
            _beside(self, self.weight, x)
            p0, p1 = (self.margin, 0.0) if self.is_am else (self.cos_m, self.sin_m)
            return FRF.mv_softmax_head(x, self.weight, label.to(x.device), self.scale, bool(self.is_am), p0, p1,
                                       self.mv_weight)
        weight = self.weight.to(x.device)
        c = torch.mm(F.normalize(x), F.normalize(weight, dim=0))
        at = label.view(-1, 1).long()
        gt = c.gather(1, at)
        if self.is_am:
            thr = gt - self.margin
            final = torch.where(gt > self.margin, gt - self.margin, gt)
        else:
            sin_theta = torch.sqrt(1.0 - torch.pow(gt, 2))
            thr = gt * self.cos_m - sin_theta * self.sin_m  # cos(theta_target + margin)
            final = torch.where(gt > 0.0, thr, gt)
        out = torch.where(c > thr, self.mv_weight * c + self.mv_weight - 1.0, c).scatter(1, at, final)
        return out * self.scale


class CircleLoss(nn.Module):
    """CircleLoss, the classification form (reference head/metrics.py:435-473): HIP kernels on device tensors, plain PyTorch on
    the host.

    On the clamped cosines: ``gamma * alpha_p * (c - delta_p)`` on the label column and ``gamma * alpha_n * (c - delta_n)``
    off it, ``alpha_p = clamp_min(O_p - c, 0)`` and ``alpha_n = clamp_min(c - O_n, 0)`` detached.  ``O_p``, ``O_n``,
    ``delta_p``, ``delta_n`` and ``gamma`` are plain attributes read on every call (``margin`` is kept and, after
    construction, not read, as in the reference); the state dict holds the key ``weight`` alone."""

    def __init__(self, feat_dim, num_class, margin=0.25, gamma=256):
        super().__init__()
        self.weight = Parameter(torch.empty(feat_dim, num_class))
        self.weight.data.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
        self.margin = margin
        self.gamma = gamma
        self.O_p = 1 + margin
        self.O_n = -margin
        self.delta_p = 1 - margin
        self.delta_n = margin

    def forward(self, feats, labels):
        if feats.is_cuda:
            _beside(self, self.weight, feats)
            return FRF.circle_head(feats, self.weight, labels.to(feats.device), self.O_p, self.O_n, self.delta_p,
                                   self.delta_n, self.gamma)
        weight = self.weight.to(feats.device)
        c = torch.mm(F.normalize(feats), F.normalize(weight, dim=0)).clamp(-1, 1)
        hot = torch.zeros_like(c).scatter_(1, labels.view(-1, 1).long(), 1).bool()
        alpha_p = torch.clamp_min(self.O_p - c.detach(), min=0.)
        alpha_n = torch.clamp_min(c.detach() - self.O_n, min=0.)
        return torch.where(hot, alpha_p * (c - self.delta_p), alpha_n * (c - self.delta_n)) * self.gamma


class AM_Softmax(nn.Module):
    """The FaceX-Zoo additive-margin softmax (reference head/metrics.py:371-392; not ``Am_softmax``, :287-333): HIP kernels on
    device tensors, plain PyTorch on the host.

    ``scale * (c - margin)`` on the label column and ``scale * c`` off it, c the clamped cosine between the NORMALISED
    embedding and the normalised ``weight`` column.  ``margin`` and ``scale`` are plain attributes read on every call; the
    state dict holds the key ``weight`` alone."""

    def __init__(self, feat_dim, num_class, margin=0.35, scale=32):
        super().__init__()
        self.weight = Parameter(torch.empty(feat_dim, num_class))
        self.weight.data.uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
        self.margin = margin
        self.scale = scale

    def forward(self, feats, labels):
        if feats.is_cuda:
            _beside(self, self.weight, feats)
            return FRF.am_softmax_n_head(feats, self.weight, labels.to(feats.device), self.margin, self.scale)
        weight = self.weight.to(feats.device)
        c = torch.mm(F.normalize(feats), F.normalize(weight, dim=0)).clamp(-1, 1)
        hot = torch.zeros_like(c).scatter_(1, labels.view(-1, 1).long(), 1).bool()
        return torch.where(hot, c - self.margin, c) * self.scale


class ArcNegFace(nn.Module):
    """ArcNegFace, "Towards Flops-constrained Face Recognition" (reference head/metrics.py:394-433): HIP kernels on device
    tensors, plain PyTorch on the host.

    With ``gt`` a row's target cosine (never clamped): the label column becomes ``a = cos(acos(gt) + margin)`` where ``gt >
    thresh`` (``thresh = cos(pi - margin)``), else ``gt - mm``; every other column becomes ``t * c + t - 1`` with ``t =
    alpha * exp(-(c - a)^2 / sigma)``, ``t`` and the ``a`` inside it constants of the graph; all times ``scale``.  The
    reference fills its logits in a Python loop over the rows with two host reads per row; both paths here are vectorised
    and read nothing on the host.  ``alpha``, ``sigma``, ``thresh``, ``mm``, ``margin`` and ``scale`` are plain attributes
    read on every call; ``weight`` is [num_class, feat_dim] and the state dict holds that key alone.  Limits: see the module
    docstring."""

    def __init__(self, feat_dim, num_class, margin=0.5, scale=64):
        super().__init__()
        self.feat_dim = feat_dim
        self.num_class = num_class
        self.scale = scale
        self.margin = margin
        self.weight = Parameter(torch.empty(num_class, feat_dim))
        self.reset_parameters()
        self.alpha = 1.2
        self.sigma = 2
        self.thresh = math.cos(math.pi - self.margin)
        self.mm = math.sin(math.pi - self.margin) * self.margin

    def reset_parameters(self):
        stdv = 1. / math.sqrt(self.weight.size(1))
        self.weight.data.uniform_(-stdv, stdv)

    def forward(self, feats, labels):
        if feats.is_cuda:
            _beside(self, self.weight, feats)
            return FRF.arcneg_head(feats, self.weight, labels.to(feats.device), self.scale, self.thresh, self.margin,
                                   self.mm, self.alpha, self.sigma)
        if labels.numel():
            FRF._check_labels(labels, self.weight.shape[0])
        weight = self.weight.to(feats.device)
        ex = feats / torch.norm(feats, 2, 1, keepdim=True)
        ew = weight / torch.norm(weight, 2, 1, keepdim=True)
        c = torch.mm(ex, ew.t())
        at = labels.view(-1, 1).long()
        gt = c.gather(1, at)
        # the reference compares the fp32 value with the double thresh (:427); a tensor comparison would round thresh
        thresh = FRF.arcneg_thresh32(self.thresh) if c.dtype == torch.float32 else self.thresh
        branch = gt.detach() > thresh
        arc = torch.cos(torch.acos(torch.where(branch, gt, torch.zeros_like(gt))) + self.margin)
        a = torch.where(branch, arc, gt - self.mm)
        t = (self.alpha * torch.exp(-torch.pow(c - a, 2) / self.sigma)).detach()
        return self.scale * (t * c + t - 1).scatter(1, at, a)


class _QueueIds(collections.abc.Set):
    """The set of labels other than -1 in a snapshot of ``SST_Prototype.labels`` (a device clone taken at call time).  It
    reads the snapshot on first use, so the forward pass that returns it waits for nothing on the host."""

    def __init__(self, snapshot):
        self._snapshot, self._ids = snapshot, None

    def _set(self):
        if self._ids is None:
            self._ids = frozenset(v for v in self._snapshot.cpu().tolist() if v != -1)
            self._snapshot = None
        return self._ids

    def __contains__(self, item):
        return item in self._set()

    def __iter__(self):
        return iter(self._set())

    def __len__(self):
        return len(self._set())

    def __repr__(self):
        return "_QueueIds(%r)" % (set(self._set()),)


class SST_Prototype(nn.Module):
    """SST_Prototype, "Semi-Siamese Training for Shallow Face Learning" (reference head/metrics.py:638-708): HIP kernels on
    device tensors, plain PyTorch on the host.

    The head has no parameter: its class matrix is the buffer ``queue`` [feat_dim, queue_size] of normalised gallery
    embeddings, the only state-dict key.  ``forward(p1, g2, p2, g1, cur_ids)`` takes two views of B identities embedded by
    the probe network (p) and the gallery network (g), normalises all four, detaches the gallery rows, and returns
    ``(output1, output2, label, id_set)``: ``output1 = scale * add_margin(p1 . queue')`` with ``queue'`` the queue whose
    columns [index, index + B) hold g2's rows, ``output2`` the same of p2 and g1, ``label = arange(B) + index``.  Then one
    ``random.random()`` draw decides which gallery view the queue keeps in that window (above 0.5: g1), ``cur_ids`` go into
    the label list there and ``index`` moves on by B, modulo queue_size -- in every mode, eval and ``no_grad`` included.
    ``add_margin`` clamps to [-1, 1] and changes the label column: ``c - margin`` for ``'am_softmax'``, ``c cos(margin) -
    sqrt(1 - c^2) sin(margin)`` for ``'arc_softmax'`` (no threshold fallback), nothing for any other ``loss_type``.

    On the device ``queue`` is the data gradient's GEMM operand as it stands and ``queue_t`` [queue_size, feat_dim], a
    non-persistent buffer rebuilt after ``load_state_dict`` and ``.to()``, the cosine GEMM's; ``labels`` is a non-persistent
    int64 buffer and ``label_list`` a property that reads it on demand.  A step writes B columns of each and nothing else;
    see ``frhip.functional.sst_forward``.  ``queue_state()`` / ``load_queue_state()`` carry ``index`` and the labels for a
    driver's state file.  Limits: see the module docstring."""

    def __init__(self, feat_dim=512, queue_size=16384, scale=30.0, loss_type='softmax', margin=0.0):
        super().__init__()
        self.queue_size = queue_size
        self.feat_dim = feat_dim
        self.scale = scale
        self.margin = margin
        self.loss_type = loss_type
        queue = torch.rand(feat_dim, queue_size).uniform_(-1, 1).renorm_(2, 1, 1e-5).mul_(1e5)
        self.register_buffer('queue', F.normalize(queue, p=2, dim=0))
        self.register_buffer('queue_t', self.queue.t().contiguous(), persistent=False)
        self.register_buffer('labels', torch.full((queue_size,), -1, dtype=torch.int64), persistent=False)
        self.index = 0
        self._generation = 0  # forward calls so far: a backward call behind a later forward call raises
        self._t_of = None  # (data_ptr, version) of the queue that queue_t was built from

    # -- the queue in both layouts

    def _queue_key(self):
        return (self.queue.data_ptr(), self.queue._version, self.queue.device, self.queue.dtype)

    def _sync_queue_t(self):
        """``queue_t`` again from ``queue`` where the latter was replaced or written by anyone but the enqueue kernel
        (``load_state_dict``, ``.to()``, an assignment): the kernel writes through pointers and moves no version."""
        if self._t_of != self._queue_key() or self.queue_t.device != self.queue.device:
            if not self.queue.is_contiguous():
                self.queue = self.queue.contiguous()
            self.queue_t = self.queue.t().contiguous()
            self._t_of = self._queue_key()

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        self._t_of = None
        return out

    def _load_from_state_dict(self, *args, **kwargs):
        super()._load_from_state_dict(*args, **kwargs)
        self._t_of = None

    # -- the label list

    @property
    def label_list(self):
        return self.labels.cpu().tolist()

    def get_id_set(self):
        return set(v for v in self.label_list if v != -1)

    def queue_state(self):
        """(index, labels as a host int64 tensor): what a driver's state file keeps besides the state dict."""
        return self.index, self.labels.detach().cpu().clone()

    def load_queue_state(self, index, labels):
        labels = torch.as_tensor(labels, dtype=torch.int64)
        if labels.shape != self.labels.shape or not 0 <= int(index) < self.queue_size:
            raise ValueError("SST_Prototype.load_queue_state: index in [0, %d) and %d labels are required"
                             % (self.queue_size, self.queue_size))
        self.labels.copy_(labels)
        self.index = int(index)

    # -- the reference's arithmetic

    def add_margin(self, cos_theta, label):
        cos_theta = cos_theta.clamp(-1, 1)
        at = label.view(-1, 1)
        if self.loss_type == 'am_softmax':
            return cos_theta.scatter(1, at, cos_theta.gather(1, at) - self.margin)
        if self.loss_type == 'arc_softmax':
            gt = cos_theta.gather(1, at)
            sin_theta = torch.sqrt(1.0 - torch.pow(gt, 2))
            return cos_theta.scatter(1, at, gt * math.cos(self.margin) - sin_theta * math.sin(self.margin))
        return cos_theta

    def compute_theta(self, p, g, label):
        i, B = self.index, p.shape[0]
        queue = torch.cat([self.queue[:, :i], g.transpose(0, 1), self.queue[:, i + B:]], 1)
        return self.add_margin(torch.mm(p, queue.detach()), label)

    def forward(self, p1, g2, p2, g1, cur_ids):
        B = p1.shape[0]
        if self.index + B > self.queue_size:  # the reference raises at its slice assignment, after it has drawn nothing
            raise RuntimeError("SST_Prototype: the window [%d, %d) runs past the queue's %d columns; queue_size must be a "
                               "multiple of the batch size" % (self.index, self.index + B, self.queue_size))
        if p1.is_cuda:
            return self._forward_device(p1, g2, p2, g1, cur_ids)
        queue = self.queue
        p1, g2, p2, g1 = F.normalize(p1), F.normalize(g2).detach(), F.normalize(p2), F.normalize(g1).detach()
        label = torch.arange(B, dtype=torch.int64) + self.index
        output1 = self.compute_theta(p1, g2, label) * self.scale
        output2 = self.compute_theta(p2, g1, label) * self.scale
        g = g1 if random.random() > 0.5 else g2
        ids = torch.as_tensor(cur_ids, dtype=torch.int64).reshape(-1)[:B]
        with torch.no_grad():
            self.queue = torch.cat([queue[:, :self.index], g.transpose(0, 1).to(queue.dtype), queue[:, self.index + B:]], 1)
            self.labels[self.index:self.index + B] = ids.to(self.labels.device)
        self.index = (self.index + B) % self.queue_size
        self._generation += 1
        return output1, output2, label, self.get_id_set()

    def _forward_device(self, p1, g2, p2, g1, cur_ids):
        if self.queue_size % 32:
            raise NotImplementedError("SST_Prototype on the HIP path needs queue_size %% 32 == 0 (the GEMM's K step), got %d; "
                                      "the host path serves any size" % self.queue_size)
        dev = p1.device
        _beside(self, self.queue, p1)
        if self.queue.dtype != torch.float32:
            raise NotImplementedError("SST_Prototype on the HIP path computes in fp32")
        self._sync_queue_t()
        B = p1.shape[0]
        ids = torch.as_tensor(cur_ids, dtype=torch.int64).reshape(-1)[:B].to(dev).contiguous()
        label = torch.arange(self.index, self.index + B, dtype=torch.int64, device=dev)
        take_g1 = random.random() > 0.5
        kind, p0, p1m = FRF.sst_margin(self.loss_type, self.margin)
        self._generation += 1
        output1, output2 = FRF.SSTHeadFn.apply(torch.cat([p1, p2]), torch.cat([g2, g1]).detach(), ids, self.queue,
                                               self.queue_t, self.labels, self.index, take_g1, kind, p0, p1m, self.scale,
                                               self)
        self.index = (self.index + B) % self.queue_size
        return output1, output2, label, _QueueIds(self.labels.clone())
