"""Margin-softmax heads with the reference's import path, constructor signatures and state-dict keys.

    from head.metrics import ArcFace, CosFace, SphereFace, Am_softmax        (reference train.py:9)
    from head.metrics import CurricularFace, MagFace                         (reference head/metrics.py:475, :512)

The four heads the reference driver can select (``HEAD_NAME``, train.py:56,178-182) and ``CurricularFace`` / ``MagFace``
(two of the FaceX-Zoo heads of the reference's head/metrics.py that its driver never names; train.py here accepts them) run
on the HIP kernels when their input is a device tensor:
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
    backward pass adds a radial term r * xhat to the feature gradient: the margin and ``loss_g`` both depend on ||x||.
On host tensors ``SphereFace`` / ``Am_softmax`` / ``CurricularFace`` / ``MagFace`` run the reference's plain-PyTorch arithmetic (the
restatement the tests compare with); ``ArcFace`` / ``CosFace`` refuse host tensors.  ``SphereFace.iter`` counts forward
calls on either path, as in the reference; train.py carries it across a resume in the State_* file.  ``CurricularFace.t``
is a buffer: the Head_* file carries it.

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
"""
import math

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
