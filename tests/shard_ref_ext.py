"""Test stand-in for the SphereFace / Am_softmax / CurricularFace methods of ``frhip.sharded_head.HipKernels`` in plain
PyTorch on the CPU, so that the ``gloo`` test can run the three heads' collective choreography without a GPU.  It extends
tests/shard_ref.py (the statistics, focal and d-logits steps are the same for every head).

Unlike the ArcFace / CosFace stand-in, this one keeps the split the HIP path has: ``ext_bwd`` returns G = d loss / d xn
(xn = the normalised rows; x itself for Am_softmax) and SphereFace's radial sums separately, and ``normalize_bwd`` /
``normalize_bwd_radial`` are the real backward of the normalisation.  What is exchanged between the ranks (G, r, the target
cosines) therefore decides the result, which is what the negative controls of the test rely on.

``LocalTargetKernels`` is a deliberately wrong variant: CurricularFace's cos(theta_target + m) from the shard's own target
cosines only (0 where the label lives on another rank), never exchanged."""
import math

import torch
import torch.nn.functional as F

from shard_ref import OracleKernels
from frhip import functional as FRF
from frhip.functional import HeadCfg, HeadSaved

_CHEB = {0: lambda x: x ** 0, 1: lambda x: x, 2: lambda x: 2 * x ** 2 - 1, 3: lambda x: 4 * x ** 3 - 3 * x,
         4: lambda x: 8 * x ** 4 - 8 * x ** 2 + 1, 5: lambda x: 16 * x ** 5 - 20 * x ** 3 + 5 * x}


def _own_hot(label_local, n):
    """(rows that own their label, one-hot [rows, n] of the owned labels)."""
    own = (label_local >= 0) & (label_local < n)
    hot = torch.zeros(label_local.shape[0], n, dtype=torch.bool)
    hot[own, label_local[own]] = True
    return own, hot


class ExtOracleKernels(OracleKernels):
    def ext_logits(self, x_all, w, label_local, kind, mi, p0, p1):
        wl = w.clone().requires_grad_(True)
        sphere = kind == FRF.SPHEREFACE
        n = w.shape[0] if sphere else w.shape[1]
        _, hot = _own_hot(label_local, n)
        with torch.enable_grad():
            if sphere:  # head/metrics.py SphereFace: out = ||x|| * (hot ? (phi - c) / (1 + lambda) + c : c)
                nrm = x_all.norm(2, 1).clamp_min(1e-12)
                inv_x = 1.0 / nrm
                xn = (x_all * inv_x[:, None]).requires_grad_(True)
                c = F.linear(xn, F.normalize(wl)).clamp(-1, 1)
                k = (mi * c.detach().acos() / 3.14159265).floor()
                phi = ((-1.0) ** k) * _CHEB[mi](c) - 2 * k
                a = torch.where(hot, (phi - c) / p0 + c, c)
                logits = a * nrm[:, None]
            else:  # Am_softmax: x is not normalised, the kernel's columns are
                inv_x, a = None, None
                xn = x_all.clone().requires_grad_(True)
                c = torch.mm(xn, wl / wl.norm(2, 0, True)).clamp(-1, 1)
                logits = torch.where(hot, c - p0, c) * p1
        saved = HeadSaved(x=xn, w=wl, label=label_local, inv_x=inv_x, cos=logits,
                          rowv=None if a is None else a.detach())
        return logits.detach(), saved, HeadCfg(kind, None, None)

    def target_cos(self, cos, label_local, n, ld):
        own, _ = _own_hot(label_local, n)
        picked = cos.gather(1, label_local.clamp(min=0)[:, None])[:, 0]
        return torch.where(own, picked, torch.zeros_like(picked))

    def curricular_logits(self, x_all, w, label_local, t, s, m, exchange, train):
        wl = w.clone().requires_grad_(True)
        n = w.shape[1]
        _, hot = _own_hot(label_local, n)
        cos_m, sin_m = math.cos(m), math.sin(m)
        th, mm = math.cos(math.pi - m), math.sin(math.pi - m) * m
        inv_x = 1.0 / x_all.norm(2, 1).clamp_min(1e-12)
        with torch.enable_grad():
            xn = (x_all * inv_x[:, None]).requires_grad_(True)
            c = torch.mm(xn, F.normalize(wl, dim=0)).clamp(-1, 1)
            tl = self.global_target_cos(c.detach(), label_local, n, exchange)
            ctm = tl * cos_m - torch.sqrt(1.0 - tl * tl) * sin_m
            if train:
                with torch.no_grad():
                    t.copy_(tl.mean() * 0.01 + (1 - 0.01) * t)
            tt = t.clone()
            out = torch.where(c.detach() > ctm[:, None], c * (tt + c), c)
            ctm_col = c * cos_m - torch.sqrt(1.0 - c * c) * sin_m  # used on the owned label column only
            final = torch.where(c > th, ctm_col, c - mm)
            logits = torch.where(hot, final, out) * s
        saved = HeadSaved(x=xn, w=wl, label=label_local, inv_x=inv_x, cos=logits, t=tt)
        return logits.detach(), saved, HeadCfg(FRF.CURRICULAR, None, None)

    def global_target_cos(self, c, label_local, n, exchange):
        return exchange(self.target_cos(c, label_local, n, n).clone())

    def ext_bwd(self, saved, cfg, g, need_x, need_w):
        G, gw = torch.autograd.grad(saved.cos, [saved.x, saved.w], g)
        r_part = (g * saved.rowv).sum(1, keepdim=True) if cfg.kind == FRF.SPHEREFACE else None
        return (G if need_x else None), (gw if need_w else None), r_part

    def sum_r(self, r_part):
        return r_part.sum(1, keepdim=True)

    def normalize_bwd(self, G, x, inv_x):
        xh = x * inv_x[:, None]
        return (G - xh * (xh * G).sum(1, keepdim=True)) * inv_x[:, None]

    def normalize_bwd_radial(self, G, x, inv_x, r):
        return self.normalize_bwd(G, x, inv_x) + r.view(-1, 1) * (x * inv_x[:, None])


class LocalTargetKernels(ExtOracleKernels):
    """Wrong on purpose: no exchange of the target cosines."""

    def global_target_cos(self, c, label_local, n, exchange):
        return self.target_cos(c, label_local, n, n)
