"""``shard_ref.OracleKernels`` with the methods the Softmax head and ``loss="Softmax"`` of frhip/sharded_head.py call besides:
the cross-entropy finalize step and the linear head's logits and gradients, in plain torch on the CPU.  Same method
signatures, same meaning of every return value; test infrastructure only.  ``FocalSlopeKernels`` is a negative control."""
import torch
import torch.nn.functional as F

import softmax_data as SD
from shard_ref import OracleKernels
from frhip.functional import HeadSaved


class SoftmaxOracleKernels(OracleKernels):
    def ce(self, ce, rank):
        l = ce.double().mean().float()
        sc = torch.zeros(8)
        sc[0] = sc[4] = l
        sc[1] = 1.0
        sc[2] = 100.0 * (rank < 1).sum() / ce.shape[0]
        sc[3] = 100.0 * (rank < 5).sum() / ce.shape[0]
        return sc

    def linear_logits(self, x_all, w, bias):
        return F.linear(x_all, w, bias), HeadSaved(x=x_all, w=w), None

    def linear_bwd(self, saved, cfg, g, need_x, need_w):
        G = g @ saved.w if need_x else None
        gw = g.t() @ saved.x if need_w else None
        gb = SD.col_sums_in_row_order(g) if need_w else None
        return G, gw, gb


class FocalSlopeKernels(SoftmaxOracleKernels):
    """The right loss with the focal slope (gamma = 2) left in scalars[1]: the backward pass is scaled by it."""

    def ce(self, ce, rank):
        sc = super().ce(ce, rank)
        sc[1] = self.focal(ce, rank, 2.0)[1]
        return sc
