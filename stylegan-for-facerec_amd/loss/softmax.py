"""``LOSS_NAME = 'Softmax'``: the reference's train.py builds ``nn.CrossEntropyLoss()`` for it (train.py:237-238) and calls
it on the logits (:300-302).  This module is that loss with the batch-mean cross entropy on the HIP row-softmax kernels
when the logits are on a ROCm device; host logits take ``F.cross_entropy``.  It returns the scalar, not a tuple.
"""
import torch.nn as nn
import torch.nn.functional as F

from frhip import functional as FRF


class CrossEntropyLoss(nn.Module):
    def forward(self, input, target):
        if input.is_cuda:
            return FRF.cross_entropy(input, target.to(input.device))
        return F.cross_entropy(input, target)
