"""The backward pass of the five heads when only one input wants a gradient: x.grad and the weight / kernel gradient are
bit-identical to those of the call where both do, with and without the weight-gradient side stream.  The launches and
their arguments are the same in all three calls and every reduction runs in a fixed order.

(5, 100): five rows leave the 4-rows-per-block row kernels a ragged last block; (8, 1001): N is no multiple of 4, so the
logits are a [:, :N] view of a padded store and the weight-gradient GEMM runs on a padded class count."""
import pytest
import torch

from frhip import synth

pytestmark = pytest.mark.gpu

D = 512
HEADS = ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def make(name, N):
    from head import metrics as H
    head = H.CurricularFace(D, N) if name == "CurricularFace" else getattr(H, name)(D, N, None)
    p = list(head.parameters())[0]
    with torch.no_grad():
        p.copy_(synth.uniform(61, "%s.%d.w" % (name, N), tuple(p.shape), -0.1, 0.1))
    return head.cuda(), list(head.parameters())[0]


def grads(head, p, x, label, gout, need_x, need_w):
    if hasattr(head, "t"):
        head.t.zero_()  # CurricularFace: every run starts from the same t
    if hasattr(head, "iter"):
        head.iter = 0  # SphereFace: and from the same lambda
    xx = x.clone().requires_grad_(need_x)
    p.requires_grad_(need_w)
    p.grad = None
    head(xx, label).backward(gout)
    return xx.grad, p.grad


@pytest.mark.parametrize("B,N", [(5, 100), (8, 1001)])
@pytest.mark.parametrize("name", HEADS)
def test_one_sided_gradients_equal_the_two_sided_ones(name, B, N, monkeypatch):
    head, p = make(name, N)
    x = synth.normal(61, "x.%d" % B, (B, D), std=0.04).cuda()  # |x| ~ 0.9: Am_softmax does not normalise x
    label = synth.labels(61, "y.%d.%d" % (B, N), B, N).cuda()
    gout = synth.normal(61, "g.%d.%d" % (B, N), (B, N)).cuda()
    for single in ("0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        gx, gw = grads(head, p, x, label, gout, True, True)
        assert gx.shape == x.shape and gw.shape == p.shape
        assert bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gw).all()) and bool(gx.any()) and bool(gw.any())
        gx1, none_w = grads(head, p, x, label, gout, True, False)
        none_x, gw1 = grads(head, p, x, label, gout, False, True)
        assert none_w is None and none_x is None
        assert torch.equal(gx1, gx), (name, single, float((gx1 - gx).abs().max()))
        assert torch.equal(gw1, gw), (name, single, float((gw1 - gw).abs().max()))
