"""Gradients with respect to the input images, host side: the oracle (oracle/irse_ref.py, float64 autograd) against the
reference's own input gradient (g15_input_grad, tests/golden/make_golden_input_grad.py), and the argument checks of the two
new C entry points (fr_stem_dgrad, fr_resize_bilinear_bwd), which run before any launch and need no GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

from frhip import synth
from oracle import irse_ref as O

from test_oracle_golden import build_state

# fixture case -> (g8_structure model, num_layers, squeeze-excite, prefix, train mode)
CASES = {"ir50_train": ("IR_50", 50, False, "", True), "ir50_eval": ("IR_50", 50, False, "", False),
         "psp_train": ("pSp", 50, True, "encoder.", True)}
NEW_ENTRIES = ("fr_stem_dgrad", "fr_resize_bilinear_bwd")


def g15_inputs():
    """(x [2, 3, 112, 112], gfeat [2, 512]) of every g15 case (make_golden_input_grad.inputs_of)."""
    return synth.uniform(15, "g15.x", (2, 3, 112, 112)), synth.normal(15, "g15.g", (2, 512))


def oracle_input_grad(golden_dir, tag):
    """float64 (features, dL/dx) of the oracle for a g15 case, loss = sum(features * gfeat)."""
    model, nl, se, prefix, train = CASES[tag]
    sd, _info = build_state(golden_dir, model)
    sd = {k: (v.detach().double() if v.is_floating_point() else v) for k, v in sd.items()}
    x, gfeat = g15_inputs()
    x = x.double().requires_grad_(True)
    avg = synth.uniform(15, "avg_image", (3, 112, 112)).double() if model == "pSp" else None
    feats = O.backbone_forward(sd, x, num_layers=nl, se=se, bn_train=train, prefix=prefix, avg_image=avg)
    (gx,) = torch.autograd.grad((feats * gfeat.double()).sum(), [x])
    return feats.detach(), gx


@pytest.fixture(scope="module")
def g15(golden_dir):
    return np.load(os.path.join(golden_dir, "g15_input_grad.npz"))


@pytest.mark.parametrize("tag", sorted(CASES))
def test_oracle_reproduces_the_reference_input_gradient(g15, golden_dir, tag):
    feats, gx = oracle_input_grad(golden_dir, tag)
    ref = torch.from_numpy(g15[tag + ".gx"]).double()
    dev = float(g15[tag + ".dev.gx"])
    assert 0 < dev < 0.05
    err = float((gx - ref).abs().max() / ref.abs().max())
    assert err <= 1.5 * dev + 1e-6, (tag, err, dev)
    assert abs(float(gx.norm()) / float(g15[tag + ".gx_norm64"]) - 1) < 1e-6
    f32 = torch.from_numpy(g15[tag + ".features"]).double()
    assert float((feats - f32).abs().max() / f32.abs().max()) < 1e-3


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7


def _dgrad(K=32, C=3, Ct=3, B=2, H=112, W=112, dtype=0, coef=True, G=1, X=1, Y=1):
    from frhip import _lib
    p = ctypes.c_void_p(16)  # never dereferenced: every case below fails its checks before a launch
    c = p if coef else None
    return _lib.lib.fr_stem_dgrad(p if G else None, p if X else None, p if Y else None, p, c, c, c, c, c, c, c, c,
                                  1.0, p, B, H, W, C, Ct, K, dtype, None)


def test_stem_dgrad_rejects_bad_arguments_without_a_gpu():
    from frhip import _lib
    lib = _lib.lib
    cases = [dict(K=48), dict(K=16), dict(C=4, Ct=3), dict(C=0), dict(K=32, C=3, Ct=6), dict(Ct=8, C=3, K=64),
             dict(coef=False), dict(G=0), dict(B=0), dict(H=0), dict(W=-1), dict(B=1 << 20, H=112, W=112),
             dict(dtype=2), dict(dtype=0, Y=0), dict(dtype=1, X=0, Y=0)]
    for kw in cases:
        assert _dgrad(**kw) == -1, kw
        assert b"fr_stem_dgrad" in lib.fr_last_error_string(), kw


def test_resize_bilinear_bwd_rejects_bad_arguments_without_a_gpu():
    from frhip import _lib
    lib = _lib.lib
    p = ctypes.c_void_p(16)
    for args in ((0, 128, 128, 112, 112), (65536, 128, 128, 112, 112), (6, 0, 128, 112, 112), (6, 128, -1, 112, 112),
                 (6, 128, 128, 0, 112), (6, 128, 128, 112, 0)):
        assert lib.fr_resize_bilinear_bwd(p, p, *args, None) == -1, args
        assert b"fr_resize_bilinear_bwd" in lib.fr_last_error_string()
    assert lib.fr_resize_bilinear_bwd(None, p, 6, 128, 128, 112, 112, None) == -1
