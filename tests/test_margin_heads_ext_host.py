"""CPU checks of the SphereFace / Am_softmax heads (reference head/metrics.py:200-333): the host path reproduces the
reference's own vectors (g14_sphere_am, tests/golden/make_golden_heads.py), SphereFace's lambda schedule, and the C ABI of
the HIP path (declared, exported, argument checks before any launch)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from frhip import synth

CASES = ("sphere_m4_it1", "sphere_m4_it10000", "sphere_m2_it10000", "am_unit", "am_small")
NEW_ENTRIES = ("fr_margin_apply", "fr_margin_apply_bwd", "fr_margin_apply_parts", "fr_normalize_bwd_radial",
               "fr_col_normalize", "fr_col_normalize_bwd")


def inputs_of(g, tag, B=8, D=512, N=100):
    """(x, weight, label, gout) of a g14 case, regenerated from synth (make_golden_heads.inputs_of); the file keeps the
    labels as a check."""
    x = synth.normal(14, tag + ".x", (B, D), std=float(g[tag + ".x_std"]))
    if tag.startswith("sphere"):
        w = synth.uniform(14, tag + ".w", (N, D), -0.1, 0.1)
    else:
        w = synth.uniform(14, tag + ".k", (D, N), -1.0, 1.0)
    label = synth.labels(14, tag + ".y", B, N)
    assert torch.equal(label, torch.from_numpy(g[tag + ".label"]))
    return x, w, label, synth.normal(14, tag + ".g", (B, N))


def gw_at_fixture_classes(g, tag, gw):
    """The weight gradient at the classes the file keeps: rows of [N, D] (SphereFace), columns of [D, N] (Am_softmax)."""
    idx = torch.from_numpy(g[tag + ".gw_index"])
    return gw.index_select(0 if tag.startswith("sphere") else 1, idx)


def make_head(g, tag, w):
    from head.metrics import Am_softmax, SphereFace
    if tag.startswith("sphere"):
        head = SphereFace(512, 100, None, m=int(g[tag + ".m"]))
        head.iter = int(g[tag + ".iter"]) - 1
        param = head.weight
    else:
        head = Am_softmax(512, 100, None, m=float(g[tag + ".m"]), s=float(g[tag + ".s"]))
        param = head.kernel
    with torch.no_grad():
        param.copy_(w)
    return head, param


@pytest.fixture(scope="module")
def g14(golden_dir):
    return np.load(os.path.join(golden_dir, "g14_sphere_am.npz"))


@pytest.mark.parametrize("tag", CASES)
def test_host_path_reproduces_the_reference(g14, tag):
    x, w, label, gout = inputs_of(g14, tag)
    head, param = make_head(g14, tag, w)
    x.requires_grad_(True)
    y = head(x, label)
    gx, gw = torch.autograd.grad(y, [x, param], gout)
    for name, got in (("logits", y), ("gx", gx), ("gw", gw_at_fixture_classes(g14, tag, gw))):
        ref = torch.from_numpy(g14[tag + "." + name])
        assert got.shape == ref.shape
        err = float((got.detach() - ref).abs().max() / ref.abs().max())
        assert err < 1e-5, (tag, name, err)
    assert abs(float(gw.double().norm()) / float(g14[tag + ".gw_norm"]) - 1) < 1e-5
    if tag.startswith("sphere"):
        assert head.iter == int(g14[tag + ".iter"]) and head.lamb == float(g14[tag + ".lamb"])


def test_fixture_covers_the_clamp(g14):
    """am_unit saturates (the backward pass must mask those entries), am_small does not; the SphereFace cases have
    lambda at both ends of its schedule."""
    assert float(g14["am_unit.saturated"]) >= 0.10 and float(g14["am_small.saturated"]) == 0.0
    assert abs(float(g14["sphere_m4_it1.lamb"]) - 1000 / 1.12) < 1e-9 and float(g14["sphere_m4_it10000.lamb"]) == 5.0


def test_sphereface_lambda_schedule():
    """lambda = max(5, 1000 / (1 + 0.12 iter)), iter incremented once per forward call (reference :236-238)."""
    from head.metrics import SphereFace
    head = SphereFace(16, 5, None)
    assert head.iter == 0
    x, y = synth.normal(3, "lam.x", (2, 16)), torch.tensor([0, 4])
    for it in (1, 2, 3):
        head(x, y)
        assert head.iter == it and head.lamb == max(5.0, 1000.0 * (1 + 0.12 * it) ** -1)
    head.iter = 1657
    head(x, y)
    assert head.lamb > 5.0  # 1000 / (1 + 0.12 * 1658) = 5.0002
    head(x, y)
    assert head.iter == 1659 and head.lamb == 5.0
    head.iter = 10 ** 6
    head(x, y)
    assert head.lamb == 5.0


def test_new_head_entries_are_declared_and_exported():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    assert _lib.lib.fr_margin_apply_parts(1024) == 1 and _lib.lib.fr_margin_apply_parts(28000) == 28


def test_new_head_entries_reject_unknown_kinds_without_a_gpu():
    """Argument checks run before any launch: other margin kinds, SphereFace m outside 0..5, bad row pitches."""
    from frhip import _lib
    lib = _lib.lib
    for kind in (0, 1, 4, -1):
        assert lib.fr_margin_apply(None, None, None, None, 8, 100, 100, kind, 4, 1.0, 1.0, None) == -1
        assert b"kind" in lib.fr_last_error_string()
        assert lib.fr_margin_apply_bwd(None, None, None, None, None, None, 8, 100, 100, 128, kind, 4, 1.0, 1.0,
                                       None) == -1
    assert lib.fr_margin_apply(None, None, None, None, 8, 100, 100, 2, 6, 1.0, 1.0, None) == -1
    assert lib.fr_margin_apply(None, None, None, None, 8, 101, 101, 3, 0, 0.35, 30.0, None) == -1  # ld % 4
    assert lib.fr_margin_apply_bwd(None, None, None, None, None, None, 8, 100, 100, 96, 3, 0, 0.35, 30.0, None) == -1
    assert lib.fr_col_normalize(None, None, None, None, 512, 100, 96, None) == -1


def test_heads_keep_the_reference_layout_and_run_on_the_host():
    """Constructor, state-dict keys and parameter shapes are the reference's ([N, D] weight / [D, N] kernel)."""
    from head.metrics import Am_softmax, SphereFace
    s, a = SphereFace(512, 10, None), Am_softmax(512, 10, None)
    assert list(s.state_dict()) == ["weight"] and tuple(s.weight.shape) == (10, 512) and s.m == 4
    assert list(a.state_dict()) == ["kernel"] and tuple(a.kernel.shape) == (512, 10) and (a.m, a.s) == (0.35, 30.0)
    y = a(synth.normal(4, "am.x", (3, 512)), torch.tensor([0, 9, 3]))
    assert y.shape == (3, 10) and y.device.type == "cpu"
