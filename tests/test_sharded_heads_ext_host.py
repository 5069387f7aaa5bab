"""CPU checks of the class-sharded SphereFace / Am_softmax / CurricularFace heads (frhip/sharded_head.py): the three new
entry points are declared in include/frhip.h, exported and prototyped and refuse bad shapes before any launch; the module's
parameter layout (``class_dim``), its slice / gather round trips, its initial draws and SphereFace's lambda schedule."""
import ctypes

import pytest
import torch

NEW_ENTRIES = ("fr_shard_target_cos", "fr_curricular_rows_from", "fr_shard_sum_parts")
# head -> (class_dim, the replicated head's parameter name)
LAYOUT = {"ArcFace": (0, "weight"), "CosFace": (0, "weight"), "SphereFace": (0, "weight"), "Am_softmax": (1, "kernel"),
          "CurricularFace": (1, "kernel")}
D, N = 16, 23


def _replicated(name):
    from head import metrics as H
    return H.CurricularFace(D, N) if name == "CurricularFace" else getattr(H, name)(D, N, None)


def test_new_entries_are_declared_exported_and_prototyped():
    from frhip import _lib
    lib = ctypes.CDLL(_lib.LIB_PATH)
    header = open(_lib.HEADER).read()
    for name in NEW_ENTRIES:
        assert "int %s(" % name in header, "include/frhip.h does not declare %s" % name
        assert name in _lib.protos, "no prototype for %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
        assert getattr(_lib.lib, name).argtypes == _lib.protos[name][1]
    assert _lib.protos["fr_shard_target_cos"][2] == ["cos", "label_local", "tl", "rows", "N", "ld", "stream"]
    assert _lib.protos["fr_curricular_rows_from"][2] == ["tl", "rowv", "mean", "t", "rows", "cos_m", "sin_m", "th", "mm",
                                                         "train", "stream"]
    assert _lib.lib.fr_abi_version() == 7


def test_new_entries_reject_bad_arguments_without_a_gpu():
    from frhip import _lib
    lib = _lib.lib
    tc = lambda r, n, ld: lib.fr_shard_target_cos(None, None, None, r, n, ld, None)  # noqa: E731
    for bad in ((0, 10, 12), (-1, 10, 12), (4, 0, 4), (4, 10, 8)):
        assert tc(*bad) == -1 and b"fr_shard_target_cos" in lib.fr_last_error_string(), bad
    rf = lambda r, train: lib.fr_curricular_rows_from(None, None, None, None, r, 0.8, 0.4, -0.8, 0.2, train, None)  # noqa: E731
    assert rf(0, 1) == -1 and b"fr_curricular_rows_from" in lib.fr_last_error_string()
    for train in (2, -1):
        msg = (rf(8, train), lib.fr_last_error_string())
        assert msg[0] == -1 and b"fr_curricular_rows_from" in msg[1] and b"train" in msg[1]
    sp = lambda parts, r: lib.fr_shard_sum_parts(None, parts, None, r, None)  # noqa: E731
    for bad in ((1, 0), (0, 4), (2, -3)):
        assert sp(*bad) == -1 and b"fr_shard_sum_parts" in lib.fr_last_error_string(), bad


def test_kinds_follow_the_functional_constants():
    from frhip import functional as FRF
    from frhip.sharded_head import KINDS
    assert KINDS == {"ArcFace": FRF.ARCFACE, "CosFace": FRF.COSFACE, "SphereFace": FRF.SPHEREFACE,
                     "Am_softmax": FRF.AM_SOFTMAX, "CurricularFace": FRF.CURRICULAR}
    from frhip.sharded_head import ShardedMarginLoss
    with pytest.raises(ValueError):
        ShardedMarginLoss(D, N, "MV_Softmax")


@pytest.mark.parametrize("name", sorted(LAYOUT))
def test_layout_and_round_trips_on_one_rank(name):
    from frhip.sharded_head import ShardedMarginLoss
    cdim, _ = LAYOUT[name]
    crit = ShardedMarginLoss(D, N, name)
    full_shape = (N, D) if cdim == 0 else (D, N)
    assert crit.class_dim == cdim and tuple(crit.weight.shape) == full_shape and crit.full_shape == full_shape
    assert (crit.lo, crit.hi) == (0, N) and crit.shard_sizes() == [N]
    full = torch.randn(full_shape)
    assert torch.equal(crit.gather_full(crit.slice_full(full)), full)
    crit.load_full_weight(full)
    assert torch.equal(crit.gather_weight(), full) and torch.equal(crit.weight.detach(), full)
    assert hasattr(crit, "t") == (name == "CurricularFace") and hasattr(crit, "iter") == (name == "SphereFace")
    if name == "CurricularFace":
        assert "t" in crit.state_dict() and tuple(crit.t.shape) == (1,) and float(crit.t) == 0.0
    with pytest.raises(ValueError):
        ShardedMarginLoss(D, N, name, full_weight=torch.zeros(full_shape[1], full_shape[0]))


@pytest.mark.parametrize("name", sorted(LAYOUT))
def test_a_shard_is_a_slice_of_the_replicated_draw(name, monkeypatch):
    """Same RNG state -> the shard is the [lo, hi) slice, along ``class_dim``, of what the replicated head draws; the
    constructor's defaults are the head's own."""
    from frhip import sharded_head as SH
    cdim, pname = LAYOUT[name]
    torch.manual_seed(5)
    ref = _replicated(name)
    full = getattr(ref, pname).detach()
    torch.manual_seed(5)
    whole = SH.ShardedMarginLoss(D, N, name)
    assert torch.equal(whole.weight.detach(), full)
    assert whole.m == ref.m and (name == "SphereFace" or whole.s == ref.s)
    monkeypatch.setattr(SH, "class_range", lambda n, world, rank: (7, 15))  # a middle rank's range
    torch.manual_seed(5)
    part = SH.ShardedMarginLoss(D, N, name)
    assert torch.equal(part.weight.detach(), full[7:15] if cdim == 0 else full[:, 7:15])
    again = SH.ShardedMarginLoss.from_head(ref)
    assert again.head_name == name and (again.in_features, again.out_features) == (D, N)
    assert torch.equal(again.weight.detach(), part.weight.detach())


def test_from_head_takes_t_and_iter_along():
    from frhip.sharded_head import ShardedMarginLoss
    cf = _replicated("CurricularFace")
    cf.t.fill_(0.25)
    assert float(ShardedMarginLoss.from_head(cf).t) == 0.25
    sf = _replicated("SphereFace")
    sf.iter = 41
    assert ShardedMarginLoss.from_head(sf).iter == 41


def test_sphereface_lambda_follows_the_replicated_heads():
    """k forward calls leave ``iter`` and lambda where head.metrics.SphereFace has them (the stand-in kernels of the gloo
    test carry the arithmetic)."""
    from frhip.sharded_head import ShardedMarginLoss
    from shard_ref_ext import ExtOracleKernels
    ref = _replicated("SphereFace")
    crit = ShardedMarginLoss.from_head(ref, kernels=ExtOracleKernels())
    x, y = torch.randn(3, D), torch.tensor([0, N - 1, 4])
    for k in range(1, 6):
        ref(x, y)
        crit(x, y)
        assert crit.iter == ref.iter == k and crit.lamb == ref.lamb
    ref.iter = crit.iter = 2000  # past the knee: LambdaMin
    ref(x, y)
    crit(x, y)
    assert crit.lamb == ref.lamb == 5.0
