"""CPU checks of the CurricularFace head (reference head/metrics.py:475-510): the host path reproduces the reference's own
vectors (g18_curricular, tests/golden/make_golden_curricular.py) including ``t``, three deliberately wrong variants each miss
them, the module keeps the reference's layout, the C ABI of the HIP path is declared, exported and checks its arguments
before any launch, and train.py's head table takes the name."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import curricular_data as CD
from frhip import synth

CASES = ("rand_t0", "built_t0", "built_t03", "built_m03")
NEW_ENTRIES = ("fr_curricular_rows", "fr_curricular_ema", "fr_curricular_apply", "fr_curricular_bwd")
B, D, N = 8, 512, 100


@pytest.fixture(scope="module")
def g18(golden_dir):
    return np.load(os.path.join(golden_dir, "g18_curricular.npz"))


def inputs_of(g, tag):
    """(x, kernel, label, gout) of a g18 case, regenerated from synth; the file keeps the labels as a check."""
    x, k, label, gout = (CD.built if tag.startswith("built") else CD.random_case)(synth, tag, B, D, N)
    assert torch.equal(label, torch.from_numpy(g[tag + ".label"]))
    return x, k, label, gout


def make_head(g, tag, k):
    from head.metrics import CurricularFace
    head = CurricularFace(D, N, m=float(g[tag + ".m"]), s=float(g[tag + ".s"]))
    with torch.no_grad():
        head.kernel.copy_(k)
        head.t.fill_(float(g[tag + ".t0"]))
    return head


def variant(x, k, label, t0, m, s, old_t=False, no_2c=False, keep_label=False):
    """The head's arithmetic written out once more with one deliberate mistake per flag; returns (logits, t)."""
    c = torch.mm(F.normalize(x), F.normalize(k, dim=0)).clamp(-1, 1)
    at = label.view(-1, 1)
    tl = c.gather(1, at)
    ctm = tl * math.cos(m) - torch.sqrt(1.0 - torch.pow(tl, 2)) * math.sin(m)
    final = torch.where(tl > math.cos(math.pi - m), ctm, tl - math.sin(math.pi - m) * m)
    t = tl.detach().mean() * 0.01 + (1 - 0.01) * t0
    tt = t0 if old_t else t
    hard = c > ctm
    reweighted = c * (tt + c)
    if no_2c:  # the factor's own c held constant: d/dc = t + c instead of t + 2c
        reweighted = c * (tt + c.detach())
    out = torch.where(hard, reweighted, c)
    if not keep_label:
        out = out.scatter(1, at, final)
    return out * s, t


def errors(g, tag, y, gx, gw):
    """{name: (error, bar)}: logits absolute, gradients relative to max|ref|, against the fp32 reference."""
    idx = torch.from_numpy(g[tag + ".gw_index"])
    res = {"logits": (float((y.detach() - torch.from_numpy(g[tag + ".logits"])).abs().max()), 1e-5)}
    for name, got in (("gx", gx), ("gw", gw.index_select(1, idx))):
        ref = torch.from_numpy(g[tag + "." + name])
        assert got.shape == ref.shape
        res[name] = (float((got - ref).abs().max() / ref.abs().max()), max(1e-5, 8 * float(g[tag + ".dev." + name])))
    return res


@pytest.mark.parametrize("tag", CASES)
def test_host_path_reproduces_the_reference(g18, tag):
    """Logits under 1e-5 absolute, gradients under max(1e-5, 8 x the reference's own fp32-vs-float64 deviation), t after the
    call for both starting values of t."""
    x, k, label, gout = inputs_of(g18, tag)
    head = make_head(g18, tag, k)
    x.requires_grad_(True)
    y = head(x, label)
    gx, gw = torch.autograd.grad(y, [x, head.kernel], gout)
    for name, (err, bar) in errors(g18, tag, y, gx, gw).items():
        assert err < bar, (tag, name, err, bar)
    assert abs(float(gw.double().norm()) / float(g18[tag + ".gw_norm"]) - 1) < 1e-5
    assert tuple(head.t.shape) == (1,) and list(head.state_dict()) == ["kernel", "t"]
    t_ref = float(g18[tag + ".t"][0])
    assert abs(float(head.t) - t_ref) <= 1e-7 * max(1.0, abs(t_ref)), (float(head.t), t_ref)


def test_fixture_covers_both_branches(g18):
    """Every built case has easy and hard negatives (10 % .. 90 % hard) and both target branches, on this test's own
    float64 restatement as in the maker; the random case is all hard (which is why the cases are built)."""
    for tag in CASES:
        x, k, label, _ = inputs_of(g18, tag)
        frac, first, second, tmax = CD.stats64(x, k, label, float(g18[tag + ".m"]))
        assert frac == pytest.approx(float(g18[tag + ".hard_fraction"]), abs=1e-12)
        assert (first, second) == (int(g18[tag + ".rows_first_branch"]), int(g18[tag + ".rows_second_branch"]))
        if tag.startswith("built"):
            CD.assert_covers_both_branches(x, k, label, float(g18[tag + ".m"]))
        else:
            assert frac == 1.0 and second == 0
    assert float(g18["built_t0.t0"]) == 0.0 and float(g18["built_t03.t0"]) == pytest.approx(0.3)
    assert float(g18["built_m03.m"]) == pytest.approx(0.3)


@pytest.mark.parametrize("flag", ["old_t", "no_2c", "keep_label"])
def test_negative_controls_miss_the_fixture(g18, flag):
    """The written-out variant equals the head's host path with no flag set, and misses g18 with any single one: the old t
    instead of the updated one, no 2c term in the backward pass, the label column not overwritten."""
    tag = "built_t03"
    x, k, label, gout = inputs_of(g18, tag)
    m, s, t0 = float(g18[tag + ".m"]), float(g18[tag + ".s"]), float(g18[tag + ".t0"])

    def run(**flags):
        xx = x.clone().requires_grad_(True)
        kk = k.clone().requires_grad_(True)
        y, t = variant(xx, kk, label, torch.full((1,), t0), m, s, **flags)
        gx, gw = torch.autograd.grad(y, [xx, kk], gout)
        return errors(g18, tag, y, gx, gw)

    assert all(err < bar for err, bar in run().values()), run()
    bad = run(**{flag: True})
    assert any(err > 10 * bar for err, bar in bad.values()), (flag, bad)
    if flag == "no_2c":  # a backward-only mistake: the logits still match
        assert bad["logits"][0] < bad["logits"][1] and bad["gx"][0] > 10 * bad["gx"][1]


def test_head_keeps_the_reference_layout():
    """Constructor (feat_dim, num_class, m = 0.5, s = 64.), parameter ``kernel`` [D, N] ~ N(0, 0.01^2), buffer ``t`` [1],
    the reference's attributes; t moves on every forward call, in eval mode and under no_grad too."""
    from head.metrics import CurricularFace
    torch.manual_seed(0)
    h = CurricularFace(512, 10)
    assert list(h.state_dict()) == ["kernel", "t"] and [n for n, _ in h.named_parameters()] == ["kernel"]
    assert tuple(h.kernel.shape) == (512, 10) and tuple(h.t.shape) == (1,) and float(h.t) == 0.0
    assert 0.008 < float(h.kernel.detach().std()) < 0.012
    assert (h.m, h.s) == (0.5, 64.0) and h.process_group is None
    assert (h.cos_m, h.sin_m) == (math.cos(0.5), math.sin(0.5))
    assert (h.threshold, h.mm) == (math.cos(math.pi - 0.5), math.sin(math.pi - 0.5) * 0.5)
    h2 = CurricularFace(16, 5, m=0.3, s=30.0)
    assert (h2.m, h2.s) == (0.3, 30.0)
    x, y = synth.normal(3, "cf.x", (3, 512)), torch.tensor([0, 9, 3])
    h.eval()
    with torch.no_grad():
        out = h(x, y)
    assert out.shape == (3, 10) and out.device.type == "cpu" and float(h.t) != 0.0
    t1 = float(h.t)
    h(x, y)
    assert float(h.t) != t1
    # the weight-decay group of train.py: the kernel is not a batch-norm parameter
    from util.utils import separate_irse_bn_paras
    bn, rest = separate_irse_bn_paras(h)
    assert bn == [] and len(rest) == 1 and rest[0] is h.kernel
    # a round trip through the state dict carries t
    h3 = CurricularFace(512, 10)
    h3.load_state_dict(h.state_dict())
    assert torch.equal(h3.t, h.t) and torch.equal(h3.kernel, h.kernel)


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    for name in ("curricular_forward", "curricular_backward", "CurricularHeadFn", "curricular_head"):
        assert hasattr(FRF, name)


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: empty shapes, row pitches that are too short or not multiples of 4, a train
    flag that is neither 0 nor 1, a non-positive scale."""
    from frhip import _lib
    lib = _lib.lib
    rows = lambda r, n, ld, train: lib.fr_curricular_rows(None, None, None, None, None, r, n, ld, 0.8, 0.4, -0.8, 0.2,  # noqa: E731
                                                          train, None)
    assert rows(0, 100, 100, 1) == -1 and rows(8, 0, 100, 1) == -1 and rows(8, 100, 96, 1) == -1
    assert b"fr_curricular_rows" in lib.fr_last_error_string()
    assert rows(8, 100, 100, 2) == -1 and b"train" in lib.fr_last_error_string()
    assert lib.fr_curricular_ema(None, None, 0.0, None) == -1 and lib.fr_curricular_ema(None, None, -0.5, None) == -1
    apply_ = lambda r, n, ld: lib.fr_curricular_apply(None, None, None, None, None, r, n, ld, 64.0, None)  # noqa: E731
    assert apply_(0, 100, 100) == -1 and apply_(8, 101, 101) == -1 and apply_(8, 100, 96) == -1
    assert b"fr_curricular_apply" in lib.fr_last_error_string()
    bwd = lambda r, n, ld, ldg: lib.fr_curricular_bwd(None, None, None, None, None, None, r, n, ld, ldg, 0.8, 0.4, 64.0,  # noqa: E731
                                                      None)
    assert bwd(0, 100, 100, 128) == -1 and bwd(8, 100, 100, 96) == -1 and bwd(8, 100, 98, 128) == -1
    assert bwd(8, 100, 100, 126) == -1 and b"fr_curricular_bwd" in lib.fr_last_error_string()


def test_device_entry_refuses_host_tensors():
    """No quiet fall-back: the functional entry is the HIP path and says so when handed host tensors."""
    from frhip import _lib
    from frhip import functional as FRF
    x, k = torch.zeros(2, 16), torch.ones(16, 5)
    with pytest.raises(_lib.FrhipError):
        FRF.curricular_head(x[:0], k, torch.tensor([], dtype=torch.long), torch.zeros(1), 64.0, 0.5)
    with pytest.raises(ValueError, match="t must be"):
        FRF.curricular_head(x, k, torch.tensor([0, 1]), torch.zeros(1, dtype=torch.float64), 64.0, 0.5)


def test_train_py_head_table_takes_the_name():
    """train.py imports the head, builds it in its ``heads`` table with ARCFACE_S and hands it the process group when
    there is more than one rank; SHARDED_HEAD still names ArcFace/CosFace only."""
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "stylegan-for-facerec_amd")
    src = open(os.path.join(root, "train.py")).read()
    assert re.search(r"from head\.metrics import [^\n]*\bCurricularFace\b", src)
    assert re.search(r'"CurricularFace":\s*CurricularFace\(emb, num_class, s=s\)', src)
    assert "head.process_group = dist.group.WORLD" in src
    assert 'cfg["HEAD_NAME"] not in ("ArcFace", "CosFace")' in src
    common = open(os.path.join(root, "configs", "_common.py")).read()
    assert "CurricularFace" in common
