"""CPU checks of the MagFace head (reference head/metrics.py:512-553): the host path reproduces the reference's own vectors
(g19_magface, tests/golden/make_golden_magface.py) for both outputs and both gradients, three deliberately wrong variants
each miss them, the module keeps the reference's layout, the C ABI of the HIP path is declared, exported and checks its
arguments before any launch, and train.py takes the name and refuses it together with SHARDED_HEAD."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import magface_data as MD
from frhip import synth

CASES = ("rand", "built", "built_am", "built_p")
NEW_ENTRIES = ("fr_magface_rows", "fr_magface_apply", "fr_magface_bwd")
PARAMS = ("margin_am", "scale", "l_a", "u_a", "l_margin", "u_margin", "lamda")
B, D, N = 8, 512, 100


@pytest.fixture(scope="module")
def g19(golden_dir):
    return np.load(os.path.join(golden_dir, "g19_magface.npz"))


def params_of(g, tag):
    return {n: float(g["%s.%s" % (tag, n)]) for n in PARAMS}


def inputs_of(g, tag):
    """(x, weight, label, gout, gg) of a g19 case, regenerated from synth; the file keeps the labels and both upstream
    gradients as a check."""
    x, k, label, gout, gg = (MD.built if tag.startswith("built") else MD.random_case)(synth, tag, B, D, N)
    assert torch.equal(label, torch.from_numpy(g[tag + ".label"]))
    assert torch.equal(gout, torch.from_numpy(g[tag + ".gout"])) and torch.equal(gg, torch.from_numpy(g[tag + ".gg"]))
    return x, k, label, gout, gg


def variant(x, k, label, p, no_radial=False, no_inside=False, fixed_margin=False):
    """The head's arithmetic written out once more with one deliberate mistake per flag; returns (logits, lamda * loss_g)."""
    nrm = torch.norm(x, dim=1, keepdim=True)
    if no_radial:  # the magnitude as a constant: gx stays in the tangent plane of normalize(x)
        nrm = nrm.detach() + 0.0 * nrm
    a = nrm.clamp(p["l_a"], p["u_a"])
    if no_inside:  # the clamp's values with the gradient of the identity
        a = nrm + (a - nrm).detach()
    m = (p["u_margin"] - p["l_margin"]) / (p["u_a"] - p["l_a"]) * (a - p["l_a"]) + p["l_margin"]
    if fixed_margin:  # m(l_a) for every row
        m = torch.full_like(a, p["l_margin"])
    loss_g = 1 / (p["u_a"] ** 2) * a + 1 / a
    c = torch.mm(F.normalize(x), F.normalize(k, dim=0)).clamp(-1, 1)
    at = label.view(-1, 1)
    tl = c.gather(1, at)
    ctm = tl * torch.cos(m) - torch.sqrt(1.0 - torch.pow(tl, 2)) * torch.sin(m)
    final = torch.where(tl > torch.cos(math.pi - m), ctm, tl - p["margin_am"])
    return c.scatter(1, at, final) * p["scale"], p["lamda"] * loss_g


def errors(g, tag, y, lg, gx, gw):
    """{name: (error, bar)}: the forward outputs to fp32 rounding (1e-6 of max|ref|: a few ulp of the largest entry; the
    reference's own fp32-vs-float64 deviation is 1e-7 .. 4e-7), the gradients within max(1e-5, 8 x the reference's own
    deviation) of max|ref|, all against the fp32 reference."""
    idx = torch.from_numpy(g[tag + ".gw_index"])
    res = {}
    for name, got in (("logits", y.detach()), ("loss_g", lg.detach()), ("gx", gx), ("gw", gw.index_select(1, idx))):
        ref = torch.from_numpy(g[tag + "." + name])
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        bar = 1e-6 if name in ("logits", "loss_g") else max(1e-5, 8 * float(g[tag + ".dev." + name]))
        res[name] = (float((got - ref).abs().max() / ref.abs().max()), bar)
    return res


def grads(y, lg, x, w, gout, gg):
    return torch.autograd.grad([y, lg], [x, w], [gout, gg])


@pytest.mark.parametrize("tag", CASES)
def test_host_path_reproduces_the_reference(g19, tag):
    x, k, label, gout, gg = inputs_of(g19, tag)
    from head.metrics import MagFace
    p = params_of(g19, tag)
    head = MagFace(D, N, **p)
    with torch.no_grad():
        head.weight.copy_(k)
    x.requires_grad_(True)
    out = head(x, label)
    assert isinstance(out, tuple) and len(out) == 2
    y, lg = out
    assert tuple(y.shape) == (B, N) and tuple(lg.shape) == (B, 1)
    gx, gw = grads(y, lg, x, head.weight, gout, gg)
    for name, (err, bar) in errors(g19, tag, y, lg, gx, gw).items():
        print(tag, name, err, bar)
        assert err < bar, (tag, name, err, bar)
    assert abs(float(gw.double().norm()) / float(g19[tag + ".gw_norm"]) - 1) < 1e-5


def test_fixture_covers_the_regimes_and_branches(g19):
    """Every built case has rows below, inside and above [l_a, u_a], both target branches, an inside row in the margin
    branch and the safety margins, on this test's own float64 statistics as in the maker; so do the sizes the GPU tests
    build.  The random case reaches neither the clamp nor the fallback branch (which is why the cases are built)."""
    for tag in CASES:
        x, k, label, _, _ = inputs_of(g19, tag)
        p = params_of(g19, tag)
        st = MD.assert_covers(x, k, label, **p) if tag.startswith("built") else MD.stats64(x, k, label, **p)
        for name in ("below", "inside", "above", "margin_rows", "fallback_rows"):
            assert st[name] == int(g19["%s.%s" % (tag, name)])
    assert float(g19["rand.inside"]) == B and float(g19["rand.fallback_rows"]) == 0
    assert float(g19["built_am.margin_am"]) == pytest.approx(0.1) and float(g19["built_p.lamda"]) == 35
    for tag, Bb, Nn in (("big1000", 64, 1000), ("big1001", 64, 1001), ("big7000", 64, 7000), ("rep", 64, 1001),
                        ("radial", 64, 1001), ("guard", 6, 1001), ("prof", 16, 300)):
        x, k, label, _, _ = MD.built(synth, tag, Bb, D, Nn)
        MD.assert_covers(x, k, label, **MD.DEFAULTS)


def test_largest_fixture_covers_the_regimes_and_branches():
    x, k, label, _, _ = MD.built(synth, "big28000", 256, D, 28000)
    MD.assert_covers(x, k, label, **MD.DEFAULTS)


@pytest.mark.parametrize("flag", ["no_radial", "no_inside", "fixed_margin"])
def test_negative_controls_miss_the_fixture(g19, flag):
    """The written-out variant meets g19 with no flag set, and misses its bar by at least 10x with any single one: no
    radial term (the magnitude held constant), no ``inside`` mask (the clamp passes gradient everywhere), a fixed margin
    m(l_a)."""
    tag = "built"
    x, k, label, gout, gg = inputs_of(g19, tag)
    p = params_of(g19, tag)

    def run(**flags):
        xx = x.clone().requires_grad_(True)
        kk = k.clone().requires_grad_(True)
        y, lg = variant(xx, kk, label, p, **flags)
        return errors(g19, tag, y, lg, *grads(y, lg, xx, kk, gout, gg))

    assert all(err < bar for err, bar in run().values()), run()
    bad = run(**{flag: True})
    print(flag, bad)
    assert any(err > 10 * bar for err, bar in bad.values()), (flag, bad)
    if flag != "fixed_margin":  # backward-only mistakes: both outputs still match, gx does not
        assert bad["logits"][0] < bad["logits"][1] and bad["loss_g"][0] < bad["loss_g"][1]
        assert bad["gx"][0] > 10 * bad["gx"][1]


def test_head_keeps_the_reference_layout():
    """Constructor (feat_dim, num_class, margin_am = 0.0, scale = 32, l_a = 10, u_a = 110, l_margin = 0.45, u_margin = 0.8,
    lamda = 20), parameter ``weight`` [D, N] with unit columns, no buffers, ``calc_margin``."""
    from head.metrics import MagFace
    torch.manual_seed(0)
    h = MagFace(512, 10)
    assert list(h.state_dict()) == ["weight"] and [n for n, _ in h.named_parameters()] == ["weight"]
    assert tuple(h.weight.shape) == (512, 10)
    assert torch.allclose(h.weight.detach().norm(dim=0), torch.ones(10), atol=1e-4)
    assert (h.margin_am, h.scale, h.l_a, h.u_a, h.l_margin, h.u_margin, h.lamda) == (0.0, 32, 10, 110, 0.45, 0.8, 20)
    h2 = MagFace(16, 5, 0.1, 64, 5, 50, 0.3, 0.6, 35)
    assert (h2.margin_am, h2.scale, h2.l_a, h2.u_a, h2.l_margin, h2.u_margin, h2.lamda) == (0.1, 64, 5, 50, 0.3, 0.6, 35)
    assert float(h.calc_margin(torch.tensor(10.0))) == pytest.approx(0.45)
    assert float(h.calc_margin(torch.tensor(110.0))) == pytest.approx(0.8)
    x, y = synth.normal(3, "mf.x", (3, 512)), torch.tensor([0, 9, 3])
    out, lg = h(x, y)
    assert out.shape == (3, 10) and lg.shape == (3, 1) and out.device.type == "cpu"
    a = x.norm(dim=1, keepdim=True).clamp(10, 110)
    assert torch.allclose(lg, 20 * (a / 110 ** 2 + 1 / a))
    from util.utils import separate_irse_bn_paras
    bn, rest = separate_irse_bn_paras(h)
    assert bn == [] and len(rest) == 1 and rest[0] is h.weight
    h3 = MagFace(512, 10)
    h3.load_state_dict(h.state_dict())
    assert torch.equal(h3.weight, h.weight)


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    for name in ("MAGFACE", "magface_forward", "magface_backward", "MagFaceHeadFn", "magface_head"):
        assert hasattr(FRF, name)
    # defaulted fields only: the five existing heads build their records as before
    assert FRF.HeadCfg(0, 32, 4).mag is None and FRF.HeadSaved().rowv is None


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: empty shapes, row pitches that are too short or not multiples of 4, a
    magnitude interval that is empty or not positive."""
    from frhip import _lib
    lib = _lib.lib
    rows = lambda r, la, ua, d=512: lib.fr_magface_rows(None, None, r, d, la, ua, 0.45, 0.8, 20.0, None)  # noqa: E731
    assert rows(0, 10.0, 110.0) == -1 and rows(8, 10.0, 110.0, 0) == -1 and b"fr_magface_rows" in lib.fr_last_error_string()
    assert rows(8, 10.0, 10.0) == -1 and rows(8, 0.0, 110.0) == -1 and b"l_a" in lib.fr_last_error_string()
    apply_ = lambda r, n, ld: lib.fr_magface_apply(None, None, None, None, r, n, ld, 32.0, 0.0, None)  # noqa: E731
    assert apply_(0, 100, 100) == -1 and apply_(8, 101, 101) == -1 and apply_(8, 100, 96) == -1
    assert b"fr_magface_apply" in lib.fr_last_error_string()
    bwd = lambda r, n, ld, ldg, la=10.0: lib.fr_magface_bwd(None, None, None, None, None, None, None, r, n, ld, ldg, 32.0,  # noqa: E731
                                                             la, 110.0, 0.45, 0.8, 20.0, None)
    assert bwd(0, 100, 100, 128) == -1 and bwd(8, 100, 100, 96) == -1 and bwd(8, 100, 98, 128) == -1
    assert bwd(8, 100, 100, 126) == -1 and b"fr_magface_bwd" in lib.fr_last_error_string()
    assert bwd(8, 100, 100, 128, la=120.0) == -1 and b"l_a" in lib.fr_last_error_string()


def test_device_entry_refuses_host_tensors():
    """No quiet fall-back: the functional entry is the HIP path and says so when handed host tensors."""
    from frhip import _lib
    from frhip import functional as FRF
    x, k = torch.zeros(2, 16), torch.ones(16, 5)
    with pytest.raises(_lib.FrhipError):  # the empty batch launches nothing and still says so
        FRF.magface_head(x[:0], k, torch.tensor([], dtype=torch.long), 32, 0.0, 10, 110, 0.45, 0.8, 20)


def test_train_py_takes_the_name_and_refuses_the_sharded_head():
    """train.py builds MagFace in its ``heads`` table, adds loss_g.mean() to the loss of a head that returns a tuple, and
    raises NotImplementedError for SHARDED_HEAD with MagFace before anything is built (``check_head_config`` is the first
    thing ``main`` does with the configuration); the other heads pass that check."""
    import train
    with pytest.raises(NotImplementedError, match="MagFace"):
        train.check_head_config(dict(HEAD_NAME="MagFace", SHARDED_HEAD=True))
    train.check_head_config(dict(HEAD_NAME="MagFace", SHARDED_HEAD=False))
    train.check_head_config(dict(HEAD_NAME="MagFace"))
    for name in ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace"):
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
    src = open(train.__file__).read()
    main = src[src.index("def main():"):]
    assert main.index("check_head_config(cfg)") < main.index("torch.cuda.is_available()") < main.index("build_backbone(cfg)")
    assert 'heads["MagFace"] = MagFace(emb, num_class)' in src and "loss = loss + loss_g.mean()" in src
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "MagFace" in common
