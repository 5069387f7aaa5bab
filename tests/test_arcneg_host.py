"""CPU checks of the ArcNegFace head (reference head/metrics.py:394-433): the host path reproduces the reference's own vectors
(g24_arcnegface, tests/golden/make_golden_arcnegface.py) bit for bit in fp32, ``from_cos`` is the reference's loop, five
deliberately wrong variants each miss the fixture's bars, the module keeps the reference's layout, the C ABI of the HIP path
is declared, exported and checks its arguments before any launch, and train.py takes the name and refuses the class-sharded
head for it."""
import ctypes
import importlib.util
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import arcneg_data as AD
from frhip import synth

CASES = ("rand", "built", "built_m03_s32")
BUILT = CASES[1:]
NEW_ENTRIES = ("fr_arcneg_apply", "fr_arcneg_bwd")
B, D, N = 8, 512, 100
REFUSAL = ("SHARDED_HEAD=True with HEAD_NAME 'ArcNegFace': the class-sharded head does not serve ArcNegFace (its target "
           "cosines need an exchange of their own); run it replicated, SHARDED_HEAD=False")


@pytest.fixture(scope="module")
def g24(golden_dir):
    return np.load(os.path.join(golden_dir, "g24_arcnegface.npz"))


def scalars(g, tag):
    """(margin, scale) of a g24 case."""
    return float(g[tag + ".margin"]), float(g[tag + ".scale"])


def inputs_of(g, tag):
    """(x, weight, label, gout) of a g24 case, regenerated from synth; the file keeps the labels as a check."""
    margin, _ = scalars(g, tag)
    if tag.startswith("built"):
        x, w, label, gout = AD.built(synth, tag, B, D, N, margin)
    else:
        x, w, label, gout = AD.random_case(synth, tag, B, D, N)
    assert torch.equal(label, torch.from_numpy(g[tag + ".label"]))
    return x, w, label, gout


def make_head(g, tag, w):
    from head.metrics import ArcNegFace
    margin, scale = scalars(g, tag)
    head = ArcNegFace(D, N, margin=margin, scale=int(scale))
    with torch.no_grad():
        head.weight.copy_(w)
    return head


def errors(g, tag, y, gx, gw):
    """{name: (error, bar)}, the bars of the GPU test: logits absolute (1e-3), gradients and the norm of the whole weight
    gradient relative to the reference's, max(5e-3, 8 x the reference's own fp32-vs-float64 deviation)."""
    idx = torch.from_numpy(g[tag + ".gw_index"])
    res = {"logits": (float((y.detach().float() - torch.from_numpy(g[tag + ".logits"])).abs().max()), 1e-3)}
    for name, got in (("gx", gx), ("gw", gw.index_select(0, idx))):
        ref = torch.from_numpy(g[tag + "." + name])
        assert got.shape == ref.shape
        res[name] = (float((got.float() - ref).abs().max() / ref.abs().max()), max(5e-3, 8 * float(g[tag + ".dev." + name])))
    res["gw_norm"] = (abs(float(gw.double().norm()) / float(g[tag + ".gw_norm"]) - 1),
                      max(5e-3, 8 * float(g[tag + ".dev.gw"])))
    return res


@pytest.mark.parametrize("tag", CASES)
def test_host_path_reproduces_the_reference_bit_for_bit(g24, tag):
    """fp32: logits and gx equal the reference's bit for bit, gw on ``gw_index`` too, and the norm of the whole of gw to
    1e-6.  A float64 copy of the module: gt and a (the label column over the scale) within 1e-12 of the fixture's float64
    values, the same branches, and the fp32 logits within the fixture's own fp32-vs-float64 deviation of it."""
    x, w, label, gout = inputs_of(g24, tag)
    margin, scale = scalars(g24, tag)
    head = make_head(g24, tag, w)
    assert (head.thresh, head.mm) == (float(g24[tag + ".thresh"]), float(g24[tag + ".mm"]))
    assert (head.alpha, head.sigma) == (float(g24[tag + ".alpha"]), float(g24[tag + ".sigma"]))
    xx = x.clone().requires_grad_(True)
    y = head(xx, label)
    gx, gw = torch.autograd.grad(y, [xx, head.weight], gout)
    assert y.dtype == torch.float32 and torch.equal(y.detach(), torch.from_numpy(g24[tag + ".logits"]))
    assert torch.equal(gx, torch.from_numpy(g24[tag + ".gx"]))
    assert torch.equal(gw.index_select(0, torch.from_numpy(g24[tag + ".gw_index"])), torch.from_numpy(g24[tag + ".gw"]))
    assert abs(float(gw.double().norm()) / float(g24[tag + ".gw_norm"]) - 1) < 1e-6
    assert list(head.state_dict()) == ["weight"]
    h64 = make_head(g24, tag, w).double()
    with torch.no_grad():
        y64 = h64(x.double(), label)
    a64 = y64.gather(1, label.view(-1, 1)).view(-1) / scale
    assert float((a64 - torch.from_numpy(g24[tag + ".a"])).abs().max()) < 1e-12
    st = AD.stats64(x, w, label, margin)
    assert float((st["gt"] - torch.from_numpy(g24[tag + ".gt"])).abs().max()) < 1e-12
    assert torch.equal(st["branch"], torch.from_numpy(g24[tag + ".branch"]).bool())
    ref64, _ = AD.from_cos(AD.cos64(x, w), label, margin, scale=scale)
    assert float((y64 - ref64).abs().max()) < 1e-12 * scale
    assert float((y.detach().double() - y64).abs().max() / y64.abs().max()) < 2 * float(g24[tag + ".dev.logits"]) + 1e-7


def test_fixture_covers_both_branches(g24):
    """Every built case has rows on the acos branch near 0.9, 0.3 and -0.5 and two rows on the linear one, none within 1e-3
    of thresh or beyond +-0.98, on this test's own float64 restatement as in the maker; the random case has the acos branch
    alone (which is why the cases are built)."""
    for tag in CASES:
        x, w, label, _ = inputs_of(g24, tag)
        margin, scale = scalars(g24, tag)
        assert (margin, scale) == ((0.3, 32.0) if tag.endswith("_m03_s32") else (0.5, 64.0))
        if tag in BUILT:
            st = AD.assert_covers(x, w, label, margin)
            assert st["branch"].tolist() == [True, True, True, False] * 2
            for i, want in enumerate((0.9, 0.3, -0.5)):
                assert abs(float(st["gt"][i]) - want) < 1e-6
            assert float(st["gt"][3]) < AD.thresh_of(margin) - 1e-2 and float(st["gt"][7]) < AD.thresh_of(margin) - 1e-2
        else:
            assert bool(AD.stats64(x, w, label, margin)["branch"].all())
    assert abs(float(g24["built.gt"][3]) + 0.95) < 5e-3 and abs(float(g24["built.gt"][7]) + 0.95) < 5e-3


# ------------------------------------------------------------------------------------------------ the reference's loop


def reference_loop(cos, labels, margin, alpha, sigma, scale):
    """head/metrics.py:418-433 as written, from the cosine matrix on: the loop over the rows with its two host reads."""
    thresh = math.cos(math.pi - margin)
    mm = math.sin(math.pi - margin) * margin
    a = torch.zeros_like(cos)
    a_scale = torch.zeros_like(cos)
    c_scale = torch.ones_like(cos)
    t_scale = torch.ones_like(cos)
    for i in range(a.size(0)):
        lb = int(labels[i])
        a_scale[i, lb] = 1
        c_scale[i, lb] = 0
        if cos[i, lb].item() > thresh:
            a[i, lb] = torch.cos(torch.acos(cos[i, lb]) + margin)
        else:
            a[i, lb] = cos[i, lb] - mm
        reweight = alpha * torch.exp(-torch.pow(cos[i, ] - a[i, lb].item(), 2) / sigma)
        t_scale[i] *= reweight.detach()
    return scale * (a_scale * a + c_scale * (t_scale * cos + t_scale - 1))


def small_cosines(dtype):
    """(cos [6, 11], labels): target cosines 0.9, 0.3, -0.5, -0.97, -0.8, -0.9 (at margin 0.5 the last three but one lie on
    either side of thresh -0.878, at margin 0.3 -0.97 alone lies below thresh -0.955), the rest random in (-0.6, 0.6)."""
    cos = synth.uniform(AD.SEED, "loop.cos", (6, 11), -0.6, 0.6).double()
    labels = torch.tensor([0, 10, 3, 7, 7, 5])
    for i, gt in enumerate((0.9, 0.3, -0.5, -0.97, -0.8, -0.9)):
        cos[i, labels[i]] = gt
    return cos.to(dtype), labels


@pytest.mark.parametrize("margin,scale", [(0.5, 64.0), (0.3, 32.0)])
def test_from_cos_is_the_reference_loop(margin, scale):
    """``from_cos`` (the restatement the entry-point tests compare with) against autograd through the reference's lines
    restated above: fp32 logits bit for bit and the gradient with respect to the cosines bit for bit, float64 within 1e-13;
    the closed form of the issue (scale * t off the label column, scale * d a / d gt on it) equals both within 1e-12."""
    for dtype, bar in ((torch.float32, 0.0), (torch.float64, 1e-13)):
        cos, labels = small_cosines(dtype)
        g = synth.uniform(AD.SEED, "loop.g", (6, 11), -1.0, 1.0).to(dtype)
        ca = cos.clone().requires_grad_(True)
        ya = reference_loop(ca, labels, margin, AD.ALPHA, AD.SIGMA, scale)
        cb = cos.clone().requires_grad_(True)
        yb, rv = AD.from_cos(cb, labels, margin, AD.ALPHA, AD.SIGMA, scale)
        ga, = torch.autograd.grad(ya, ca, g)
        gb, = torch.autograd.grad(yb, cb, g, retain_graph=True)
        assert float((ya - yb).detach().abs().max()) <= bar * scale, dtype
        assert float((ga - gb).abs().max()) <= bar * scale, dtype
        assert rv["branch"].tolist() == [float(cos[i, labels[i]]) > AD.thresh_of(margin) for i in range(6)]
        assert any(rv["branch"].tolist()) and not all(rv["branch"].tolist())
    gt, a = rv["gt"].detach(), rv["a"].detach()
    th = torch.acos(gt) + margin
    da = torch.where(rv["branch"], torch.sin(th) / torch.sqrt(1 - gt * gt), torch.ones_like(gt))
    t = AD.ALPHA * torch.exp(-(cos - a.view(-1, 1)) ** 2 / AD.SIGMA)
    closed = (scale * t).scatter(1, labels.view(-1, 1), (scale * da).view(-1, 1)) * g
    assert float((closed - gb).abs().max()) < 1e-12 * scale


def reference_heads():
    """The reference's head/metrics.py as a module of its own (it imports torch and math alone), loaded from the tree that
    tests/golden/make_golden.py names and under a private name: nothing is imported through ``sys.path`` and the project's
    own ``head.metrics`` stays what it is.  None where that tree is not there."""
    maker = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "make_golden.py")).read()
    path = os.path.join(re.search(r'^REF = "([^"]+)"', maker, re.M).group(1), "head", "metrics.py")
    if not os.path.isfile(path):
        return None
    spec = importlib.util.spec_from_file_location("_reference_head_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_from_cos_is_the_reference_module_where_it_is_importable():
    """The same against the reference's own class (its loop unpatched), where its tree is there to import; elsewhere this
    part alone is skipped: ``reference_loop`` above restates those lines."""
    ref_heads = reference_heads()
    if ref_heads is None:
        pytest.skip("the reference is not importable here")
    from head import metrics as own
    assert ref_heads.ArcNegFace is not own.ArcNegFace and "for i in range(a.size(0))" in open(ref_heads.__file__).read()
    x, w, label, gout = AD.built(synth, "module", 6, 32, 25)
    for dtype, bar in ((torch.float32, 0.0), (torch.float64, 1e-12)):
        ref = ref_heads.ArcNegFace(32, 25)
        with torch.no_grad():
            ref.weight.data = w.clone().to(dtype)
        xa = x.clone().to(dtype).requires_grad_(True)
        ya = ref(xa, label)
        xb = x.clone().to(dtype).requires_grad_(True)
        ex = xb / torch.norm(xb, 2, 1, keepdim=True)
        ew = w.to(dtype) / torch.norm(w.to(dtype), 2, 1, keepdim=True)
        yb, rv = AD.from_cos(torch.mm(ex, ew.t()), label)
        assert any(rv["branch"].tolist()) and not all(rv["branch"].tolist())
        ga, = torch.autograd.grad(ya, xa, gout.to(dtype))
        gb, = torch.autograd.grad(yb, xb, gout.to(dtype))
        assert float((ya - yb).detach().abs().max()) <= bar * 64, dtype
        assert float((ga - gb).abs().max()) <= bar * 64 * float(ga.abs().max()), dtype


# ------------------------------------------------------------------------------------------------ negative controls


def variant(x, w, label, margin, scale, t_attached=False, label_reweighted=False, acos_everywhere=False,
            t_centred_on_gt=False):
    """The head's arithmetic written out once more with one deliberate mistake per flag."""
    thresh, mm = math.cos(math.pi - margin), math.sin(math.pi - margin) * margin
    ex = x / torch.norm(x, 2, 1, keepdim=True)
    ew = w / torch.norm(w, 2, 1, keepdim=True)
    c = torch.mm(ex, ew.t())
    at = label.view(-1, 1)
    gt = c.gather(1, at)
    branch = torch.ones_like(gt, dtype=torch.bool) if acos_everywhere else gt.detach().double() > thresh
    arc = torch.cos(torch.acos(torch.where(branch, gt, torch.zeros_like(gt))) + margin)
    a = torch.where(branch, arc, gt - mm)
    centre = gt if t_centred_on_gt else a
    t = AD.ALPHA * torch.exp(-torch.pow(c - centre.detach(), 2) / AD.SIGMA)
    if not t_attached:
        t = t.detach()
    body = t * c + t - 1
    if label_reweighted:  # c_scale dropped: the label column is a plus its re-weighted cosine
        return scale * (body + torch.zeros_like(c).scatter(1, at, a))
    return scale * body.scatter(1, at, a)


@pytest.mark.parametrize("flag", ["t_attached", "label_reweighted", "acos_everywhere", "t_centred_on_gt"])
def test_negative_controls_miss_the_fixture(g24, flag):
    """The written-out variant meets the bars of the GPU test (``errors``) on every case with no flag set, and misses them on
    the built batch with any single one: t left attached (backward only: the logits still match), the label column
    re-weighted too, the acos branch taken for every row, t centred on gt instead of a."""

    def run(tag, **flags):
        x, w, label, gout = inputs_of(g24, tag)
        xx = x.clone().requires_grad_(True)
        ww = w.clone().requires_grad_(True)
        y = variant(xx, ww, label, *scalars(g24, tag), **flags)
        gx, gw = torch.autograd.grad(y, [xx, ww], gout)
        return errors(g24, tag, y, gx, gw)

    for tag in CASES:
        assert all(err < bar for err, bar in run(tag).values()), (tag, run(tag))
    bad = {tag: run(tag, **{flag: True}) for tag in BUILT}
    print(flag, bad)
    for tag, res in bad.items():
        assert any(not err < bar for err, bar in res.values()), (flag, tag, res)  # NaN misses too
    if flag == "t_attached":
        assert all(res["logits"][0] < res["logits"][1] for res in bad.values())
        assert all(not res["gx"][0] < res["gx"][1] for res in bad.values())


def test_thresh_rounded_up_to_fp32_takes_the_other_branch():
    """cos(pi - 0.5) rounds UP to fp32.  A row whose target cosine is that fp32 value lies above the double thresh: the
    reference (an fp32 value read on the host against the double) takes the acos branch, and so do ``from_cos`` and the
    value the kernel is given -- the largest fp32 not above the double, one ulp below.  Comparing against the rounded
    threshold (what a tensor-against-scalar comparison does) takes the linear branch: a moves by about 0.117, far beyond
    the 1e-3 bar.  At margin 0.3 the nearest fp32 lies below the double and is passed as it is."""
    from frhip import functional as FRF
    thresh = math.cos(math.pi - 0.5)
    up = float(torch.tensor(thresh, dtype=torch.float64).float())
    assert up > thresh
    t32 = FRF.arcneg_thresh32(thresh)
    assert t32 < thresh < up and float(torch.nextafter(torch.tensor(t32), torch.tensor(1.0))) == up
    assert float(torch.tensor(t32)) == t32  # an fp32 value
    low = math.cos(math.pi - 0.3)
    assert FRF.arcneg_thresh32(low) == float(torch.tensor(low, dtype=torch.float64).float()) <= low
    cos, labels = small_cosines(torch.float32)
    cos[0, labels[0]] = up
    cos[1, labels[1]] = t32
    good, rv = AD.from_cos(cos, labels)
    assert rv["branch"].tolist()[:2] == [True, False]
    ref = reference_loop(cos, labels, 0.5, AD.ALPHA, AD.SIGMA, 64.0)
    assert torch.equal(good, ref)
    kernel_view, rk = AD.from_cos(cos, labels, thresh=t32)  # the fp32 comparison of the kernel
    assert torch.equal(kernel_view, ref) and rk["branch"].tolist() == rv["branch"].tolist()
    bad, rb = AD.from_cos(cos, labels, thresh=up)
    assert rb["branch"].tolist()[:2] == [False, False]
    shift = float((bad - ref)[0, labels[0]].abs()) / 64.0
    print("a moves by", shift)
    assert 0.11 < shift < 0.125 and not float((bad - ref).abs().max()) < 1e-3


# ------------------------------------------------------------------------------------------------ the module


def test_head_keeps_the_reference_layout():
    """Constructor (feat_dim, num_class, margin = 0.5, scale = 64), parameter ``weight`` [N, D] uniform within +-1/sqrt(D)
    (the reference's reset_parameters), the reference's attributes, a state dict with the key ``weight`` alone, the default
    repr, attributes read on every call, out-of-range labels, the empty batch on the host."""
    from head.metrics import ArcNegFace
    sig = inspect.signature(ArcNegFace.__init__)
    E = inspect.Parameter.empty
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("feat_dim", E), ("num_class", E), ("margin", 0.5), ("scale", 64)]
    torch.manual_seed(0)
    h = ArcNegFace(512, 10)
    assert list(h.state_dict()) == ["weight"] and [n for n, _ in h.named_parameters()] == ["weight"]
    assert list(h.buffers()) == [] and tuple(h.weight.shape) == (10, 512)
    stdv = 1.0 / math.sqrt(512)
    assert float(h.weight.detach().abs().max()) <= stdv and float(h.weight.detach().abs().max()) > 0.9 * stdv
    assert repr(h) == "ArcNegFace()"
    assert (h.feat_dim, h.num_class, h.margin, h.scale, h.alpha, h.sigma) == (512, 10, 0.5, 64, 1.2, 2)
    assert (h.thresh, h.mm) == (math.cos(math.pi - 0.5), math.sin(math.pi - 0.5) * 0.5)
    torch.manual_seed(0)
    again = ArcNegFace(512, 10)
    assert torch.equal(again.weight, h.weight)
    again.reset_parameters()
    assert not torch.equal(again.weight, h.weight)
    h2 = ArcNegFace(16, 5, margin=0.3, scale=32)
    assert (h2.margin, h2.scale, h2.thresh) == (0.3, 32, math.cos(math.pi - 0.3))
    y = torch.tensor([0, 9, 3])
    x = synth.normal(3, "an.x", (3, 512)) / 512 ** 0.5 + 0.9 * torch.nn.functional.normalize(h.weight.detach()[y])
    x[2] = -3.0 * h.weight.detach()[3] + 0.01 * x[2]  # gt near -1: the linear branch
    out = h(x, y)
    assert out.shape == (3, 10) and out.device.type == "cpu"
    seen = [out]
    for name, v in (("alpha", 1.0), ("sigma", 3), ("scale", 16.0), ("margin", 0.3), ("mm", 0.5), ("thresh", 2.0)):
        setattr(h, name, v)  # plain attributes, read on every call
        seen.append(h(x, y))
        assert not torch.equal(seen[-1], seen[-2]), name
    for bad in (10, -1):  # the reference's Python indexing would wrap -1 to the last class
        with pytest.raises(RuntimeError, match="out of bounds"):
            h(x, torch.tensor([0, bad, 3]))
    assert h(x[:0], y[:0]).shape == (0, 10)
    from util.utils import separate_irse_bn_paras
    bn, rest = separate_irse_bn_paras(h)
    assert bn == [] and len(rest) == 1 and rest[0] is h.weight
    h3 = ArcNegFace(512, 10)
    h3.load_state_dict(h.state_dict())
    assert torch.equal(h3.weight, h.weight)


# ------------------------------------------------------------------------------------------------ the C ABI, train.py


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    assert _lib.protos["fr_arcneg_apply"][2] == ["cos", "label", "rowv", "out", "rows", "N", "ld", "thresh", "margin", "mm",
                                                 "alpha", "sigma", "s", "stream"]
    assert _lib.protos["fr_arcneg_bwd"][2] == ["g", "cos", "label", "rowv", "gcos", "rows", "N", "ld", "ldg", "alpha", "sigma",
                                               "s", "stream"]
    for name in ("ARCNEG", "arcneg_forward", "arcneg_backward", "ArcNegHeadFn", "arcneg_head", "arcneg_thresh32"):
        assert hasattr(FRF, name)
    assert FRF.ARCNEG == 11 and FRF.AM_SOFTMAX_N == 10 and FRF.MV_SOFTMAX == 8
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frhip.h")).read()
    at = header.index("ArcNegFace (head/metrics.py:394-433)")
    assert at < header.index("int fr_arcneg_apply(") < header.index("int fr_arcneg_bwd(")
    assert ":418-433" in header[at:header.index("int fr_arcneg_apply(")]  # each declaration cites its reference lines
    assert ":418-433" in header[header.index("int fr_arcneg_apply("):header.index("int fr_arcneg_bwd(")]
    assert "NaN" in header[at:header.index("int fr_arcneg_bwd(")] and "outside [0, N)" in header[at:header.index("int fr_arcneg_bwd(")]


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: empty shapes, row pitches that are too short or not multiples of 4."""
    from frhip import _lib
    lib = _lib.lib
    apply_ = lambda r, n, ld: lib.fr_arcneg_apply(None, None, None, None, r, n, ld, -0.8775826, 0.5, 0.2397, 1.2, 2.0, 64.0, None)  # noqa: E731
    assert apply_(0, 100, 100) == -1 and apply_(8, 0, 100) == -1 and apply_(8, 101, 100) == -1 and apply_(8, 101, 102) == -1
    assert apply_(-1, 100, 100) == -1 and apply_(8, 100, 96) == -1
    assert b"fr_arcneg_apply" in lib.fr_last_error_string()
    bwd = lambda r, n, ld, ldg: lib.fr_arcneg_bwd(None, None, None, None, None, r, n, ld, ldg, 1.2, 2.0, 64.0, None)  # noqa: E731
    assert bwd(0, 100, 100, 128) == -1 and bwd(8, 0, 100, 128) == -1 and bwd(8, 100, 100, 96) == -1
    assert bwd(8, 100, 98, 128) == -1 and bwd(8, 100, 96, 128) == -1 and bwd(8, 100, 100, 126) == -1
    assert b"fr_arcneg_bwd" in lib.fr_last_error_string()


def test_device_entry_refuses_host_tensors():
    """No quiet fall-back: the functional entry is the HIP path and says so when handed host tensors."""
    from frhip import _lib
    from frhip import functional as FRF
    x, w = torch.zeros(2, 16), torch.ones(5, 16)
    with pytest.raises(_lib.FrhipError):  # the empty batch launches nothing and still says so
        FRF.arcneg_head(x[:0], w, torch.tensor([], dtype=torch.long), 64.0, -0.8775826, 0.5, 0.2397, 1.2, 2.0)


def test_train_py_takes_the_name_and_refuses_the_sharded_head():
    """train.py builds ArcNegFace as the last head inside the fork_rng block and raises NotImplementedError, word for word
    the siblings' sentence, for SHARDED_HEAD with ArcNegFace before anything is built; NOT_SHARDED keeps its six keys (the
    name lives in a second mapping), and the other heads pass or fail that check as before."""
    import train
    with pytest.raises(NotImplementedError) as e:
        train.check_head_config(dict(HEAD_NAME="ArcNegFace", SHARDED_HEAD=True))
    assert str(e.value) == REFUSAL
    train.check_head_config(dict(HEAD_NAME="ArcNegFace", SHARDED_HEAD=False))
    train.check_head_config(dict(HEAD_NAME="ArcNegFace"))
    assert sorted(train.NOT_SHARDED) == ["AM_Softmax", "AdaCos", "CircleLoss", "MV_Softmax", "MagFace", "NPCFace"]
    assert list(train.NOT_SHARDED_ROW_VALUE) == ["ArcNegFace"]
    for name in train.NOT_SHARDED:
        with pytest.raises(NotImplementedError, match=name):
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
        train.check_head_config(dict(HEAD_NAME=name))
    for name in ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace"):
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
    src = open(train.__file__).read()
    fork = src.index("with torch.random.fork_rng(devices=[])")
    last = src.index('heads["ArcNegFace"] = ArcNegFace(emb, num_class)')
    assert fork < src.index('heads["AM_Softmax"]') < last < src.index("head = heads[cfg")
    assert "heads[" not in src[last + 10:src.index("head = heads[cfg")]  # the last line of the block
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "ArcNegFace" in common
