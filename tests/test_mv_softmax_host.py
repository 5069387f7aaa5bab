"""CPU checks of the MV_Softmax head (reference head/metrics.py:555-590): the host path reproduces the reference's own
vectors (g22_mv_softmax, tests/golden/make_golden_mv_softmax.py), four deliberately wrong variants each miss them, the module
keeps the reference's layout, the C ABI of the HIP path is declared, exported and checks its arguments before any launch, and
train.py takes the name and refuses the class-sharded head for it."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import mv_softmax_data as MD
from frhip import synth

CASES = ("rand_am", "rand_arc", "built_am", "built_arc", "built_am_m05", "built_arc_m05")
BUILT = CASES[2:]
NEW_ENTRIES = ("fr_mv_softmax_apply", "fr_mv_softmax_bwd")
B, D, N = 8, 512, 100


@pytest.fixture(scope="module")
def g22(golden_dir):
    return np.load(os.path.join(golden_dir, "g22_mv_softmax.npz"))


def scalars(g, tag):
    """(is_am, margin, mv_weight, scale) of a g22 case."""
    return (bool(g[tag + ".is_am"]),) + tuple(float(g["%s.%s" % (tag, n)]) for n in ("margin", "mv_weight", "scale"))


def inputs_of(g, tag):
    """(x, weight, label, gout) of a g22 case, regenerated from synth; the file keeps the labels as a check."""
    is_am, margin, _, _ = scalars(g, tag)
    if tag.startswith("built"):
        x, k, label, gout = MD.built(synth, tag, B, D, N, is_am, margin)
    else:
        x, k, label, gout = MD.random_case(synth, tag, B, D, N)
    assert torch.equal(label, torch.from_numpy(g[tag + ".label"]))
    return x, k, label, gout


def make_head(g, tag, k):
    from head.metrics import MV_Softmax
    is_am, margin, w, s = scalars(g, tag)
    head = MV_Softmax(D, N, is_am, margin=margin, mv_weight=w, scale=s)
    with torch.no_grad():
        head.weight.copy_(k)
    return head


class _ScaleGrad(torch.autograd.Function):
    """The identity with its gradient multiplied by ``f`` where ``mask`` is set."""

    @staticmethod
    def forward(ctx, t, mask, f):
        ctx.save_for_backward(mask)
        ctx.f = f
        return t.clone()

    @staticmethod
    def backward(ctx, g):
        mask, = ctx.saved_tensors
        return torch.where(mask, g * ctx.f, g), None, None


def variant(x, k, label, is_am, margin, w, s, am_branch_at_zero=False, no_offset=False, arcface_fallback=False,
            hard_grad_s=False):
    """The head's arithmetic written out once more with one deliberate mistake per flag."""
    c = torch.mm(F.normalize(x), F.normalize(k, dim=0))
    at = label.view(-1, 1)
    gt = c.gather(1, at)
    if is_am:
        thr = gt - margin
        final = torch.where(gt > (0.0 if am_branch_at_zero else margin), gt - margin, gt)
    else:
        thr = gt * math.cos(margin) - torch.sqrt(1.0 - torch.pow(gt, 2)) * math.sin(margin)
        if arcface_fallback:  # ArcFace's rule (head/metrics.py:124-127) in place of ``gt > 0, else gt``
            final = torch.where(gt > math.cos(math.pi - margin), thr, gt - math.sin(margin) * margin)
        else:
            final = torch.where(gt > 0.0, thr, gt)
    hard = c > thr
    lifted = w * c + (0.0 if no_offset else w - 1.0)
    if hard_grad_s:  # the value of w c + w - 1 with the gradient of c
        lifted = _ScaleGrad.apply(lifted, hard, 1.0 / w)
    return torch.where(hard, lifted, c).scatter(1, at, final) * s


def errors(g, tag, y, gx, gw):
    """{name: (error, bar)}: logits absolute (1e-3), gradients and the norm of the whole weight gradient relative to the
    reference's, max(5e-3, 8 x the reference's own fp32-vs-float64 deviation)."""
    idx = torch.from_numpy(g[tag + ".gw_index"])
    res = {"logits": (float((y.detach() - torch.from_numpy(g[tag + ".logits"])).abs().max()), 1e-3)}
    for name, got in (("gx", gx), ("gw", gw.index_select(1, idx))):
        ref = torch.from_numpy(g[tag + "." + name])
        assert got.shape == ref.shape
        res[name] = (float((got - ref).abs().max() / ref.abs().max()), max(5e-3, 8 * float(g[tag + ".dev." + name])))
    res["gw_norm"] = (abs(float(gw.double().norm()) / float(g[tag + ".gw_norm"]) - 1),
                      max(5e-3, 8 * float(g[tag + ".dev.gw"])))
    return res


@pytest.mark.parametrize("tag", CASES)
def test_host_path_reproduces_the_reference(g22, tag):
    """Logits within 1e-3 absolute, gradients within max(5e-3, 8 x the reference's own fp32-vs-float64 deviation) of
    max|ref| per tensor, the norm of the whole weight gradient likewise (the fixture's bars)."""
    x, k, label, gout = inputs_of(g22, tag)
    head = make_head(g22, tag, k)
    x.requires_grad_(True)
    y = head(x, label)
    gx, gw = torch.autograd.grad(y, [x, head.weight], gout)
    res = errors(g22, tag, y, gx, gw)
    print(tag, res)
    for name, (err, bar) in res.items():
        assert err < bar, (tag, name, err, bar)
    assert list(head.state_dict()) == ["weight"]
    assert float(g22[tag + ".dev.logits"]) < 1e-6


def test_fixture_covers_the_four_kinds_of_row(g22):
    """Every built case has rows without a hard negative, rows with two planted hard ones (and an easy one above the bulk),
    rows with 0 < gt < margin and rows in the gt <= 0 branch (every negative hard in both), none near a decision boundary,
    on this test's own float64 restatement as in the maker; the recorded gt, thr and count are that restatement's.  The
    random cases are all hard (which is why the cases are built)."""
    for tag in CASES:
        x, k, label, _ = inputs_of(g22, tag)
        is_am, margin, w, s = scalars(g22, tag)
        assert is_am == tag.split("_")[1].startswith("am")
        st = MD.assert_covers(x, k, label, is_am, margin) if tag in BUILT else MD.stats64(x, k, label, is_am, margin)
        assert tuple(st[n] for n in MD.KINDS) == tuple(int(g22["%s.rows_%s" % (tag, n)]) for n in MD.KINDS)
        assert torch.equal(st["count"], torch.from_numpy(g22[tag + ".count"]))
        for name in ("gt", "thr"):
            assert float((st[name] - torch.from_numpy(g22["%s.%s" % (tag, name)])).abs().max()) < 1e-12
        if tag in BUILT:
            assert tuple(st[n] for n in MD.KINDS) == (2, 2, 2, 2) and st["min_gap"] >= 0.04
            # the easy planted negative of a planted row lies between the bulk and thr
            c = F.normalize(x.double()) @ F.normalize(k.double(), dim=0)
            easy = (c[1] < st["thr"][1]) & (c[1] > st["thr"][1] - 0.06)
            assert int(easy.sum()) == 1
        else:
            assert bool((st["count"] == N - 1).all())
        assert (margin, w, s) == ((0.5, 1.3, 64.0) if tag.endswith("_m05") else (0.35, 1.12, 32.0))


@pytest.mark.parametrize("flag", ["am_branch_at_zero", "no_offset", "arcface_fallback", "hard_grad_s"])
def test_negative_controls_miss_the_fixture(g22, flag):
    """The written-out variant meets the bars on every case with no flag set, and misses them on at least one built case
    with any single one: the AM form branching on gt > 0, hard negatives as w c without + w - 1, the arc form with ArcFace's
    fallback (gt > cos(pi - m), else gt - mm), hard negatives with gradient s instead of s w (backward only: the logits
    still match)."""

    def run(tag, **flags):
        x, k, label, gout = inputs_of(g22, tag)
        xx = x.clone().requires_grad_(True)
        kk = k.clone().requires_grad_(True)
        y = variant(xx, kk, label, *scalars(g22, tag), **flags)
        gx, gw = torch.autograd.grad(y, [xx, kk], gout)
        return errors(g22, tag, y, gx, gw)

    for tag in CASES:
        assert all(err < bar for err, bar in run(tag).values()), (tag, run(tag))
    bad = {tag: run(tag, **{flag: True}) for tag in BUILT}
    print(flag, bad)
    missed = [tag for tag, res in bad.items() if any(not err < bar for err, bar in res.values())]  # NaN misses too
    assert missed, (flag, bad)
    if flag == "hard_grad_s":  # a backward-only mistake: the logits still match
        assert all(res["logits"][0] < res["logits"][1] for res in bad.values())
        assert any(not res["gx"][0] < res["gx"][1] for res in bad.values())


def test_head_keeps_the_reference_layout():
    """Constructor (feat_dim, num_class, is_am required; margin = 0.35, mv_weight = 1.12, scale = 32), parameter ``weight``
    [D, N] with unit columns (uniform, renormed), the reference's attributes (the unused ``threshold`` and ``mm`` among
    them), a state dict with the key ``weight`` alone, attributes read on every call, the empty batch on the host."""
    import inspect
    from head.metrics import MV_Softmax
    sig = inspect.signature(MV_Softmax.__init__)
    E = inspect.Parameter.empty
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("feat_dim", E), ("num_class", E), ("is_am", E), ("margin", 0.35), ("mv_weight", 1.12), ("scale", 32)]
    with pytest.raises(TypeError):
        MV_Softmax(512, 10)
    torch.manual_seed(0)
    h = MV_Softmax(512, 10, True)
    assert list(h.state_dict()) == ["weight"] and [n for n, _ in h.named_parameters()] == ["weight"]
    assert list(h.buffers()) == [] and tuple(h.weight.shape) == (512, 10)
    assert float((h.weight.detach().norm(dim=0) - 1).abs().max()) < 1e-4
    assert (h.margin, h.mv_weight, h.scale, h.is_am) == (0.35, 1.12, 32, True)
    assert (h.cos_m, h.sin_m) == (math.cos(0.35), math.sin(0.35))
    assert (h.threshold, h.mm) == (math.cos(math.pi - 0.35), math.sin(0.35) * 0.35)
    h2 = MV_Softmax(16, 5, False, margin=0.5, mv_weight=1.3, scale=64.0)
    assert (h2.margin, h2.mv_weight, h2.scale, h2.is_am, h2.cos_m) == (0.5, 1.3, 64.0, False, math.cos(0.5))
    y = torch.tensor([0, 9, 3])
    x = synth.normal(3, "mv.x", (3, 512)) / 512 ** 0.5 + 0.2 * h.weight.detach()[:, y].t()  # gt ~ 0.2, every negative hard
    out = h(x, y)
    assert out.shape == (3, 10) and out.device.type == "cpu"
    seen = [out]
    for name, v in (("mv_weight", 1.3), ("margin", 0.1), ("scale", 16.0), ("is_am", False), ("cos_m", math.cos(0.6))):
        setattr(h, name, v)  # plain attributes, read on every call; the arc form reads cos_m / sin_m, not margin
        seen.append(h(x, y))
        assert not torch.equal(seen[-1], seen[-2]), name
    h.margin = 0.9
    assert torch.equal(h(x, y), seen[-1])  # is_am false: margin itself is not read
    assert h(x[:0], y[:0]).shape == (0, 10)
    # the weight-decay group of train.py: the weight is not a batch-norm parameter
    from util.utils import separate_irse_bn_paras
    bn, rest = separate_irse_bn_paras(h)
    assert bn == [] and len(rest) == 1 and rest[0] is h.weight
    h3 = MV_Softmax(512, 10, True)
    h3.load_state_dict(h.state_dict())
    assert torch.equal(h3.weight, h.weight)


def test_from_cos_is_the_head_on_valid_labels(g22):
    """``from_cos`` (the restatement the entry-point tests compare with) on the float64 cosines of a built case equals the
    host path in float64, logits and the gradient with respect to the cosines through to x."""
    for tag in ("built_am", "built_arc_m05"):
        x, k, label, gout = inputs_of(g22, tag)
        is_am, margin, w, s = scalars(g22, tag)
        head = make_head(g22, tag, k).double()
        xa = x.double().requires_grad_(True)
        ya = head(xa, label)
        xb = x.double().requires_grad_(True)
        yb, _ = MD.from_cos(F.normalize(xb) @ F.normalize(k.double(), dim=0), label, is_am, margin, w, s)
        assert float((ya - yb).detach().abs().max()) < 1e-12
        ga, = torch.autograd.grad(ya, xa, gout.double())
        gb, = torch.autograd.grad(yb, xb, gout.double())
        assert float((ga - gb).abs().max()) < 1e-10 * float(ga.abs().max())


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    for name in ("MV_SOFTMAX", "mv_softmax_forward", "mv_softmax_backward", "MVSoftmaxHeadFn", "mv_softmax_head"):
        assert hasattr(FRF, name)
    assert FRF.MV_SOFTMAX == 8 and FRF.NPCFACE == 7 and FRF.ADACOS == 6
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frhip.h")).read()
    at = header.index("MV_Softmax (head/metrics.py:555-590)")
    assert at < header.index("int fr_mv_softmax_apply(") < header.index("int fr_mv_softmax_bwd(")
    assert ":576-589" in header[at:header.index("int fr_mv_softmax_bwd(")]  # each declaration cites its reference lines


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: empty shapes, row pitches that are too short or not multiples of 4."""
    from frhip import _lib
    lib = _lib.lib
    apply_ = lambda r, n, ld: lib.fr_mv_softmax_apply(None, None, None, None, r, n, ld, 1, 0.35, 0.0, 1.12, 32.0, None)  # noqa: E731
    assert apply_(0, 100, 100) == -1 and apply_(8, 0, 100) == -1 and apply_(8, 101, 100) == -1 and apply_(8, 101, 102) == -1
    assert apply_(-1, 100, 100) == -1 and apply_(8, 100, 96) == -1
    assert b"fr_mv_softmax_apply" in lib.fr_last_error_string()
    bwd = lambda r, n, ld, ldg: lib.fr_mv_softmax_bwd(None, None, None, None, None, r, n, ld, ldg, 1.12, 32.0, None)  # noqa: E731
    assert bwd(0, 100, 100, 128) == -1 and bwd(8, 0, 100, 128) == -1 and bwd(8, 100, 100, 96) == -1
    assert bwd(8, 100, 98, 128) == -1 and bwd(8, 100, 96, 128) == -1 and bwd(8, 100, 100, 126) == -1
    assert b"fr_mv_softmax_bwd" in lib.fr_last_error_string()


def test_device_entry_refuses_host_tensors():
    """No quiet fall-back: the functional entry is the HIP path and says so when handed host tensors."""
    from frhip import _lib
    from frhip import functional as FRF
    x, k = torch.zeros(2, 16), torch.ones(16, 5)
    with pytest.raises(_lib.FrhipError):  # the empty batch launches nothing and still says so
        FRF.mv_softmax_head(x[:0], k, torch.tensor([], dtype=torch.long), 32.0, True, 0.35, 0.0, 1.12)


def test_train_py_takes_the_name_and_refuses_the_sharded_head():
    """train.py builds MV_Softmax in its ``heads`` table off the generator, after NPCFace, and raises NotImplementedError
    for SHARDED_HEAD with MV_Softmax before anything is built; the other eight heads pass or fail that check as before."""
    import train
    with pytest.raises(NotImplementedError, match="MV_Softmax"):
        train.check_head_config(dict(HEAD_NAME="MV_Softmax", SHARDED_HEAD=True))
    train.check_head_config(dict(HEAD_NAME="MV_Softmax", SHARDED_HEAD=False))
    train.check_head_config(dict(HEAD_NAME="MV_Softmax"))
    train.check_head_config(dict(HEAD_NAME="MV_Softmax", MV_IS_AM=False))
    for name in ("MagFace", "AdaCos", "NPCFace"):
        with pytest.raises(NotImplementedError, match=name):
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
        train.check_head_config(dict(HEAD_NAME=name))
    for name in ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace"):
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
    src = open(train.__file__).read()
    fork = src.index("with torch.random.fork_rng(devices=[])")
    assert fork < src.index('heads["NPCFace"]') \
        < src.index('heads["MV_Softmax"] = MV_Softmax(emb, num_class, cfg.get("MV_IS_AM", True))') \
        < src.index("head = heads[cfg")
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "MV_Softmax" in common and "MV_IS_AM" in common
