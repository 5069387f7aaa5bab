"""CPU checks of the NPCFace head (reference head/metrics.py:592-636): the host path reproduces the reference's own vectors
(g21_npcface, tests/golden/make_golden_npcface.py), four deliberately wrong variants each miss them, the module keeps the
reference's layout, the C ABI of the HIP path is declared, exported and checks its arguments before any launch, and train.py
takes the name and refuses the class-sharded head for it."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import npcface_data as ND
from frhip import synth

CASES = ("rand", "built", "built_m03", "built_t12")
BUILT = CASES[1:]
NEW_ENTRIES = ("fr_npcface_rows", "fr_npcface_apply", "fr_npcface_bwd")
ATTRS = ("m0", "m1", "t", "a")
B, D, N = 8, 512, 100


@pytest.fixture(scope="module")
def g21(golden_dir):
    return np.load(os.path.join(golden_dir, "g21_npcface.npz"))


def inputs_of(g, tag):
    """(x, kernel, label, gout) of a g21 case, regenerated from synth; the file keeps the labels as a check."""
    x, k, label, gout = (ND.built if tag.startswith("built") else ND.random_case)(synth, tag, B, D, N)
    assert torch.equal(label, torch.from_numpy(g[tag + ".label"]))
    return x, k, label, gout


def make_head(g, tag, k):
    from head.metrics import NPCFace
    head = NPCFace(D, N, margin=float(g[tag + ".margin"]), scale=float(g[tag + ".scale"]))
    for name in ATTRS:
        setattr(head, name, float(g["%s.%s" % (tag, name)]))
    with torch.no_grad():
        head.kernel.copy_(k)
    return head


def variant(x, k, label, margin, s, m0, m1, t, a, count_label=False, no_clamp=False, fixed_m0=False, grad_newm=False):
    """The head's arithmetic written out once more with one deliberate mistake per flag."""
    c = torch.mm(F.normalize(x), F.normalize(k, dim=0)).clamp(-1, 1)
    at = label.view(-1, 1)
    gt = c.gather(1, at)
    sin_theta = torch.sqrt(1.0 - torch.pow(gt, 2))
    ctm = gt * math.cos(margin) - sin_theta * math.sin(margin)
    hard = (c > ctm).to(c.dtype)
    if not count_label:
        hard = hard.scatter(1, at, 0)
    count = hard.sum(1, keepdim=True)
    if not no_clamp:
        count = count.clamp(1, c.shape[1])
    avg = (hard * c).sum(1, keepdim=True) / count
    if not grad_newm:
        avg = avg.detach()
    newm = m0 + m1 * avg
    if fixed_m0:
        newm = torch.full_like(avg, m0)
    final = torch.where(gt > 0, gt * torch.cos(newm) - sin_theta * torch.sin(newm), gt)
    out = torch.where(c > ctm, t * c + a, c).scatter(1, at, final)
    return out * s


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
def test_host_path_reproduces_the_reference(g21, tag):
    """Logits under 1e-5 absolute, gradients under max(1e-5, 8 x the reference's own fp32-vs-float64 deviation), the norm of
    the whole kernel gradient within 1e-5 (the bars of test_curricular_host.py)."""
    x, k, label, gout = inputs_of(g21, tag)
    head = make_head(g21, tag, k)
    x.requires_grad_(True)
    y = head(x, label)
    gx, gw = torch.autograd.grad(y, [x, head.kernel], gout)
    for name, (err, bar) in errors(g21, tag, y, gx, gw).items():
        assert err < bar, (tag, name, err, bar)
    assert abs(float(gw.double().norm()) / float(g21[tag + ".gw_norm"]) - 1) < 1e-5
    assert list(head.state_dict()) == ["kernel"]


def test_fixture_covers_the_three_kinds_of_row(g21):
    """Every built case has rows in the gt <= 0 branch (all negatives hard), rows without a hard negative (the clamp of the
    count) and rows with planted ones (avg ~ 0.8, the margin far from m0), none near a decision boundary, on this test's
    own float64 restatement as in the maker; the recorded avg and count are that restatement's.  The random case is all
    hard with avg ~ 0 (which is why the cases are built)."""
    for tag in CASES:
        x, k, label, _ = inputs_of(g21, tag)
        margin = float(g21[tag + ".margin"])
        st = ND.assert_covers(x, k, label, margin) if tag in BUILT else ND.stats64(x, k, label, margin)
        assert (st["negative"], st["none"], st["some"]) == tuple(int(g21["%s.rows_%s" % (tag, n)])
                                                                 for n in ("negative", "none", "some"))
        assert torch.equal(st["count"], torch.from_numpy(g21[tag + ".count"]))
        assert float((st["avg"] - torch.from_numpy(g21[tag + ".avg"])).abs().max()) < 1e-12
        if tag in BUILT:
            planted = st["count"][(st["gt"] > 0) & (st["count"] > 0)]
            assert bool(((planted == 2) | (planted == 3)).all()) and float(st["avg"].max()) > 0.75
        else:
            assert bool((st["count"] == N - 1).all()) and float(st["avg"].abs().max()) < 0.02
    assert float(g21["built_m03.margin"]) == pytest.approx(0.3)
    assert [float(g21["built_t12." + n]) for n in ATTRS] == pytest.approx([0.3, 0.3, 1.2, 0.1])
    assert [float(g21["built." + n]) for n in ATTRS] == pytest.approx([0.4, 0.2, 1.1, 0.2])


@pytest.mark.parametrize("flag", ["count_label", "no_clamp", "fixed_m0", "grad_newm"])
def test_negative_controls_miss_the_fixture(g21, flag):
    """The written-out variant meets the bars on every case with no flag set, and misses them on at least one built case
    with any single one: the label column counted among the hard negatives, no clamp of the count at 1 (0 / 0 on the rows
    without hard negatives), the margin fixed at m0, a gradient let through newm."""

    def run(tag, **flags):
        x, k, label, gout = inputs_of(g21, tag)
        xx = x.clone().requires_grad_(True)
        kk = k.clone().requires_grad_(True)
        y = variant(xx, kk, label, float(g21[tag + ".margin"]), float(g21[tag + ".scale"]),
                    *(float(g21["%s.%s" % (tag, n)]) for n in ATTRS), **flags)
        gx, gw = torch.autograd.grad(y, [xx, kk], gout)
        return errors(g21, tag, y, gx, gw)

    for tag in CASES:
        assert all(err < bar for err, bar in run(tag).values()), (tag, run(tag))
    bad = {tag: run(tag, **{flag: True}) for tag in BUILT}
    print(flag, bad)
    missed = [tag for tag, res in bad.items() if any(not err < bar for err, bar in res.values())]  # NaN misses too
    assert missed, (flag, bad)
    if flag == "grad_newm":  # a backward-only mistake: the logits still match
        assert all(res["logits"][0] < res["logits"][1] for res in bad.values())
        assert any(not res["gx"][0] < res["gx"][1] for res in bad.values())


def test_head_keeps_the_reference_layout():
    """Constructor (feat_dim = 512, num_class = 86876, margin = 0.5, scale = 64), parameter ``kernel`` [D, N] with unit
    columns (uniform, renormed), the reference's attributes, a state dict with the key ``kernel`` alone."""
    import inspect
    from head.metrics import NPCFace
    sig = inspect.signature(NPCFace.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [
        ("feat_dim", 512), ("num_class", 86876), ("margin", 0.5), ("scale", 64)]
    torch.manual_seed(0)
    h = NPCFace(512, 10)
    assert list(h.state_dict()) == ["kernel"] and [n for n, _ in h.named_parameters()] == ["kernel"]
    assert list(h.buffers()) == [] and tuple(h.kernel.shape) == (512, 10)
    assert float((h.kernel.detach().norm(dim=0) - 1).abs().max()) < 1e-4
    assert (h.margin, h.scale, h.num_class) == (0.5, 64, 10)
    assert (h.m0, h.m1, h.t, h.a) == (0.40, 0.20, 1.10, 0.20)
    assert (h.cos_m, h.sin_m) == (math.cos(0.5), math.sin(0.5))
    assert (h.cos_m0, h.sin_m0) == (math.cos(0.40), math.sin(0.40))
    h2 = NPCFace(16, 5, margin=0.3, scale=30.0)
    assert (h2.margin, h2.scale, h2.cos_m) == (0.3, 30.0, math.cos(0.3))
    x, y = synth.normal(3, "npc.x", (3, 512)), torch.tensor([0, 9, 3])
    out = h(x, y)
    assert out.shape == (3, 10) and out.device.type == "cpu"
    h.t, h.a = 1.3, 0.05  # plain attributes, read on every call
    assert not torch.equal(h(x, y), out)
    assert h(x[:0], y[:0]).shape == (0, 10)
    # the weight-decay group of train.py: the kernel is not a batch-norm parameter
    from util.utils import separate_irse_bn_paras
    bn, rest = separate_irse_bn_paras(h)
    assert bn == [] and len(rest) == 1 and rest[0] is h.kernel
    h3 = NPCFace(512, 10)
    h3.load_state_dict(h.state_dict())
    assert torch.equal(h3.kernel, h.kernel)


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    for name in ("NPCFACE", "npcface_forward", "npcface_backward", "NPCFaceHeadFn", "npcface_head"):
        assert hasattr(FRF, name)
    assert FRF.NPCFACE == 7 and FRF.ADACOS == 6


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: empty shapes, row pitches that are too short or not multiples of 4."""
    from frhip import _lib
    lib = _lib.lib
    rows = lambda r, n, ld: lib.fr_npcface_rows(None, None, None, r, n, ld, 0.8, 0.4, 0.4, 0.2, None)  # noqa: E731
    assert rows(0, 100, 100) == -1 and rows(8, 0, 100) == -1 and rows(8, 101, 100) == -1 and rows(8, 101, 102) == -1
    assert b"fr_npcface_rows" in lib.fr_last_error_string()
    apply_ = lambda r, n, ld: lib.fr_npcface_apply(None, None, None, None, r, n, ld, 1.1, 0.2, 64.0, None)  # noqa: E731
    assert apply_(0, 100, 100) == -1 and apply_(8, 101, 101) == -1 and apply_(8, 100, 96) == -1
    assert b"fr_npcface_apply" in lib.fr_last_error_string()
    bwd = lambda r, n, ld, ldg: lib.fr_npcface_bwd(None, None, None, None, None, r, n, ld, ldg, 1.1, 64.0, None)  # noqa: E731
    assert bwd(0, 100, 100, 128) == -1 and bwd(8, 100, 100, 96) == -1 and bwd(8, 100, 98, 128) == -1
    assert bwd(8, 100, 100, 126) == -1 and b"fr_npcface_bwd" in lib.fr_last_error_string()


def test_device_entry_refuses_host_tensors():
    """No quiet fall-back: the functional entry is the HIP path and says so when handed host tensors."""
    from frhip import _lib
    from frhip import functional as FRF
    x, k = torch.zeros(2, 16), torch.ones(16, 5)
    with pytest.raises(_lib.FrhipError):  # the empty batch launches nothing and still says so
        FRF.npcface_head(x[:0], k, torch.tensor([], dtype=torch.long), 64.0, 0.8, 0.4, 0.4, 0.2, 1.1, 0.2)


def test_train_py_takes_the_name_and_refuses_the_sharded_head():
    """train.py builds NPCFace in its ``heads`` table off the generator, after AdaCos, and raises NotImplementedError for
    SHARDED_HEAD with NPCFace before anything is built; the other heads pass that check as before."""
    import train
    with pytest.raises(NotImplementedError, match="NPCFace"):
        train.check_head_config(dict(HEAD_NAME="NPCFace", SHARDED_HEAD=True))
    train.check_head_config(dict(HEAD_NAME="NPCFace", SHARDED_HEAD=False))
    train.check_head_config(dict(HEAD_NAME="NPCFace"))
    for name in ("MagFace", "AdaCos"):
        with pytest.raises(NotImplementedError, match=name):
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
    for name in ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace"):
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
    src = open(train.__file__).read()
    fork = src.index("with torch.random.fork_rng(devices=[])")
    assert fork < src.index('heads["AdaCos"]') < src.index('heads["NPCFace"] = NPCFace(emb, num_class') \
        < src.index("head = heads[cfg")
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "NPCFace" in common
