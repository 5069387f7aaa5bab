"""CPU checks of the AdaCos head (reference head/metrics.py:336-369): the host path reproduces the reference's own vectors
(g20_adacos, tests/golden/make_golden_adacos.py) including the scale it moves on every call, three deliberately wrong
variants each miss them, the module keeps the reference's layout with ``scale`` as a non-persistent buffer, the C ABI of the
HIP path is declared, exported and checks its arguments before any launch, and train.py takes the name and refuses it
together with SHARDED_HEAD."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import adacos_data as AD
from frhip import synth

NEW_ENTRIES = ("fr_adacos_rows", "fr_adacos_scale", "fr_adacos_apply")
D, N = 512, 100
# the scale against the fixture's: fp32 sums in another order than the reference's build may take (8 ulp of fp32); float64
SCALE_BAR = {torch.float32: 1e-6, torch.float64: 1e-12}


@pytest.fixture(scope="module")
def g20(golden_dir):
    return np.load(os.path.join(golden_dir, "g20_adacos.npz"))


def calls_of(g, tag):
    """The calls of a g20 case, regenerated from synth; the file keeps the labels and the upstream gradient as a check."""
    calls = AD.batches(synth, tag, D, N)
    for name, (x, W, label, gout), _, _ in calls:
        assert torch.equal(label, torch.from_numpy(g[name + ".label"]))
        assert torch.equal(gout, torch.from_numpy(g[name + ".gout"]))
    return calls


def make_head(W, dtype=torch.float32):
    from head.metrics import AdaCos
    head = AdaCos(D, N)
    with torch.no_grad():
        head.W.copy_(W)
    head = head.to(dtype)
    if dtype == torch.float64:  # .double() converts the buffer's fp32 initial value; the reference starts from the double
        head.scale.fill_(AD.scale0(N))
    return head


def variant(x, W, label, s_old, upper_median=False, with_target=False, old_scale_out=False):
    """The head's arithmetic written out once more with one deliberate mistake per flag; returns (logits, new scale)."""
    c = F.linear(F.normalize(x), F.normalize(W))
    hot = torch.zeros_like(c).scatter_(1, label.view(-1, 1), 1).bool()
    with torch.no_grad():
        e = torch.exp(s_old * c)
        if not with_target:
            e = e.masked_fill(hot, 0.0)
        b_avg = e.sum() / c.shape[0]
        th = torch.sort(torch.acos(c[hot].clamp(-1 + 1e-7, 1 - 1e-7))).values
        n = th.numel()
        med = th[n // 2] if upper_median else th[(n - 1) // 2]
        s_new = torch.log(b_avg) / torch.cos(torch.clamp(med, max=math.pi / 4))
    return (s_old if old_scale_out else s_new) * c, s_new


def errors(g, name, y, gx, gw, scale):
    """{name: (error, bar)}: the bars of test_curricular_host.py -- logits absolute, gradients relative to max|ref| within
    max(1e-5, 8 x the reference's own fp32-vs-float64 deviation) -- and the scale relative, all against the fp32
    reference."""
    idx = torch.from_numpy(g[name + ".gw_index"])
    res = {"logits": (float((y.detach() - torch.from_numpy(g[name + ".logits"])).abs().max()), 1e-5)}
    for k, got in (("gx", gx), ("gw", gw.index_select(0, idx))):
        ref = torch.from_numpy(g[name + "." + k])
        assert got.shape == ref.shape
        res[k] = (float((got - ref).abs().max() / ref.abs().max()), max(1e-5, 8 * float(g["%s.dev.%s" % (name, k)])))
    ref = float(g[name + ".scale"])
    res["scale"] = (abs(float(scale) / ref - 1), SCALE_BAR[torch.float32])
    return res


@pytest.mark.parametrize("tag", ["rand", "built_even", "built_odd"])
def test_host_path_reproduces_the_reference(g20, tag):
    """Logits, both gradients and the scale after the call, in fp32 against the reference's fp32 run and in float64 against
    its float64 run."""
    (name, (x, W, label, gout), _, _), = calls_of(g20, tag)
    head = make_head(W)
    assert float(head.scale) == pytest.approx(AD.scale0(N), rel=1e-7)
    x.requires_grad_(True)
    y = head(x, label)
    gx, gw = torch.autograd.grad(y, [x, head.W], gout)
    for k, (err, bar) in errors(g20, name, y, gx, gw, head.scale).items():
        print(tag, k, err, bar)
        assert err < bar, (tag, k, err, bar)
    assert abs(float(gw.double().norm()) / float(g20[name + ".gw_norm"]) - 1) < 1e-5
    assert tuple(head.scale.shape) == (1,) and head.scale.dtype == torch.float32
    h64 = make_head(W, torch.float64)
    y64 = h64(x.detach().double(), label)
    assert y64.dtype == torch.float64 and h64.scale.dtype == torch.float64
    ref64 = float(g20[name + ".scale64"])
    assert abs(float(h64.scale) / ref64 - 1) < SCALE_BAR[torch.float64], (float(h64.scale), ref64)
    assert float((y64.detach().float() - torch.from_numpy(g20[name + ".logits"])).abs().max()) < 1e-5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_trajectory_of_three_calls(g20, dtype):
    """The scale moves on every call and the next call uses the moved value inside exp: three batches, the recorded scale
    after each; the last call in eval mode under no_grad, where it moves all the same."""
    calls = calls_of(g20, "traj")
    head = make_head(calls[0][1][1], dtype)
    key = ".scale" if dtype == torch.float32 else ".scale64"
    seen = []
    for i, (name, (x, W, label, gout), _, _) in enumerate(calls):
        before = head.scale.clone()
        if i == 2:
            head.eval()
            with torch.no_grad():
                y = head(x.to(dtype), label)
        else:
            y = head(x.to(dtype), label)
        assert not torch.equal(before, head.scale)
        ref = float(g20[name + key])
        assert abs(float(head.scale) / ref - 1) < SCALE_BAR[dtype], (name, float(head.scale), ref)
        assert float((y.detach().float() - torch.from_numpy(g20[name + ".logits"])).abs().max()) < 1e-5
        seen.append(float(head.scale))
    # a head that kept the initial scale inside exp would repeat call 0's arithmetic: the recorded scales differ by 1e-3
    assert abs(seen[1] - seen[0]) > 1e-3 and abs(seen[2] - seen[1]) > 1e-3


def test_fixture_covers_both_branches(g20):
    """Each case takes the branch of min(pi/4, theta_med) it is built for, on this test's own float64 statistics as in the
    maker; so do the sizes the GPU tests build."""
    for tag in AD.CASES:
        s = AD.scale0(N)
        for name, (x, W, label, _), branch, mid_gap in calls_of(g20, tag):
            st = AD.assert_covers(x, W, label, s, branch, mid_gap)
            assert st["theta_med"] == pytest.approx(float(g20[name + ".theta_med"]), abs=1e-12)
            assert st["scale"] == pytest.approx(float(g20[name + ".scale64"]), rel=1e-12)
            s = st["scale"]
    assert float(g20["built_even.theta_med"]) == pytest.approx(0.5, abs=1e-6)
    assert float(g20["built_even.upper_med"]) == pytest.approx(0.6, abs=1e-6)
    assert float(g20["rand.theta_med"]) > 1.4


@pytest.mark.parametrize("flag", ["upper_median", "with_target", "old_scale_out"])
def test_negative_controls_miss_the_fixture(g20, flag):
    """The written-out variant meets g20 with no flag set, and misses its bar by more than 100x with any single one: the
    upper median of the even batch, the target column inside B_avg, the output scaled by the old scale."""
    (name, (x, W, label, gout), _, _), = calls_of(g20, "built_even")

    def run(**flags):
        xx = x.clone().requires_grad_(True)
        ww = W.clone().requires_grad_(True)
        y, s_new = variant(xx, ww, label, torch.tensor(AD.scale0(N), dtype=torch.float32), **flags)
        return errors(g20, name, y, *torch.autograd.grad(y, [xx, ww], gout), s_new)

    assert all(err < bar for err, bar in run().values()), run()
    bad = run(**{flag: True})
    print(flag, bad)
    which = "logits" if flag == "old_scale_out" else "scale"
    assert bad[which][0] > 100 * bad[which][1], (flag, bad)
    if flag == "old_scale_out":  # the buffer itself still moves as it should
        assert bad["scale"][0] < bad["scale"][1]


def test_head_keeps_the_reference_layout():
    """Constructor (feat_dim, num_classes), parameter ``W`` [N, D] from xavier_uniform_, the state dict holds ``W`` alone,
    ``scale`` is a non-persistent one-float buffer that follows .double(), the initial value, ``process_group``."""
    from head.metrics import AdaCos
    torch.manual_seed(0)
    h = AdaCos(512, 10)
    torch.manual_seed(0)
    want = torch.nn.init.xavier_uniform_(torch.empty(10, 512))
    assert torch.equal(h.W.detach(), want)
    assert list(h.state_dict()) == ["W"] and [n for n, _ in h.named_parameters()] == ["W"]
    assert [n for n, _ in h.named_buffers()] == ["scale"] and "scale" in h._non_persistent_buffers_set
    assert tuple(h.scale.shape) == (1,) and h.scale.dtype == torch.float32
    assert float(h.scale) == pytest.approx(math.sqrt(2) * math.log(9), rel=1e-7)
    assert float(AdaCos(8, 2).scale) == 0.0
    assert h.process_group is None
    assert h.double().scale.dtype == torch.float64 and h.W.dtype == torch.float64
    h = h.float()
    out = h(synth.normal(3, "ac.x", (3, 512)), torch.tensor([0, 9, 3]))
    assert out.shape == (3, 10) and out.device.type == "cpu" and list(h.state_dict()) == ["W"]
    from util.utils import separate_irse_bn_paras
    bn, rest = separate_irse_bn_paras(h)
    assert bn == [] and len(rest) == 1 and rest[0] is h.W
    h3 = AdaCos(512, 10)
    h3.load_state_dict(h.state_dict())  # the reference's Head_* files: the key W alone
    assert torch.equal(h3.W, h.W)


def test_empty_batch_leaves_the_scale():
    from head.metrics import AdaCos
    h = AdaCos(16, 10)
    before = h.scale.clone()
    out = h(torch.zeros(0, 16), torch.zeros(0, dtype=torch.long))
    assert out.shape == (0, 10) and torch.equal(h.scale, before)


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    for name in ("ADACOS", "adacos_forward", "adacos_backward", "AdaCosHeadFn", "adacos_head"):
        assert hasattr(FRF, name)
    assert FRF.ADACOS == 6 and FRF.MAGFACE == 5


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: empty shapes, row pitches that are too short or not multiples of 4, a
    negative row count; fr_adacos_scale over no rows is a successful no-op (the scale stays)."""
    from frhip import _lib
    lib = _lib.lib
    rows = lambda r, n, ld: lib.fr_adacos_rows(None, None, None, None, r, n, ld, None)  # noqa: E731
    assert rows(0, 100, 100) == -1 and rows(8, 0, 100) == -1 and rows(8, 101, 100) == -1 and rows(8, 101, 102) == -1
    assert b"fr_adacos_rows" in lib.fr_last_error_string()
    assert lib.fr_adacos_scale(None, -1, None, None) == -1 and b"fr_adacos_scale" in lib.fr_last_error_string()
    assert lib.fr_adacos_scale(None, 0, None, None) == 0
    apply_ = lambda r, n, lds, ldo: lib.fr_adacos_apply(None, None, None, r, n, lds, ldo, None)  # noqa: E731
    assert apply_(0, 100, 100, 128) == -1 and apply_(8, 0, 100, 128) == -1 and apply_(8, 100, 96, 128) == -1
    assert apply_(8, 100, 100, 96) == -1 and apply_(8, 101, 101, 102) == -1
    assert b"fr_adacos_apply" in lib.fr_last_error_string()


def test_device_entry_refuses_host_tensors():
    """No quiet fall-back: the functional entry is the HIP path and says so when handed host tensors."""
    from frhip import _lib
    from frhip import functional as FRF
    x, w = torch.zeros(2, 16), torch.ones(5, 16)
    with pytest.raises(_lib.FrhipError):  # the empty batch launches nothing and still says so
        FRF.adacos_head(x[:0], w, torch.tensor([], dtype=torch.long), torch.ones(1))


def test_forward_and_backward_never_read_the_scale_on_the_host():
    """The scale reaches the kernels through its device pointer only: neither function's source converts it."""
    import inspect
    from frhip import functional as FRF
    for fn in (FRF.adacos_forward, FRF.adacos_backward):
        src = inspect.getsource(fn)
        src = src[src.index('"""', src.index('"""') + 3):]  # past the docstring
        assert ".item(" not in src and ".cpu(" not in src and ".tolist(" not in src, fn.__name__
        assert not re.search(r"(?<![.\w])float\(", src), fn.__name__  # ``.float()`` of a tensor is a dtype cast


def test_train_py_takes_the_name_and_refuses_the_sharded_head():
    """train.py builds AdaCos in its ``heads`` table off the generator, keeps ``head_scale`` in the State_* file, and raises
    NotImplementedError for SHARDED_HEAD with AdaCos before anything is built; the other heads pass that check as before."""
    import train
    with pytest.raises(NotImplementedError, match="AdaCos"):
        train.check_head_config(dict(HEAD_NAME="AdaCos", SHARDED_HEAD=True))
    train.check_head_config(dict(HEAD_NAME="AdaCos", SHARDED_HEAD=False))
    train.check_head_config(dict(HEAD_NAME="AdaCos"))
    with pytest.raises(NotImplementedError, match="MagFace"):
        train.check_head_config(dict(HEAD_NAME="MagFace", SHARDED_HEAD=True))
    for name in ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace"):
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
    src = open(train.__file__).read()
    assert 'heads["AdaCos"] = AdaCos(emb, num_class)' in src and '"head_scale"' in src
    fork = src.index("with torch.random.fork_rng(devices=[])")
    assert fork < src.index('heads["AdaCos"]') < src.index("head = heads[cfg")
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "AdaCos" in common
