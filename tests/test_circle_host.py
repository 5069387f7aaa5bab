"""CPU checks of the CircleLoss and AM_Softmax heads (reference head/metrics.py:435-473 and :371-392): the host paths
reproduce the reference's own vectors (g23_circle, tests/golden/make_golden_circle.py), ``from_cos`` (the restatement the
entry-point tests compare with) is pinned against autograd through the reference's lines on given cosines, six deliberately
wrong variants each miss what they should, the modules keep the reference's layout, the C ABI of the HIP path is declared,
exported and checks its arguments before any launch, and train.py takes the names and refuses the class-sharded head."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import circle_data as CD
from frhip import synth

CASES = ("circle_rand", "circle_built", "circle_built_m04", "am_rand", "am_built", "am_built_m05")
NEW_ENTRIES = ("fr_circle_apply", "fr_circle_bwd")
B, D, N = 8, 512, 100


@pytest.fixture(scope="module")
def g23(golden_dir):
    return np.load(os.path.join(golden_dir, "g23_circle.npz"))


def head_of(tag):
    return tag.split("_")[0]


def scalars(g, tag):
    """(margin, gamma or scale) of a g23 case."""
    return float(g[tag + ".margin"]), float(g[tag + ".scale"])


def inputs_of(g, tag):
    """(x, weight, label, gout) of a g23 case, regenerated from synth; the file keeps the labels as a check."""
    if "built" in tag:
        x, k, label, gout = CD.built(synth, tag, B, D, N, head_of(tag), scalars(g, tag)[0])
    else:
        x, k, label, gout = CD.random_case(synth, tag, B, D, N)
    assert torch.equal(label, torch.from_numpy(g[tag + ".label"]))
    return x, k, label, gout


def make_head(g, tag, k):
    from head.metrics import AM_Softmax, CircleLoss
    margin, scale = scalars(g, tag)
    head = CircleLoss(D, N, margin=margin, gamma=scale) if head_of(tag) == "circle" else AM_Softmax(D, N, margin, scale)
    with torch.no_grad():
        head.weight.copy_(k)
    return head


def logit_bar(scale):
    """The siblings' 1e-3 was set with scales up to 64; a larger scale makes the same cosine error that much larger."""
    return 1e-3 * max(1.0, scale / 64.0)


def errors(g, tag, y, gx, gw):
    """{name: (error, bar)}: logits absolute, gradients and the norm of the whole weight gradient relative to the
    reference's, max(5e-3, 8 x the reference's own fp32-vs-float64 deviation)."""
    idx = torch.from_numpy(g[tag + ".gw_index"])
    res = {"logits": (float((y.detach() - torch.from_numpy(g[tag + ".logits"])).abs().max()), logit_bar(scalars(g, tag)[1]))}
    for name, got in (("gx", gx), ("gw", gw.index_select(1, idx))):
        ref = torch.from_numpy(g[tag + "." + name])
        assert got.shape == ref.shape
        res[name] = (float((got - ref).abs().max() / ref.abs().max()), max(5e-3, 8 * float(g[tag + ".dev." + name])))
    res["gw_norm"] = (abs(float(gw.double().norm()) / float(g[tag + ".gw_norm"]) - 1),
                      max(5e-3, 8 * float(g[tag + ".dev.gw"])))
    return res


@pytest.mark.parametrize("tag", CASES)
def test_host_path_reproduces_the_reference(g23, tag):
    """Logits within 1e-3 x max(1, scale / 64) absolute, gradients within max(5e-3, 8 x the reference's own fp32-vs-float64
    deviation) of max|ref| per tensor, the norm of the whole weight gradient likewise (the fixture's bars)."""
    x, k, label, gout = inputs_of(g23, tag)
    head = make_head(g23, tag, k)
    x.requires_grad_(True)
    y = head(x, label)
    gx, gw = torch.autograd.grad(y, [x, head.weight], gout)
    res = errors(g23, tag, y, gx, gw)
    print(tag, res)
    for name, (err, bar) in res.items():
        assert err < bar, (tag, name, err, bar)
    assert list(head.state_dict()) == ["weight"]
    assert float(g23[tag + ".dev.logits"]) < 1e-6


def test_fixture_plants_what_random_data_lacks(g23):
    """Every built case has a row with a target cosine near +0.9, one near -0.3 and a row with the three planted negatives
    (dead, barely alive, near +0.6), max |c| < 0.99, on this test's own float64 restatement as in the maker; the recorded
    gt and dead counts are that restatement's.  The random cases have no dead negative (which is why the cases are built)."""
    for tag in CASES:
        x, k, label, _ = inputs_of(g23, tag)
        margin, scale = scalars(g23, tag)
        st = CD.assert_covers(x, k, label, margin) if "built" in tag else CD.stats64(x, k, label, margin)
        assert torch.equal(st["dead"], torch.from_numpy(g23[tag + ".dead"]))
        assert float((st["gt"] - torch.from_numpy(g23[tag + ".gt"])).abs().max()) < 1e-12
        assert st["max_abs_c"] < 0.99 and abs(st["max_abs_c"] - float(g23[tag + ".max_abs_c"])) < 1e-12
        if "built" in tag:
            assert st["dead"].tolist() == [0, 1, 0, 0, 0, 1, 0, 0] and st["planted"].tolist() == [i % 4 == 1 for i in range(B)]
            c = CD.cosines64(x, k)[1]
            for want in (-margin + CD.PLANTED[0], -margin + CD.PLANTED[1], CD.STRONG):
                assert float((c - want).abs().min()) < 1e-6, want
        else:
            assert not bool(st["dead"].any()) and st["max_abs_c"] < 0.2
        assert (margin, scale) == {"circle_built_m04": (0.4, 80.0), "am_built_m05": (0.5, 64.0)}.get(
            tag, CD.DEFAULTS[head_of(tag)])


# ------------------------------------------------------------------------------------------------ from_cos


def reference_lines(cos, label, head, margin, scale):
    """The reference's own lines from ``cos_theta = cos_theta.clamp(-1, 1)`` on (:455-473, :384-392), on a given cosine
    matrix, with bool masks in place of its uint8 ones."""
    cos_theta = cos.clamp(-1, 1)
    if head == "am":
        cos_theta_m = cos_theta - margin
        index = torch.zeros_like(cos_theta)
        index.scatter_(1, label.data.view(-1, 1), 1)
        index = index.bool()
        output = cos_theta * 1.0
        output[index] = cos_theta_m[index]
        output *= scale
        return output
    O_p, O_n, delta_p, delta_n = CD.circle_constants(margin)
    index_pos = torch.zeros_like(cos_theta)
    index_pos.scatter_(1, label.data.view(-1, 1), 1)
    index_pos = index_pos.bool()
    index_neg = torch.ones_like(cos_theta)
    index_neg.scatter_(1, label.data.view(-1, 1), 0)
    index_neg = index_neg.bool()
    alpha_p = torch.clamp_min(O_p - cos_theta.detach(), min=0.)
    alpha_n = torch.clamp_min(cos_theta.detach() - O_n, min=0.)
    logit_p = alpha_p * (cos_theta - delta_p)
    logit_n = alpha_n * (cos_theta - delta_n)
    output = cos_theta * 1.0
    output[index_pos] = logit_p[index_pos]
    output[index_neg] = logit_n[index_neg]
    output *= scale
    return output


def hand_cosines(dtype, margin):
    """[6, 40] cosines on a grid, with exactly +-1, values beyond +-1, O_n itself and its neighbours in ``dtype``, a value
    below O_n and a NaN row (row 4); labels 0, 39, 7, 3, 5, 11.  Row 3's label column holds a cosine beyond +1."""
    cos = (torch.round(synth.uniform(CD.SEED, "host.hand", (6, 40), -0.9, 0.9) * 64) / 64).to(dtype)
    o_n = torch.tensor(-margin, dtype=dtype)
    up, down = torch.nextafter(o_n, o_n + 1), torch.nextafter(o_n, o_n - 1)
    for row in (0, 1, 2):
        cos[row, 10:19] = torch.stack([torch.tensor(v, dtype=dtype) for v in (1.0, -1.0, 1.0 + 2.0 ** -20, -1.0 - 2.0 ** -20)]
                                      + [o_n, up, down, o_n - 0.2, o_n + 0.01])
    cos[3, 3] = 1.0 + 2.0 ** -20
    cos[4] = float("nan")
    return cos, torch.tensor([0, 39, 7, 3, 5, 11])


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])
@pytest.mark.parametrize("head,margin,scale", [("circle", 0.25, 256.0), ("circle", 0.4, 80.0), ("am", 0.35, 32.0),
                                               ("am", 0.5, 64.0)])
def test_from_cos_is_the_reference_on_given_cosines(head, margin, scale, dtype):
    """``from_cos`` and ``grad_from_cos`` equal the reference's lines and autograd through them bit for bit, in fp32 and in
    float64, NaN in the same places: the values, d out / d cos (from an upstream gradient of ones) and the gradient of a
    random upstream g -- which pins autograd's order (g * gamma) * alpha at gamma = 80, where g * (gamma * alpha) rounds
    differently -- and the closed-interval pass mask (gradient at exactly +-1, none beyond, none on the NaN row)."""
    cos, label = hand_cosines(dtype, margin)
    leaf = cos.clone().requires_grad_(True)
    ref = reference_lines(leaf, label, head, margin, scale)
    out, dout, parts = CD.from_cos(cos, label, head, margin, scale)
    assert torch.equal(torch.isnan(out), torch.isnan(ref)) and bool(torch.isnan(out[4]).all()) and not bool(torch.isnan(out[:4]).any())
    assert torch.equal(out.nan_to_num(7.0), ref.detach().nan_to_num(7.0))
    d_ref, = torch.autograd.grad(ref, leaf, torch.ones_like(ref), retain_graph=True)
    assert not bool(torch.isnan(d_ref).any()) and torch.equal(dout, d_ref)
    g = synth.uniform(CD.SEED, "host.hand.g", (6, 40), -1.0, 1.0).to(dtype)
    g_ref, = torch.autograd.grad(ref, leaf, g)
    mine = CD.grad_from_cos(cos, label, g, head, margin, scale)
    assert torch.equal(mine, g_ref)
    assert not bool(mine[4].any()) and not bool(mine[0, 12:14].any()) and float(mine[0, 10]) != 0  # passes at exactly +1
    assert float(mine[0, 11]) != 0 or head == "circle"  # and at exactly -1 (where CircleLoss's negative is dead anyway)
    if head == "circle":
        assert not bool(out[0, 14].any()) and not bool(out[0, 16:18].any()) and not bool(mine[0, 16:18].any())  # dead
        assert float(out[0, 15]) != 0 and float(mine[0, 15]) != 0  # the neighbour above O_n is alive
        if scale == 80.0 and dtype == torch.float32:
            other = torch.where(parts["mask"], g * (scale * parts["alpha"]), torch.zeros_like(g))
            assert not torch.equal(other, g_ref)  # the order matters at a gamma that is no power of two


def test_from_cos_is_the_head_on_valid_labels(g23):
    """``from_cos`` on the float64 cosines of a built case equals the host path in float64, logits and the gradient with
    respect to x (through its d out / d cos)."""
    for tag in ("circle_built", "circle_built_m04", "am_built_m05"):
        x, k, label, gout = inputs_of(g23, tag)
        margin, scale = scalars(g23, tag)
        head = make_head(g23, tag, k).double()
        xa = x.double().requires_grad_(True)
        ya = head(xa, label)
        xb = x.double().requires_grad_(True)
        cb = F.normalize(xb) @ F.normalize(k.double(), dim=0)
        yb, dout, _ = CD.from_cos(cb.detach(), label, head_of(tag), margin, scale)
        assert float((ya.detach() - yb).abs().max()) < 1e-12 * scale
        ga, = torch.autograd.grad(ya, xa, gout.double())
        gb, = torch.autograd.grad(cb, xb, gout.double() * dout)
        assert float((ga - gb).abs().max()) < 1e-10 * float(ga.abs().max())


# ------------------------------------------------------------------------------------------------ negative controls


def variant(x, k, label, head, margin, scale, alpha_attached=False, no_clamp_min=False, label_as_negative=False,
            unnormalised_x=False, margin_everywhere=False):
    """The heads' arithmetic written out once more with one deliberate mistake per flag."""
    c = torch.mm(x if unnormalised_x else F.normalize(x), F.normalize(k, dim=0)).clamp(-1, 1)
    hot = torch.zeros_like(c).scatter_(1, label.view(-1, 1), 1).bool()
    if head == "am":
        return (c - margin if margin_everywhere else torch.where(hot, c - margin, c)) * scale
    o_p, o_n, delta_p, delta_n = CD.circle_constants(margin)
    ca = c if alpha_attached else c.detach()
    alpha_p, alpha_n = o_p - ca, ca - o_n
    if not no_clamp_min:
        alpha_p, alpha_n = torch.clamp_min(alpha_p, min=0.), torch.clamp_min(alpha_n, min=0.)
    logit_n = alpha_n * (c - delta_n)
    return torch.where(hot, logit_n if label_as_negative else alpha_p * (c - delta_p), logit_n) * scale


CONTROLS = [("circle", "alpha_attached"), ("circle", "no_clamp_min"), ("circle", "label_as_negative"),
            ("am", "unnormalised_x"), ("am", "margin_everywhere")]


@pytest.mark.parametrize("head,flag", CONTROLS)
def test_negative_controls_miss_the_fixture(g23, head, flag):
    """The written-out variant meets the bars on every case of its head with no flag set, and misses them on a built case
    with any single one: alpha left attached (backward only: the logits still match), no ``clamp_min`` (the planted dead
    negative comes alive), the label column given the negative's formula; AM_Softmax with the embeddings left unnormalised
    (what ``Am_softmax`` does) and with the margin on every column."""
    tags = [t for t in CASES if head_of(t) == head]

    def run(tag, **flags):
        x, k, label, gout = inputs_of(g23, tag)
        xx = x.clone().requires_grad_(True)
        kk = k.clone().requires_grad_(True)
        y = variant(xx, kk, label, head, *scalars(g23, tag), **flags)
        gx, gw = torch.autograd.grad(y, [xx, kk], gout)
        return errors(g23, tag, y, gx, gw), y.detach()

    for tag in tags:
        assert all(err < bar for err, bar in run(tag)[0].values()), (tag, run(tag)[0])
    bad = {tag: run(tag, **{flag: True}) for tag in tags if "built" in tag}
    print(flag, {tag: res for tag, (res, _) in bad.items()})
    for tag, (res, y) in bad.items():
        assert any(not err < bar for err, bar in res.values()), (flag, tag, res)  # every built case catches it
    if flag == "alpha_attached":
        assert all(res["logits"][0] < res["logits"][1] and not res["gx"][0] < res["gx"][1] for res, _ in bad.values())
    if flag == "no_clamp_min":  # it is the planted dead negative of rows 1 and 5 that comes alive, and nothing else
        for tag, (res, y) in bad.items():
            diff = (y - torch.from_numpy(g23[tag + ".logits"])).abs() > res["logits"][1]
            assert diff.sum(1).tolist() == [0, 1, 0, 0, 0, 1, 0, 0], diff.sum(1)
        assert all(r < b for r, b in run("circle_rand", no_clamp_min=True)[0].values())  # random data cannot tell


def test_backward_without_the_pass_mask_misses_the_hand_made_cosines():
    """The fourth CircleLoss control: a backward pass without the clamp's pass mask differs from autograd through the
    reference's lines exactly at the cosines beyond +-1 (and on the NaN row) of the hand-made matrix; the fixture keeps
    max |c| < 0.99 and cannot tell."""
    cos, label = hand_cosines(torch.float32, 0.25)
    leaf = cos.clone().requires_grad_(True)
    g = synth.uniform(CD.SEED, "host.hand.g", (6, 40), -1.0, 1.0)
    g_ref, = torch.autograd.grad(reference_lines(leaf, label, "circle", 0.25, 256.0), leaf, g)
    parts = CD.from_cos(cos, label, "circle", 0.25, 256.0)[2]
    unmasked = (g * 256.0) * parts["alpha"]
    differs = ~((unmasked == g_ref) | (torch.isnan(unmasked) & torch.isnan(g_ref)))
    assert torch.equal(differs, ~parts["mask"] & ((unmasked != 0) | torch.isnan(unmasked)))
    assert bool(differs[0, 12]) and bool(differs[3, 3]) and bool(differs[4].all()) and not bool(differs[0, 10:12].any())
    assert not bool(differs[0, 13])  # beyond -1 the negative is dead anyway: alpha_n = 0 there


# ------------------------------------------------------------------------------------------------ the modules


def test_import_head_metrics_exposes_both_classes():
    import head.metrics as H
    from head.metrics import AM_Softmax, CircleLoss  # noqa: F401  -- the FaceX-Zoo config's import line
    assert H.AM_Softmax is not H.Am_softmax and issubclass(H.CircleLoss, torch.nn.Module)
    assert "CircleLoss" in H.__doc__ and "AM_Softmax" in H.__doc__


def test_heads_keep_the_reference_layout():
    """Constructors (feat_dim, num_class, margin, gamma / scale with the reference's defaults), parameter ``weight`` [D, N]
    with unit columns, the reference's attributes, a state dict with the key ``weight`` alone, attributes read on every
    call, the empty batch on the host."""
    import inspect
    from head.metrics import AM_Softmax, CircleLoss
    E = inspect.Parameter.empty
    for cls, tail in ((CircleLoss, [("margin", 0.25), ("gamma", 256)]), (AM_Softmax, [("margin", 0.35), ("scale", 32)])):
        sig = inspect.signature(cls.__init__)
        assert [(n, p.default) for n, p in list(sig.parameters.items())[1:]] == [("feat_dim", E), ("num_class", E)] + tail
        assert [n for n in inspect.signature(cls.forward).parameters] == ["self", "feats", "labels"]
        torch.manual_seed(0)
        h = cls(512, 10)
        assert list(h.state_dict()) == ["weight"] and [n for n, _ in h.named_parameters()] == ["weight"]
        assert list(h.buffers()) == [] and tuple(h.weight.shape) == (512, 10)
        assert float((h.weight.detach().norm(dim=0) - 1).abs().max()) < 1e-4
        from util.utils import separate_irse_bn_paras
        bn, rest = separate_irse_bn_paras(h)
        assert bn == [] and len(rest) == 1 and rest[0] is h.weight
        h2 = cls(512, 10)
        h2.load_state_dict(h.state_dict())
        assert torch.equal(h2.weight, h.weight)
        assert h(torch.zeros(0, 512), torch.zeros(0, dtype=torch.long)).shape == (0, 10)
    h = CircleLoss(512, 10)
    assert (h.margin, h.gamma, h.O_p, h.O_n, h.delta_p, h.delta_n) == (0.25, 256, 1.25, -0.25, 0.75, 0.25)
    h4 = CircleLoss(16, 5, margin=0.4, gamma=80)
    assert (h4.O_p, h4.O_n, h4.delta_p, h4.delta_n, h4.gamma) == (1 + 0.4, -0.4, 1 - 0.4, 0.4, 80)
    a = AM_Softmax(512, 10)
    assert (a.margin, a.scale) == (0.35, 32)
    y = torch.tensor([0, 9, 3])
    x = synth.normal(3, "circle.x", (3, 512)) / 512 ** 0.5 + 0.2 * h.weight.detach()[:, y].t()
    seen = [h(x, y)]
    assert seen[0].shape == (3, 10) and seen[0].device.type == "cpu"
    for name, v in (("gamma", 64), ("O_p", 1.5), ("O_n", 0.0), ("delta_p", 0.5), ("delta_n", 0.1)):
        setattr(h, name, v)  # plain attributes, read on every call
        seen.append(h(x, y))
        assert not torch.equal(seen[-1], seen[-2]), name
    h.margin = 0.9
    assert torch.equal(h(x, y), seen[-1])  # margin is read by the constructor alone, as in the reference
    seen = [a(x, y)]
    for name, v in (("margin", 0.1), ("scale", 16.0)):
        setattr(a, name, v)
        seen.append(a(x, y))
        assert not torch.equal(seen[-1], seen[-2]), name
    assert float((a(3.0 * x, y) - a(x, y)).detach().abs().max()) < 1e-4  # the embeddings are normalised, unlike Am_softmax's


# ------------------------------------------------------------------------------------------------ the ABI


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    assert _lib.protos["fr_circle_apply"][2] == ["cos", "label", "out", "rows", "N", "ld", "o_p", "o_n", "delta_p", "delta_n",
                                                 "gamma", "stream"]
    assert _lib.protos["fr_circle_bwd"][2] == ["g", "cos", "label", "gcos", "rows", "N", "ld", "ldg", "o_p", "o_n", "gamma",
                                               "stream"]
    for name in ("CIRCLE", "AM_SOFTMAX_N", "circle_forward", "circle_backward", "am_softmax_n_forward",
                 "am_softmax_n_backward", "CircleHeadFn", "AMSoftmaxNHeadFn", "circle_head", "am_softmax_n_head"):
        assert hasattr(FRF, name)
    assert (FRF.MV_SOFTMAX, FRF.CIRCLE, FRF.AM_SOFTMAX_N, FRF.AM_SOFTMAX) == (8, 9, 10, 3)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frhip.h")).read()
    at = header.index("CircleLoss (head/metrics.py:435-473)")
    assert header.index("int fr_mv_softmax_bwd(") < at < header.index("int fr_circle_apply(") \
        < header.index("int fr_circle_bwd(") < header.index("int fr_ce_rows(")
    assert ":455-472" in header[at:header.index("int fr_circle_apply(")]  # each declaration cites its reference lines
    assert ":463-464" in header[header.index("int fr_circle_apply("):header.index("int fr_circle_bwd(")]
    assert ":371-392" in header[at:header.index("int fr_circle_apply(")]  # where AM_Softmax's kernels are


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: empty shapes, row pitches that are too short or not multiples of 4."""
    from frhip import _lib
    lib = _lib.lib
    apply_ = lambda r, n, ld: lib.fr_circle_apply(None, None, None, r, n, ld, 1.25, -0.25, 0.75, 0.25, 256.0, None)  # noqa: E731
    assert apply_(0, 100, 100) == -1 and apply_(8, 0, 100) == -1 and apply_(8, 101, 100) == -1 and apply_(8, 101, 102) == -1
    assert apply_(-1, 100, 100) == -1 and apply_(8, 100, 96) == -1
    assert b"fr_circle_apply" in lib.fr_last_error_string()
    bwd = lambda r, n, ld, ldg: lib.fr_circle_bwd(None, None, None, None, r, n, ld, ldg, 1.25, -0.25, 256.0, None)  # noqa: E731
    assert bwd(0, 100, 100, 128) == -1 and bwd(8, 0, 100, 128) == -1 and bwd(8, 100, 100, 96) == -1
    assert bwd(8, 100, 98, 128) == -1 and bwd(8, 100, 96, 128) == -1 and bwd(8, 100, 100, 126) == -1
    assert b"fr_circle_bwd" in lib.fr_last_error_string()


def test_device_entries_refuse_host_tensors():
    """No quiet fall-back: the functional entries are the HIP path and say so when handed host tensors."""
    from frhip import _lib
    from frhip import functional as FRF
    x, k, none = torch.zeros(2, 16), torch.ones(16, 5), torch.tensor([], dtype=torch.long)
    with pytest.raises(_lib.FrhipError):  # the empty batch launches nothing and still says so
        FRF.circle_head(x[:0], k, none, 1.25, -0.25, 0.75, 0.25, 256.0)
    with pytest.raises(_lib.FrhipError):
        FRF.am_softmax_n_head(x[:0], k, none, 0.35, 32.0)


def test_train_py_takes_the_names_and_refuses_the_sharded_head():
    """train.py builds the two heads in its ``heads`` table off the generator, after MV_Softmax, and raises
    NotImplementedError for SHARDED_HEAD with either before anything is built; the other heads pass or fail that check as
    before."""
    import train
    for name in ("CircleLoss", "AM_Softmax"):
        with pytest.raises(NotImplementedError, match=name):
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=False))
        train.check_head_config(dict(HEAD_NAME=name))
    for name in ("MagFace", "AdaCos", "NPCFace", "MV_Softmax"):
        with pytest.raises(NotImplementedError, match=name):
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
        train.check_head_config(dict(HEAD_NAME=name))
    for name in ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace"):
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
    src = open(train.__file__).read()
    fork = src.index("with torch.random.fork_rng(devices=[])")
    assert fork < src.index('heads["MV_Softmax"]') < src.index('heads["CircleLoss"] = CircleLoss(emb, num_class)') \
        < src.index('heads["AM_Softmax"] = AM_Softmax(emb, num_class)') < src.index("head = heads[cfg")
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "CircleLoss" in common and "AM_Softmax" in common
