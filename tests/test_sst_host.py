"""SST_Prototype on the host (no GPU): the module's host path against the reference's own vectors (g27, a trajectory of five
calls per loss type that wraps and overwrites the queue), its state, errors and driver state, negative controls that show
what g27 pins, ``ParamEMA`` on host modules, and the C ABI of the five new entry points.

g27 holds no inputs: tests/sst_data.py rebuilds them from the counter-based generator, as the maker did."""
import copy
import ctypes
import math
import os
import random

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sst_data as SD
from frhip import synth
from head.metrics import SST_Prototype

B, D, Q, CALLS = 8, 512, 32, 5
COIN_SEED = 27
NEW_ENTRIES = ("fr_sst_enqueue", "fr_sst_apply", "fr_sst_bwd", "fr_ema_step", "fr_ema_chunk_elems")


@pytest.fixture(scope="module")
def g27(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g27_sst_prototype.npz")))


@pytest.fixture(scope="module")
def queue0():
    return SD.initial_queue(synth, "g27", D, Q)


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).tobytes()


def make_head(queue0, loss_type, margin, size=Q):
    head = SST_Prototype(D, size, scale=SD.SCALE, loss_type=loss_type, margin=margin)
    if size == Q:
        head.queue = queue0.clone()
    return head


# ------------------------------------------------------------------------------------------------ the host path against g27


@pytest.mark.parametrize("loss_type,margin", SD.LOSS_TYPES)
def test_host_path_reproduces_g27_bit_for_bit(g27, queue0, loss_type, margin):
    head = make_head(queue0, loss_type, margin)
    assert list(head.state_dict().keys()) == ["queue"]
    random.seed(COIN_SEED)
    for k in range(CALLS):
        pre = "%s.%d." % (loss_type, k)
        p1, g2, p2, g1, ids, go1, go2 = SD.step(synth, "g27." + loss_type, k, B, D, Q, queue0)
        SD.assert_covers(p1, g2, p2, g1)
        index = head.index
        a1, a2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
        b1, b2 = g1.clone().requires_grad_(True), g2.clone().requires_grad_(True)
        o1, o2, label, id_set = head(a1, b2, a2, b1, ids)
        ((o1 * go1).sum() + (o2 * go2).sum()).backward()
        assert b1.grad is None and b2.grad is None  # the gallery rows are detached
        for name, got in (("out1", o1), ("out2", o2), ("gp1", a1.grad), ("gp2", a2.grad),
                          ("window", head.queue[:, index:index + B])):
            assert got.dtype == torch.float32 and bits(got) == bits(g27[pre + name]), (
                pre + name, float((got.detach().double() - torch.from_numpy(g27[pre + name]).double()).abs().max()))
        assert label.dtype == torch.int64 and label.shape == (B,) and label.tolist() == g27[pre + "label"].tolist()
        coin = int(torch.equal(head.queue[:, index:index + B], F.normalize(g1).t()))
        assert coin == int(g27[pre + "coin"]) and head.index == int(g27[pre + "index"])
        assert head.label_list == g27[pre + "label_list"].tolist()
        assert isinstance(id_set, set) and sorted(id_set) == g27[pre + "id_set"].tolist() == sorted(head.get_id_set())
        assert abs(float(head.queue.double().norm()) - float(g27[pre + "queue_norm"])) < 1e-12
    assert g27[loss_type + ".coins"].tolist() == [int(g27["%s.%d.coin" % (loss_type, k)]) for k in range(CALLS)]
    assert set(g27[loss_type + ".coins"].tolist()) == {0, 1}


def test_every_mode_advances_the_queue(queue0):
    head = make_head(queue0, "softmax", 0.0).eval()
    p1, g2, p2, g1, ids, _, _ = SD.step(synth, "modes", 0, B, D, Q, queue0)
    with torch.no_grad():
        head(p1, g2, p2, g1, ids)
    assert head.index == B and head.label_list[:B] == ids.tolist() and head.label_list[B:] == [-1] * (Q - B)
    assert not torch.equal(head.queue[:, :B], queue0[:, :B]) and torch.equal(head.queue[:, B:], queue0[:, B:])
    o1, _, label, _ = head(p1[:1], g2[:1], p2[:1], g1[:1], [5])  # B = 1: the label keeps its dimension
    assert label.shape == (1,) and label.tolist() == [B] and o1.shape == (1, Q) and head.index == B + 1


def test_wrap_around_raises_and_leaves_the_state_alone(queue0):
    head = make_head(queue0, "am_softmax", 0.35)
    p1, g2, p2, g1, ids, _, _ = SD.step(synth, "wrap", 0, B, D, Q, queue0)
    head.load_queue_state(Q - B + 1, [-1] * Q)
    random.seed(3)
    before = random.getstate()
    with pytest.raises(RuntimeError, match="runs past the queue"):
        head(p1, g2, p2, g1, ids)
    assert head.index == Q - B + 1 and head.label_list == [-1] * Q and torch.equal(head.queue, queue0)
    assert random.getstate() == before  # no coin was drawn


def test_queue_state_round_trips_and_any_size_runs_on_the_host(queue0):
    head = make_head(queue0, "arc_softmax", 0.5)
    random.seed(5)
    for k in range(2):
        p1, g2, p2, g1, ids, _, _ = SD.step(synth, "state", k, B, D, Q, queue0)
        head(p1, g2, p2, g1, ids)
    index, labels = head.queue_state()
    assert index == 2 * B and labels.dtype == torch.int64 and labels.tolist() == head.label_list
    other = make_head(queue0, "arc_softmax", 0.5)
    other.load_state_dict(head.state_dict())
    other.load_queue_state(index, labels)
    assert other.index == index and other.label_list == head.label_list and torch.equal(other.queue, head.queue)
    p1, g2, p2, g1, ids, _, _ = SD.step(synth, "state", 2, B, D, Q, queue0)
    random.seed(6)
    a = head(p1, g2, p2, g1, ids)
    random.seed(6)
    b = other(p1, g2, p2, g1, ids)
    assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1]) and a[3] == b[3]
    with pytest.raises(ValueError):
        other.load_queue_state(Q, labels)
    odd = SST_Prototype(D, 48)  # not a multiple of 32: the host path serves it
    o1, o2, label, ids_ = odd(p1, g2, p2, g1, ids)
    assert o1.shape == (B, 48) and odd.index == B and ids_ == set(ids.tolist())
    cols = odd.queue.norm(dim=0)
    assert float((cols - 1).abs().max()) < 1e-6  # the initial queue is normalised, as the reference's


# ------------------------------------------------------------------------------------------------ negative controls


def restated(queue0, loss_type, margin, k_calls, wrong=None):
    """The trajectory restated with one thing done wrong: 'stale' (the window not substituted), 'fallback' (ArcFace's
    threshold fallback on the label column), 'other_view' (the queue fed the other view), 'margin_first' (the margin before
    the clamp), 'attached' (the gallery rows and the queue left in the graph).  Returns per call (out1, out2, gp1, gp2,
    window, gg: the largest gradient entry that reached g)."""
    queue, index, res = queue0.clone(), 0, []
    random.seed(COIN_SEED)
    for k in range(k_calls):
        p1, g2, p2, g1, ids, go1, go2 = SD.step(synth, "g27." + loss_type, k, B, D, Q, queue0)
        a1, a2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
        b1, b2 = g1.clone().requires_grad_(True), g2.clone().requires_grad_(True)
        n1, n2 = F.normalize(b1), F.normalize(b2)
        if wrong != "attached":
            n1, n2 = n1.detach(), n2.detach()
        label = torch.arange(B) + index
        at = label.view(-1, 1)

        def margin_of(c):
            if loss_type == "am_softmax":
                return c.scatter(1, at, c.gather(1, at) - margin)
            if loss_type == "arc_softmax":
                gt = c.gather(1, at)
                phi = gt * math.cos(margin) - torch.sqrt(1.0 - torch.pow(gt, 2)) * math.sin(margin)
                if wrong == "fallback":
                    phi = torch.where(gt > math.cos(math.pi - margin), phi, gt - math.sin(math.pi - margin) * margin)
                return c.scatter(1, at, phi)
            return c

        def theta(p, g):
            qq = queue if wrong == "stale" else torch.cat([queue[:, :index], g.t(), queue[:, index + B:]], 1)
            c = torch.mm(F.normalize(p), qq if wrong == "attached" else qq.detach())
            c = margin_of(c).clamp(-1, 1) if wrong == "margin_first" else margin_of(c.clamp(-1, 1))
            return c * SD.SCALE

        o1, o2 = theta(a1, n2), theta(a2, n1)
        ((o1 * go1).sum() + (o2 * go2).sum()).backward()
        take_g1 = (random.random() > 0.5) != (wrong == "other_view")
        g = (n1 if take_g1 else n2).detach()
        queue = torch.cat([queue[:, :index], g.t(), queue[:, index + B:]], 1)
        gg = max(0.0 if t.grad is None else float(t.grad.abs().max()) for t in (b1, b2))
        res.append((o1.detach(), o2.detach(), a1.grad, a2.grad, queue[:, index:index + B].clone(), gg))
        index = (index + B) % Q
    return res


def misses(g27, loss_type, res):
    """The names of the g27 tensors a restated trajectory does not reproduce bit for bit."""
    bad = []
    for k, r in enumerate(res):
        for name, got in zip(("out1", "out2", "gp1", "gp2", "window"), r):
            if bits(got) != bits(g27["%s.%d.%s" % (loss_type, k, name)]):
                bad.append("%d.%s" % (k, name))
    return bad


def test_the_restatement_itself_reproduces_g27(g27, queue0):
    for loss_type, margin in SD.LOSS_TYPES:
        res = restated(queue0, loss_type, margin, CALLS)
        assert misses(g27, loss_type, res) == [] and all(r[5] == 0.0 for r in res)


@pytest.mark.parametrize("wrong,loss_type,margin", [("stale", "softmax", 0.0), ("other_view", "softmax", 0.0),
                                                    ("stale", "arc_softmax", 0.5), ("other_view", "am_softmax", 0.35)])
def test_negative_controls_miss_g27(g27, queue0, wrong, loss_type, margin):
    bad = misses(g27, loss_type, restated(queue0, loss_type, margin, CALLS, wrong))
    assert bad, (wrong, "reproduces g27")
    if wrong == "other_view":  # the logits of call 0 do not see the queue's new content; the window does
        assert "0.window" in bad and "0.out1" not in bad
    if wrong == "stale":
        assert "0.out1" in bad and "0.window" not in bad


def test_negative_control_attached_gallery_rows(g27, queue0):
    """With the gallery rows and the substituted queue left in the graph the probe gradients are still g27's -- the vectors
    cannot see it -- but a gradient reaches g; the module's host path leaves ``g.grad`` None
    (test_host_path_reproduces_g27_bit_for_bit)."""
    res = restated(queue0, "am_softmax", 0.35, 2, "attached")
    assert misses(g27, "am_softmax", res) == [] and all(r[5] > 1e-3 for r in res)


def test_negative_control_threshold_fallback(g27, queue0):
    """ArcFace's fallback replaces phi by gt - mm where gt <= cos(pi - margin) = -0.878.  g27's target cosines lie in
    [0.2, 0.95], where it never acts, so it reproduces g27; on a row with its target at -0.95 it differs from the head,
    which has no fallback (head/metrics.py:661-665)."""
    assert misses(g27, "arc_softmax", restated(queue0, "arc_softmax", 0.5, CALLS, "fallback")) == []
    head = make_head(queue0, "arc_softmax", 0.5)
    g = torch.zeros(1, D)
    g[0, 0] = 1.0
    p = torch.zeros(1, D)
    p[0, 0], p[0, 1] = -0.95, math.sqrt(1 - 0.95 ** 2)
    o1, _, _, _ = head(p, g, p, g, [1])
    gt = torch.tensor(-0.95)
    want = (gt * math.cos(0.5) - torch.sqrt(1.0 - gt * gt) * math.sin(0.5)) * SD.SCALE
    fallback = (gt - math.sin(math.pi - 0.5) * 0.5) * SD.SCALE
    assert abs(float(o1[0, 0]) - float(want)) < 1e-4 and abs(float(o1[0, 0]) - float(fallback)) > 1.0


def test_negative_control_margin_before_the_clamp(g27, queue0):
    """With every cosine inside [-1, 1] and a label value that stays there, clamp and margin commute: g27, whose target
    cosines lie in [0.2, 0.95] at margins 0.35 and 0.5, cannot see the order.  A margin of 1.5 on a target cosine of 0.6
    can: the head gives scale * (0.6 - 1.5), the wrong order scale * -1."""
    for loss_type, margin in SD.LOSS_TYPES[1:]:
        assert misses(g27, loss_type, restated(queue0, loss_type, margin, CALLS, "margin_first")) == []
    head = make_head(queue0, "am_softmax", 1.5)
    g = torch.zeros(1, D)
    g[0, 0] = 1.0
    p = torch.zeros(1, D)
    p[0, 0], p[0, 1] = 0.6, 0.8
    o1, _, _, _ = head(p, g, p, g, [1])
    assert abs(float(o1[0, 0]) - SD.SCALE * (0.6 - 1.5)) < 1e-4 and abs(float(o1[0, 0]) + SD.SCALE) > 1.0


# ------------------------------------------------------------------------------------------------ ParamEMA on the host


@pytest.mark.parametrize("alpha", [0.999, 0.5])
def test_param_ema_on_host_modules_is_the_torch_expression(alpha):
    from frhip.optim import ParamEMA
    torch.manual_seed(3)
    src = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.BatchNorm1d(5), torch.nn.Linear(5, 3))
    dst = copy.deepcopy(src)
    with torch.no_grad():
        for p in src.parameters():
            p.add_(torch.randn_like(p))
        dst[1].running_mean.fill_(2.0)
    ema = ParamEMA(dst, src, alpha)
    want = [p.detach().clone() for p in dst.parameters()]
    for step in range(3):
        ema.step()
        for w, d, s in zip(want, dst.parameters(), src.parameters()):
            w.copy_(w * alpha + s.detach() * (1.0 - alpha))
            assert bits(d) == bits(w), step
        with torch.no_grad():
            for p in src.parameters():
                p.mul_(1.01)
    assert float(dst[1].running_mean[0]) == 2.0 and float(src[1].running_mean[0]) == 0.0  # buffers are not touched
    with pytest.raises(ValueError):
        ParamEMA(torch.nn.Linear(3, 3), torch.nn.Linear(3, 3, bias=False))


def test_param_ema_host_step_equals_the_float32_restatement():
    from frhip.optim import ParamEMA
    rng = np.random.default_rng(5)
    a, b = torch.nn.Linear(33, 17), torch.nn.Linear(33, 17)
    d0, s0 = rng.standard_normal((17, 33)).astype(np.float32), rng.standard_normal((17, 33)).astype(np.float32)
    with torch.no_grad():
        a.weight.copy_(torch.from_numpy(d0))
        b.weight.copy_(torch.from_numpy(s0))
    ParamEMA(a, b, 0.999).step()
    a32, b32 = np.float32(0.999), np.float32(1.0 - 0.999)
    want = (a32 * d0).astype(np.float32) + (b32 * s0).astype(np.float32)
    assert bits(a.weight) == want.astype(np.float32).tobytes()


# ------------------------------------------------------------------------------------------------ the C ABI


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7
    assert _lib.lib.fr_ema_chunk_elems() == _lib.lib.fr_sgd_chunk_elems()
    assert ctypes.sizeof(_lib.FrEmaTensor) == 24 == _lib.lib.fr_struct_size(9)
    assert _lib.protos["fr_sst_enqueue"][2] == ["gn", "ids", "qt", "q", "labels", "index", "B", "D", "Q", "stream"]
    assert _lib.protos["fr_ema_step"][2] == ["table_dev", "chunks_dev", "nchunks", "a", "b", "stream"]
    for name in ("sst_forward", "sst_backward", "SSTHeadFn", "sst_margin"):
        assert hasattr(FRF, name)
    assert FRF.sst_margin("am_softmax", 0.35) == (1, 0.35, 0.0) and FRF.sst_margin("anything", 0.3) == (0, 0.0, 0.0)
    assert FRF.sst_margin("arc_softmax", 0.5) == (2, math.cos(0.5), math.sin(0.5))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frhip.h")).read()
    at = header.index("SST_Prototype (head/metrics.py:638-708")
    e, a, b = (header.index("int %s(" % n) for n in ("fr_sst_enqueue", "fr_sst_apply", "fr_sst_bwd"))
    assert at < e < a < b
    assert ":675-680" in header[at:e] and ":654-673" in header[e:a] and ":654-673" in header[a:b]
    assert "infinite" in header[a:b] and "NaN" in header[e:a]


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch."""
    from frhip import _lib
    lib = _lib.lib
    enq = lambda index, b, d, q: lib.fr_sst_enqueue(None, None, None, None, None, index, b, d, q, None)  # noqa: E731
    assert enq(0, 0, 512, 32) == -1 and enq(-1, 8, 512, 32) == -1 and enq(25, 8, 512, 32) == -1 and enq(0, 8, 0, 32) == -1
    assert enq(24, 8, 512, 32) == -1 and b"required" in lib.fr_last_error_string()  # the shape passes, the pointers do not
    apply_ = lambda rows, b, q, ld, ldw, index, kind: lib.fr_sst_apply(  # noqa: E731
        None, None, None, rows, b, q, ld, ldw, index, kind, 0.0, 0.0, 30.0, None)
    assert apply_(24, 8, 32, 32, 32, 0, 0) == -1 and apply_(8, 8, 32, 30, 32, 0, 0) == -1 and apply_(8, 8, 30, 30, 32, 0, 0) == -1
    assert apply_(16, 8, 32, 32, 8, 0, 0) == -1 and apply_(8, 8, 32, 32, 32, 25, 0) == -1 and apply_(8, 8, 32, 32, 32, 0, 3) == -1
    assert b"fr_sst_apply" in lib.fr_last_error_string()
    assert apply_(16, 8, 32, 32, 32, 24, 2) == -1 and b"required" in lib.fr_last_error_string()
    bwd = lambda rows, b, q, ld, ldg, ldw, index, kind: lib.fr_sst_bwd(  # noqa: E731
        None, None, None, None, None, rows, b, q, ld, ldg, ldw, index, kind, 0.0, 0.0, 30.0, None)
    assert bwd(8, 8, 32, 32, 28, 32, 0, 0) == -1 and bwd(8, 8, 32, 32, 34, 32, 0, 0) == -1 and bwd(9, 8, 32, 32, 32, 32, 0, 0) == -1
    assert b"fr_sst_bwd" in lib.fr_last_error_string()
    assert lib.fr_ema_step(None, None, 0, 0.5, 0.5, None) == 0 and lib.fr_ema_step(None, None, -3, 0.5, 0.5, None) == 0
    assert lib.fr_ema_step(None, None, 4, 0.5, 0.5, None) == -1 and b"fr_ema_step" in lib.fr_last_error_string()


def test_device_entries_refuse_host_tensors():
    """No quiet fall-back: the functional entry is the HIP path and says so when handed host tensors."""
    from frhip import _lib
    from frhip import functional as FRF
    z = torch.zeros(16, 32)
    with pytest.raises(_lib.FrhipError):
        FRF.sst_forward(z, z, torch.zeros(8, dtype=torch.int64), torch.zeros(32, 32), torch.zeros(32, 32),
                        torch.zeros(32, dtype=torch.int64), 0, True, 0, 0.0, 0.0, 30.0)
