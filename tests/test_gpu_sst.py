"""SST_Prototype and ParamEMA on the GPU: the head against the reference's own vectors (g27), larger sizes against float64,
the C entry points alone in guarded buffers on hand-made cosines, the pipeline (no host read, no ATen GEMM, the one-step
rule, reproducibility, every mode advances the queue), fr_ema_step bit for bit, and one semi-siamese step end to end.

Bars, and where each comes from:
  logits              1e-3 absolute against the reference / float64: the project's bar (BASELINE.json)
  g27 gradients       max(5e-3, 8 x the reference's own fp32-vs-float64 deviation ``dev.*``) of max|ref|: the sibling heads' bar
  larger sizes        gradients by norm within max(1e-3, 8 x the host fp32 run's own deviation), as test_gpu_arcneg.py
  entry points        bit for bit the torch fp32 expression on the same cosines (a NaN is a NaN, whatever its payload), its
                      square root taken correctly rounded (sst_data.sqrt_rn: torch.sqrt of host float32 is an ulp off in
                      about 6 elements of 1000, the kernels' sqrtf is not)
  queue, labels, EMA  exact
"""
import copy
import ctypes
import math
import os
import random

import numpy as np
import pytest
import torch

import sst_data as SD
from head_support import Guarded, assert_forward_stays_on_device, maxrel, relerr
from test_gpu_loss_optim import IDLE, SIZES, Arena, device_table, shuffled_chunks

pytestmark = pytest.mark.gpu

from frhip import _lib, ops, synth  # noqa: E402
from frhip._lib import FR_F32  # noqa: E402
from head.metrics import SST_Prototype  # noqa: E402

B, D, Q, CALLS = 8, 512, 32, 5
COIN_SEED = 27


@pytest.fixture(autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g27(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "g27_sst_prototype.npz")))


def bits(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if torch.is_tensor(a) else a).tobytes()


def same_bits_or_nan(got, want):
    """Equal bit for bit wherever ``want`` is a number; a NaN where it is a NaN."""
    got, want = got.detach().cpu().numpy(), want.detach().cpu().numpy()
    nan = np.isnan(want)
    return bool((np.isnan(got) == nan).all()) and got[~nan].tobytes() == want[~nan].tobytes()


def row_normalize(x):
    """fr_row_normalize's rows of a device tensor [R, D]."""
    x = x.contiguous().float()
    xn, inv = torch.empty_like(x), torch.empty(x.shape[0], device=x.device)
    ops.call("fr_row_normalize", x, xn, None, inv, x.shape[0], x.shape[0], x.shape[1], 0, FR_F32, ops.current_stream_ptr())()
    return xn


def device_head(queue0, loss_type, margin, size):
    head = SST_Prototype(queue0.shape[0], size, scale=SD.SCALE, loss_type=loss_type, margin=margin)
    head.queue = queue0.clone()
    return head.cuda()


def step_on_device(head, p1, g2, p2, g1, ids, go1, go2):
    """One forward + backward on the device: (out1, out2, label, id_set, gp1, gp2)."""
    a1, a2 = p1.cuda().requires_grad_(True), p2.cuda().requires_grad_(True)
    b1, b2 = g1.cuda().requires_grad_(True), g2.cuda().requires_grad_(True)
    o1, o2, label, id_set = head(a1, b2, a2, b1, ids)
    ((o1 * go1.cuda()).sum() + (o2 * go2.cuda()).sum()).backward()
    assert b1.grad is None and b2.grad is None
    return o1.detach().cpu(), o2.detach().cpu(), label, id_set, a1.grad.cpu(), a2.grad.cpu()


# ------------------------------------------------------------------------------------------------ g27 on the device


@pytest.mark.parametrize("loss_type,margin", SD.LOSS_TYPES)
def test_device_head_matches_the_reference(g27, loss_type, margin):
    queue0 = SD.initial_queue(synth, "g27", D, Q)
    head = device_head(queue0, loss_type, margin, Q)
    written = torch.zeros(Q, dtype=torch.bool)
    random.seed(COIN_SEED)
    figures = {}
    for k in range(CALLS):
        pre = "%s.%d." % (loss_type, k)
        p1, g2, p2, g1, ids, go1, go2 = SD.step(synth, "g27." + loss_type, k, B, D, Q, queue0)
        SD.assert_covers(p1, g2, p2, g1)
        index = head.index
        o1, o2, label, id_set, gp1, gp2 = step_on_device(head, p1, g2, p2, g1, ids, go1, go2)
        for name, got in (("out1", o1), ("out2", o2)):
            figures[pre + name] = float((got.double() - torch.from_numpy(g27[pre + name]).double()).abs().max())
            assert figures[pre + name] < 1e-3, figures
        for name, got in (("gp1", gp1), ("gp2", gp2)):
            fig = (maxrel(got, torch.from_numpy(g27[pre + name])), max(5e-3, 8 * float(g27[pre + "dev." + name])))
            figures[pre + name] = fig
            assert fig[0] < fig[1], figures
        assert label.is_cuda and label.dtype == torch.int64 and label.shape == (B,)
        assert label.cpu().tolist() == g27[pre + "label"].tolist()
        assert head.index == int(g27[pre + "index"])
        assert sorted(id_set) == g27[pre + "id_set"].tolist() and id_set == set(g27[pre + "id_set"].tolist())
        assert head.label_list == g27[pre + "label_list"].tolist() and head.get_id_set() == set(id_set)
        window = head.queue[:, index:index + B].t()
        n1, n2 = row_normalize(g1.cuda()), row_normalize(g2.cuda())
        coin = int(g27[pre + "coin"])
        assert bits(window) == bits(n1 if coin else n2) and bits(n1) != bits(n2)  # the coin, and fr_row_normalize's bits
        assert float((window.cpu().double() - torch.from_numpy(g27[pre + "window"]).double().t()).abs().max()) < 1e-6
        assert bits(head.queue_t) == bits(head.queue.t().contiguous())
        written[index:index + B] = True
        keep = ~written
        assert bits(head.queue[:, keep.cuda()]) == bits(queue0[:, keep])  # every other column keeps its initial bits
    print("g27 on the device:", loss_type, figures)


# ------------------------------------------------------------------------------------------------ larger sizes


def big_case(tag, Bb, Qb, index, loss_type, margin, backward):
    queue0 = SD.initial_queue(synth, tag, D, Qb)
    p1, g2, p2, g1, ids, go1, go2 = SD.step(synth, tag, 0, Bb, D, Qb, queue0)
    SD.assert_covers(p1, g2, p2, g1)
    head = device_head(queue0, loss_type, margin, Qb)
    head.load_queue_state(index, [-1] * Qb)
    random.seed(1)
    if not backward:
        with torch.no_grad():
            o1, o2, label, _ = head(p1.cuda(), g2.cuda(), p2.cuda(), g1.cuda(), ids)
        r1, r2, _, _ = SD.reference64(queue0, index, p1, g2, p2, g1, loss_type, margin, SD.SCALE, go1, go2)
        return dict(out1=float((o1.cpu().double() - r1).abs().max()), out2=float((o2.cpu().double() - r2).abs().max())), head
    o1, o2, label, _, gp1, gp2 = step_on_device(head, p1, g2, p2, g1, ids, go1, go2)
    r1, r2, rg1, rg2 = SD.reference64(queue0, index, p1, g2, p2, g1, loss_type, margin, SD.SCALE, go1, go2)
    host = SST_Prototype(D, Qb, scale=SD.SCALE, loss_type=loss_type, margin=margin)
    host.queue = queue0.clone()
    host.load_queue_state(index, [-1] * Qb)
    a1, a2 = p1.clone().requires_grad_(True), p2.clone().requires_grad_(True)
    h1, h2, _, _ = host(a1, g2, a2, g1, ids)
    ((h1 * go1).sum() + (h2 * go2).sum()).backward()
    assert label.cpu().tolist() == list(range(index, index + Bb)) and head.index == (index + Bb) % Qb
    return dict(out1=float((o1.double() - r1).abs().max()), out2=float((o2.double() - r2).abs().max()),
                gp1=(relerr(gp1, rg1), relerr(a1.grad, rg1)), gp2=(relerr(gp2, rg2), relerr(a2.grad, rg2))), head


@pytest.mark.parametrize("Bb,Qb,index,loss_type,margin", [(8, 96, 88, "arc_softmax", 0.5), (64, 1024, 960, "am_softmax", 0.35)])
def test_larger_sizes_against_float64(Bb, Qb, index, loss_type, margin):
    """B = 8, Q = 96 from index 88 (the window at the row's end; three 32-column tiles) and B = 64, Q = 1024 from 960,
    forward + backward, against float64: logits within 1e-3, gradients by norm within max(1e-3, 8 x the host fp32 run's own
    deviation)."""
    figures, head = big_case("big%d" % Qb, Bb, Qb, index, loss_type, margin, True)
    print("B = %d, Q = %d:" % (Bb, Qb), figures)
    assert figures["out1"] < 1e-3 and figures["out2"] < 1e-3, figures
    for name in ("gp1", "gp2"):
        assert figures[name][0] < max(1e-3, 8 * figures[name][1]), (name, figures)
    assert bits(head.queue_t) == bits(head.queue.t().contiguous())


def test_default_size_logits_against_float64():
    """B = 256, Q = 16384 (the head's default queue), forward only: logits within 1e-3 of float64."""
    figures, head = big_case("big16384", 256, 16384, 512, "arc_softmax", 0.5, False)
    print("B = 256, Q = 16384:", figures)
    assert figures["out1"] < 1e-3 and figures["out2"] < 1e-3, figures
    assert head.index == 768


# ------------------------------------------------------------------------------------------------ fr_sst_apply, fr_sst_bwd

KINDS = (("softmax", 0.0), ("am_softmax", 0.35), ("arc_softmax", 0.5))


def hand_made(rows, Bh, Qh, index, ldw):
    """cos [rows, Qh] and cw [rows, ldw] on the host: random cosines in (-0.9, 0.9), target cosines 0.2 .. 0.95 on the
    label columns of cw, garbage where nothing may be read (the window of cos: 7, cw outside the row's block: 9), and the
    special rows: exactly +-1, raw values 1 + 2^-23 and -1 - 2^-22, both outside and inside the window but off the label
    column, and a NaN row."""
    cos = synth.uniform(31, "hand.cos.%d.%d" % (rows, index), (rows, Qh), -0.9, 0.9)
    cw = torch.full((rows, ldw), 9.0)
    inner = synth.uniform(31, "hand.cw.%d.%d" % (rows, index), (rows, Bh), -0.9, 0.9)
    for m in range(rows):
        blk, j = m // Bh, m % Bh
        inner[m, j] = 0.2 + 0.75 * ((m * 5) % rows) / max(1, rows - 1)
        cw[m, blk * Bh:(blk + 1) * Bh] = inner[m]
    out_cols = [c for c in range(Qh) if not index <= c < index + Bh]
    specials = (1.0, -1.0, 1.0 + 2.0 ** -23, -1.0 - 2.0 ** -22)
    for t, v in enumerate(specials):
        cos[0, out_cols[3 + 5 * t]] = v
        cos[rows - 1, out_cols[-2 - 3 * t]] = v
        m = 1 + t % (rows - 1)
        cw[m, (m // Bh) * Bh + (m % Bh + 1 + t) % Bh] = v  # off the label column j = m % Bh
    cos[:, index:index + Bh] = 7.0
    cos[3, :] = float("nan")
    cw[3, :] = float("nan")
    return cos, cw


def substituted(cos, cw, Bh, index):
    full = cos.clone()
    for m in range(cos.shape[0]):
        blk = m // Bh
        full[m, index:index + Bh] = cw[m, blk * Bh:(blk + 1) * Bh]
    return full


@pytest.mark.parametrize("rows", [8, 16])
@pytest.mark.parametrize("index", [0, 88])
def test_apply_and_bwd_on_hand_made_cosines(rows, index):
    """fr_sst_apply and fr_sst_bwd alone, B = 8, Q = 96 at pitch 100 (four padding columns), the window at column 0 and at
    Q - B, rows = B and 2 B, all three kinds: bit for bit the torch fp32 expression on the substituted cosines; gcos exactly
    0 in the window and the padding, gwin the window columns in the rows' blocks and 0 outside; guard bands intact."""
    Bh, Qh, ld, ldg, ldw = 8, 96, 100, 128, 32
    cos, cw = hand_made(rows, Bh, Qh, index, ldw)
    full = substituted(cos, cw, Bh, index)
    label = torch.arange(rows) % Bh + index
    g = synth.normal(31, "hand.g.%d.%d" % (rows, index), (rows, Qh))
    cos_d = torch.full((rows, ld), 5.0)
    cos_d[:, :Qh] = cos
    cos_d, cw_d, g_d = cos_d.cuda(), cw.cuda(), g.cuda()
    st = ops.current_stream_ptr()
    win = torch.zeros(Qh, dtype=torch.bool)
    win[index:index + Bh] = True
    for kind, (loss_type, margin) in enumerate(KINDS):
        p0, p1 = (math.cos(margin), math.sin(margin)) if kind == 2 else (margin, 0.0)
        want = SD.from_cos(full, label, loss_type, margin, SD.SCALE, sqrt=SD.sqrt_rn)
        out = Guarded(rows, ld)
        ops.call("fr_sst_apply", cos_d, cw_d, out.t, rows, Bh, Qh, ld, ldw, index, kind, p0, p1, SD.SCALE, st)()
        torch.cuda.synchronize()
        out.assert_guards("fr_sst_apply")
        assert same_bits_or_nan(out.t[:, :Qh], want), (kind, float((out.t[:, :Qh].cpu() - want).abs().nan_to_num().max()))
        assert bool((out.t[:, Qh:] == 0).all())
        assert float(want[0].abs().max()) == SD.SCALE  # the clamp acted on the row of specials
        # the backward expression: (g * s) * d under the clamp's pass mask of the raw cosine
        gs = g * SD.SCALE
        passed = (full >= -1) & (full <= 1)
        d = torch.ones_like(full)
        if kind == 2:
            c = full.gather(1, label.view(-1, 1))
            d = d.scatter(1, label.view(-1, 1), p0 + (c / SD.sqrt_rn(1 - c * c)) * p1)
        gfull = torch.where(passed, gs * d, torch.zeros_like(gs))
        gcos, gwin = Guarded(rows, ldg), Guarded(rows, ldw)
        ops.call("fr_sst_bwd", g_d, cos_d, cw_d, gcos.t, gwin.t, rows, Bh, Qh, ld, ldg, ldw, index, kind, p0, p1, SD.SCALE,
                 st)()
        torch.cuda.synchronize()
        gcos.assert_guards("fr_sst_bwd gcos")
        gwin.assert_guards("fr_sst_bwd gwin")
        got = gcos.t.cpu()
        assert bits(got[:, :Qh][:, ~win]) == bits(gfull[:, ~win]), kind
        assert bool((got[:, :Qh][:, win] == 0).all()) and bool((got[:, Qh:] == 0).all())
        assert bits(got[3]) == bits(torch.zeros(ldg))  # the NaN row passes nothing
        wgot = gwin.t.cpu()
        for m in range(rows):
            blk = m // Bh
            inside = torch.zeros(ldw, dtype=torch.bool)
            inside[blk * Bh:(blk + 1) * Bh] = True
            assert bits(wgot[m, inside]) == bits(gfull[m, win]), (kind, m)
            assert bool((wgot[m, ~inside] == 0).all()), (kind, m)
        assert bool(torch.isfinite(wgot).all()) and float(wgot.abs().max()) > 0


@pytest.mark.parametrize("Bh,Dh,Qh,index", [(8, 512, 96, 88), (70, 100, 160, 3)])
def test_enqueue_writes_the_window_and_nothing_else(Bh, Dh, Qh, index):
    gn = row_normalize(synth.normal(32, "enq.g", (Bh, Dh)).cuda())
    ids = (torch.arange(Bh, dtype=torch.int64) * 3 + 11).cuda()
    q0 = synth.uniform(32, "enq.q", (Dh, Qh))
    q, qt, labels = Guarded(Dh, Qh), Guarded(Qh, Dh), Guarded(2 * Qh)
    q.t.copy_(q0)
    qt.t.copy_(q0.t())
    lab = labels.t.view(torch.int64)
    lab.fill_(-1)
    ops.call("fr_sst_enqueue", gn, ids, qt.t, q.t, lab, index, Bh, Dh, Qh, ops.current_stream_ptr())()
    torch.cuda.synchronize()
    for buf, what in ((q, "q"), (qt, "qt"), (labels, "labels")):
        buf.assert_guards("fr_sst_enqueue " + what)
    want = q0.clone()
    want[:, index:index + Bh] = gn.cpu().t()
    assert bits(q.t) == bits(want) and bits(qt.t) == bits(want.t().contiguous())
    want_l = torch.full((Qh,), -1, dtype=torch.int64)
    want_l[index:index + Bh] = ids.cpu()
    assert lab.cpu().tolist() == want_l.tolist()


# ------------------------------------------------------------------------------------------------ the pipeline


def small_head(loss_type="arc_softmax", margin=0.5, size=96):
    queue0 = SD.initial_queue(synth, "pipe", D, size)
    return device_head(queue0, loss_type, margin, size), queue0


def test_forward_waits_for_no_host_read_and_calls_no_aten_gemm(monkeypatch):
    head, queue0 = small_head()
    p1, g2, p2, g1, ids, _, _ = SD.step(synth, "pipe", 0, B, D, 96, queue0)
    xc = torch.cat([p1, p2]).cuda().requires_grad_(True)
    gc2, gc1, idc = g2.cuda(), g1.cuda(), ids.cuda()

    def call(x, _unused):
        return head(x[:B], gc2, x[B:], gc1, idc)[0]

    names = assert_forward_stays_on_device(monkeypatch, call, xc, idc, xc)
    assert head.index == 3 * B and any("sst" in n for n in names), sorted(set(names))


def test_backward_after_a_second_forward_raises():
    head, queue0 = small_head()
    p1, g2, p2, g1, ids, _, _ = SD.step(synth, "pipe", 0, B, D, 96, queue0)
    a1 = p1.cuda().requires_grad_(True)
    o1, _, _, _ = head(a1, g2.cuda(), p2.cuda(), g1.cuda(), ids)
    head(a1, g2.cuda(), p2.cuda(), g1.cuda(), ids)
    with pytest.raises(RuntimeError, match="the queue holds one step at a time"):
        o1.sum().backward()


def test_two_runs_from_one_seed_are_bit_identical_and_every_mode_advances_the_queue():
    runs = []
    for _ in range(2):
        head, queue0 = small_head("am_softmax", 0.35)
        random.seed(9)
        res = []
        for k in range(3):
            p1, g2, p2, g1, ids, go1, go2 = SD.step(synth, "pipe", k, B, D, 96, queue0)
            o1, o2, _, _, gp1, gp2 = step_on_device(head, p1, g2, p2, g1, ids, go1, go2)
            res += [o1, o2, gp1, gp2]
        runs.append(res + [head.queue.cpu(), head.queue_t.cpu(), head.labels.cpu()])
    assert all(bits(a) == bits(b) for a, b in zip(*runs))
    head.eval()
    before = head.queue.clone()
    with torch.no_grad():
        o1, _, label, id_set = head(p1.cuda(), g2.cuda(), p2.cuda(), g1.cuda(), [5] * B)
    assert head.index == 4 * B and not o1.requires_grad and label.cpu().tolist() == list(range(3 * B, 4 * B))
    assert 5 in id_set and head.label_list[3 * B:4 * B] == [5] * B
    assert not torch.equal(head.queue[:, 3 * B:4 * B], before[:, 3 * B:4 * B])
    assert torch.equal(head.queue[:, :3 * B], before[:, :3 * B]) and torch.equal(head.queue[:, 4 * B:], before[:, 4 * B:])
    o1, _, label, _ = head(p1[:1].cuda(), g2[:1].cuda(), p2[:1].cuda(), g1[:1].cuda(), torch.tensor([6]))  # B = 1
    assert label.shape == (1,) and o1.shape == (1, 96)
    sd = head.state_dict()
    assert list(sd.keys()) == ["queue"]
    other = SST_Prototype(D, 96, scale=SD.SCALE, loss_type="am_softmax", margin=0.35).cuda()
    other.load_state_dict(sd)
    other.load_queue_state(*head.queue_state())
    random.seed(4)
    a = head(p1.cuda(), g2.cuda(), p2.cuda(), g1.cuda(), ids)
    random.seed(4)
    b = other(p1.cuda(), g2.cuda(), p2.cuda(), g1.cuda(), ids)  # queue_t is rebuilt from the loaded queue
    assert bits(a[0]) == bits(b[0]) and bits(a[1]) == bits(b[1]) and bits(other.queue_t) == bits(head.queue_t)


def test_sizes_the_device_path_refuses():
    head = SST_Prototype(D, 48).cuda()
    p1, g2, p2, g1, ids, _, _ = SD.step(synth, "odd", 0, B, D, 48, SD.initial_queue(synth, "odd", D, 48))
    with pytest.raises(NotImplementedError, match="queue_size % 32"):
        head(p1.cuda(), g2.cuda(), p2.cuda(), g1.cuda(), ids)
    assert head.index == 0
    o1, _, _, _ = SST_Prototype(D, 48)(p1, g2, p2, g1, ids)
    assert o1.shape == (B, 48)
    head, _ = small_head()
    head.load_queue_state(96 - B + 1, [-1] * 96)
    with pytest.raises(RuntimeError, match="runs past the queue"):
        head(p1.cuda(), g2.cuda(), p2.cuda(), g1.cuda(), ids)
    assert head.index == 96 - B + 1 and head.get_id_set() == set()


# ------------------------------------------------------------------------------------------------ fr_ema_step


@pytest.mark.parametrize("alpha", [0.999, 0.5])
def test_ema_step_bit_for_bit(alpha):
    """Two steps over tensors of 1 .. 12289 elements in one guarded arena at offsets off 16 bytes: dst is bit for bit the
    np.float32 restatement (two products and a sum, each rounded), src, the bands and the tensor without a chunk untouched."""
    rng = np.random.default_rng(21)
    arena = Arena(("dst", "src"))
    state = {}
    for name in arena.names:
        for t, n in enumerate(SIZES + (IDLE,)):
            state[name, t] = rng.standard_normal(n).astype(np.float32)
            arena.set(name, t, state[name, t])
    arena.upload()
    raw, table = device_table(_lib.FrEmaTensor, [dict(dst=arena.ptr("dst", t), src=arena.ptr("src", t), n=n)
                                                 for t, n in enumerate(SIZES + (IDLE,))])
    chunks, nchunks = shuffled_chunks(22)
    assert _lib.lib.fr_ema_chunk_elems() == 4096
    a, b = float(alpha), float(1.0 - alpha)
    a32, b32 = np.float32(a), np.float32(b)
    for step in range(2):
        ops.Launch("fr_ema_step", [table, ctypes.c_void_p(chunks.data_ptr()), nchunks, a, b, ops.current_stream_ptr()])()
        got = arena.download("fr_ema_step, step %d" % step)
        for t in range(len(SIZES)):
            want = (a32 * state["dst", t]).astype(np.float32) + (b32 * state["src", t]).astype(np.float32)
            want = want.astype(np.float32)
            mine = arena.get(got, "dst", t)
            diff = int((mine.view(np.int32) != want.view(np.int32)).sum())
            assert diff == 0, (step, t, SIZES[t], diff, "elements differ from the fp32 restatement")
            assert arena.get(got, "src", t).tobytes() == state["src", t].tobytes()
            state["dst", t] = want
        for name in arena.names:
            assert arena.get(got, name, len(SIZES)).tobytes() == state[name, len(SIZES)].tobytes(), (step, "idle", name)
    assert _lib.lib.fr_ema_step(table, ctypes.c_void_p(chunks.data_ptr()), 0, a, b, ops.current_stream_ptr()) == 0
    assert arena.download("nchunks = 0").tobytes() == got.tobytes()


# ------------------------------------------------------------------------------------------------ one semi-siamese step


def semi_siamese_run(steps=3):
    from backbone.model_irse import IR_50
    from frhip.optim import SGD, ParamEMA
    from loss.softmax import CrossEntropyLoss
    from util.utils import separate_irse_bn_paras
    Bs, Qs, alpha = 4, 32, 0.999
    torch.manual_seed(5)
    random.seed(5)
    probe = IR_50([112, 112])
    synth.fill_state_dict(probe.state_dict(), 15)
    probe.output_layer[1].p = 0.0
    gallery = copy.deepcopy(probe)
    probe, gallery = probe.cuda().train(), gallery.cuda().train()
    head = device_head(SD.initial_queue(synth, "e2e", D, Qs), "am_softmax", 0.35, Qs)
    bn, wo = separate_irse_bn_paras(probe)
    opt = SGD([{"params": wo, "weight_decay": 5e-4}, {"params": bn}], lr=0.01, momentum=0.9)
    ema = ParamEMA(gallery, probe, alpha)
    ce = CrossEntropyLoss()
    a32, b32 = np.float32(alpha), np.float32(1.0 - alpha)
    want = [p.detach().cpu().numpy().copy() for p in gallery.parameters()]
    record = []
    for k in range(steps):
        x1 = synth.uniform(7, "e2e.x1.%d" % k, (Bs, 3, 112, 112)).cuda()
        x2 = synth.uniform(7, "e2e.x2.%d" % k, (Bs, 3, 112, 112)).cuda()
        x = torch.cat([x1, x2])
        with torch.no_grad():
            g = gallery(x)
        p = probe(x)
        state = random.getstate()
        take_g1 = random.random() > 0.5
        random.setstate(state)
        index = head.index
        o1, o2, label, _ = head(p[:Bs], g[Bs:], p[Bs:], g[:Bs], torch.arange(Bs) + 10 * k)
        loss = (ce(o1, label) + ce(o2, label)) / 2
        opt.zero_grad()
        loss.backward()
        assert math.isfinite(float(loss.detach()))
        for name, q in probe.named_parameters():
            assert q.grad is not None and bool(torch.isfinite(q.grad).all()), name
        assert all(q.grad is None for q in gallery.parameters())
        opt.step()
        ema.step()
        torch.cuda.synchronize()
        chosen = row_normalize(g[:Bs] if take_g1 else g[Bs:])
        assert bits(head.queue[:, index:index + Bs].t()) == bits(chosen), k
        for w, q, s in zip(want, gallery.parameters(), probe.parameters()):
            w[...] = ((a32 * w).astype(np.float32) + (b32 * s.detach().cpu().numpy()).astype(np.float32)).astype(np.float32)
            assert bits(q) == w.tobytes(), k
        record += [loss.detach().cpu(), head.queue.cpu()]
    record += [q.detach().cpu() for q in probe.parameters()] + [q.detach().cpu() for q in gallery.parameters()]
    return record


def test_one_semi_siamese_step_end_to_end():
    """IR_50 probe and gallery (a deep copy) in train mode, two views of 4 identities stacked into one batch of 8, Q = 32,
    three steps of gallery forward under no_grad, probe forward, the head, the mean of the two cross entropies, backward,
    SGD and ParamEMA: finite loss and probe gradients, no gallery gradient, the gallery parameters bit for bit the np.float32
    restatement of the three updates, every written window bit for bit the normalised gallery embedding of the chosen
    view, and a second run from the same seeds bit-identical."""
    first = semi_siamese_run()
    second = semi_siamese_run()
    assert len(first) == len(second) and all(bits(a) == bits(b) for a, b in zip(first, second))
