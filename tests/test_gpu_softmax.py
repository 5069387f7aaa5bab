"""The Softmax head (reference head/metrics.py:12-63) and the LOSS_NAME 'Softmax' cross entropy on the HIP path: the new C
entry points alone in sentinel-filled buffers (fr_ce_finalize, fr_col_sums, fr_pack_rows, fr_pad_cols), the head against
float64 and against the reference's own vectors (g25), the loss against float64 ``F.cross_entropy``, the pipeline (no
device-to-host copy and no ATen GEMM in the forward pass, bit-reproducible, label errors, the empty batch), the class-sharded
forms on one rank and on two ranks sharing a GPU, and train.py end to end, replicated and sharded, with bit-for-bit resumes.

Bars.  Entry points that only move or add numbers in a fixed order are compared bit for bit.  The head is held to
max(2e-6, 8 x the deviation of torch's own fp32 CPU expression on the same operands from float64), measured with
``HS.maxrel`` (the form of test_gpu_arcneg.py's entry-point bars): 2e-6 is about eight fp32 ulps of the largest magnitude.
The loss is held to 2e-6 relative and the sharded forms to the bars of test_gpu_sharded_heads_ext.py."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_support as HS
import softmax_data as SD
from frhip import synth
from head_support import Guarded, SENTINEL, maxrel

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
D = SD.D


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


@pytest.fixture(scope="module")
def g25(golden_dir):
    return np.load(os.path.join(golden_dir, "g25_softmax.npz"))


def make(w, b):
    from head.metrics import Softmax
    head = Softmax(w.shape[1], w.shape[0], None)
    with torch.no_grad():
        head.weight.copy_(w)
        head.bias.copy_(b)
    return head


def bar(fp32, ref64):
    return max(2e-6, 8 * maxrel(fp32, ref64))


# ------------------------------------------------------------------------------------------------ C ABI, guarded


def _finalize(name, ce, rank, *gamma):
    from frhip import ops
    out = Guarded(8)
    ops.call(name, ce, rank, ce.shape[0], *gamma, out.t, ops.current_stream_ptr())()
    torch.cuda.synchronize()
    out.assert_guards(name)
    return out.t.cpu()


@pytest.mark.parametrize("zero", [False, True])
@pytest.mark.parametrize("rows", [1, 7, 300])
def test_ce_finalize(rows, zero):
    """fr_ce_finalize into a sentinel-filled buffer: the loss within one fp32 ulp of the float64 mean, scalars[4] with the
    bits fr_focal_finalize leaves on the same input, the slope exactly 1, both precisions exact, slots 5..7 untouched.  An
    all-zero ce (where fr_focal_finalize at gamma = 0 computes 0 * inf): loss 0, slope 1, nothing NaN."""
    ce = torch.zeros(rows) if zero else synth.uniform(25, "fin.ce%d" % rows, (rows,), 0.0, 12.0)
    rank = (synth.labels(25, "fin.rank%d" % rows, rows, 9)).to(torch.int32)
    got = _finalize("fr_ce_finalize", ce.cuda(), rank.cuda())
    focal = _finalize("fr_focal_finalize", ce.cuda(), rank.cuda(), 2.0)
    mean = float(ce.double().mean())
    ulp = float(np.spacing(np.float32(abs(mean)))) if mean else 0.0
    print("rows", rows, "loss", float(got[0]), "float64 mean", mean, "ulp", ulp, "focal at gamma 0:",
          _finalize("fr_focal_finalize", ce.cuda(), rank.cuda(), 0.0)[:2].tolist())
    assert abs(float(got[0].double()) - mean) <= ulp, (float(got[0]), mean, ulp)
    assert torch.equal(got[4:5].view(torch.int32), focal[4:5].view(torch.int32)) and torch.equal(got[0], got[4])
    assert float(got[1]) == 1.0
    for slot, k in ((2, 1), (3, 5)):
        want = np.float32(100.0) * np.float32(int((rank < k).sum())) / np.float32(rows)
        assert float(got[slot]) == float(want) == float(focal[slot]), (slot, float(got[slot]), float(want))
    assert bool((got[5:] == SENTINEL).all()) and not bool(torch.isnan(got).any())
    if zero:
        assert float(got[0]) == 0.0


@pytest.mark.parametrize("rows,N,ldg", [(5, 1, 32), (7, 33, 64), (64, 1001, 1024), (300, 4133, 4160)])
def test_col_sums(rows, N, ldg):
    """fr_col_sums in a guarded buffer, bit for bit the torch fp32 loop over the rows in order; the padding columns of g hold
    a sentinel it must not read into a sum."""
    from frhip import ops
    g = synth.normal(25, "cs.g%d" % N, (rows, N))
    gp = torch.full((rows, ldg), 12345.0)
    gp[:, :N] = g
    out = Guarded(N)
    ops.call("fr_col_sums", gp.cuda(), rows, N, ldg, out.t, ops.current_stream_ptr())()
    torch.cuda.synchronize()
    out.assert_guards("fr_col_sums")
    want = SD.col_sums_in_row_order(g)
    assert torch.equal(out.t.cpu(), want), float((out.t.cpu() - want).abs().max())
    if rows > 4:  # the order matters: another order gives other bits somewhere
        assert not torch.equal(SD.col_sums_in_row_order(g.flip(0)), want) or N == 1


@pytest.mark.parametrize("N", [1, 33, 1001])
def test_pack_rows(N):
    """fr_pack_rows at D = 512 in guarded buffers: [Np, D] and its transpose [D, Np] exact, the padding rows / columns and
    the bias's tail zero; without a bias the packed bias is all zero."""
    from frhip import ops
    Np = (N + 31) // 32 * 32
    w = synth.normal(25, "pk.w%d" % N, (N, D))
    b = synth.uniform(25, "pk.b%d" % N, (N,))
    for bias in (b, None):
        wp, wt, bp = Guarded(Np, D), Guarded(D, Np), Guarded(Np)
        ops.call("fr_pack_rows", w.cuda(), None if bias is None else bias.cuda(), wp.t, wt.t, bp.t, N, Np, D, Np,
                 ops.current_stream_ptr())()
        torch.cuda.synchronize()
        for buf, name in ((wp, "wp"), (wt, "wt"), (bp, "biasp")):
            buf.assert_guards(name)
        assert torch.equal(wp.t[:N].cpu(), w) and not bool(wp.t[N:].any())
        assert torch.equal(wt.t[:, :N].cpu(), w.t()) and not bool(wt.t[:, N:].any())
        assert torch.equal(bp.t[:N].cpu(), b if bias is not None else torch.zeros(N)) and not bool(bp.t[N:].any())


@pytest.mark.parametrize("rows,N,ldg,ldo", [(5, 1, 1, 32), (7, 33, 36, 64), (300, 4133, 4133, 4160)])
def test_pad_cols(rows, N, ldg, ldo):
    """fr_pad_cols in a guarded buffer: the first N columns with g's bits, the rest zero, whatever g's pitch."""
    from frhip import ops
    g = synth.normal(25, "pc.g%d" % N, (rows, N))
    gp = torch.full((rows, ldg), 12345.0)
    gp[:, :N] = g
    out = Guarded(rows, ldo)
    ops.call("fr_pad_cols", gp.cuda(), out.t, rows, N, ldg, ldo, ops.current_stream_ptr())()
    torch.cuda.synchronize()
    out.assert_guards("fr_pad_cols")
    assert torch.equal(out.t[:, :N].cpu(), g) and not bool(out.t[:, N:].any())


# ------------------------------------------------------------------------------------------------ the head


def head_case(B, N):
    x, w, b, _ = SD.case(synth, B, N)
    return x, w, b, synth.normal(25, "head.g%dx%d" % (B, N), (B, N))


def expression(x, w, b, g):
    """(logits, gx, gw, gb) of F.linear under the upstream gradient g, in the dtype of the operands."""
    return F.linear(x, w, b), g @ w, g.t() @ x, g.sum(0)


@pytest.mark.parametrize("B,N", [(7, 33), (64, 1001), (16, 4133), (8, 28000)])
def test_head_against_float64(B, N):
    """Forward and backward at D = 512 with a non-zero bias: logits, gx, gweight and gbias within ``bar`` of float64; the
    padding columns of the logit store are zero; one-sided backward calls give the bits of the two-sided one; gbias is, bit
    for bit, the torch loop over the rows in order."""
    from frhip import functional as FRF
    x, w, b, g = head_case(B, N)
    ref = expression(x.double(), w.double(), b.double(), g.double())
    f32 = expression(x, w, b, g)
    head = make(w, b).cuda()
    xc = x.cuda().requires_grad_(True)
    y = head(xc, None)
    y.backward(g.cuda())
    got = (y.detach().cpu(), xc.grad.cpu(), head.weight.grad.cpu(), head.bias.grad.cpu())
    figures = {n: (maxrel(a, r), bar(f, r)) for n, a, f, r in zip(("logits", "gx", "gw", "gb"), got, f32, ref)}
    print(B, N, figures)
    for name, (err, lim) in figures.items():
        assert err <= lim, (name, figures)
    assert torch.equal(got[3], SD.col_sums_in_row_order(g))
    with torch.no_grad():
        logits, saved, cfg = FRF.softmax_linear_forward(x.cuda(), head.weight.detach(), head.bias.detach())
        assert torch.equal(logits.cpu(), got[0]) and cfg.ld == (N + 3) // 4 * 4 and logits.stride(0) == cfg.ld
        store = torch.as_strided(logits, (B, cfg.ld), (cfg.ld, 1))
        assert not bool(store[:, N:].any())
        both = FRF.softmax_linear_backward(saved, cfg, g.cuda(), True, True)
        only_x = FRF.softmax_linear_backward(saved, cfg, g.cuda(), True, False)
        only_w = FRF.softmax_linear_backward(saved, cfg, g.cuda(), False, True)
    assert only_x[1] is None and only_x[2] is None and only_w[0] is None
    assert torch.equal(both[0], only_x[0]) and torch.equal(both[1], only_w[1]) and torch.equal(both[2], only_w[2])
    for a, c in zip(both, got[1:]):
        assert torch.equal(a.cpu(), c)


@pytest.mark.parametrize("B,N", SD.CASES)
def test_device_matches_the_reference(g25, B, N):
    """g25, head + loss: logits, loss, gx, gbias and the kept rows of gw within ``bar`` of the reference's fp32 values, the
    bar from the deviation of those values (torch's fp32 CPU expression) from a float64 run of the same expression."""
    from loss.softmax import CrossEntropyLoss
    tag = SD.tag_of(B, N)
    x, w, b, label = SD.case(synth, B, N)
    assert torch.equal(label, torch.from_numpy(g25[tag + ".label"]))
    idx = torch.from_numpy(g25[tag + ".gw_index"])
    xd, wd, bd = x.double().requires_grad_(True), w.double().requires_grad_(True), b.double().requires_grad_(True)
    y64 = F.linear(xd, wd, bd)
    l64 = F.cross_entropy(y64, label)
    gx64, gw64, gb64 = torch.autograd.grad(l64, [xd, wd, bd])
    ref64 = dict(logits=y64.detach(), loss=l64.detach().view(1), gx=gx64, gw=gw64.index_select(0, idx), gb=gb64)
    head = make(w, b).cuda()
    xc = x.cuda().requires_grad_(True)
    y = head(xc, label.cuda())
    loss = CrossEntropyLoss()(y, label.cuda())
    loss.backward()
    got = dict(logits=y.detach().cpu(), loss=loss.detach().cpu().view(1), gx=xc.grad.cpu(),
               gw=head.weight.grad.cpu().index_select(0, idx), gb=head.bias.grad.cpu())
    figures = {}
    for name in got:
        want = torch.from_numpy(g25["%s.%s" % (tag, name)]).view(got[name].shape)
        figures[name] = (maxrel(got[name], want), bar(want, ref64[name]))
    print(tag, figures)
    for name, (err, lim) in figures.items():
        assert err <= lim, (name, figures)
    assert abs(float(head.weight.grad.double().norm()) / float(g25[tag + ".gw_norm"]) - 1) <= figures["gw"][1]


# ------------------------------------------------------------------------------------------------ the loss


@pytest.mark.parametrize("B,N", [(5, 1), (7, 33), (64, 1001), (16, 4133)])
def test_cross_entropy_against_float64(B, N):
    """FRF.cross_entropy against float64 F.cross_entropy: loss within 2e-6 relative, gradient maxrel <= 1e-5 (exactly zero
    at N = 1, where the reference's is), every gradient row summing to 0 within 1e-6 of its largest entry, and the gradient
    bit for bit fr_focal_bwd run by hand at slope 1."""
    from frhip import functional as FRF, ops
    z = synth.normal(25, "ce.z%d" % N, (B, N), std=3.0)
    label = synth.labels(25, "ce.y%d" % N, B, N)
    label[0], label[B - 1] = 0, N - 1
    zd = z.double().requires_grad_(True)
    l64 = F.cross_entropy(zd, label)
    (g64,) = torch.autograd.grad(l64, [zd])
    zc = z.cuda().requires_grad_(True)
    loss = FRF.cross_entropy(zc, label.cuda())
    loss.backward()
    grad = zc.grad.cpu()
    rel = abs(float(loss.detach()) - float(l64.detach())) / max(1.0, abs(float(l64.detach())))
    rows = (grad.double().sum(1).abs(), grad.double().abs().max(1).values)
    print(B, N, "loss", float(loss.detach()), float(l64.detach()), rel, "grad", maxrel(grad, g64) if N > 1 else 0.0,
          "row sums / largest", float((rows[0] / rows[1].clamp(min=1e-30)).max()))
    assert rel <= 2e-6
    if float(g64.abs().max()) == 0.0:
        assert not bool(grad.any())
    else:
        assert maxrel(grad, g64) <= 1e-5
    assert bool((rows[0] <= 1e-6 * rows[1]).all()), (rows[0] / rows[1].clamp(min=1e-30)).max()
    st = ops.current_stream_ptr()
    lse, ce = torch.empty(B, device="cuda"), torch.empty(B, device="cuda")
    rank = torch.empty(B, device="cuda", dtype=torch.int32)
    ops.call("fr_ce_rows", zc.detach(), label.cuda(), lse, ce, rank, B, N, N, st)()
    scalars = torch.tensor([0.0, 1.0, 0, 0, 0, 0, 0, 0], device="cuda")
    by_hand = Guarded(B, N)
    ops.call("fr_focal_bwd", zc.detach(), label.cuda(), lse, scalars, torch.ones(1, device="cuda"), by_hand.t, B, N, N, st)()
    torch.cuda.synchronize()
    by_hand.assert_guards("fr_focal_bwd")
    assert torch.equal(by_hand.t.cpu(), grad)


# ------------------------------------------------------------------------------------------------ the pipeline


def test_forward_waits_for_no_host_read_and_calls_no_aten_gemm(monkeypatch):
    """torch.profiler over head + loss (labels validated by the caller, as in train.py): no device-to-host copy, no scalar
    read, no ATen GEMM; the same over forward + backward with torch.mm / matmul / F.linear raising; the kernels that ran are
    the new ones."""
    from frhip import functional as FRF
    from loss.softmax import CrossEntropyLoss
    B, N = 16, 301
    x, w, b, label = SD.case(synth, B, N)
    head, crit = make(w, b).cuda(), CrossEntropyLoss()
    xc, lc = x.cuda().requires_grad_(True), label.cuda()
    monkeypatch.setattr(FRF, "CHECK_LABELS", False)
    names = HS.assert_forward_stays_on_device(monkeypatch, lambda xx, ll: crit(head(xx, ll), ll), xc, lc, head.weight)
    assert bool(torch.isfinite(head.bias.grad).all())
    for kernel in ("pack_rows_kernel", "ce_rows_kernel", "ce_finalize_kernel"):
        assert sum(kernel in n for n in names) == 1, (kernel, sorted(set(names)))
    assert not any("focal_finalize" in n or "row_normalize" in n for n in names), sorted(set(names))


def test_reproducible_labels_checked_and_empty_batch(monkeypatch):
    """Bitwise equal logits, loss and the three gradients run to run and with FRHIP_SINGLE_STREAM=1; a label of N raises the
    shared label check's error under CHECK_LABELS; the empty batch gives [0, N] logits, a NaN loss and zero gradients."""
    from frhip import functional as FRF
    from loss.softmax import CrossEntropyLoss
    B, N = 96, 7001
    x, w, b, label = SD.case(synth, B, N)
    head, crit = make(w, b).cuda(), CrossEntropyLoss()
    outs = []
    for single in ("0", "0", "1"):
        monkeypatch.setenv("FRHIP_SINGLE_STREAM", single)
        head.zero_grad()
        xc = x.cuda().requires_grad_(True)
        y = head(xc, label.cuda())
        loss = crit(y, label.cuda())
        loss.backward()
        outs.append([t.detach().cpu().clone() for t in (y, loss, xc.grad, head.weight.grad, head.bias.grad)])
    for o in outs[1:]:
        for a, c in zip(outs[0], o):
            assert torch.equal(a, c)
    assert FRF.CHECK_LABELS
    bad = label.clone()
    bad[3] = N
    with pytest.raises(RuntimeError, match="out of bounds for dimension 1 with size %d" % N):
        crit(y.detach(), bad.cuda())
    head.zero_grad()
    xe = torch.empty(0, D, device="cuda", requires_grad=True)
    ye = head(xe, torch.empty(0, dtype=torch.long, device="cuda"))
    assert tuple(ye.shape) == (0, N)
    le = crit(ye, torch.empty(0, dtype=torch.long, device="cuda"))
    assert le.dim() == 0 and bool(torch.isnan(le))
    ye.sum().backward()
    assert head.weight.grad is not None and not bool(head.weight.grad.any()) and not bool(head.bias.grad.any())
    assert tuple(xe.grad.shape) == (0, D)


# ------------------------------------------------------------------------------------------------ the class-sharded forms


def _rel(a, b):
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("N,B", [(100, 8), (1001, 16), (7000, 64)])
@pytest.mark.parametrize("name", ["Softmax", "ArcFace"])
def test_one_rank_equals_replicated_head(name, N, B):
    """Without a process group the sharded module is the whole head: over two steps loss, both precisions and every
    gradient (the bias's included) equal the replicated HIP head + CrossEntropyLoss + accuracy -- loss 2e-6 relative,
    gradients 1e-5 by norm -- and the host path on the CPU within 1e-3 (the bars of test_gpu_sharded_heads_ext.py)."""
    from frhip.sharded_head import ShardedMarginLoss
    from head import metrics as H
    from loss.softmax import CrossEntropyLoss
    from oracle import irse_ref as O
    from util.utils import accuracy
    x0, w, b, y = SD.case(synth, B, N)
    if name == "Softmax":
        head = make(w, b).cuda()
        crit = ShardedMarginLoss.from_head(head, loss="Softmax").cuda()
    else:
        w = w * 0.05
        head = H.ArcFace(D, N, None).cuda()
        with torch.no_grad():
            head.weight.copy_(w)
        crit = ShardedMarginLoss(D, N, "ArcFace", loss="Softmax", full_weight=w).cuda()
    assert (crit.lo, crit.hi) == (0, N) and crit.grad_scale == 1.0 and crit.loss == "Softmax"
    pairs = list(zip(crit.parameters(), head.parameters()))
    assert len(pairs) == (2 if name == "Softmax" else 1)
    for step in range(2):
        crit.zero_grad()
        head.zero_grad()
        x = x0.cuda().requires_grad_(True)
        loss, p1, p5 = crit(x, y.cuda())
        loss.backward()
        xr = x0.cuda().requires_grad_(True)
        logits = head(xr, y.cuda())
        rloss = CrossEntropyLoss()(logits, y.cuda())
        rloss.backward()
        e1, e5 = accuracy(logits.detach(), y.cuda(), topk=(1, 5))
        rels = [_rel(x.grad, xr.grad)] + [_rel(pc.grad, ph.grad) for pc, ph in pairs]
        print("%s N %d B %d step %d: loss %.8f replicated %.8f  gx, gw(, gb) %s" % (
            name, N, B, step, float(loss.detach()), float(rloss), rels))
        assert abs(float(loss.detach()) - float(rloss)) <= 2e-6 * max(1.0, abs(float(rloss)))
        assert float(p1) == float(e1) and float(p5) == float(e5)
        assert all(r <= 1e-5 for r in rels), rels
        xo = x0.clone().requires_grad_(True)
        hw = w.clone().requires_grad_(True)
        hb = b.clone().requires_grad_(True)
        if name == "Softmax":
            lo = F.cross_entropy(F.linear(xo, hw, hb), y)
            host = torch.autograd.grad(lo, [xo, hw, hb])
        else:
            lo = F.cross_entropy(O.arcface_forward(xo, hw, y, s=64.0, m=0.5, easy_margin=False), y)
            host = torch.autograd.grad(lo, [xo, hw])
        assert abs(float(loss.detach()) - float(lo)) < 1e-3
        for got, want in zip([x.grad] + [pc.grad for pc, _ in pairs], host):
            assert _rel(got.cpu(), want) < 1e-3
    with pytest.raises(RuntimeError):
        crit(x.detach(), torch.full((B,), N, device="cuda"))
    with pytest.raises(Exception):
        crit(x0, y)  # host tensors: no CPU fallback


def test_two_ranks_sharing_one_gpu():
    """World 2 over gloo on GPU 0 (3 GPU processes in all): the comparisons of tests/test_softmax_gloo.py with the HIP
    kernels, in tests/shard_softmax_worker.py."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
           "127.0.0.1", "--master-port", "29587", os.path.join(HERE, "shard_softmax_worker.py")]
    out = HS.child(cmd, REPO, env, 300)
    assert out.returncode == 0 and "SHARD_SOFTMAX_WORKER_OK" in out.stdout, out.stdout[-4000:] + out.stderr[-1500:]


# ------------------------------------------------------------------------------------------------ train.py

SOFT = dict(HEAD_NAME="Softmax", LOSS_NAME="Softmax")


def test_train_py_softmax_replicated_resumes_bit_for_bit(tmp_path):
    """HEAD_NAME = LOSS_NAME = 'Softmax' on the synthetic config: 12 steps with finite loss, the Head_* file with ``weight``
    [12, 512] and ``bias`` [12]; 12 steps straight == 6 steps, stop at the epoch boundary, resume for 6, bit for bit."""
    losses, sd, sa, _ = HS.straight_and_resumed(tmp_path, SOFT, "Softmax", 2)
    assert list(sd) == ["weight", "bias"] and tuple(sd["weight"].shape) == (12, 512) and tuple(sd["bias"].shape) == (12,)
    assert bool(torch.isfinite(sd["weight"]).all()) and bool(sd["bias"].any())  # the bias moved off zero
    assert not torch.equal(sa["weight"], sd["weight"]) and not torch.equal(sa["bias"], sd["bias"])


def _sharded_train(tmp, tag, cfg, max_steps=0):
    model_dir, stdout = HS.run_train(tmp, tag, dict(cfg, SHARDED_HEAD=True), max_steps=max_steps, limit=300)
    assert "Training Loss" in stdout and "nan" not in stdout.lower(), stdout[-2000:]
    return model_dir, stdout


def test_train_py_sharded_arcface_with_the_softmax_loss(tmp_path):
    """HEAD_NAME = 'ArcFace', LOSS_NAME = 'Softmax', SHARDED_HEAD: 3 steps with a finite loss, where the parent commit
    raised NotImplementedError."""
    d, log = _sharded_train(tmp_path, "arc", dict(HEAD_NAME="ArcFace", LOSS_NAME="Softmax"), max_steps=3)
    sd = torch.load(HS.ckpt(d, "Head_ArcFace_Epoch_1_Batch_3_"), map_location="cpu")
    assert list(sd) == ["weight"] and bool(torch.isfinite(sd["weight"]).all())


def test_train_py_sharded_softmax_resumes_bit_for_bit(tmp_path):
    """The class-sharded Softmax head under the cross entropy: 12 steps straight == 6 steps, stop, resume for 6 -- backbone,
    weight, bias and momentum bit for bit; the Head_* file holds the gathered ``weight`` (12, 512) and ``bias`` (12,), the
    Optimizer_* file a momentum buffer of each shape."""
    a_dir, _ = _sharded_train(tmp_path, "straight", SOFT)
    b1_dir, _ = _sharded_train(tmp_path, "first", SOFT, max_steps=6)
    sd = torch.load(HS.ckpt(b1_dir, "Head_Softmax_Epoch_1_Batch_6_"), map_location="cpu")
    assert list(sd) == ["weight", "bias"] and tuple(sd["weight"].shape) == (12, 512) and tuple(sd["bias"].shape) == (12,)
    assert bool(torch.isfinite(sd["weight"]).all()) and bool(sd["bias"].any())
    osd = torch.load(HS.ckpt(b1_dir, "Optimizer_Softmax_Epoch_1_Batch_6_"), map_location="cpu")
    shapes = [tuple(v["momentum_buffer"].shape) for v in osd["state"].values()]
    assert (12, 512) in shapes and (12,) in shapes
    b2_dir, log = _sharded_train(tmp_path, "second", HS.resume_cfg(SOFT, b1_dir, "Softmax"))
    assert "Resuming at epoch 1 batch 6" in log and "Loading Optimizer Checkpoint" in log
    HS.assert_same_checkpoints(a_dir, b2_dir, "Softmax", "Epoch_2_Batch_12_")
