"""CPU checks of the Softmax head (reference head/metrics.py:12-63) and the LOSS_NAME 'Softmax' cross entropy: the host paths
are ``F.linear`` / ``F.cross_entropy`` and reproduce the reference's own vectors (g25_softmax,
tests/golden/make_golden_softmax.py) bit for bit, three deliberately wrong variants each miss them, the module keeps the
reference's layout, the C ABI of the HIP path is declared, exported and checks its arguments before any launch, and train.py
takes both names."""
import ctypes
import inspect
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import softmax_data as SD
from frhip import synth

NEW_ENTRIES = ("fr_ce_finalize", "fr_pack_rows", "fr_pad_cols", "fr_col_sums")
MISS = 1e-3  # a wrong variant must miss by far more than any fp32 bar of the GPU tests (2e-6 .. 1e-5)


@pytest.fixture(scope="module")
def g25(golden_dir):
    return np.load(os.path.join(golden_dir, "g25_softmax.npz"))


def inputs_of(g, B, N):
    x, w, b, label = SD.case(synth, B, N)
    assert torch.equal(label, torch.from_numpy(g[SD.tag_of(B, N) + ".label"]))
    return x, w, b, label


def make_head(w, b):
    from head.metrics import Softmax
    head = Softmax(w.shape[1], w.shape[0], None)
    with torch.no_grad():
        head.weight.copy_(w)
        head.bias.copy_(b)
    return head


def ref(g, B, N, name):
    return torch.from_numpy(g["%s.%s" % (SD.tag_of(B, N), name)])


def maxrel(got, want):
    return float((got.double() - want.double()).abs().max() / want.double().abs().max())


@pytest.mark.parametrize("B,N", SD.CASES)
def test_host_path_is_f_linear_and_f_cross_entropy_bit_for_bit(g25, B, N):
    """Logits, loss, gx, gbias and the kept rows of gw equal the reference's fp32 values bit for bit, and the expressions
    ``F.linear`` / ``F.cross_entropy`` evaluated here; the norm of the whole of gw to 1e-6."""
    from loss.softmax import CrossEntropyLoss
    x, w, b, label = inputs_of(g25, B, N)
    assert int(label[0]) == 0 and int(label[-1]) == N - 1 and float(b.abs().min()) > 0
    assert 5.0 < float(g25[SD.tag_of(B, N) + ".logit_absmax"]) < 12.0
    head = make_head(w, b)
    xx = x.clone().requires_grad_(True)
    y = head(xx, label)
    loss = CrossEntropyLoss()(y, label)
    assert loss.dim() == 0  # the scalar, not FocalLoss's tuple
    loss.backward()
    assert torch.equal(y, F.linear(x, w, b)) and torch.equal(loss, F.cross_entropy(F.linear(x, w, b), label))
    assert torch.equal(y.detach(), ref(g25, B, N, "logits"))
    assert torch.equal(loss.detach(), ref(g25, B, N, "loss"))
    assert torch.equal(xx.grad, ref(g25, B, N, "gx"))
    assert torch.equal(head.bias.grad, ref(g25, B, N, "gb"))
    idx = ref(g25, B, N, "gw_index")
    assert torch.equal(idx, SD.gw_rows(label, N))
    assert torch.equal(head.weight.grad.index_select(0, idx), ref(g25, B, N, "gw"))
    assert abs(float(head.weight.grad.double().norm()) / float(g25[SD.tag_of(B, N) + ".gw_norm"]) - 1) < 1e-6
    # the bias gradient is the column sum of d loss / d logits; in row order it is fr_col_sums' definition
    z = y.detach().clone().requires_grad_(True)
    (gz,) = torch.autograd.grad(F.cross_entropy(z, label), [z])
    assert maxrel(SD.col_sums_in_row_order(gz), ref(g25, B, N, "gb")) < 1e-6


@pytest.mark.parametrize("B,N", SD.CASES)
def test_wrong_variants_miss_the_fixture(g25, B, N):
    """No bias; the bias added before the scale of a margin head (ArcFace's path at m = 0: s * (cos + bias)); the loss summed
    instead of averaged.  Each misses g25 by more than ``MISS``; the right expressions do not."""
    x, w, b, label = inputs_of(g25, B, N)
    logits, loss = ref(g25, B, N, "logits"), ref(g25, B, N, "loss")
    right = F.linear(x, w, b)
    assert maxrel(right, logits) < 1e-6 and maxrel(F.cross_entropy(right, label), loss) < 1e-6
    no_bias = F.linear(x, w)
    assert maxrel(no_bias, logits) > MISS and maxrel(F.cross_entropy(no_bias, label), loss) > MISS
    margin_path = 64.0 * (F.linear(F.normalize(x), F.normalize(w)) + b)
    assert maxrel(margin_path, logits) > MISS and maxrel(F.cross_entropy(margin_path, label), loss) > MISS
    summed = F.cross_entropy(right, label, reduction="sum")
    assert maxrel(summed, loss) > MISS and abs(float(summed) / float(loss) - B) < 1e-5
    gb = ref(g25, B, N, "gb")
    z = right.clone().requires_grad_(True)
    (gz,) = torch.autograd.grad(F.cross_entropy(z, label, reduction="sum"), [z])
    assert maxrel(gz.sum(0), gb) > MISS


# ------------------------------------------------------------------------------------------------ the module


def test_head_keeps_the_reference_layout():
    """Constructor (in_features, out_features, device_id), parameters ``weight`` [N, D] (xavier_uniform_) and ``bias`` [N]
    (zero), state-dict keys in the reference's order, the labels accepted and ignored, the empty batch on the host."""
    from head.metrics import Softmax
    from util.utils import separate_irse_bn_paras
    sig = inspect.signature(Softmax.__init__)
    assert list(sig.parameters)[1:] == ["in_features", "out_features", "device_id"]
    torch.manual_seed(0)
    h = Softmax(512, 10, None)
    assert list(h.state_dict()) == ["weight", "bias"] and [n for n, _ in h.named_parameters()] == ["weight", "bias"]
    assert list(h.buffers()) == [] and tuple(h.weight.shape) == (10, 512) and tuple(h.bias.shape) == (10,)
    assert (h.in_features, h.out_features, h.device_id) == (512, 10, None)
    bound = math.sqrt(6.0 / (512 + 10))  # xavier_uniform_, gain 1
    assert 0.9 * bound < float(h.weight.detach().abs().max()) <= bound
    assert bool((h.bias.detach() == 0).all())
    torch.manual_seed(0)
    same = torch.empty(10, 512)
    torch.nn.init.xavier_uniform_(same)
    assert torch.equal(same, h.weight.detach())  # the reference's draw from the same generator state
    x = synth.uniform(3, "sm.x", (3, 512))
    y = torch.tensor([0, 9, 3])
    with torch.no_grad():
        h.bias.copy_(synth.uniform(3, "sm.b", (10,)))
    out = h(x)
    assert out.shape == (3, 10) and out.device.type == "cpu"
    assert torch.equal(out, h(x, y)) and torch.equal(out, h(x, label=y)) and torch.equal(out, F.linear(x, h.weight, h.bias))
    assert h(x[:0], y[:0]).shape == (0, 10)
    bn, rest = separate_irse_bn_paras(h)
    assert bn == [] and len(rest) == 2 and rest[0] is h.weight and rest[1] is h.bias
    h2 = Softmax(512, 10, None)
    h2.load_state_dict(h.state_dict())
    assert torch.equal(h2.weight, h.weight) and torch.equal(h2.bias, h.bias)


def test_host_loss_is_nn_cross_entropy():
    from loss.softmax import CrossEntropyLoss
    z = synth.normal(4, "sm.z", (5, 7), std=3.0)
    y = torch.tensor([0, 6, 2, 2, 5])
    assert torch.equal(CrossEntropyLoss()(z, y), torch.nn.CrossEntropyLoss()(z, y))
    assert list(CrossEntropyLoss().state_dict()) == []


# ------------------------------------------------------------------------------------------------ the C ABI


def test_new_entries_are_declared_and_exported():
    from frhip import _lib
    from frhip import functional as FRF
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_ENTRIES:
        assert name in _lib.protos, "include/frhip.h does not declare %s" % name
        assert hasattr(lib, name), "libfrhip.so does not export %s" % name
    assert _lib.lib.fr_abi_version() == 7  # no struct changed
    assert _lib.protos["fr_ce_finalize"][2] == ["ce", "rank", "rows", "scalars", "stream"]
    assert _lib.protos["fr_col_sums"][2] == ["g", "rows", "N", "ldg", "out", "stream"]
    assert _lib.protos["fr_pack_rows"][2] == ["w", "bias", "wp", "wt", "biasp", "rows", "rows_pad", "D", "ldt", "stream"]
    assert _lib.protos["fr_pad_cols"][2] == ["g", "out", "rows", "N", "ldg", "ldo", "stream"]
    for name in ("SOFTMAX", "softmax_linear_forward", "softmax_linear_backward", "SoftmaxHeadFn", "softmax_head",
                 "CrossEntropyFn", "cross_entropy"):
        assert hasattr(FRF, name)
    assert FRF.SOFTMAX == 12 and FRF.ARCNEG == 11 and FRF.ARCFACE == 0
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "frhip.h")).read()
    at = header.index("Softmax head (head/metrics.py:12-63)")
    assert at < header.index("int fr_pack_rows(") < header.index("int fr_pad_cols(") < header.index("int fr_col_sums(")
    ce = header.index("int fr_ce_finalize(")
    assert header.index("int fr_focal_bwd(") < ce < at and "train.py:237-238" in header[header.index("int fr_focal_bwd("):ce]


def test_new_entries_reject_bad_arguments_without_a_gpu():
    """Argument checks run before any launch: empty shapes, row pitches that are too short or not multiples of 4, missing
    pointers.  Every refusal returns -1 and names its entry point."""
    from frhip import _lib
    lib = _lib.lib
    one = ctypes.c_void_p(16)  # a pointer that is not NULL; no call below gets as far as a launch
    fin = lambda rows, ce=one, rank=one, sc=one: lib.fr_ce_finalize(ce, rank, rows, sc, None)  # noqa: E731
    assert fin(0) == -1 and fin(-1) == -1 and fin(8, ce=None) == -1 and fin(8, rank=None) == -1 and fin(8, sc=None) == -1
    assert b"fr_ce_finalize" in lib.fr_last_error_string()
    cs = lambda rows, n, ldg, g=one, out=one: lib.fr_col_sums(g, rows, n, ldg, out, None)  # noqa: E731
    assert cs(0, 33, 64) == -1 and cs(7, 0, 64) == -1 and cs(-1, 33, 64) == -1 and cs(7, 33, 32) == -1
    assert cs(7, 33, 64, g=None) == -1 and cs(7, 33, 64, out=None) == -1
    assert b"fr_col_sums" in lib.fr_last_error_string()
    def pk(rows, pad, d, ldt, w=one, wp=one, wt=one):
        return lib.fr_pack_rows(w, None, wp, wt, None, rows, pad, d, ldt, None)

    assert pk(0, 64, 512, 64) == -1 and pk(33, 64, 0, 64) == -1 and pk(33, 32, 512, 64) == -1  # empty, pad < rows
    assert pk(33, 64, 512, 32) == -1 and pk(33, 64, 512, 66) == -1  # pitch too short, not a multiple of 4
    assert pk(33, 64, 512, 64, w=None) == -1 and pk(33, 64, 512, 64, wp=None) == -1 and pk(33, 64, 512, 64, wt=None) == -1
    assert b"fr_pack_rows" in lib.fr_last_error_string()
    pc = lambda rows, n, ldg, ldo, g=one, out=one: lib.fr_pad_cols(g, out, rows, n, ldg, ldo, None)  # noqa: E731
    assert pc(0, 33, 33, 64) == -1 and pc(7, 0, 33, 64) == -1 and pc(7, 33, 32, 64) == -1  # empty, input pitch too short
    assert pc(7, 33, 33, 32) == -1 and pc(7, 33, 33, 34) == -1  # output pitch too short, not a multiple of 4
    assert pc(7, 33, 33, 64, g=None) == -1 and pc(7, 33, 33, 64, out=None) == -1
    assert b"fr_pad_cols" in lib.fr_last_error_string()


def test_device_entries_refuse_host_tensors():
    """No quiet fall-back: the functional entries are the HIP path and say so when handed host tensors, the empty batch
    (which launches nothing) included."""
    from frhip import _lib
    from frhip import functional as FRF
    x, w, b = torch.zeros(2, 32), torch.ones(5, 32), torch.ones(5)
    y = torch.tensor([0, 4])
    for rows in (2, 0):
        with pytest.raises(_lib.FrhipError):
            FRF.softmax_head(x[:rows], w, b)
        with pytest.raises(_lib.FrhipError):
            FRF.cross_entropy(torch.zeros(rows, 5), y[:rows])


# ------------------------------------------------------------------------------------------------ train.py, the sharded head


def test_train_py_takes_both_names():
    """check_head_config accepts HEAD_NAME 'Softmax' with and without SHARDED_HEAD and keeps its refusals; train.py builds
    the head inside a fork_rng block of its own, just before ArcNegFace, and selects the HIP cross entropy for LOSS_NAME
    'Softmax'."""
    import train
    for cfg in (dict(HEAD_NAME="Softmax"), dict(HEAD_NAME="Softmax", SHARDED_HEAD=False),
                dict(HEAD_NAME="Softmax", SHARDED_HEAD=True)):
        train.check_head_config(cfg)
    assert "Softmax" not in train.NOT_SHARDED and "Softmax" not in train.NOT_SHARDED_ROW_VALUE
    assert sorted(train.NOT_SHARDED) == ["AM_Softmax", "AdaCos", "CircleLoss", "MV_Softmax", "MagFace", "NPCFace"]
    src = open(train.__file__).read()
    outer = src.index("with torch.random.fork_rng(devices=[])")
    inner = src.index("with torch.random.fork_rng(devices=[])", outer + 10)
    line = src.index('heads["Softmax"] = Softmax(emb, num_class, None)')
    assert outer < src.index('heads["AM_Softmax"]') < inner < line < src.index('heads["ArcNegFace"]')
    assert src.index('heads["ArcNegFace"]') < src.index("head = heads[cfg")
    assert src[inner:line].count("\n") == 1  # the block holds this line alone
    assert "from loss.softmax import CrossEntropyLoss" in src
    assert 'CrossEntropyLoss() if cfg["LOSS_NAME"] == "Softmax" else torch.nn.CrossEntropyLoss()' in src
    assert "SHARDED_HEAD needs LOSS_NAME 'Focal'" in src  # every other loss name is still refused
    common = open(os.path.join(os.path.dirname(train.__file__), "configs", "_common.py")).read()
    assert "| Softmax" in common


def test_seeded_heads_keep_their_initial_weights():
    """Drawing the Softmax head inside a fork_rng block leaves the generator where it was: what is drawn after it has the
    bits it had without it."""
    from head.metrics import Softmax
    torch.manual_seed(7)
    before = torch.rand(4)
    torch.manual_seed(7)
    with torch.random.fork_rng(devices=[]):
        Softmax(16, 5, None)
    assert torch.equal(torch.rand(4), before)


def test_sharded_head_names_and_slices():
    """One rank, no process group, on the host (nothing is launched): the Softmax head and loss are known names, the bias is
    a second parameter sliced like the weight's rows, and the one-dimensional slice / gather round trip."""
    from frhip import functional as FRF
    from frhip import sharded_head as SH
    from head.metrics import Softmax
    assert SH.LINEAR_KINDS == {"Softmax": FRF.SOFTMAX} and "Softmax" not in SH.KINDS  # KINDS: the five margin heads
    assert SH.CLASS_DIM["Softmax"] == 0 and "Softmax" in SH.DEFAULTS
    with pytest.raises(ValueError, match="loss must be one of"):
        SH.ShardedMarginLoss(16, 5, "ArcFace", loss="Hinge")
    assert SH.ShardedMarginLoss(16, 5, "ArcFace").loss == "Focal"
    head = Softmax(16, 5, None)
    with torch.no_grad():
        head.bias.copy_(torch.arange(5.0))
    crit = SH.ShardedMarginLoss.from_head(head, loss="Softmax")
    assert crit.loss == "Softmax" and [n for n, _ in crit.named_parameters()] == ["weight", "bias"]
    assert torch.equal(crit.weight, head.weight) and torch.equal(crit.bias, head.bias)
    assert torch.equal(crit.gather_weight(), head.weight) and torch.equal(crit.gather_bias(), head.bias)
    assert torch.equal(crit.slice_full(torch.arange(5.0)), torch.arange(5.0))
    crit.load_full_weight(torch.ones(5, 16), torch.full((5,), 2.0))
    assert bool((crit.weight == 1).all()) and bool((crit.bias == 2).all())
    fresh = SH.ShardedMarginLoss(16, 5, "Softmax", loss="Softmax")
    assert bool((fresh.bias == 0).all()) and tuple(fresh.weight.shape) == (5, 16)
    with pytest.raises(ValueError, match="full_bias"):
        SH.ShardedMarginLoss(16, 5, "Softmax", full_bias=torch.zeros(4))
