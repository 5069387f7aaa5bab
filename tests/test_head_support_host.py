"""Negative controls for tests/head_support.py, on the host: a helper that quietly stopped checking would pass every GPU
test that leans on it, so each moved check is shown here to raise on the smallest violation and to pass without one.  And
train.py's refusal of SHARDED_HEAD, message by message, against the text it had as five separate blocks."""
import pytest
import torch

import head_support as HS


def test_guarded_buffer_catches_one_float_on_either_side():
    """Guarded(3, 5) on the host: the interior has the shape asked for and starts a multiple of 16 bytes into the flat
    buffer; untouched guard bands pass; one float written to the last element of the front band, or to the first of the
    back band, raises."""
    g = HS.Guarded(3, 5, device="cpu")
    assert tuple(g.t.shape) == (3, 5) and g.flat.numel() == 2 * HS.BAND + 15 and bool((g.flat == HS.SENTINEL).all())
    assert (g.t.data_ptr() - g.flat.data_ptr()) % 16 == 0 and g.t.data_ptr() - g.flat.data_ptr() == 4 * HS.BAND
    g.assert_guards("untouched")
    g.t.fill_(1.0)  # the interior is the caller's
    g.assert_guards("interior written")
    assert bool((g.flat[HS.BAND:HS.BAND + 15] == 1.0).all())
    for where, index in (("front", HS.BAND - 1), ("back", HS.BAND + 15)):
        g = HS.Guarded(3, 5, device="cpu")
        g.flat[index] = 0.5
        with pytest.raises(AssertionError, match=where):
            g.assert_guards(where)


def test_ckpt_wants_exactly_one_file(tmp_path):
    with pytest.raises(AssertionError, match="Head_X_"):
        HS.ckpt(tmp_path, "Head_X_")
    (tmp_path / "Head_X_Epoch_1_a.pth").write_bytes(b"")
    (tmp_path / "Backbone_Epoch_1.pth").write_bytes(b"")
    assert HS.ckpt(tmp_path, "Head_X_") == str(tmp_path / "Head_X_Epoch_1_a.pth")
    (tmp_path / "Head_X_Epoch_1_b.pth").write_bytes(b"")
    with pytest.raises(AssertionError, match="Head_X_"):
        HS.ckpt(tmp_path, "Head_X_")
    assert HS.ckpt(tmp_path, "Head_X_Epoch_1_b") == str(tmp_path / "Head_X_Epoch_1_b.pth")


def test_state_comparison_sees_one_bit_and_the_key_order():
    a = {"kernel": torch.tensor([[1.0, -2.0], [0.25, 3.0]]), "t": torch.tensor([0.5])}
    same = {k: v.clone() for k, v in a.items()}
    HS.assert_same_state(a, same, "equal")
    one_bit = {k: v.clone() for k, v in a.items()}
    one_bit["kernel"][1, 0] = torch.nextafter(a["kernel"][1, 0], torch.tensor(1.0))
    assert float(one_bit["kernel"][1, 0]) - 0.25 == 2.0 ** -25  # the neighbouring fp32 value: 2^-2 x 2^-23
    with pytest.raises(AssertionError, match="kernel"):
        HS.assert_same_state(a, one_bit, "one bit")
    with pytest.raises(AssertionError, match="order"):
        HS.assert_same_state(a, {"t": a["t"], "kernel": a["kernel"]}, "order")
    with pytest.raises(AssertionError, match="missing"):
        HS.assert_same_state(a, {"kernel": a["kernel"]}, "missing")


def test_maxrel_and_relerr_by_hand():
    """got = (3, 4.5), ref = (3, 4): the difference is (0, 0.5).  maxrel = 0.5 / max|ref| = 0.5 / 4; relerr =
    |(0, 0.5)| / |(3, 4)| = 0.5 / 5.  Both in float64, whatever the inputs' type."""
    got, ref = torch.tensor([3.0, 4.5]), torch.tensor([3.0, 4.0])
    assert HS.maxrel(got, ref) == 0.125 and HS.relerr(got, ref) == 0.1
    assert HS.maxrel(ref, ref) == 0.0 and HS.relerr(ref, ref) == 0.0
    assert HS.maxrel(got.double(), ref) == 0.125


REFUSALS = {
    "MagFace": "SHARDED_HEAD=True with HEAD_NAME 'MagFace': the class-sharded head does not serve MagFace (its radial term and "
               "loss_g need an exchange of their own); run it replicated, SHARDED_HEAD=False",
    "AdaCos": "SHARDED_HEAD=True with HEAD_NAME 'AdaCos': the class-sharded head does not serve AdaCos (its row sums and "
              "target cosines need an exchange of their own); run it replicated, SHARDED_HEAD=False",
    "NPCFace": "SHARDED_HEAD=True with HEAD_NAME 'NPCFace': the class-sharded head does not serve NPCFace (its target cosines "
               "and per-row hard sums and counts need an exchange of their own); run it replicated, SHARDED_HEAD=False",
    "MV_Softmax": "SHARDED_HEAD=True with HEAD_NAME 'MV_Softmax': the class-sharded head does not serve MV_Softmax (its target "
                  "cosines need an exchange of their own); run it replicated, SHARDED_HEAD=False",
    "CircleLoss": "SHARDED_HEAD=True with HEAD_NAME 'CircleLoss': the class-sharded head does not serve CircleLoss (it is "
                  "element-wise on the cosines and needs no exchange of its own, but it is not wired into the sharded head); "
                  "run it replicated, SHARDED_HEAD=False",
    "AM_Softmax": "SHARDED_HEAD=True with HEAD_NAME 'AM_Softmax': the class-sharded head does not serve AM_Softmax (it is "
                  "element-wise on the cosines and needs no exchange of its own, but it is not wired into the sharded head); "
                  "run it replicated, SHARDED_HEAD=False",
}


def test_check_head_config_keeps_every_refusal_word_for_word():
    """The six heads the class-sharded head does not serve: the NotImplementedError's text is character for character what
    train.py raised when each head had a block of its own; without SHARDED_HEAD, and for the heads the sharded head does
    serve, nothing is raised."""
    import train
    assert sorted(train.NOT_SHARDED) == sorted(REFUSALS)
    for name, text in REFUSALS.items():
        with pytest.raises(NotImplementedError) as e:
            train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
        assert str(e.value) == text
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=False))
        train.check_head_config(dict(HEAD_NAME=name))
    for name in ("ArcFace", "CosFace", "SphereFace", "Am_softmax", "CurricularFace"):
        train.check_head_config(dict(HEAD_NAME=name, SHARDED_HEAD=True))
