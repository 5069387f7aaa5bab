"""Host tests of RandAugment (no GPU): the numpy restatement of tests/randaug_ref.py against the installed Pillow, called as
the reference's ``func`` calls it -- every served operation x 10 magnitudes x both signs, bit for bit, with the coverage
the comparison needs asserted and with negative controls the same comparison catches; the host class
``data_processing.randaugment.Rand_Augment`` and the restatement against the recorded outputs of the reference's own class
(g28); the policy draws of ``GpuRandAugment``; the C ABI of ``fr_randaug_u8`` and its refusals, which come back before any
launch; ``train.check_randaug_config``."""
import ctypes
import inspect
import os
import random

import numpy as np
import pytest
import torch
from PIL import Image, ImageEnhance, ImageOps

import randaug_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g28_randaugment.npz")


def _images():
    rng = np.random.RandomState(5)
    return {"112x112": rng.randint(0, 256, (112, 112, 3)).astype(np.uint8),
            "37x53": rng.randint(0, 256, (37, 53, 3)).astype(np.uint8),
            "9x7": rng.randint(0, 256, (9, 7, 3)).astype(np.uint8),
            "constant": np.full((20, 20, 3), (200, 17, 90), np.uint8),
            "lowrange": rng.randint(90, 154, (64, 48, 3)).astype(np.uint8)}


IMAGES = _images()


def _ranges():
    from data_processing.randaugment import Rand_Augment
    return Rand_Augment().ranges


def pillow(img, name, value, sign):
    """The served operation through Pillow, the calls of the reference's ``func`` with the sign given."""
    im = Image.fromarray(img)
    if name == "translateX":
        out = im.transform(im.size, Image.AFFINE, (1, 0, value * im.size[0] * sign, 0, 1, 0), fill=128)
    elif name == "translateY":
        out = im.transform(im.size, Image.AFFINE, (1, 0, 0, 0, 1, value * im.size[1] * sign), fill=128)
    elif name == "color":
        out = ImageEnhance.Color(im).enhance(1 + value * sign)
    elif name == "contrast":
        out = ImageEnhance.Contrast(im).enhance(1 + value * sign)
    elif name == "brightness":
        out = ImageEnhance.Brightness(im).enhance(1 + value * sign)
    elif name == "posterize":
        out = ImageOps.posterize(im, value)
    elif name == "solarize":
        out = ImageOps.solarize(im, value)
    elif name == "autocontrast":
        out = ImageOps.autocontrast(im)
    elif name == "invert":
        out = ImageOps.invert(im)
    else:
        assert name == "equalize"
        out = im
    return np.asarray(out)


def restated(img, name, value, sign, **kw):
    """The same step through the restatement, by way of the (code, float32 parameter) pair the kernel is given."""
    h, w = img.shape[:2]
    par = R.parameter(name, value, sign, h, w)
    if not kw:
        return R.apply(img, R.CODE[name], par)
    if name in ("translateX", "translateY"):
        return getattr(R, name)(img, int(par), **kw)
    return getattr(R, name)(img, par, **kw)


def sweep():
    ranges = _ranges()
    for key, img in IMAGES.items():
        for name in R.SERVED:
            for m in range(10):
                for sign in (-1, 1):
                    yield key, img, name, ranges[name][m], m, sign


def test_restatement_equals_pillow_bit_for_bit():
    n = 0
    for key, img, name, value, m, sign in sweep():
        got, want = restated(img, name, value, sign), pillow(img, name, value, sign)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (key, name, m, sign, int((got != want).sum()))
        n += 1
    assert n == len(IMAGES) * len(R.SERVED) * 20


def test_the_sweep_covers_clipping_and_truncation():
    """What the blend comparison rests on: for factors above 1 values clip at 0 and at 255, for factors in [0, 1] some value
    truncates to a byte that rounding would not give; the shifts reach both directions and bring black in."""
    ranges = _ranges()
    low = high = trunc = 0
    for key, img in IMAGES.items():
        for name in ("color", "contrast", "brightness"):
            d = {"brightness": 0, "contrast": R.contrast_mean(img)}.get(name)
            d = R.luma(img)[..., None] if d is None else d
            for m in range(10):
                for sign in (-1, 1):
                    a = np.float32(1 + ranges[name][m] * sign)
                    t = R.blend_value(d, img, a)
                    if a > 1:
                        low += int((t < 0).sum())
                        high += int((t > 255).sum())
                    else:
                        assert 0 <= a <= 1 and t.min() >= 0 and t.max() <= 255, (key, name, a)  # the clip never acts
                        trunc += int((np.trunc(t) != np.floor(t + 0.5)).sum())
    print("values below 0: %d, above 255: %d (factors > 1); truncated != rounded: %d (factors in [0, 1])" % (low, high, trunc))
    assert low > 0 and high > 0 and trunc > 0
    shifts = {R.shift_of(ranges["translateX"][m], img.shape[1], s) for img in IMAGES.values() for m in range(10)
              for s in (-1, 1)}
    assert min(shifts) < 0 < max(shifts) and 0 in shifts, sorted(shifts)
    assert [int(b) for b in ranges["posterize"]] == [8, 8, 7, 7, 6, 6, 5, 5, 4, 4]
    assert np.array_equal(ranges["solarize"], np.linspace(256, 231, 10))


CONTROLS = [("blend in double", ("color", "contrast", "brightness"), {"mode": "f64"}),
            ("blend with a fused multiply-add", ("color", "contrast", "brightness"), {"mode": "fma"}),
            ("rounding instead of truncation", ("color", "contrast", "brightness"), {"rounding": "round"}),
            ("fill 128 in translate", ("translateX", "translateY"), {"fill": 128}),
            ("contrast mean without + 0.5", ("contrast",), {"half": False}),
            ("color with L in float", ("color",), {"luma_mode": "float"})]


@pytest.mark.parametrize("what,names,kw", CONTROLS, ids=[c[0] for c in CONTROLS])
def test_negative_controls_break_equality(what, names, kw):
    """The comparison with Pillow on the same inputs catches each wrong restatement."""
    wrong = total = 0
    for key, img, name, value, m, sign in sweep():
        if name in names:
            total += 1
            wrong += not np.array_equal(restated(img, name, value, sign, **kw), pillow(img, name, value, sign))
    print("%s: %d of %d cases differ from Pillow" % (what, wrong, total))
    assert wrong > 0, what


def test_the_integer_contrast_mean_is_the_double_one():
    """The kernel forms int(sum / count + 0.5) as (2 * sum + count) // (2 * count): equal for every count the LDS budget
    admits at the sums where rounding could tell them apart (k * count +- 1 around the half points), and on the images."""
    for count in (1, 2, 3, 63, 400, 1961, 3072, 12544, 16384, 20821):
        sums = {0, 255 * count}
        for k in range(0, 255, 7):
            for delta in (-2, -1, 0, 1, 2):
                for base in (k * count, k * count + count // 2, k * count + (count + 1) // 2):
                    if 0 <= base + delta <= 255 * count:
                        sums.add(base + delta)
        for total in sums:
            assert R.contrast_mean_integer(total, count) == int(float(total) / float(count) + 0.5), (total, count)
    for img in IMAGES.values():
        l = R.luma(img)
        assert R.contrast_mean_integer(l.sum(), l.size) == R.contrast_mean(img)


# ------------------------------------------------------------------------------------------------ g28: the reference's class


def _signs(seq):
    it = iter(seq)
    return lambda choices: next(it)


def test_g28_host_class_and_restatement(monkeypatch):
    from data_processing.randaugment import Rand_Augment
    g = np.load(GOLDEN)
    ra = Rand_Augment()
    assert ra.transforms == [str(n) for n in g["transforms"]] and len(ra.transforms) == 13
    assert ra.Numbers == int(g["numbers"]) == 6 and ra.max_Magnitude == int(g["max_magnitude"]) == 10
    tables = sorted(k[len("ranges."):] for k in g.files if k.startswith("ranges."))
    assert tables == sorted(ra.ranges) == sorted(ra.func) and "invert" in tables and "invert" not in ra.transforms
    for name in tables:
        assert np.array_equal(np.asarray(ra.ranges[name]), g["ranges." + name]), name
    assert Rand_Augment(3, 4).Numbers == 3 and Rand_Augment(3, 4).max_Magnitude == 4
    for key in ("random", "lowrange"):
        img = g["in." + key]
        assert img.shape == (16, 12, 3)
        for name in R.SERVED:
            want = g["single.%s.%s" % (key, name)]
            for m in range(10):
                for j, sign in enumerate((-1, 1)):
                    monkeypatch.setattr(random, "choice", _signs([sign]))
                    assert np.array_equal(ra.test_single_operation(img, name, m), want[m, j]), (key, name, m, sign)
                    assert np.array_equal(restated(img, name, ra.ranges[name][m], sign), want[m, j]), (key, name, m, sign)
    for i in range(3):
        names, mags = [str(n) for n in g["chain.%d.ops" % i]], g["chain.%d.mags" % i]
        signs, img, want = g["chain.%d.signs" % i], g["in." + str(g["chain.%d.input" % i])], g["chain.%d.out" % i]
        assert len(names) == 6 and set(names) <= set(R.SERVED)
        h, w = img.shape[:2]
        pars = [R.parameter(n, ra.ranges[n][m], s, h, w) for n, m, s in zip(names, mags, signs)]
        assert np.array_equal(R.chain(img, [R.CODE[n] for n in names], pars), want), i
        monkeypatch.setattr(random, "choice", _signs([s for s in signs if s != 0]))
        monkeypatch.setattr(ra, "rand_augment", lambda: list(zip(names, mags)))
        assert np.array_equal(ra(img), want), i


def test_host_class_runs_all_13_operations():
    """The host class refuses nothing: every name of ``transforms`` (and ``invert``) returns an image of the input's shape,
    ``equalize`` its input, and a call draws ``Numbers`` operations from numpy's generator."""
    from data_processing.randaugment import Rand_Augment
    ra = Rand_Augment()
    img = IMAGES["37x53"]
    for name in ra.transforms + ["invert"]:
        for m in (0, 5, -1):
            out = ra.test_single_operation(img, name, m)
            assert out.shape == img.shape and out.dtype == np.uint8, name
    assert np.array_equal(ra.test_single_operation(img, "equalize"), img)
    np.random.seed(3)
    plan = ra.rand_augment()
    assert len(plan) == 6 and all(n in ra.transforms and 0 <= m < 10 for n, m in plan)
    np.random.seed(3)
    random.seed(3)
    a = ra(img)
    np.random.seed(3)
    random.seed(3)
    assert np.array_equal(ra(img), a) and a.shape == img.shape


# ------------------------------------------------------------------------------------------------ the policy draws


def test_policy_draws():
    from frhip.input_pipeline import RANDAUG_CODE, RANDAUG_RANGES, SERVED, GpuRandAugment
    assert SERVED == R.SERVED and RANDAUG_CODE == R.CODE
    ranges = _ranges()
    for name in SERVED:
        assert np.array_equal(np.asarray(RANDAUG_RANGES[name], np.float64), np.asarray(ranges[name], np.float64)), name
    assert GpuRandAugment().num == 5 and GpuRandAugment(ops=("color", "invert", "solarize")).num == 1
    assert GpuRandAugment(num=16).num == 16
    for bad in (dict(num=0), dict(num=17), dict(max_magnitude=0), dict(max_magnitude=11), dict(ops=("color",))):
        with pytest.raises(ValueError):
            GpuRandAugment(**bad)
    with pytest.raises(ValueError, match="unknown operation"):
        GpuRandAugment(ops=("colour",))

    h, w = 112, 96
    ra = GpuRandAugment()
    gen = torch.Generator().manual_seed(11)
    op, par = ra.draw(4000, gen, (h, w))  # 20 000 steps
    assert op.dtype == torch.uint8 and par.dtype == torch.float32 and tuple(op.shape) == tuple(par.shape) == (4000, 5)
    op2, par2 = ra.draw(4000, torch.Generator().manual_seed(11), (h, w))
    assert torch.equal(op, op2) and torch.equal(par, par2)  # the same draws from the same generator state
    op3, _ = ra.draw(4000, gen, (h, w))
    assert not torch.equal(op, op3)  # and the generator moves on
    op, par = op.numpy().ravel(), par.numpy().ravel()
    # every (name, magnitude index, sign) the reference can reach is seen, and nothing else
    allowed = {}
    for name in SERVED:
        for m in range(10):
            for sign in (-1, 1):
                allowed.setdefault(R.CODE[name], {}).setdefault(float(R.parameter(name, ranges[name][m], sign, h, w)), set()
                                                                ).add((name, m, sign))
    seen = set()
    for code, p in zip(op.tolist(), par.tolist()):
        assert code in allowed and p in allowed[code], (code, p)
        seen |= allowed[code][p]
    assert seen == {(n, m, s) for n in SERVED for m in range(10) for s in (-1, 1)}
    # a narrower policy: only its names, magnitude indices below max_magnitude
    few = GpuRandAugment(num=3, max_magnitude=4, ops=("solarize", "brightness", "translateY"))
    op, par = few.draw(2000, torch.Generator().manual_seed(2), (h, w))
    assert tuple(op.shape) == (2000, 3) and set(op.numpy().ravel().tolist()) == {R.CODE["solarize"], R.CODE["brightness"],
                                                                                R.CODE["translateY"]}
    thr = par[op == R.CODE["solarize"]].numpy()
    assert set(thr.tolist()) == {float(np.float32(ranges["solarize"][m])) for m in range(4)}
    bright = par[op == R.CODE["brightness"]].numpy()
    assert set(bright.tolist()) == {float(np.float32(1 + ranges["brightness"][m] * s)) for m in range(4) for s in (-1, 1)}


def test_unserved_operations_are_refused_by_name():
    from frhip.input_pipeline import UNSERVED, GpuRandAugment
    assert sorted(UNSERVED) == sorted(R.UNSERVED)
    with pytest.raises(NotImplementedError, match="'rotate' is not served on the device: it goes through an RGBA composite"):
        GpuRandAugment(ops=("rotate",))
    for name, why in (("shearX", "bicubic affine resample"), ("shearY", "bicubic affine resample"),
                      ("sharpness", "3x3 smoothing filter")):
        with pytest.raises(NotImplementedError, match="'%s' is not served on the device: it needs .*%s" % (name, why)):
            GpuRandAugment(ops=("color", name))


# ------------------------------------------------------------------------------------------------ C ABI


def test_c_abi_of_the_randaug_entry():
    from frhip import _lib
    lib = _lib.lib
    header = open(_lib.HEADER).read()
    name = "fr_randaug_u8"
    assert "int %s(" % name in header and name in _lib.protos and hasattr(lib, name)
    assert _lib.protos[name][2] == ["src", "labels", "idx", "op", "par", "dst", "label_out", "M", "B", "K", "H", "W", "stream"]
    assert _lib.protos[name][1] == [ctypes.c_void_p] * 7 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    assert _lib.protos["fr_augment_u8"][2] == ["src", "xtab", "ytab", "crop", "flip", "lut", "out", "B", "Hin", "Win", "Hr",
                                               "Wr", "S", "kx", "ky", "stream"]  # the sibling keeps its signature
    assert lib.fr_abi_version() == 7 and "#define FR_ABI_VERSION 7" in header


def test_randaug_entry_refuses_before_any_launch():
    """Every refusal returns before the launch, so host pointers (never dereferenced) stand in for device ones."""
    from frhip import _lib
    lib = _lib.lib
    mem = ctypes.create_string_buffer(64)
    p = ctypes.cast(mem, ctypes.c_void_p)

    def call(M=13, B=9, K=6, H=112, W=112, src=p, labels=p, idx=p, op=p, par=p, dst=p, label_out=p):
        return lib.fr_randaug_u8(src, labels, idx, op, par, dst, label_out, M, B, K, H, W, None)

    def refused(rc, word):
        assert rc < 0, rc
        msg = lib.fr_last_error_string()
        assert b"fr_randaug_u8" in msg and word in msg, msg

    assert call(B=0) == 0 and call(B=-3) == 0
    assert call(B=0, K=0, H=1000, W=1000, src=None, op=None, par=None, dst=None) == 0  # the empty batch is served
    refused(call(B=65536), b"65535")
    for k in (0, -1, 17):
        refused(call(K=k), b"1..16")
    for hole in ("src", "op", "par", "dst"):
        refused(call(**{hole: None}), b"required")
    refused(call(M=0), b"M <= 0")
    refused(call(M=-5), b"M <= 0")
    for h, w in ((148, 148), (128, 163), (1, 20822), (0, 112), (112, -1)):
        refused(call(H=h, W=w), b"LDS")
    refused(call(H=46341, W=46341), b"LDS")  # H * W beyond 2**31


# ------------------------------------------------------------------------------------------------ train.py


def test_check_randaug_config():
    import train
    from frhip.input_pipeline import SERVED
    on = {"GPU_INPUT_PIPELINE": True, "GPU_RANDAUGMENT": True}
    for off in ({}, {"GPU_RANDAUGMENT": False}, {"GPU_INPUT_PIPELINE": True},
                {"GPU_RANDAUGMENT": False, "GPU_RANDAUGMENT_OPS": ["rotate"]}):
        assert train.check_randaug_config(off) is None
    assert train.check_randaug_config(on) == (None, 10, SERVED)
    assert train.check_randaug_config(dict(on, GPU_RANDAUGMENT_NUM=3, GPU_RANDAUGMENT_MAX_MAGNITUDE=4,
                                           GPU_RANDAUGMENT_OPS=["color", "invert"])) == (3, 4, ("color", "invert"))
    with pytest.raises(NotImplementedError, match="GPU_RANDAUGMENT=True needs GPU_INPUT_PIPELINE=True: RandAugment runs on "
                                                  "the GPU input pipeline .* the host workers do not run it"):
        train.check_randaug_config({"GPU_RANDAUGMENT": True})
    with pytest.raises(NotImplementedError, match="the host workers do not run it"):
        train.check_randaug_config({"GPU_RANDAUGMENT": True, "GPU_INPUT_PIPELINE": False})
    with pytest.raises(NotImplementedError, match="GPU_RANDAUGMENT_OPS: 'rotate' is not served on the device: it goes through "
                                                  "an RGBA composite"):
        train.check_randaug_config(dict(on, GPU_RANDAUGMENT_OPS=["color", "rotate"]))
    with pytest.raises(NotImplementedError, match="'sharpness' is not served on the device: it needs a 3x3 smoothing filter"):
        train.check_randaug_config(dict(on, GPU_RANDAUGMENT_OPS=("sharpness",)))
    with pytest.raises(NotImplementedError, match="'shearX' is not served on the device: it needs Pillow's bicubic"):
        train.check_randaug_config(dict(on, GPU_RANDAUGMENT_OPS=["shearX"]))
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError, match="GPU_RANDAUGMENT must be True or False"):
            train.check_randaug_config({"GPU_INPUT_PIPELINE": True, "GPU_RANDAUGMENT": bad})
    for bad in (0, 17, -1, 2.0, True, "3"):
        with pytest.raises(ValueError, match=r"GPU_RANDAUGMENT_NUM must be None or an integer in 1\.\.16"):
            train.check_randaug_config(dict(on, GPU_RANDAUGMENT_NUM=bad))
    for bad in (0, 11, None, 5.0, True):
        with pytest.raises(ValueError, match=r"GPU_RANDAUGMENT_MAX_MAGNITUDE must be an integer in 1\.\.10"):
            train.check_randaug_config(dict(on, GPU_RANDAUGMENT_MAX_MAGNITUDE=bad))
    for bad in ("color", 3, {"color": 1}):
        with pytest.raises(ValueError, match="GPU_RANDAUGMENT_OPS must be None or a list"):
            train.check_randaug_config(dict(on, GPU_RANDAUGMENT_OPS=bad))
    with pytest.raises(ValueError, match="GPU_RANDAUGMENT_OPS: unknown operation 'colour'"):
        train.check_randaug_config(dict(on, GPU_RANDAUGMENT_OPS=["colour"]))
    with pytest.raises(ValueError, match="GPU_RANDAUGMENT_OPS: no operation given"):
        train.check_randaug_config(dict(on, GPU_RANDAUGMENT_OPS=[]))
    with pytest.raises(ValueError, match="GPU_RANDAUGMENT_NUM=None draws"):
        train.check_randaug_config(dict(on, GPU_RANDAUGMENT_OPS=["color"]))
    from configs._common import stage3
    cfg = stage3("x")
    assert (cfg["GPU_RANDAUGMENT"], cfg["GPU_RANDAUGMENT_NUM"], cfg["GPU_RANDAUGMENT_MAX_MAGNITUDE"],
            cfg["GPU_RANDAUGMENT_OPS"]) == (False, None, 10, None)
    assert train.check_randaug_config(cfg) is None  # the shipped defaults are off
    src = inspect.getsource(train.main)
    assert src.index("check_randaug_config(cfg)") < src.index("torch.cuda.is_available()") < src.index("build_backbone(cfg)")
