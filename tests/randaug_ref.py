"""numpy restatement of the served RandAugment operations (data_processing/randaugment.py on Pillow), the arithmetic spelled
out: what ``fr_randaug_u8`` is held to bit for bit (tests/test_gpu_randaug.py) and what tests/test_randaug_host.py pins
against the installed Pillow.  A plain module, not a test module.

Images are uint8 [H, W, 3].  Every function returns a new uint8 array: Pillow rounds to uint8 between operations.

``blend``: ``Image.blend(degenerate, image, a)`` is ``d + a * (i - d)`` in float32 with the product and the sum rounded
separately; Pillow truncates where 0 <= a <= 1 and clips otherwise (<= 0 -> 0, >= 255 -> 255, else truncates).  Inside
0 <= a <= 1 the value lies between d and i, so the clip never acts there and one expression serves both branches.
The keyword arguments of ``blend`` / ``luma`` / ``contrast_mean`` / ``translate`` exist for the negative controls of the
host test (each must break equality with Pillow); the defaults are the restatement."""
import math

import numpy as np

SERVED = ("autocontrast", "equalize", "solarize", "color", "posterize", "contrast", "brightness", "translateX",
          "translateY", "invert")
UNSERVED = ("rotate", "shearX", "shearY", "sharpness")
CODE = {"equalize": 0, "autocontrast": 1, "solarize": 2, "color": 3, "posterize": 4, "contrast": 5, "brightness": 6,
        "translateX": 7, "translateY": 8, "invert": 9}
SIGNED = ("color", "contrast", "brightness", "translateX", "translateY")  # the reference draws random.choice([-1, 1])


def blend_value(d, i, a, mode="f32"):
    """``d + a * (i - d)`` before it becomes a byte, as float64 holding the value the mode computes: 'f32' (Pillow:
    product and sum each rounded to float32), 'f64' (the blend in double), 'fma' (exact product and sum, one rounding to
    float32).  ``d``, ``i``: integer arrays (degenerate, image)."""
    d, i = np.broadcast_arrays(np.asarray(d, np.int64), np.asarray(i, np.int64))
    a32 = np.float32(a)
    if mode == "f32":
        prod = (a32 * (i - d).astype(np.float32)).astype(np.float32)
        return (d.astype(np.float32) + prod).astype(np.float32).astype(np.float64)
    if mode == "f64":
        return d.astype(np.float64) + float(a) * (i - d).astype(np.float64)
    if mode == "fma":  # a float32 times a 9-bit integer plus an 8-bit integer is exact in double: one rounding follows
        return (d.astype(np.float64) + float(a32) * (i - d).astype(np.float64)).astype(np.float32).astype(np.float64)
    raise ValueError(mode)


def blend(d, i, a, mode="f32", rounding="trunc"):
    """The byte: <= 0 -> 0, >= 255 -> 255, else truncated (Pillow) or, rounding='round', rounded (a negative control)."""
    t = blend_value(d, i, a, mode)
    core = np.floor(t + 0.5) if rounding == "round" else np.trunc(t)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, core)).astype(np.uint8)


def luma(img, mode="int"):
    """Pillow's RGB -> L: (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16.  mode 'float': the ITU-R 601 weights in
    floating point, rounded (a negative control)."""
    v = img.astype(np.int64)
    if mode == "float":
        return np.floor(v[..., 0] * 0.299 + v[..., 1] * 0.587 + v[..., 2] * 0.114 + 0.5).astype(np.int64)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def contrast_mean(img, half=True):
    """ImageEnhance.Contrast's degenerate value: int(ImageStat.Stat(image.convert('L')).mean[0] + 0.5), in double."""
    l = luma(img)
    return int(float(int(l.sum())) / float(l.size) + (0.5 if half else 0.0))


def contrast_mean_integer(total, count):
    """The integer form the kernel uses: (2 * sum + count) // (2 * count)."""
    return (2 * int(total) + int(count)) // (2 * int(count))


def brightness(img, a, **kw):
    return blend(0, img, a, **kw)


def color(img, a, luma_mode="int", **kw):
    return blend(luma(img, luma_mode)[..., None], img, a, **kw)


def contrast(img, a, half=True, **kw):
    return blend(contrast_mean(img, half), img, a, **kw)


def solarize(img, thr):
    return np.where(img.astype(np.float64) < float(thr), img, 255 - img).astype(np.uint8)


def posterize(img, bits):
    return (img & np.uint8((0xFF << (8 - int(bits))) & 0xFF)).astype(np.uint8)


def invert(img):
    return (255 - img).astype(np.uint8)


def equalize(img):
    """The reference's ``equalize`` returns its input."""
    return img.copy()


def autocontrast(img):
    out = np.empty_like(img)
    for c in range(3):
        ch = img[..., c]
        lo, hi = int(ch.min()), int(ch.max())
        if hi <= lo:
            out[..., c] = ch
            continue
        scale = 255.0 / (hi - lo)
        offset = -lo * scale
        lut = np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)], np.uint8)
        out[..., c] = lut[ch]
    return out


def shift_of(magnitude, extent, sign):
    """The integer shift of translateX / translateY: floor(d + 0.5), d = magnitude * extent * sign in double."""
    return int(math.floor(float(magnitude) * extent * sign + 0.5))


def translate(img, sx, sy, fill=0):
    """out[y][x] = in[y + sy][x + sx] where that lies inside the image, else ``fill`` (Pillow: black)."""
    h, w = img.shape[:2]
    out = np.full_like(img, fill)
    ys, xs = np.arange(h) + int(sy), np.arange(w) + int(sx)
    yok, xok = (ys >= 0) & (ys < h), (xs >= 0) & (xs < w)
    out[np.ix_(yok, xok)] = img[np.ix_(ys[yok], xs[xok])]
    return out


def translateX(img, sx, **kw):
    return translate(img, sx, 0, **kw)


def translateY(img, sy, **kw):
    return translate(img, 0, sy, **kw)


def apply(img, code, par):
    """One step as the kernel sees it: an operation code and its float32 parameter."""
    code, par = int(code), np.float32(par)
    if code == 1:
        return autocontrast(img)
    if code == 2:
        return solarize(img, par)
    if code == 3:
        return color(img, par)
    if code == 4:
        return posterize(img, int(par))
    if code == 5:
        return contrast(img, par)
    if code == 6:
        return brightness(img, par)
    if code == 7:
        return translateX(img, int(par))
    if code == 8:
        return translateY(img, int(par))
    if code == 9:
        return invert(img)
    return img.copy()


def chain(img, ops, pars):
    for code, par in zip(ops, pars):
        img = apply(img, code, par)
    return img


def parameter(name, value, sign, h, w):
    """The float32 ``par`` of one step from the reference's table value and the drawn sign (formed in double)."""
    if name in ("color", "contrast", "brightness"):
        return np.float32(1 + float(value) * sign)
    if name == "translateX":
        return np.float32(shift_of(value, w, sign))
    if name == "translateY":
        return np.float32(shift_of(value, h, sign))
    if name in ("solarize", "posterize"):
        return np.float32(value)
    return np.float32(0.0)
