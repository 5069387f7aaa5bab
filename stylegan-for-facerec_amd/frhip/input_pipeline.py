"""GPU-side training-input pipeline.

The reference transforms every sample on a host worker (dataset.py:85-88 applying the Compose of train.py:108-116):
PIL resize to 128x128, random 112x112 crop, random flip, ToTensor, Normalize -> a float32 [3,112,112] tensor per image
(150 KB) that is collated and copied to the GPU.  At >= 14 k images/s per GPU that host work cannot feed eight GPUs.
Here the workers only DECODE: a sample is the uint8 HWC image as stored (37 KB at 112x112, a quarter of the bytes over
PCIe), the batch is staged as uint8 [B,H,W,3], and ONE HIP launch (``fr_augment_u8``) produces the float32 NCHW batch:
Pillow's 8-bit bilinear resample restated bit-exactly, evaluated only inside each image's crop window, flip, and the
ToTensor/Normalize arithmetic as a 256-entry table per channel.  Crop offsets and flips are drawn on the host (the
reference's random stream -- torchvision's use of the global torch RNG -- is not reproduced; the draws are uniform
over the same ranges).

Scope of the bit-exactness claim: Pillow resamples horizontally, then vertically -- except for extreme aspect ratios
(observed with the installed Pillow 12.2 only beyond ~100:1, e.g. 500x3 -> 128x128, where it runs the vertical pass first
and the uint8 rounding of the intermediate image differs).  Staged images whose aspect ratio exceeds ``MAX_ASPECT`` = 16
are refused instead of being transformed with unverified rounding; aligned face crops are square.

``resize_tables`` is Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for the bilinear filter
(``src/libImaging/Resample.c``); tests pin it against the installed Pillow through ``oracle/input_ref.py``.
"""
import math

import numpy as np
import torch

from . import ops

PRECISION_BITS = 32 - 8 - 2
MAX_ASPECT = 16  # largest staged-image aspect ratio the transform accepts (see the module docstring)


def _axis_table(in_size, out_size):
    """int32 [out_size, ksize + 2]: (first input index, tap count, integer weights) per output index."""
    scale = filterscale = float(in_size) / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = filterscale  # bilinear: support 1.0, stretched when shrinking
    ksize = int(math.ceil(support)) * 2 + 1
    tab = np.zeros((out_size, ksize + 2), np.int32)
    inv = 1.0 / filterscale
    one = float(1 << PRECISION_BITS)
    for o in range(out_size):
        center = (o + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        hi = min(int(center + support + 0.5), in_size)
        weights = []
        total = 0.0
        for i in range(lo, hi):
            d = abs((i - center + 0.5) * inv)
            w = 1.0 - d if d < 1.0 else 0.0
            weights.append(w)
            total += w
        tab[o, 0], tab[o, 1] = lo, hi - lo
        for j, w in enumerate(weights):
            if total != 0.0:
                w = w / total
            tab[o, 2 + j] = int(w * one - 0.5) if w < 0 else int(w * one + 0.5)
    return tab


def resize_tables(in_h, in_w, out_h, out_w):
    """(xtab [out_w, kx+2], ytab [out_h, ky+2]) for ``Image.resize((out_w, out_h), BILINEAR)`` of an in_h x in_w image.
    An axis whose size does not change gets the identity table (one tap of weight 2**22), which is what skipping that
    pass amounts to."""
    return _axis_table(in_w, out_w), _axis_table(in_h, out_h)


def normalize_lut(mean, std):
    """float32 [256, 3]: uint8 value -> ((v / 255) - mean) / std, rounded to float32 after every step (ToTensor,
    Normalize)."""
    v = np.arange(256, dtype=np.float32)[:, None] / np.float32(255.0)
    return ((v - np.asarray(mean, np.float32)[None, :]) / np.asarray(std, np.float32)[None, :]).astype(np.float32)


# ---- RandAugment (data_processing/randaugment.py) on the device: the operations fr_randaug_u8 serves, their codes, and
# the ten-point magnitude tables of the reference class (tests pin them against Rand_Augment().ranges)
SERVED = ("autocontrast", "equalize", "solarize", "color", "posterize", "contrast", "brightness", "translateX",
          "translateY", "invert")
UNSERVED = {
    "rotate": "it goes through an RGBA composite of a resampled image",
    "shearX": "it needs Pillow's bicubic affine resample",
    "shearY": "it needs Pillow's bicubic affine resample",
    "sharpness": "it needs a 3x3 smoothing filter",
}
RANDAUG_CODE = {"equalize": 0, "autocontrast": 1, "solarize": 2, "color": 3, "posterize": 4, "contrast": 5,
                "brightness": 6, "translateX": 7, "translateY": 8, "invert": 9}  # equalize: the reference's is the identity
RANDAUG_RANGES = {
    "translateX": np.linspace(0, 0.2, 10), "translateY": np.linspace(0, 0.2, 10), "color": np.linspace(0.0, 0.9, 10),
    "posterize": np.round(np.linspace(8, 4, 10), 0), "solarize": np.linspace(256, 231, 10),
    "contrast": np.linspace(0.0, 0.5, 10), "brightness": np.linspace(0.0, 0.3, 10), "autocontrast": np.zeros(10),
    "equalize": np.zeros(10), "invert": np.zeros(10)}
RANDAUG_MAX_STEPS = 16  # K of fr_randaug_u8
RANDAUG_LDS_BUDGET = 64 * 1024  # H * W * 3 bytes + 3 * 256 table words


def check_randaug_ops(ops, who="GpuRandAugment"):
    """The tuple of served names for ``ops`` (None: the served set); an unserved or unknown name is refused by name.
    ``who``: what the message blames (the class, or train.py's config key)."""
    ops = SERVED if ops is None else tuple(ops)
    if not ops:
        raise ValueError("%s: no operation given" % who)
    for name in ops:
        if name in UNSERVED:
            raise NotImplementedError("%s: '%s' is not served on the device: %s; the device path serves %s "
                                      "(the host class data_processing.randaugment.Rand_Augment runs all 13)"
                                      % (who, name, UNSERVED[name], ", ".join(SERVED)))
        if name not in RANDAUG_CODE:
            raise ValueError("%s: unknown operation %r; the device path serves %s" % (who, name, ", ".join(SERVED)))
    return ops


class GpuRandAugment(object):
    """The reference's ``Rand_Augment`` policy on a staged uint8 batch: ``num`` operations per image, drawn uniformly with
    replacement from ``ops``, each at a magnitude index uniform in ``[0, max_magnitude)`` and with a sign where the
    reference's operation draws one.  The reference's ``np.random`` / ``random`` streams are not reproduced.

        ra = GpuRandAugment()
        op, par = ra.draw(B, generator, (H, W))
        out = ra(u8, op, par)                                # uint8 [B,H,W,3] -> uint8 [B,H,W,3], one launch
    """

    def __init__(self, num=None, max_magnitude=10, ops=SERVED):
        self.ops = check_randaug_ops(ops)
        self.num = len(self.ops) // 2 if num is None else int(num)  # the reference's rule, on the given list
        self.max_magnitude = int(max_magnitude)
        if not 1 <= self.num <= RANDAUG_MAX_STEPS:
            raise ValueError("GpuRandAugment: num must lie in 1..%d, got %r" % (RANDAUG_MAX_STEPS, num))
        if not 1 <= self.max_magnitude <= 10:
            raise ValueError("GpuRandAugment: max_magnitude must lie in 1..10 (the tables hold ten points), got %r"
                             % (max_magnitude,))
        self._codes = np.array([RANDAUG_CODE[n] for n in self.ops], np.uint8)
        self._values = np.stack([np.asarray(RANDAUG_RANGES[n], np.float64) for n in self.ops])  # [ops, 10]

    @staticmethod
    def parameters(codes, values, signs, h, w):
        """float32 ``par`` from operation codes, table values and signs (arrays of one shape), formed in double: the
        factor 1 + value * sign of color / contrast / brightness, the shift floor(value * extent * sign + 0.5) of a
        translation, the table value itself for solarize / posterize, 0 elsewhere."""
        codes, values, signs = np.asarray(codes), np.asarray(values, np.float64), np.asarray(signs, np.float64)
        par = np.zeros(codes.shape, np.float64)
        blend = (codes == 3) | (codes == 5) | (codes == 6)
        par[blend] = 1 + values[blend] * signs[blend]
        plain = (codes == 2) | (codes == 4)
        par[plain] = values[plain]
        for code, extent in ((7, w), (8, h)):
            m = codes == code
            par[m] = np.floor(values[m] * extent * signs[m] + 0.5)
        return par.astype(np.float32)

    def draw(self, batch, generator, size):
        """(op uint8 [B,K], par float32 [B,K]) on the host for images of ``size`` = (H, W), which is required because the
        shift of a translation is a fraction of H or W (``generator`` may be None: the global one): three draws of [B,K] from
        ``generator`` -- names, magnitude indices, signs (drawn for every step, used where the operation has one)."""
        shape = (batch, self.num)
        which = torch.randint(0, len(self.ops), shape, generator=generator).numpy()
        index = torch.randint(0, self.max_magnitude, shape, generator=generator).numpy()
        sign = torch.randint(0, 2, shape, generator=generator).numpy() * 2 - 1
        codes = self._codes[which]
        par = self.parameters(codes, self._values[which, index], sign, int(size[0]), int(size[1]))
        return torch.from_numpy(codes), torch.from_numpy(par)

    @staticmethod
    def check_size(h, w):
        if h * w * 3 + 3 * 256 * 4 > RANDAUG_LDS_BUDGET:
            raise ValueError("GpuRandAugment: %dx%d images exceed the kernel's LDS budget (H * W * 3 + 3072 <= %d bytes; "
                             "128x128 fits)" % (h, w, RANDAUG_LDS_BUDGET))

    def launch(self, src, op, par, b, h, w, idx=None, labels=None, label_out=None):
        """``fr_randaug_u8`` on ``src`` (the batch, or with ``idx`` int32 [b] a store the batch is gathered from): the
        uint8 [b,h,w,3] result.  ``op`` / ``par`` as ``draw`` returns them (host or device)."""
        self.check_size(h, w)
        dev = src.device
        _to_device = GpuTrainTransform._to_device  # the pinned, asynchronous copy of the crop / flip draws
        op, par = _to_device(op, torch.uint8, dev), _to_device(par, torch.float32, dev)
        if tuple(op.shape) != tuple(par.shape) or op.dim() != 2 or op.shape[0] != b:
            raise ValueError("GpuRandAugment: op / par must both be [B, K] with B = %d, got %s and %s"
                             % (b, tuple(op.shape), tuple(par.shape)))
        out = torch.empty(b, h, w, 3, device=dev, dtype=torch.uint8)
        ops.call("fr_randaug_u8", src, labels, idx, op, par, out, label_out, int(src.shape[0]), b, int(op.shape[1]), h, w,
                 ops.current_stream_ptr())()
        return out

    def __call__(self, u8, op=None, par=None, idx=None, labels=None, label_out=None, generator=None):
        if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
            raise ValueError("GpuRandAugment: expected uint8 [B, H, W, 3], got %s %s" % (u8.dtype, tuple(u8.shape)))
        h, w = int(u8.shape[1]), int(u8.shape[2])
        b = int(u8.shape[0]) if idx is None else int(idx.shape[0])
        if op is None or par is None:
            op, par = self.draw(b, generator, (h, w))
        if idx is not None:
            idx = GpuTrainTransform._to_device(idx, torch.int32, u8.device)
        return self.launch(u8.contiguous(), op, par, b, h, w, idx, labels, label_out)


class GpuTrainTransform(object):
    """Batch form of the reference's train transform on staged uint8 images.

        tf = GpuTrainTransform(112, RGB_MEAN, RGB_STD)
        x = tf(u8_batch.to(device, non_blocking=True))        # uint8 [B,H,W,3] -> float32 [B,3,112,112]

    ``generator``: a ``torch.Generator`` (CPU) for the crop / flip draws; default is the global RNG.
    ``randaug``: a ``GpuRandAugment`` applied to the decoded images before the resize (one more launch), or None; its
    draws follow the batch's crop / flip draws on the same generator.
    """

    def __init__(self, size=112, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5), flip_p=0.5, randaug=None):
        self.size, self.big = int(size), int(128 * size / 112)  # train.py:109
        self.flip_p = float(flip_p)
        self.randaug = randaug
        self.lut_host = torch.from_numpy(normalize_lut(mean, std))
        self._tables = {}  # (device, H, W) -> (xtab, ytab, lut, kx, ky)

    def tables(self, device, h, w):
        key = (str(device), h, w)
        if key not in self._tables:
            xt, yt = resize_tables(h, w, self.big, self.big)
            self._tables[key] = (torch.from_numpy(xt).to(device), torch.from_numpy(yt).to(device),
                                 self.lut_host.to(device), xt.shape[1] - 2, yt.shape[1] - 2)
        return self._tables[key]

    def draw(self, batch, generator=None):
        """(crop int32 [B,2] = (x0, y0), flip uint8 [B]) on the host."""
        span = self.big - self.size + 1
        crop = torch.randint(0, span, (batch, 2), generator=generator, dtype=torch.int32)
        flip = (torch.rand(batch, generator=generator) < self.flip_p).to(torch.uint8)
        return crop, flip

    @staticmethod
    def _to_device(t, dtype, dev):
        """Host draws go through pinned memory with an asynchronous copy: a pageable host-to-device copy would make the
        host wait for everything already queued on the stream, i.e. for the previous training step."""
        t = t.to(dtype).contiguous()
        if t.is_cuda:
            return t
        return t.pin_memory().to(dev, non_blocking=True)

    def __call__(self, u8, crop=None, flip=None, generator=None, validate=True, op=None, par=None):
        """``validate=False``: the caller guarantees 0 <= crop <= big - size (skips the host-side range check, which is a
        device synchronisation when ``crop`` already lives on the device).  ``op`` / ``par``: the RandAugment chain per
        image when ``randaug`` is set (default: drawn from ``generator`` after the crop / flip draws)."""
        if u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3:
            raise ValueError("GpuTrainTransform: expected uint8 [B, H, W, 3], got %s %s" % (u8.dtype, tuple(u8.shape)))
        b, h, w, _ = u8.shape
        if b and (h > MAX_ASPECT * w or w > MAX_ASPECT * h):
            raise ValueError("GpuTrainTransform: %dx%d images exceed the supported aspect ratio of %d:1" % (h, w, MAX_ASPECT))
        if crop is None or flip is None:
            crop, flip = self.draw(b, generator)
        if self.randaug is not None and b:  # on the decoded image, before the resize; fr_augment_u8 below is unchanged
            if op is None or par is None:
                op, par = self.randaug.draw(b, generator, (h, w))
            u8 = self.randaug.launch(u8.contiguous(), op, par, b, h, w)
        span = self.big - self.size
        if b and validate and (int(crop.min()) < 0 or int(crop.max()) > span):
            raise ValueError("GpuTrainTransform: crop offsets must lie in [0, %d]" % span)
        dev = u8.device
        xtab, ytab, lut, kx, ky = self.tables(dev, h, w)
        crop, flip = self._to_device(crop, torch.int32, dev), self._to_device(flip, torch.uint8, dev)
        out = torch.empty(b, 3, self.size, self.size, device=dev, dtype=torch.float32)
        ops.call("fr_augment_u8", u8.contiguous(), xtab, ytab, crop, flip, lut, out, b, h, w, self.big, self.big,
                 self.size, kx, ky, ops.current_stream_ptr())()
        return out
