"""RandAugment on the host, under the reference's import path (``data_processing.randaugment.Rand_Augment``).

The class keeps the reference's public surface -- the 13 names of ``transforms`` in its order, ``Numbers``,
``max_Magnitude``, the ten-point ``ranges`` tables, ``func``, ``rand_augment()``, ``__call__`` on an array and
``test_single_operation`` -- and runs every operation through Pillow, on current numpy (the reference's table uses
``np.int``, which numpy 2 no longer has).  Two things the reference's code does and this one keeps, because they decide
the pixels: ``equalize`` returns its input, and the ``fill=128`` handed to ``Image.transform`` is not Pillow's
``fillcolor``, so what a shear or a translation brings in from outside the image is black.

The device path (``frhip.input_pipeline.GpuRandAugment``, kernel ``fr_randaug_u8``) serves ``frhip.input_pipeline.SERVED``;
the four names of ``frhip.input_pipeline.UNSERVED`` run here only."""
import random

import numpy as np
from PIL import Image, ImageEnhance, ImageOps

TRANSFORMS = ("autocontrast", "equalize", "rotate", "solarize", "color", "posterize", "contrast", "brightness",
              "sharpness", "shearX", "shearY", "translateX", "translateY")

def _sign():
    return random.choice([-1, 1])


def _affine(img, coeffs, resample=Image.NEAREST):
    # no fillcolor: pixels from outside the image are black, as in the reference (whose fill=128 Pillow does not read)
    return img.transform(img.size, Image.AFFINE, coeffs, resample)


def _rotate_with_fill(img, degrees):
    turned = img.convert("RGBA").rotate(degrees)
    grey = Image.new("RGBA", turned.size, (128,) * 4)
    return Image.composite(turned, grey, turned).convert(img.mode)


def make_ranges():
    """The ten magnitudes of every operation, index 0 the mildest."""
    return {
        "shearX": np.linspace(0, 0.3, 10),
        "shearY": np.linspace(0, 0.3, 10),
        "translateX": np.linspace(0, 0.2, 10),
        "translateY": np.linspace(0, 0.2, 10),
        "rotate": np.linspace(0, 360, 10),
        "color": np.linspace(0.0, 0.9, 10),
        "posterize": np.round(np.linspace(8, 4, 10), 0).astype(int),
        "solarize": np.linspace(256, 231, 10),
        "contrast": np.linspace(0.0, 0.5, 10),
        "sharpness": np.linspace(0.0, 0.9, 10),
        "brightness": np.linspace(0.0, 0.3, 10),
        "autocontrast": [0] * 10,
        "equalize": [0] * 10,
        "invert": [0] * 10,
    }


def make_func():
    """name -> f(PIL image, magnitude) -> PIL image; a sign is drawn from ``random`` where the operation has one."""
    return {
        "shearX": lambda img, m: _affine(img, (1, m * _sign(), 0, 0, 1, 0), Image.BICUBIC),
        "shearY": lambda img, m: _affine(img, (1, 0, 0, m * _sign(), 1, 0), Image.BICUBIC),
        "translateX": lambda img, m: _affine(img, (1, 0, m * img.size[0] * _sign(), 0, 1, 0)),
        "translateY": lambda img, m: _affine(img, (1, 0, 0, 0, 1, m * img.size[1] * _sign())),
        "rotate": _rotate_with_fill,
        "color": lambda img, m: ImageEnhance.Color(img).enhance(1 + m * _sign()),
        "posterize": lambda img, m: ImageOps.posterize(img, int(m)),
        "solarize": lambda img, m: ImageOps.solarize(img, m),
        "contrast": lambda img, m: ImageEnhance.Contrast(img).enhance(1 + m * _sign()),
        "sharpness": lambda img, m: ImageEnhance.Sharpness(img).enhance(1 + m * _sign()),
        "brightness": lambda img, m: ImageEnhance.Brightness(img).enhance(1 + m * _sign()),
        "autocontrast": lambda img, m: ImageOps.autocontrast(img),
        "equalize": lambda img, m: img,
        "invert": lambda img, m: ImageOps.invert(img),
    }


class Rand_Augment(object):
    """``Numbers`` operations drawn with replacement from ``transforms``, each at a magnitude index drawn from
    ``[0, max_Magnitude)``, applied in order to a uint8 [H, W, 3] array."""

    def __init__(self, Numbers=None, max_Magnitude=None):
        self.transforms = list(TRANSFORMS)
        self.Numbers = len(self.transforms) // 2 if Numbers is None else Numbers
        self.max_Magnitude = 10 if max_Magnitude is None else max_Magnitude
        self.ranges = make_ranges()
        self.func = make_func()

    def rand_augment(self):
        """[(name, magnitude index)] * Numbers, from numpy's global generator (indices first, then names)."""
        magnitudes = np.random.randint(0, self.max_Magnitude, self.Numbers)
        names = np.random.choice(self.transforms, self.Numbers)
        return list(zip(names, magnitudes))

    def _apply(self, image, op_name, M):
        return self.func[op_name](image, self.ranges[op_name][M])

    def __call__(self, image):
        image = Image.fromarray(image)
        for op_name, M in self.rand_augment():
            image = self._apply(image, op_name, M)
        return np.asarray(image)

    def test_single_operation(self, image, op_name, M=-1):
        """One operation at magnitude index ``M`` (-1: the strongest) on an array (or a PIL image)."""
        if not isinstance(image, Image.Image):
            image = Image.fromarray(image)
        return np.asarray(self._apply(image, op_name, M))
