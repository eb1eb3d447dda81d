"""The mlx.data operator surface for the image path, over the gfx950 kernels.

Same names, keyword arguments and error behaviour as mlx-data 0.2.0
(``python/src/wrap_dataset.h``, ``wrap_buffer.cpp``, ``wrap_stream.cpp``):

    dset = (buffer_from_vector(samples)
            .shuffle().to_stream()
            .load_image("image")
            .image_resize_smallest_side("image", 256)
            .image_center_crop("image", 224, 224)
            .batch(32)
            .key_transform("image", lambda x: x.astype("float32") / 255)
            .prefetch(8, 8))

The image ops only record geometry; ``batch`` runs the resize, crop and
mirror of the whole batch as one fused GPU launch and writes the stacked
(B, H, W, C) uint8 tensor.  ``image_to_float(key)`` before ``batch`` (this
build's one addition to the surface) replaces the trailing
``key_transform(..., lambda x: x.astype("float32") / 255)``: the same launch
then writes the float32 batch, bit-identical to that lambda.  With several
devices (``set_devices``) a batch of at least 64 images per device is split
into contiguous slices, one per device; smaller batches go whole to one
device, consecutive batches rotating over the devices.  ``batch(n, device=d)`` builds the image keys' batches in device
memory instead (``DeviceArray``: DLPack producer, ``numpy()`` copies back);
import torch before this package when torch consumes them, so both share one
HIP runtime.  Reading an unbatched image materialises it with its own launch.
There is no CPU resize: without a visible GPU the image ops raise.

``image_normalize(key, mean=None, std=None, dtype="float32", layout="hwc",
output_key="")`` (with ``image_normalize_if``; the second addition to the
surface) ends the chain in the form a training step consumes:
``((x.astype("float32") / 255) - mean) / std`` in float32 operations, cast to
``float32``, ``float16`` or ``bfloat16`` (round to nearest even), as
``(B, H, W, C)`` (``hwc``) or ``(B, C, H, W)`` (``chw``).  ``mean`` / ``std``
are ``None`` (``x / 255`` only), a number, or one value per channel, in [0, 1]
units like ``torchvision.transforms.Normalize`` after ``ToTensor``.  Like
``image_to_float`` it only marks the pending image, so ``batch(n, device=d)``
writes the final tensor from the resize launch itself -- no second pass over
the batch -- and ``DeviceArray`` exports it through DLPack (float16 as
``kDLFloat``/16, bfloat16 as ``kDLBfloat``/16).  No image op may follow it; a
batch takes one format and one channel count per key; ragged batches pad with
zeros (or ``pad``); videos ``(F, H, W, C)`` take ``hwc`` only.

First version of the host side: a host batch (``batch(n)`` without
``device=``) and a direct read of an unbatched normalised image are produced
by the same device calls into a block of the device batch pool and copied back
with one device-to-host copy, without the chunk overlap the uint8 and
``image_to_float`` host batches have.  float32 and float16 come back as NumPy
arrays; bfloat16 has no NumPy type, so a host batch of it (and
``DeviceArray.numpy()``) raises ``RuntimeError``: use ``device=`` and
``torch.from_dlpack``.

``image_resize(key, w, h, output_key="", *, filter="triangle")`` and
``image_resize_smallest_side(key, size, output_key="", *, filter="triangle")``
(and their ``_if`` forms) take the resampling filter of the resize:
``"triangle"`` (mlx-data's, the default), ``"catmullrom"`` (PIL ``BICUBIC``,
torch ``bicubic`` with ``antialias=True``), ``"mitchell"`` or
``"cubicbspline"``.  An unknown name raises ``ValueError`` when the op is made.
A pending image carries the filter of its one resize (a second resize
materialises the first); a resize to the size the image already has is the
identity for every filter.

Photometric augmentation stays in the launch too (the third addition):
``image_color_twist(key, brightness=1.0, contrast=1.0, saturation=1.0,
hue=0.0, output_key="")``, ``image_color_matrix(key, matrix, output_key="")``
(a 3x3 or 3x4 matrix for ``[r g b 1]`` in [0, 1] units) and
``image_random_color_twist(key, brightness=None, contrast=None,
saturation=None, hue=None, output_key="")`` (each ``None`` or a ``(lo, hi)``
range, drawn per image -- once per video -- from the ``set_state`` generator
in that order), with their ``_if`` forms.  The map is a per-pixel 3x4 affine
on the uint8 result, rounded and clamped back to uint8: brightness scales,
contrast scales about 0.5 (the fixed-centre form, not torchvision's blend with
the image mean), saturation blends with the luma, hue (degrees) rotates the
YIQ chroma; hue is applied first and brightness last.  RGB images only.  The
op only marks the pending image: crops and flips still compose after it,
``image_to_float`` / ``image_normalize`` stack on top, and ``batch`` runs the
map as one more kernel behind the resize of the same call.  A resize or a
second colour op after it materialises the first.  Bad arguments raise
``ValueError`` when the op is made.

The tone operations that depend on the image's own content stay in the launch
as well (the fourth addition): ``image_posterize(key, bits, output_key="")``,
``image_solarize(key, threshold=128, output_key="")``,
``image_autocontrast(key, output_key="")``, ``image_equalize(key,
output_key="")`` and ``image_contrast(key, factor, output_key="")``, with
their ``_if`` forms.  They are Pillow's ``ImageOps.posterize`` / ``solarize``
/ ``autocontrast`` / ``equalize`` and ``ImageEnhance.Contrast`` on the uint8
result, bit for bit (``image_contrast`` blends with the grey of the image's
mean luma; ``image_color_twist``'s contrast keeps its fixed centre).  RGB
images only.  The op only marks the pending image and ``batch`` runs a
per-image histogram, a table builder and a lookup behind the resize of the
same call.  The stage order in a launch is tone, colour, output form: a
colour op, ``image_to_float``, ``image_normalize`` and flips compose after a
tone op; crops compose after posterize and solarize and materialise the other
three first (their statistics are those of the uncropped result); a resize, a
second tone op, or a tone op after a colour op materialises what is pending.
A video's frames each use their own statistics.  Bad arguments raise
``ValueError`` when the op is made.

The affine warps of the augmentation policies stay in the launch too (the
fifth addition): ``image_affine(key, matrix)`` (six numbers, Pillow's AFFINE
data: output pixel -> source position), ``image_shear(key, x=0.0, y=0.0)``,
``image_translate(key, x=0.0, y=0.0)`` (pixels; the content moves by -t, as in
timm) and ``image_affine_rotate(key, angle)`` (degrees, Pillow's sign, about
the centre, same size), each with ``resample="nearest" | "bilinear"``,
``fill=0`` (a scalar or ``(r, g, b)`` in 0..255) and ``output_key=""``, and
the random forms ``image_random_shear(key, x=None, y=None)``,
``image_random_translate(key, x=None, y=None)`` and
``image_random_affine_rotate(key, angle)`` with ``(lo, hi)`` pairs (one
uniform draw per given range, x then y; a video draws once), all with ``_if``
forms.  They are Pillow's ``Image.transform(size, AFFINE, ..., fillcolor=)``
and ``Image.rotate(angle, resample, fillcolor=)`` on the uint8 result, bit for
bit; ``image_rotate`` stays the reference's op.  RGB images only.  The op only
marks the pending image and ``batch`` warps behind the resize of the same
call.  The stage order in a launch is geometry, warp, tone, colour, output
form: crops and flips before the warp are part of what it marks, tone and
colour ops, ``image_to_float`` and ``image_normalize`` compose after it, and a
crop, flip, resize or ``image_rotate`` after a warp, or a warp after a warp,
tone or colour op, materialises what is pending.  Bad arguments raise
``ValueError`` when the op is made.

The enhance ops complete the op set of the PIL augmentation policies (the
sixth addition): ``image_sharpness(key, factor)``, ``image_color(key, factor)``
and ``image_brightness(key, factor)`` are Pillow's ``ImageEnhance.Sharpness``,
``.Color`` and ``.Brightness`` (``Image.blend(degenerate, image, factor)`` with
the 3 x 3 ``SMOOTH`` filter, the luma grey and black as the degenerate image)
on the uint8 result, bit for bit; ``ImageEnhance.Contrast`` is
``image_contrast``.  The random forms ``image_random_sharpness(key,
factor=(lo, hi))``, ``image_random_color`` and ``image_random_brightness``
draw one uniform factor per image (a video draws once); all take
``output_key=""`` and have ``_if`` forms.  Factors are finite and in 0..1e6.
RGB images only.  The op only marks the pending image and ``batch`` runs it
in the same call, behind the warp and before the tone op: the stage order is
geometry, warp, enhance, tone, colour, output form.  Tone and colour ops,
``image_to_float`` and ``image_normalize`` compose after an enhance op,
``image_random_h_flip`` composes after all three and a crop after
``image_color`` / ``image_brightness``; a crop after ``image_sharpness`` (the
copied outer ring is the uncropped window's), a resize, ``image_rotate``, a
warp or a second enhance op, or an enhance op after a tone or colour op,
materialises what is pending.  Bad arguments raise ``ValueError`` when the op
is made.

``load_image`` decodes JPEG natively (``csrc/jpeg.cpp``, the reference's
libjpeg path, ``core/image/ImageJPEG.cpp``).  With a device visible it only
parses the markers of a sequential file and the batch launch runs the whole
decode on the GPU -- Huffman (``csrc/jpeghuff.hip``), IDCT, upsampling,
colour (``csrc/jpegdev.hip``) -- before resizing, with the same bytes;
progressive and other files are entropy-decoded on the host first.
``set_device_entropy(False)`` keeps the Huffman decode on the host for every
file, ``set_device_decode(False)`` decodes whole on the host.

``batch_mix(batch_size, key, mixup_alpha=0.0, cutmix_alpha=0.0, prob=1.0,
switch_prob=0.5, mode="batch", lam_key="mix_lam", partner_key="mix_partner",
...)`` batches like ``batch`` and runs MixUp / CutMix (timm's
``FastCollateMixup``) across the images of ``key`` inside the same launch:
image ``i`` is mixed with image ``n - 1 - i``, ``lam`` and the boxes are drawn
per batch, pair or element from the thread's state, and the batch gains the
weight of each sample's own label and its partner's index.  The images must
be pending RGB images of one crop size; ``image_to_float`` /
``image_normalize`` compose.
Other formats go to a Pillow hook that follows the reference's stb_image
rules (``core/image/ImageSTBI.cpp``: 1/2/3 channels kept, 4 -> 3, 16-bit >> 8).
"""
import io

import numpy as np

from . import capi  # noqa: F401  (loads libmxd_amd.so before anything else binds a HIP runtime)
from . import _pipeline  # noqa: F401
from ._pipeline import (Buffer, DeviceArray, Stream, buffer_from_vector, device_decode, device_entropy, devices,
                        set_device_decode, set_device_entropy, set_devices, set_image_decoder, set_state)

__all__ = ["Buffer", "Stream", "DeviceArray", "buffer_from_vector", "set_state", "set_devices", "devices",
           "set_device_decode", "device_decode", "set_device_entropy", "device_entropy"]


def _decode(path, data, from_memory, info):
    """Non-JPEG images (the reference's stb_image fallback, core/image/ImageSTBI.cpp:14-58):
    channels = min(stbi channels, 3) -- grey 1, grey+alpha 2, RGB 3, RGBA -> RGB;
    16-bit samples are scaled to 8 bits with >> 8 (stbi__convert_16_to_8); 1-bit
    images are expanded to 0/255 grey."""
    from PIL import Image

    try:
        im = Image.open(io.BytesIO(data.tobytes()) if from_memory else path)
        if info:
            return np.array([im.width, im.height], dtype=np.int64)
        if im.mode in ("L", "RGB", "LA"):
            a = np.asarray(im)
        elif im.mode in ("I;16", "I;16B", "I;16L", "I"):
            a = (np.asarray(im).astype(np.int64) >> 8).clip(0, 255).astype(np.uint8)
        elif im.mode == "1":
            a = np.asarray(im.convert("L"))
        else:  # palette, RGBA, CMYK, ...
            a = np.asarray(im.convert("RGB"))
    except (OSError, ValueError, SyntaxError):
        return None
    if a.ndim == 2:
        a = a[:, :, None]
    return np.ascontiguousarray(a, dtype=np.uint8)


set_image_decoder(_decode)


def _add_if_variants(cls):
    """``<op>_if(cond, ...)``: the op when ``cond`` holds, else the dataset
    unchanged (``Dataset::*_if``, ``Dataset.cpp``)."""
    for name in ("key_transform", "load_image", "image_resize_smallest_side", "image_resize",
                 "image_center_crop", "image_random_crop", "image_random_h_flip", "image_random_area_crop",
                 "image_rotate", "image_channel_reduction", "image_to_float", "image_normalize",
                 "image_color_twist", "image_color_matrix", "image_random_color_twist",
                 "image_posterize", "image_solarize", "image_autocontrast", "image_equalize", "image_contrast",
                 "image_affine", "image_shear", "image_translate", "image_affine_rotate", "image_random_shear",
                 "image_random_translate", "image_random_affine_rotate",
                 "image_sharpness", "image_color", "image_brightness", "image_random_sharpness",
                 "image_random_color", "image_random_brightness"):
        def op_if(self, cond, *args, _name=name, **kwargs):
            return getattr(self, _name)(*args, **kwargs) if cond else self

        op_if.__name__ = name + "_if"
        setattr(cls, name + "_if", op_if)


def _stream_iter(self):
    return self


def _stream_next(self):
    s = self.next()
    if not s:
        raise StopIteration
    return s


def _buffer_iter(self):
    for i in range(len(self)):
        yield self[i]


_add_if_variants(Buffer)
_add_if_variants(Stream)
Stream.__iter__ = _stream_iter
Stream.__next__ = _stream_next
Buffer.__iter__ = _buffer_iter

