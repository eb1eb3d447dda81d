"""Helpers of the formatted-output tests (tests/test_out_format.py,
tests/test_gpu_out_format.py): the NumPy / torch statement of what a result
byte becomes under an mxd_out_format, and a runner of mxd_resize_crop_batch_fmt
on device buffers (like gpu_util.run_device)."""
import numpy as np
import torch

from mlx_data_amd import capi

IMAGENET_MEAN = (0.485, 0.456, 0.406)
IMAGENET_STD = (0.229, 0.224, 0.225)
ELEMS = {"float32": capi.MXD_ELEM_F32, "float16": capi.MXD_ELEM_F16, "bfloat16": capi.MXD_ELEM_BF16}
LAYOUTS = {"hwc": capi.MXD_LAYOUT_HWC, "chw": capi.MXD_LAYOUT_CHW}


def expected_table(elem, channels, mean=None, std=None):
    """(channels, 256) integer bits of ((u8.astype("float32") / 255) - mean) /
    std, then .astype("float16") / torch's .to(torch.bfloat16): uint32 for
    float32, uint16 otherwise.  mean / std: None, a scalar or one per channel."""
    q = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None], (256, channels))
    y = q.astype("float32") / np.float32(255)
    if mean is not None or std is not None:
        m = np.broadcast_to(np.asarray(0.0 if mean is None else mean, np.float32), (channels,))
        s = np.broadcast_to(np.asarray(1.0 if std is None else std, np.float32), (channels,))
        with np.errstate(over="ignore"):
            y = (y - m) / s
    assert y.dtype == np.float32
    if elem == "float32":
        bits = y.view(np.uint32)
    elif elem == "float16":
        with np.errstate(over="ignore"):
            bits = y.astype("float16").view(np.uint16)
    else:
        bits = torch.from_numpy(np.ascontiguousarray(y)).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    return np.ascontiguousarray(bits.T)


def expect(table, want_u8):
    """The formatted image of (H, W, C) result bytes: table[c][q] per channel."""
    c = want_u8.shape[2]
    return np.stack([table[k][want_u8[:, :, k]] for k in range(c)], axis=2)


class FmtRun:
    """Sources and formatted destinations of a batch in device memory, and its
    descriptor array; launch(fmt-ish) runs mxd_resize_crop_batch_fmt and reads
    every image back as (H, W, C) integer bits.

    elem / layout fix the destinations' geometry: rows ``dst_pad`` elements
    longer than the pixels, planes (CHW) ``plane_pad`` elements longer than
    crop_h rows -- one plane_stride per call, sized for its largest image --
    and each destination ``dst_shift`` elements past a 256-byte boundary.
    ``rgba_weighted``: one flag for every image, or one per image."""

    def __init__(self, images, geoms, elem, layout, dst_pad=0, plane_pad=0, dst_shift=0, rgba_weighted=0,
                 src_align=16, device=0):
        self.images, self.geoms, self.elem, self.layout = images, geoms, elem, layout
        self.es = 4 if elem == "float32" else 2
        self.device = device
        es = self.es
        pitches, offs, total = [], [], 0
        for img in images:
            h, w, c = img.shape
            p = (w * c + src_align - 1) // src_align * src_align
            pitches.append(p)
            offs.append(total)
            total += (p * h + 255) // 256 * 256
        self.src = capi.DeviceBuffer(total + 256, device)
        host = np.zeros(total + 256, np.uint8)
        for img, p, o in zip(images, pitches, offs):
            h, w, c = img.shape
            host[o: o + p * h].reshape(h, p)[:, : w * c] = img.reshape(h, w * c)
        self.src.upload(host)
        chw = layout == "chw"
        self.plane_stride = 0
        if chw:
            self.plane_stride = max((g[4] + dst_pad) * es * g[5] for g in geoms) + plane_pad * es
        self.dsts, entries = [], []
        weighted = rgba_weighted if isinstance(rgba_weighted, (list, tuple)) else [rgba_weighted] * len(images)
        for img, g, p, o, wt in zip(images, geoms, pitches, offs, weighted):
            rw, rh, cx, cy, cw, ch, flip = g
            c = img.shape[2]
            dpitch = (cw * (1 if chw else c) + dst_pad) * es
            size = self.plane_stride * c if chw else dpitch * ch
            d = capi.DeviceBuffer(size + 256 + dst_shift * es, device)
            self.dsts.append((d, dpitch, size))
            entries.append(dict(src=self.src.ptr + o, src_stride=p, src_w=img.shape[1], src_h=img.shape[0], channels=c,
                                resize_w=rw, resize_h=rh, crop_x=cx, crop_y=cy, crop_w=cw, crop_h=ch, flip=int(flip),
                                dst=d.ptr + dst_shift * es, dst_stride=dpitch, rgba_weighted=int(wt)))
        self.dst_shift = dst_shift
        self.arr, self.n = capi.make_images(entries)

    def fmt(self, mean=None, std=None):
        return capi.make_out_format(ELEMS[self.elem], LAYOUTS[self.layout], mean, std, self.plane_stride)

    def launch(self, mean=None, std=None, stream=None):
        """Clears the destinations (0xff bytes), launches, returns the outputs
        and, per image, whether every byte outside its elements kept 0xff."""
        for d, _, _ in self.dsts:
            d.memset(0xFF)
        capi.check(capi.lib().mxd_device_synchronize(self.device))
        capi.resize_crop_batch_fmt(self.arr, self.n, self.fmt(mean, std), self.device,
                                   stream.handle if stream else None)
        if stream:
            stream.synchronize()
        return self.read()

    def read(self):
        es, chw = self.es, self.layout == "chw"
        ut = np.uint32 if es == 4 else np.uint16
        outs, clean = [], []
        for (d, dpitch, size), g, img in zip(self.dsts, self.geoms, self.images):
            cw, ch, c = g[4], g[5], img.shape[2]
            raw = d.download((size + 256 + self.dst_shift * es,), np.uint8)
            body = raw[self.dst_shift * es: self.dst_shift * es + size]
            mask = np.ones(raw.shape, bool)
            if chw:
                planes = [body[k * self.plane_stride: k * self.plane_stride + dpitch * ch].reshape(ch, dpitch)
                          for k in range(c)]
                out = np.stack([pl[:, : cw * es].copy().view(ut) for pl in planes], axis=2)
                for k in range(c):
                    m = mask[self.dst_shift * es + k * self.plane_stride:][: dpitch * ch].reshape(ch, dpitch)
                    m[:, : cw * es] = False
            else:
                rows = body.reshape(ch, dpitch)
                out = rows[:, : cw * c * es].copy().view(ut).reshape(ch, cw, c)
                mask[self.dst_shift * es:][: dpitch * ch].reshape(ch, dpitch)[:, : cw * c * es] = False
            outs.append(out)
            clean.append(bool((raw[mask] == 0xFF).all()))
        return outs, clean

    def free(self):
        for d, _, _ in self.dsts:
            d.free()
        self.src.free()
