"""NumPy restatement of Pillow's ImageFilter.GaussianBlur / BoxBlur on (h, w, 3)
uint8 images: the closed form of one extended box pass with clamped indices,
uint32 arithmetic, a byte rounding after every pass (include/mxd_amd.h)."""
import numpy as np

F = np.float32


def params(radius, gaussian):
    """(fr, ww, fw, passes): float32 throughout, except the double square root."""
    fr = F(radius)
    if gaussian:
        s2 = F(F(F(radius) * F(radius)) / F(3))
        big = F(np.sqrt(12.0 * np.float64(s2) + 1.0))
        lo = F(np.floor(F(F(big - F(1)) / F(2))))
        a = F(F(F(2) * lo + F(1)) * F(F(lo * F(lo + F(1))) - F(F(3) * s2)))
        fr = F(lo + F(a / F(F(6) * F(s2 - F(F(lo + F(1)) * F(lo + F(1)))))))
    ww = int(F(F(1 << 24) / F(F(fr * F(2)) + F(1))))
    return fr, ww, ((1 << 24) - (2 * int(fr) + 1) * ww) // 2, 3 if gaussian else 1


def box_pass(img, axis, R, ww, fw):
    n = img.shape[axis]
    at = lambda d: np.take(img, np.clip(np.arange(n) + d, 0, n - 1), axis=axis).astype(np.uint32)  # noqa: E731
    box = sum(at(d) for d in range(-R, R + 1))
    return ((np.uint32(ww) * box + np.uint32(fw) * (at(-R - 1) + at(R + 1)) + np.uint32(1 << 23)) >> np.uint32(24)).astype(np.uint8)


def blur(img, radius, gaussian):
    fr, ww, fw, passes = params(radius, gaussian)
    for axis in (1, 0):
        for _ in range(passes if fr != 0 else 0):
            img = box_pass(img, axis, int(fr), ww, fw)
    return img.copy()
