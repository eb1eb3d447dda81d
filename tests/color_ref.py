"""Reference statements of the colour transform for
tests/test_color.py and tests/test_gpu_color.py: NumPy only, nothing from the
code under test."""
import numpy as np

YIQ = np.array([[0.299, 0.587, 0.114], [0.595716, -0.274453, -0.321263], [0.211456, -0.522591, 0.311135]])


def twist_ref(brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0):
    """float64 (3, 4) matrix [A | t] of M = B . C . S . H for [r g b 1] in
    [0, 1] units (the offset column NOT yet multiplied by 255)."""
    a = np.radians(hue)
    rot = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    m = np.eye(4)

    def step(a3, t=(0, 0, 0)):
        s = np.eye(4)
        s[:3, :3] = a3
        s[:3, 3] = t
        return s

    m = step(np.linalg.inv(YIQ) @ rot @ YIQ) @ m
    m = step(saturation * np.eye(3) + (1 - saturation) * np.outer(np.ones(3), YIQ[0])) @ m
    m = step(contrast * np.eye(3), [0.5 * (1 - contrast)] * 3) @ m
    m = step(brightness * np.eye(3)) @ m  # (scales the offset column too)
    return m[:3]


def to_bytes_units(m01):
    """A (3, 3) or (3, 4) matrix in [0, 1] units -> float32 (3, 4) in byte units."""
    m = np.zeros((3, 4))
    m01 = np.asarray(m01, np.float64)
    m[:, : m01.shape[1]] = m01
    m[:, 3] *= 255.0
    return m.astype(np.float32)


def apply_ref(rgb, m):
    """The arithmetic of section 2 on (..., 3) uint8 pixels: float32 products
    and sums in the stated order, each rounded, then the project's encode."""
    m = np.asarray(m, np.float32).reshape(3, 4).copy()
    m[np.abs(m) < np.float32(2.0 ** -100)] = 0
    q = [rgb[..., k].astype(np.float32) for k in range(3)]
    out = np.empty(rgb.shape, np.uint8)
    for c in range(3):
        v = ((m[c, 0] * q[0] + m[c, 1] * q[1]) + m[c, 2] * q[2]) + m[c, 3]
        assert v.dtype == np.float32
        out[..., c] = np.clip(v + np.float32(0.5), np.float32(0), np.float32(255)).astype(np.uint8)
    return out


IDENTITY = np.eye(3, 4, dtype=np.float32)
# clamps at both ends; negative entries; a channel permutation (BGR)
CLAMPING = np.array([[3.0, 0, 0, -200.0], [0, 2.5, 0.5, -150.0], [0.25, 0, 4.0, -300.0]], np.float32)
NEGATIVE = np.array([[-1.0, 0, 0, 255.0], [0.5, -0.75, 0.3, 120.0], [-0.2, -0.3, 1.5, 10.5]], np.float32)
SWAP = np.array([[0, 0, 1.0, 0], [0, 1.0, 0, 0], [1.0, 0, 0, 0]], np.float32)


def eight_matrices():
    """Eight different matrices: the identity, saturating ones, twists."""
    tw = [to_bytes_units(twist_ref(*p)) for p in ((1.3, 0.7, 1.6, 25.0), (0.6, 1.8, 0.0, -90.0), (1.0, 1.0, 2.5, 0.0))]
    return [IDENTITY, CLAMPING, NEGATIVE, SWAP, np.zeros((3, 4), np.float32)] + tw
