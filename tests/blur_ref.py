"""References for MXD_ENHANCE_GAUSSIAN_BLUR (include/mxd_amd.h), both on the
weights of mxd_gaussian_weights: a NumPy float32 restatement in the contract's
operation order, and a float64 direct 2-D convolution."""
import numpy as np

from mlx_data_amd import capi


def reflect_index(i, n):
    """torch / NumPy 'reflect' of the indices i into 0..n-1 (period 2 (n - 1); 0 for n == 1)."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    i = np.mod(i, 2 * (n - 1))
    return np.where(i < n, i, 2 * (n - 1) - i)


def blur_f32(img, kernel_size, sigma):
    """The contract's arithmetic on an (h, w, 3) uint8 image: H then V, symmetric form,
    every product and sum a float32 operation, rint, clamp."""
    w = capi.gaussian_weights(sigma, kernel_size)
    r = (kernel_size - 1) // 2
    h_, w_ = img.shape[:2]
    q = img.astype(np.int32)
    xs, ys = np.arange(w_), np.arange(h_)
    a = w[r] * q.astype(np.float32)
    for d in range(1, r + 1):
        pair = q[:, reflect_index(xs - d, w_)] + q[:, reflect_index(xs + d, w_)]
        a = a + w[r + d] * pair.astype(np.float32)
    assert a.dtype == np.float32
    v = w[r] * a
    for d in range(1, r + 1):
        pair = a[reflect_index(ys - d, h_)] + a[reflect_index(ys + d, h_)]
        v = v + w[r + d] * pair
    assert v.dtype == np.float32
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def blur_f64(img, kernel_size, sigma):
    """float64: the direct 2-D convolution with the outer product of the same weights over
    the reflect-indexed image (not rounded)."""
    w = capi.gaussian_weights(sigma, kernel_size).astype(np.float64)
    r = (kernel_size - 1) // 2
    h_, w_ = img.shape[:2]
    q = img.astype(np.float64)
    xs, ys = np.arange(w_), np.arange(h_)
    out = np.zeros(q.shape)
    for j in range(kernel_size):
        rows = q[reflect_index(ys + j - r, h_)]
        for i in range(kernel_size):
            out += (w[j] * w[i]) * rows[:, reflect_index(xs + i - r, w_)]
    return out


def rand_image(h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
