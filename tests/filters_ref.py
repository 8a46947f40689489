"""The bilateral filter in float64 (reference filters.py:107-148, any odd window): the yardstick of tests/test_gpu_edge_aware.py,
itself checked against the fp32 oracle in tests/test_edge_aware_cpu.py."""
import numpy as np


def bilateral_f64(x, ksize=5, sigma_spatial=5.0, sigma_color=0.1):
    """per plane, replicate pad of ksize // 2; the weight of a tap exp(-(dx^2 + dy^2) / (2 sigma_spatial^2))
    exp(-(v - centre)^2 / (2 sigma_color^2)); sum w v / (sum w + 1e-5)"""
    x = np.asarray(x, np.float64)
    r = ksize // 2
    h, w = x.shape[-2:]
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)], mode="edge")
    num, den = np.zeros_like(x), np.zeros_like(x)
    for i in range(ksize):
        for j in range(ksize):
            s = xp[..., i:i + h, j:j + w]
            wgt = np.exp(-((i - r) ** 2 + (j - r) ** 2) / (2.0 * sigma_spatial ** 2) - (s - x) ** 2 / (2.0 * sigma_color ** 2))
            num += wgt * s
            den += wgt
    return num / (den + 1e-5)


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))
