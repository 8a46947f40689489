"""What the gradients with respect to the four scalars of Polyblur are, restated for the tests in NumPy / torch by
hand (float64 unless asked otherwise; CPU only), beside autograd_ref.py (the non-blind step) and estimation_grad_ref.py (the estimation).

The polynomial out = a3 K^3 x + a2 K^2 x + a1 K x + beta x, a3 = alpha / 2 - beta + 2, a2 = 3 beta - alpha - 6, a1 = 5 - 3 beta +
alpha / 2, with upstream gradient G:

    d loss / d alpha = 1/2 <G, K (1 - K)^2 x>,      d loss / d beta = <G, (1 - K)^3 x>,

evaluated from the detail images u1 = x - K x, u2 = u1 - K u1, u3 = u2 - K u2: d beta = sum G u3, d alpha = 1/2 sum G (u2 - u3).

The estimation's model v = c^2 / (m^2 + 1e-8) - b^2 (v = sigma^2, rho^2, clamped to [0.09, 16] before the root): with dv_e =
d loss / d v_e, zero where the clamp is active,

    d loss / d c = sum_e dv_e 2 c / (m_e^2 + 1e-8),      d loss / d b = -2 b sum_e dv_e.

The blind call chains both, n_iter times.  Every function takes the switches of the tests' mutants (what a wrong implementation would
compute); the defaults are the truth."""
import json
import os

import numpy as np
import torch

import autograd_ref as ar
import estimation_grad_ref as er

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "params_grad.npz")


# ---------------------------------------------------------------------------------------------
# the polynomial
# ---------------------------------------------------------------------------------------------
def details(x, k, method, dtype=torch.float64):
    """(u2, u3) of x (B,C,H,W) for k (kb,kc,kh,kw) under the boundary of `method`, numpy arrays of `dtype`"""
    xt, kt = torch.tensor(np.asarray(x), dtype=dtype), torch.tensor(np.ascontiguousarray(k), dtype=dtype)
    u1 = xt - ar.apply_k(xt, kt, method)
    u2 = u1 - ar.apply_k(u1, kt, method)
    u3 = u2 - ar.apply_k(u2, kt, method)
    return u2.numpy(), u3.numpy()


def poly_param_rows(x, k, g, method, dtype=torch.float64, half=0.5, direct_term=True, one_plane=False):
    """(rows, 2): (d / d alpha, d / d beta) per image as the engine counts images -- B, or B * C when the kernel has one set of taps
    per plane (the image then goes in as B * C one-channel images).  Mutants: half=1 (the 1/2 dropped), direct_term=False (the
    `+ x` of (1 - K)^3 x dropped), one_plane=True (plane 0 in place of the sum over an image's planes)"""
    u2, u3 = details(x, k, method, dtype)
    np_dtype = u2.dtype
    g, x = np.asarray(g, np_dtype), np.asarray(x, np_dtype)
    pa, pb = g * (u2 - u3), g * (u3 if direct_term else u3 - x)
    B, C = x.shape[:2]
    if np.asarray(k).shape[1] > 1:
        pa, pb = pa.reshape(B * C, 1, -1), pb.reshape(B * C, 1, -1)
    else:
        pa, pb = pa.reshape(B, C, -1), pb.reshape(B, C, -1)
    if one_plane:
        pa, pb = pa[:, :1], pb[:, :1]
    return np.stack([np_dtype.type(half) * pa.sum(axis=(1, 2)), pb.sum(axis=(1, 2))], axis=1)


def rank3_param_rows(x, k, w, alpha, b, method, **mutant):
    """the same for inverse_filtering_rank3 with loss = sum(w * out): the polynomial's rows on the padded domain, for the upstream
    gradient that passes the clamp"""
    xp, kk, g, _ = ar.rank3_upstream(x, k, w, alpha, b, method)
    return poly_param_rows(xp, kk, g, method, **mutant)


def smooth_image(seed, shape):
    """a blurred image in [0.05, 0.95] (float32 values) from additions and multiplications alone -- uniform noise under three
    circular [1 2 1] / 4 passes along either axis --, so that every machine gets the same bits; and weights in [-1, 1]"""
    rng = np.random.default_rng(seed)
    x = rng.random(shape)
    w = rng.uniform(-1, 1, shape).astype(np.float32)
    for _ in range(3):
        for ax in (-2, -1):
            x = 0.25 * np.roll(x, 1, ax) + 0.5 * x + 0.25 * np.roll(x, -1, ax)
    lo, hi = x.min(axis=(1, 2, 3), keepdims=True), x.max(axis=(1, 2, 3), keepdims=True)
    return (0.05 + 0.9 * (x - lo) / (hi - lo)).astype(np.float32), w


def make_kernel(seed, kshape, kind):
    """'rank1': an axis-aligned Gaussian; 'oblique': a Gaussian at an angle (point-symmetric, not separable); 'dense': a caller's
    kernel that is neither separable nor point-symmetric.  One per (image, plane) of kshape, each of its own width; float32, sum 1.
    (The goldens store the kernels: exp is not the same bits on every machine.)"""
    rng = np.random.default_rng(seed)
    kb, kc, kh, kw = kshape
    yy, xx = np.meshgrid(np.arange(kh) - kh // 2, np.arange(kw) - kw // 2, indexing="ij")
    out = np.zeros(kshape)
    for i in range(kb):
        for j in range(kc):
            s1, s2 = rng.uniform(0.8, 1.2) * max(kw, 3) / 5.0, rng.uniform(0.5, 0.8) * max(kh, 3) / 6.0
            if kind == "dense":
                kk = rng.random((kh, kw)) ** 3 * np.exp(-0.5 * ((xx / (1.5 * s1)) ** 2 + (yy / (1.5 * s2)) ** 2))
            else:
                t = 0.0 if kind == "rank1" else rng.uniform(0.4, 1.1)
                u, v = np.cos(t) * xx + np.sin(t) * yy, -np.sin(t) * xx + np.cos(t) * yy
                kk = np.exp(-0.5 * ((u / s1) ** 2 + (v / s2) ** 2))
            out[i, j] = kk / kk.sum()
    return out.astype(np.float32)


# (function, image shape, kernel shape, kind of kernel, method, (alpha, beta)).  Sides that cross a wave and a window edge and hold
# the kernel: W in {10, 63, 64, 65, 130}, H in {6, 17, 33}, C in {1, 3, 4}, B = 2 -- B = 1 under 'direct', the only 'direct' form the
# reference runs (filters.py:45-49: one kernel for the whole batch) --; kernels 3 x 3, 5 x 9 and 25 x 25, per image and per plane
POLY = [
    ("polynomial", (2, 1, 6, 10), (2, 1, 3, 3), "rank1", "fft", (6, 1)),
    ("polynomial", (2, 3, 17, 63), (2, 1, 5, 9), "oblique", "fft", (2, 3)),
    ("polynomial", (2, 3, 17, 65), (2, 3, 5, 9), "dense", "fft", (6, 1)),
    ("polynomial", (2, 4, 33, 64), (2, 1, 25, 25), "oblique", "fft", (6, 1)),
    ("polynomial", (2, 1, 33, 130), (2, 1, 25, 25), "dense", "fft", (2, 3)),
    ("polynomial", (2, 4, 33, 130), (2, 4, 3, 3), "dense", "fft", (2, 3)),
    ("polynomial", (2, 3, 33, 65), (1, 1, 5, 9), "oblique", "fft", (2, 3)),
    ("polynomial", (1, 3, 17, 65), (1, 1, 5, 9), "dense", "direct", (6, 1)),
    ("polynomial", (1, 1, 33, 63), (1, 1, 25, 25), "rank1", "direct", (2, 3)),
    ("polynomial", (1, 4, 6, 10), (1, 1, 3, 3), "oblique", "direct", (6, 1)),
    ("rank3", (2, 3, 17, 63), (2, 1, 5, 9), "oblique", "fft", (6, 1)),
    ("rank3", (2, 1, 33, 65), (2, 1, 25, 25), "rank1", "fft", (2, 3)),
    ("rank3", (2, 4, 6, 10), (2, 4, 3, 3), "dense", "fft", (6, 1)),
    ("rank3", (1, 3, 17, 64), (1, 1, 3, 3), "dense", "direct", (2, 3)),
    ("rank3", (1, 1, 33, 130), (1, 1, 25, 25), "dense", "direct", (6, 1)),
]

# the estimation: make_golden_blind_autograd.ESTIMATION's shapes and clamp states, and one unblurred noise image on which both
# variances clamp (sigma and rho at 0.3): (shape, blur of the input or None, clamp state of (sigma, rho) asked for or None)
BOTH_CLAMPED = (True, True)
ESTIMATION = [
    ((1, 1, 16, 24), (2.2, 1.1), None),
    ((2, 3, 37, 45), (2.2, 1.1), (False, False)),
    ((2, 3, 40, 48), (2.4, 0.25), (False, True)),
    ((1, 3, 64, 56), (1.8, 1.0), (False, False)),
    ((1, 3, 32, 40), None, BOTH_CLAMPED),
]
EST_C, EST_B = 0.362, 0.464            # gaussian_blur_estimation's defaults
BLIND_C, BLIND_B = 0.352, 0.768        # polyblur_deblurring's


def noise_image(seed, shape):
    """unblurred uniform noise in [0.05, 0.95]: its gradient magnitudes put sigma^2 and rho^2 far below 0.09"""
    return (0.05 + 0.9 * np.random.default_rng(seed).random(shape)).astype(np.float32)


def estimation_dv(r, grad_kernel_b, dtype=np.float64, gate=True):
    """dv_e = d loss / d (sigma^2, rho^2) of one record for the upstream gradient of its kernel, and the two magnitudes m_e
    (estimation_grad_ref.estimate_backward's first half).  gate=False: the clamp's gate ignored (a mutant)"""
    sigma, rho = dtype(r["sigma"]), dtype(r["rho"])
    gK = np.asarray(grad_kernel_b, dtype).reshape(r["ker_size"], r["ker_size"])
    K, X, Y, c, s = er.taps(dtype(r["theta"]), sigma, rho, r["ker_size"], dtype)
    gE = (gK - (gK * K).sum()) * K
    d_i1 = (gE * dtype(-0.5) * (c * c * X * X + 2 * s * c * X * Y + s * s * Y * Y)).sum()
    d_i2 = (gE * dtype(-0.5) * (s * s * X * X - 2 * s * c * X * Y + c * c * Y * Y)).sum()
    d_par = (d_i1 * (-2 / sigma ** 3), d_i2 * (-2 / rho ** 3))
    dv = [d / (2 * par) if (0.09 <= v <= 16.0 or not gate) else dtype(0) for d, par, v in zip(d_par, (sigma, rho), r["v"])]
    m = [dtype(r["interp"][i]) for i in (r["i_min"], r["i_ortho"])]
    return dv, m


def estimation_param_rows(recs, grad_kernel, dtype=np.float64, gate=True, eps=1e-8):
    """(B, 2): (d / d c, d / d b) per image for the upstream gradient of the (B,1,k,k) kernels.  Mutants: gate=False, eps=0"""
    rows = []
    for bi, r in enumerate(recs):
        dv, m = estimation_dv(r, np.asarray(grad_kernel)[bi], dtype, gate)
        c, b = dtype(r["c"]), dtype(r["b"])
        rows.append([sum(d * 2 * c / (mm * mm + dtype(eps)) for d, mm in zip(dv, m)), -2 * b * sum(dv)])
    return np.asarray(rows, dtype)


# ---------------------------------------------------------------------------------------------
# the blind call: every iteration adds to all four
# ---------------------------------------------------------------------------------------------
def blind_param_grads(x, w, n_iter, alpha, beta, method, c=BLIND_C, b=BLIND_B, steps=None, last_only=False):
    """d sum(w * blind(x)) / d (c, b, alpha, beta), float64, summed over the images.  last_only: the last iteration's own
    contribution alone (a mutant: nothing reaches the earlier iterations)"""
    if steps is None:
        _, steps = er.blind(x, n_iter, alpha, beta, method, c, b)
    g = np.asarray(w, np.float64)
    total = np.zeros(4)
    for n, (xi, recs, _) in enumerate(reversed(steps)):
        xt = torch.tensor(xi, requires_grad=True)
        kt = torch.tensor(er.kernels(recs), requires_grad=True)
        at, bt = torch.tensor(float(alpha), dtype=torch.float64, requires_grad=True), torch.tensor(float(beta), dtype=torch.float64, requires_grad=True)
        ar.rank3(xt, kt, at, bt, method).clip(0.0, 1.0).backward(torch.tensor(g))
        cb = estimation_param_rows(recs, kt.grad.numpy()).sum(axis=0)
        total += np.array([cb[0], cb[1], float(at.grad), float(bt.grad)])
        if last_only:
            break
        g = xt.grad.numpy() + er.estimate_backward(recs, grad_kernel=kt.grad.numpy())
    return total


# ---------------------------------------------------------------------------------------------
# the goldens, and the figures the tolerances come from
# ---------------------------------------------------------------------------------------------
def load_golden():
    z = np.load(GOLDEN)
    return z, json.loads(str(z["cases"]))


def rel_error(got, want):
    """largest |got - want| relative to the case's larger gradient"""
    got, want = np.asarray(got, np.float64).reshape(-1), np.asarray(want, np.float64).reshape(-1)
    return float(np.abs(got - want).max() / np.abs(want).max())


# The tolerances, relative to the case's larger gradient.  E is the error of the reference's own float32 gradient against the float64
# truth -- the reference's float64 for the polynomial, this restatement for the estimation and the blind call --, recorded as
# make_golden_params_autograd.py printed it, and every tolerance is 6 E of its own setting (between 4 E and 8 E; the factor DESIGN.md
# 4.15 took).  tests/test_params_autograd_cpu.py measures every E again and holds each tolerance to its interval.
TOL_FACTOR = 6.0
# the polynomial: per case -- the reference has a float64 gradient for each, and the cases differ a hundredfold (p00, the 6 x 10 image
# under a 3 x 3 kernel, has gradients of 6e-3 from sixty samples: its E must not set the bound of a 33 x 130 image)
E_POLY = {"p00": 3.14e-4, "p01": 1.26e-6, "p02": 1.82e-6, "p03": 6.32e-6, "p04": 7.09e-6, "p05": 1.11e-5, "p06": 9.80e-6, "p07": 1.60e-6,
          "p08": 1.21e-6, "p09": 5.78e-5, "p10": 1.24e-6, "p11": 7.96e-6, "p12": 1.13e-5, "p13": 6.96e-5, "p14": 1.26e-6}
# the estimation (one (c, b) throughout): per clamp state, the largest E over its cases -- with neither variance clamped (e00, e01, e03;
# e00 the largest) and with rho clamped low (e02).  With both clamped the gradient is exactly (0, 0): no tolerance
E_EST = {"unclamped": 2.83e-7, "rho_low": 6.55e-6}
# the blind call: per (alpha, beta, method), the largest E over n_iter = 1 .. 3 (b01; b05; b06)
E_BLIND = {(6, 1, "fft"): 4.67e-6, (2, 3, "fft"): 2.37e-6, (6, 1, "direct"): 2.42e-5}
TOL_POLY = {k: TOL_FACTOR * e for k, e in E_POLY.items()}
TOL_EST = {k: TOL_FACTOR * e for k, e in E_EST.items()}
TOL_BLIND = {k: TOL_FACTOR * e for k, e in E_BLIND.items()}


def est_setting(case):
    """the clamp state of an estimation case of the goldens: 'unclamped', 'rho_low' or 'both'"""
    flags = {tuple(f) for f in case["clamped"]}
    return {((False, False),): "unclamped", ((False, True),): "rho_low", ((True, True),): "both"}[tuple(sorted(flags))]


def blind_setting(case):
    return (case["alpha"], case["beta"], case["method"])
