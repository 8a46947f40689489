"""What the gradient of the blind estimation is, restated for the tests in NumPy by hand (float64 unless asked otherwise; CPU only;
DESIGN.md 4.8), as autograd_ref.py restates the non-blind step.

Forward (blur_estimation.py:18-79, q = 0): g = channel mean, n = (g - lo) / (hi - lo), gx / gy = the spectral derivative of n
(filters.py:159-186: a circular correlation of every row / column with the impulse response `deriv_kernel`), mags[a] =
max |cos t_a gx - sin t_a gy| over the pixels (masked ones count as 0), interp = W mags (Keys' cubic), i_min = argmin interp,
(sigma, rho) = sqrt(clamp(c^2 / (m^2 + 1e-8) - b^2, 0.09, 16)) of interp[i_min] and interp[i_ortho], kernel = the normalised
Gaussian of (theta, sigma, rho) on the grid arange(k) - (k - 1) // 2.

Backward: `estimate_backward` walks that chain in reverse with the forward's own values (arg-max pixels and signs, i_min, the
clamp's state) -- the amax to its arg-max pixel, amin / amax of the range shared evenly among ties, as torch does.

`blind` / `blind_gradient`: the blind call as estimate -> autograd_ref's rank-3 chain -> clip, n_iter times, and its gradient by
chaining this file's backward with torch's float64 autograd of that chain; `detach_kernel=True` treats every estimated kernel as
a constant (what the gradient would be without the estimation's path)."""
import numpy as np
import torch

import autograd_ref as ar

N_ANGLES, N_INTERP = 6, 30
SAT_THRESHOLD = 0.99


def deriv_kernel(N, dtype=np.float64):
    """d with (spectral derivative of x)[j] = sum_m x[m] d[(j - m) mod N]: d[0] = 0, N odd: (pi / N) (-1)^n / sin(pi n / N),
    N even: (pi / N) (-1)^n / tan(pi n / N) (the Nyquist bin is dropped by real())"""
    n = np.arange(1, N, dtype=np.float64)
    sign = np.where(np.arange(1, N) % 2 == 1, -1.0, 1.0)
    d = np.zeros(N)
    d[1:] = (np.pi / N) * sign / (np.sin(np.pi * n / N) if N % 2 else np.tan(np.pi * n / N))
    return d.astype(dtype)


def deriv_matrix(N, dtype=np.float64):
    """M[j, m] = d[(j - m) mod N]: the derivative of a line x is M @ x, its adjoint M.T @ g"""
    d = deriv_kernel(N, dtype)
    j, m = np.meshgrid(np.arange(N), np.arange(N), indexing="ij")
    return d[(j - m) % N]


def deriv_kernel_by_ifft(N):
    """the same impulse response from the reference's own recipe (filters.py:172-184) on a unit impulse, 1-D, float64"""
    U = np.fft.fftshift(np.fft.fft(np.eye(N)[0]))
    freq = (np.arange(N) - N // 2) / N
    return np.real(np.fft.ifft(np.fft.ifftshift(2 * np.pi * freq * (-U.imag + 1j * U.real))))


def interp_weights(n_angles=N_ANGLES, n_interp=N_INTERP, dtype=np.float64):
    """Keys' cubic weights of cubic_interpolator (blur_estimation.py:138-148), rows normalised by their sum + 1e-5"""
    x = np.linspace(0, 180, n_angles + 1) / n_interp
    xn = (np.arange(n_interp) * (180 / n_interp)) / n_interp
    t = np.abs(xn[:, None] - x[None, :])
    w = np.where(t < 1, (1.5 * t - 2.5) * t * t + 1, np.where(t < 2, ((-0.5 * t + 2.5) * t - 4) * t + 2, 0.0))
    return (w / (w.sum(axis=1, keepdims=True) + 1e-5)).astype(dtype)


def angles(n_angles=N_ANGLES, dtype=np.float64):
    t = np.linspace(0, np.pi, n_angles + 1)
    return np.cos(t).astype(dtype), np.sin(t).astype(dtype)


def taps(theta, sigma, rho, k, dtype=np.float64):
    """create_gaussian_filter (blur_estimation.py:189-232) of one image -> (kernel, X, Y, c, s)"""
    th = dtype(-theta)
    c, s = np.cos(th), np.sin(th)
    i1, i2 = 1 / (sigma * sigma), 1 / (rho * rho)
    t = (np.arange(k) - (k - 1) // 2).astype(dtype)
    X, Y = np.meshgrid(t, t, indexing="xy")
    Q = (c * c * i1 + s * s * i2) * X * X + 2 * s * c * (i1 - i2) * X * Y + (c * c * i2 + s * s * i1) * Y * Y
    E = np.exp(-0.5 * Q)
    return (E / E.sum()).astype(dtype), X, Y, c, s


def estimate(img, c=0.362, b=0.464, ker_size=25, discard_saturation=False, dtype=np.float64):
    """the forward of every image of a (B,C,H,W) batch -> list of records (dicts)"""
    img = np.asarray(img, dtype)
    B, C, H, W = img.shape
    Mw, Mh = deriv_matrix(W, dtype), deriv_matrix(H, dtype)
    cs, sn = angles(dtype=dtype)
    Wt = interp_weights(dtype=dtype)
    out = []
    for bi in range(B):
        g = img[bi].mean(axis=0, dtype=dtype)
        lo, hi = g.min(), g.max()
        n = (g - lo) / (hi - lo)
        gx, gy = n @ Mw.T, Mh @ n
        if discard_saturation:
            mask = g > dtype(SAT_THRESHOLD)
            gx, gy = np.where(mask, 0, gx), np.where(mask, 0, gy)
        proj = cs[:, None, None] * gx[None] - sn[:, None, None] * gy[None]
        flat = np.abs(proj).reshape(len(cs), -1)
        arg = flat.argmax(axis=1)
        mags = flat[np.arange(len(cs)), arg]
        runner = np.sort(flat, axis=1)[:, -2]
        interp = Wt @ mags
        i_min = int(np.argmin(interp))
        theta_deg = int(i_min * (180 / N_INTERP))
        i_ortho = int(((theta_deg + 90) % 180) / (180 / N_INTERP))
        v = [dtype(c * c) / (interp[i] * interp[i] + dtype(1e-8)) - dtype(b * b) for i in (i_min, i_ortho)]
        sigma, rho = (np.sqrt(np.clip(x, dtype(0.09), dtype(16.0))) for x in v)
        theta = dtype(theta_deg) * dtype(np.pi) / dtype(180)
        kernel = taps(theta, sigma, rho, ker_size, dtype)[0]
        out.append(dict(gray=g, lo=lo, hi=hi, arg=arg, sign=np.sign(proj.reshape(len(cs), -1)[np.arange(len(cs)), arg]), mags=mags,
                        runner=runner, interp=interp, i_min=i_min, i_ortho=i_ortho, v=v, sigma=sigma, rho=rho, theta=theta,
                        kernel=kernel, ker_size=ker_size, c=c, b=b, shape=(C, H, W)))
    return out


def kernels(recs):
    return np.stack([r["kernel"] for r in recs])[:, None]


def estimate_backward(recs, grad_kernel=None, grad_sigma_rho=None, dtype=np.float64):
    """d loss / d image (B,C,H,W) for the upstream gradients of the (B,1,k,k) kernels and / or of (sigma, rho) (B,2)"""
    cs, sn = angles(dtype=dtype)
    Wt = interp_weights(dtype=dtype)
    grads = []
    for bi, r in enumerate(recs):
        C, H, W = r["shape"]
        sigma, rho = dtype(r["sigma"]), dtype(r["rho"])
        d_sigma = d_rho = dtype(0)
        if grad_kernel is not None:
            gK = np.asarray(grad_kernel, dtype)[bi].reshape(r["ker_size"], r["ker_size"])
            K, X, Y, c, s = taps(dtype(r["theta"]), sigma, rho, r["ker_size"], dtype)
            gE = (gK - (gK * K).sum()) * K
            d_i1 = (gE * dtype(-0.5) * (c * c * X * X + 2 * s * c * X * Y + s * s * Y * Y)).sum()
            d_i2 = (gE * dtype(-0.5) * (s * s * X * X - 2 * s * c * X * Y + c * c * Y * Y)).sum()
            d_sigma, d_rho = d_i1 * (-2 / sigma ** 3), d_i2 * (-2 / rho ** 3)
        if grad_sigma_rho is not None:
            d_sigma = d_sigma + dtype(np.asarray(grad_sigma_rho)[bi, 0])
            d_rho = d_rho + dtype(np.asarray(grad_sigma_rho)[bi, 1])
        interp = r["interp"].astype(dtype)
        d_interp = np.zeros(len(interp), dtype)
        cc = dtype(r["c"] * r["c"])
        for i, v, d_par, par in ((r["i_min"], r["v"][0], d_sigma, sigma), (r["i_ortho"], r["v"][1], d_rho, rho)):
            d_v = d_par / (2 * par) if 0.09 <= v <= 16.0 else dtype(0)
            m = interp[i]
            d_interp[i] += d_v * (-2 * cc * m) / (m * m + dtype(1e-8)) ** 2
        d_mags = Wt.T @ d_interp
        g = r["gray"].astype(dtype)
        lo, hi = dtype(r["lo"]), dtype(r["hi"])
        dw, dh = deriv_kernel(W, dtype), deriv_kernel(H, dtype)
        dn = np.zeros((H, W), dtype)
        for a in range(len(cs)):
            ia, ja = divmod(int(r["arg"][a]), W)
            coef_x = d_mags[a] * dtype(r["sign"][a]) * cs[a]
            coef_y = -d_mags[a] * dtype(r["sign"][a]) * sn[a]
            dn[ia, :] += coef_x * dw[(ja - np.arange(W)) % W]
            dn[:, ja] += coef_y * dh[(ia - np.arange(H)) % H]
        rng = hi - lo
        dg = dn / rng
        d_lo = (dn * (g - hi)).sum() / (rng * rng)
        d_hi = -(dn * (g - lo)).sum() / (rng * rng)
        at_lo, at_hi = g == lo, g == hi
        dg = dg + at_lo * (d_lo / at_lo.sum()) + at_hi * (d_hi / at_hi.sum())
        grads.append(np.broadcast_to(dg / C, (C, H, W)))
    return np.stack(grads).astype(dtype)


# ---------------------------------------------------------------------------------------------
# the blind call: estimate -> rank-3 chain -> clip, n_iter times
# ---------------------------------------------------------------------------------------------
def blind(x, n_iter, alpha, beta, method, c=0.352, b=0.768, ker_size=25):
    """-> (output, the per-iteration (input, records, unclamped output) list), float64"""
    x = np.asarray(x, np.float64)
    steps = []
    for _ in range(n_iter):
        recs = estimate(x, c, b, ker_size)
        k = kernels(recs)
        yu = ar.rank3_unclamped(torch.tensor(x), torch.tensor(k), alpha, beta, method).numpy()
        steps.append((x, recs, yu))
        x = np.clip(yu, 0.0, 1.0)
    return x, steps


def blind_gradient(x, w, n_iter, alpha, beta, method, c=0.352, b=0.768, ker_size=25, detach_kernel=False, steps=None):
    """d sum(w * blind(x)) / d x, float64"""
    if steps is None:
        _, steps = blind(x, n_iter, alpha, beta, method, c, b, ker_size)
    g = np.asarray(w, np.float64)
    for xi, recs, _ in reversed(steps):
        xt = torch.tensor(xi, requires_grad=True)
        kt = torch.tensor(kernels(recs), requires_grad=True)
        ar.rank3(xt, kt, alpha, beta, method).clip(0.0, 1.0).backward(torch.tensor(g))
        g = xt.grad.numpy()
        if not detach_kernel:
            g = g + estimate_backward(recs, grad_kernel=kt.grad.numpy())
    return g


# ---------------------------------------------------------------------------------------------
# inputs and the margins a case must keep (the golden generator searches its seeds for them; the CPU test recomputes them)
# ---------------------------------------------------------------------------------------------
def blurred_noise(seed, shape, sig=(2.2, 1.1), angle=0.6):
    """uniform noise blurred by an oblique Gaussian (circular, through the FFT) and scaled into [0.05, 0.95]; float32 values"""
    rng = np.random.default_rng(seed)
    B, C, H, W = shape
    x = rng.random(shape)
    fy, fx = np.meshgrid(np.fft.fftfreq(H), np.fft.fftfreq(W), indexing="ij")
    u, v = np.cos(angle) * fx + np.sin(angle) * fy, -np.sin(angle) * fx + np.cos(angle) * fy
    G = np.exp(-2 * np.pi ** 2 * ((sig[0] * u) ** 2 + (sig[1] * v) ** 2))
    y = np.real(np.fft.ifft2(np.fft.fft2(x) * G))
    lo, hi = y.min(axis=(1, 2, 3), keepdims=True), y.max(axis=(1, 2, 3), keepdims=True)
    return (0.05 + 0.9 * (y - lo) / (hi - lo)).astype(np.float32)


def margins(recs):
    """of one estimation: (smallest relative gap of a directional maximum to its runner-up, smallest gap of the two lowest / two
    highest gray values relative to the range, relative gap of the two smallest interpolated magnitudes, smallest relative distance
    of an unclamped sigma^2 / rho^2 to 0.09 and 16 -- inf when clamped well inside, i.e. beyond the bounds by 1 % --, flags (sigma
    clamped, rho clamped) per image)"""
    amax = gray = imin = clamp = np.inf
    flags = []
    for r in recs:
        amax = min(amax, float(np.min((r["mags"] - r["runner"]) / r["mags"])))
        s = np.sort(r["gray"].reshape(-1))
        gray = min(gray, float(min(s[1] - s[0], s[-1] - s[-2]) / (s[-1] - s[0])))
        t = np.sort(r["interp"])
        imin = min(imin, float((t[1] - t[0]) / abs(t[0])))
        fl = []
        for v in r["v"]:
            clamp = min(clamp, min(abs(float(v) - 0.09) / 0.09, abs(float(v) - 16.0) / 16.0))
            fl.append(not (0.09 <= v <= 16.0))
        flags.append(tuple(fl))
    return amax, gray, imin, clamp, flags


def case_ok(recs, amax=1e-3, gray=1e-3, imin=1e-3, clamp=1e-2):
    m = margins(recs)
    return m[0] >= amax and m[1] >= gray and m[2] >= imin and m[3] >= clamp


# ---------------------------------------------------------------------------------------------
# the cases of pb_estimate_blur_backward alone (tests/test_gpu_blind_autograd.py), beside the goldens' estimation cases
# ---------------------------------------------------------------------------------------------
def _searched(seed, shape, sig):
    while True:
        x = blurred_noise(seed, shape, sig)
        if case_ok(estimate(x)):
            return x
        seed += 1


def edges_image():
    """strong edges at the border: a horizontal step pair in the last row and a vertical one in the last column that ends in the
    last row -- arg-max pixels in row 0 (around the seam), in the last row and in the last column (the CPU test asserts it)"""
    x = 0.45 + 0.1 * blurred_noise(31, (1, 1, 33, 47), (1.5, 1.5))
    x[0, 0, 32, 10], x[0, 0, 32, 11] = 0.02, 0.97
    x[0, 0, 32, 46], x[0, 0, 31, 46] = 0.10, 0.93
    return x.astype(np.float32)


def ties_image():
    """several pixels at exactly 0 and exactly 1 in every channel: d lo and d hi are split evenly among them"""
    x = blurred_noise(41, (1, 3, 30, 44), (1.8, 1.0)).copy()
    for i, j in ((3, 5), (12, 30), (25, 9)):
        x[0, :, i, j] = 0.0
    for i, j in ((7, 21), (18, 40), (22, 2), (28, 28)):
        x[0, :, i, j] = 1.0
    return x


def saturated_image():
    """discard_saturation=True: the largest gradients lie on saturated pixels (next to dark ones) and must not be picked"""
    x = (0.1 + 0.8 * blurred_noise(51, (1, 3, 36, 40), (1.6, 1.2))).astype(np.float32)
    x[0, :, 10:14, 8] = 0.03
    x[0, :, 10:14, 9:12] = 0.995
    x[0, :, 24, 20:25] = 0.02
    x[0, :, 25:28, 20:25] = 0.997
    return x


def backward_cases():
    """-> (id, image, discard_saturation), float32 images"""
    return [("130x257", _searched(61, (1, 1, 130, 257), (2.2, 1.1)), False),      # several workgroups per image, no multiple of anything
            ("edges", edges_image(), False), ("ties", ties_image(), False), ("saturated", saturated_image(), True)]


def kernel_weights(seed, B, k=25):
    return np.random.default_rng(seed).uniform(-1, 1, (B, 1, k, k)).astype(np.float32)


def per_image_error(got, want):
    """largest |got - want| relative to max |want|, per image -> the largest over the batch"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(max(np.abs(g - w).max() / np.abs(w).max() for g, w in zip(got, want)))


# The GPU test's tolerance for pb_estimate_blur_backward, relative to max |grad| per image: 4 x the largest error of the float32 CPU
# evaluation of this restatement against float64 over backward_cases() and the goldens' estimation cases
# (2.30e-6, the 130 x 257 case; tests/test_blind_autograd_cpu.py measures it again and holds the constant to it)
TOL_EST = 9.2e-6
# 4 x the largest |restatement - golden| / max |golden| over tests/golden/blind_grad.npz (1.39e-5, b06: two iterations under
# 'direct'): the reference's own float32 error
BOUND_GOLDEN = 5.6e-5
