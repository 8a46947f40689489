"""The gradients of the polynomial with the pure-phase filter (deblurring.py:141-169, not_symmetric=True; p2o: filters.py:255-273),
restated in NumPy float64 for the tests (CPU only).  A helper of tests/test_phase_autograd_cpu.py,
tests/test_gpu_phase_autograd.py and tests/golden/make_golden_phase_autograd.py; it builds on tests/phase_ref.py and, for the chain
with the mask, on tests/halo_grad_ref.py.

With N = H W, eps = 1e-8, K = fft2(p2o(k)), r = |K|, C = conj(K) / (r + eps), P = ((a3 K + a2) K + a1) K + b,
P' = (3 a3 K + 2 a2) K + a1, M = C P, G = fft2(g), Y = fft2(x):

    image   grad_x = Re ifft2(conj(M) G)
    taps    A = (1 / N) sum over the planes that share the kernel of Y conj(G)
            C_K = -conj(K)^2 / (2 r (r + eps)^2)        C_Kbar = 1 / (r + eps) - r / (2 (r + eps)^2)
            S = A (C_K P + C P') + conj(A C_Kbar P)
            grad_k[i][j] = Re fft2(S) at row (i - kh // 2) mod H, column (j - kw // 2) mod W

The chain (inverse_filtering_nonsymmetric under grad): replicate pad by kw // 2 -> polynomial -> crop -> [halo masking] -> clamp."""
import contextlib
import functools

import numpy as np

import halo_grad_ref as hg
import halo_ref as hr
import phase_ref as pr

F32, F64 = np.float32, np.float64
EPS = 1e-8

MUTANTS = ["C constant", "conj term dropped", "M for conj(M)", "roll by (kh - 1) // 2", "one plane", "no 1 / N", "flip forgotten"]


def coefficients(alpha, b):
    return alpha / 2 - b + 2, 3 * b - alpha - 6, 5 - 3 * b + alpha / 2


def _parts(k, shape, alpha, b):
    a3, a2, a1 = coefficients(alpha, b)
    K = pr.otf(np.asarray(k, F64), shape, True)
    r = np.abs(K)
    C = np.conj(K) / (r + EPS)
    P = ((a3 * K + a2) * K + a1) * K + b
    dP = (3 * a3 * K + 2 * a2) * K + a1
    return K, r, C, P, dP


def forward(x, k, alpha, b):
    """x (B,C,H,W), the whole domain; k (B or 1, C or 1, kh, kw) -> float64, unclamped"""
    x = np.asarray(x, F64)
    _, _, C, P, _ = _parts(k, x.shape[-2:], alpha, b)
    return np.fft.ifft2(C * P * np.fft.fft2(x)).real


def backward(x, k, g, alpha, b, mutant=None):
    """-> (grad_x, grad_k in k.shape), float64.  mutant: a backward wrong in one way (MUTANTS; "flip forgotten" is chain_backward's)"""
    x, k, g = np.asarray(x, F64), np.asarray(k, F64), np.asarray(g, F64)
    H, W = x.shape[-2:]
    kh, kw = k.shape[-2:]
    K, r, C, P, dP = _parts(k, (H, W), alpha, b)
    G, Y = np.fft.fft2(g), np.fft.fft2(x)
    M = C * P
    gx = np.fft.ifft2((M if mutant == "M for conj(M)" else np.conj(M)) * G).real
    A = Y * np.conj(G)                                         # per plane; the sum over the planes sharing a kernel comes last (linear)
    if mutant != "no 1 / N":
        A = A / (H * W)
    with np.errstate(divide="ignore", invalid="ignore"):
        CK = np.where(r > 0, -np.conj(K) ** 2 / (2 * r * (r + EPS) ** 2), 0)         # (|K| at 0: autograd's subgradient 0)
    CKb = 1 / (r + EPS) - r / (2 * (r + EPS) ** 2)
    if mutant == "C constant":
        S = A * C * dP
    elif mutant == "conj term dropped":
        S = A * (CK * P + C * dP)
    else:
        S = A * (CK * P + C * dP) + np.conj(A * CKb * P)
    F = np.fft.fft2(S).real
    ry = (kh - 1) // 2 if mutant == "roll by (kh - 1) // 2" else kh // 2
    rx = (kw - 1) // 2 if mutant == "roll by (kh - 1) // 2" else kw // 2
    gk = np.roll(F, (ry, rx), axis=(-2, -1))[..., :kh, :kw]
    if k.shape[1] == 1:
        gk = gk[:, :1] if mutant == "one plane" else gk.sum(axis=1, keepdims=True)
    if k.shape[0] == 1:
        gk = gk.sum(axis=0, keepdims=True)
    return gx, gk


# ---------------------------------------------------------------------------------------------
# the chain: pad -> polynomial -> crop -> [halo masking] -> clamp
# ---------------------------------------------------------------------------------------------
def pad(x, p):
    return np.pad(np.asarray(x, F64), ((0, 0), (0, 0), (p, p), (p, p)), mode="edge")


def pad_adjoint(g, p):
    g = np.array(g, F64)
    g[..., p, :] += g[..., :p, :].sum(axis=-2)
    g[..., -p - 1, :] += g[..., -p:, :].sum(axis=-2)
    g = g[..., p:-p, :]
    g[..., :, p] += g[..., :, :p].sum(axis=-1)
    g[..., :, -p - 1] += g[..., :, -p:].sum(axis=-1)
    return g[..., :, p:-p]


def _derivative_f32_frequencies(v, axis):
    """filters.py:172-184 in float64 as the REFERENCE evaluates it there: its frequencies and their product with 2 pi are float32
    (filters.py:175-178: an integer tensor divided by an integer) whatever the image's type"""
    v = np.asarray(v, F64)
    n = v.shape[axis]
    m = (F32(2 * np.pi) * ((np.arange(n) - n // 2).astype(F32) / F32(n))).astype(F64).reshape((n, 1) if axis == -2 else (1, n))
    U = np.fft.fftshift(np.fft.fft2(v), axes=(-2, -1))
    return np.fft.ifft2(np.fft.ifftshift(m * (1j * U), axes=(-2, -1))).real


@contextlib.contextmanager
def reference_frequencies():
    """halo_grad_ref's float64 derivative with the reference's float32 frequencies, for the comparison with the reference's float64
    autograd (the goldens) alone: 2e-8 of the largest entry apart from the exact ones"""
    global _REFERENCE_FREQUENCIES
    dx, dy = hg.dx, hg.dy
    _REFERENCE_FREQUENCIES = True
    hg.dx = lambda v, dtype=F64: _derivative_f32_frequencies(v, -1) if dtype == F64 else dx(v, dtype)
    hg.dy = lambda v, dtype=F64: _derivative_f32_frequencies(v, -2) if dtype == F64 else dy(v, dtype)
    try:
        yield
    finally:
        hg.dx, hg.dy = dx, dy
        _REFERENCE_FREQUENCIES = False


_REFERENCE_FREQUENCIES = False


def chain_unclamped(x, k, alpha, b, correlate=False, remove_halo=False, grad_img=None):
    """-> (the unclamped output, the polynomial's cropped output y, (gx, gy) the mask used), float64"""
    x, k = np.asarray(x, F64), np.asarray(k, F64)
    kk = k[..., ::-1, ::-1] if correlate else k
    p = k.shape[-1] // 2
    y = forward(pad(x, p), kk, alpha, b)[..., p:-p, p:-p]
    if not remove_halo:
        return y, y, None
    gx, gy = (hg.dx(x), hg.dy(x)) if grad_img is None else (np.asarray(a, F64) for a in grad_img)
    return hg.halo_numpy(x, y, gx, gy), y, (gx, gy)


def chain_backward(x, k, w, alpha, b, correlate=False, remove_halo=False, grad_img=None, mutant=None):
    """the gradients of sum(w * clamp(chain)) -> dict x, k [, gx, gy], float64"""
    x, k = np.asarray(x, F64), np.asarray(k, F64)
    kk = k[..., ::-1, ::-1] if correlate else k
    p = k.shape[-1] // 2
    out, y, gs = chain_unclamped(x, k, alpha, b, correlate, remove_halo, grad_img)
    g = np.asarray(w, F64) * ((out > 0) & (out < 1))
    grads = {"x": np.zeros_like(x)}
    if remove_halo:
        hb = hg.hand_backward(x, y, gs[0], gs[1], g)
        grads["x"] = hb["x"] + (hg.fourier_backward(hb["gx"], hb["gy"]) if grad_img is None else 0)
        if grad_img is not None:
            grads["gx"], grads["gy"] = hb["gx"], hb["gy"]
        g = hb["y"]
    gp = np.pad(g, ((0, 0), (0, 0), (p, p), (p, p)))
    gxp, gk = backward(pad(x, p), kk, gp, alpha, b, mutant)
    grads["x"] = grads["x"] + pad_adjoint(gxp, p)
    grads["k"] = gk[..., ::-1, ::-1] if correlate and mutant != "flip forgotten" else gk
    return grads


def rel_error(got, want):
    """largest |got - want| relative to the largest |want|"""
    want = np.asarray(want, F64)
    return float(np.abs(np.asarray(got, F64) - want).max() / np.abs(want).max())


def weights(shape, seed):
    """upstream weights with 0.25 <= |w| < 1 and a random sign"""
    rng = np.random.default_rng(seed)
    return (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 1, shape)).astype(F32)


# ---------------------------------------------------------------------------------------------
# cases.  All sizes the polynomial sees are PADDED ones: the image of a phase_ref-style case, replicate-padded by kw // 2, is the
# domain of compute_polynomial; the chain pads for itself.
# (name, image (B,C,H,W), image seed, kernel (h,w), kernel seed, kernel batch, kernel channels, kind, (alpha, b))
# ---------------------------------------------------------------------------------------------
_EXTRA = [
    # phase_ref's direct_96x120 with another kernel: that one's spectrum falls to 3.6e-4 and the reference's own float32 tap
    # gradient is then 2.6e-5 off its float64 one, beyond what a case may cost (test_phase_autograd_cpu.py: 2e-5)
    ("direct_96x120_k8113", (1, 3, 84, 108), 8110, (9, 13), 8113, 1, 1, "dense", (2, 3)),
    ("broadcast_b2", (2, 3, 30, 34), 8150, (7, 11), 8151, 1, 1, "dense", (2, 3)),           # one kernel for two images: the sum lands in kernel.grad
]
POLY_NAMES = ["single_stage_16x24", "direct_96x120_k8113", "prime_97x101", "bluestein_rows_48x55_c1", "bluestein_cols_55x48_c4",
              "three_images_three_kernels", "one_kernel_per_plane", "k3x49", "k8x8", "streak_15x15", "alpha6_b1", "k21x5", "broadcast_b2"]
LONG = "tall_bluestein_2190x40"          # an 8192-point Bluestein core in the columns, the 1024-thread workgroup: restatement only
# the cases whose gradients the reference's autograd wrote into tests/golden/nonblind_phase_grad.npz
GOLDEN_POLY = ["single_stage_16x24", "bluestein_rows_48x55_c1", "one_kernel_per_plane", "k8x8", "alpha6_b1", "broadcast_b2"]


def case_named(name):
    for c in _EXTRA:
        if c[0] == name:
            return c
    return pr.case_named(name)[:9]


@functools.lru_cache(maxsize=None)
def poly_case(name):
    """-> dict: x the padded domain, k, w, alpha, b (float32 values), read-only"""
    c = case_named(name)
    x, k = pr.case_inputs(c)
    xp = pad(x, k.shape[-1] // 2).astype(F32)
    out = dict(x=xp, k=k, w=weights(xp.shape, c[2] + 7), alpha=c[8][0], b=c[8][1])
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def poly_want(name):
    c = poly_case(name)
    return backward(c["x"], c["k"], c["w"], c["alpha"], c["b"])


# chain cases: (name, image shape, kernel (h,w), kernel batch, (alpha, b), correlate, halo: None / "built" / "own", seed)
# The seeds were searched by tests/golden/make_golden_phase_autograd.py (chain_case(seed=None)) until the margins of chain_ok hold.
CHAIN_CASES = [
    ("chain_correlate_7x9", (1, 3, 20, 24), (7, 9), 1, (6, 1), True, None, 9700),
    ("chain_even_6x8_b2", (2, 2, 18, 22), (6, 8), 2, (2, 3), False, None, 9710),
    ("chain_halo_built", (2, 3, 20, 24), (5, 9), 1, (6, 1), False, "built", 9720),
    ("chain_halo_own", (1, 3, 20, 24), (7, 7), 1, (6, 1), False, "own", 9731),
]


def chain_inputs(case, seed):
    _, shape, kshape, kb, (alpha, b), correlate, halo, _ = case
    x = (0.3 + 0.4 * hr.image(shape, seed).astype(F64)).astype(F32) if halo != "own" else hg.blind_input(shape, seed, amp=0.3)
    k = pr.make_kernel(kshape, seed + 50, kb)
    grad_img = None
    if halo == "built":
        y = chain_unclamped(x, k, alpha, b, correlate)[0]
        gx, gy = hr.reversed_gradients(hg.dx(y), seed + 1, hr.plane_scales(shape), 0.08, np.asarray(x, F64) - y)
        band, mo = hg.kink_band(y, gx, gy)
        gy[band] = np.sqrt(1e-3 * np.abs(gx.astype(F64)) * mo)[band].astype(F32)
        grad_img = (gx, gy)
    return dict(x=x, k=k, w=weights(shape, seed + 70), grad_img=grad_img, alpha=alpha, b=b, correlate=correlate, remove_halo=halo is not None)


def chain_margins(c):
    """-> (distance of the nearest unclamped float64 output sample from 0 and 1, share of samples at or beyond them, whether the kink
    band of the mask is empty, share of samples the mask moves)"""
    out, y, gs = chain_unclamped(c["x"], c["k"], c["alpha"], c["b"], c["correlate"], c["remove_halo"], c["grad_img"])
    margin = float(np.minimum(np.abs(out), np.abs(out - 1)).min())
    clamped = float(np.mean((out <= 0) | (out >= 1)))
    band = bool(hg.kink_band(y, gs[0], gs[1])[0].any()) if c["remove_halo"] else False
    moved = float(np.mean(out != y)) if c["remove_halo"] else 0.0
    return margin, clamped, not band, moved


def chain_ok(c):
    margin, clamped, band_empty, _ = chain_margins(c)
    return margin > 1e-4 and clamped <= 0.01 and band_empty


@functools.lru_cache(maxsize=None)
def chain_case(name, seed=-1):
    """the inputs of a chain case at its recorded seed; seed None: searched from the recorded one on"""
    assert not _REFERENCE_FREQUENCIES, "the inputs of a case are built with the exact derivative: fetch the case first"
    case = [c for c in CHAIN_CASES if c[0] == name][0]
    s = case[7] if seed in (-1, None) else seed
    for _ in range(1 if seed == -1 else 400):
        c = chain_inputs(case, s)
        if seed == -1 or chain_ok(c):
            break
        s += 1
    else:
        raise RuntimeError("no seed found for %s" % name)
    c["seed"] = s
    for v in list(c.values()) + list(c["grad_img"] or ()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def chain_want(name):
    c = chain_case(name)
    return chain_backward(c["x"], c["k"], c["w"], c["alpha"], c["b"], c["correlate"], c["remove_halo"], c["grad_img"])


# ---------------------------------------------------------------------------------------------
# tolerances.  E: the reference's own float32 autograd against its float64 autograd, relative to the largest entry of the float64
# gradient, on exactly the inputs above (tests/golden/make_golden_phase_autograd.py measures it and stores every figure in
# tests/golden/nonblind_phase_grad.npz: `E`); TOL is held between 4 E and 8 E per group (tests/test_phase_autograd_cpu.py).
# ---------------------------------------------------------------------------------------------
# the largest E of the group: compute_polynomial on the padded domains (POLY_NAMES and LONG; image: tall_bluestein_2190x40, taps:
# k21x5), and the chain cases (image, grad_img: chain_halo_built, taps: chain_halo_built)
E_MAX = {"poly_x": 4.74e-7, "poly_k": 9.42e-6, "chain_x": 6.88e-7, "chain_k": 1.86e-6, "chain_g": 4.42e-6}
TOL = {"poly_x": 2.4e-6, "poly_k": 4.7e-5, "chain_x": 3.5e-6, "chain_k": 9.3e-6, "chain_g": 2.2e-5}          # 5 E
# what a case may cost (the CPU test asserts it of every case): E of the taps, E of the image
E_CAP = {"k": 2e-5, "x": 1e-6}


def golden():
    import json
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "nonblind_phase_grad.npz"))
    return d, json.loads(str(d["E"]))
