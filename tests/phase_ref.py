"""A local restatement of the reference's compute_polynomial_fft with the pure-phase filter (deblurring.py:141-169,
not_symmetric=True) in NumPy, complex64 (the reference's arithmetic) or complex128 (the conditioning check), and the non-blind
chain around it from the oracle's own pad / edgetaper / crop / halo masking.  A helper of tests/test_phase_cpu.py and
tests/test_gpu_phase.py; tests/test_phase_cpu.py pins it to the reference's outputs (tests/golden/nonblind_phase.npz)."""
import numpy as np

from oracle import polyblur_ref as ref

F32 = np.float32


def make_kernel(shape, seed, batch=1, channels=1):
    k = np.random.default_rng(seed).random((batch, channels) + tuple(shape)) ** 3
    return (k / k.sum(axis=(-2, -1), keepdims=True)).astype(np.float32)


def streak_kernel(shape, seed):
    """a motion streak: a few random taps along a slanted line on a faint dense floor (no zero of the spectrum)"""
    h, w = shape
    rng = np.random.default_rng(seed)
    k = 0.02 * rng.random((h, w)) / (h * w)
    n = max(h, w)
    for t in range(n):
        k[min(h - 1, t * h // n), min(w - 1, (t * w // n + t % 2) % w)] += rng.random() ** 2 / n
    return (k / k.sum()).astype(np.float32)[None, None]


def otf(kernel, shape, double):
    k = np.asarray(kernel, np.float64 if double else F32)
    kh, kw = k.shape[-2:]
    big = np.zeros(k.shape[:-2] + tuple(shape), k.dtype)
    big[..., :kh, :kw] = k
    big = np.roll(big, (-(kh // 2), -(kw // 2)), axis=(-2, -1))
    return np.fft.fft2(big).astype(np.complex128 if double else np.complex64)


def compute_polynomial_fft(x, kernel, alpha, b, not_symmetric=True, double=False):
    """x: (B,C,H,W), the whole domain; kernel: (B or 1, C or 1, h, w).  Unclamped."""
    real, cplx = (np.float64, np.complex128) if double else (F32, np.complex64)
    Y = np.fft.fft2(np.asarray(x, real)).astype(cplx)
    K = otf(kernel, x.shape[-2:], double)
    if not_symmetric:
        Y = ((np.conj(K) / (np.abs(K) + real(1e-8))).astype(cplx) * Y).astype(cplx)
    a3, a2, a1 = alpha / 2 - b + 2, 3 * b - alpha - 6, 5 - 3 * b + alpha / 2
    X = real(a3) * Y
    X = K * X + real(a2) * Y
    X = K * X + real(a1) * Y
    X = K * X + real(b) * Y
    return np.fft.ifft2(X.astype(cplx)).real.astype(real)


def _one(x, k, alpha, b, remove_halo, do_edgetaper, grad_img, double):
    r = k.shape[-1] // 2
    xp = ref.replicate_pad(np.asarray(x, F32), r)
    if do_edgetaper:
        xp = ref.edgetaper(xp, k, method="fft")
    y = ref.crop(compute_polynomial_fft(xp, k, alpha, b, True, double), r)
    if remove_halo:
        y = ref.halo_masking(ref.crop(xp, r), y.astype(F32), grad_img)
    return np.clip(y, 0, 1).astype(np.float64 if double else F32)


def inverse_filtering_nonsymmetric(x, kernel, alpha=2, b=4, correlate=False, remove_halo=False, do_edgetaper=False,
                                   grad_img=None, double=False):
    """the chain, image by image (and channel by channel where the kernel has one plane per channel: the edgetaper's weights
    are normalised per plane, as in the engine)"""
    x = np.asarray(x, F32)
    k = np.asarray(kernel, F32)
    if correlate:
        k = k[..., ::-1, ::-1]
    k = np.broadcast_to(k, (x.shape[0],) + k.shape[1:])
    out = np.empty(x.shape, np.float64 if double else F32)
    for i in range(x.shape[0]):
        g = None if grad_img is None else tuple(np.asarray(gp)[i:i + 1] for gp in grad_img)
        if k.shape[1] == 1:
            out[i:i + 1] = _one(x[i:i + 1], k[i:i + 1], alpha, b, remove_halo, do_edgetaper, g, double)
        else:
            for c in range(x.shape[1]):
                gc = None if g is None else tuple(gp[:, c:c + 1] for gp in g)
                out[i:i + 1, c:c + 1] = _one(x[i:i + 1, c:c + 1], k[i:i + 1, c:c + 1], alpha, b, remove_halo, do_edgetaper, gc, double)
    return out


# ---------------------------------------------------------------------------------------------
# the cases tests/test_gpu_phase.py runs against the restatement; tests/test_phase_cpu.py checks the conditioning of each
# (name, image (B,C,H,W), image seed, kernel (h,w), kernel seed, kernel batch, kernel channels, kind, (alpha, b), forms)
# forms: "plain" and / or "full" (edgetaper + halo masking; not for a kernel taller than wide)
# ---------------------------------------------------------------------------------------------
CASES = [
    ("single_stage_16x24", (1, 3, 12, 20), 8100, (5, 5), 8101, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("direct_96x120", (1, 3, 84, 108), 8110, (9, 13), 8111, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("prime_97x101", (1, 3, 85, 89), 8120, (13, 13), 8121, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("bluestein_rows_48x55_c1", (1, 1, 40, 47), 8130, (9, 9), 8131, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("bluestein_cols_55x48_c4", (1, 4, 47, 40), 8140, (9, 9), 8141, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("three_images_three_kernels", (3, 3, 30, 34), 8150, (7, 11), 8151, 3, 1, "dense", (2, 3), ("plain", "full")),
    ("one_kernel_per_plane", (2, 3, 30, 34), 8160, (9, 12), 8161, 2, 3, "dense", (2, 3), ("plain", "full")),
    ("k3x49", (1, 3, 50, 70), 8170, (3, 49), 8171, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("k49x3", (1, 3, 50, 70), 8170, (49, 3), 8172, 1, 1, "dense", (2, 3), ("plain",)),
    ("k8x8", (1, 3, 50, 70), 8170, (8, 8), 8173, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("k1x2", (1, 3, 50, 70), 8170, (1, 2), 8174, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("k48x31", (1, 3, 50, 70), 8170, (48, 31), 8175, 1, 1, "dense", (2, 3), ("plain",)),
    ("streak_15x15", (1, 3, 40, 52), 8180, (15, 15), 8181, 1, 1, "streak", (2, 3), ("plain", "full")),
    ("alpha6_b1", (1, 2, 40, 52), 8190, (11, 14), 8191, 1, 1, "dense", (6, 1), ("plain", "full")),
    ("k21x5", (1, 3, 50, 70), 8170, (21, 5), 8600, 1, 1, "dense", (2, 3), ("plain",)),
    # sides in (2048, 4096] that are not 7-smooth (2190 = 2 * 3 * 5 * 73): Bluestein cores of 8192 points -- columns two to a
    # 1024-thread workgroup with 128 KB of LDS, rows on 64 KB: what a 4K image with a 25- or 49-wide kernel runs
    ("tall_bluestein_2190x40", (1, 3, 2186, 36), 8220, (5, 5), 8221, 1, 1, "dense", (2, 3), ("plain", "full")),
    ("wide_bluestein_40x2190", (1, 1, 36, 2186), 8230, (5, 5), 8231, 1, 1, "dense", (2, 3), ("plain",)),
    ("mid_530x730", (1, 3, 500, 700), 8200, (49, 31), 8201, 1, 1, "dense", (2, 3), ("plain",)),
]
# compute_polynomial(..., not_symmetric=True) on an un-padded domain: (name, the case whose inputs it crops, (rows, columns))
POLY_CASES = [("per_plane_29x33", "one_kernel_per_plane", (29, 33))]
FP16_CASES = [("fp16_64x84", (1, 3, 50, 70), 8170, (12, 15), 8210, 1, 1, "dense", (2, 3), ("plain", "full"))]


def case_inputs(case):
    from polyblur_amd.synthetic import synthetic_blurry_batch
    _, shape, seed, kshape, kseed, kb, kc, kind = case[:8]
    x, _ = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=seed)
    x = (0.3 + 0.4 * x).astype(np.float32)
    k = streak_kernel(kshape, kseed) if kind == "streak" else make_kernel(kshape, kseed, kb, kc)
    return x, k


def case_named(name):
    return [c for c in CASES if c[0] == name][0]


def poly_inputs(pcase):
    x, k = case_inputs(case_named(pcase[1]))
    return np.ascontiguousarray(x[..., :pcase[2][0], :pcase[2][1]]), k
