"""Halo masking (deblurring.py:173-208) in float64, inputs on which the mask has an effect far above any tolerance, a gauge that
proves it from the reference alone, and float64 mutants that are each wrong in one way.  A helper of tests/test_halo_cpu.py
(which proves the gauge and the mutants' rejection for every input set below, without a GPU) and of tests/test_gpu_halo.py.

Why: z = max(M / (nM + M), 0) with M one sample's gradient product and nM the plane's gradient energy is ~1 / (H W) on a natural
image, so on the project's other inputs the mask moves the output by less than the tolerances it is checked at.  grad_img is the
caller's: gradients that are sparse and reversed against the output's x-derivative put z anywhere in (0, 1).

    gx = -a s sign(ox) u   on ~8 % of a plane's samples, chosen where |ox| is at least the plane's median (no last bit flips a sign)
    a  = 3 median|ox| / (number of such samples): M / nM ~ 1 whatever the plane's size;  u in (0.25, 1)
    gx, gy += uniform noise of 0.02 a s (gx: times median|ox| / |ox| where that is below 1, which bounds the noise's M):
                M of either sign on every other sample, z == 0 on about half of them
    s  = 1 ... 30, another one for every plane of a call: nM ~ s^2, so another plane's nM is far off

Tolerances (issue "halo masking: tests that can tell the mask from a no-op"): four times the error of the fp32 NumPy oracle
against the float64 chain on the same inputs -- room for another summation order in nM and in the line transforms, fp32 both.
tests/test_halo_cpu.py measures them again and asserts that each constant is between four and eight times its figure."""
import functools

import numpy as np

from oracle import polyblur_ref as ref

F32, F64 = np.float32, np.float64
ALPHA, BETA = 6, 1

# measured oracle-vs-float64 error (max over the group's sets), times four, rounded up
TOL_STAGE = 7.1e-7          # pb_halo_mask sets: oracle halo_masking vs halo_f64, 1.76e-7 (the 1024 x 1028 plane)
TOL_INV = 3.3e-6            # fp32 non-blind chains (pad, [edgetaper], polynomial, mask, clamp): 8.04e-7 (taps_k29_w48_fft)
TOL_INV_HALF = 9.8e-4       # the same with the image and the output rounded to fp16: 2.442e-4 (half an fp16 step below 1)
TOL_PIPE, TOL_PIPE_HALF = 2e-5, 1e-3      # the blind pipeline keeps the project's own


# ---------------------------------------------------------------------------------------------
# the stage
# ---------------------------------------------------------------------------------------------
def spectral_dx_f64(y):
    """gout_x of filters.py:172-184 in float64: fftshift(fft2) * i 2 pi f_w, ifftshift, ifft2, real"""
    y = np.asarray(y, F64)
    w = y.shape[-1]
    U = np.fft.fftshift(np.fft.fft2(y), axes=(-2, -1))
    fw = (np.arange(w) - w // 2) / w
    return np.fft.ifft2(np.fft.ifftshift(2.0 * np.pi * fw * (1j * U), axes=(-2, -1))).real


def halo_parts(y, gx, gy):
    """(ox, M, nM) of the reference: M = -gx ox - gy gy (sic, deblurring.py:174), nM per (B,C) plane (:206)"""
    gx, gy = np.asarray(gx, F64), np.asarray(gy, F64)
    ox = spectral_dx_f64(y)
    return ox, -gx * ox - gy * gy, (gx * gx + gy * gy).sum(axis=(-2, -1), keepdims=True)


def finish(v, clamp, cur=None, smooth=None):
    if clamp:
        v = np.clip(v, 0.0, 1.0)
    if cur is not None:
        v = np.clip(np.clip(v, 0.0, 1.0) + (np.asarray(cur, F64) - np.asarray(smooth, F64)), 0.0, 1.0)
    return v


def halo_f64(x, y, gx, gy, clamp, cur=None, smooth=None, parts=False):
    """halo_masking (deblurring.py:193-208) in float64, then the final clamp (:239) and the recombination with the prefilter's
    detail layer (:84,88) where asked.  parts: also z and |nM + M| / nM (the distance from the pole of M / (nM + M))"""
    x, y = np.asarray(x, F64), np.asarray(y, F64)
    _, M, nM = halo_parts(y, gx, gy)
    z = np.maximum(M / (nM + M), 0.0)
    out = finish(y + z * (x - y), clamp, cur, smooth)
    return (out, z, np.abs(nM + M) / nM) if parts else out


def power(want, unmasked, tol, z, pole, factor=50):
    """What a comparison at `tol` can see on these inputs, from the reference alone; every test asserts it before it compares.
    -> None, or a string that says which condition fails"""
    want, unmasked = np.asarray(want, F64), np.asarray(unmasked, F64)
    moved = (np.abs(want - unmasked) >= factor * tol).reshape(-1, want.shape[-2] * want.shape[-1]).mean(axis=1)
    if moved.min() < 0.05:
        return "the mask moves %.1f %% of the samples of plane %d by %g" % (100 * moved.min(), int(moved.argmin()), factor * tol)
    if np.mean(z > 0) < 0.10 or np.mean(z == 0) < 0.10:
        return "z > 0 on %.1f %%, z == 0 on %.1f %%" % (100 * np.mean(z > 0), 100 * np.mean(z == 0))
    if pole.min() < 0.25:
        return "|nM + M| / nM = %.3g" % pole.min()
    return None


# ---------------------------------------------------------------------------------------------
# mutants: halo_f64 wrong in one way.  Each takes the set's dict (keys below) and returns what the wrong kernel would store,
# or None where it does not apply to the set.
# ---------------------------------------------------------------------------------------------
def _mutant(s, M=None, nM=None, clip_z=True, x=None, clamp=None, inner=True, copy=False):
    x = s["xc"] if x is None else x
    y = s["y"]
    _, M0, nM0 = halo_parts(y, s["gx"], s["gy"])
    M = M0 if M is None else M
    nM = nM0 if nM is None else nM
    z = M / (nM + M)
    if clip_z:
        z = np.maximum(z, 0.0)
    v = y.copy() if copy else y + z * (x - y)
    clamp = s["clamp"] if clamp is None else clamp
    if inner:
        return finish(v, clamp, s.get("cur"), s.get("smooth"))
    if clamp:
        v = np.clip(v, 0.0, 1.0)
    return np.clip(v + (s["cur"] - s["smooth"]), 0.0, 1.0)


def _m_copy(s):
    return _mutant(s, copy=True)


def _m_gy_oy(s):
    y = s["y"]
    h = y.shape[-2]
    U = np.fft.fftshift(np.fft.fft2(y), axes=(-2, -1))
    fh = ((np.arange(h) - h // 2) / h)[:, None]
    oy = np.fft.ifft2(np.fft.ifftshift(2.0 * np.pi * fh * (1j * U), axes=(-2, -1))).real
    return _mutant(s, M=-np.asarray(s["gx"], F64) * spectral_dx_f64(y) - np.asarray(s["gy"], F64) * oy)


def _m_no_max(s):
    return _mutant(s, clip_z=False)


def _plane_nM(s):
    return halo_parts(s["y"], s["gx"], s["gy"])[2]


def _m_neighbour_nM(s):
    nM = _plane_nM(s)
    if nM.shape[0] * nM.shape[1] < 2:
        return None
    return _mutant(s, nM=np.roll(nM.reshape(-1), 1).reshape(nM.shape))


def _m_image_nM(s):
    nM = _plane_nM(s)
    if nM.shape[1] < 2:
        return None
    return _mutant(s, nM=np.broadcast_to(nM.sum(axis=1, keepdims=True), nM.shape))


def _m_ratio(s):
    _, M, nM = halo_parts(s["y"], s["gx"], s["gy"])
    z = np.maximum(M / nM, 0.0)
    return finish(s["y"] + z * (s["xc"] - s["y"]), s["clamp"], s.get("cur"), s.get("smooth"))


def _m_pitch(s):
    """x is the interior of a padded plane (after the edgetaper); the wrong kernel walks it with the pitch of the output"""
    if s.get("xp") is None:
        return None
    xp, r = s["xp"], s["r"]
    h, w = s["y"].shape[-2:]
    pp = xp.shape[-1]
    flat = xp.reshape(xp.shape[:2] + (-1,))[..., r * pp + r:]
    return _mutant(s, x=flat[..., :h * w].reshape(xp.shape[:2] + (h, w)))


def _m_no_clamp(s):
    if not s["clamp"] or s.get("cur") is not None:
        return None
    return _mutant(s, clamp=False)


def _m_no_inner_clip(s):
    if s.get("cur") is None:
        return None
    return _mutant(s, inner=False)


MUTANTS = {
    "copy of y": _m_copy,
    "gy * oy": _m_gy_oy,
    "no max(., 0)": _m_no_max,
    "nM of the neighbouring plane": _m_neighbour_nM,
    "nM of the whole image": _m_image_nM,
    "M / nM": _m_ratio,
    "x with pitch W": _m_pitch,
    "no final clamp": _m_no_clamp,
    "recombination without the inner clip": _m_no_inner_clip,
}


# ---------------------------------------------------------------------------------------------
# input builders
# ---------------------------------------------------------------------------------------------
def plane_scales(shape, top=30.0):
    """1 ... top, one per plane, neighbours far apart (a few planes: spread over the whole range)"""
    b, c = shape[:2]
    p = b * c
    if p <= 8:
        return (top ** (np.arange(p) / max(p - 1, 1))).reshape(b, c, 1, 1)
    return (top ** ((np.arange(p) * 0.381966) % 1.0)).reshape(b, c, 1, 1)           # (golden-ratio steps: neighbours never close)


def reversed_gradients(ox, seed, scales=None, fraction=0.08, diff=None, gain=1.0, others=()):
    """(gx, gy) float32 for an output whose float64 x-derivative is ox (B,C,H,W): see the head of this file.
    diff: |x - y|; the reversed samples are then drawn where it, too, is at least its median (gain 1), or are the samples of
    the largest |x - y| (gain < 1: a = 3 gain median|ox| / count, M / nM ~ 1 / gain, z close to 1 -- what fp16 images need).
    others: the x-derivatives of further outputs the same planes are to serve (one golden pair for four variants of the chain):
    reversed samples only where all agree in sign and none is below the median, noise bounded by the largest of them"""
    ox = np.asarray(ox, F64)
    b, c, h, w = ox.shape
    p, n = b * c, h * w
    rng = np.random.default_rng(seed)
    a = np.abs(ox).reshape(p, n)
    med = np.median(a, axis=1, keepdims=True)
    nsp = max(1, int(round(fraction * n)))
    r = rng.random((p, n))
    if diff is not None:
        d = np.abs(np.asarray(diff, F64)).reshape(p, n)
        if gain < 1.0:
            r = 1.0 - d / (d.max() + 1.0)
        else:
            r[d < np.median(d, axis=1, keepdims=True)] = 2.0
    big = a
    for o in others:
        o = np.asarray(o, F64).reshape(p, n)
        r[(np.sign(o) != np.sign(ox.reshape(p, n))) | (np.abs(o) < med)] = 2.0
        big = np.maximum(big, np.abs(o))
    r[a < med] = 2.0                                          # never chosen: at least a quarter of the plane stays
    idx = np.argpartition(r, nsp - 1, axis=1)[:, :nsp]
    amp = 3.0 * gain * med / nsp
    s = (np.ones((p, 1)) if scales is None else np.asarray(scales, F64).reshape(p, 1)) * amp
    u = rng.uniform(0.25, 1.0, (p, nsp))
    gx = np.zeros((p, n))
    np.put_along_axis(gx, idx, -np.sign(np.take_along_axis(ox.reshape(p, n), idx, axis=1)) * u, axis=1)
    damp = med / np.maximum(big, med)                           # (|noise ox| <= 0.02 a s median|ox|: no sample near the pole)
    gx = s * (gx + 0.02 * damp * rng.uniform(-1.0, 1.0, (p, n)))
    gy = s * 0.02 * rng.uniform(-1.0, 1.0, (p, n))
    return gx.reshape(ox.shape).astype(F32), gy.reshape(ox.shape).astype(F32)


# the shapes of the stage's sets (Engine.halo_mask -> pb_halo_mask, fp32, no clamp) and what each reaches
STAGE_SHAPES = [
    (1, 3, 32, 48),         # four samples per lane
    (2, 3, 33, 50),         # scalar, several planes of different energies
    (1, 2, 34, 50),         # H W % 4 == 0, W % 4 != 0: the energy sum vectorised, the mask scalar
    (1, 1, 2, 4), (1, 1, 2, 3),     # the smallest planes of either form
    (1, 1, 8, 9),           # small, ragged
    (1, 1, 96, 128),        # more than one block per plane in the energy sum
    (1, 1, 520, 512),       # more than 64 partial sums per plane: the fold kernel's second trip
    (1, 1, 1024, 1028),     # the cap of 256 blocks per plane
    (16385, 4, 2, 4),       # 65 540 planes: the plane loop above the cap of gridDim.y
]


def shape_id(shape):
    return "x".join(str(v) for v in shape)


@functools.lru_cache(maxsize=None)
def stage_set(shape):
    """random x, y in (0, 1), at least 0.1 apart, and built gradients; everything a test or a mutant needs, float64 where it is a reference"""
    seed = 9000 + sum(v * m for v, m in zip(shape, (1, 7, 131, 1009)))
    rng = np.random.default_rng(seed)
    x = rng.random(shape, dtype=F32)
    y = ((x + F32(0.1) + F32(0.8) * rng.random(shape, dtype=F32)) % F32(1)).astype(F32)     # |x - y| >= 0.1 on every sample
    gx, gy = reversed_gradients(spectral_dx_f64(y), seed + 1, plane_scales(shape))
    want, z, pole = halo_f64(x, y, gx, gy, False, parts=True)
    s = dict(x=x, xc=x.astype(F64), y=y.astype(F64), y32=y, gx=gx, gy=gy, clamp=False, want=want, unmasked=y.astype(F64), z=z,
             pole=pole, xp=None, r=0)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


# ---------------------------------------------------------------------------------------------
# the non-blind chain in float64 (deblurring.py:211-239), one kernel per image
# ---------------------------------------------------------------------------------------------
def _otf64(k, shape):
    kh, kw = k.shape[-2:]
    big = np.zeros(k.shape[:-2] + tuple(shape))
    big[..., :kh, :kw] = k
    return np.fft.fft2(np.roll(big, (-(kh // 2), -(kw // 2)), axis=(-2, -1)))


def _apply64(x, k, method):
    """filters.py:14-49: 'fft' a circular convolution over the domain, 'direct' a zero-padded 'same' correlation"""
    if method == "fft":
        return np.fft.ifft2(np.fft.fft2(x) * _otf64(k, x.shape[-2:])).real
    kh, kw = k.shape[-2:]
    h, w = x.shape[-2:]
    ty, tx = (kh - 1) // 2, (kw - 1) // 2
    xp = np.pad(x, [(0, 0), (0, 0), (ty, kh - 1 - ty), (tx, kw - 1 - tx)])
    out = np.zeros_like(x)
    for i in range(kh):
        for j in range(kw):
            out += k[:, :, i:i + 1, j:j + 1] * xp[:, :, i:i + h, j:j + w]
    return out


def _taper_weight64(proj, n):
    z = np.fft.ifft(np.abs(np.fft.fft(proj, n - 1, axis=-1)) ** 2, axis=-1).real        # edgetaper.py:11-15
    z = np.concatenate([z, z[..., :1]], axis=-1)
    return 1.0 - z / z.max(axis=-1, keepdims=True)


def chain_f64(x, k, taper, method, phase=False, alpha=ALPHA, b=BETA):
    """pad -> [edgetaper] -> polynomial -> crop, float64: (the padded plane the mask's x is cropped from, its crop, y unclamped)"""
    x, k = np.asarray(x, F64), np.asarray(k, F64)
    k = np.broadcast_to(k, (x.shape[0],) + k.shape[1:])
    r = k.shape[-1] // 2
    xp = ref.replicate_pad(x, r)
    if taper:
        wgt = _taper_weight64(k.sum(axis=-1), xp.shape[-2])[..., :, None] * _taper_weight64(k.sum(axis=-2), xp.shape[-1])[..., None, :]
        for _ in range(3):
            xp = wgt * xp + (1.0 - wgt) * _apply64(xp, k, method)
    a3, a2, a1 = alpha / 2 - b + 2, 3 * b - alpha - 6, 5 - 3 * b + alpha / 2
    if method == "fft":
        Y, K = np.fft.fft2(xp), _otf64(k, xp.shape[-2:])
        if phase:
            Y = np.conj(K) / (np.abs(K) + 1e-8) * Y
        t = np.fft.ifft2(((a3 * K + a2) * K + a1) * K * Y + b * Y).real
    else:
        t = a3 * xp
        t = _apply64(t, k, method) + a2 * xp
        t = _apply64(t, k, method) + a1 * xp
        t = _apply64(t, k, method) + b * xp
    return xp, ref.crop(xp, r), ref.crop(t, r), r


def make_kernel(shape, seed, batch=1):
    """dense and not point-symmetric (rng.random ** 3, normalised), one per image"""
    k = np.random.default_rng(seed).random((batch, 1) + tuple(shape)) ** 3
    return (k / k.sum(axis=(-2, -1), keepdims=True)).astype(F32)


def image(shape, seed, half=False):
    """fp32: a synthetic blurry image with 1 % of its samples at 0 and 1 % at 1 (the final clamp acts on a few samples of
    every set, whatever the kernel).  fp16: white noise in
    (0.15, 0.85) -- neighbours far apart, so that the polynomial moves many samples by many fp16 steps"""
    if half:
        return (0.15 + 0.7 * np.random.default_rng(seed).random(shape)).astype(np.float16)
    from polyblur_amd.synthetic import synthetic_blurry_batch
    x = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=seed)[0]
    r = np.random.default_rng(seed + 7).random(shape)
    x[r < 0.01], x[r > 0.99] = 0.0, 1.0
    return x


def gaussian_kernel(shape, seed, batch=1):
    """an anisotropic Gaussian of another size and angle per image plus 10 % of make_kernel: not point-symmetric, and a
    spectrum that spans (0, 1) over the image's band (the polynomial's gain reaches 1.8)"""
    from polyblur_amd.synthetic import gaussian_psf
    assert shape[0] == shape[1]
    g = np.stack([gaussian_psf(1.4 + 0.4 * i, 0.9 + 0.2 * i, 30.0 + 50.0 * i, shape[0]) for i in range(batch)])[:, None]
    return (0.9 * g + 0.1 * make_kernel(shape, seed, batch)).astype(F32)


# (name, entry, image shape, kernel (h, w), method, edgetaper, fp16 image, own gradients)
# entry: "info" Engine.inverse_filter (25 x 25 records), "taps" inverse_filter_taps, "phase" inverse_filter_phase_taps,
#        "rank3" / "nonsym": the Python API
A, B_ = (1, 3, 32, 48), (2, 1, 33, 50)
INVERSE_CASES = [(("info_%s_%s_%s" % (shape_id(sh), m, "taper" if t else "plain")), "info", sh, (25, 25), m, t, False, False)
                 for sh in (A, B_) for m in ("fft", "direct") for t in (False, True)]
INVERSE_CASES += [
    # the interior of a padded plane: pad 13 -> a pitch of W + 26; pad 14 -> the first sample 14 (pitch + 1) samples in
    ("taps_k27_w48_fft", "taps", A, (27, 27), "fft", True, False, False),
    ("taps_k27_w48_direct", "taps", A, (27, 27), "direct", True, False, False),
    ("taps_k29_w48_fft", "taps", A, (29, 29), "fft", True, False, False),
    ("taps_k29_w48_direct", "taps", A, (29, 29), "direct", True, False, False),
    ("taps_k29_w50_fft", "taps", B_, (29, 29), "fft", True, False, False),
    ("phase_k9x13_w48", "phase", A, (9, 13), "fft", True, False, False),
    ("phase_k9x13_w50_plain", "phase", B_, (9, 13), "fft", False, False, False),
    ("rank3_w50_direct", "rank3", (2, 3, 33, 50), (11, 14), "direct", True, False, False),
    ("rank3_w48_fft", "rank3", A, (25, 25), "fft", True, False, False),
    ("nonsym_w48", "nonsym", A, (7, 11), "fft", True, False, False),
]
HALF_CASES = [
    ("half_taps_w48_taper", "taps", A, (25, 25), "fft", True, True, False),
    ("half_taps_w48_plain", "taps", A, (25, 25), "direct", False, True, False),
    ("half_taps_w50_taper", "taps", B_, (25, 25), "direct", True, True, False),
    ("half_taps_w50_plain", "taps", B_, (25, 25), "fft", False, True, False),
    ("half_rank3_w48", "rank3", A, (11, 11), "fft", True, True, False),
    ("half_nonsym_w50", "nonsym", (2, 3, 33, 50), (9, 9), "fft", True, True, False),
]
# grad0 = None: the gradients of the image the mask blends with.  At these sizes z ~ 1 / (H W) may reach the gauge.
OWN_CASES = [
    ("own_8x9", "taps", (1, 1, 8, 9), (5, 5), "fft", False, False, True),
    ("own_12x16", "taps", (1, 3, 12, 16), (5, 5), "fft", True, False, True),
]


def case_named(name):
    return [c for c in INVERSE_CASES + HALF_CASES + OWN_CASES if c[0] == name][0]


@functools.lru_cache(maxsize=None)
def inverse_set(name):
    """the inputs of a non-blind case, its float64 references (masked: want; not masked: unmasked) and the mutants' operands"""
    _, entry, shape, kshape, method, taper, half, own = case_named(name)
    seed = 9500 + sum(ord(ch) * (i + 1) for i, ch in enumerate(name))
    x = image(shape, seed, half)
    k = gaussian_kernel(kshape, seed + 50, shape[0]) if half and kshape[0] == kshape[1] else make_kernel(kshape, seed + 50, shape[0])
    xp, xc, y, r = chain_f64(x, k, taper, method, phase=entry in ("phase", "nonsym"))
    if own:                                                   # fourier_gradients of the crop (deblurring.py:200-201,237)
        h = xc.shape[-2]
        U = np.fft.fftshift(np.fft.fft2(xc), axes=(-2, -1))
        fh = ((np.arange(h) - h // 2) / h)[:, None]
        gx = spectral_dx_f64(xc)
        gy = np.fft.ifft2(np.fft.ifftshift(2.0 * np.pi * fh * (1j * U), axes=(-2, -1))).real
    elif half:                                                # (z close to 1 where |x - y| is largest; energies 1 ... 9)
        gx, gy = reversed_gradients(spectral_dx_f64(y), seed + 1, plane_scales(shape, 3.0), 0.12, xc - y, 0.1)
    else:
        gx, gy = reversed_gradients(spectral_dx_f64(y), seed + 1, plane_scales(shape), 0.08, xc - y)
    want, z, pole = halo_f64(xc, y, gx, gy, True, parts=True)
    s = dict(x=x, k=k, xc=xc, y=y, gx=gx, gy=gy, clamp=True, want=want, unmasked=np.clip(y, 0.0, 1.0), z=z, pole=pole,
             xp=xp if taper else None, r=r, method=method, taper=taper, entry=entry, own=own)
    for v in s.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return s


# ---------------------------------------------------------------------------------------------
# what tests/golden/make_golden_halo.py hands to the reference itself (tests/golden/halo_strong.npz)
# ---------------------------------------------------------------------------------------------
GOLDEN_SHAPES = [(2, 3, 33, 50), (1, 3, 32, 48)]
GOLDEN_VARIANTS = [(m, t) for m in ("fft", "direct") for t in (False, True)]


@functools.lru_cache(maxsize=None)
def golden_inverse_inputs(shape):
    """an image, one 13 x 13 kernel per image and ONE pair of gradient planes for the four variants of the chain (built on the
    output of 'fft' without the edgetaper with a look at the other three; the script asserts the gauge for all four)"""
    seed = 9700 + shape[-1]
    x = image(shape, seed)
    k = make_kernel((13, 13), seed + 50, shape[0])
    _, xc, y, _ = chain_f64(x, k, False, "fft")
    others = [spectral_dx_f64(chain_f64(x, k, t, m)[2]) for m, t in GOLDEN_VARIANTS[1:]]
    gx, gy = reversed_gradients(spectral_dx_f64(y), seed + 1, plane_scales(shape), 0.08, xc - y, others=others)
    return x, k, gx, gy


def oracle_inverse(s):
    """the fp32 NumPy oracle on a non-blind set (the tolerance's yardstick)"""
    x = np.asarray(s["x"], F32)
    k = np.broadcast_to(s["k"], (x.shape[0],) + s["k"].shape[1:])
    grad = None if s["own"] else (s["gx"], s["gy"])
    if s["entry"] in ("phase", "nonsym"):
        import phase_ref
        return phase_ref.inverse_filtering_nonsymmetric(x, k, ALPHA, BETA, remove_halo=True, do_edgetaper=s["taper"], grad_img=grad)
    return ref.inverse_filtering_rank3(x, k, ALPHA, BETA, remove_halo=True, do_edgetaper=s["taper"], grad_img=grad, method=s["method"])


# ---------------------------------------------------------------------------------------------
# the fused recombination (cur != nullptr in halo_kernel): reachable through the blind pipeline only, which always asks for the
# final clamp first -- there the inner clip is the identity and its mutant computes the same.  The float64 arithmetic is checked
# against that mutant on the CPU without the final clamp, where the two differ
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recombined_set():
    s = dict(stage_set((2, 3, 33, 50)))
    rng = np.random.default_rng(9900)
    s["cur"] = rng.random(s["x"].shape)
    s["smooth"] = np.clip(s["cur"] + 0.1 * rng.standard_normal(s["x"].shape), 0.0, 1.0)
    s["y"] = s["y"] * 1.6 - 0.3                               # (samples on either side of the inner clip)
    s["gx"], s["gy"] = reversed_gradients(spectral_dx_f64(s["y"]), 9901, plane_scales(s["x"].shape, 5.0), 0.12)
    s["clamp"] = False                                        # (after a final clamp the inner clip is the identity)
    s["want"], s["z"], s["pole"] = halo_f64(s["xc"], s["y"], s["gx"], s["gy"], False, s["cur"], s["smooth"], parts=True)
    s["unmasked"] = finish(s["y"], False, s["cur"], s["smooth"])
    return s


# ---------------------------------------------------------------------------------------------
# the blind pipeline (polyblur_deblurring(..., remove_halo=True)): the gradients are the image's own, so the input is found,
# not built.  z is one sample's share of the plane's gradient energy: a flat image with one sharp vertical line per plane
# (a tenth of the samples carry the energy), a slow wave across it (samples where the output's derivative keeps its sign:
# z == 0), row offsets (gy != 0), beta < 0 (the polynomial inverts the line's high frequencies: the reversal the mask looks
# for) and c = 1 (the estimator reports a wide blur although the line is sharp, so the polynomial does something).
# On (1,3,24,40) the mask then moves a tenth of every plane's samples by 20 tolerances and more, up to 1.3e-2.
# No such input exists for the fp16 case at (2,3,512,640): its tolerance of 1e-3 asks for z |x - y| >= 0.02 on 16 384 samples
# of a plane, and the z of a plane sum to about |beta| at most.
# ---------------------------------------------------------------------------------------------
PIPE_KW = dict(n_iter=1, c=1.0, b=0.468, alpha=6, beta=-3, remove_halo=True)
PIPE_SHAPE = (1, 3, 24, 40)


def pipeline_image(shape=PIPE_SHAPE, seed=9800, amp=0.3, wave=0.1, rows=0.03):
    rng = np.random.default_rng(seed)
    b, c, h, w = shape
    x = np.full(shape, 0.5, F32)
    x += (wave * np.sin(2 * np.pi * (np.arange(w) / w + 0.13)))[None, None, None, :].astype(F32)
    x += (rows * rng.standard_normal((b, c, h, 1))).astype(F32)
    for bi in range(b):
        for ci in range(c):
            x[bi, ci, :, rng.integers(4, w - 4)] += amp * rng.choice([-1, 1])
    return np.clip(x, 0, 1).astype(F32)


def _spectral_dy_f64(x):
    h = x.shape[-2]
    U = np.fft.fftshift(np.fft.fft2(np.asarray(x, F64)), axes=(-2, -1))
    fh = ((np.arange(h) - h // 2) / h)[:, None]
    return np.fft.ifft2(np.fft.ifftshift(2.0 * np.pi * fh * (1j * U), axes=(-2, -1))).real


@functools.lru_cache(maxsize=None)
def pipeline_set(prefiltering):
    """one iteration of the blind call: the oracle's answer (what the GPU is compared with, at the project's tolerance), and
    the float64 mask on the oracle's kernel estimate (what the gauge and the mutants are computed from)"""
    x = pipeline_image()
    oracle_out, infos = ref.polyblur_deblurring(x, prefiltering=prefiltering, return_info=True, **PIPE_KW)
    kernel = infos[0]["kernel"][:, None]
    src, cur, smooth = x, None, None
    if prefiltering:
        smooth, _ = ref.edge_aware_filtering(x, 2.0, 0.8, "bilateral")
        src, cur = smooth, x.astype(F64)
        smooth = smooth.astype(F64)
    _, xc, y, r = chain_f64(src, kernel, False, "fft", alpha=PIPE_KW["alpha"], b=PIPE_KW["beta"])
    gx, gy = spectral_dx_f64(x), _spectral_dy_f64(x)
    want, z, pole = halo_f64(xc, y, gx, gy, True, cur, smooth, parts=True)
    return dict(x=x, oracle=oracle_out, theta=[float(i["theta"][0]) for i in infos], xc=xc, y=y, gx=gx, gy=gy, clamp=True, cur=cur,
                smooth=smooth, want=want, unmasked=finish(y, True, cur, smooth), z=z, pole=pole, xp=None, r=r)
