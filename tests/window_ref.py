"""A float64 reference of the wrap boundary's polynomial and a float64 restatement of the composite filter's window halos
(csrc/khat.h), in NumPy; tap sets that dial any halo pair, and spectrally white inputs.  A helper of
tests/test_window_ref_cpu.py and tests/test_gpu_window_conformance.py: the cases both walk are listed at the end.

Under the wrap boundary the deconvolution is ONE circular filter a3 K^3 + a2 K^2 + a1 K + b on the replicate-padded plane
(deblurring.py:139-169, 211-239).  reference64 applies exactly that in complex128 with no rounding on the way; the project's
oracle (oracle/polyblur_ref.py) rounds to complex64 after every transform and sits up to 4.7e-7 away from it
(tests/test_window_ref_cpu.py measures and bounds that)."""
import functools

import numpy as np

PAD = 12                   # the replicate pad of the chain: the radius of a 25 x 25 kernel
KSIZE = 2 * PAD + 1
HALO_TOL = 1e-8            # csrc/khat.h: KH_HALO_TOL


def coefficients(alpha, beta):
    """(a3, a2, a1, b) of deblurring.py:133-135"""
    return alpha / 2 - beta + 2, 3 * beta - alpha - 6, 5 - 3 * beta + alpha / 2, beta


def reference64(x, taps, alpha, beta, domain=False):
    """x: (B, C, H, W); taps: (B, kh, kw), one kernel per image.  The filter a3 K^3 + a2 K^2 + a1 K + b, K placed as psf_to_otf
    places it (filters.py:255-273), applied circularly to the plane replicate-padded by 12 and cropped -- or, domain=True, to
    the plane as given (compute_polynomial).  float64 / complex128 throughout; unclamped."""
    x = np.asarray(x, np.float64)
    k = np.asarray(taps, np.float64)
    assert x.ndim == 4 and k.ndim == 3 and k.shape[0] == x.shape[0], (x.shape, k.shape)
    xp = x if domain else np.pad(x, [(0, 0), (0, 0), (PAD, PAD), (PAD, PAD)], mode="edge")
    kh, kw = k.shape[-2:]
    big = np.zeros((k.shape[0], 1) + xp.shape[-2:], np.float64)
    assert kh <= big.shape[-2] and kw <= big.shape[-1], "the kernel's box must fit the domain"
    big[:, 0, :kh, :kw] = k
    K = np.fft.fft2(np.roll(big, (-(kh // 2), -(kw // 2)), axis=(-2, -1)))
    a3, a2, a1, b = coefficients(alpha, beta)
    y = np.fft.ifft2((((a3 * K + a2) * K + a1) * K + b) * np.fft.fft2(xp)).real
    return y if domain else y[..., PAD:-PAD, PAD:-PAD]


def _tails(m, n):
    """tail[r] = sum of m[i] over |i - n| > r, r = 0 .. n, for the 2 n + 1 values m"""
    o = np.abs(np.arange(2 * n + 1) - n)
    return np.array([m[o > r].sum() for r in range(n + 1)])


def composite_halos(taps, alpha, beta):
    """-> ((hx, hy), ((inside_x, at_x), (inside_y, at_y))): the window halos csrc/khat.h gives the one-pass filter of these taps.
    Per axis: m = the marginal of |taps| over the other axis, |a3| m*m*m + |a2| m*m + |a1| m (1-D convolution powers) bounds the
    composite's marginal, the halo is the smallest radius whose outside mass is < 1e-8 -- x rounded up to a multiple of 4 (at
    least 4), y to even (at least 2).  inside / at: the outside mass at the radius before the chosen one and at the chosen one,
    in units of 1e-8 (inside is inf for radius 0): how far an fp32 sum may stray before it chooses otherwise."""
    k = np.abs(np.asarray(taps, np.float64))
    assert k.ndim == 2 and k.shape[0] % 2 == 1 and k.shape[1] % 2 == 1, k.shape
    a3, a2, a1, _ = coefficients(alpha, beta)
    radii, margins = [], []
    for m in (k.sum(axis=0), k.sum(axis=1)):            # x: over the rows; y: over the columns
        n = m.size // 2
        m2 = np.convolve(m, m)
        m3 = np.convolve(m2, m)
        c = abs(a3) * m3
        c[n:n + m2.size] += abs(a2) * m2
        c[2 * n:2 * n + m.size] += abs(a1) * m
        t = _tails(c, 3 * n)
        r = int(np.argmax(t < HALO_TOL))
        assert t[r] < HALO_TOL
        radii.append(r)
        margins.append((float(t[r - 1] / HALO_TOL) if r else float("inf"), float(t[r] / HALO_TOL)))
    hx = max(4, (radii[0] + 3) // 4 * 4)
    hy = max(2, (radii[1] + 1) // 2 * 2)
    return (hx, hy), tuple(margins)


SOFT = 1e-5                # the scale of a soft ring (dial_taps)


def _soft_scale(r):
    """the scale of the outermost pair of lines of a soft axis of radius r: 1e-5, grown with the cube of the 2 r - 1 lines inside
    it from r = 5 on.  (The mass just inside the composite's radius is ~ 24 s / n^3 for n lines of mass 1 / n and a ring of
    s / n: a constant 1e-5 gives 7e-8 at r = 8 and 2e-8 at r = 12, too close to 1e-8 for the margin below; the mass at the radius,
    ~ 24 s^2 / n^3, stays below 2e-10 for every r.)"""
    return SOFT * max(1.0, (2 * r - 1) ** 3 / 400.0)


def dial_taps(rx, ry, soft, seed, alpha=6.0, beta=1.0):
    """25 x 25 point-symmetric non-negative fp32 taps summing to 1 on the box (2 ry + 1) x (2 rx + 1): random values in
    [0.2, 1], symmetrised; soft (one flag, or one per axis (x, y)): the outermost columns / rows of the box scaled by 1e-5
    (_soft_scale).  A hard axis has composite radius 3 r (2 r where a3 = 0), a soft one 3 r - 2 (2 r - 1): the ring's share of
    the outermost two radii is below the tolerance.
    Asserts its own margin under (alpha, beta): on both axes the outside mass is >= 10 x 1e-8 just inside the radius and
    <= 0.1 x 1e-8 at it, so that no fp32 evaluation of the rule can choose another radius."""
    sx, sy = (soft, soft) if isinstance(soft, (bool, np.bool_)) else soft
    assert 0 <= rx <= PAD and 0 <= ry <= PAD and not (sx and rx < 2) and not (sy and ry < 2)
    rng = np.random.default_rng(seed)
    box = rng.uniform(0.2, 1.0, (2 * ry + 1, 2 * rx + 1))
    box = 0.5 * (box + box[::-1, ::-1])
    if sy:
        box[[0, -1], :] *= _soft_scale(ry)
    if sx:
        box[:, [0, -1]] *= _soft_scale(rx)
    k = np.zeros((KSIZE, KSIZE), np.float64)
    k[PAD - ry:PAD + ry + 1, PAD - rx:PAD + rx + 1] = box / box.sum()
    k = k.astype(np.float32)
    assert np.array_equal(k, k[::-1, ::-1])
    _, margins = composite_halos(k, alpha, beta)
    for inside, at in margins:
        assert inside >= 10.0 and at <= 0.1, (rx, ry, soft, seed, margins)
    return k


def flat(shape, seed):
    """0.5 + U(-0.10, 0.10) per sample: spectrally white, std 0.058 (float64; the caller rounds to the plane's type)"""
    return 0.5 + np.random.default_rng(seed).uniform(-0.10, 0.10, shape)


def impulses(shape):
    """0.5 everywhere plus 0.3 at one sample in each quadrant and at (0, 0): the output is the filter's own response"""
    x = np.full(shape, 0.5)
    H, W = shape[-2:]
    for y, xx in ((0, 0), (H // 4, W // 4), (H // 4 + 1, 3 * W // 4), (3 * H // 4, W // 4 + 1), (3 * H // 4 + 1, 3 * W // 4 + 1)):
        x[..., y, xx] += 0.3
    return x


# ---------------------------------------------------------------------------------------------
# the halo grid and the tap sets that dial it
# ---------------------------------------------------------------------------------------------
HX = tuple(range(4, 37, 4))                 # every column halo csrc/khat.h can emit
HY = tuple(range(2, 37, 2))                 # every row halo


def _dial_axis(h, quantum, least, first):
    """-> (r, soft) of the smallest box radius whose composite radius under alpha = 6, beta = 1 rounds to the halo h; hard first"""
    for soft in (False, True):
        for r in range(2 if soft else first, PAD + 1):
            raw = 3 * r - (2 if soft else 0)
            if max(least, (raw + quantum - 1) // quantum * quantum) == h:
                return r, soft
    raise ValueError("no box dials the halo %d" % h)


def dial_for(hx, hy):
    """-> (rx, ry, (soft x, soft y)) of the tap set whose composite halos under alpha = 6, beta = 1 are (hx, hy)"""
    (rx, sx), (ry, sy) = _dial_axis(hx, 4, 4, 1), _dial_axis(hy, 2, 2, 0)     # (at least three columns: no identity filter)
    return rx, ry, (sx, sy)


@functools.lru_cache(maxsize=None)
def taps_for(hx, hy):
    """the tap set of the sweeps for the halo pair (hx, hy) under alpha = 6, beta = 1, read-only"""
    rx, ry, soft = dial_for(hx, hy)
    k = dial_taps(rx, ry, soft, 1000 * hx + hy)
    k.setflags(write=False)
    return k


# ---------------------------------------------------------------------------------------------
# the three window forms and the cases of the sweeps (tests/test_gpu_window_conformance.py runs them,
# tests/test_window_ref_cpu.py checks the conditions they rest on)
# ---------------------------------------------------------------------------------------------
# csrc/common.h: PB_POLY_MIN_TX = 24, PB_POLY_MIN_TY = 16, PB_POLY_MIN_AREA = 768; PB_TALL_MAX_HY = 36, PB_TALL_MIN_AREA = 1536;
# PB_POLY128_MIN_T = 56.  (window columns, window rows, largest hx, largest hy, smallest tile area)
FORMS = {"pairs": (64, 64, 20, 24, 768), "tall": (64, 128, 20, 36, 1536), "w128": (128, 128, 36, 36, 0)}
ALPHA, BETA = 6.0, 1.0
ALPHA2, BETA2 = 2.0, 3.0


def tile(form, hx, hy):
    wx, wy = FORMS[form][:2]
    return wx - 2 * hx, wy - 2 * hy


def admits(form, hx, hy):
    _, _, mx, my, area = FORMS[form]
    tx, ty = tile(form, hx, hy)
    return hx <= mx and hy <= my and tx * ty >= area


def admitted_values(form):
    """-> (the column halos, the row halos) the form admits with some halo on the other axis"""
    return (tuple(hx for hx in HX if any(admits(form, hx, hy) for hy in HY)),
            tuple(hy for hy in HY if any(admits(form, hx, hy) for hx in HX)))


def corners(form):
    """the joint corners of the form's admitted halo pairs: smallest and largest halo on either axis, each with the smallest and
    the largest the other axis then admits"""
    xs, ys = admitted_values(form)
    out = []
    for hx in (xs[0], xs[-1]):
        col = [hy for hy in HY if admits(form, hx, hy)]
        out += [(hx, col[0]), (hx, col[-1])]
    for hy in (ys[0], ys[-1]):
        row = [hx for hx in HX if admits(form, hx, hy)]
        out += [(row[0], hy), (row[-1], hy)]
    return tuple(sorted(set(out)))


def centre(form):
    xs, ys = admitted_values(form)
    return xs[len(xs) // 2], ys[len(ys) // 2]


def _ragged(t):
    """about 2.3 tiles of side t, not a multiple of 4"""
    n = int(2.3 * t)
    return n + 1 if n % 4 == 0 else n


def sweep_shape(form, hx, hy):
    """(H, W) of a sweep case: on both axes two whole tiles of the form, a ragged third and a first window that wraps.  A halo pair
    the form does not admit gets the 128 x 128 form's shape; the 64 x 128 form is only taken from 128 rows on."""
    f = form if admits(form, hx, hy) else "w128"
    tx, ty = tile(f, hx, hy)
    H, W = _ragged(ty), _ragged(tx)
    return (max(H, 129) if form == "tall" else H), W


def sweep_cases(form, hx):
    """the cases of one sweep test: (hx, hy, (C, H, W)) for every row halo; three planes at the form's corners"""
    return [(hx, hy, ((3 if (hx, hy) in corners(form) else 1),) + sweep_shape(form, hx, hy)) for hy in HY]


def coef2_case(form, key):
    """a corner of the sweep once more under alpha = 2, beta = 3 (a3 = 0: other spectra, smaller halos) -> (the halos the same taps
    then have, the case's (C, H, W): the sweep's shape for those halos)"""
    h2, _ = composite_halos(taps_for(*key), ALPHA2, BETA2)
    return h2, (3,) + sweep_shape(form, *h2)


# geometry edges: per form its smallest halo pair and a large one (the 128 x 128 form: the smallest pairs that leave a 64 x 64
# window no tile, one per axis, since the cost model gives it nothing smaller)
EDGE_HALOS = {"pairs": ((4, 2), (16, 16)), "tall": ((4, 2), (16, 30)), "w128": ((24, 2), (32, 32))}


def edge_shapes(form, hx, hy):
    """(H, W) of the geometry sweep at one halo pair: per axis 9, T - 1, T, T + 1, 2 T - 1, 2 T + 4, 3 T + 2 (a plane smaller than
    one window, one tile exactly, an odd number of tiles -- the pair with no second window --, every W mod 4), a third of their
    product; and one shape whose second pair of the second tile row lies inside the plane on 16-byte boundaries (the loaders'
    all-16-byte path).  The 64 x 128 form keeps H >= 128: 128, 129, T + 1, 2 T - 1, 2 T + 3, 3 T + 2 from there on."""
    tx, ty = tile(form, hx, hy)
    side = lambda t: [9, t - 1, t, t + 1, 2 * t - 1, 2 * t + 4, 3 * t + 2]
    ws = side(tx)
    hs = sorted({h for h in [128, 129, ty + 1, 2 * ty - 1, 2 * ty + 3, 3 * ty + 2] if h >= 128}) if form == "tall" else side(ty)
    out = [(h, w) for j, h in enumerate(hs) for i, w in enumerate(ws) if (i + j) % 3 == 0]
    out.append((max(3 * ty + hy + 1, 129 if form == "tall" else 0), (4 * tx + hx + 3) // 4 * 4 + 4))
    return out


IMPULSE_HALOS = {"pairs": (12, 12), "tall": (12, 20), "w128": (28, 20)}
FP16_HALOS = {f: corners(f) + (centre(f),) for f in ("pairs", "w128")}
DOMAIN_HALOS = {"pairs": ((4, 4), (12, 8), (20, 16)), "w128": ((28, 6), (24, 24), (36, 36))}


# batches through the merged launch: ((B, C, H, W), the halo pair of each image's tap set) -- one image per window form; more than
# 64 records of two forms alternating
BATCHES = (((3, 3, 200, 150), ((28, 20), (8, 30), (4, 4))), ((70, 1, 72, 80), ((28, 20), (4, 4)) * 35))
BATCH_SEED = 4242


def flat_image(shape, seed, dtype=np.float32):
    x = flat(shape, seed).astype(dtype)
    x.setflags(write=False)
    return x


def all_fp32_cases():
    """every (taps key (hx, hy), (alpha, beta), input kind, (C, H, W), seed) the GPU file compares an fp32 or fp16 plane of against
    reference64 -- what tests/test_window_ref_cpu.py checks the clamp share and the oracle's distance on"""
    out = []
    for form in FORMS:
        for hx in HX:
            out += [((hx, hy), (ALPHA, BETA), "flat", shp) for hx, hy, shp in sweep_cases(form, hx)]
        for key in corners(form):
            out.append((key, (ALPHA2, BETA2), "flat", coef2_case(form, key)[1]))
        for hx, hy in EDGE_HALOS[form]:
            out += [((hx, hy), (ALPHA, BETA), "flat", (1, h, w)) for h, w in edge_shapes(form, hx, hy)]
        hx, hy = IMPULSE_HALOS[form]
        out.append(((hx, hy), (ALPHA, BETA), "impulses", (1,) + sweep_shape(form, hx, hy)))
    for form, halos in FP16_HALOS.items():
        out += [((hx, hy), (ALPHA, BETA), "flat16", (1,) + sweep_shape(form, hx, hy)) for hx, hy in halos]
    return out


def case_seed(key, shape):
    return 7 + 1000 * key[0] + 31 * key[1] + shape[-1] + 613 * shape[-2]


@functools.lru_cache(maxsize=None)
def case_input(kind, key, shape):
    """the (1, C, H, W) input of a case, read-only: fp32 (fp16 for 'flat16')"""
    if kind == "impulses":
        x = impulses((1,) + shape).astype(np.float32)
    else:
        x = flat((1,) + shape, case_seed(key, shape)).astype(np.float16 if kind == "flat16" else np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=4096)
def case_reference(kind, key, shape, coef=(ALPHA, BETA)):
    """clip(reference64) of a case, read-only"""
    y = np.clip(reference64(case_input(kind, key, shape), taps_for(*key)[None], *coef), 0.0, 1.0)
    y.setflags(write=False)
    return y
