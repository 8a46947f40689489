"""The blur estimation restated in NumPy float64 for any direction count, with inputs whose answer depends on WHERE the maximum
sits (CPU only; DESIGN.md 0, "Which tests carry the estimation's extremes").  Beside estimation_grad_ref.py, whose pieces (deriv_kernel, taps, margins, case_ok, blurred_noise)
this file uses and whose `estimate` it leaves alone.

Forward (blur_estimation.py:18-79 with the grids of deblurring.py:62-63, both truncated to whole degrees): g = channel mean,
(lo, hi) = range or the (q, 1 - q) quantiles, n = clip((g - lo) / (hi - lo)), gx / gy = the spectral derivative of n along rows /
columns (numpy.fft, float64), masked where the RAW g > 0.99, mags[k] = max |cos t_k gx - sin t_k gy|, interp = Keys' weights @
mags, i_min = the first arg-min, i_ortho by truncation, (sigma, rho) through the clamp, the taps.

Builders: seeded, analytic images that put the arg-max pixel, the range's extremes, the masked pixels, the arg-min index or the
clamp where a test wants them.  Gauges: `loss_without` (what a kernel loses that skips a region), the margins of
estimation_grad_ref.  Mutants: one-line changes of the forward (`forward(..., mutant=name)`) -- what a kernel that is subtly wrong
would compute; tests/test_estimation_ref_cpu.py proves that the cases of cases() reject each of them by 10 tolerances.
"""
import functools

import numpy as np

import estimation_grad_ref as eg

SAT = 0.99
F32 = np.float32


# ---------------------------------------------------------------------------------------------
# pieces
# ---------------------------------------------------------------------------------------------
def spectral_derivative(x, axis):
    """filters.py:159-186 along one axis, float64: multiply bin k by 2 pi i f_k, the Nyquist bin of an even length dropped"""
    x = np.asarray(x, np.float64)
    N = x.shape[axis]
    f = np.fft.fftfreq(N)
    if N % 2 == 0:
        f[N // 2] = 0.0
    shape = [1] * x.ndim
    shape[axis] = N
    return np.real(np.fft.ifft(np.fft.fft(x, axis=axis) * (2j * np.pi * f).reshape(shape), axis=axis))


def grids(n_angles, n_interp):
    """deblurring.py:62-63: both grids in whole degrees (.long())"""
    return np.linspace(0, 180, n_angles + 1).astype(np.int64), np.arange(n_interp) * (180 / n_interp) // 1


def grid_weights(n_angles, n_interp, dtype=np.float64):
    """cubic_interpolator (blur_estimation.py:138-148) on the truncated grids, both divided by n_interp (:157)"""
    th, it = grids(n_angles, n_interp)
    x, xn = th.astype(np.float64) / n_interp, np.asarray(it, np.float64) / n_interp
    t = np.abs(xn[:, None] - x[None, :])
    w = np.where(t < 1, (1.5 * t - 2.5) * t * t + 1, np.where(t < 2, ((-0.5 * t + 2.5) * t - 4) * t + 2, 0.0))
    return (w / (w.sum(axis=1, keepdims=True) + 1e-5)).astype(dtype)


def gray32(img):
    """the gray plane in float32 as the reference's mean forms it: channels summed in order, divided by C"""
    x = np.asarray(img)
    if x.dtype == np.uint8:
        x = x.astype(F32) * F32(1.0 / 255.0)
    x = x.astype(F32)
    s = x[:, 0].copy()
    for ch in range(1, x.shape[1]):
        s = s + x[:, ch]
    C = x.shape[1]
    return s if C == 1 else (s / F32(3) if C == 3 else s * F32(1.0 / C))


def quantile(flat, q):
    """torch.quantile's linear interpolation between order statistics, float64 (flat: sorted)"""
    r = q * (flat.size - 1)
    f = int(np.floor(r))
    return flat[f] + (r - f) * (flat[min(f + 1, flat.size - 1)] - flat[f])


MUTANTS = ("last_row", "unpaired_row", "first_row", "last_col", "first_col", "cols2", "cols4", "cols8", "cols16", "cols32",
           "image0", "no_mask", "mask_ge", "mask_normalised", "mask_gx_only", "plus_sin", "table7", "fold7", "default_weights",
           "last_min", "ortho_round", "no_clamp", "first_partial", "quantile_floor")


def forward(img, n_angles=6, n_interp=30, q=0.0, discard_saturation=False, c=0.362, b=0.468, ker_size=25, force_theta_deg=None,
            mutant=None):
    """every image of a (B,C,H,W) batch (float32 / float16 / uint8 values, arithmetic in float64) -> list of records.
    mutant: one of MUTANTS -- the same forward with one line changed."""
    x = np.asarray(img)
    x = x.astype(np.float64) / (255.0 if x.dtype == np.uint8 else 1.0)
    B, C, H, W = x.shape
    t = np.pi * np.arange(n_angles + 1) / n_angles
    if mutant == "table7":                                  # the 7-direction table whatever n_angles says
        t = (np.pi * np.arange(13) / 6)[:n_angles + 1]
    cs, sn = np.cos(t), np.sin(t)
    if mutant == "plus_sin":
        sn = -sn
    Wt = grid_weights(n_angles, n_interp)
    if mutant == "default_weights":                         # the cached table of the default grids read with this call's strides
        flat = np.zeros(max(n_interp * (n_angles + 1), 210))
        flat[:210] = grid_weights(6, 30).reshape(-1)
        Wt = flat[:n_interp * (n_angles + 1)].reshape(n_interp, n_angles + 1)
    step = 180 / n_interp
    out = []
    for bi in range(B):
        g = x[bi].mean(axis=0)
        flat = np.sort(g.reshape(-1))
        if q > 0:
            lo, hi = quantile(flat, float(F32(q))), quantile(flat, float(F32(1.0 - q)))
            if mutant == "quantile_floor":                  # the order statistic below the rank, no interpolation
                lo, hi = flat[int(np.floor(float(F32(q)) * (flat.size - 1)))], flat[int(np.floor(float(F32(1.0 - q)) * (flat.size - 1)))]
        else:
            lo, hi = flat[0], flat[-1]
            if mutant == "first_partial":                   # the range of the first row pair only
                lo, hi = g[:2].min(), g[:2].max()
        n = np.clip((g - lo) / (hi - lo), 0.0, 1.0)
        gx, gy = spectral_derivative(n, 1), spectral_derivative(n, 0)
        if discard_saturation and mutant != "no_mask":
            mask = g > float(F32(SAT))
            if mutant == "mask_ge":
                mask = g >= float(F32(SAT))
            if mutant == "mask_normalised":
                mask = n > float(F32(SAT))
            gx = np.where(mask, 0.0, gx)
            if mutant != "mask_gx_only":
                gy = np.where(mask, 0.0, gy)
        seen = np.ones((H, W), bool)                        # the pixels the maxima are taken over
        if mutant == "last_row":
            seen[H - 1] = False
        if mutant == "unpaired_row" and H % 2:
            seen[H - 1] = False
        if mutant == "first_row":
            seen[0] = False
        if mutant == "last_col":
            seen[:, W - 1] = False
        if mutant == "first_col":
            seen[:, 0] = False
        if mutant and mutant.startswith("cols"):            # the ragged last tile of width 2 .. 32 (all of it where W is a multiple)
            tw = int(mutant[4:])
            seen[:, (W - 1) // tw * tw:] = False
        out.append(dict(gray=g, lo=lo, hi=hi, gx=gx, gy=gy, cs=cs, sn=sn, seen=seen, shape=(C, H, W)))
    for bi, r in enumerate(out):
        src = out[0] if mutant == "image0" else r           # every image's maxima taken from image 0
        flatr = (response(src) * src["seen"][None]).reshape(n_angles + 1, -1)
        arg = flatr.argmax(axis=1)
        mags = flatr[np.arange(n_angles + 1), arg]
        flatr[np.arange(n_angles + 1), arg] = 0.0
        runner = flatr.max(axis=1)                          # the largest response at another pixel
        del flatr
        if mutant == "fold7":                               # directions k >= 7 folded as 0
            mags = np.where(np.arange(n_angles + 1) < 7, mags, 0.0)
        interp = Wt @ mags
        i_min = int(np.argmin(interp))
        if mutant == "last_min":
            i_min = int(n_interp - 1 - np.argmin(interp[::-1]))
        theta_deg = int(F32(i_min) * F32(step))
        if force_theta_deg is not None:
            theta_deg = int(force_theta_deg)
            i_min = int(F32(theta_deg) / F32(step))
        ortho = F32((theta_deg + 90) % 180) / F32(step)
        i_ortho = int(np.rint(ortho)) % n_interp if mutant == "ortho_round" else int(ortho)
        v = [c * c / (interp[i] * interp[i] + 1e-8) - b * b for i in (i_min, i_ortho)]
        vc = v if mutant == "no_clamp" else [np.clip(u, 0.09, 16.0) for u in v]
        sigma, rho = (np.sqrt(np.maximum(u, 1e-12)) for u in vc)
        theta = theta_deg * np.pi / 180
        r.update(arg=arg, mags=mags, runner=runner, interp=interp, i_min=i_min, i_ortho=i_ortho, v=v, sigma=sigma, rho=rho,
                 theta=theta, theta_deg=theta_deg, kernel=eg.taps(np.float64(theta), sigma, rho, ker_size)[0], ker_size=ker_size, c=c, b=b)
    return out


def response(r):
    """|cos t_k gx - sin t_k gy| of one record -> (n_angles + 1, H, W)"""
    return np.abs(r["cs"][:, None, None] * r["gx"][None] - r["sn"][:, None, None] * r["gy"][None])


def loss_without(recs, region):
    """what every direction's maximum loses when the pixels of `region` (an (H,W) bool array) are left out of it, relative to the
    image's largest maximum (the scale of `err`) -- per image -> (B, n_angles + 1)"""
    out = []
    for r in recs:
        resp = response(r)
        full = resp.reshape(len(resp), -1).max(axis=1)
        rest = (resp * ~region[None]).reshape(len(resp), -1).max(axis=1)
        out.append((full - rest) / full.max())
    return np.array(out)


def region(H, W, name):
    m = np.zeros((H, W), bool)
    if name == "last_row" or (name == "unpaired_row" and H % 2):
        m[H - 1] = True
    elif name == "first_row":
        m[0] = True
    elif name == "last_col":
        m[:, W - 1] = True
    elif name == "first_col":
        m[:, 0] = True
    elif name.startswith("cols"):
        tw = int(name[4:])
        m[:, (W - 1) // tw * tw:] = True
    return m


# ---------------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------------
def _background(H, W, seed, amp):
    """a smooth periodic plane of amplitude <= amp: six low harmonics with seeded phases"""
    rng = np.random.default_rng(seed)
    y, x = np.meshgrid(np.arange(H) / H, np.arange(W) / W, indexing="ij")
    f = np.zeros((H, W))
    for _ in range(6):
        ky, kx = rng.integers(0, 3, 2)
        f += np.cos(2 * np.pi * (ky * y + kx * x) + rng.uniform(0, 2 * np.pi)) * rng.uniform(0.5, 1.0)
    return amp * f / np.abs(f).max()


def _ridge(H, W, at, phi, amp, widths):
    """a short Gaussian ridge at pixel `at` = (row, column), its long axis at angle phi, on the torus"""
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    dy = (y - at[0] + H / 2) % H - H / 2
    dx = (x - at[1] + W / 2) % W - W / 2
    u, v = np.cos(phi) * dx + np.sin(phi) * dy, -np.sin(phi) * dx + np.cos(phi) * dy
    # (across the ridge one flank is 1.6 times as wide as the other: a point-symmetric ridge has two equal maxima per direction)
    return amp * np.exp(-0.5 * ((u / widths[1]) ** 2 + (v / np.where(v < 0, widths[0], 1.6 * widths[0])) ** 2))


WHERE = {"tl": lambda H, W: (0, 0), "tr": lambda H, W: (0, W - 1), "bl": lambda H, W: (H - 1, 0), "br": lambda H, W: (H - 1, W - 1),
         "last_row": lambda H, W: (H - 1, W // 2), "last_col": lambda H, W: (H // 2, W - 1), "first_row": lambda H, W: (0, W // 3),
         "first_col": lambda H, W: (H // 3, 0), "middle": lambda H, W: (H // 2, W // 2)}


def planted(B, C, H, W, where, phi=0.9, seed=1, amp=0.6, widths=(0.8, 2.5), bg=0.09, base=0.2):
    """(B,C,H,W) float32: a smooth low-contrast background and ONE short oriented ridge per image.  `where`: a name of WHERE or a
    list of names, one per image (a shorter list is cycled: the images of a batch get their ridge in different places).
    The channels are the gray plane times (0.9, 1.0, 1.1, ...) / their mean: the mean of the channels is the plane again."""
    names = [where] * B if isinstance(where, str) else [where[i % len(where)] for i in range(B)]
    imgs = []
    for bi in range(B):
        at = WHERE[names[bi]](H, W)
        g = base + bg + _background(H, W, seed + 17 * bi, bg) + _ridge(H, W, at, phi + 0.4 * bi, amp, widths)
        g[np.unravel_index(np.argmin(g), g.shape)] -= 0.004     # a smooth plane's two lowest values are closer than the range gauge allows
        gains = 1.0 + 0.1 * (np.arange(C) - (C - 1) / 2)
        imgs.append(g[None] * gains[:, None, None])
    return np.stack(imgs).astype(F32)


def extremes(B, C, H, W, lo_at, hi_at, dtype=np.float32, seed=100):
    """the gray plane's minimum at pixel lo_at and its maximum at hi_at ((row, column), negative indices from the end), every
    other pixel at least 0.05 of the range away; noise between, so that no two gradients tie.  Image bi of a batch has its own
    range (the extremes move by 0.02 bi)."""
    rng = np.random.default_rng(seed)
    g = 0.35 + 0.3 * rng.random((B, 1, H, W))
    for bi in range(B):
        g[bi, 0][lo_at] = 0.08 + 0.02 * bi
        g[bi, 0][hi_at] = 0.93 - 0.02 * bi
    x = np.repeat(g, C, axis=1)
    if dtype == np.uint8:
        return np.rint(x * 255).astype(np.uint8)
    return x.astype(dtype)


def saturated(H, W, seed=5, C=1):
    """discard_saturation: the strongest response sits on pixels whose RAW gray exceeds 0.99 -- a 2 x 2 block at 0.995 with
    one-pixel dark lines (0.05 .. 0.10) to its right and below it, mid-gray behind them: the block's corner pixel has the
    largest gx AND gy of the plane (the derivative at a pixel is the alternating sum of the differences around it, so the pixel
    in front of a thin dark line beats the line's own).  A second structure of the same shape at EXACTLY float32(0.99) -- not
    above 0.99 raw, above it once normalised by (lo, hi) = (0.05, 0.997) -- carries the next strongest response with smaller
    jumps; a weak ridge elsewhere the third.  lo > 0 and hi < 1."""
    g = 0.3 + 0.04 + _background(H, W, seed, 0.04)
    for (r, c), top, peak, right, below in (((H // 4, max(W // 4, 2)), 0.995, 0.997, (0.09, 0.05), (0.10, 0.06)),
                                            (((3 * H) // 4 - 2, (3 * W) // 4), F32(SAT), F32(SAT), (0.16, 0.12), (0.17, 0.13))):
        g[r:r + 2, c - 1:c + 1] = top
        g[r, c - 1] = peak
        g[r:r + 2, c + 1] = right
        g[r + 2, c - 1:c + 1] = below
    g = g + _ridge(H, W, (H // 2, W // 8), 0.7, 0.25, (0.9, 2.5))
    return np.repeat(g[None, None], C, axis=1).astype(F32)


def _wave(H, W, t0, freq=0.9, sharp=1.0):
    """a plane wave of direction t0 under a Gaussian window: gradients along t0, next to none across"""
    y, x = np.meshgrid(np.arange(H) - H / 2, np.arange(W) - W / 2, indexing="ij")
    u = np.cos(t0) * x - np.sin(t0) * y
    win = np.exp(-0.5 * ((x - 1.3) ** 2 + (y + 0.6) ** 2) / (min(H, W) / 5.0) ** 2)
    return (0.5 + 0.4 * win * np.cos(freq * sharp * u + 0.7))[None, None].astype(F32)     # (0.7, the offsets: no point symmetry)


def search_oriented(H, W, n_angles, n_interp):
    """theta index -> (wave direction in degrees, sharpness) of the first windowed wave -- sharpness 1.0, 0.6, 1.5, 0.8, 1.25; whole
    degrees 0 .. 179, then the half degrees -- whose estimate has that index with every margin kept.  About 1800 forwards per
    grid: what ORIENTED below was made with, not run by the tests (which check every entry of it instead)."""
    table = {}
    for sharp in (1.0, 0.6, 1.5, 0.8, 1.25):
        for t2 in list(range(0, 360, 2)) + list(range(1, 360, 2)):
            r = forward(_wave(H, W, np.deg2rad(t2 / 2.0), sharp=sharp), n_angles, n_interp)
            if r[0]["i_min"] not in table and eg.case_ok(r):
                table[r[0]["i_min"]] = (t2 / 2.0, sharp)
    return table


# search_oriented(24, 32, 6, n_interp) for the indices the tests ask for: all of 30; 0, 3, 6 of 7; 0, 1, 31, 32, 63 of 64.  It
# finds none for 1 and 29 of 30 nor for 3 of 7 (at n_interp = 7 the rows 3 and 4 both interpolate to mags[3] alone -- the nodes 77
# and 102 degrees over 7 are within one step of 90 / 7 only --, so interp[3] and interp[4] differ by their row sums' 1e-5 alone:
# a near-tie below the arg-min gauge)
ORIENTED = {30: {0: (77.0, 1.0), 2: (103.5, 1.0), 3: (104.0, 1.0), 4: (109.0, 1.0), 5: (111.0, 1.0), 6: (127.5, 1.0), 7: (133.0, 1.0),
                 8: (136.0, 1.0), 9: (139.0, 1.0), 10: (145.0, 1.0), 11: (158.0, 1.0), 12: (163.0, 1.0), 13: (166.0, 1.0),
                 14: (172.0, 1.0), 15: (0.0, 1.0), 16: (8.0, 1.0), 17: (12.0, 0.6), 18: (16.0, 1.0), 19: (18.0, 1.0), 20: (24.0, 1.0),
                 21: (38.0, 1.0), 22: (44.0, 1.0), 23: (45.0, 1.0), 24: (49.0, 1.0), 25: (53.0, 1.0), 26: (70.0, 1.0), 27: (76.0, 1.0),
                 28: (77.0, 0.6)},
            7: {0: (76.0, 1.0), 6: (45.0, 1.0)},
            64: {0: (89.0, 1.0), 1: (112.5, 1.25), 31: (175.0, 1.0), 32: (0.0, 1.0), 63: (68.0, 1.0)}}


def oriented(H, W, theta_index, n_interp):
    """the 24 x 32 windowed wave of ORIENTED whose estimate (n_angles = 6) is theta index `theta_index`"""
    t = ORIENTED[n_interp][theta_index]
    return _wave(H, W, np.deg2rad(t[0]), sharp=t[1])


def anisotropic(seed, shape, sig, contrast=1.0):
    """noise under an oblique Gaussian of stds `sig`: wide ones drive sigma / rho onto the upper clamp (4.0)"""
    return (0.5 + contrast * (eg.blurred_noise(seed, shape, sig) - 0.5)).astype(F32)


def sharp(seed, shape):
    """unblurred noise: gradients of the order of the range, sigma and rho on the lower clamp (0.3)"""
    x = 0.05 + 0.9 * np.random.default_rng(seed).random(shape)
    if x.shape[-1] * x.shape[-2] > 6:
        x[..., 1, 2], x[..., -2, 1] = 0.02, 0.98              # one lowest and one highest value (the range gauge)
    return x.astype(F32)


def tied(H, W, seed=9):
    """symmetric under x <-> -x (column j <-> column (W - j) % W): in exact arithmetic mags[k] = mags[n - k], so interp[i] =
    interp[N - i]; whether the float32 sums agree too is for the CPU test to say"""
    g = eg.blurred_noise(seed, (1, 1, H, W), (2.5, 0.8), 0.0)[0, 0].astype(np.float64)
    g = 0.5 * (g + g[:, (-np.arange(W)) % W])
    return g[None, None].astype(F32)


def quantised(H, W, levels, seed=11, dtype=np.float32, heavy=0.7):
    """values from `levels` only: a fraction `heavy` of the pixels at levels[len // 2] (one radix bin holds most of the image),
    the rest spread over the others in smooth patches -- heavy ties at every order statistic"""
    rng = np.random.default_rng(seed)
    f = _background(H, W, seed, 1.0) + 0.35 * rng.standard_normal((H, W))
    order = np.argsort(np.argsort(f.reshape(-1))).reshape(H, W) / max(H * W - 1, 1)
    lv = np.asarray(levels)
    mid = len(lv) // 2
    others = np.delete(np.arange(len(lv)), mid)
    lo_share = (1 - heavy) / 2
    idx = np.full((H, W), mid)
    below, above = others[others < mid], others[others > mid]
    for part, sel, span in ((below, order < lo_share, (0, lo_share)), (above, order > 1 - lo_share, (1 - lo_share, 1))):
        pos = np.clip(((order - span[0]) / (span[1] - span[0]) * len(part)).astype(int), 0, len(part) - 1)
        idx = np.where(sel, part[pos], idx)
    return lv[idx][None, None].astype(dtype)


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_gpu_estimation_planted.py (tests/test_estimation_ref_cpu.py proves their gauges)
# ---------------------------------------------------------------------------------------------
COLS_PLANS = (2160, 1080, 4320, 512, 640, 720, 768, 800, 960, 1024, 1200, 1280, 1440, 1536, 1600, 2048, 2560, 3072, 4096)
# height -> (lognb of the narrow tile, of the wide tile) of the plans PB_COLS_PLANS compiles a wide (1024-thread) instance for;
# 1080 never takes it (choose_cols keeps 16 columns where W % 16 == 0, the plan refuses other widths), 1200, 1280 and 2560 have none
WIDE_PLANS = {2160: (2, 3), 4320: (1, 2), 512: (3, 4), 640: (3, 4), 720: (3, 4), 768: (3, 4), 800: (3, 4), 960: (3, 4), 1024: (3, 4),
              1440: (2, 3), 1536: (2, 3), 1600: (2, 3), 2048: (2, 3), 3072: (1, 2), 4096: (1, 2)}
ANGLE_COUNTS = (1, 2, 3, 5, 7, 12)
INTERP_COUNTS = (7, 30, 64)
# n_angles = 1 has mags[0] = mags[1] (the directions 0 and pi), so interp = (w0 + w1) m: the gap of its two smallest entries is a
# property of the weights alone -- 8.6e-4 at n_interp = 64, below the 1e-3 gauge on every image
DROPPED_GRIDS = ((1, 64),)
C_STRONG = 0.8                # ... of the saturated and the quantised ones, whose jumps are of the order of the range
C0, B0 = 0.45, 0.468          # the affine model of the planted cases: both sigma and rho inside the clamp


class Case:
    """id, theme, build() -> image, the options of the call, targets = ((image, region name, direction), ...): the maxima of
    `direction` of `image` must lose 10 tolerances without `region`; engines = the contexts the GPU test runs it on"""

    def __init__(self, id, theme, build, targets=(), engines=("default",), exempt=(), **opts):
        self.id, self.theme, self.build, self.targets, self.engines, self.exempt = id, theme, build, tuple(targets), engines, exempt
        self.opts = dict(dict(n_angles=6, n_interp=30, q=0.0, discard_saturation=False, c=C0, b=B0), **opts)

    def __repr__(self):
        return self.id


_REGION_DIR = {"last_row": 0, "unpaired_row": 0, "first_row": 0, "last_col": 3, "first_col": 3}
_WHERE_TARGETS = {"last_row": ("last_row", "unpaired_row"), "first_row": ("first_row",), "last_col": ("last_col",),
                  "first_col": ("first_col",), "br": ("last_row", "last_col"), "tl": ("first_row",), "middle": ()}


def _targets(H, W, names, tile=None):
    out = []
    for bi, name in enumerate(names):
        for reg in _WHERE_TARGETS[name]:
            if reg == "unpaired_row" and H % 2 == 0:
                continue
            if name == "br" and reg == "last_col":
                continue                                   # (a corner's ridge: the row is the named target, the column comes with it)
            out.append((bi, reg, _REGION_DIR[reg]))
        if tile and name == "last_col":
            out.append((bi, "cols%d" % tile, 3))
    return tuple(out)


# the ridge's angle where the default (0.9) leaves the gap of the two smallest interpolated magnitudes below 1e-3: the first of
# (0.5, 1.3, 0.2, 1.7, ...) that keeps every margin
_PHI = {"1x1x37x75_first_row": 0.5, "1x1x37x75_first_row_sat": 0.5, "2x1x512x32_last_row+last_col": 0.2, "a2_i64_1x1x37x75_br": 1.7,
        "a2_i64_1x1x64x96_br": 1.7, "a2_i64_1x1x1080x32_br": 1.7, "a5_i30_1x1x37x75_br": 0.5, "a7_i64_1x1x37x75_br": 0.5,
        "a7_i64_1x1x64x96_br": 1.3}


# ... and the noise seed of `extremes` where 100 leaves it below: the first of 101, 102, ... that keeps every margin
_SEED = {"extremes_3x3x33x45_float32_-1.-1": 103, "extremes_2x3x34x48_float16_-1.-1": 102, "extremes_1x1x33x1920_float32_-1.1000": 101}


def _planted_case(theme, B, C, H, W, names, engines=("default",), tile=None, tag="", phi=0.9, **opts):
    names = [names] if isinstance(names, str) else list(names)
    full = [names[i % len(names)] for i in range(B)]
    cid = "%s%dx%dx%dx%d_%s%s" % (tag, B, C, H, W, "+".join(names), "_sat" if opts.get("discard_saturation") else "")
    return Case(cid, theme, functools.partial(planted, B, C, H, W, full, _PHI.get(cid, phi)), _targets(H, W, full, tile), engines, **opts)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    # -- where the maxima are taken: the run-time-plan column kernel ------------------------------------------------------------
    for H, W, tile in ((37, 75, 16), (64, 96, 16), (45, 70, 16), (16, 15, 16), (15, 16, 16), (97, 101, 16)):
        for where in ("last_row", "last_col", "first_row", "first_col", "br"):
            for sat in (False, True):
                out.append(_planted_case("where", 1, 1, H, W, where, tile=tile, discard_saturation=sat))
    out.append(_planted_case("where", 3, 3, 37, 75, ("tl", "last_col", "last_row"), tile=16))
    out.append(_planted_case("where", 3, 2, 45, 70, ("br", "first_col", "last_row"), tile=16, discard_saturation=True))
    out.append(Case("1x1x2x3_noise", "where", functools.partial(sharp, 21, (1, 1, 2, 3))))
    # -- the compiled column plans, narrow tile (and the run-time kernel at the same heights: PB_COLS_FIXED=0) --------------------
    both = ("default", "runtime_cols")
    for H in COLS_PLANS:
        out.append(_planted_case("fixed_narrow", 2, 1, H, 32, ("last_row", "last_col"), both))
        out.append(_planted_case("fixed_narrow", 2, 1, H, 32, ("first_row", "br"), both, phi=0.2, discard_saturation=True))
    # -- ... wide tile: the smallest batch and width with P * (W / (4 << lognb)) >= 200 (line_choice.h: choose_cols), the ridge in the last image's
    # last tile
    wide = ("middle", "tl", "last_row", "first_col", "middle", "first_row", "last_col", "br")
    for H, (narrow, wide_lognb) in WIDE_PLANS.items():
        W = 25 * (4 << narrow)                              # B = 8: 8 * (W / (4 << lognb)) = 200
        out.append(_planted_case("fixed_wide", 8, 1, H, W, wide, both, tile=2 << wide_lognb, phi=1.3 if W == 800 else 0.9))     # (0.9 at W = 800: arg-min gap 9.6e-4)
    # -- extended radices, through-memory columns, a fold of more than 512 tiles ---------------------------------------------------
    out.append(_planted_case("long", 1, 1, 3240, 24, "br", both))
    out.append(_planted_case("long", 1, 3, 4320, 32, "last_col", both))
    out.append(_planted_case("long", 1, 1, 8200, 10, "br"))
    out.append(_planted_case("long", 1, 1, 20736, 10, "last_row"))
    out.append(_planted_case("long", 1, 1, 8, 8200, "last_col", tile=16))
    # -- direction counts ----------------------------------------------------------------------------------------------------------
    for na in ANGLE_COUNTS:
        for ni in INTERP_COUNTS:
            if (na, ni) in DROPPED_GRIDS:
                continue
            for H, W in ((37, 75), (64, 96), (1080, 32)):
                out.append(_planted_case("angles", 1, 1, H, W, "br", tag="a%d_i%d_" % (na, ni), n_angles=na, n_interp=ni))
    # (the plan of a height with a radix above 16 -- 3240 = 9 x 15 x 24 -- is chosen by choose_cols' ext_variant: not for n_angles != 6)
    out.append(_planted_case("angles", 1, 1, 3240, 24, "br", tag="a12_i30_", n_angles=12, n_interp=30))
    out.append(_planted_case("angles", 1, 1, 4320, 32, "br", tag="a5_i64_", n_angles=5, n_interp=64))
    # -- the mask -------------------------------------------------------------------------------------------------------------------
    for H, W, eng in ((37, 75, ("default",)), (64, 96, ("default",)), (1080, 32, both), (3240, 24, both), (8200, 10, ("default",))):
        out.append(Case("saturated_%dx%d" % (H, W), "mask", functools.partial(saturated, H, W), engines=eng, discard_saturation=True, c=C_STRONG))
    # -- the range ------------------------------------------------------------------------------------------------------------------
    gray = ("default", "two_launches")
    for B, C, H, W, lo_at, hi_at, dt, eng in (
            (1, 1, 33, 45, (0, 0), (-1, -1), np.float32, gray), (1, 3, 33, 45, (-1, 23), (0, 0), np.float32, gray),
            (1, 4, 34, 48, (-2, 3), (-1, -1), np.float32, gray), (3, 3, 33, 45, (-1, -1), (-1, 5), np.float32, gray),
            (1, 1, 33, 45, (-1, -1), (0, 0), np.float16, ("default",)), (2, 3, 34, 48, (-1, -1), (-2, 7), np.float16, ("default",)),
            (1, 3, 33, 45, (-1, 11), (-1, -1), np.uint8, ("default",)), (2, 1, 34, 48, (-2, 9), (-1, -1), np.uint8, ("default",)),
            (1, 1, 33, 1920, (-1, 1000), (-1, -1), np.float32, ("default", "runtime_rows")),
            (1, 3, 33, 3840, (-1, -1), (-1, 77), np.float32, ("default", "runtime_rows"))):
        cid = "extremes_%dx%dx%dx%d_%s_%s" % (B, C, H, W, np.dtype(dt).name, "%d.%d" % lo_at)
        out.append(Case(cid, "range", functools.partial(extremes, B, C, H, W, lo_at, hi_at, dt, _SEED.get(cid, 100)), engines=eng))
    # -- the scalar chain -------------------------------------------------------------------------------------------------------------
    for ni in (30, 7, 64):
        for i in ORIENTED[ni]:
            out.append(Case("oriented_i%d_of_%d" % (i, ni), "chain", functools.partial(oriented, 24, 32, i, ni), n_interp=ni, c=0.362))
    out.append(Case("clamp_high_sigma", "chain", functools.partial(anisotropic, 117, (1, 1, 48, 64), (7.0, 6.0)), c=0.362))
    out.append(Case("clamp_high_both", "chain", functools.partial(anisotropic, 177, (1, 1, 48, 64), (9.0, 8.5)), c=0.362))
    out.append(Case("clamp_low", "chain", functools.partial(sharp, 76, (1, 1, 48, 64)), c=0.362))
    out.append(Case("clamp_none", "chain", functools.partial(anisotropic, 100, (2, 3, 48, 64), (2.2, 1.1)), c=0.362))
    out.append(Case("force_theta", "chain", functools.partial(anisotropic, 77, (1, 1, 48, 64), (2.2, 1.1)), c=0.362, force_theta_deg=132.0))
    # -- quantiles ----------------------------------------------------------------------------------------------------------------------
    for dt, levels in ((np.float32, (-0.3, -0.05, 0.1, 0.2, 0.5, 0.8, 1.0, 1.4)), (np.uint8, (3, 20, 77, 128, 200, 250, 255))):
        for H, W in ((5, 5), (5, 7), (97, 131), (160, 224)):
            for q in (1e-4, 0.02, 0.25):
                out.append(Case("quantised_%s_%dx%d_q%g" % (np.dtype(dt).name, H, W, q), "quantile",
                                functools.partial(quantised, H, W, levels, 100 if q > 0.1 else (13 if (dt, H) == (np.uint8, 97) else 11), dt,
                                                  0.4 if q > 0.1 else 0.7),
                                exempt=("amax", "gray"), q=q, c=C_STRONG))
    return tuple(out)


def golden_cases():
    """the entries of tests/golden/estimation_planted.npz (tests/golden/make_golden_estimation.py): every direction count on a
    small planted image, q and the mask cycling through {0, 1e-4, 0.02} x {off, on}; the saturated image with and without the
    mask; a quantised image -> (name, Case)"""
    out = []
    n = 0
    for na in ANGLE_COUNTS:
        for ni in INTERP_COUNTS:
            q, sat = (0.0, 1e-4, 0.02)[n % 3], (n // 3) % 2 == 1
            n += 1
            out.append(("g%02d_a%d_i%d" % (n, na, ni),
                        _planted_case("golden", 1, 1 + 2 * (n % 2), 37, 75, "br", tag="golden_a%d_i%d_" % (na, ni), phi=0.5 + 0.13 * n,
                                      n_angles=na, n_interp=ni, q=q, discard_saturation=sat)))
    for sat in (False, True):
        out.append(("saturated_%d" % sat, Case("golden_saturated_%d" % sat, "golden", functools.partial(saturated, 37, 75, 5, 3),
                                               discard_saturation=sat, c=C_STRONG)))
    out.append(("quantised", Case("golden_quantised", "golden", functools.partial(quantised, 97, 131, (-0.3, -0.05, 0.1, 0.2, 0.5, 0.8, 1.0, 1.4)),
                                  q=0.02, c=C_STRONG)))
    return out


@functools.lru_cache(maxsize=None)
def image(case):
    x = case.build()
    x.setflags(write=False)
    return x


def gauges(case, recs=None):
    """estimation_grad_ref.margins of a case -> (arg-max gap, gray-range gap, arg-min gap, clamp distance, exact_tie).  exact_tie:
    the two smallest interpolated magnitudes are both exactly 0 because their rows of weights are all zero (sparse grids: no node
    within two steps) -- zeros in any arithmetic, a tie the FIRST index must win, which is what the issue's `tied` case was for: the
    arg-min gap is exempt (inf).  theta, i_min and sigma (4.0: interp[i_min] == 0) of such a case are fixed by the grid alone;
    its mags, interp and rho carry what depends on the image, and the clamp distance (of rho: sigma^2 is far beyond 16) is kept."""
    recs = run(case) if recs is None else recs
    o = case.opts
    dead = np.flatnonzero(~grid_weights(o["n_angles"], o["n_interp"]).any(axis=1))
    tie = all(r["i_min"] in dead for r in recs) and len(dead) > 1 and o.get("force_theta_deg") is None
    with np.errstate(invalid="ignore", divide="ignore"):       # (the arg-min gap of margins() divides by the smallest entry)
        m = eg.margins(recs)
    return m[:2] + (np.inf, m[3], True) if tie else m[:4] + (False,)


def gauges_ok(case, recs=None):
    m = gauges(case, recs)
    return (m[0] >= 1e-3 or "amax" in case.exempt) and (m[1] >= 1e-3 or "gray" in case.exempt) and m[2] >= 1e-3 and m[3] >= 1e-2


def run(case, mutant=None, **over):
    """the float64 forward of a case (a mutant's, or with options replaced)"""
    o = dict(case.opts, **over)
    return forward(image(case), o["n_angles"], o["n_interp"], o["q"], o["discard_saturation"], o["c"], o["b"],
                   force_theta_deg=o.get("force_theta_deg"), mutant=mutant)


def err(got, want, field):
    """the tests' error measures: mags / interp relative to the image's largest maximum, sigma / rho / kernel absolute"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    if field in ("mags", "interp"):
        return float(np.abs(got - want).max() / np.abs(want).max())
    return float(np.abs(got - want).max())


# 4 x the float32 oracle's largest error against `forward` over cases() (measured again by
# tests/test_estimation_ref_cpu.py::test_tolerances_are_four_times_the_oracles_error, which holds these constants to it)
TOL = {"mags": 3.0e-6, "interp": 3.3e-6, "sigma": 1.9e-5, "rho": 1.9e-5}
TOL_KERNEL = 1e-5                  # tests/test_gpu_parity.py::test_estimate_blur
# |float64 forward - tests/golden/estimation_planted.npz|: 4 x the largest measured (sigma 3.41e-5, rho 1.03e-5, kernel 2.03e-6) --
# the reference's own float32 error, as estimation_grad_ref.BOUND_GOLDEN
BOUND_GOLDEN = {"sigma": 1.4e-4, "rho": 4.1e-5, "kernel": 8.1e-6}

# which case rejects which mutant, in which field (tests/test_estimation_ref_cpu.py::test_every_mutant_is_rejected)
KILLERS = {"last_row": ("1x1x64x96_last_row", "mags"), "unpaired_row": ("1x1x37x75_last_row", "mags"),
           "first_row": ("1x1x64x96_first_row", "mags"), "last_col": ("1x1x64x96_last_col", "mags"),
           "first_col": ("1x1x64x96_first_col", "mags"), "cols2": ("1x1x37x75_last_col", "mags"), "cols4": ("1x1x37x75_last_col", "mags"),
           "cols8": ("1x1x37x75_last_col", "mags"), "cols16": ("1x1x37x75_last_col", "mags"), "cols32": ("1x1x37x75_last_col", "mags"),
           "image0": ("3x3x37x75_tl+last_col+last_row", "mags"), "no_mask": ("saturated_64x96", "mags"),
           "mask_ge": ("saturated_64x96", "mags"), "mask_normalised": ("saturated_64x96", "mags"),
           "mask_gx_only": ("saturated_64x96", "mags"), "plus_sin": ("1x1x64x96_br", "mags"), "table7": ("a12_i30_1x1x37x75_br", "mags"),
           "fold7": ("a12_i30_1x1x37x75_br", "mags"), "default_weights": ("a5_i30_1x1x37x75_br", "interp"),
           "last_min": ("a1_i7_1x1x37x75_br", "theta"), "ortho_round": ("oriented_i63_of_64", "rho"), "no_clamp": ("clamp_low", "sigma"),
           "first_partial": ("extremes_1x3x33x45_float32_-1.23", "mags"), "quantile_floor": ("quantised_float32_5x5_q0.0001", "mags")}
