"""What the gradients of the non-blind step are, restated for the tests (float64 unless asked otherwise; CPU only).

Two statements of the same mathematics, for a kh x kw kernel k with ODD sides on a domain of H x W:

  zero form (method='direct'):  (K x)[p] = sum_ij k[i,j] x[p + (i - kh//2, j - kw//2)],    x = 0 outside the domain
  wrap form (method='fft'):     (K x)[p] = sum_ij k[i,j] x[(p + (kh//2 - i, kw//2 - j)) mod (H, W)]

1. torch: the forms through F.conv2d, the polynomial a3 K^3 x + a2 K^2 x + a1 K x + b x by Horner (deblurring.py:113-169), the
   chain replicate pad -> polynomial -> crop -> clamp (deblurring.py:211-239); gradients by torch.autograd.
2. numpy, by hand: K, its adjoint K^T (the same form with every offset negated) and the lag correlation
   L(u, v)[i,j] = sum_planes sum_p u[p] v[p + off(i,j)]; from them grad_x and grad_k of convolve2d and of the polynomial.

Kernels are (kb, kc, kh, kw) with kb in (1, B), kc in (1, C): broadcast dimensions share taps, and their gradients add up."""
import numpy as np
import torch
import torch.nn.functional as F


def coefficients(alpha, b):
    return alpha / 2 - b + 2, 3 * b - alpha - 6, 5 - 3 * b + alpha / 2      # a3, a2, a1 (deblurring.py:133-135)


# ---------------------------------------------------------------------------------------------
# 1. torch
# ---------------------------------------------------------------------------------------------
def apply_k(x, k, method):
    """K x for x (B,C,H,W) and k (kb,kc,kh,kw), tensors of one dtype"""
    B, C, H, W = x.shape
    kh, kw = k.shape[-2:]
    assert kh % 2 == 1 and kw % 2 == 1
    ry, rx = kh // 2, kw // 2
    wgt = k.expand(B, C, kh, kw).reshape(B * C, 1, kh, kw)
    if method == "direct":
        xp = F.pad(x, (rx, rx, ry, ry))
    elif method == "fft":
        iy = torch.arange(-ry, H + ry) % H
        ix = torch.arange(-rx, W + rx) % W
        xp = x[:, :, iy][:, :, :, ix]
        wgt = wgt.flip(-2, -1)
    else:
        raise ValueError(method)
    return F.conv2d(xp.reshape(1, B * C, H + 2 * ry, W + 2 * rx), wgt, groups=B * C).reshape(B, C, H, W)


def polynomial(x, k, alpha, b, method, keep=None):
    a3, a2, a1 = coefficients(alpha, b)
    t0 = a3 * x
    t1 = apply_k(t0, k, method) + a2 * x
    t2 = apply_k(t1, k, method) + a1 * x
    if keep is not None:
        keep.update(t0=t0, t1=t1, t2=t2)
    return apply_k(t2, k, method) + b * x


def rank3_unclamped(x, k, alpha, b, method, correlate=False):
    if correlate:
        k = k.flip(-2, -1)
    pad = k.shape[-1] // 2
    y = polynomial(F.pad(x, (pad, pad, pad, pad), mode="replicate"), k, alpha, b, method)
    return y[..., pad:-pad, pad:-pad]


def rank3(x, k, alpha, b, method, correlate=False):
    return torch.clamp(rank3_unclamped(x, k, alpha, b, method, correlate), 0.0, 1.0)


FUNCTIONS = {
    "convolve2d": lambda x, k, alpha, b, method, correlate=False: apply_k(x, k, method),
    "polynomial": lambda x, k, alpha, b, method, correlate=False: polynomial(x, k, alpha, b, method),
    "rank3": rank3,
}


def gradients(func, x, k, w, alpha=2, b=3, method="fft", correlate=False, dtype=torch.float64):
    """y, d/dx and d/dk of loss = sum(w * y), as numpy arrays of `dtype`"""
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    kt = torch.tensor(np.asarray(k), dtype=dtype, requires_grad=True)
    y = FUNCTIONS[func](xt, kt, alpha, b, method, correlate)
    (y * torch.tensor(np.asarray(w), dtype=dtype)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), kt.grad.numpy()


# ---------------------------------------------------------------------------------------------
# 2. numpy, by hand
# ---------------------------------------------------------------------------------------------
def shifted(v, dy, dx, method):
    """s[..., p] = v[..., p + (dy, dx)]: zero outside the domain ('direct') or modulo it ('fft')"""
    H, W = v.shape[-2:]
    if method == "fft":
        return np.roll(v, (-dy, -dx), axis=(-2, -1))
    out = np.zeros_like(v)
    ys, ye = max(0, -dy), min(H, H - dy)
    xs, xe = max(0, -dx), min(W, W - dx)
    if ys < ye and xs < xe:
        out[..., ys:ye, xs:xe] = v[..., ys + dy:ye + dy, xs + dx:xe + dx]
    return out


def offset(i, j, kh, kw, method):
    return (i - kh // 2, j - kw // 2) if method == "direct" else (kh // 2 - i, kw // 2 - j)


def hand_k(x, k, method, adjoint=False):
    """K x, or K^T x: the same form with every offset negated"""
    B, C = x.shape[:2]
    kh, kw = k.shape[-2:]
    kk = np.broadcast_to(k, (B, C, kh, kw))
    out = np.zeros_like(x)
    s = -1 if adjoint else 1
    for i in range(kh):
        for j in range(kw):
            dy, dx = offset(i, j, kh, kw, method)
            out += kk[:, :, i, j, None, None] * shifted(x, s * dy, s * dx, method)
    return out


def hand_lag(u, v, kshape, method, extra=(0, 0)):
    """L(u, v) in the shape of a (kb,kc,kh,kw) kernel: planes that share taps are summed.  extra: a deliberate error of the lag
    (the tests' discriminating-power condition)"""
    B, C = u.shape[:2]
    kb, kc, kh, kw = kshape
    full = np.zeros((B, C, kh, kw), u.dtype)
    for i in range(kh):
        for j in range(kw):
            dy, dx = offset(i, j, kh, kw, method)
            full[:, :, i, j] = (u * shifted(v, dy + extra[0], dx + extra[1], method)).sum(axis=(-2, -1))
    if kc == 1:
        full = full.sum(axis=1, keepdims=True)
    if kb == 1:
        full = full.sum(axis=0, keepdims=True)
    return full


def hand_pairs(func, x, k, g, alpha, b, method):
    """the (u, v) pairs whose lag correlations add up to d loss / d k for the upstream gradient g of convolve2d / polynomial"""
    if func == "convolve2d":
        return [(g, x)]
    a3, a2, a1 = coefficients(alpha, b)
    t0 = a3 * x
    t1 = hand_k(t0, k, method) + a2 * x
    t2 = hand_k(t1, k, method) + a1 * x
    g2 = hand_k(g, k, method, adjoint=True)
    g1 = hand_k(g2, k, method, adjoint=True)
    return [(g, t2), (g2, t1), (g1, t0)]


def hand_gradients(func, x, k, g, alpha, b, method, extra=(0, 0)):
    """grad_x, grad_k and the per-lag normaliser sum |u| |v| for the upstream gradient g (convolve2d / polynomial)"""
    x, k, g = (np.asarray(a, np.float64) for a in (x, k, g))
    pairs = hand_pairs(func, x, k, g, alpha, b, method)
    gk = sum(hand_lag(u, v, k.shape, method, extra) for u, v in pairs)
    norm = sum(hand_lag(np.abs(u), np.abs(v), k.shape, method) for u, v in pairs)
    if func == "convolve2d":
        gx = hand_k(g, k, method, adjoint=True)
    else:
        a3, a2, a1 = coefficients(alpha, b)
        g2, g1 = pairs[1][0], pairs[2][0]
        gx = b * g + a1 * g2 + a2 * g1 + a3 * hand_k(g1, k, method, adjoint=True)
    return gx, gk, norm


def rank3_upstream(x, k, w, alpha, b, method, correlate=False):
    """what reaches the polynomial inside the rank-3 chain -- (padded image, taps as applied, upstream gradient on the padded
    domain: w under the clamp's mask, zero in the pad), float64 -- and the unclamped output"""
    x, k, w = (np.asarray(a, np.float64) for a in (x, k, w))
    y = rank3_unclamped(torch.tensor(x), torch.tensor(k), alpha, b, method, correlate).numpy()
    pad = k.shape[-1] // 2
    g = np.pad(w * ((y > 0) & (y < 1)), ((0, 0), (0, 0), (pad, pad), (pad, pad)))
    xp = np.pad(x, ((0, 0), (0, 0), (pad, pad), (pad, pad)), mode="edge")
    return xp, np.ascontiguousarray(k[..., ::-1, ::-1] if correlate else k), g, y


def normalised_error(got, want, norm):
    """max over the lags of |got - want| / sum |u| |v| (a lag no sample pair reaches -- norm 0 -- must be exactly 0)"""
    err = np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64))
    live = norm > 0
    return float(np.max(np.where(live, err / np.where(live, norm, 1.0), np.where(err > 0, np.inf, 0.0))))


# ---------------------------------------------------------------------------------------------
# the same pieces through torch (fast for 2401 lags), and the cases both test files share
# ---------------------------------------------------------------------------------------------
def lag(u, v, kshape, method, dtype=torch.float64):
    """L(u, v) in the shape of the kernel: d/dk of sum(u * K v)"""
    k = torch.zeros(tuple(kshape), dtype=dtype, requires_grad=True)
    (apply_k(torch.tensor(np.asarray(v), dtype=dtype), k, method) * torch.tensor(np.asarray(u), dtype=dtype)).sum().backward()
    return k.grad.numpy()


def adjoint(g, k, method):
    """K^T g: d/dx of sum(g * K x), float64"""
    x = torch.zeros(tuple(g.shape), dtype=torch.float64, requires_grad=True)
    (apply_k(x, torch.tensor(np.asarray(k), dtype=torch.float64), method) * torch.tensor(np.asarray(g), dtype=torch.float64)).sum().backward()
    return x.grad.numpy()


def pairs(func, x, k, w, alpha, b, method, correlate=False):
    """float64 (u, v) pairs whose lag correlations add up to kernel.grad of loss = sum(w * func(x, k)) -- for rank3 on the padded
    domain, in the orientation the taps are applied in -- and whether that orientation is the kernel's rotated by 180 degrees"""
    x, k, w = (np.asarray(a, np.float64) for a in (x, k, w))
    if func == "rank3":
        x, k, w, _ = rank3_upstream(x, k, w, alpha, b, method, correlate)
    if func == "convolve2d":
        return [(w, x)], False
    keep = {}
    polynomial(torch.tensor(x), torch.tensor(np.ascontiguousarray(k)), alpha, b, method, keep)
    g2 = adjoint(w, k, method)
    g1 = adjoint(g2, k, method)
    return [(w, keep["t2"].numpy()), (g2, keep["t1"].numpy()), (g1, keep["t0"].numpy())], bool(correlate and func == "rank3")


def kernel_grad_parts(func, x, k, w, alpha, b, method, correlate=False, shift=False):
    """(kernel.grad, per-lag normaliser sum |u| |v|) from the pairs, float64, in kernel.shape.  shift: every lag taken one sample
    off along x -- what a misplaced tap gradient would be (the discriminating-power condition)"""
    ps, flipped = pairs(func, x, k, w, alpha, b, method, correlate)
    kshape = np.asarray(k).shape
    gk = sum(lag(u, shifted(v, 0, 1, method) if shift else v, kshape, method) for u, v in ps)
    norm = sum(lag(np.abs(u), np.abs(v), kshape, method) for u, v in ps)
    if flipped:
        gk, norm = gk[..., ::-1, ::-1], norm[..., ::-1, ::-1]
    return gk, norm


def case_inputs(seed, xshape, kshape):
    """i.i.d. uniform noise in [0, 1], weights in [-1, 1], a dense kernel that is not point-symmetric (all float32 values)"""
    rng = np.random.default_rng(seed)
    x = rng.random(xshape).astype(np.float32)
    w = rng.uniform(-1, 1, xshape).astype(np.float32)
    k = rng.random(kshape) ** 3
    return x, w, (k / k.sum(axis=(-2, -1), keepdims=True)).astype(np.float32)


def clamp_margin(y):
    """(distance of the nearest unclamped value to 0 or 1, fraction of clamped samples)"""
    return float(np.minimum(np.abs(y), np.abs(y - 1)).min()), float(np.mean((y <= 0) | (y >= 1)))


# The GPU test's shapes (tests/test_gpu_autograd.py), each under both boundaries where the forward takes it:
# (name, functions, image shape, kernel shape, methods, seed).  For convolve2d / polynomial the image IS the domain; for rank3 the
# domain is the image padded by kw // 2 (the seeds of those were searched on the CPU for the clamp margin: test_autograd_cpu.py
# asserts it).  alpha, b = 6, 1 throughout (the clamp is active).
BOTH = ("fft", "direct")
GPU_CASES = [
    ("3x3_on_8x9", ("convolve2d", "polynomial"), (1, 1, 8, 9), (1, 1, 3, 3), BOTH, 501),                # less than one tile
    ("1x5_on_16x16", ("convolve2d", "polynomial"), (1, 1, 16, 16), (1, 1, 1, 5), BOTH, 502),
    ("5x9_on_37x53", ("convolve2d", "polynomial"), (2, 3, 37, 53), (2, 1, 5, 9), BOTH, 503),           # distinct kernels per image
    ("7x7_planes_on_33x40", ("convolve2d", "polynomial"), (2, 3, 33, 40), (2, 3, 7, 7), BOTH, 504),    # one kernel per plane
    ("25x25_on_64x64", ("polynomial",), (1, 1, 64, 64), (1, 1, 25, 25), BOTH, 505),
    ("25x25_on_65x67", ("convolve2d", "polynomial"), (1, 1, 65, 67), (1, 1, 25, 25), BOTH, 506),
    ("25x25_on_26x27", ("polynomial",), (1, 1, 26, 27), (1, 1, 25, 25), ("fft",), 507),                # the lags reach around the domain
    ("27x27_on_70x83", ("polynomial",), (1, 2, 70, 83), (1, 1, 27, 27), BOTH, 508),                    # large-kernel tables
    ("49x49_on_70x83", ("convolve2d", "polynomial"), (1, 2, 70, 83), (1, 1, 49, 49), BOTH, 509),
    ("5x5_on_200x300", ("polynomial",), (2, 1, 200, 300), (2, 1, 5, 5), BOTH, 510),                    # several workgroups, several tiles each
    ("3x5_broadcast_on_20x24", ("convolve2d", "polynomial"), (2, 3, 20, 24), (1, 1, 3, 5), BOTH, 511),
    # rank3: image shapes whose padded domains are 21x25, 18x20, 64x65, 70x83, 20x24
    ("rank3_5x9", ("rank3",), (2, 3, 13, 17), (2, 1, 5, 9), BOTH, 520),
    ("rank3_7x7_planes", ("rank3",), (2, 3, 12, 14), (2, 3, 7, 7), BOTH, 530),
    ("rank3_25x25", ("rank3",), (1, 1, 40, 41), (1, 1, 25, 25), BOTH, 540),
    ("rank3_49x49", ("rank3",), (1, 2, 22, 35), (1, 1, 49, 49), BOTH, 550),
    ("rank3_3x5_broadcast", ("rank3",), (2, 3, 16, 20), (1, 1, 3, 5), BOTH, 560),
]
ALPHA, BETA = 6, 1


def gpu_cases():
    """-> (id, func, method, x, w, k), one entry per (shape, function, boundary)"""
    for name, funcs, xshape, kshape, methods, seed in GPU_CASES:
        for func in funcs:
            for method in methods:
                seeds = RANK3_SEEDS.get((name, method), seed) if func == "rank3" else seed
                yield ("%s-%s-%s" % (name, func, method), func, method) + case_inputs(seeds, xshape, kshape)


def tap_cases():
    """-> (id, method, x, w, k): pb_tap_gradient alone, L(w, x) on every shape above whose image is the domain"""
    for name, funcs, xshape, kshape, methods, seed in GPU_CASES:
        if "rank3" not in funcs:
            for method in methods:
                yield ("%s-%s" % (name, method), method) + case_inputs(seed, xshape, kshape)


# The kernel-gradient tolerance, normalised per lag by sum |u| |v|: 4 x the largest such error of the float32 CPU evaluation of this
# restatement against float64 over every case above and every golden (4.78e-7, golden c19: the 49 x 49 rank-3 case under 'direct';
# tests/test_autograd_cpu.py measures it again and holds the constant to it)
TOL_K = 1.9e-6

# seeds of the rank3 cases, per boundary: the first at or after the case's base seed with no unclamped float64 output within 1e-3 of
# 0 or 1 and at least 5 % of the samples clamped
RANK3_SEEDS = {("rank3_5x9", "fft"): 521, ("rank3_5x9", "direct"): 570, ("rank3_7x7_planes", "fft"): 546, ("rank3_7x7_planes", "direct"): 543,
               ("rank3_25x25", "fft"): 546, ("rank3_25x25", "direct"): 552, ("rank3_49x49", "fft"): 573, ("rank3_49x49", "direct"): 557,
               ("rank3_3x5_broadcast", "fft"): 600, ("rank3_3x5_broadcast", "direct"): 568}
