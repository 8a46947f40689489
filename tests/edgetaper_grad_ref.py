"""What the gradients of the edgetaper are, restated for the tests (float64; CPU only).

The domain is Hp x Wp, the image as given to edgetaper.  One kernel has kh x kw taps (ODD sides), projections
ky[i] = sum_j k[i][j], kx[j] = sum_i k[i][j], and n blends.  Weights, PER KERNEL (edgetaper.py:10-23 takes torch.max over the whole
kernel tensor; the engine normalises each kernel by its own maximum, so every golden has a kernel batch of 1):

    ac_y[l] = sum_m ky[m] ky[m + l],  l = 0 .. kh - 1 (0 beyond)
    z_y[p]  = ac_y[p] + ac_y[Hp - 1 - p],  p = 0 .. Hp - 1          (period Hp - 1, z[Hp - 1] := z[0])
    v1[p]   = 1 - z_y[p] / ac_y[0];        v2 the same from kx and Wp;        A[py, px] = v1[py] v2[px]

Forward: x_0 = x, x_{i+1} = A x_i + (1 - A) (K x_i), K = convolve2d under the call's boundary (autograd_ref.apply_k).
Backward, g_n the upstream gradient, for i = n - 1 .. 0:

    u_i = (1 - A) g_{i+1};   g_i = A g_{i+1} + K^T u_i;   Kbar += L(u_i, x_i);   Abar += sum_channels g_{i+1} (x_i - K x_i)

then once per kernel and axis:  vbar1[py] = sum_px Abar v2[px] (vbar2 alike);  zbar[p] = -vbar[p] / ac[0];
acbar[l] = zbar[l] + zbar[Hp - 1 - l];  acbar[0] += sum_p vbar[p] z[p] / ac[0]^2;  kbar[m] = sum_l acbar[l] (k[m + l] + k[m - l]);
Kbar[i][j] += kbar_y[i] + kbar_x[j].

Two evaluations: `backward`, by hand as above (K^T and L are autograd_ref's, which tests/test_autograd_cpu.py pins), and
`autograd_gradients`, torch.autograd through `forward_torch`.  `backward(..., mutant=)` holds the six deliberate errors the CPU
test must be able to tell from the truth.

Tolerances (relative to the largest entry of the float64 gradient; E from tests/golden/make_golden_edgetaper_autograd.py's printout,
the reference's float32 gradient against its float64 one; the tolerance is 6 E, between 4 E and 8 E as DESIGN 4.13 did for TOL_DT):

    group                                    E image    E taps     tolerance image, taps                      engine: image, taps
    taper (edgetaper, t0 .. t5)              7.27e-7    9.72e-7    TOL_ET_X 4.4e-6, TOL_ET_K 5.8e-6           not measured yet
    chain (inverse_filtering_rank3, r0, r1)  3.10e-7    7.66e-7    TOL_CHAIN_X 1.9e-6, TOL_CHAIN_K 4.6e-6     not measured yet

The blind cases (float32 goldens only) take blind_tolerance of tests/test_gpu_blind_autograd.py and estimation_grad_ref.BOUND_GOLDEN.
"""
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import autograd_ref as ar
import estimation_grad_ref as er

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "edgetaper_grad.npz")

# (name, image shape, kernel shape, method, n_tapers, seed)
TAPER_CASES = [
    ("t0_ends_overlap", (1, 3, 9, 12), (1, 1, 5, 7), "fft", 3, 900),          # both ends' terms of z overlap on both axes (side < 2 k - 1)
    ("t1_tall_direct", (2, 3, 9, 12), (1, 1, 7, 5), "direct", 3, 901),        # taller than wide: 'direct' only; a broadcast kernel; B = 2
    ("t2_wide_31", (1, 1, 41, 53), (1, 1, 9, 31), "fft", 3, 902),             # above 25 taps: the large-kernel tables
    ("t3_single_blend", (1, 3, 30, 20), (1, 1, 11, 3), "direct", 1, 903),
    ("t4_two_channels", (1, 2, 16, 64), (1, 1, 5, 9), "fft", 2, 904),         # C other than 1 and 3
    ("t5_ring_inside", (1, 3, 60, 70), (1, 1, 25, 25), "fft", 3, 905),        # ring strictly inside the plane
]
GOLDEN_TAPER = [c[0] for c in TAPER_CASES]
# restatement only: one kernel per image, one kernel per plane, and no blend at all
EXTRA_CASES = [
    ("x0_per_image", (2, 3, 9, 12), (2, 1, 5, 7), "fft", 3, 910),
    ("x1_per_plane", (1, 3, 9, 12), (1, 3, 5, 7), "direct", 2, 911),
    ("x2_no_blend", (1, 3, 9, 12), (1, 1, 5, 7), "fft", 0, 912),
]
# inverse_filtering_rank3(do_edgetaper=True): (name, image shape, kernel shape, method, correlate, remove_halo, base seed)
CHAIN_CASES = [
    ("r0_correlate", (2, 3, 13, 17), (1, 1, 5, 9), "fft", True, False, 920),
    ("r1_direct", (1, 3, 12, 14), (1, 1, 7, 7), "direct", False, False, 940),
]
ALPHA, BETA = ar.ALPHA, ar.BETA
# the first seed at or after the base with no unclamped float64 output within 1e-3 of 0 or 1 and at least 5 % of the samples clamped
# (make_golden_edgetaper_autograd.py --search prints them; tests/test_edgetaper_autograd_cpu.py asserts the margins)
CHAIN_SEEDS = {"r0_correlate": 921, "r1_direct": 948}
# polyblur_deblurring(edgetaping=True), B = 1: (name, shape, blur of the input, n_iter, alpha, beta, method, base seed)
BLIND_CASES = [
    ("b0_fft", (1, 3, 18, 22), (2.2, 1.1), 1, 6, 1, "fft", 9500),
    ("b1_fft_two", (1, 3, 18, 22), (2.2, 1.1), 2, 2, 3, "fft", 9600),
]

TOL_ET_X, TOL_ET_K = 4.4e-6, 5.8e-6
TOL_CHAIN_X, TOL_CHAIN_K = 1.9e-6, 4.6e-6
MUTANTS = ("constant_weights", "no_normalisation", "no_far_end", "one_channel", "x0_for_xi", "period_n")
MUTANT_BOUND = 1e-3


def rel_error(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def taper_inputs(seed, xshape, kshape):
    """uniform image, uniform normalised kernel, upstream weights with 0.25 <= |w| < 1 and a random sign (float32 values)"""
    rng = np.random.default_rng(seed)
    x = rng.random(xshape).astype(np.float32)
    k = rng.random(kshape)
    k = (k / k.sum(axis=(-2, -1), keepdims=True)).astype(np.float32)
    w = (rng.uniform(0.25, 1.0, xshape) * rng.choice([-1.0, 1.0], xshape)).astype(np.float32)
    return x, k, w


def taper_case(name):
    for c in TAPER_CASES + EXTRA_CASES:
        if c[0] == name:
            x, k, w = taper_inputs(c[5], c[1], c[2])
            return dict(name=name, x=x, k=k, w=w, method=c[3], n=c[4])
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------
# the weights of one kernel along one axis, and their chain
# ---------------------------------------------------------------------------------------------
def autocorrelation(proj):
    kk = len(proj)
    return np.array([np.dot(proj[:kk - l], proj[l:]) for l in range(kk)])


def axis_weight(proj, n, period=None):
    """-> (v, z, ac) along an axis of n samples"""
    period = n - 1 if period is None else period
    ac = autocorrelation(np.asarray(proj, np.float64))
    lag = lambda l: ac[l] if 0 <= l < len(ac) else 0.0
    z = np.array([lag(p) + lag(period - p) for p in range(n)])
    return 1.0 - z / ac[0], z, ac


def axis_chain(vbar, proj, n, mutant=None):
    """vbar (n) -> the gradient of the projection"""
    proj = np.asarray(proj, np.float64)
    kk = len(proj)
    period = n if mutant == "period_n" else n - 1
    _, z, ac = axis_weight(proj, n, period)
    zbar = -vbar / ac[0]
    acbar = np.zeros(kk)
    for p in range(n):                                         # each p to the lag or lags it read
        if p < kk:
            acbar[p] += zbar[p]
        if 0 <= period - p < kk and mutant != "no_far_end":
            acbar[period - p] += zbar[p]
    if mutant != "no_normalisation":
        acbar[0] += np.dot(vbar, z) / ac[0] ** 2
    kbar = np.zeros(kk)
    for m in range(kk):
        for l in range(kk):
            kbar[m] += acbar[l] * ((proj[m + l] if m + l < kk else 0.0) + (proj[m - l] if m - l >= 0 else 0.0))
    return kbar


def blend_weights(k, H, W, period_n=False):
    """A in the shape (kb, kc, H, W), with v1 (kb, kc, H) and v2 (kb, kc, W)"""
    k = np.asarray(k, np.float64)
    kb, kc = k.shape[:2]
    v1, v2 = np.zeros((kb, kc, H)), np.zeros((kb, kc, W))
    for b in range(kb):
        for c in range(kc):
            v1[b, c] = axis_weight(k[b, c].sum(1), H, H if period_n else None)[0]
            v2[b, c] = axis_weight(k[b, c].sum(0), W, W if period_n else None)[0]
    return v1[..., :, None] * v2[..., None, :], v1, v2


def _K(x, k, method):
    return ar.apply_k(torch.tensor(np.ascontiguousarray(x)), torch.tensor(np.ascontiguousarray(k)), method).numpy()


def forward(x, k, method, n, keep=None, period_n=False):
    x, k = np.asarray(x, np.float64), np.asarray(k, np.float64)
    A = blend_weights(k, x.shape[-2], x.shape[-1], period_n)[0]
    xs = [x]
    for _ in range(n):
        xs.append(A * xs[-1] + (1.0 - A) * _K(xs[-1], k, method))
    if keep is not None:
        keep.update(xs=xs, A=A)
    return xs[-1]


def _to_kernel_planes(full, kshape):
    """(B, C, ...) summed over the dimensions the kernel broadcasts along"""
    if kshape[1] == 1:
        full = full.sum(axis=1, keepdims=True)
    if kshape[0] == 1:
        full = full.sum(axis=0, keepdims=True)
    return full


def backward(x, k, w, method, n, mutant=None):
    """d sum(w * edgetaper(x, k)) / d x and / d k by hand, float64"""
    x, k, g = (np.asarray(a, np.float64) for a in (x, k, w))
    H, W = x.shape[-2:]
    period_n = mutant == "period_n"
    keep = {}
    forward(x, k, method, n, keep, period_n)
    xs, A = keep["xs"], keep["A"]
    _, v1, v2 = blend_weights(k, H, W, period_n)
    gk, Abar = np.zeros(k.shape), np.zeros(A.shape)
    for i in reversed(range(n)):
        xi = xs[0] if mutant == "x0_for_xi" else xs[i]
        u = (1.0 - A) * g
        gk = gk + ar.lag(u, xi, k.shape, method)
        d = g * (xi - _K(xi, k, method))
        if mutant == "one_channel" and k.shape[1] == 1:
            d = np.concatenate([d[:, :1], np.zeros_like(d[:, 1:])], axis=1)
        Abar = Abar + _to_kernel_planes(d, k.shape)
        g = A * g + ar.adjoint(u, k, method)
    if mutant != "constant_weights":
        for b in range(k.shape[0]):
            for c in range(k.shape[1]):
                vbar1 = Abar[b, c] @ v2[b, c]
                vbar2 = v1[b, c] @ Abar[b, c]
                gk[b, c] += axis_chain(vbar1, k[b, c].sum(1), H, mutant)[:, None] + axis_chain(vbar2, k[b, c].sum(0), W, mutant)[None, :]
    return g, gk


# ---------------------------------------------------------------------------------------------
# the same forward through torch, for torch.autograd
# ---------------------------------------------------------------------------------------------
def _axis_weight_torch(proj, n):
    kk = proj.shape[-1]
    ac = [(proj[..., :kk - l] * proj[..., l:]).sum(-1) for l in range(kk)]
    zero = torch.zeros_like(ac[0])
    lag = lambda l: ac[l] if 0 <= l < kk else zero
    z = torch.stack([lag(p) + lag(n - 1 - p) for p in range(n)], dim=-1)
    return 1.0 - z / ac[0].unsqueeze(-1)


def forward_torch(x, k, method, n):
    """edgetaper with per-kernel normalisation on tensors of one dtype"""
    A = _axis_weight_torch(k.sum(-1), x.shape[-2]).unsqueeze(-1) * _axis_weight_torch(k.sum(-2), x.shape[-1]).unsqueeze(-2)
    for _ in range(n):
        x = A * x + (1.0 - A) * ar.apply_k(x, k, method)
    return x


def autograd_gradients(x, k, w, method, n, dtype=torch.float64):
    xt = torch.tensor(np.asarray(x), dtype=dtype, requires_grad=True)
    kt = torch.tensor(np.asarray(k), dtype=dtype, requires_grad=True)
    y = forward_torch(xt, kt, method, n)
    (y * torch.tensor(np.asarray(w), dtype=dtype)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), (torch.zeros_like(kt) if kt.grad is None else kt.grad).numpy()      # (n = 0: k is not reached)


# ---------------------------------------------------------------------------------------------
# inverse_filtering_rank3(do_edgetaper=True) and the blind call with edgetaping, through torch
# ---------------------------------------------------------------------------------------------
def rank3_taper_unclamped(x, k, alpha, b, method, correlate=False):
    """replicate pad -> three blends -> polynomial -> crop (deblurring.py:211-239)"""
    if correlate:
        k = k.flip(-2, -1)
    pad = k.shape[-1] // 2
    xp = forward_torch(F.pad(x, (pad, pad, pad, pad), mode="replicate"), k, method, 3)
    return ar.polynomial(xp, k, alpha, b, method)[..., pad:-pad, pad:-pad]


def chain_case(name, seed=None):
    for c in CHAIN_CASES:
        if c[0] == name:
            x, w, k = ar.case_inputs(CHAIN_SEEDS[name] if seed is None else seed, c[1], c[2])
            return dict(name=name, x=x, k=k, w=w, method=c[3], correlate=c[4], remove_halo=c[5])
    raise KeyError(name)


def chain_unclamped(c):
    return rank3_taper_unclamped(torch.tensor(np.asarray(c["x"], np.float64)), torch.tensor(np.asarray(c["k"], np.float64)), ALPHA, BETA,
                                 c["method"], c["correlate"]).numpy()


def chain_ok(c):
    margin, clamped = ar.clamp_margin(chain_unclamped(c))
    return margin > 1e-3 and clamped >= 0.05


def chain_gradients(c, dtype=torch.float64):
    xt = torch.tensor(np.asarray(c["x"]), dtype=dtype, requires_grad=True)
    kt = torch.tensor(np.asarray(c["k"]), dtype=dtype, requires_grad=True)
    y = torch.clamp(rank3_taper_unclamped(xt, kt, ALPHA, BETA, c["method"], c["correlate"]), 0.0, 1.0)
    (y * torch.tensor(np.asarray(c["w"]), dtype=dtype)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), kt.grad.numpy()


def blind_steps(x, n_iter, alpha, beta, method, c=0.352, b=0.768):
    """the blind call with edgetaping, float64 -> the per-iteration (input, records, unclamped output) list, or None as soon as an
    iteration misses a margin (estimation_grad_ref.case_ok; no unclamped output within 1e-3 of 0 or 1)"""
    xi, steps = np.asarray(x, np.float64), []
    for _ in range(n_iter):
        recs = er.estimate(xi, c, b)
        if not er.case_ok(recs):
            return None
        yu = rank3_taper_unclamped(torch.tensor(xi), torch.tensor(er.kernels(recs)), alpha, beta, method).numpy()
        if ar.clamp_margin(yu)[0] <= 1e-3:
            return None
        steps.append((xi, recs, yu))
        xi = np.clip(yu, 0.0, 1.0)
    return steps


def blind_gradient(x, w, n_iter, alpha, beta, method):
    """d sum(w * polyblur_deblurring(x, edgetaping=True)) / d x, float64 (estimation_grad_ref.blind_gradient with the taper)"""
    g = np.asarray(w, np.float64)
    for xi, recs, _ in reversed(blind_steps(x, n_iter, alpha, beta, method)):
        xt = torch.tensor(xi, requires_grad=True)
        kt = torch.tensor(er.kernels(recs), requires_grad=True)
        torch.clamp(rank3_taper_unclamped(xt, kt, alpha, beta, method), 0.0, 1.0).clip(0.0, 1.0).backward(torch.tensor(g))
        g = xt.grad.numpy() + er.estimate_backward(recs, grad_kernel=kt.grad.numpy())
    return g


# ---------------------------------------------------------------------------------------------
# the golden's reader
# ---------------------------------------------------------------------------------------------
def read_golden(path=GOLDEN):
    """-> (arrays, the JSON table `E` of the maker's figures per case, the JSON list of blind cases)"""
    d = np.load(path)
    return d, json.loads(str(d["E"])), json.loads(str(d["blind"]))
