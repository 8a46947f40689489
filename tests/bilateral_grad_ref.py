"""The gradient of the bilateral filter (filters.py:107-148) with respect to the image, restated for the tests (CPU
only).  A helper of tests/test_bilateral_autograd_cpu.py, tests/test_gpu_bilateral_autograd.py and
tests/golden/make_golden_prefilter_autograd.py; it builds on tests/estimation_grad_ref.py and tests/halo_grad_ref.py.

Per plane v, R = ksize // 2, q over the window of p with the replicate pad as an index clamp, upstream g:

    s_pq = exp(-(dx^2 + dy^2) / (2 ss^2))      d_pq = v_q - v_p      w_pq = s_pq exp(-d_pq^2 / (2 sc^2))
    D_p = sum_q w_pq      S1_p = sum_q w_pq d_pq      S2_p = sum_q w_pq d_pq^2
    out_p = (v_p D_p + S1_p) / (D_p + 1e-5)     G_p = g_p / (D_p + 1e-5)

    cen_p = G_p / sc^2 (S2_p + (v_p - out_p) S1_p)
    T_r'  = sum_{p in the image, |p - r'| <= R} G_p w_pr' (1 - (v_r' - out_p)(v_r' - v_p) / sc^2)      r' over the padded domain
    grad[r] = cen_r + sum_{r' that clamps to r} T_r'

stated in torch twice: the reference's formula for autograd (forward) and the three steps by hand (backward), the latter in
float64 and -- the yardstick of the GPU test's tolerance -- in float32.  Mutants of the backward, each wrong in one way:
"weights constant" (the gradient of sum w v / (sum w + 1e-5) with w held fixed), "centre dropped" (cen = 0) and "no fold" (the
pad's samples taken for constants: T cropped, exact away from the border)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import autograd_ref as ar
import estimation_grad_ref as er
import halo_grad_ref as hg

EPS = 1e-5
MUTANTS = ("weights constant", "centre dropped")
BORDER_MUTANT = "no fold"


def _offsets(R):
    return [(dy, dx) for dy in range(-R, R + 1) for dx in range(-R, R + 1)]


def forward(v, ksize=5, ss=5.0, sc=0.1):
    """the reference's formula on a torch tensor of any float dtype; autograd gives its gradient"""
    R = ksize // 2
    H, W = v.shape[-2:]
    vp = F.pad(v, (R, R, R, R), mode="replicate") if R else v
    num, den = torch.zeros_like(v), torch.zeros_like(v)
    for dy, dx in _offsets(R):
        q = vp[..., R + dy:R + dy + H, R + dx:R + dx + W]
        w = float(np.exp(-(dx * dx + dy * dy) / (2.0 * ss * ss))) * torch.exp(-(q - v) ** 2 / (2.0 * sc * sc))
        num, den = num + w * q, den + w
    return num / (den + EPS)


def forward64(v, ksize=5, ss=5.0, sc=0.1):
    return forward(torch.tensor(np.asarray(v, np.float64)), ksize, ss, sc).numpy()


def autograd_backward(v, g, ksize, ss, sc):
    vt = torch.tensor(np.asarray(v, np.float64), requires_grad=True)
    forward(vt, ksize, ss, sc).backward(torch.tensor(np.asarray(g, np.float64)))
    return vt.grad.numpy()


def backward(v, g, ksize, ss, sc, dtype=np.float64, mutant=None):
    """the three steps by hand, every operation in `dtype`"""
    tt = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    v, g = torch.tensor(np.asarray(v), dtype=tt), torch.tensor(np.asarray(g), dtype=tt)
    R = ksize // 2
    H, W = v.shape[-2:]
    Hp, Wp = H + 2 * R, W + 2 * R
    ic2, hc, hs = 1.0 / (sc * sc), 1.0 / (2.0 * sc * sc), 1.0 / (2.0 * ss * ss)
    vp = F.pad(v, (R, R, R, R), mode="replicate") if R else v
    # centre term, out and G: one walk of the window
    D, S1, S2 = torch.zeros_like(v), torch.zeros_like(v), torch.zeros_like(v)
    for dy, dx in _offsets(R):
        d = vp[..., R + dy:R + dy + H, R + dx:R + dx + W] - v
        w = float(np.exp(-(dx * dx + dy * dy) * hs)) * torch.exp(-d * d * hc)
        D, S1, S2 = D + w, S1 + w * d, S2 + w * d * d
    out = (v * D + S1) / (D + EPS)
    G = g / (D + EPS)
    cen = G * ic2 * (S2 + (v - out) * S1)
    if mutant in ("weights constant", "centre dropped"):
        cen = torch.zeros_like(cen)
    # tap term: a gather on the padded domain; G, out and v of the image at padded position r' + (dy, dx), G = 0 outside the image
    G2, o2, v2 = (F.pad(a, (2 * R,) * 4) for a in (G, out, v))
    T = torch.zeros(v.shape[:-2] + (Hp, Wp), dtype=tt)
    for dy, dx in _offsets(R):
        sl = (Ellipsis, slice(R + dy, R + dy + Hp), slice(R + dx, R + dx + Wp))
        e = vp - v2[sl]
        w = float(np.exp(-(dx * dx + dy * dy) * hs)) * torch.exp(-e * e * hc)
        f = 1.0 if mutant == "weights constant" else 1.0 - (vp - o2[sl]) * e * ic2
        T = T + G2[sl] * w * f
    # fold: the adjoint of the replicate pad, rows then columns
    if mutant == "no fold":
        return (cen + T[..., R:R + H, R:R + W]).numpy()
    A = T[..., R:R + H, :].clone()
    A[..., 0, :] += T[..., :R, :].sum(-2)
    A[..., -1, :] += T[..., R + H:, :].sum(-2)
    Bf = A[..., :, R:R + W].clone()
    Bf[..., :, 0] += A[..., :, :R].sum(-1)
    Bf[..., :, -1] += A[..., :, R + W:].sum(-1)
    return (cen + Bf).numpy()


def case_error(got, want):
    """largest |got - want| relative to the case's largest |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


def missed(got, want, bound):
    """where got misses want by at least bound x the largest |want|"""
    return np.abs(np.asarray(got, np.float64) - want) >= bound * np.abs(want).max()


# ---------------------------------------------------------------------------------------------
# the cases of pb_bilateral_backward alone
# ---------------------------------------------------------------------------------------------
SIGMAS = [(5.0, 0.1), (1.5, 0.02), (3.0, 0.05), (12.0, 0.5)]
KSIZES = [1, 3, 5, 7, 13, 25]
TINY, TILE, WIDE, MANY = (1, 1, 2, 2), (2, 3, 17, 65), (1, 2, 33, 130), (65540, 1, 2, 4)
CASES = ([(TINY, k, SIGMAS[0]) for k in (1, 3, 25)]                    # a window far larger than the plane: every corner folds (R + 1)^2
         + [(TILE, k, s) for k in KSIZES for s in SIGMAS]              # one column past a 64-wide tile, one row past a 16-row tile
         + [(WIDE, 5, SIGMAS[0]), (WIDE, 13, SIGMAS[2])]               # three tiles across, three down
         + [(MANY, 3, SIGMAS[0])])                                     # more planes than gridDim.z holds


def case_id(case):
    shape, k, (ss, sc) = case
    return "%s-k%d-s%g-c%g" % ("x".join(str(n) for n in shape), k, ss, sc)


@functools.lru_cache(maxsize=None)
def case_inputs(shape, sc):
    """samples uniform in an interval of min(1, 10 sc) around 0.5 -- at any sigma_color most windows hold samples within a few
    sigma_color of their centre, so the weights' own derivatives matter at most samples --, upstream 0.25 <= |g| < 1 of either
    sign; float32 values"""
    rng = np.random.default_rng(4120 + sum(shape))
    v = (0.5 + min(1.0, 10.0 * sc) * (rng.random(shape) - 0.5)).astype(np.float32)
    g = (rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    return v, g


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """float64 gradient of a case: computed once, shared, never written to"""
    shape, k, (ss, sc) = case
    v, g = case_inputs(shape, sc)
    want = backward(v, g, k, ss, sc)
    want.setflags(write=False)
    return want


# The GPU test's tolerance for pb_bilateral_backward, relative to the case's largest |grad|: 4 x the largest error of the float32
# CPU evaluation of backward() against float64 over CASES (tests/test_bilateral_autograd_cpu.py measures it again and holds the
# constant between four and eight times it; the figures: DESIGN.md 4.12)
TOL_BILATERAL = 5.4e-6


# ---------------------------------------------------------------------------------------------
# the blind call with prefiltering=True: estimate on the input, the bilateral split, the non-blind step on the smooth part (with
# the mask where asked: its x is the smooth part) and its own clamp (deblurring.py:239), + noise, clip (deblurring.py:63-84)
# ---------------------------------------------------------------------------------------------
PLAIN_KW = dict(c=0.352, b=0.768, alpha=6, beta=1)                      # (the driver's c and b; alpha, beta as the blind goldens')
HALO_KW = dict(c=1.0, b=0.468, alpha=6, beta=-3)                       # (halo_ref.PIPE_KW's: the mask finds work)
# (shape, n_iter, remove_halo)
GOLDEN_BLIND = [((1, 3, 20, 24), 1, False), ((1, 3, 18, 22), 2, False), ((1, 3, 20, 24), 1, True), ((1, 3, 16, 20), 2, True)]


def blind_kw(halo):
    return HALO_KW if halo else PLAIN_KW


def blind(x, n_iter, halo, method="fft"):
    """-> (output, per-iteration (input, records, smooth part, the step's unclamped output, unclamped polynomial output, the unclipped
    sum with the noise)), float64"""
    kw = blind_kw(halo)
    x0 = np.asarray(x, np.float64)
    gx, gy = (hg.dx(x0), hg.dy(x0)) if halo else (None, None)
    steps, xi = [], x0
    for _ in range(n_iter):
        recs = er.estimate(xi, kw["c"], kw["b"], 25)
        smooth = forward64(xi)
        yu = ar.rank3_unclamped(torch.tensor(smooth), torch.tensor(er.kernels(recs)), kw["alpha"], kw["beta"], method).numpy()
        m = hg.halo_torch(torch.tensor(smooth), torch.tensor(yu), torch.tensor(gx), torch.tensor(gy)).numpy() if halo else yu
        out = np.clip(m, 0.0, 1.0) + (xi - smooth)
        steps.append((xi, recs, smooth, m, yu, out))
        xi = np.clip(out, 0.0, 1.0)
    return xi, steps


def blind_gradient(x, w, n_iter, halo, method="fft", steps=None, mutant=None, trace=None):
    """d sum(w * blind(x)) / d x, float64.  mutant "smooth detached": the bilateral filter taken for a constant.
    trace: gets, per iteration from the last to the first, the largest upstream entry the bilateral stage receives"""
    kw = blind_kw(halo)
    x0 = np.asarray(x, np.float64)
    if steps is None:
        _, steps = blind(x0, n_iter, halo, method)
    g = np.asarray(w, np.float64)
    acc_x, acc_y = np.zeros_like(x0), np.zeros_like(x0)
    for xi, recs, _, _, _, _ in reversed(steps):
        xt = torch.tensor(xi, requires_grad=True)
        kt = torch.tensor(er.kernels(recs), requires_grad=True)
        smooth = forward(xt)
        if mutant == "smooth detached":
            smooth = smooth.detach().requires_grad_(True)
        else:
            smooth.retain_grad()
        yu = ar.rank3_unclamped(smooth, kt, kw["alpha"], kw["beta"], method)
        if halo:
            gxt, gyt = torch.tensor(hg.dx(x0), requires_grad=True), torch.tensor(hg.dy(x0), requires_grad=True)
            m = hg.halo_torch(smooth, yu, gxt, gyt)
        else:
            m = yu
        (torch.clamp(m, 0.0, 1.0) + (xt - smooth)).clip(0.0, 1.0).backward(torch.tensor(g))
        g = xt.grad.numpy() + er.estimate_backward(recs, grad_kernel=kt.grad.numpy())
        if trace is not None:
            trace.append(float(smooth.grad.abs().max()))
        if halo:
            acc_x, acc_y = acc_x + gxt.grad.numpy(), acc_y + gyt.grad.numpy()
    if halo:
        g = g + hg.fourier_backward(acc_x, acc_y)
    return g


def blind_margins_ok(steps, x0, halo):
    """the margins of make_golden_blind_autograd.py at every iteration's input -- arg-max runner-up, range ends, clamp states, outputs
    1e-3 away from 0 and 1 (the step's own, which it clamps, and the sum with the noise, which the driver clips) -- and, with the
    mask, an empty kink band"""
    gx, gy = (hg.dx(x0), hg.dy(x0)) if halo else (None, None)
    for xi, recs, smooth, m, yu, out in steps:
        if not er.case_ok(recs) or ar.clamp_margin(m)[0] <= 1e-3 or ar.clamp_margin(out)[0] <= 1e-3:
            return False
        if halo and hg.kink_band(yu, gx, gy)[0].any():
            return False
    return True


def blind_input(shape, seed, halo):
    """the inputs of the blind goldens plus noise of 0.01 for the prefilter to take out: halo_grad_ref's line image with the mask,
    estimation_grad_ref's blurred noise without"""
    if halo:
        return hg.blind_input(shape, seed)
    x = er.blurred_noise(seed, shape).astype(np.float64) + 0.01 * np.random.default_rng(seed + 1).standard_normal(shape)
    return np.clip(x, 0.0, 1.0).astype(np.float32)


def blind_case(shape, n_iter, halo, seed=None, tries=4000):
    s = 9700 + sum(shape) + 100 * n_iter + (1000 if halo else 0) if seed is None else seed
    for _ in range(tries):
        x = blind_input(shape, s, halo)
        _, steps = blind(x, n_iter, halo)
        if seed is not None or blind_margins_ok(steps, np.asarray(x, np.float64), halo):
            break
        s += 1
    else:
        raise RuntimeError("no seed found for %r" % ((shape, n_iter, halo),))
    w = np.random.default_rng(s + 70).uniform(-1, 1, shape).astype(np.float32)
    return dict(x=x, w=w, steps=steps, seed=s)


# 4 x the largest |restatement - golden| relative to the image's largest golden entry over tests/golden/prefilter_grad.npz: the
# reference's own float32 error (tests/test_bilateral_autograd_cpu.py measures it again)
BOUND_GOLDEN_PREFILTER = 1.6e-5


def blind_tolerances(x, w, n_iter, halo, method="fft", steps=None):
    """-> dict(want, tol, upstream): the bound the blind gradient is held to without prefiltering -- tests/test_gpu_blind_autograd.py's,
    with the mask tests/test_gpu_halo_autograd.py's (hg.blind_tolerances) -- plus, per iteration, TOL_BILATERAL x the largest
    upstream entry the bilateral stage receives there (float64)"""
    trace = []
    want = blind_gradient(x, w, n_iter, halo, method, steps=steps, trace=trace)
    tol = n_iter * hg.TOL_X * hg.pad_factors(want.shape, 12) + (er.TOL_EST + (n_iter * hg.TOL_SUM if halo else 0.0)) * hg.image_max(want)
    return dict(want=want, tol=tol + TOL_BILATERAL * sum(trace), upstream=trace)
