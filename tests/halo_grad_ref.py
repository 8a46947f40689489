"""The gradients of halo masking (deblurring.py:173-208) and of the spectral derivative (filters.py:159-186), restated for the
tests (CPU only).  A helper of tests/test_halo_autograd_cpu.py, tests/test_gpu_halo_autograd.py and
tests/golden/make_golden_halo_autograd.py; it builds on tests/halo_ref.py.

Per plane, inputs x (the image), y (the deblurred image), gx, gy (grad_img), upstream g:

    ox = Dx y        nM = sum gx^2 + gy^2        M = -gx ox - gy^2  (sic)        r = M / (nM + M)        z = max(r, 0)
    out = y + z (x - y)

    dz = g (x - y)   q = (r >= 0) ? dz / (nM + M)^2 : 0        dM = q nM        S = sum_plane -q M
    grad_x = g z     grad_y = g (1 - z) - Dx(-gx dM)     grad_gx = -ox dM + 2 gx S     grad_gy = -2 gy dM + 2 gy S
    fourier_gradients backward: grad_in = -(Dx ggx + Dy ggy)

stated twice in float64 -- NumPy by hand (hand_backward) and torch with autograd (halo_torch) -- and once more in float32 NumPy
(hand_backward(dtype=float32): the yardstick of the GPU test's tolerances).

Inputs of the stage: halo_ref.stage_set with the samples on the kink repaired (repaired_set).  A float32 evaluation of ox errs by
about 2e-7 of max |ox|, so a sample with |M| < 1e-4 (|gx| max|ox| + gy^2) could change sides of max(., 0); gy is raised there to
sqrt(1e-3 |gx| max|ox|), which empties the band in one pass (asserted)."""
import functools

import numpy as np
import torch

from oracle import polyblur_ref as ref
import autograd_ref as ar
import estimation_grad_ref as er
import halo_ref as hr

F32, F64 = np.float32, np.float64
NAMES = ("x", "y", "gx", "gy")


# ---------------------------------------------------------------------------------------------
# the spectral derivative: float64, and the fp32 oracle's
# ---------------------------------------------------------------------------------------------
def dx(v, dtype=F64):
    return hr.spectral_dx_f64(v) if dtype == F64 else ref.spectral_gradients(np.asarray(v, F32))[0]


def dy(v, dtype=F64):
    return hr._spectral_dy_f64(v) if dtype == F64 else ref.spectral_gradients(np.asarray(v, F32))[1]


def _torch_derivative(v, axis):
    """filters.py:172-184 with float64 frequencies: fftshift(fft2) * i 2 pi f, ifftshift, ifft2, real"""
    n = v.shape[axis]
    f = (torch.arange(n, dtype=torch.float64) - n // 2) / n
    f = f.reshape((n, 1) if axis == -2 else (1, n))
    U = torch.fft.fftshift(torch.fft.fft2(v), dim=(-2, -1))
    return torch.fft.ifft2(torch.fft.ifftshift(2.0 * np.pi * f * (1j * U), dim=(-2, -1))).real


def fourier_gradients_torch(v):
    return _torch_derivative(v, -1), _torch_derivative(v, -2)


def halo_torch(x, y, gx=None, gy=None, mutant=None):
    """halo_masking (deblurring.py:193-208) on float64 tensors, unclamped; autograd gives its gradients.  mutant: a backward that is
    wrong in one way (MUTANTS below), stated as the graph it would be the gradient of"""
    if gx is None:
        gx, gy = fourier_gradients_torch(x)
        if mutant == "grad_img detached":
            gx, gy = gx.detach(), gy.detach()
    ox = _torch_derivative(y, -1)
    M = -gx * ox - gy * gy
    nM = (gx * gx + gy * gy).sum(dim=(-2, -1), keepdim=True)
    z = torch.clamp(M / (nM + M), min=0)
    if mutant == "z detached":
        z = z.detach()
    return y + z * (x - y)


# ---------------------------------------------------------------------------------------------
# by hand
# ---------------------------------------------------------------------------------------------
def forward_parts(x, y, gx, gy, dtype=F64):
    x, y, gx, gy = (np.asarray(a, dtype) for a in (x, y, gx, gy))
    ox = np.asarray(dx(y, dtype), dtype)
    nM = (gx * gx + gy * gy).sum(axis=(-2, -1), keepdims=True, dtype=dtype)
    M = -gx * ox - gy * gy
    r = M / (nM + M)
    return ox, nM, M, r, np.maximum(r, dtype(0))


def hand_backward(x, y, gx, gy, g, dtype=F64, mutant=None):
    """-> dict of the four gradients.  mutant: one of MUTANTS' by-hand names, None for the formulas above"""
    x, y, gx, gy, g = (np.asarray(a, dtype) for a in (x, y, gx, gy, g))
    ox, nM, M, r, z = forward_parts(x, y, gx, gy, dtype)
    oy = None
    if mutant == "gy * oy":                                  # the forward the reference's name suggests, and its own backward
        oy = np.asarray(dy(y, dtype), dtype)
        M = -gx * ox - gy * oy
        r = M / (nM + M)
        z = np.maximum(r, dtype(0))
    if mutant == "nM of the neighbouring plane":
        if nM.shape[0] * nM.shape[1] < 2:
            return None
        nM = np.roll(nM.reshape(-1), 1).reshape(nM.shape)
        r = M / (nM + M)
        z = np.maximum(r, dtype(0))
    act = (r > 0) if mutant == "open side at r == 0" else (r >= 0)
    den = nM + M
    dz = g * (x - y)
    q = np.where(act, dz / (den * den), dtype(0)).astype(dtype)
    dM = q * nM
    S = (-q * M).sum(axis=(-2, -1), keepdims=True, dtype=dtype)
    if mutant == "S dropped":
        S = np.zeros_like(S)
    D = dy if mutant == "Dy for Dx" else dx
    sign = dtype(1) if mutant == "+D for -D" else dtype(-1)
    out = {"x": g * z, "y": g * (1 - z) + sign * np.asarray(D(-gx * dM, dtype), dtype), "gx": -ox * dM + 2 * gx * S}
    if mutant == "gy * oy":
        out["y"] = out["y"] - np.asarray(dy(-gy * dM, dtype), dtype)
        out["gy"] = -oy * dM + 2 * gy * S
    else:
        out["gy"] = -2 * gy * dM + 2 * gy * S
    return out


def fourier_backward(ggx, ggy, dtype=F64):
    out = 0
    if ggx is not None:
        out = out - np.asarray(dx(ggx, dtype), dtype)
    if ggy is not None:
        out = out - np.asarray(dy(ggy, dtype), dtype)
    return out


def autograd_backward(x, y, gx, gy, g, mutant=None):
    """the four gradients from torch.autograd of halo_torch, float64"""
    ts = [torch.tensor(np.asarray(a, F64), requires_grad=True) for a in (x, y, gx, gy)]
    halo_torch(*ts, mutant=mutant).backward(torch.tensor(np.asarray(g, F64)))
    return {n: (t.grad.numpy() if t.grad is not None else np.zeros(t.shape)) for n, t in zip(NAMES, ts)}


# mutants of the stage's backward, each wrong in one way (stage_mutant evaluates them)
MUTANTS = ["z detached", "S dropped", "+D for -D", "gy * oy", "open side at r == 0", "nM of the neighbouring plane", "Dy for Dx"]


def stage_mutant(name, s):
    """the four gradients a backward wrong in one way would give on the set s, or None where it does not apply"""
    if name == "z detached":
        return autograd_backward(s["x"], s["y"], s["gx"], s["gy"], s["g"], mutant=name)
    if name == "open side at r == 0" and not s["zeros"]:
        return None
    return hand_backward(s["x"], s["y"], s["gx"], s["gy"], s["g"], mutant=name)


def plane_error(got, want):
    """largest |got - want| per plane relative to that plane's largest |want| -> the largest over the planes"""
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    e = np.abs(got - want).max(axis=(-2, -1))
    n = np.abs(want).max(axis=(-2, -1))
    return float(np.max(e / n))


def plane_fraction(a, b, bound):
    """per plane, the fraction of samples where |a - b| >= bound x the plane's largest |a| -> the smallest over the planes"""
    a, b = np.asarray(a, F64), np.asarray(b, F64)
    n = np.abs(a).max(axis=(-2, -1), keepdims=True)
    return float((np.abs(a - b) >= bound * n).mean(axis=(-2, -1)).min())


# ---------------------------------------------------------------------------------------------
# the stage's input sets
# ---------------------------------------------------------------------------------------------
def kink_band(y, gx, gy):
    """samples whose side of max(., 0) a float32 evaluation could change"""
    gx, gy = np.asarray(gx, F64), np.asarray(gy, F64)
    ox = dx(y)
    mo = np.abs(ox).max(axis=(-2, -1), keepdims=True)
    return np.abs(-gx * ox - gy * gy) < 1e-4 * (np.abs(gx) * mo + gy * gy), mo


# the stage's shapes on the GPU (issue "Differentiable halo masking"), and what each reaches
STAGE_SHAPES = [
    (1, 3, 32, 48),         # four samples per lane
    (2, 3, 33, 50),         # scalar form, planes of energies 1 ... 30
    (1, 2, 34, 50),         # H W % 4 == 0, W % 4 != 0
    (1, 1, 2, 4), (1, 1, 2, 3), (1, 1, 8, 9),       # the smallest planes; odd and even N in both axes
    (1, 1, 96, 128),        # several workgroups per plane
    (1, 1, 520, 512),       # more partial sums per plane than one wave folds in one trip
    (16385, 4, 2, 4),       # 65 540 planes: more than a grid's y / z dimension holds
]
ZEROS_SHAPE = (1, 2, 16, 20)    # a tenth of the samples with gx == gy == 0 exactly: r == 0, the closed side of the clamp


@functools.lru_cache(maxsize=None)
def repaired_set(shape, zeros=False):
    """halo_ref.stage_set(shape) with the kink band emptied, an upstream gradient g with 0.25 <= |g| < 1, the float64 forward and
    backward"""
    s = hr.stage_set(tuple(shape))
    gx, gy = s["gx"].copy(), s["gy"].copy()
    band, mo = kink_band(s["y"], gx, gy)
    repaired = int(band.sum())
    gy[band] = np.sqrt(1e-3 * np.abs(gx.astype(F64)) * mo)[band].astype(F32)
    seed = 9100 + sum(v * m for v, m in zip(shape, (1, 7, 131, 1009)))
    rng = np.random.default_rng(seed)
    if zeros:
        hole = rng.random(shape) < 0.1
        gx[hole], gy[hole] = 0.0, 0.0
    assert not kink_band(s["y"], gx, gy)[0].any()
    g = (rng.choice([-1.0, 1.0], shape) * rng.uniform(0.25, 1, shape)).astype(F32)     # (no sample without an upstream gradient)
    out = dict(x=s["x"], y=s["y32"], gx=gx, gy=gy, g=g, repaired=repaired, zeros=bool(zeros))
    ox, nM, M, r, z = forward_parts(out["x"], out["y"], gx, gy)
    out.update(z=z, r=r, pole=np.abs(nM + M) / nM, want=hand_backward(out["x"], out["y"], gx, gy, g))
    # the gradient of the same stage without the mask (out = y)
    out["unmasked"] = {"x": np.zeros(shape), "y": g.astype(F64), "gx": np.zeros(shape), "gy": np.zeros(shape)}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def stage_cases():
    return [(hr.shape_id(s), s, False) for s in STAGE_SHAPES] + [("zeros_" + hr.shape_id(ZEROS_SHAPE), ZEROS_SHAPE, True)]


def active_sets_agree(s):
    """the float32 evaluation puts every sample on the side of max(., 0) the float64 one does"""
    r32 = forward_parts(s["x"], s["y"], s["gx"], s["gy"], F32)[3]
    return bool(np.array_equal(r32 >= 0, s["r"] >= 0))


# The GPU test's tolerances for pb_halo_mask_backward alone, relative to a plane's largest entry of the gradient in question: 4 x
# the largest error of the float32 NumPy evaluation of hand_backward against float64 over stage_cases() -- the 65 540 planes of
# eight samples apart (MANY: the largest of 65 540 planes' errors, a few of them 0.1 away from the pole of M / (nM + M))
# (tests/test_halo_autograd_cpu.py measures them again and holds each constant between four and eight times its figure)
TOL_STAGE = {"x": 1.2e-6, "y": 7.4e-7, "gx": 1.2e-6, "gy": 1.5e-6}
TOL_STAGE_MANY = {"x": 4.8e-6, "y": 2.3e-6, "gx": 6.3e-6, "gy": 2.2e-6}
MANY = (16385, 4, 2, 4)


def stage_tolerance(shape):
    return TOL_STAGE_MANY if tuple(shape) == MANY else TOL_STAGE


# pb_fourier_gradients_backward, relative to a plane's largest entry: the same rule on FOURIER_SHAPES
TOL_FOURIER = 1.0e-6
FOURIER_SHAPES = [(1, 2, 8, 9), (2, 1, 9, 8), (1, 3, 33, 50), (1, 1, 64, 48)]


def fourier_case(shape):
    rng = np.random.default_rng(9300 + sum(shape))
    return rng.uniform(-1, 1, shape).astype(F32), rng.uniform(-1, 1, shape).astype(F32)


# ---------------------------------------------------------------------------------------------
# the non-blind chain with the mask, float64 torch: pad -> polynomial -> crop -> halo_masking -> clamp
# ---------------------------------------------------------------------------------------------
def chain_torch(x, k, gx, gy, alpha, b, method, mutant=None, clamp=True):
    y = ar.rank3_unclamped(x, k, alpha, b, method)
    out = halo_torch(x, y, gx, gy, mutant=mutant)
    return torch.clamp(out, 0.0, 1.0) if clamp else out


def chain_gradients(x, k, grad_img, w, alpha, b, method, mutant=None, mask=True):
    """-> (unclamped output, dict of d sum(w * out) / d x, k, gx, gy), float64.  grad_img None: the image's own, inside the graph.
    mask=False: the same chain without the mask"""
    xt = torch.tensor(np.asarray(x, F64), requires_grad=True)
    kt = torch.tensor(np.asarray(k, F64), requires_grad=True)
    gs = [None, None] if grad_img is None else [torch.tensor(np.asarray(a, F64), requires_grad=True) for a in grad_img]
    if mask:
        out = chain_torch(xt, kt, gs[0], gs[1], alpha, b, method, mutant, clamp=False)
    else:
        out = ar.rank3_unclamped(xt, kt, alpha, b, method)
    (torch.clamp(out, 0.0, 1.0) * torch.tensor(np.asarray(w, F64))).sum().backward()
    grads = {"x": xt.grad.numpy(), "k": kt.grad.numpy()}
    if grad_img is not None and mask:
        grads.update({n: (t.grad.numpy() if t.grad is not None else np.zeros(t.shape)) for n, t in zip(("gx", "gy"), gs)})
    return out.detach().numpy(), grads


# ---------------------------------------------------------------------------------------------
# the blind call with remove_halo=True: grad_img = fourier_gradients(x0), once, for every iteration (deblurring.py:61,83)
# ---------------------------------------------------------------------------------------------
def blind(x, n_iter, kw, method="fft", ker_size=25):
    """-> (output, per-iteration (input, records, unclamped masked output, unclamped polynomial output)), float64"""
    x0 = np.asarray(x, F64)
    gx, gy = dx(x0), dy(x0)
    steps, xi = [], x0
    for _ in range(n_iter):
        recs = er.estimate(xi, kw["c"], kw["b"], ker_size)
        k = er.kernels(recs)
        yu = ar.rank3_unclamped(torch.tensor(xi), torch.tensor(k), kw["alpha"], kw["beta"], method).numpy()
        out = halo_torch(torch.tensor(xi), torch.tensor(yu), torch.tensor(gx), torch.tensor(gy)).numpy()
        steps.append((xi, recs, out, yu))
        xi = np.clip(out, 0.0, 1.0)
    return xi, steps


def blind_gradient(x, w, n_iter, kw, method="fft", ker_size=25, steps=None, mutant=None, mask=True, trace=None):
    """d sum(w * blind(x)) / d x, float64.  mask=False: the gradient of the same call without remove_halo, at the same inputs of
    every iteration -- what taking the mask for a constant 0 would give"""
    x0 = np.asarray(x, F64)
    if steps is None:
        _, steps = blind(x0, n_iter, kw, method, ker_size)
    g0x, g0y = dx(x0), dy(x0)
    g = np.asarray(w, F64)
    acc_x, acc_y = np.zeros_like(x0), np.zeros_like(x0)
    for xi, recs, _, _ in reversed(steps):
        xt = torch.tensor(xi, requires_grad=True)
        kt = torch.tensor(er.kernels(recs), requires_grad=True)
        gxt, gyt = torch.tensor(g0x, requires_grad=True), torch.tensor(g0y, requires_grad=True)
        yu = ar.rank3_unclamped(xt, kt, kw["alpha"], kw["beta"], method)
        yu.retain_grad()
        out = halo_torch(xt, yu, gxt, gyt, mutant=mutant if mutant == "z detached" else None) if mask else yu
        torch.clamp(out, 0.0, 1.0).clip(0.0, 1.0).backward(torch.tensor(g))
        g = xt.grad.numpy() + er.estimate_backward(recs, grad_kernel=kt.grad.numpy())
        if trace is not None:                                # (the largest upstream of the polynomial's backward, this input's gradient)
            trace.append((float(yu.grad.abs().max()), g))
        if mask and mutant != "z detached":
            acc_x, acc_y = acc_x + gxt.grad.numpy(), acc_y + gyt.grad.numpy()
    if mask and mutant not in ("grad_img detached", "z detached"):
        g = g + fourier_backward(acc_x, acc_y)
    return g


def blind_margins_ok(steps, gx, gy):
    """the margins of make_golden_blind_autograd.py at every iteration -- arg-max runner-up, range ends, clamp states, outputs 1e-3
    away from 0 and 1 -- and an empty kink band"""
    for xi, recs, out, yu in steps:
        if not er.case_ok(recs) or ar.clamp_margin(out)[0] <= 1e-3 or kink_band(yu, gx, gy)[0].any():
            return False
    return True


def blind_input(shape, seed, amp=0.3):
    """halo_ref's line image plus noise of 0.01"""
    x = hr.pipeline_image(shape, seed=seed, amp=amp).astype(F64) + 0.01 * np.random.default_rng(seed + 1).standard_normal(shape)
    return np.clip(x, 0.0, 1.0).astype(F32)


def golden_cases(d):
    import json
    return json.loads(str(d["cases"]))


# ---------------------------------------------------------------------------------------------
# what tests/golden/make_golden_halo_autograd.py hands to the reference itself (tests/golden/halo_grad.npz)
# ---------------------------------------------------------------------------------------------
GOLDEN_STAGE = [((1, 1, 2, 3), False), ((1, 1, 8, 9), False), ((2, 2, 9, 10), False), (ZEROS_SHAPE, True)]
# (image shape, kernel (h, w), method, grad_img=None?)
GOLDEN_CHAIN = [((2, 3, 13, 17), (5, 9), "fft", False), ((1, 3, 13, 17), (7, 7), "direct", False),
                ((2, 3, 20, 24), (9, 9), "fft", True), ((1, 3, 20, 24), (9, 9), "direct", True)]
GOLDEN_BLIND = [((2, 3, 20, 24), 1), ((1, 3, 24, 40), 2)]


def halo_numpy(x, y, gx, gy):
    z = forward_parts(x, y, gx, gy)[4]
    return np.asarray(y, F64) + z * (np.asarray(x, F64) - np.asarray(y, F64))


def chain_case(shape, kshape, method, own, seed=None, tries=400):
    """inputs of a non-blind case.  own: grad_img=None on the line image with beta < 0 (halo_ref.PIPE_KW's alpha, beta) and a
    Gaussian-like kernel; otherwise halo_ref's image, a dense kernel and built (reversed) gradients, alpha, beta = 6, 1.  The seed is
    searched (seed None) until no unclamped float64 output lies within 1e-3 of 0 or 1, at least 5 % of the samples are clamped and
    the kink band is empty"""
    alpha, beta = (hr.PIPE_KW["alpha"], hr.PIPE_KW["beta"]) if own else (hr.ALPHA, hr.BETA)
    s = 9400 + sum(shape) + 10 * sum(kshape) + (1000 if own else 0) if seed is None else seed
    for _ in range(tries):
        if own:
            x, k = blind_input(shape, s, amp=0.42), hr.gaussian_kernel(kshape, s + 50, shape[0])   # (a line of 0.42: 5 % clamped)
        else:
            x, k = hr.image(shape, s), hr.make_kernel(kshape, s + 50, shape[0])
        y = ar.rank3_unclamped(torch.tensor(np.asarray(x, F64)), torch.tensor(np.asarray(k, F64)), alpha, beta, method).numpy()
        if own:
            gx, gy = dx(x), dy(x)
        else:
            gx, gy = hr.reversed_gradients(dx(y), s + 1, hr.plane_scales(shape), 0.08, np.asarray(x, F64) - y)
            band, mo = kink_band(y, gx, gy)
            gy[band] = np.sqrt(1e-3 * np.abs(gx.astype(F64)) * mo)[band].astype(F32)
        out = halo_numpy(x, y, gx, gy)
        margin, clamped = ar.clamp_margin(out)
        if seed is not None or (margin > 1e-3 and clamped >= 0.05 and not kink_band(y, gx, gy)[0].any()):
            break
        s += 1
    else:
        raise RuntimeError("no seed found for %r" % ((shape, kshape, method, own),))
    w = np.random.default_rng(s + 70).uniform(-1, 1, shape).astype(F32)
    return dict(x=x, k=k, w=w, grad_img=None if own else (gx, gy), alpha=alpha, beta=beta, seed=s)


def blind_case(shape, n_iter, seed=None, tries=2000):
    s = 9600 + sum(shape) + 100 * n_iter if seed is None else seed
    for _ in range(tries):
        x = blind_input(shape, s)
        w = np.random.default_rng(s + 70).uniform(-1, 1, shape).astype(F32)
        _, steps = blind(x, n_iter, hr.PIPE_KW)
        if seed is not None or (blind_margins_ok(steps, dx(x), dy(x)) and blind_moved(x, w, n_iter, steps) >= 0.06):
            break
        s += 1
    else:
        raise RuntimeError("no seed found for %r" % ((shape, n_iter),))
    return dict(x=x, w=w, steps=steps, seed=s)


def blind_moved(x, w, n_iter, steps, ref=None):
    """the gauge of a blind case: the smallest fraction of a plane's samples on which the gradient with the mask and the gradient of
    the same call without it differ by 50 tolerances (the golden generator asks for 6 %, the CPU test for 5 %)"""
    ref = blind_tolerances(x, w, n_iter, hr.PIPE_KW, steps=steps) if ref is None else ref
    plain = blind_gradient(x, w, n_iter, hr.PIPE_KW, steps=steps, mask=False)
    return float((np.abs(ref["want"] - plain) >= 50 * ref["tol"]).mean(axis=(-2, -1)).min())


# ---------------------------------------------------------------------------------------------
# bounds against the goldens and the composed tolerances of the chain and blind cases (tests/test_gpu_halo_autograd.py's head)
# ---------------------------------------------------------------------------------------------
# 4 x the largest |restatement - golden| relative to the largest golden entry (of a plane: stage cases; of the tensor: chain cases)
# over the float64 cases of tests/golden/halo_grad.npz: the reference's float32 frequencies (filters.py:175-176)
BOUND_GOLDEN_F64 = 3.8e-7
# the same over the blind cases, per image: the reference's own float32 error
BOUND_GOLDEN_BLIND = 1.7e-5
TOL_X = 4e-5                                                  # tests/test_gpu_autograd.py's per-sample tolerance of rank-3
TOL_SUM = max(TOL_STAGE.values()) + TOL_FOURIER


def pad_factors(shape, pad):
    f = np.ones(shape)
    f[..., [0, -1], :] *= 1 + pad
    f[..., :, [0, -1]] *= 1 + pad
    return f


def image_max(a):
    return np.abs(a).max(axis=(1, 2, 3), keepdims=True)


def chain_tolerances(x, k, grad_img, w, alpha, b, method):
    """-> dict(want = the float64 gradients, tol = per gradient an array or scalar, upstream = the largest |gradient| the
    polynomial's backward receives, gk = kernel.grad again from the lag correlations)"""
    x64, k64 = np.asarray(x, F64), np.asarray(k, F64)
    out, want = chain_gradients(x64, k64, grad_img, w, alpha, b, method)
    y = ar.rank3_unclamped(torch.tensor(x64), torch.tensor(k64), alpha, b, method).numpy()
    gx, gy = (dx(x64), dy(x64)) if grad_img is None else grad_img
    g = np.asarray(w, F64) * ((out > 0) & (out < 1))
    hb = hand_backward(x64, y, gx, gy, g)
    U = float(np.abs(hb["y"]).max())
    pad = k64.shape[-1] // 2
    tol = {"x": TOL_X * pad_factors(x64.shape, pad) * U + TOL_SUM * image_max(want["x"])}
    if grad_img is not None:
        # the stage's tolerance, and what the polynomial's own error in y does to these gradients: the stage is handed the engine's
        # float32 y, which the project holds to halo_ref.TOL_INV of the float64 chain's; to first order sample i of a gradient moves
        # by at most TOL_INV x sum_j |d grad[i] / d y[j]| -- the Jacobian's absolute row sums, by differences of 1e-6 in float64 (no
        # sample changes sides: the kink band is empty), all planes at once since a plane's gradients depend on its own y alone
        H, W = x64.shape[-2:]
        base, rows = hand_backward(x64, y, gx, gy, g), {"gx": np.zeros(x64.shape), "gy": np.zeros(x64.shape)}
        for j in range(H * W):
            yj = y.copy()
            yj[..., j // W, j % W] += 1e-6
            hj = hand_backward(x64, yj, gx, gy, g)
            for n in rows:
                rows[n] += np.abs(hj[n] - base[n]) / 1e-6
        for n in rows:
            tol[n] = TOL_STAGE[n] * np.abs(want[n]).max(axis=(-2, -1), keepdims=True) + hr.TOL_INV * rows[n]
    widen = ((0, 0), (0, 0), (pad, pad), (pad, pad))
    xp = np.pad(x64, widen, mode="edge")
    gk, norm = ar.kernel_grad_parts("polynomial", xp, k64, np.pad(hb["y"], widen), alpha, b, method)
    _, flat = ar.kernel_grad_parts("polynomial", xp, k64, np.pad(np.full(x64.shape, U), widen), alpha, b, method)
    tol["k"] = ar.TOL_K * norm + TOL_STAGE["y"] * flat
    return dict(want=want, tol=tol, upstream=U, gk=gk, out=out)


def blind_tolerances(x, w, n_iter, kw, method="fft", steps=None):
    """-> dict(want, tol): the bound tests/test_gpu_blind_autograd.py holds the blind gradient to -- er.TOL_EST x the image's largest
    gradient entry plus n_iter x rank-3's per-sample tolerance (|w| <= 1) -- plus, per iteration, the stage's and the spectral
    derivative's tolerances x the image's largest gradient entry"""
    want = blind_gradient(x, w, n_iter, kw, method, steps=steps)
    tol = n_iter * TOL_X * pad_factors(want.shape, 12) + (er.TOL_EST + n_iter * TOL_SUM) * image_max(want)
    return dict(want=want, tol=tol)
