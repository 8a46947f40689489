"""The gradient of the domain-transform recursive filter (domain_transform.py:6-85) with respect to the image and to the guide,
restated for the tests (CPU only, NumPy float64, sequential loops along a line).  A helper of
tests/test_dt_autograd_cpu.py, tests/test_gpu_dt_autograd.py and tests/golden/make_golden_dt_autograd.py.

A call is 2 N passes, rows then columns for iteration k = 0 .. N - 1, a_k = exp(log_a_k).  One pass along a line of n samples, input
x (C channels), weights v_i = exp(d_i log_a_k) shared by the channels, d_i = 1 + ratio sum_c |J_c,i - J_c,i-1| (i >= 1), ratio =
sigma_s / sigma_r:

    forward   f_0 = x_0;            f_i = x_i + v_i (f_{i-1} - x_i)
              g_{n-1} = f_{n-1};    g_i = f_i + v_{i+1} (g_{i+1} - f_i)
    backward  P_0 = G_0;            P_i = G_i + v_i P_{i-1}                     G: the adjoint of g
              fbar_i = (1 - v_{i+1}) P_i (i < n-1);   fbar_{n-1} = P_{n-1}
              vbar_{i+1} += sum_c P_i (g_{i+1} - f_i)
              Q_{n-1} = fbar_{n-1}; Q_i = fbar_i + v_{i+1} Q_{i+1}
              xbar_i = (1 - v_i) Q_i (i >= 1);        xbar_0 = Q_0
              vbar_i += sum_c Q_i (f_{i-1} - x_i)
    weights   Dbar_i = sum_k log_a_k v_{k,i} vbar_{k,i}                         one plane for the rows, one for the columns
    guide     Jbar_c,i = ratio (s_c,i Dbar_i - s_c,i+1 Dbar_{i+1}),  s_c,i = sign(J_c,i - J_c,i-1), sign(0) = 0

Mutants of the backward, each wrong in one way (MUTANTS): "weights constant" (vbar = 0: no gradient through the guide), "ends
dropped" (xbar_0 and fbar_{n-1} taken for 0), "one a" (iteration 0's coefficient in every iteration), "vbar one channel" (vbar
from channel 0 alone) and "sign of zero is one"."""
import functools
import json
import math
import os

import numpy as np

# (sigma_s, sigma_r, num_iterations): the settings of tests/golden/dt_grad.npz and of the GPU tests
SETTINGS = [(2.0, 0.8, 1), (6.0, 0.4, 2), (60.0, 0.4, 3)]
MUTANTS = ("weights constant", "ends dropped", "one a", "vbar one channel", "sign of zero is one")

# The GPU tests' tolerance per setting, relative to a gradient's largest entry: 4 .. 8 x E, E = the largest error of the reference's
# float32 gradients against its float64 ones over the setting's golden cases and both gradients (tests/test_dt_autograd_cpu.py
# measures E again from the golden and holds the constants there; the figures: DESIGN.md 4.13)
TOL_DT = {SETTINGS[0]: 1.0e-6, SETTINGS[1]: 2.0e-6, SETTINGS[2]: 6.0e-6}

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "dt_grad.npz")


def log_a(sigma_s, k, N):
    """the logarithm of iteration k's feedback coefficient (domain_transform.py:50,53), in double"""
    return -math.sqrt(2.0) / (sigma_s * math.sqrt(3.0) * 2.0 ** (N - (k + 1)) / math.sqrt(4.0 ** N - 1.0))


def _domain(J, ratio):
    """d along the last axis, (B,1,H,W); d[..., 0] = 1 is never used"""
    d = np.ones((J.shape[0], 1) + J.shape[2:])
    d[..., 1:] += ratio * np.abs(np.diff(J, axis=-1)).sum(axis=1, keepdims=True)
    return d


def _pass_forward(x, v):
    n = x.shape[-1]
    f = x.copy()
    for i in range(1, n):
        f[..., i] = x[..., i] + v[..., i] * (f[..., i - 1] - x[..., i])
    g = f.copy()
    for i in range(n - 2, -1, -1):
        g[..., i] = f[..., i] + v[..., i + 1] * (g[..., i + 1] - f[..., i])
    return f, g


def _pass_backward(x, v, G, mutant):
    """-> (xbar, vbar) of one pass along the last axis"""
    n = x.shape[-1]
    f, g = _pass_forward(x, v)
    P = G.copy()
    for i in range(1, n):
        P[..., i] = G[..., i] + v[..., i] * P[..., i - 1]
    fbar = P.copy()
    fbar[..., :n - 1] = (1.0 - v[..., 1:]) * P[..., :n - 1]
    if mutant == "ends dropped":
        fbar[..., n - 1] = 0.0
    Q = fbar.copy()
    for i in range(n - 2, -1, -1):
        Q[..., i] = fbar[..., i] + v[..., i + 1] * Q[..., i + 1]
    xbar = Q.copy()
    xbar[..., 1:] = (1.0 - v[..., 1:]) * Q[..., 1:]
    if mutant == "ends dropped":
        xbar[..., 0] = 0.0
    vbar = np.zeros_like(v)
    t = P[..., :n - 1] * (g[..., 1:] - f[..., :n - 1]) + Q[..., 1:] * (f[..., :n - 1] - x[..., 1:])
    vbar[..., 1:] = t[:, :1] if mutant == "vbar one channel" else t.sum(axis=1, keepdims=True)
    if mutant == "weights constant":
        vbar[:] = 0.0
    return xbar, vbar


def _swap(a):
    return np.ascontiguousarray(np.swapaxes(a, -1, -2))


def forward(I, J, sigma_s, sigma_r, N, passes=None, one_a=False):
    """recursive_filter(I, sigma_s, sigma_r, N, joint_image=J) in float64 (J None: guided by I); passes: gets (input, v,
    log_a, rows) of every pass, the column passes in transposed layout; one_a: the mutant's filter, iteration 0's coefficient in
    every iteration"""
    I = np.asarray(I, np.float64)
    J = I if J is None else np.asarray(J, np.float64)
    ratio = sigma_s / sigma_r
    dx, dy = _domain(J, ratio), _domain(_swap(J), ratio)
    F = I.copy()
    for k in range(N):
        la = log_a(sigma_s, 0 if one_a else k, N)
        for rows, d in ((True, dx), (False, dy)):
            x = F if rows else _swap(F)
            v = np.exp(d * la)
            if passes is not None:
                passes.append((x, v, la, rows))
            g = _pass_forward(x, v)[1]
            F = g if rows else _swap(g)
    return F


def backward(I, J, g, sigma_s, sigma_r, N, mutant=None):
    """-> (dI, dJ) of sum(g * recursive_filter(I, ..., joint_image=J)), float64.  J None: guided by I -- (dI with both paths, None)"""
    assert mutant is None or mutant in MUTANTS, mutant
    I = np.asarray(I, np.float64)
    guide = I if J is None else np.asarray(J, np.float64)
    ratio = sigma_s / sigma_r
    passes = []
    forward(I, guide, sigma_s, sigma_r, N, passes, one_a=mutant == "one a")
    G = np.asarray(g, np.float64)
    Dx = np.zeros((I.shape[0], 1) + I.shape[2:])
    Dy = np.zeros_like(_swap(Dx))
    for x, v, la, rows in reversed(passes):
        xbar, vbar = _pass_backward(x, v, G if rows else _swap(G), mutant)
        if rows:
            Dx += la * v * vbar
        else:
            Dy += la * v * vbar
        G = xbar if rows else _swap(xbar)
    sign = (lambda d: np.where(d >= 0, 1.0, -1.0)) if mutant == "sign of zero is one" else np.sign
    dJ = np.zeros_like(guide)
    tx = sign(np.diff(guide, axis=-1)) * Dx[..., 1:]
    dJ[..., 1:] += tx
    dJ[..., :-1] -= tx
    ty = _swap(sign(np.diff(_swap(guide), axis=-1)) * Dy[..., 1:])
    dJ[..., 1:, :] += ty
    dJ[..., :-1, :] -= ty
    dJ *= ratio
    return (G + dJ, None) if J is None else (G, dJ)


def rel_error(got, want):
    """largest |got - want| relative to the largest |want|"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---------------------------------------------------------------------------------------------
# inputs, and the golden file
# ---------------------------------------------------------------------------------------------
def inputs(shape, seed, joint=True, quantised=False):
    """-> (x, j or None, w): uniform float32 samples, upstream 0.25 <= |w| < 1 of either sign; quantised: the guide in multiples of
    1/8 -- many equal neighbours, and differences that float32 holds exactly"""
    rng = np.random.default_rng(seed)
    x = rng.random(shape, dtype=np.float32)
    j = rng.random(shape, dtype=np.float32)
    w = (rng.uniform(0.25, 1.0, shape) * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    if quantised:
        j = (np.round(j * 8.0) / 8.0).astype(np.float32)
    return x, (j if joint else None), w


def setting_of(case):
    return (float(case["sigma_s"]), float(case["sigma_r"]), int(case["num_iterations"]))


@functools.lru_cache(maxsize=None)
def golden():
    """-> (the npz, its list of cases); a case's arrays: d[case["x"]], d[case["w"]], d[case["j"]] with a joint image, and
    d[name + "_dx64"], "_dx32", with a joint image "_dj64", "_dj32"."""
    d = np.load(GOLDEN)
    return d, json.loads(str(d["cases"]))


@functools.lru_cache(maxsize=None)
def golden_case(name):
    """-> (case, x, j or None, w, {"dx64", "dx32"[, "dj64", "dj32"]}): read once, shared, never written to"""
    d, cases = golden()
    c = [c for c in cases if c["name"] == name][0]
    grads = {k: d[name + "_" + k] for k in ("dx64", "dx32", "dj64", "dj32") if name + "_" + k in d.files}
    return c, d[c["x"]], (d[c["j"]] if c["j"] else None), d[c["w"]], grads


@functools.lru_cache(maxsize=None)
def reference(shape, setting, seed, joint=True, quantised=False):
    """float64 gradients of a GPU test's case: computed once, shared, never written to -> (x, j, w, dI, dJ)"""
    x, j, w = inputs(shape, seed, joint, quantised)
    dI, dJ = backward(x, j, w, *setting)
    for a in (x, j, w, dI, dJ):
        if a is not None:
            a.setflags(write=False)
    return x, j, w, dI, dJ
