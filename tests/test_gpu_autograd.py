"""Gradients of the non-blind step on the GPU: polyblur_amd.convolve2d / compute_polynomial /
inverse_filtering_rank3 under torch.autograd and pb_tap_gradient alone, against the float64 restatement (tests/autograd_ref.py,
which tests/test_autograd_cpu.py pins to the reference's own autograd) and against the reference's goldens.

Tolerances
  * image gradient, weights w in [-1, 1]: 4e-5 per sample for convolve2d and the polynomial -- the project's 2e-5 for caller taps
    per unit of input range; the adjoint is the same pass on an input of range 2.  For inverse_filtering_rank3 times the number of
    padded samples the replicate pad folds into that pixel: (1 + p [edge row]) (1 + p [edge column]), p = kw // 2.
  * kernel gradient, normalised per lag by sum |u| |v|: ar.TOL_K = 1.9e-6 = 4 x the float32 CPU evaluation's own error
    (tests/test_autograd_cpu.py measures it, and asserts for every case here that a lag one sample off would exceed 10 x this and
    that no rank-3 case has an unclamped value within 1e-3 of 0 or 1).
  * forward values under grad against the fused no-grad path: 2e-5.
Shapes: ar.GPU_CASES -- less than one tile, no multiple of the tile, lags beyond the remainder and around the domain, the
large-kernel tables, several workgroups with several tiles each, per-image / per-plane / broadcast kernels."""
import functools
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import autograd_ref as ar
from polyblur_amd import _capi as capi

TOL_X, TOL_FWD = 4e-5, 2e-5
CASES = {c[0]: c[1:] for c in ar.gpu_cases()}
TAP_CASES = {c[0]: c[1:] for c in ar.tap_cases()}
BND = {"fft": capi.PB_WRAP, "direct": capi.PB_ZERO}


@functools.lru_cache(maxsize=None)
def reference(cid):
    """float64 (y, x.grad, kernel.grad, per-lag normaliser) of a case: computed once, shared, never written to"""
    func, method, x, w, k = CASES[cid]
    y, gx, gk = ar.gradients(func, x, k, w, ar.ALPHA, ar.BETA, method)
    _, norm = ar.kernel_grad_parts(func, x, k, w, ar.ALPHA, ar.BETA, method)
    return y, gx, gk, norm


def engine_call(func, x, k, alpha, b, method, correlate=False):
    import polyblur_amd as pa
    if func == "convolve2d":
        return pa.convolve2d(x, k, method=method)
    if func == "polynomial":
        return pa.compute_polynomial(x, k, alpha, b, method=method)
    return pa.inverse_filtering_rank3(x, k, alpha, b, correlate=correlate, method=method)


def engine_gradients(func, x, k, w, alpha, b, method, correlate=False, upstream=None):
    """(y, x.grad, kernel.grad) of loss = sum(w * y) by the engine, as numpy arrays"""
    import torch
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    kt = torch.tensor(k, device="cuda", requires_grad=True)
    y = engine_call(func, xt, kt, alpha, b, method, correlate)
    assert y.requires_grad and y.grad_fn is not None
    (y * torch.tensor(w, device="cuda")).sum().backward()
    assert xt.grad.shape == xt.shape and kt.grad.shape == kt.shape and kt.grad.dtype == kt.dtype and kt.grad.is_cuda
    return y.detach().cpu().numpy(), xt.grad.cpu().numpy(), kt.grad.cpu().numpy()


def image_tolerance(func, xshape, kw):
    tol = np.full(xshape, TOL_X)
    if func == "rank3":
        p = kw // 2
        tol[..., [0, -1], :] *= 1 + p
        tol[..., :, [0, -1]] *= 1 + p
    return tol


def check(cid, func, got, want, norm, kw):
    y, gx, gk = got
    wy, wgx, wgk = want
    ex = float(np.max(np.abs(gx - wgx) / image_tolerance(func, gx.shape, kw)))
    ek = ar.normalised_error(gk, wgk, norm)
    ey = float(np.abs(y - wy).max())
    print("%-44s forward %.3g | grad_x %.3g of its tolerance (%.3g abs) | grad_k normalised %.3g (tolerance %.3g)"
          % (cid, ey, ex, float(np.abs(gx - wgx).max()), ek, ar.TOL_K))
    assert ex <= 1.0, (cid, ex)
    assert ek <= ar.TOL_K, (cid, ek)


# ---------------------------------------------------------------------------------------------
# the feature switch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["fft", "direct"])
@pytest.mark.parametrize("func", ["convolve2d", "polynomial", "rank3"])
def test_grad_in_grad_out_and_untouched_without(func, method):
    import torch
    x, w, k = ar.case_inputs(77, (2, 3, 21, 26), (2, 1, 5, 7))
    for gi, gk_ in ((True, False), (False, True), (True, True)):
        xt = torch.tensor(x, device="cuda", requires_grad=gi)
        kt = torch.tensor(k, device="cuda", requires_grad=gk_)
        y = engine_call(func, xt, kt, 6, 1, method)
        assert y.requires_grad
        y.backward(torch.tensor(w, device="cuda"))
        assert (xt.grad is not None) == gi and (kt.grad is not None) == gk_
    # without grad: the same bits as under torch.no_grad(), and no graph
    plain = engine_call(func, torch.tensor(x, device="cuda"), torch.tensor(k, device="cuda"), 6, 1, method)
    assert not plain.requires_grad
    with torch.no_grad():
        quiet = engine_call(func, xt, kt, 6, 1, method)
    assert not quiet.requires_grad and torch.equal(plain, quiet)
    # the chain under grad agrees with the fused path
    assert float((y.detach() - plain).abs().max()) < TOL_FWD


# ---------------------------------------------------------------------------------------------
# against float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_gradients_against_float64(cid):
    func, method, x, w, k = CASES[cid]
    y, gx, gk, norm = reference(cid)
    check(cid, func, engine_gradients(func, x, k, w, ar.ALPHA, ar.BETA, method), (y, gx, gk), norm, k.shape[-1])


@pytest.mark.parametrize("cid", list(TAP_CASES))
def test_tap_gradient_alone(cid):
    """pb_tap_gradient on i.i.d. noise: store, then accumulate with a scale"""
    import torch
    from polyblur_amd.engine import get_engine
    method, x, w, k = TAP_CASES[cid]
    B, C, H, W = x.shape
    kb, kc, kh, kw = k.shape
    want, norm = ar.lag(w, x, k.shape, method), ar.lag(np.abs(w), np.abs(x), k.shape, method)
    eng = get_engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    u, v = torch.tensor(w, device="cuda"), torch.tensor(x, device="cuda")
    eshape = (B * C, 1, H, W) if kc > 1 else (B, C, H, W)
    g = torch.full((eshape[0], kh, kw), float("nan"), device="cuda")
    eng.tap_gradient_ptr(u.data_ptr(), v.data_ptr(), eshape, kh, kw, BND[method], g.data_ptr())
    first = g.clone()
    eng.tap_gradient_ptr(u.data_ptr(), v.data_ptr(), eshape, kh, kw, BND[method], g.data_ptr(), scale=0.5, accumulate=True)
    torch.cuda.synchronize()

    def folded(t):
        t = t.cpu().numpy().astype(np.float64).reshape(B, kc, kh, kw)
        return t.sum(0, keepdims=True) if kb == 1 else t
    e1, e2 = ar.normalised_error(folded(first), want, norm), ar.normalised_error(folded(g), 1.5 * want, 1.5 * norm)
    print("%-32s normalised error %.3g, after accumulate %.3g (tolerance %.3g)" % (cid, e1, e2, ar.TOL_K))
    assert e1 <= ar.TOL_K and e2 <= ar.TOL_K, (cid, e1, e2)


def test_goldens_of_the_reference(golden):
    d = golden("nonblind_grad.npz")
    for c in json.loads(str(d["cases"])):
        n = c["name"]
        x, w, k = d[n + "_x"], d[n + "_w"], d[n + "_k"]
        y, gx, gk = engine_gradients(c["func"], x, k, w, c["alpha"], c["b"], c["method"], c["correlate"])
        _, norm = ar.kernel_grad_parts(c["func"], x, k, w, c["alpha"], c["b"], c["method"], c["correlate"])
        ex = float(np.max(np.abs(gx - d[n + "_gx"]) / image_tolerance(c["func"], gx.shape, k.shape[-1])))
        ek = ar.normalised_error(gk, d[n + "_gk"], norm)
        print("%s %-10s %-6s grad_x %.3g of its tolerance | grad_k normalised %.3g (tolerance %.3g)" % (n, c["func"], c["method"], ex, ek, ar.TOL_K))
        assert ex <= 1.0 and ek <= ar.TOL_K, (c, ex, ek)


# ---------------------------------------------------------------------------------------------
# the engine against itself
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["fft", "direct"])
@pytest.mark.parametrize("xshape,kshape", [((2, 3, 37, 53), (2, 1, 5, 9)), ((1, 2, 70, 83), (1, 1, 27, 27)), ((1, 1, 65, 67), (1, 1, 25, 25))])
def test_adjoint_identity(xshape, kshape, method):
    """<K x, g> == <x, K^T g> with K x the forward and K^T g the backward of convolve2d, both dot products in float64 on the host"""
    import torch
    x, g, k = ar.case_inputs(91, xshape, kshape)
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    y = engine_call("convolve2d", xt, torch.tensor(k, device="cuda"), 0, 0, method)
    y.backward(torch.tensor(g, device="cuda"))
    lhs = np.vdot(y.detach().cpu().numpy().astype(np.float64), g.astype(np.float64))
    rhs = np.vdot(x.astype(np.float64), xt.grad.cpu().numpy().astype(np.float64))
    bound = 2e-5 * np.abs(g).sum(dtype=np.float64) + 4e-5 * np.abs(x).sum(dtype=np.float64)
    print("adjoint identity", xshape, kshape, method, "difference %.3g (bound %.3g)" % (abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


@pytest.mark.parametrize("cid", ["5x5_on_200x300-polynomial-fft", "49x49_on_70x83-polynomial-direct", "rank3_7x7_planes-rank3-fft"])
def test_two_identical_backward_calls_give_identical_bits(cid):
    func, method, x, w, k = CASES[cid]
    a = engine_gradients(func, x, k, w, ar.ALPHA, ar.BETA, method)
    b = engine_gradients(func, x, k, w, ar.ALPHA, ar.BETA, method)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_a_call_between_forward_and_backward_changes_nothing():
    import torch
    import polyblur_amd as pa
    func, method, x, w, k = CASES["5x9_on_37x53-polynomial-fft"]
    want = engine_gradients(func, x, k, w, ar.ALPHA, ar.BETA, method)
    xt = torch.tensor(x, device="cuda", requires_grad=True)
    kt = torch.tensor(k, device="cuda", requires_grad=True)
    y = pa.compute_polynomial(xt, kt, ar.ALPHA, ar.BETA, method=method)
    other_x, _, other_k = ar.case_inputs(5, (1, 2, 70, 83), (1, 1, 27, 27))
    with torch.no_grad():                                   # a bystander with other shapes, taps and scratch sizes
        pa.inverse_filtering_rank3(torch.tensor(other_x, device="cuda"), torch.tensor(other_k, device="cuda"), 2, 3, method="direct")
    (y * torch.tensor(w, device="cuda")).sum().backward()
    assert np.array_equal(xt.grad.cpu().numpy(), want[1]) and np.array_equal(kt.grad.cpu().numpy(), want[2])


def test_workspace_grows_by_the_documented_scratch():
    """the kernel-gradient path of the polynomial: four plane sets of the domain and the partial tables (each rounded up to 256 bytes)"""
    import torch
    from polyblur_amd.engine import Engine
    x, w, k = ar.case_inputs(6, (1, 2, 70, 83), (1, 1, 27, 27))
    B, C, H, W = x.shape
    eng = Engine(0)
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        xt, gt = torch.tensor(x, device="cuda"), torch.tensor(w, device="cuda")
        out, gx = torch.empty_like(xt), torch.empty_like(xt)
        gk = torch.empty((B, 27, 27), device="cuda")
        ks = eng.set_taps(k.reshape(B, 27, 27))
        eng.compute_polynomial_taps_ptr(xt.data_ptr(), out.data_ptr(), x.shape, ks, 6, 1, capi.PB_ZERO)
        before = eng.workspace_bytes()
        eng.compute_polynomial_taps_backward_ptr(xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), None, x.shape, ks, 6, 1, capi.PB_ZERO)
        assert eng.workspace_bytes() == before                 # (the image-only path: the forward's own scratch)
        eng.compute_polynomial_taps_backward_ptr(xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), gk.data_ptr(), x.shape, ks, 6, 1, capi.PB_ZERO)
        eng.synchronize()
        r256 = lambda n: (n + 255) // 256 * 256
        tiles = C * ((H + 31) // 32) * ((W + 31) // 32)
        G = min(tiles, max(1, 1024 // B))
        assert eng.workspace_bytes() - before == 4 * r256(4 * B * C * H * W) + r256(4 * B * G * 27 * 27)
        ks.free()
    finally:
        eng.close()
