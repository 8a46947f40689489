"""The differentiable bilateral prefilter on the GPU: pb_bilateral_backward alone, polyblur_amd.bilateral_filter /
edge_aware_filtering under torch.autograd, and polyblur_deblurring / PolyblurDeblurring with prefiltering=True under grad --
against the float64 restatement (tests/bilateral_grad_ref.py, which tests/test_bilateral_autograd_cpu.py pins to autograd of the
reference's formula, proves discriminating and measures the tolerance for) and against the reference's goldens
(tests/golden/prefilter_grad.npz).

Tolerances
  * the backward alone, relative to the case's largest entry: bg.TOL_BILATERAL = 4 x the error of the float32 CPU evaluation of
    the same three steps against float64 over the same cases; ksize 1: g / (1 + 1e-5) to 2 ulp;
  * the blind call (bg.blind_tolerances), per sample: the bound tests/test_gpu_blind_autograd.py holds the blind gradient to
    (er.TOL_EST x the image's largest gradient entry + n_iter x rank-3's 4e-5 x its pad factors) -- with remove_halo
    tests/test_gpu_halo_autograd.py's, which adds the mask's and the spectral derivative's tolerances per iteration -- plus, per
    iteration, bg.TOL_BILATERAL x the largest upstream entry the bilateral stage receives there (float64);
  * the forward under grad against the fused path under torch.no_grad(): 2e-5 x n_iter."""
import functools
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import bilateral_grad_ref as bg
from polyblur_amd import _capi as capi

TOL_FWD = 2e-5


def cuda(a, **kw):
    import torch
    return torch.tensor(np.asarray(a), device="cuda", **kw)


def engine_backward(v, g, ksize, ss, sc):
    """pb_bilateral_backward through the engine, into a plane full of NaN: written, not accumulated"""
    import torch
    from polyblur_amd.engine import get_engine
    eng = get_engine(0)
    vt, gt = cuda(v), cuda(g)
    out = torch.full_like(vt, float("nan"))
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.bilateral_backward_ptr(vt.data_ptr(), gt.data_ptr(), out.data_ptr(), v.shape, ksize, ss, sc)
    torch.cuda.current_stream().synchronize()
    return out.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# pb_bilateral_backward alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bg.CASES, ids=bg.case_id)
def test_backward_alone_against_float64(case):
    shape, k, (ss, sc) = case
    v, g = bg.case_inputs(shape, sc)
    want = bg.case_reference(case)
    got = engine_backward(v, g, k, ss, sc)
    err = bg.case_error(got, want)
    print("%s: %.3g of max |grad| = %.3g (tolerance %.3g)" % (bg.case_id(case), err, np.abs(want).max(), bg.TOL_BILATERAL))
    assert np.isfinite(got).all()
    assert err <= bg.TOL_BILATERAL, (case, err)


@pytest.mark.parametrize("shape", [bg.TINY, bg.TILE], ids=bg.hg.hr.shape_id)
def test_ksize_1_is_the_upstream_over_one_plus_eps(shape):
    v, g = bg.case_inputs(shape, 0.1)
    got = engine_backward(v, g, 1, 5.0, 0.1)
    want = (g.astype(np.float64) / (1.0 + 1e-5)).astype(np.float32)
    ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)).max()
    print("ksize 1: %d ulp from g / (1 + 1e-5)" % ulp)
    assert ulp <= 2


def test_the_same_call_twice_gives_equal_bits():
    for case in ((bg.TILE, 13, bg.SIGMAS[0]), (bg.TINY, 25, bg.SIGMAS[0]), (bg.WIDE, 5, bg.SIGMAS[0])):
        shape, k, (ss, sc) = case
        v, g = bg.case_inputs(shape, sc)
        assert np.array_equal(engine_backward(v, g, k, ss, sc), engine_backward(v, g, k, ss, sc))


def test_bad_arguments_are_refused_before_any_launch():
    """a grad_in that aliases an input, an even or too large window, a sigma of 0, a plane of one row: PB_ERR_BADARG, nothing written"""
    import torch
    from polyblur_amd.engine import get_engine
    eng = get_engine(0)
    shape = (1, 2, 8, 9)
    v, g = torch.rand(shape, device="cuda"), torch.rand(shape, device="cuda")
    out = torch.full(shape, 7.0, device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    ptrs = (v.data_ptr(), g.data_ptr(), out.data_ptr())
    for args in ((v.data_ptr(), g.data_ptr(), v.data_ptr(), shape, 5, 5.0, 0.1), (v.data_ptr(), g.data_ptr(), g.data_ptr(), shape, 5, 5.0, 0.1),
                 ptrs + (shape, 4, 5.0, 0.1), ptrs + (shape, 27, 5.0, 0.1), ptrs + (shape, 0, 5.0, 0.1), ptrs + (shape, 5, 0.0, 0.1),
                 ptrs + (shape, 5, 5.0, 0.0), ptrs + ((1, 2, 1, 72), 5, 5.0, 0.1), (v.data_ptr(), None, out.data_ptr(), shape, 5, 5.0, 0.1)):
        with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):
            eng.bilateral_backward_ptr(*args)
    torch.cuda.current_stream().synchronize()
    assert bool((out == 7.0).all())


def test_workspace_grows_by_the_documented_scratch():
    """two plane sets and one padded plane set (each buffer rounded up to 256 bytes)"""
    import torch
    from polyblur_amd.engine import Engine
    shape, k = (1, 2, 33, 50), 7
    P, H, W = shape[0] * shape[1], shape[2], shape[3]
    v, g = torch.rand(shape, device="cuda"), torch.rand(shape, device="cuda")
    out = torch.empty_like(v)
    r256 = lambda n: (n + 255) // 256 * 256
    eng = Engine(0)
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.bilateral_ptr(v.data_ptr(), out.data_ptr(), capi.PB_F32, shape, k, 5.0, 0.1)
        before = eng.workspace_bytes()
        for _ in range(2):
            eng.bilateral_backward_ptr(v.data_ptr(), g.data_ptr(), out.data_ptr(), shape, k, 5.0, 0.1)
        eng.synchronize()
        assert eng.workspace_bytes() - before == 2 * r256(4 * P * H * W) + r256(4 * P * (H + k - 1) * (W + k - 1))
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------
# bilateral_filter and edge_aware_filtering under autograd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [(bg.TILE, 5, bg.SIGMAS[0]), (bg.TILE, 7, bg.SIGMAS[2]), (bg.TINY, 25, bg.SIGMAS[0])], ids=bg.case_id)
def test_bilateral_filter_function(case):
    import torch
    import polyblur_amd as pa
    shape, k, (ss, sc) = case
    v, g = bg.case_inputs(shape, sc)
    xt = cuda(v, requires_grad=True)
    out = pa.bilateral_filter(xt, k, ss, sc)
    assert out.requires_grad and out.grad_fn is not None
    out.backward(cuda(g))
    assert xt.grad.shape == xt.shape and xt.grad.dtype == torch.float32 and xt.grad.is_cuda
    err = bg.case_error(xt.grad.cpu().numpy(), bg.case_reference(case))
    print("%s through the Function: %.3g (tolerance %.3g)" % (bg.case_id(case), err, bg.TOL_BILATERAL))
    assert err <= bg.TOL_BILATERAL
    # the forward is pb_bilateral whatever the mode: the bits under torch.no_grad() and of a tensor that asks for nothing
    with torch.no_grad():
        quiet = pa.bilateral_filter(xt, k, ss, sc)
    plain = pa.bilateral_filter(cuda(v), k, ss, sc)
    assert not quiet.requires_grad and not plain.requires_grad
    assert np.array_equal(out.detach().cpu().numpy(), quiet.cpu().numpy()) and torch.equal(quiet, plain)
    assert float(np.abs(plain.cpu().numpy() - bg.forward64(v, k, ss, sc)).max()) <= 2e-6


def test_edge_aware_filtering_puts_both_results_in_the_graph():
    """loss = sum(a * smooth) + sum(b * noise), noise = img - smooth: d loss / d img = b + backward(a - b)"""
    import torch
    import polyblur_amd as pa
    shape = bg.TILE
    v, a = bg.case_inputs(shape, 0.1)
    b = np.random.default_rng(77).uniform(-1, 1, shape).astype(np.float32)
    xt = cuda(v, requires_grad=True)
    smooth, noise = pa.edge_aware_filtering(xt, 2.0, 0.8)
    assert smooth.grad_fn is not None and noise.grad_fn is not None
    ((smooth * cuda(a)).sum() + (noise * cuda(b)).sum()).backward()
    up = a.astype(np.float64) - b
    want = b + bg.backward(v, up, 5, 5.0, 0.1)
    err = float(np.abs(xt.grad.cpu().numpy() - want).max())
    bound = bg.TOL_BILATERAL * np.abs(bg.backward(v, up, 5, 5.0, 0.1)).max() + 2.0 ** -23 * np.abs(want).max()
    print("edge_aware_filtering: both outputs %.3g (bound %.3g)" % (err, bound))
    assert err <= bound
    xt.grad = None                                            # the noise alone: img - smooth still reaches the filter
    pa.edge_aware_filtering(xt, 2.0, 0.8)[1].backward(cuda(b))
    want = b + bg.backward(v, -b.astype(np.float64), 5, 5.0, 0.1)
    assert float(np.abs(xt.grad.cpu().numpy() - want).max()) <= bg.TOL_BILATERAL * np.abs(want - b).max() + 2.0 ** -23 * np.abs(want).max()
    with torch.no_grad():
        qs, qn = pa.edge_aware_filtering(xt, 2.0, 0.8)
    assert not qs.requires_grad and not qn.requires_grad
    assert torch.equal(qs, smooth.detach()) and torch.equal(qn, noise.detach())
    for other in ("domain_transform", "normalized_convolution"):
        with pytest.raises(NotImplementedError, match="edge_aware_filtering has no backward pass: the edge-aware filters are not differentiated"):
            pa.edge_aware_filtering(xt, 2.0, 0.8, prefilter=other)


# ---------------------------------------------------------------------------------------------
# the blind call with prefiltering=True
# ---------------------------------------------------------------------------------------------
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prefilter_grad.npz")
BLIND = ["p%02d" % n for n in range(len(bg.GOLDEN_BLIND))]


@functools.lru_cache(maxsize=None)
def blind_reference(name):
    """float64 gradient and tolerance of a golden case: computed once, shared, never written to"""
    d = np.load(GOLDEN)
    c = [c for c in json.loads(str(d["cases"])) if c["name"] == name][0]
    x, w = d[name + "_x"], d[name + "_w"]
    return c, x, w, d[name + "_dx"], bg.blind_tolerances(x, w, c["n_iter"], c["remove_halo"])


@pytest.mark.parametrize("module", [False, True], ids=["function", "module"])
@pytest.mark.parametrize("name", BLIND)
def test_blind_gradients_against_the_goldens_and_float64(name, module):
    import torch
    import polyblur_amd as pa
    c, x, w, gref, ref = blind_reference(name)
    kw = dict(bg.blind_kw(c["remove_halo"]), n_iter=c["n_iter"], remove_halo=c["remove_halo"], prefiltering=True)
    xt = cuda(x, requires_grad=True)
    y = pa.PolyblurDeblurring()(xt, sigma_r=0.8, **kw) if module else pa.polyblur_deblurring(xt, **kw)
    assert y.requires_grad and y.grad_fn is not None
    (y * cuda(w)).sum().backward()
    g = xt.grad.cpu().numpy()
    with torch.no_grad():
        quiet = pa.polyblur_deblurring(xt, **kw)
    plain = pa.polyblur_deblurring(cuda(x), **kw)
    assert not quiet.requires_grad and not plain.requires_grad and torch.equal(quiet, plain)
    efwd = float((y.detach() - quiet).abs().max())
    want, tol = ref["want"], ref["tol"]
    e64 = float(np.max(np.abs(g - want) / tol))
    eref = float(np.max(np.abs(g - gref) / (tol + bg.BOUND_GOLDEN_PREFILTER * np.abs(gref).max(axis=(1, 2, 3), keepdims=True))))
    print("%s n_iter %d remove_halo %s: forward under grad vs no_grad %.3g (tolerance %.3g) | gradient %.3g of its tolerance against "
          "float64 (%.3g abs, max |grad| %.3g, upstream of the filter %s), %.3g against the reference's float32"
          % (name, c["n_iter"], c["remove_halo"], efwd, TOL_FWD * c["n_iter"], e64, np.abs(g - want).max(), np.abs(want).max(),
             ", ".join("%.3g" % u for u in ref["upstream"]), eref))
    assert efwd <= TOL_FWD * c["n_iter"], (name, efwd)
    assert e64 <= 1.0 and eref <= 1.0, (name, e64, eref)


def test_blind_refusals_and_a_bogus_prefilter_on_rocm_tensors():
    import polyblur_amd as pa
    x = cuda(np.random.default_rng(5).random((1, 3, 16, 18), dtype=np.float32), requires_grad=True)
    for other in ("domain_transform", "normalized_convolution"):
        with pytest.raises(NotImplementedError, match=r"polyblur_deblurring\(prefiltering=True\) has no backward pass: the edge-aware prefilters are not differentiated"):
            pa.polyblur_deblurring(x, prefiltering=True, prefilter=other)
    with pytest.raises(ValueError, match="prefilter must be 'bilateral', 'domain_transform' or 'normalized_convolution'"):
        pa.polyblur_deblurring(x, prefiltering=True, prefilter="bogus")
    with pytest.raises(NotImplementedError, match=r"polyblur_deblurring\(prefiltering=True\) has no backward pass"):
        pa.polyblur_deblurring(x.half().detach().requires_grad_(True), prefiltering=True)
