"""The differentiable blind path on the GPU: polyblur_amd.gaussian_blur_estimation, pb_estimate_blur_backward alone,
and polyblur_deblurring / PolyblurDeblurring under torch.autograd -- against the float64 restatement (tests/estimation_grad_ref.py,
which tests/test_blind_autograd_cpu.py pins to the reference's own autograd) and against the reference's goldens.

Tolerances
  * the estimation's backward, relative to max |grad| per image: er.TOL_EST = 4 x the error of the float32 CPU evaluation of the
    restatement against float64 over the same cases (tests/test_blind_autograd_cpu.py measures it and holds the constant to it);
  * the blind gradient, per sample: er.TOL_EST x max |grad| of the image, plus n_iter x the per-sample tolerance
    tests/test_gpu_autograd.py uses for rank-3 (4e-5 x its pad factors) x max |upstream weight| (1 here);
  * the forward under grad against the same call under torch.no_grad(): 2e-5 x n_iter;
  * the forward of gaussian_blur_estimation: the bits of the blind driver's record; against the oracle's golden kernels (stages_A.npz) and the
    float64 restatement 1e-5 per tap, the figure tests/test_gpu_parity.py holds pb_estimate_blur to."""
import functools
import json

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import estimation_grad_ref as er
from polyblur_amd import _capi as capi

TOL_X, TOL_FWD, TOL_KERNEL = 4e-5, 2e-5, 1e-5
BACKWARD = {c[0]: c[1:] for c in er.backward_cases()}


def golden_cases(golden, kind):
    d = golden("blind_grad.npz")
    return [(c, d[c["name"] + "_x"], d[c["name"] + "_w"], d[c["name"] + "_gx"]) for c in json.loads(str(d["cases"])) if c["kind"] == kind]


@functools.lru_cache(maxsize=None)
def backward_reference(cid):
    """float64 (records, kernel weights, image gradient) of a case of the backward alone: computed once, shared, never written to"""
    x, sat = BACKWARD[cid]
    recs = er.estimate(x, discard_saturation=sat)
    w = er.kernel_weights(5, x.shape[0])
    return recs, w, er.estimate_backward(recs, grad_kernel=w)


def cuda(a, **kw):
    import torch
    return torch.tensor(np.asarray(a), device="cuda", **kw)


# ---------------------------------------------------------------------------------------------
# the forward of gaussian_blur_estimation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ker_size", [25, 13])
@pytest.mark.parametrize("half", [False, True])
@pytest.mark.parametrize("q", [0.0, 1e-4])
def test_forward_is_the_blind_drivers_kernel(q, half, ker_size):
    import torch
    import polyblur_amd as pa
    x = cuda(er.blurred_noise(11, (2, 3, 37, 45)))
    if half:
        x = x.half()
    k = pa.gaussian_blur_estimation(x, q=q, c=0.352, b=0.768, ker_size=ker_size)
    _, info = pa.polyblur_deblurring(x, n_iter=1, q=q, ker_size=ker_size, return_info=True)
    r0 = 12 - ker_size // 2
    want = info[0]["kernel"][:, r0:r0 + ker_size, r0:r0 + ker_size]
    assert k.dtype == torch.float32 and k.is_cuda and tuple(k.shape) == (2, 1, ker_size, ker_size) and not k.requires_grad
    assert np.array_equal(k.cpu().numpy()[:, 0], want)
    s, r, t = pa.gaussian_blur_estimation(x, q=q, c=0.352, b=0.768, ker_size=ker_size, return_2d_filters=False)
    for got, name in ((s, "sigma"), (r, "rho"), (t, "theta")):
        assert tuple(got.shape) == (2, 1) and np.array_equal(got.cpu().numpy()[:, 0], info[0][name])


def test_forward_of_arrays_and_cpu_tensors_and_against_float64(golden):
    import torch
    import polyblur_amd as pa
    g = golden("stages_A.npz")
    k = pa.gaussian_blur_estimation(g["x"], q=0.0, c=0.362, b=0.468)
    assert float(np.abs(k.reshape(len(k), -1) - g["kernel"].reshape(len(k), -1)).max()) < TOL_KERNEL
    x = er.blurred_noise(12, (2, 3, 40, 48))
    want = er.kernels(er.estimate(x))
    on_gpu = pa.gaussian_blur_estimation(cuda(x), q=0.0).cpu().numpy()
    err = float(np.abs(on_gpu - want).max())
    print("estimated kernel against the float64 restatement: %.3g per tap (tolerance %.3g)" % (err, TOL_KERNEL))
    assert err <= TOL_KERNEL
    arr = pa.gaussian_blur_estimation(x, q=0.0)
    cpu = pa.gaussian_blur_estimation(torch.from_numpy(x), q=0.0)
    assert isinstance(arr, np.ndarray) and arr.dtype == np.float32 and np.array_equal(arr, on_gpu)
    assert isinstance(cpu, torch.Tensor) and not cpu.is_cuda and np.array_equal(cpu.numpy(), on_gpu)
    # the grids the counts imply are accepted, anything else is not
    pa.gaussian_blur_estimation(x, q=0.0, thetas=torch.linspace(0, 180, 7).unsqueeze(0), interpolated_thetas=torch.arange(0, 180, 6.0).unsqueeze(0))
    with pytest.raises(ValueError):
        pa.gaussian_blur_estimation(x, q=0.0, thetas=torch.linspace(0, 170, 7))
    with pytest.raises(NotImplementedError):
        pa.gaussian_blur_estimation(x, q=0.0, ker_size=24)
    with pytest.raises(NotImplementedError):
        pa.gaussian_blur_estimation(np.zeros((1, 2, 16, 16), np.float32), multichannel=True)
    assert len(pa.gaussian_blur_estimation(x, q=0.0, ker_size=31, return_2d_filters=False)) == 3


# ---------------------------------------------------------------------------------------------
# pb_estimate_blur_backward alone
# ---------------------------------------------------------------------------------------------
def engine_backward(x, w, sat=False, c=0.362, b=0.464):
    import torch
    import polyblur_amd as pa
    xt = cuda(x, requires_grad=True)
    k = pa.gaussian_blur_estimation(xt, q=0.0, c=c, b=b, discard_saturation=sat)
    assert k.requires_grad and k.grad_fn is not None
    (k * cuda(w)).sum().backward()
    assert xt.grad.shape == xt.shape and xt.grad.dtype == torch.float32 and xt.grad.is_cuda
    return k.detach().cpu().numpy(), xt.grad.cpu().numpy()


@pytest.mark.parametrize("cid", list(BACKWARD))
def test_backward_alone_against_float64(cid):
    x, sat = BACKWARD[cid]
    recs, w, want = backward_reference(cid)
    k, g = engine_backward(x, w, sat)
    err = er.per_image_error(g, want)
    print("%-12s kernel %.3g | gradient %.3g of max |grad| = %.3g (tolerance %.3g)" % (cid, np.abs(k - er.kernels(recs)).max(), err, np.abs(want).max(), er.TOL_EST))
    assert err <= er.TOL_EST, (cid, err)
    # two samples of one pixel's channels get the same bits
    assert all(np.array_equal(g[:, 0], g[:, c]) for c in range(1, g.shape[1]))


def test_backward_alone_on_the_golden_shapes(golden):
    for c, x, w, gx in golden_cases(golden, "estimation"):
        want = er.estimate_backward(er.estimate(x), grad_kernel=w)
        _, g = engine_backward(x, w)
        e64, eref = er.per_image_error(g, want), er.per_image_error(g, gx)
        print("%s %-14s against float64 %.3g (tolerance %.3g) | against the reference's float32 %.3g (bound %.3g)"
              % (c["name"], x.shape, e64, er.TOL_EST, eref, er.TOL_EST + er.BOUND_GOLDEN))
        assert e64 <= er.TOL_EST and eref <= er.TOL_EST + er.BOUND_GOLDEN, (c, e64, eref)
        if any(f[1] for f in c["clamped"]):                  # rho clamped at 0.3: sigma's branch alone reaches the image
            assert np.abs(g).max() > 0


def test_sigma_rho_gradients_and_the_clamped_branch(golden):
    """return_2d_filters=False under grad: upstream gradients of sigma and of rho, one at a time; a clamped rho passes nothing"""
    import torch
    import polyblur_amd as pa
    for c, x, _, _ in golden_cases(golden, "estimation"):
        recs = er.estimate(x)
        for which in (0, 1):
            up = np.zeros((x.shape[0], 2))
            up[:, which] = 1.0
            want = er.estimate_backward(recs, grad_sigma_rho=up)
            xt = cuda(x, requires_grad=True)
            out = pa.gaussian_blur_estimation(xt, q=0.0, return_2d_filters=False)
            assert out[0].grad_fn is not None and not out[2].requires_grad
            out[which].sum().backward()
            g = xt.grad.cpu().numpy()
            for bi in range(x.shape[0]):
                if c["clamped"][bi][which]:
                    assert not g[bi].any() and not want[bi].any()
                else:
                    assert er.per_image_error(g[bi:bi + 1], want[bi:bi + 1]) <= er.TOL_EST


# ---------------------------------------------------------------------------------------------
# the blind call under grad
# ---------------------------------------------------------------------------------------------
def blind_tolerance(want, n_iter, pad=12):
    tol = np.full(want.shape, TOL_X)
    tol[..., [0, -1], :] *= 1 + pad
    tol[..., :, [0, -1]] *= 1 + pad
    return n_iter * tol + er.TOL_EST * np.abs(want).max(axis=(1, 2, 3), keepdims=True)


@pytest.mark.parametrize("module", [False, True])
def test_blind_gradients_against_the_goldens_and_float64(golden, module):
    import torch
    import polyblur_amd as pa
    seen = set()
    for c, x, w, gx in golden_cases(golden, "blind"):
        n_iter, alpha, beta, method = c["n_iter"], c["alpha"], c["beta"], c["method"]
        seen.add(n_iter)
        xt = cuda(x, requires_grad=True)
        if module:
            y = pa.PolyblurDeblurring()(xt, n_iter=n_iter, alpha=alpha, beta=beta, b=0.768, sigma_r=0.8, method=method)
        else:
            y = pa.polyblur_deblurring(xt, n_iter=n_iter, alpha=alpha, beta=beta, method=method)
        assert y.requires_grad and y.grad_fn is not None
        (y * cuda(w)).sum().backward()
        g = xt.grad.cpu().numpy()
        assert xt.grad.shape == xt.shape and xt.grad.dtype == torch.float32 and xt.grad.is_cuda
        with torch.no_grad():
            quiet = pa.polyblur_deblurring(xt, n_iter=n_iter, alpha=alpha, beta=beta, method=method)
        plain = pa.polyblur_deblurring(cuda(x), n_iter=n_iter, alpha=alpha, beta=beta, method=method)
        assert not quiet.requires_grad and not plain.requires_grad and torch.equal(quiet, plain)
        efwd = float((y.detach() - quiet).abs().max())
        want = er.blind_gradient(x, w, n_iter, alpha, beta, method)
        e64 = float(np.max(np.abs(g - want) / blind_tolerance(want, n_iter)))
        eref = float(np.max(np.abs(g - gx) / (blind_tolerance(want, n_iter) + er.BOUND_GOLDEN * np.abs(gx).max(axis=(1, 2, 3), keepdims=True))))
        print("%s %-6s n_iter %d (%g, %g): forward under grad vs no_grad %.3g (tolerance %.3g) | gradient %.3g of its tolerance against float64 "
              "(%.3g abs, max |grad| %.3g), %.3g against the reference's float32"
              % (c["name"], method, n_iter, alpha, beta, efwd, TOL_FWD * n_iter, e64, np.abs(g - want).max(), np.abs(want).max(), eref))
        assert efwd <= TOL_FWD * n_iter, (c, efwd)
        assert e64 <= 1.0 and eref <= 1.0, (c, e64, eref)
    assert seen == {1, 2, 3}


def test_without_grad_nothing_is_recorded():
    import torch
    import polyblur_amd as pa
    x = cuda(er.blurred_noise(13, (2, 3, 37, 45)))
    xg = x.clone().requires_grad_(True)
    k = pa.gaussian_blur_estimation(x, q=0.0)
    with torch.no_grad():
        kq = pa.gaussian_blur_estimation(xg, q=0.0)
    kg = pa.gaussian_blur_estimation(xg, q=0.0)
    assert not k.requires_grad and not kq.requires_grad and kg.grad_fn is not None
    assert torch.equal(k, kq) and torch.equal(k, kg.detach())


def test_blind_backward_repeated_eight_times_gives_identical_bits(golden):
    import polyblur_amd as pa
    c, x, w, _ = [t for t in golden_cases(golden, "blind") if t[0]["n_iter"] == 2][0]
    grads = []
    for _ in range(8):
        xt = cuda(x, requires_grad=True)
        (pa.polyblur_deblurring(xt, n_iter=2, alpha=c["alpha"], beta=c["beta"], method=c["method"]) * cuda(w)).sum().backward()
        grads.append(xt.grad.cpu().numpy())
    assert all(np.array_equal(grads[0], g) for g in grads[1:])


def test_workspace_grows_by_the_documented_scratch():
    """three fp32 planes per image and the partials: per workgroup 8 bytes of counts and 13 (value, index) pairs, per image 13 pairs
    and the 224-byte coefficient block (each buffer rounded up to 256 bytes)"""
    import torch
    from polyblur_amd.engine import Engine
    x = BACKWARD["130x257"][0]
    B, C, H, W = x.shape
    eng = Engine(0)
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        opts = Engine.make_options(c=0.362, b=0.464, q=0.0)
        xt, gk, gin = cuda(x), cuda(er.kernel_weights(5, B)), torch.empty((B, C, H, W), device="cuda")
        rec = torch.empty((B, capi.INFO_DTYPE.itemsize // 4), device="cuda")
        eng.estimate_blur_ptr(xt.data_ptr(), capi.PB_F32, x.shape, opts, rec.data_ptr())
        before = eng.workspace_bytes()
        for _ in range(2):
            eng.estimate_blur_backward_ptr(xt.data_ptr(), x.shape, opts, rec.data_ptr(), gk.data_ptr(), None, 25, gin.data_ptr())
        eng.synchronize()
        r256 = lambda n: (n + 255) // 256 * 256
        bpi = max(1, min((H * W + 2047) // 2048, max(1, 2048 // B)))
        assert bpi > 1
        assert eng.workspace_bytes() - before == 3 * r256(4 * B * H * W) + r256(B * bpi * (8 + 8 * 13) + B * (8 * 13 + 224))
        # what the C ABI refuses, before any launch
        for bad, ks in ((Engine.make_options(q=1e-4), 25), (opts, 24), (opts, 27)):
            with pytest.raises(capi.PolyblurHipError, match="PB_ERR_UNSUPPORTED"):
                eng.estimate_blur_backward_ptr(xt.data_ptr(), x.shape, bad, rec.data_ptr(), gk.data_ptr(), None, ks, gin.data_ptr())
    finally:
        eng.close()
