"""Learnable parameters on the GPU: pb_compute_polynomial_taps_params_backward and pb_estimate_blur_params_backward
alone against the float64 restatement (tests/params_grad_ref.py, which tests/test_params_autograd_cpu.py pins to the reference's own
autograd), and the public functions and the module with alpha, beta, c and b as tensors against the goldens
(tests/golden/params_grad.npz).

Tolerances, relative to the case's larger gradient: pr.TOL_POLY per case, pr.TOL_EST per clamp state, pr.TOL_BLIND per (alpha, beta,
method) -- each 6 times the reference's own float32 error E against the float64 truth in that setting (params_grad_ref.py); where
the engine is compared with the reference's float32 value the reference's own error E is added to the bound."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import autograd_ref as ar
import estimation_grad_ref as er
import params_grad_ref as pr
from offset_operands import carve, guards_intact
from polyblur_amd import _capi as capi

BND = {"fft": capi.PB_WRAP, "direct": capi.PB_ZERO}


@functools.lru_cache(maxsize=None)
def golden():
    return pr.load_golden()


def cases(kind):
    return [c for c in golden()[1] if c["kind"] == kind]


def cuda(a, **kw):
    import torch
    return torch.tensor(np.asarray(a), device="cuda", **kw)


def param(v, where="cuda", dtype=None, shape=()):
    import torch
    return torch.full(shape, float(v), dtype=dtype or torch.float32, device=where, requires_grad=True)


@functools.lru_cache(maxsize=None)
def poly_reference(name):
    """(case, image, weights, kernel, float64 golden, what reaches the polynomial: domain image, taps as applied, upstream gradient;
    the restatement's rows): computed once, shared, never written to"""
    z, cs = golden()
    c = next(c for c in cs if c["name"] == name)
    x, w = pr.smooth_image(c["seed"], tuple(c["xshape"]))
    k = z[name + "_k"]
    if c["func"] == "rank3":
        xp, kk, g, _ = ar.rank3_upstream(x, k, w, c["alpha"], c["beta"], c["method"])
        xp, kk, g = (np.ascontiguousarray(a, np.float32) for a in (xp, kk, g))
    else:
        xp, kk, g = x, k, w
    return c, x, w, k, z[name + "_g64"], (xp, kk, g), pr.poly_param_rows(xp, kk, g, c["method"])


def engine_poly_rows(xp, kk, g, c, offset=0):
    """pb_compute_polynomial_taps_params_backward on operands `offset` elements off a 16-byte boundary -> the (rows, 2) array"""
    import torch
    from polyblur_amd._frontend import bound_engine
    from polyblur_amd.nonblind import _check_kernel
    taps, eshape = _check_kernel(kk, c["method"], xp.shape, pad_domain=False, circular_only=False)
    bx, vx = carve(xp, offset)
    bg, vg = carve(g, offset)
    bo, vo = carve(np.zeros((eshape[0], 2), np.float32), offset)
    with bound_engine(vx) as eng:
        ks = eng.set_taps(taps)
        try:
            eng.compute_polynomial_taps_params_backward_ptr(vx.data_ptr(), vg.data_ptr(), vo.data_ptr(), eshape, ks, c["alpha"], c["beta"], BND[c["method"]])
        finally:
            ks.free()
    torch.cuda.synchronize()
    assert guards_intact(bo, vo) and guards_intact(bx, vx) and guards_intact(bg, vg)
    return vo.cpu().numpy()


POLY_NAMES = ["p%02d" % n for n in range(len(pr.POLY))]


# ---------------------------------------------------------------------------------------------
# the two entry points alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", POLY_NAMES)
def test_polynomial_entry_point_against_float64(name):
    c, x, w, k, g64, (xp, kk, g), want = poly_reference(name)
    rows = engine_poly_rows(xp, kk, g, c)
    scale = np.abs(want).max()
    err = float(np.abs(rows - want).max() / scale)
    tot = pr.rel_error(rows.astype(np.float64).sum(axis=0), g64)
    tol = pr.TOL_POLY[name]
    print("%s %-10s %s rows %.3g, sum against the float64 golden %.3g (tolerance %.3g)" % (name, c["func"], c["method"], err, tot, tol))
    assert rows.shape == want.shape and err <= tol and tot <= tol, (name, err, tot)
    # the same call gives the same bits; operands at element offsets 1, 2 and 3 give the aligned call's bits
    assert np.array_equal(engine_poly_rows(xp, kk, g, c).view(np.int32), rows.view(np.int32))
    for off in (1, 2, 3):
        assert np.array_equal(engine_poly_rows(xp, kk, g, c, off).view(np.int32), rows.view(np.int32)), (name, off)
    # the mutants the CPU test tells apart are told apart here too: the 1/2 dropped, the `+ x` dropped
    for m in (dict(half=1.0), dict(direct_term=False)):
        assert float(np.abs(rows - pr.poly_param_rows(xp, kk, g, c["method"], **m)).max() / scale) > 2 * tol


def test_polynomial_entry_point_refusals_and_scratch():
    import torch
    from polyblur_amd.engine import Engine, PolyblurHipError as PolyblurError
    x = cuda(np.random.default_rng(1).random((2, 3, 20, 24), dtype=np.float32))
    g, out = torch.ones_like(x), torch.zeros(2, 2, device="cuda")
    torch.cuda.synchronize()
    eng = Engine(0)                                                              # (a context of its own: its scratch starts empty)
    try:
        odd, even = eng.set_taps(np.full((2, 5, 5), 0.04, np.float32)), eng.set_taps(np.full((2, 4, 5), 0.05, np.float32))
        tall = eng.set_taps(np.full((2, 21, 3), 1 / 63, np.float32))
        try:
            before = eng.workspace_bytes()
            call = lambda xp, gp, op, ks=odd, shape=x.shape, bnd=capi.PB_WRAP: eng.compute_polynomial_taps_params_backward_ptr(xp, gp, op, shape, ks, 2, 3, bnd)
            for args in ((None, g.data_ptr(), out.data_ptr()), (x.data_ptr(), None, out.data_ptr()), (x.data_ptr(), g.data_ptr(), None),
                         (x.data_ptr(), g.data_ptr(), x.data_ptr()), (x.data_ptr(), g.data_ptr(), g.data_ptr())):
                with pytest.raises(PolyblurError, match="PB_ERR_BADARG"):
                    call(*args)
            with pytest.raises(PolyblurError, match="PB_ERR_UNSUPPORTED.*odd sides only"):
                call(x.data_ptr(), g.data_ptr(), out.data_ptr(), ks=even)
            with pytest.raises(PolyblurError, match="PB_ERR_BADARG.*does not fit"):
                call(x.data_ptr(), g.data_ptr(), out.data_ptr(), ks=tall)
            with pytest.raises(PolyblurError, match="PB_ERR_BADARG"):
                call(x.data_ptr(), g.data_ptr(), out.data_ptr(), shape=(3, 3, 20, 24))
            with pytest.raises(PolyblurError, match="PB_ERR_BADARG"):
                call(x.data_ptr(), g.data_ptr(), out.data_ptr(), bnd=7)
            assert eng.workspace_bytes() == before                               # every refusal came before any scratch, any launch
            call(x.data_ptr(), g.data_ptr(), out.data_ptr())
            eng.synchronize()
            # pb_workspace_bytes reports the scratch: two plane sets of the domain and the partials, beside what the passes keep
            plane = 2 * 3 * 20 * 24 * 4
            grown = eng.workspace_bytes() - before
            assert grown >= 2 * plane + 2 * 2 * 8, grown
            call(x.data_ptr(), g.data_ptr(), out.data_ptr())
            eng.synchronize()
            assert eng.workspace_bytes() - before == grown                       # (a second call allocates nothing)
        finally:
            for ks in (odd, even, tall):
                ks.free()
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def estimation_reference(name):
    z, cs = golden()
    c = next(c for c in cs if c["name"] == name)
    x, w = z[name + "_x"], z[name + "_w"]
    recs = er.estimate(x, pr.EST_C, pr.EST_B)
    return c, x, w, z[name + "_g32"], recs, pr.estimation_param_rows(recs, w)


def engine_estimation(x, w, offset=0, want_in=True, want_cb=True, old=False):
    """pb_estimate_blur then pb_estimate_blur_params_backward (old: pb_estimate_blur_backward) -> (grad_in or None, grad_cb or None)"""
    import torch
    from polyblur_amd._frontend import bound_engine
    from polyblur_amd.estimation import _F32
    B = x.shape[0]
    bx, vx = carve(x, offset)
    bk, vk = carve(np.ascontiguousarray(w.reshape(B, 25, 25)), offset)
    bi, vi = carve(np.zeros_like(x), offset)
    bc, vc = carve(np.full((B, 2), 7.0, np.float32), offset)
    rec = torch.empty((B, _F32), dtype=torch.float32, device="cuda")
    with bound_engine(vx) as eng:
        o = eng.make_options(c=pr.EST_C, b=pr.EST_B)
        eng.estimate_blur_ptr(vx.data_ptr(), capi.PB_F32, x.shape, o, rec.data_ptr())
        if old:
            eng.estimate_blur_backward_ptr(vx.data_ptr(), x.shape, o, rec.data_ptr(), vk.data_ptr(), None, 25, vi.data_ptr())
        else:
            eng.estimate_blur_params_backward_ptr(vx.data_ptr(), x.shape, o, rec.data_ptr(), vk.data_ptr(), None, 25,
                                                  vi.data_ptr() if want_in else None, vc.data_ptr() if want_cb else None)
    torch.cuda.synchronize()
    assert all(guards_intact(b, v) for b, v in ((bx, vx), (bk, vk), (bi, vi), (bc, vc)))
    if not want_in:
        assert not vi.any()                                                      # (the scatter was not launched: nothing written)
    if not want_cb or old:
        assert bool((vc == 7.0).all())
    return vi.cpu().numpy() if want_in else None, vc.cpu().numpy() if want_cb and not old else None


EST_NAMES = ["e%02d" % n for n in range(len(pr.ESTIMATION))]


@pytest.mark.parametrize("name", EST_NAMES)
def test_estimation_entry_point_against_float64(name):
    c, x, w, g32, recs, want = estimation_reference(name)
    gin_old, _ = engine_estimation(x, w, old=True)
    gin, cb = engine_estimation(x, w)
    _, cb_alone = engine_estimation(x, w, want_in=False)
    gin_alone, _ = engine_estimation(x, w, want_cb=False)
    # the old entry point is the new one with grad_cb = NULL; with both outputs each has the bits it has alone
    assert np.array_equal(gin.view(np.int32), gin_old.view(np.int32)) and np.array_equal(gin_alone.view(np.int32), gin_old.view(np.int32))
    assert np.array_equal(cb.view(np.int32), cb_alone.view(np.int32))
    for off in (1, 2, 3):
        gi, gc = engine_estimation(x, w, off)
        assert np.array_equal(gc.view(np.int32), cb.view(np.int32)) and np.array_equal(gi.view(np.int32), gin.view(np.int32)), (name, off)
    if all(all(f) for f in c["clamped"]):
        assert not cb.any() and not want.any() and not g32.any()                 # both variances clamped: exactly (0, 0)
        return
    scale = np.abs(want).max()
    err = float(np.abs(cb - want).max() / scale)
    tot = pr.rel_error(cb.astype(np.float64).sum(axis=0), want.sum(axis=0))
    tol = pr.TOL_EST[pr.est_setting(c)]
    print("%s rows %.3g, sum %.3g of the larger gradient (tolerance %.3g); against the reference's float32 %.3g"
          % (name, err, tot, tol, pr.rel_error(cb.astype(np.float64).sum(axis=0), g32)))
    assert err <= tol and tot <= tol, (name, err, tot)
    for m in (dict(gate=False),) if any(any(f) for f in c["clamped"]) else ():
        assert float(np.abs(cb - pr.estimation_param_rows(recs, w, **m)).max() / scale) > 2 * tol


def test_estimation_entry_point_refusals():
    import torch
    from polyblur_amd._frontend import bound_engine
    from polyblur_amd.engine import PolyblurHipError as PolyblurError
    from polyblur_amd.estimation import _F32
    x = cuda(er.blurred_noise(3, (1, 3, 16, 24)))
    gk, gin, cb = torch.ones(1, 25, 25, device="cuda"), torch.zeros_like(x), torch.zeros(1, 2, device="cuda")
    rec = torch.empty((1, _F32), dtype=torch.float32, device="cuda")
    with bound_engine(x) as eng:
        o = eng.make_options(c=pr.EST_C, b=pr.EST_B)
        eng.estimate_blur_ptr(x.data_ptr(), capi.PB_F32, x.shape, o, rec.data_ptr())
        call = lambda gi, gc, opts=o, k=25: eng.estimate_blur_params_backward_ptr(x.data_ptr(), x.shape, opts, rec.data_ptr(), gk.data_ptr(), None, k, gi, gc)
        with pytest.raises(PolyblurError, match="PB_ERR_BADARG.*pb_estimate_blur_params_backward: null argument"):
            call(None, None)
        with pytest.raises(PolyblurError, match="PB_ERR_BADARG"):
            call(x.data_ptr(), cb.data_ptr())
        with pytest.raises(PolyblurError, match="PB_ERR_BADARG.*grad_cb aliases"):
            call(gin.data_ptr(), gin.data_ptr())
        with pytest.raises(PolyblurError, match="PB_ERR_UNSUPPORTED.*q = "):
            call(None, cb.data_ptr(), opts=eng.make_options(c=pr.EST_C, b=pr.EST_B, q=1e-4))
        with pytest.raises(PolyblurError, match="PB_ERR_UNSUPPORTED.*ker_size 24"):
            call(None, cb.data_ptr(), k=24)
        with pytest.raises(PolyblurError, match="PB_ERR_BADARG.*pb_estimate_blur_backward: null argument"):
            eng.estimate_blur_backward_ptr(x.data_ptr(), x.shape, o, rec.data_ptr(), gk.data_ptr(), None, 25, None)
    torch.cuda.synchronize()
    assert not cb.any() and not gin.any()


# ---------------------------------------------------------------------------------------------
# the public functions
# ---------------------------------------------------------------------------------------------
def public_poly(c, x, k, w, alpha, beta, x_grad=False, k_grad=False):
    import polyblur_amd as pa
    xt, kt = cuda(x, requires_grad=x_grad), cuda(k, requires_grad=k_grad)
    if c["func"] == "polynomial":
        y = pa.compute_polynomial(xt, kt, alpha, beta, method=c["method"])
    else:
        y = pa.inverse_filtering_rank3(xt, kt, alpha, beta, method=c["method"])
    return xt, kt, y


@pytest.mark.parametrize("name", POLY_NAMES)
def test_public_polynomial_against_the_goldens(name):
    import torch
    c, x, w, k, g64, _, _ = poly_reference(name)
    # a 0-dim float32 parameter on the device and a (1,) float64 one on the CPU; only they require grad
    at, bt = param(c["alpha"]), param(c["beta"], "cpu", torch.float64, (1,))
    xt, kt, y = public_poly(c, x, k, w, at, bt)
    assert y.grad_fn is not None and y.requires_grad
    with torch.no_grad():                                                        # under no_grad a tensor is a number: the existing path
        assert torch.equal(public_poly(c, x, k, w, at, bt)[2], public_poly(c, x, k, w, c["alpha"], c["beta"])[2])
    # the forward under grad is the forward under grad with float(t), bit for bit
    assert torch.equal(y.detach(), public_poly(c, x, k, w, c["alpha"], c["beta"], x_grad=True)[2].detach())
    (y * cuda(w)).sum().backward()
    assert xt.grad is None and kt.grad is None                                   # the image is data: no image gradient
    assert at.grad.shape == at.shape and at.grad.dtype == torch.float32 and at.grad.is_cuda
    assert bt.grad.shape == bt.shape and bt.grad.dtype == torch.float64 and not bt.grad.is_cuda
    got = np.array([float(at.grad), float(bt.grad)])
    err = pr.rel_error(got, g64)
    print("%s %-10s %s (d alpha, d beta) = %s against the float64 golden: %.3g (tolerance %.3g)" % (name, c["func"], c["method"], got, err, pr.TOL_POLY[name]))
    assert err <= pr.TOL_POLY[name], (name, got, g64)
    # a parameter on the CPU and the same one on the device: the same value
    a2, b2 = param(c["alpha"], "cpu"), param(c["beta"], "cuda", torch.float64, (1,))
    (public_poly(c, x, k, w, a2, b2)[2] * cuda(w)).sum().backward()
    assert float(a2.grad) == float(at.grad) and float(b2.grad) == float(bt.grad)
    assert not a2.grad.is_cuda and b2.grad.is_cuda and b2.grad.dtype == torch.float64


@pytest.mark.parametrize("name", ["p02", "p06", "p07", "p10", "p13"])
def test_image_and_kernel_gradients_do_not_move(name):
    """grad_x and grad_taps of the existing backward, with and without a parameter asking: the same bits"""
    c, x, w, k, g64, _, _ = poly_reference(name)
    xt, kt, y = public_poly(c, x, k, w, c["alpha"], c["beta"], True, True)
    (y * cuda(w)).sum().backward()
    at, bt = param(c["alpha"]), param(c["beta"])
    x2, k2, y2 = public_poly(c, x, k, w, at, bt, True, True)
    (y2 * cuda(w)).sum().backward()
    assert np.array_equal(x2.grad.cpu().numpy().view(np.int32), xt.grad.cpu().numpy().view(np.int32))
    assert np.array_equal(k2.grad.cpu().numpy().view(np.int32), kt.grad.cpu().numpy().view(np.int32))
    assert pr.rel_error([float(at.grad), float(bt.grad)], g64) <= pr.TOL_POLY[name]
    # one parameter alone: the other stays a number
    a3 = param(c["alpha"])
    (public_poly(c, x, k, w, a3, c["beta"])[2] * cuda(w)).sum().backward()
    assert float(a3.grad) == float(at.grad)


@pytest.mark.parametrize("name", EST_NAMES)
def test_public_estimation_against_the_goldens(name):
    import torch
    import polyblur_amd as pa
    c, x, w, g32, recs, want = estimation_reference(name)
    ct, bt = param(pr.EST_C, "cpu"), param(pr.EST_B, "cuda", torch.float64, (1,))
    xt = cuda(x)
    k = pa.gaussian_blur_estimation(xt, q=0.0, c=ct, b=bt)
    assert k.grad_fn is not None and torch.equal(k.detach(), pa.gaussian_blur_estimation(xt, q=0.0, c=pr.EST_C, b=pr.EST_B))
    (k * cuda(w)).sum().backward()
    assert xt.grad is None                                                       # the calibration case: no image gradient
    assert ct.grad.shape == ct.shape and not ct.grad.is_cuda and bt.grad.shape == (1,) and bt.grad.is_cuda and bt.grad.dtype == torch.float64
    got, truth = np.array([float(ct.grad), float(bt.grad)]), want.sum(axis=0)
    if all(all(f) for f in c["clamped"]):
        assert not got.any() and not g32.any()
    else:
        e64, e32, key = pr.rel_error(got, truth), pr.rel_error(got, g32), pr.est_setting(c)
        print("%s (d c, d b) = %s: against float64 %.3g (tolerance %.3g), against the reference's float32 %.3g" % (name, got, e64, pr.TOL_EST[key], e32))
        assert e64 <= pr.TOL_EST[key] and e32 <= pr.TOL_EST[key] + pr.E_EST[key], (name, got, truth)
    # beside an image that requires grad: the image's gradient has the bits it has without the parameters
    x1, x2 = cuda(x, requires_grad=True), cuda(x, requires_grad=True)
    (pa.gaussian_blur_estimation(x1, q=0.0, c=pr.EST_C, b=pr.EST_B) * cuda(w)).sum().backward()
    c2 = param(pr.EST_C)
    (pa.gaussian_blur_estimation(x2, q=0.0, c=c2, b=pr.EST_B) * cuda(w)).sum().backward()
    assert np.array_equal(x1.grad.cpu().numpy().view(np.int32), x2.grad.cpu().numpy().view(np.int32)) and float(c2.grad) == float(ct.grad)
    # (sigma, rho) as outputs
    c3 = param(pr.EST_C)
    s, r, t = pa.gaussian_blur_estimation(xt, q=0.0, c=c3, b=pr.EST_B, return_2d_filters=False)
    assert s.grad_fn is not None and not t.requires_grad
    (s.sum() + r.sum()).backward()
    assert np.isfinite(float(c3.grad)) and (float(c3.grad) == 0.0) == all(all(f) for f in c["clamped"])


def blind_call(module, x, ps, c, **extra):
    import polyblur_amd as pa
    kw = dict(n_iter=c["n_iter"], c=ps[0], b=ps[1], alpha=ps[2], beta=ps[3], q=0.0, method=c["method"], **extra)
    return pa.PolyblurDeblurring()(x, **kw) if module else pa.polyblur_deblurring(x, **kw)


@pytest.mark.parametrize("module", [False, True])
def test_blind_gradients_against_the_goldens_and_float64(module):
    import torch
    z, _ = golden()
    for c in cases("blind"):
        x, w, g32 = z[c["name"] + "_x"], z[c["name"] + "_w"], z[c["name"] + "_g32"]
        truth = pr.blind_param_grads(x, w, c["n_iter"], c["alpha"], c["beta"], c["method"])
        ps = [param(pr.BLIND_C), param(pr.BLIND_B, "cpu"), param(c["alpha"], "cuda", torch.float64, (1,)), param(c["beta"], "cpu", torch.float64)]
        xt = cuda(x)
        y = blind_call(module, xt, ps, c)
        assert y.grad_fn is not None
        floats = [pr.BLIND_C, pr.BLIND_B, c["alpha"], c["beta"]]
        assert torch.equal(y.detach(), blind_call(module, cuda(x, requires_grad=True), floats, c).detach())     # the forward under grad with float(t)
        with torch.no_grad():
            assert torch.equal(blind_call(module, xt, ps, c), blind_call(module, xt, floats, c))
        (y * cuda(w)).sum().backward()
        assert xt.grad is None and all(p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device == p.device for p in ps)
        got = np.array([float(p.grad) for p in ps])
        e64, e32, key = pr.rel_error(got, truth), pr.rel_error(got, g32), pr.blind_setting(c)
        print("%s n_iter %d %s: against float64 %.3g (tolerance %.3g), against the reference's float32 %.3g" % (c["name"], c["n_iter"], c["method"], e64, pr.TOL_BLIND[key], e32))
        assert e64 <= pr.TOL_BLIND[key] and e32 <= pr.TOL_BLIND[key] + pr.E_BLIND[key], (c["name"], got, truth, g32)
        if c["n_iter"] > 1:                                                      # every iteration adds: the last one alone is somewhere else
            last = pr.blind_param_grads(x, w, c["n_iter"], c["alpha"], c["beta"], c["method"], last_only=True)
            assert pr.rel_error(got, last) > 2 * pr.TOL_BLIND[key]


@pytest.mark.parametrize("name", ["h00", "t00"])
def test_two_iterations_with_the_halo_mask_and_with_the_edgetaper(name):
    import torch
    z, cs = golden()
    c = next(c for c in cs if c["name"] == name)
    x, w, g32 = z[c["of"] + "_x"], z[c["of"] + "_w"], z[name + "_g32"]
    extra = {key: c[key] for key in ("remove_halo", "edgetaping") if key in c}
    ps = [param(v) for v in (pr.BLIND_C, pr.BLIND_B, c["alpha"], c["beta"])]
    xt = cuda(x, requires_grad=True)                                             # (beside an image that asks too)
    y = blind_call(False, xt, ps, c, **extra)
    (y * cuda(w)).sum().backward()
    got = np.array([float(p.grad) for p in ps])
    err, bound = pr.rel_error(got, g32), pr.TOL_BLIND[pr.blind_setting(c)] + pr.E_BLIND[pr.blind_setting(c)]
    print("%s %s (d c, d b, d alpha, d beta) = %s against the reference's float32: %.3g (bound %.3g)" % (name, extra, got, err, bound))
    assert xt.grad is not None and err <= bound, (name, got, g32)


def test_refusals_on_rocm_tensors():
    import torch
    import polyblur_amd as pa
    x, k = cuda(np.random.default_rng(2).random((1, 3, 16, 18), dtype=np.float32)), cuda(pr.make_kernel(5, (1, 1, 3, 5), "dense"))
    reason = "the gradients with respect to alpha and b are not built for the pure-phase filter"
    for what, call in (("compute_polynomial(not_symmetric=True)", lambda: pa.compute_polynomial(x, k, param(2), 3, not_symmetric=True)),
                       ("inverse_filtering_nonsymmetric", lambda: pa.inverse_filtering_nonsymmetric(x, k, b=param(4, "cpu")))):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == "%s has no backward pass: %s" % (what, reason)
    with torch.no_grad():                                                        # nothing asks: the pure-phase call runs with float(t)
        assert torch.equal(pa.compute_polynomial(x, k, param(2), 3, not_symmetric=True), pa.compute_polynomial(x, k, 2, 3, not_symmetric=True))
    with pytest.raises(NotImplementedError, match="alpha requires grad and the image is not a float32 ROCm tensor"):
        pa.inverse_filtering_rank3(x.half(), k, alpha=param(2))
    with pytest.raises(ValueError, match="one-element tensor"):
        pa.compute_polynomial(x, k, cuda([2.0, 3.0]), 3)
    with pytest.raises(NotImplementedError, match="odd sides only"):
        pa.compute_polynomial(x, cuda(np.full((1, 1, 4, 5), 0.05, np.float32)), param(2), 3)
    # a parameter lives on the CPU or on the image's device
    with pytest.raises(ValueError, match="alpha lives on cuda:0 and the image on cpu"):
        pa.compute_polynomial(x.cpu(), k.cpu(), cuda(2.0), 3)
    with pytest.raises(ValueError, match="c lives on cuda:0 and the image on the host"):
        pa.polyblur_deblurring(x.cpu().numpy()[0, 0], c=param(0.35))
    # a tensor that does not require grad is a number
    assert torch.equal(pa.compute_polynomial(x, k, cuda(2.0), torch.tensor([3.0], dtype=torch.float64)), pa.compute_polynomial(x, k, 2, 3))


def test_the_readmes_calibration_example_runs():
    """README: Adam on c and b over sharp / blurry pairs -- the pairs are data, the loss is finite, c and b move, no image gradient"""
    import torch
    from polyblur_amd import polyblur_deblurring
    pairs = [(cuda(pr.smooth_image(70 + s, (2, 3, 48, 64))[0]), cuda(er.blurred_noise(s, (2, 3, 48, 64), (1.6, 1.0)))) for s in range(3)]
    c = torch.tensor(0.35, requires_grad=True); b = torch.tensor(0.75, requires_grad=True)
    opt = torch.optim.Adam([c, b], lr=1e-2)
    for sharp, blurry in pairs:
        loss = (polyblur_deblurring(blurry, n_iter=1, c=c, b=b, alpha=6, beta=1) - sharp).square().mean()
        opt.zero_grad(); loss.backward(); opt.step()
        assert np.isfinite(float(loss.detach())) and blurry.grad is None and sharp.grad is None
        assert np.isfinite(float(c.grad)) and np.isfinite(float(b.grad)) and float(c.grad) != 0.0 and float(b.grad) != 0.0
    assert abs(float(c.detach()) - 0.35) > 1e-3 and abs(float(b.detach()) - 0.75) > 1e-3
