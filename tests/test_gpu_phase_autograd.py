"""Gradients of the polynomial with the pure-phase filter on the GPU: pb_compute_polynomial_phase_taps_backward
through the engine, and polyblur_amd.compute_polynomial(not_symmetric=True) / inverse_filtering_nonsymmetric under torch.autograd,
against the float64 restatement (tests/phase_grad_ref.py, which tests/test_phase_autograd_cpu.py pins to the reference's own
autograd) and against the reference's goldens (tests/golden/nonblind_phase_grad.npz).

Tolerances: pg.TOL, relative to the largest entry of the float64 gradient -- five times the reference's own float32 error against its
float64 gradients on these very inputs, per group (polynomial / chain; image, taps, grad_img).  The forward under grad is the no-grad
call's, bit for bit.
Shapes (padded sizes): 16 x 24 single-stage plans, 96 x 120 multi-stage direct plans, 48 x 55 / 55 x 48 Bluestein rows / columns,
97 x 101 prime sides, C = 1 .. 4 (an unpaired last plane), three images with three kernels, one kernel per plane, one kernel
broadcast over two images, kernels 3 x 49, 21 x 5, 8 x 8 (even), a 15 x 15 streak, (alpha, b) = (6, 1), and 2190 x 40 -- an
8192-point Bluestein core in the columns, the 1024-thread workgroup."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import phase_grad_ref as pg
import phase_ref as pr


def _cuda(a, grad=False):
    import torch
    return torch.tensor(np.asarray(a), device="cuda", requires_grad=grad)


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def golden():
    return pg.golden()


def engine_shape(c):
    """the shape and the (B', kh, kw) taps the engine takes for a case: one kernel per plane -> B C one-channel images"""
    B, C, H, W = c["x"].shape
    kb, kc, kh, kw = c["k"].shape
    taps = np.ascontiguousarray(np.broadcast_to(c["k"], (B, kc, kh, kw))).reshape(B * kc, kh, kw)
    return ((B * C, 1, H, W) if kc > 1 else (B, C, H, W)), taps


def engine_backward(eng, c, want_x=True, want_k=True):
    """pb_compute_polynomial_phase_taps_backward on a case -> (grad_x or None, grad_taps (B', kh, kw) or None) as arrays"""
    import torch
    eshape, taps = engine_shape(c)
    xt, gt = _cuda(c["x"]), _cuda(c["w"])
    gx = torch.full_like(xt, float("nan")) if want_x else None
    gk = torch.full(taps.shape, float("nan"), device="cuda") if want_k else None
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    ks = eng.set_taps(taps)
    try:
        eng.compute_polynomial_phase_taps_backward_ptr(xt.data_ptr(), gt.data_ptr(), gx.data_ptr() if want_x else None,
                                                       gk.data_ptr() if want_k else None, eshape, ks, c["alpha"], c["b"])
    finally:
        ks.free()
    return (None if gx is None else _np(gx)), (None if gk is None else _np(gk))


def fold(gk, kshape, B):
    """the engine's (B', kh, kw) tap gradient in the kernel's shape (the batch sum of a broadcast kernel in float64)"""
    gk = np.asarray(gk, np.float64).reshape(B, kshape[1], kshape[2], kshape[3])
    return gk.sum(axis=0, keepdims=True) if kshape[0] == 1 and B > 1 else gk


@pytest.fixture(scope="module")
def eng():
    from polyblur_amd.engine import get_engine
    return get_engine(0)


def public_gradients(c, grad_x=True, grad_k=True):
    import torch
    import polyblur_amd as pa
    xt, kt = _cuda(c["x"], grad_x), _cuda(c["k"], grad_k)
    y = pa.compute_polynomial(xt, kt, c["alpha"], c["b"], method="fft", not_symmetric=True)
    assert y.requires_grad and y.grad_fn is not None
    (y * _cuda(c["w"])).sum().backward()
    with torch.no_grad():
        quiet = pa.compute_polynomial(xt, kt, c["alpha"], c["b"], method="fft", not_symmetric=True)
    assert not quiet.requires_grad and torch.equal(quiet, y.detach())          # the forward under grad: the no-grad call's bits
    if grad_k:
        assert kt.grad.shape == kt.shape and kt.grad.dtype == kt.dtype and kt.grad.is_cuda
    return _np(y), (_np(xt.grad) if grad_x else None), (_np(kt.grad) if grad_k else None)


# ---------------------------------------------------------------------------------------------
# against float64 and the goldens
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pg.POLY_NAMES)
def test_compute_polynomial_gradients(name):
    c = pg.poly_case(name)
    wx, wk = pg.poly_want(name)
    y, gx, gk = public_gradients(c)
    ey = float(np.abs(y - pg.forward(c["x"], c["k"], c["alpha"], c["b"])).max())
    ex, ek = pg.rel_error(gx, wx), pg.rel_error(gk, wk)
    print("%-28s forward %.3g | grad_x %.3g (tolerance %.3g) | grad_k %.3g (tolerance %.3g)" % (name, ey, ex, pg.TOL["poly_x"], ek, pg.TOL["poly_k"]))
    assert ey < 2e-5, (name, ey)
    assert ex <= pg.TOL["poly_x"], (name, ex)
    assert ek <= pg.TOL["poly_k"], (name, ek)
    if name in pg.GOLDEN_POLY:
        d, _ = golden()
        gex, gek = pg.rel_error(gx, d[name + "_dx"]), pg.rel_error(gk, d[name + "_dk"])
        print("%-28s against the reference's float64 autograd: grad_x %.3g grad_k %.3g" % (name, gex, gek))
        assert gex <= pg.TOL["poly_x"] and gek <= pg.TOL["poly_k"], (name, gex, gek)


def test_long_bluestein_columns(eng):
    """2190 x 40: the columns on an 8192-point Bluestein core, two to a 1024-thread workgroup -- the entry point against the
    restatement (its float64 gradients fit no golden)"""
    c = pg.poly_case(pg.LONG)
    wx, wk = pg.poly_want(pg.LONG)
    gx, gk = engine_backward(eng, c)
    ex, ek = pg.rel_error(gx, wx), pg.rel_error(fold(gk, c["k"].shape, c["x"].shape[0]), wk)
    print("%-28s grad_x %.3g (tolerance %.3g) | grad_k %.3g (tolerance %.3g)" % (pg.LONG, ex, pg.TOL["poly_x"], ek, pg.TOL["poly_k"]))
    assert ex <= pg.TOL["poly_x"] and ek <= pg.TOL["poly_k"], (ex, ek)


@pytest.mark.parametrize("name", [c[0] for c in pg.CHAIN_CASES])
def test_chain_gradients(name):
    """inverse_filtering_nonsymmetric under grad: pad -> polynomial -> crop -> [mask] -> clamp; with remove_halo=True a caller's
    grad_img that requires grad, or grad_img=None (the image's own gradients, inside the graph)"""
    import torch
    import polyblur_amd as pa
    c = pg.chain_case(name)
    want = pg.chain_want(name)
    xt, kt = _cuda(c["x"], True), _cuda(c["k"], True)
    gs = None if c["grad_img"] is None else tuple(_cuda(a, True) for a in c["grad_img"])
    y = pa.inverse_filtering_nonsymmetric(xt, kt, c["alpha"], c["b"], correlate=c["correlate"], remove_halo=c["remove_halo"], grad_img=gs)
    assert y.requires_grad and y.grad_fn is not None
    (y * _cuda(c["w"])).sum().backward()
    with torch.no_grad():
        fused = pa.inverse_filtering_nonsymmetric(xt, kt, c["alpha"], c["b"], correlate=c["correlate"], remove_halo=c["remove_halo"], grad_img=gs)
    assert float((fused - y.detach()).abs().max()) < 2e-5               # (the fused no-grad chain: the same values)
    got = {"x": _np(xt.grad), "k": _np(kt.grad)}
    if gs is not None:
        got.update(gx=_np(gs[0].grad), gy=_np(gs[1].grad))
    d, _ = golden()
    for n, tol in (("x", "chain_x"), ("k", "chain_k"), ("gx", "chain_g"), ("gy", "chain_g")):
        if n not in got:
            continue
        e, ge = pg.rel_error(got[n], want[n]), pg.rel_error(got[n], d["%s_d%s" % (name, n)])
        print("%-22s grad_%-2s %.3g, against the golden %.3g (tolerance %.3g)" % (name, n, e, ge, pg.TOL[tol]))
        assert e <= pg.TOL[tol] and ge <= pg.TOL[tol], (name, n, e, ge)


def test_chain_with_a_constant_grad_img():
    """remove_halo=True with a caller's grad_img that does not require grad: the same image and kernel gradients, none for the planes"""
    import polyblur_amd as pa
    name = "chain_halo_built"
    c, want = pg.chain_case(name), pg.chain_want(name)
    xt, kt = _cuda(c["x"], True), _cuda(c["k"], True)
    gs = tuple(_cuda(a) for a in c["grad_img"])
    y = pa.inverse_filtering_nonsymmetric(xt, kt, c["alpha"], c["b"], remove_halo=True, grad_img=gs)
    (y * _cuda(c["w"])).sum().backward()
    assert gs[0].grad is None and gs[1].grad is None
    assert pg.rel_error(_np(xt.grad), want["x"]) <= pg.TOL["chain_x"] and pg.rel_error(_np(kt.grad), want["k"]) <= pg.TOL["chain_k"]


# ---------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["single_stage_16x24", "bluestein_cols_55x48_c4", "one_kernel_per_plane", "k8x8"])
def test_shares_of_the_full_call_and_repeats(eng, name):
    """grad_x only and grad_taps only are bit-equal to their share of the full call (a NULL output changes no bit of the other), and
    the same call twice gives the same bits"""
    c = pg.poly_case(name)
    gx, gk = engine_backward(eng, c)
    assert np.isfinite(gx).all() and np.isfinite(gk).all()
    only_x, none_k = engine_backward(eng, c, want_k=False)
    none_x, only_k = engine_backward(eng, c, want_x=False)
    assert none_k is None and none_x is None
    assert np.array_equal(only_x, gx) and np.array_equal(only_k, gk)
    again = engine_backward(eng, c)
    assert np.array_equal(again[0], gx) and np.array_equal(again[1], gk)


def test_operands_at_an_element_offset(eng):
    """no access is wider than its element: every operand one to three floats off its allocation gives the aligned call's bits"""
    import torch
    c = pg.poly_case("bluestein_rows_48x55_c1")
    gx, gk = engine_backward(eng, c)
    eshape, taps = engine_shape(c)

    def off(a, n, fill=None):
        a = np.asarray(a, np.float32)
        buf = torch.full((a.size + n,), float("nan"), device="cuda")
        view = buf[n:].view(a.shape)
        if fill is None:
            view.copy_(_cuda(a))
        return buf, view
    (_, xt), (_, gt), (_, ox), (_, ok) = off(c["x"], 1), off(c["w"], 3), off(gx, 1, 0), off(gk, 2, 0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    ks = eng.set_taps(taps)
    try:
        eng.compute_polynomial_phase_taps_backward_ptr(xt.data_ptr(), gt.data_ptr(), ox.data_ptr(), ok.data_ptr(), eshape, ks, c["alpha"], c["b"])
    finally:
        ks.free()
    assert np.array_equal(_np(ox), gx) and np.array_equal(_np(ok), gk)


@pytest.mark.parametrize("grads", [(True, False), (False, True)], ids=["image", "kernel"])
def test_only_what_requires_grad(grads):
    c = pg.poly_case("alpha6_b1")
    _, gx, gk = public_gradients(c, *grads)
    _, fx, fk = public_gradients(c)
    assert (gx is None) != grads[0] and (gk is None) != grads[1]
    assert np.array_equal(gx, fx) if grads[0] else np.array_equal(gk, fk)


def test_an_image_does_not_depend_on_the_batch(eng):
    c = pg.poly_case("three_images_three_kernels")
    gx, gk = engine_backward(eng, c)
    for i in range(3):
        lone = dict(c, x=c["x"][i:i + 1], k=c["k"][i:i + 1], w=c["w"][i:i + 1])
        lx, lk = engine_backward(eng, lone)
        assert np.array_equal(lx, gx[i:i + 1]) and np.array_equal(lk, gk[i:i + 1]), i


def test_scratch_does_not_collide_with_other_calls():
    """a plain and a blind call between the forward and the backward, and between two backward calls: the same bits"""
    import torch
    import polyblur_amd as pa
    c = pg.poly_case("streak_15x15")
    _, gx, gk = public_gradients(c)
    xt, kt = _cuda(c["x"], True), _cuda(c["k"], True)
    y = pa.compute_polynomial(xt, kt, c["alpha"], c["b"], not_symmetric=True)
    other, ok = pr.case_inputs(("other", (1, 3, 96, 80), 8501, (5, 5), 8502, 1, 1, "dense"))
    with torch.no_grad():
        pa.inverse_filtering_rank3(_cuda(other), _cuda(ok), 2, 3, method="fft")
        pa.inverse_filtering_nonsymmetric(_cuda(other), _cuda(ok), 2, 3)
        pa.polyblur_deblurring(_cuda(other), n_iter=2, remove_halo=True)
    (y * _cuda(c["w"])).sum().backward()
    assert np.array_equal(_np(xt.grad), gx) and np.array_equal(_np(kt.grad), gk)


def test_phase_budget_and_workspace():
    """a budget of one byte: groups of a single plane pair -- two groups for C = 4 -- give the bits of the default budget, which
    holds both pairs in one group; pb_workspace_bytes reports the scratch DESIGN.md 4.14 states: with grad_taps the planes of K
    and A and, per pair of a group, one of g and one of x; without, K and one of g per pair (units of 256 bytes)"""
    import torch
    from polyblur_amd.engine import Engine
    c = pg.poly_case("bluestein_cols_55x48_c4")
    H, W = c["x"].shape[-2:]
    plane = 8 * H * W
    up = lambda n: (n + 255) // 256 * 256
    outs = []
    for budget, pairs in ((0, 2), (1, 1)):
        e = Engine(0)
        try:
            e.set_phase_budget(budget)
            e.set_stream(torch.cuda.current_stream().cuda_stream)
            # (the forward first: the two line plans' tables are the context's from then on, and its scratch is its own)
            eshape, taps = engine_shape(c)
            ks, xt = e.set_taps(taps), _cuda(c["x"])
            e.compute_polynomial_taps_ptr(xt.data_ptr(), torch.empty_like(xt).data_ptr(), eshape, ks, c["alpha"], c["b"], not_symmetric=True)
            ks.free()
            before = e.workspace_bytes()
            only_x = engine_backward(e, c, want_k=False)[0]
            e.synchronize()
            assert e.workspace_bytes() - before == up(plane) + up(pairs * plane), (budget, e.workspace_bytes() - before)
            outs.append(engine_backward(e, c))
            e.synchronize()
            assert e.workspace_bytes() - before == 2 * up(plane) + 2 * up(pairs * plane), (budget, e.workspace_bytes() - before)
            assert np.array_equal(only_x, outs[-1][0])
        finally:
            e.close()
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_c_abi_refusals(eng):
    """bad arguments and unsupported sides are refused before any launch: the outputs keep their NaN fill"""
    import torch
    from polyblur_amd._capi import PolyblurHipError
    c = pg.poly_case("single_stage_16x24")
    eshape, taps = engine_shape(c)
    xt, gt = _cuda(c["x"]), _cuda(c["w"])
    gx = torch.full_like(xt, float("nan"))
    gk = torch.full(taps.shape, float("nan"), device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    ks = eng.set_taps(taps)
    call = lambda *a, shape=eshape: eng.compute_polynomial_phase_taps_backward_ptr(*a, shape, ks, 2, 3)
    try:
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG.*both null"):
            call(xt.data_ptr(), gt.data_ptr(), None, None)
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG.*grad_out is null"):
            call(xt.data_ptr(), None, gx.data_ptr(), gk.data_ptr())
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG.*needs x"):
            call(None, gt.data_ptr(), None, gk.data_ptr())
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG.*aliases"):
            call(xt.data_ptr(), gt.data_ptr(), xt.data_ptr(), gk.data_ptr())
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
            call(xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), gk.data_ptr(), shape=(2,) + tuple(eshape[1:]))      # one kernel, two images
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
            call(xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), gk.data_ptr(), shape=(1, 3, 5, 24))                  # 5 rows > 5 - 1
        with pytest.raises(PolyblurHipError, match="PB_ERR_UNSUPPORTED"):
            call(xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), gk.data_ptr(), shape=(1, 1, 8, 8209))                # 8209 is prime: not held in LDS
        eng.synchronize()
        assert bool(torch.isnan(gx).all()) and bool(torch.isnan(gk).all())
    finally:
        ks.free()


def test_public_refusals_beside_a_rocm_tensor():
    import torch
    import polyblur_amd as pa
    c = pg.poly_case("single_stage_16x24")
    xt, kt = _cuda(c["x"], True), _cuda(c["k"], True)
    cases = [
        ("float32 images", lambda: pa.inverse_filtering_nonsymmetric(xt.detach().half(), kt, 2, 3)),
        ("kernel requires grad and is a CPU tensor", lambda: pa.compute_polynomial(xt, torch.tensor(c["k"], requires_grad=True), 2, 3, not_symmetric=True)),
        ("img requires grad and is a CPU tensor", lambda: pa.inverse_filtering_nonsymmetric(torch.tensor(c["x"], requires_grad=True), kt, 2, 3)),
        ("edgetaper is not differentiated", lambda: pa.inverse_filtering_nonsymmetric(xt, kt, 2, 3, do_edgetaper=True)),
        ("halo masking is differentiated for float32 ROCm tensors only",
         lambda: pa.inverse_filtering_nonsymmetric(xt, kt, 2, 3, remove_halo=True, grad_img=(c["x"], c["x"]))),
        ("not held in LDS", lambda: pa.compute_polynomial(torch.zeros(1, 1, 8, 8209, device="cuda", requires_grad=True), kt[:, :, :, :3], 2, 3, not_symmetric=True)),
    ]
    for reason, call in cases:
        with pytest.raises(NotImplementedError, match=reason):
            call()


# ---------------------------------------------------------------------------------------------
# the use case: fit a PSF that is not point-symmetric to a sharp / blurry pair
# ---------------------------------------------------------------------------------------------
def test_a_short_fit_lowers_the_loss():
    """a few Adam steps on a streak PSF from a wrong start (the README's snippet)"""
    import torch
    from polyblur_amd import convolve2d, inverse_filtering_nonsymmetric
    from polyblur_amd.synthetic import synthetic_blurry_batch
    sharp = torch.tensor(0.2 + 0.6 * synthetic_blurry_batch(1, 3, 96, 128, seed0=8800)[0].astype(np.float32), device="cuda")
    true_psf = torch.tensor(pr.streak_kernel((9, 9), 8801), device="cuda")
    with torch.no_grad():
        blurry = convolve2d(sharp, true_psf, method="fft")
    logits = torch.zeros(1, 1, 9, 9, device="cuda", requires_grad=True)             # the wrong start: a flat PSF
    opt = torch.optim.Adam([logits], lr=0.2)
    losses = []
    for _ in range(6):
        psf = torch.softmax(logits.flatten(), 0).view(1, 1, 9, 9)
        restored = inverse_filtering_nonsymmetric(blurry, psf, alpha=2, b=3)
        loss = ((restored - sharp) ** 2).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("fit:", " ".join("%.5f" % v for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
