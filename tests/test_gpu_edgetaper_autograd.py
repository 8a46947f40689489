"""The differentiable edgetaper on the GPU: pb_edgetaper_taps_backward alone against the float64 restatement
(tests/edgetaper_grad_ref.py, which tests/test_edgetaper_autograd_cpu.py pins to the reference's own autograd), and edgetaper,
inverse_filtering_rank3(do_edgetaper=True) and polyblur_deblurring(edgetaping=True) under torch.autograd against the reference's goldens.

Tolerances, relative to the largest entry of the float64 gradient: eg.TOL_ET_X / eg.TOL_ET_K for the blends, eg.TOL_CHAIN_X /
eg.TOL_CHAIN_K for the rank-3 chain -- 6 x the reference's own float32 error per group (edgetaper_grad_ref's table); the blind cases
take blind_tolerance of tests/test_gpu_blind_autograd.py plus the goldens' own float32 error (er.BOUND_GOLDEN); forwards under grad
against the fused no-grad call: TOL_FWD of tests/test_gpu_autograd.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import autograd_ref as ar
import edgetaper_grad_ref as eg
import estimation_grad_ref as er
from polyblur_amd import _capi as capi
from test_gpu_autograd import TOL_FWD
from test_gpu_blind_autograd import blind_tolerance

BND = {"fft": capi.PB_WRAP, "direct": capi.PB_ZERO}
ENTRY_CASES = [c[0] for c in eg.TAPER_CASES + eg.EXTRA_CASES]


@functools.lru_cache(maxsize=None)
def reference(name):
    """float64 (image gradient, tap gradient) of a case: computed once, shared, never written to"""
    c = eg.taper_case(name)
    return eg.backward(c["x"], c["k"], c["w"], c["method"], c["n"])


def cuda(a, **kw):
    import torch
    return torch.tensor(np.asarray(a), device="cuda", **kw)


def entry(c, want_x=True, want_k=True, eng=None):
    """pb_edgetaper_taps_backward on a case -> (grad_x or None, grad_taps folded to kernel.shape or None), numpy"""
    import torch
    from polyblur_amd.engine import get_engine
    x, k, w = c["x"], c["k"], c["w"]
    B, C, H, W = x.shape
    kb, kc, kh, kw = k.shape
    eshape = (B * C, 1, H, W) if kc > 1 else (B, C, H, W)
    taps = np.ascontiguousarray(np.broadcast_to(k, (B, kc, kh, kw))).reshape(B * kc, kh, kw)
    if eng is None:
        eng = get_engine(0)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
    xt, gt = cuda(x), cuda(w)
    gx = torch.full(x.shape, float("nan"), device="cuda") if want_x else None
    gk = torch.full(taps.shape, float("nan"), device="cuda") if want_k else None
    ks = eng.set_taps(taps)
    try:
        eng.edgetaper_taps_backward_ptr(xt.data_ptr(), gt.data_ptr(), gx.data_ptr() if want_x else None, gk.data_ptr() if want_k else None,
                                        eshape, ks, BND[c["method"]], c["n"])
    finally:
        ks.free()
    if want_k:
        gk = gk.cpu().numpy().reshape(B, kc, kh, kw)
        gk = gk.sum(0, keepdims=True) if kb == 1 and B > 1 else gk
    return (gx.cpu().numpy() if want_x else None), gk


def public(c, **kw):
    """edgetaper under grad -> (output, x.grad, kernel.grad), numpy"""
    import polyblur_amd as pa
    xt, kt = cuda(c["x"], requires_grad=True), cuda(c["k"], requires_grad=True)
    y = pa.edgetaper(xt, kt, n_tapers=c["n"], method=c["method"], **kw)
    assert y.requires_grad and y.grad_fn is not None
    (y * cuda(c["w"])).sum().backward()
    return y.detach(), xt.grad.cpu().numpy(), kt.grad.cpu().numpy()


# ---------------------------------------------------------------------------------------------
# the engine entry against float64
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ENTRY_CASES)
def test_engine_entry_against_float64(name):
    c = eg.taper_case(name)
    want_x, want_k = reference(name)
    gx, gk = entry(c)
    assert np.isfinite(gx).all() and np.isfinite(gk).all()
    if c["n"] == 0:                                           # the copy path
        assert np.array_equal(gx, c["w"]) and not gk.any() and not want_k.any()
        return
    ex, ek = eg.rel_error(gx, want_x), eg.rel_error(gk, want_k)
    print("%-18s image %.3g (tolerance %.3g) | taps %.3g (tolerance %.3g)" % (name, ex, eg.TOL_ET_X, ek, eg.TOL_ET_K))
    assert ex <= eg.TOL_ET_X and ek <= eg.TOL_ET_K, (name, ex, ek)


@pytest.mark.parametrize("name", ["t0_ends_overlap", "t2_wide_31", "x1_per_plane"])
def test_a_null_output_changes_no_bit_of_the_other(name):
    c = eg.taper_case(name)
    gx, gk = entry(c)
    only_x, none_k = entry(c, want_k=False)
    none_x, only_k = entry(c, want_x=False)
    assert none_k is None and none_x is None
    assert np.array_equal(gx, only_x) and np.array_equal(gk, only_k)


@pytest.mark.parametrize("name", ["t1_tall_direct", "t5_ring_inside"])
def test_two_identical_backward_calls_give_identical_bits(name):
    c = eg.taper_case(name)
    a, b = entry(c), entry(c)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    p, q = public(c), public(c)
    assert np.array_equal(p[1], q[1]) and np.array_equal(p[2], q[2])


# ---------------------------------------------------------------------------------------------
# the public functions against the reference's goldens
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eg.GOLDEN_TAPER)
def test_edgetaper_against_the_goldens_and_the_bits_without_grad(name):
    import torch
    import polyblur_amd as pa
    d, table, _ = eg.read_golden()
    c = eg.taper_case(name)
    y, gx, gk = public(c)
    with torch.no_grad():
        quiet = pa.edgetaper(cuda(c["x"], requires_grad=True), cuda(c["k"]), n_tapers=c["n"], method=c["method"])
    assert not quiet.requires_grad and torch.equal(quiet, y)
    ex, ek = eg.rel_error(gx, d[name + "_dx"]), eg.rel_error(gk, d[name + "_dk"])
    print("%-18s image %.3g (tolerance %.3g, reference float32 %.3g) | kernel %.3g (tolerance %.3g, reference float32 %.3g)"
          % (name, ex, eg.TOL_ET_X, table[name]["E_x"], ek, eg.TOL_ET_K, table[name]["E_k"]))
    assert ex <= eg.TOL_ET_X and ek <= eg.TOL_ET_K, (name, ex, ek)


def test_only_the_image_or_only_the_kernel_requires_grad():
    import polyblur_amd as pa
    c = eg.taper_case("t4_two_channels")
    _, gx, gk = public(c)
    xt = cuda(c["x"], requires_grad=True)
    (pa.edgetaper(xt, cuda(c["k"]), n_tapers=c["n"], method=c["method"]) * cuda(c["w"])).sum().backward()
    kt = cuda(c["k"], requires_grad=True)
    (pa.edgetaper(cuda(c["x"]), kt, n_tapers=c["n"], method=c["method"]) * cuda(c["w"])).sum().backward()
    assert np.array_equal(xt.grad.cpu().numpy(), gx) and np.array_equal(kt.grad.cpu().numpy(), gk)


@pytest.mark.parametrize("name", [c[0] for c in eg.CHAIN_CASES])
def test_rank3_with_edgetaper_against_the_goldens(name):
    import torch
    import polyblur_amd as pa
    d, table, _ = eg.read_golden()
    c = eg.chain_case(name)
    kw = dict(correlate=c["correlate"], do_edgetaper=True, method=c["method"])
    xt, kt = cuda(c["x"], requires_grad=True), cuda(c["k"], requires_grad=True)
    y = pa.inverse_filtering_rank3(xt, kt, eg.ALPHA, eg.BETA, **kw)
    assert y.requires_grad and y.grad_fn is not None
    (y * cuda(c["w"])).sum().backward()
    with torch.no_grad():
        quiet = pa.inverse_filtering_rank3(xt, kt, eg.ALPHA, eg.BETA, **kw)
    efwd = float((y.detach() - quiet).abs().max())
    ex, ek = eg.rel_error(xt.grad.cpu().numpy(), d[name + "_dx"]), eg.rel_error(kt.grad.cpu().numpy(), d[name + "_dk"])
    print("%-14s forward under grad vs the fused call %.3g (tolerance %.3g) | image %.3g (tolerance %.3g) | kernel %.3g (tolerance %.3g)"
          % (name, efwd, TOL_FWD, ex, eg.TOL_CHAIN_X, ek, eg.TOL_CHAIN_K))
    assert efwd <= TOL_FWD
    assert ex <= eg.TOL_CHAIN_X and ek <= eg.TOL_CHAIN_K, (name, ex, ek)


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_forward_with_the_halo_mask_agrees_with_the_fused_call(method):
    """the mask's image is the tapered, cropped one, its gradients its own (deblurring.py:236-238)"""
    import torch
    import polyblur_amd as pa
    x, w, k = ar.case_inputs(77, (2, 3, 24, 30), (1, 1, 5, 9))
    xt, kt = cuda(x, requires_grad=True), cuda(k, requires_grad=True)
    y = pa.inverse_filtering_rank3(xt, kt, 2, 3, remove_halo=True, do_edgetaper=True, method=method)
    with torch.no_grad():
        quiet = pa.inverse_filtering_rank3(xt, kt, 2, 3, remove_halo=True, do_edgetaper=True, method=method)
    efwd = float((y.detach() - quiet).abs().max())
    print("remove_halo + do_edgetaper, %s: forward under grad vs the fused call %.3g (tolerance %.3g)" % (method, efwd, TOL_FWD))
    assert efwd <= TOL_FWD
    (y * cuda(w)).sum().backward()
    assert torch.isfinite(xt.grad).all() and torch.isfinite(kt.grad).all() and float(kt.grad.abs().max()) > 0


@pytest.mark.parametrize("module", [False, True])
def test_blind_with_edgetaping_against_the_goldens(module):
    import torch
    import polyblur_amd as pa
    d, _, blind = eg.read_golden()
    for c in blind:
        x, w, gx = d[c["name"] + "_x"], d[c["name"] + "_w"], d[c["name"] + "_gx"]
        n_iter, alpha, beta, method = c["n_iter"], c["alpha"], c["beta"], c["method"]
        xt = cuda(x, requires_grad=True)
        if module:
            y = pa.PolyblurDeblurring()(xt, n_iter=n_iter, alpha=alpha, beta=beta, b=0.768, sigma_r=0.8, edgetaping=True, method=method)
        else:
            y = pa.polyblur_deblurring(xt, n_iter=n_iter, alpha=alpha, beta=beta, edgetaping=True, method=method)
        assert y.requires_grad and y.grad_fn is not None
        (y * cuda(w)).sum().backward()
        g = xt.grad.cpu().numpy()
        with torch.no_grad():
            quiet = pa.polyblur_deblurring(xt, n_iter=n_iter, alpha=alpha, beta=beta, edgetaping=True, method=method)
        efwd = float((y.detach() - quiet).abs().max())
        eref = float(np.max(np.abs(g - gx) / (blind_tolerance(gx, n_iter) + er.BOUND_GOLDEN * np.abs(gx).max(axis=(1, 2, 3), keepdims=True))))
        print("%s %s n_iter %d: forward under grad vs no_grad %.3g (tolerance %.3g) | gradient %.3g of its tolerance against the reference's "
              "float32 (%.3g abs, max |grad| %.3g)" % (c["name"], method, n_iter, efwd, TOL_FWD * n_iter, eref, np.abs(g - gx).max(), np.abs(gx).max()))
        assert efwd <= TOL_FWD * n_iter, (c, efwd)
        assert eref <= 1.0, (c, eref)


# ---------------------------------------------------------------------------------------------
# the engine against itself
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t1_tall_direct", "t2_wide_31", "t5_ring_inside"])
def test_adjoint_identity(name):
    """<E x, y> == <x, E^T y> with the kernel fixed: the blends are linear in the image.  Both dot products in float64 on the host; the
    bound is the one tests/test_gpu_autograd.py holds convolve2d's identity to"""
    import polyblur_amd as pa
    c = eg.taper_case(name)
    x, g = c["x"], c["w"]
    xt = cuda(x, requires_grad=True)
    y = pa.edgetaper(xt, cuda(c["k"]), n_tapers=c["n"], method=c["method"])
    y.backward(cuda(g))
    lhs = np.vdot(y.detach().cpu().numpy().astype(np.float64), g.astype(np.float64))
    rhs = np.vdot(x.astype(np.float64), xt.grad.cpu().numpy().astype(np.float64))
    bound = 2e-5 * np.abs(g).sum(dtype=np.float64) + 4e-5 * np.abs(x).sum(dtype=np.float64)
    print("adjoint identity", name, "difference %.3g (bound %.3g)" % (abs(lhs - rhs), bound))
    assert abs(lhs - rhs) <= bound


def test_a_call_between_forward_and_backward_changes_nothing():
    import torch
    import polyblur_amd as pa
    c = eg.taper_case("t0_ends_overlap")
    _, want_x, want_k = public(c)
    xt, kt = cuda(c["x"], requires_grad=True), cuda(c["k"], requires_grad=True)
    y = pa.edgetaper(xt, kt, n_tapers=c["n"], method=c["method"])
    other = eg.taper_case("t2_wide_31")
    with torch.no_grad():                                   # a bystander with other shapes, taps and scratch sizes
        pa.edgetaper(cuda(other["x"]), cuda(other["k"]), method="fft")
        pa.inverse_filtering_rank3(cuda(other["x"]), cuda(other["k"]), 2, 3, do_edgetaper=True, method="fft")
    (y * cuda(c["w"])).sum().backward()
    assert np.array_equal(xt.grad.cpu().numpy(), want_x) and np.array_equal(kt.grad.cpu().numpy(), want_k)


def test_workspace_grows_by_the_documented_scratch():
    """image only: three plane sets ("etg.u", "etg.ag", "etg.g"); with the taps n_tapers + 3, one plane per image ("etg.abar"),
    B * (H + W) floats ("etg.vbar") and the partial tables -- each rounded up to 256 bytes"""
    import torch
    from polyblur_amd.engine import Engine
    c = eg.taper_case("t2_wide_31")                          # (tap tables: the passes themselves take no scratch)
    x, k, n = c["x"], c["k"], c["n"]
    B, C, H, W = x.shape
    kh, kw = k.shape[-2:]
    eng = Engine(0)
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        xt, gt = cuda(x), cuda(c["w"])
        out, gx = torch.empty_like(xt), torch.empty_like(xt)
        gk = torch.empty((B, kh, kw), device="cuda")
        ks = eng.set_taps(k.reshape(B, kh, kw))
        eng.edgetaper_taps_ptr(xt.data_ptr(), out.data_ptr(), x.shape, ks, capi.PB_WRAP, n)
        before = eng.workspace_bytes()
        r256 = lambda v: (v + 255) // 256 * 256
        plane_set = r256(4 * B * C * H * W)
        eng.edgetaper_taps_backward_ptr(None, gt.data_ptr(), gx.data_ptr(), None, x.shape, ks, capi.PB_WRAP, n)
        assert eng.workspace_bytes() - before == 3 * plane_set
        eng.edgetaper_taps_backward_ptr(xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), gk.data_ptr(), x.shape, ks, capi.PB_WRAP, n)
        eng.synchronize()
        tiles = C * ((H + 31) // 32) * ((W + 31) // 32)
        G = min(tiles, max(1, 1024 // B))
        assert eng.workspace_bytes() - before == (4 * plane_set + r256(4 * (n - 1) * B * C * H * W) + r256(4 * B * H * W) + r256(4 * B * (H + W))
                                                  + r256(4 * B * G * kh * kw))
        ks.free()
    finally:
        eng.close()


def test_what_the_c_abi_refuses():
    import torch
    from polyblur_amd.engine import Engine
    c = eg.taper_case("t0_ends_overlap")
    x, k = c["x"], c["k"]
    B, C, H, W = x.shape
    kh, kw = k.shape[-2:]
    eng = Engine(0)
    try:
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        xt, gt, gx = cuda(x), cuda(c["w"]), torch.zeros(x.shape, device="cuda")
        gk = torch.zeros((B, kh, kw), device="cuda")
        ks = eng.set_taps(k.reshape(B, kh, kw))
        even = eng.set_taps(np.full((B, 4, 6), 1 / 24, np.float32))
        tall = eng.set_taps(np.full((B, 9, 7), 1 / 63, np.float32))                  # nine rows on a domain of nine: at most rows - 1
        before = eng.workspace_bytes()
        call = lambda *a: eng.edgetaper_taps_backward_ptr(*a)
        bad = [
            ("PB_ERR_BADARG", (xt.data_ptr(), gt.data_ptr(), None, None, x.shape, ks, capi.PB_WRAP, 3)),                       # both outputs null
            ("PB_ERR_BADARG", (xt.data_ptr(), None, gx.data_ptr(), None, x.shape, ks, capi.PB_WRAP, 3)),                       # no upstream
            ("PB_ERR_BADARG", (None, gt.data_ptr(), gx.data_ptr(), gk.data_ptr(), x.shape, ks, capi.PB_WRAP, 3)),              # the taps need x
            ("PB_ERR_BADARG", (xt.data_ptr(), gt.data_ptr(), gt.data_ptr(), None, x.shape, ks, capi.PB_WRAP, 3)),              # grad_x aliases grad_out
            ("PB_ERR_BADARG", (xt.data_ptr(), gt.data_ptr(), xt.data_ptr(), None, x.shape, ks, capi.PB_WRAP, 3)),              # grad_x aliases x
            ("PB_ERR_BADARG", (xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), gx.data_ptr(), x.shape, ks, capi.PB_WRAP, 3)),     # the outputs alias
            ("PB_ERR_BADARG", (xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), gk.data_ptr(), x.shape, ks, capi.PB_WRAP, -1)),    # n_tapers < 0
            ("PB_ERR_BADARG", (xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), gk.data_ptr(), x.shape, ks, 7, 3)),                # no such boundary
            ("PB_ERR_BADARG", (xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), None, x.shape, tall, capi.PB_ZERO, 3)),            # does not fit
            ("PB_ERR_UNSUPPORTED", (xt.data_ptr(), gt.data_ptr(), gx.data_ptr(), None, x.shape, even, capi.PB_WRAP, 3)),       # even sides
        ]
        for code, args in bad:
            with pytest.raises(capi.PolyblurHipError, match=code):
                call(*args)
        eng.synchronize()
        assert eng.workspace_bytes() == before and not gx.any() and not gk.any()     # every refusal came before any launch
        for s in (ks, even, tall):
            s.free()
    finally:
        eng.close()


def test_the_pure_phase_chain_with_edgetaper_is_still_refused():
    import polyblur_amd as pa
    c = eg.taper_case("t0_ends_overlap")
    with pytest.raises(NotImplementedError, match="edgetaper is not differentiated"):
        pa.inverse_filtering_nonsymmetric(cuda(c["x"], requires_grad=True), cuda(c["k"]), 2, 3, do_edgetaper=True)


def test_even_sides_and_float16_are_still_refused_on_the_gpu():
    import polyblur_amd as pa
    c = eg.taper_case("t0_ends_overlap")
    xg = cuda(c["x"], requires_grad=True)
    with pytest.raises(NotImplementedError, match="odd sides only"):
        pa.edgetaper(xg, cuda(np.full((1, 1, 4, 6), 1 / 24, np.float32)))
    with pytest.raises(NotImplementedError, match="odd sides only"):
        pa.inverse_filtering_rank3(xg, cuda(np.full((1, 1, 4, 6), 1 / 24, np.float32)), 2, 3, do_edgetaper=True, method="fft")
    with pytest.raises(NotImplementedError, match="edgetaper is not differentiated"):
        pa.inverse_filtering_rank3(cuda(c["x"]).half(), cuda(c["k"], requires_grad=True), 2, 3, do_edgetaper=True, method="fft")
