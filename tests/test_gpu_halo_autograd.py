"""Differentiable halo masking on the GPU: pb_halo_mask_backward and pb_fourier_gradients_backward alone,
polyblur_amd.fourier_gradients / halo_masking, inverse_filtering_rank3(remove_halo=True) and the blind call with remove_halo=True under
torch.autograd -- against the float64 restatement (tests/halo_grad_ref.py, which tests/test_halo_autograd_cpu.py pins to the
reference's own autograd, proves discriminating and measures the tolerances for) and against the reference's goldens
(tests/golden/halo_grad.npz).

Tolerances
  * the stage alone, per gradient, relative to a plane's largest entry: hg.TOL_STAGE (hg.TOL_STAGE_MANY for the 65 540 planes) = 4 x
    the error of the float32 NumPy evaluation against float64 over the same sets; hg.TOL_FOURIER likewise;
  * the chain (hg.chain_tolerances): the per-sample tolerance tests/test_gpu_autograd.py uses for rank-3 (4e-5 x its pad factors) x
    the largest upstream the polynomial's backward receives (the stage's grad_y under the clamp's mask, float64), plus the stage's
    and the spectral derivative's tolerances x the image's largest gradient entry; grad_img's gradients: the stage's tolerance x
    the plane's largest entry plus halo_ref.TOL_INV (what the project holds the float32 chain's y to) x the absolute row sums of
    d grad / d y, the first-order effect of the polynomial's own error on them; kernel gradients per lag: autograd_ref.TOL_K x
    sum |u| |v| plus the stage's grad_y tolerance x the same sum for a constant upstream of the largest |grad_y|;
  * the blind call (hg.blind_tolerances): the bound tests/test_gpu_blind_autograd.py holds the blind gradient to plus, per
    iteration, the stage's and the spectral derivative's tolerances x the image's largest gradient entry;
  * the forward under grad against the same call under torch.no_grad(): 2e-5 x n_iter."""
import functools
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import halo_grad_ref as hg
import halo_ref as hr
from polyblur_amd import _capi as capi

TOL_FWD = 2e-5
STAGE = {cid: (shape, zeros) for cid, shape, zeros in hg.stage_cases()}


def cuda(a, **kw):
    import torch
    return torch.tensor(np.asarray(a), device="cuda", **kw)


def golden_cases(golden, kind):
    d = golden("halo_grad.npz")
    return [(c, {k[len(c["name"]) + 1:]: d[k] for k in d.files if k.startswith(c["name"] + "_")}) for c in hg.golden_cases(d) if c["kind"] == kind]


def stage_backward(s, want=(True, True, True, True)):
    """pb_halo_mask_backward on the set s through the engine: the asked-for gradients as arrays, None for the others"""
    import torch
    from polyblur_amd.engine import get_engine
    eng = get_engine(0)
    ins = [cuda(s[k]) for k in ("x", "y", "gx", "gy", "g")]
    outs = [torch.full_like(ins[0], float("nan")) if w else None for w in want]
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.halo_mask_backward_ptr(*[t.data_ptr() for t in ins], *[o.data_ptr() if o is not None else None for o in outs], s["x"].shape)
    torch.cuda.current_stream().synchronize()
    return [o.cpu().numpy() if o is not None else None for o in outs]


# ---------------------------------------------------------------------------------------------
# pb_halo_mask_backward alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(STAGE))
def test_stage_backward_against_float64(cid):
    shape, zeros = STAGE[cid]
    s = hg.repaired_set(shape, zeros)
    tol = hg.stage_tolerance(shape)
    got = stage_backward(s)
    errs = {n: hg.plane_error(g, s["want"][n]) for n, g in zip(hg.NAMES, got)}
    print(cid, " ".join("%s %.3g (tolerance %.3g)" % (n, errs[n], tol[n]) for n in hg.NAMES))
    assert all(np.isfinite(g).all() for g in got)
    assert all(errs[n] <= tol[n] for n in hg.NAMES), (cid, errs)


def test_stage_forward_classifies_every_sample_as_float64_does():
    """z > 0 exactly where the float64 forward has it (the kink band is empty), so the backward's active set is the reference's"""
    from polyblur_amd.engine import get_engine
    for cid in ("1x3x32x48", "2x3x33x50", "zeros_1x2x16x20"):
        shape, zeros = STAGE[cid]
        s = hg.repaired_set(shape, zeros)
        out = get_engine(0).halo_mask(s["x"], s["y"], s["gx"], s["gy"])
        assert np.array_equal(out != s["y"], (s["z"] > 0) & (s["x"] != s["y"]))


def test_every_combination_of_null_outputs():
    """an output that is asked for gets the bits it gets when all four are; all four NULL is refused"""
    import torch
    from polyblur_amd.engine import get_engine
    s = hg.repaired_set((2, 3, 33, 50))
    full = stage_backward(s)
    for want in itertools.product((False, True), repeat=4):
        if not any(want):
            continue
        got = stage_backward(s, want)
        for w, g, f in zip(want, got, full):
            assert (g is None) == (not w)
            assert g is None or np.array_equal(g, f), want
    t = cuda(s["x"])
    with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):
        get_engine(0).halo_mask_backward_ptr(*[t.data_ptr()] * 5, None, None, None, None, s["x"].shape)
    out = torch.empty_like(t)
    with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):                 # an output that aliases an input
        get_engine(0).halo_mask_backward_ptr(t.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), out.data_ptr(), t.data_ptr(), None, None, None, s["x"].shape)


def test_unsupported_line_lengths_are_refused_before_any_launch():
    """a width beyond the spectral derivative's lines: PB_ERR_UNSUPPORTED from both entry points, and nothing is written"""
    import torch
    from polyblur_amd.engine import get_engine
    eng = get_engine(0)
    shape = (1, 1, 2, 65538)
    assert capi.load_library().pb_fft_length_supported(shape[-1]) == 0
    t = torch.zeros(shape, device="cuda")
    out = torch.full(shape, 7.0, device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    with pytest.raises(capi.PolyblurHipError, match="PB_ERR_UNSUPPORTED"):
        eng.halo_mask_backward_ptr(*[t.data_ptr()] * 5, out.data_ptr(), None, None, None, shape)
    with pytest.raises(capi.PolyblurHipError, match="PB_ERR_UNSUPPORTED"):
        eng.fourier_gradients_backward_ptr(t.data_ptr(), None, shape, out.data_ptr())
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------
# pb_fourier_gradients_backward alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hg.FOURIER_SHAPES, ids=hr.shape_id)
def test_fourier_gradients_backward_against_float64(shape):
    import torch
    from polyblur_amd.engine import get_engine
    eng = get_engine(0)
    ggx, ggy = hg.fourier_case(shape)
    tx, ty = cuda(ggx), cuda(ggy)
    for use_x, use_y in ((True, True), (True, False), (False, True)):
        out = torch.full_like(tx, float("nan"))
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.fourier_gradients_backward_ptr(tx.data_ptr() if use_x else None, ty.data_ptr() if use_y else None, shape, out.data_ptr())
        want = hg.fourier_backward(ggx if use_x else None, ggy if use_y else None)
        err = hg.plane_error(out.cpu().numpy(), want)
        print(shape, use_x, use_y, "%.3g (tolerance %.3g)" % (err, hg.TOL_FOURIER))
        assert err <= hg.TOL_FOURIER
    with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):
        eng.fourier_gradients_backward_ptr(None, None, shape, tx.data_ptr())


def test_fourier_gradients_function_and_kinds():
    import torch
    import polyblur_amd as pa
    shape = (1, 3, 33, 50)
    x, w = hg.fourier_case(shape)
    xt = cuda(x, requires_grad=True)
    gx, gy = pa.fourier_gradients(xt)
    assert gx.grad_fn is not None and gy.grad_fn is not None
    (gx * cuda(w)).sum().backward()                               # one output only: the other's transform is skipped
    assert hg.plane_error(xt.grad.cpu().numpy(), hg.fourier_backward(w, None)) <= hg.TOL_FOURIER
    xt.grad = None
    gx, gy = pa.fourier_gradients(xt)
    ((gx * cuda(w)).sum() + (gy * cuda(x)).sum()).backward()
    assert hg.plane_error(xt.grad.cpu().numpy(), hg.fourier_backward(w, x)) <= hg.TOL_FOURIER
    plain = pa.fourier_gradients(cuda(x))
    arr, cpu = pa.fourier_gradients(x), pa.fourier_gradients(torch.from_numpy(x))
    assert not plain[0].requires_grad and torch.equal(plain[0], gx.detach()) and torch.equal(plain[1], gy.detach())
    for k in (0, 1):
        assert isinstance(arr[k], np.ndarray) and np.array_equal(arr[k], plain[k].cpu().numpy())
        assert isinstance(cpu[k], torch.Tensor) and not cpu[k].is_cuda and np.array_equal(cpu[k].numpy(), arr[k])
        assert hg.plane_error(arr[k], (hg.dx, hg.dy)[k](x)) <= hg.TOL_FOURIER


# ---------------------------------------------------------------------------------------------
# halo_masking
# ---------------------------------------------------------------------------------------------
def test_halo_masking_function_against_the_goldens_and_float64(golden):
    import torch
    import polyblur_amd as pa
    for c, d in golden_cases(golden, "stage"):
        s = hg.repaired_set(tuple(c["shape"]), c["zeros"])
        assert all(np.array_equal(d[k], s[k]) for k in hg.NAMES + ("g",))           # the builder's, still
        ts = [cuda(s[k], requires_grad=True) for k in hg.NAMES]
        out = pa.halo_masking(ts[0], ts[1], (ts[2], ts[3]))
        assert out.grad_fn is not None
        out.backward(cuda(s["g"]))
        for n, t in zip(hg.NAMES, ts):
            e64, eref = hg.plane_error(t.grad.cpu().numpy(), s["want"][n]), hg.plane_error(t.grad.cpu().numpy(), d["d" + n])
            print(c["name"], n, "%.3g against float64, %.3g against the reference (tolerance %.3g, + %.3g)" % (e64, eref, hg.TOL_STAGE[n], hg.BOUND_GOLDEN_F64))
            assert e64 <= hg.TOL_STAGE[n] and eref <= hg.TOL_STAGE[n] + hg.BOUND_GOLDEN_F64
        # forward: the engine's pb_halo_mask, whatever the kind of the operands; nothing recorded without grad
        plain = pa.halo_masking(*[t.detach() for t in ts[:2]], (ts[2].detach(), ts[3].detach()))
        with torch.no_grad():
            quiet = pa.halo_masking(ts[0], ts[1], (ts[2], ts[3]))
        arr = pa.halo_masking(s["x"], s["y"], (s["gx"], s["gy"]))
        assert not plain.requires_grad and not quiet.requires_grad
        assert torch.equal(plain, out.detach()) and torch.equal(plain, quiet) and np.array_equal(arr, plain.cpu().numpy())
        # only what is asked for is computed: the image's gradient alone
        xt = cuda(s["x"], requires_grad=True)
        pa.halo_masking(xt, cuda(s["y"]), (cuda(s["gx"]), cuda(s["gy"]))).backward(cuda(s["g"]))
        assert torch.equal(xt.grad, ts[0].grad)


# ---------------------------------------------------------------------------------------------
# inverse_filtering_rank3(remove_halo=True)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_reference(name):
    """float64 gradients of a golden chain case and what its tolerances are made of: computed once, shared, never written to"""
    d = np.load(hg_golden_path())
    c = [c for c in hg.golden_cases(d) if c["name"] == name][0]
    x, k, w = d[name + "_x"], d[name + "_k"], d[name + "_w"]
    grad_img = None if c["own"] else (d[name + "_gx"], d[name + "_gy"])
    return c, x, k, w, grad_img, hg.chain_tolerances(x, k, grad_img, w, c["alpha"], c["beta"], c["method"])


def hg_golden_path():
    import os
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "halo_grad.npz")


@pytest.mark.parametrize("name", ["c00", "c01", "c02", "c03"])
def test_chain_gradients_against_the_goldens_and_float64(golden, name):
    import torch
    import polyblur_amd as pa
    d = golden("halo_grad.npz")
    c, x, k, w, grad_img, ref = chain_reference(name)
    want, tol = ref["want"], ref["tol"]
    xt, kt = cuda(x, requires_grad=True), cuda(k, requires_grad=True)
    gs = None if grad_img is None else tuple(cuda(g, requires_grad=True) for g in grad_img)
    call = lambda a, b, g: pa.inverse_filtering_rank3(a, b, c["alpha"], c["beta"], remove_halo=True, grad_img=g, method=c["method"])
    y = call(xt, kt, gs)
    assert y.requires_grad and y.grad_fn is not None
    (y * cuda(w)).sum().backward()
    got = {"x": xt.grad, "k": kt.grad}
    if gs is not None:
        got.update(gx=gs[0].grad, gy=gs[1].grad)
    for n, g in got.items():
        g = g.cpu().numpy()
        e64 = float(np.max(np.abs(g - want[n]) / tol[n]))
        eref = float(np.max(np.abs(g - d[name + "_d" + n]) / (tol[n] + hg.BOUND_GOLDEN_F64 * np.abs(want[n]).max())))
        print("%s %-6s %s: %.3g of its tolerance against float64 (%.3g abs, max |grad| %.3g), %.3g against the reference"
              % (name, c["method"], n, e64, np.abs(g - want[n]).max(), np.abs(want[n]).max(), eref))
        assert e64 <= 1.0 and eref <= 1.0, (name, n, e64, eref)
    # the forward under grad against the fused path; without grad nothing is recorded and the bits are the fused path's
    det = None if gs is None else tuple(g.detach() for g in gs)
    with torch.no_grad():
        quiet = call(xt, kt, gs)
    plain = call(cuda(x), cuda(k), det)
    assert not quiet.requires_grad and not plain.requires_grad and torch.equal(quiet, plain)
    efwd = float((y.detach() - quiet).abs().max())
    print("%s forward under grad vs no_grad %.3g (tolerance %.3g)" % (name, efwd, TOL_FWD))
    assert efwd <= TOL_FWD


def test_chain_gradient_of_grad_img_alone():
    """grad_img's planes require grad, the image and the kernel do not: the call is still differentiable"""
    import polyblur_amd as pa
    c, x, k, w, grad_img, ref = chain_reference("c00")
    gs = tuple(cuda(g, requires_grad=True) for g in grad_img)
    y = pa.inverse_filtering_rank3(cuda(x), cuda(k), c["alpha"], c["beta"], remove_halo=True, grad_img=gs, method=c["method"])
    (y * cuda(w)).sum().backward()
    for n, g in zip(("gx", "gy"), gs):
        assert float(np.max(np.abs(g.grad.cpu().numpy() - ref["want"][n]) / ref["tol"][n])) <= 1.0


def test_chain_backward_repeated_eight_times_gives_identical_bits():
    import polyblur_amd as pa
    c, x, k, w, grad_img, _ = chain_reference("c00")
    runs = []
    for _ in range(8):
        ts = [cuda(a, requires_grad=True) for a in (x, k) + tuple(grad_img)]
        y = pa.inverse_filtering_rank3(ts[0], ts[1], c["alpha"], c["beta"], remove_halo=True, grad_img=(ts[2], ts[3]), method=c["method"])
        (y * cuda(w)).sum().backward()
        runs.append([t.grad.cpu().numpy() for t in ts])
    assert all(np.array_equal(a, b) for r in runs[1:] for a, b in zip(runs[0], r))


# ---------------------------------------------------------------------------------------------
# the blind call with remove_halo=True
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def blind_reference(name):
    d = np.load(hg_golden_path())
    c = [c for c in hg.golden_cases(d) if c["name"] == name][0]
    x, w = d[name + "_x"], d[name + "_w"]
    return c, x, w, d[name + "_dx"], hg.blind_tolerances(x, w, c["n_iter"], hr.PIPE_KW)


@pytest.mark.parametrize("module", [False, True])
@pytest.mark.parametrize("name", ["b00", "b01"])
def test_blind_gradients_against_the_goldens_and_float64(name, module):
    import torch
    import polyblur_amd as pa
    c, x, w, gref, ref = blind_reference(name)
    kw = dict(hr.PIPE_KW, n_iter=c["n_iter"])
    xt = cuda(x, requires_grad=True)
    if module:
        y = pa.PolyblurDeblurring()(xt, sigma_r=0.8, **kw)
    else:
        y = pa.polyblur_deblurring(xt, **kw)
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
    eref = float(np.max(np.abs(g - gref) / (tol + hg.BOUND_GOLDEN_BLIND * np.abs(gref).max(axis=(1, 2, 3), keepdims=True))))
    print("%s n_iter %d: forward under grad vs no_grad %.3g (tolerance %.3g) | gradient %.3g of its tolerance against float64 (%.3g abs, "
          "max |grad| %.3g), %.3g against the reference's float32" % (name, c["n_iter"], efwd, TOL_FWD * c["n_iter"], e64,
                                                                      np.abs(g - want).max(), np.abs(want).max(), eref))
    assert efwd <= TOL_FWD * c["n_iter"], (name, efwd)
    assert e64 <= 1.0 and eref <= 1.0, (name, e64, eref)


def test_workspace_grows_by_the_documented_scratch():
    """two plane sets, nM and S of P floats each and bpp partial sums per plane (each buffer rounded up to 256 bytes); without the
    grad0 outputs no S and no partials; without grad_y no second plane set"""
    import torch
    from polyblur_amd.engine import Engine
    shape = (1, 1, 96, 128)
    s = hg.repaired_set(shape)
    P, HW = shape[0] * shape[1], shape[2] * shape[3]
    bpp = min(256, max(1, (HW + 4095) // 4096))
    assert bpp > 1
    r256 = lambda n: (n + 255) // 256 * 256
    ins = [cuda(s[k]) for k in ("x", "y", "gx", "gy", "g")]
    outs = [torch.empty_like(ins[0]) for _ in range(4)]
    for want, extra in (((True, False, False, False), 0), ((True, True, False, False), r256(4 * P * HW)),
                        ((True, True, True, True), r256(4 * P * HW) + r256(4 * P * bpp) + r256(4 * P))):
        eng = Engine(0)
        try:
            eng.set_stream(torch.cuda.current_stream().cuda_stream)
            eng.halo_mask_ptr(*[t.data_ptr() for t in ins[:4]], outs[0].data_ptr(), shape)      # the forward's own scratch first
            before = eng.workspace_bytes()
            for _ in range(2):
                eng.halo_mask_backward_ptr(*[t.data_ptr() for t in ins], *[o.data_ptr() if w else None for o, w in zip(outs, want)], shape)
            eng.synchronize()
            assert eng.workspace_bytes() - before == r256(4 * P * HW) + r256(4 * P) + extra, want
        finally:
            eng.close()
