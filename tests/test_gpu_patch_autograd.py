"""The differentiable patch decomposition on the GPU: pb_extract_patches_backward and pb_overlap_add_backward alone
against the float64 restatement (tests/patch_grad_ref.py, which tests/test_patch_autograd_cpu.py pins to the oracle and gradchecks),
polyblur_amd.image_to_patches / patches_to_image with and without grad, and PolyblurDeblurring(patch_decomposition=True) under grad
against the same computation composed of torch ops around the package's own differentiable polyblur_deblurring.

Tolerances, each relative to the largest entry of the reference
  * the extraction's backward: none -- the upstream gradients are k / 64, every partial sum is exact in float32, the result must
    be the float64 gradient bit for bit;
  * the overlap-add's backward: pg.TOL_OLA per case = 6 x the float32 error of the restatement itself on the case;
  * the module's image gradient against the composed computation, per entry: pg.TOL_OLA of the lattice x the largest entry +
    summation_slack, what the order of that entry's float32 sum can change (computed per entry, justified there);
  * the module's parameter gradients: pr.TOL_FACTOR x pg.E_PARAMS, the composed computation's own float32 error against the float64
    truth of the same composition;
  * the module's output: TOL_FWD of tests/test_gpu_autograd.py."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import params_grad_ref as pr
import patch_grad_ref as pg
from offset_operands import bits, carve, guards_intact, poisoned
from polyblur_amd import _capi as capi
from polyblur_amd.synthetic import synthetic_blurry_batch
from test_gpu_autograd import TOL_FWD

NAMES = sorted(pg.CASES)
BLIND = dict(n_iter=2, alpha=6, beta=1, ker_size=13)         # (the setting of pg.PARAM_TRUTH)


def cuda(a, **kw):
    import torch
    return torch.tensor(np.asarray(a), device="cuda", **kw)


def engine():
    import torch
    from polyblur_amd.engine import get_engine
    eng = get_engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    return eng


@functools.lru_cache(maxsize=None)
def extraction_reference(name):
    up = pg.dyadic_upstream(name)
    want = pg.extraction_gradient(name, up)
    up.setflags(write=False), want.setflags(write=False)
    return up, want


@functools.lru_cache(maxsize=None)
def ola_reference(name):
    p, w = pg.ola_inputs(name)
    grad, v = pg.ola_gradient(name, p, w)
    for a in (p, w, grad, v):
        a.setflags(write=False)
    return p, w, grad, v


def windows(g):
    import torch
    return pg.window(g["ph"], torch.float32).numpy(), pg.window(g["pw"], torch.float32).numpy()


def extract_backward(name, up, offset=0):
    """pb_extract_patches_backward into a plane full of NaN, every pointer `offset` elements off -> (gradient, guards intact)"""
    import torch
    shape, g = pg.case(name)
    held = [carve(np.array(up), offset), carve(poisoned(shape, torch.float32), offset)]       # (a copy: the owner's array is read-only)
    torch.cuda.synchronize()
    eng = engine()
    eng.extract_patches_backward_ptr(held[0][1].data_ptr(), held[1][1].data_ptr(), shape, g)
    torch.cuda.synchronize()
    return held[1][1].cpu().numpy(), all(guards_intact(b, v) for b, v in held) and np.array_equal(held[0][1].cpu().numpy(), up)


def overlap_add_backward(name, p, w, offset=0):
    import torch
    shape, g = pg.case(name)
    wy, wx = windows(g)
    held = [carve(a, offset) for a in (np.array(p), np.array(w), poisoned(p.shape, torch.float32), wy, wx)]
    torch.cuda.synchronize()
    eng = engine()
    eng.overlap_add_backward_ptr(held[0][1].data_ptr(), held[1][1].data_ptr(), held[2][1].data_ptr(), shape, g, held[3][1].data_ptr(),
                                 held[4][1].data_ptr())
    torch.cuda.synchronize()
    return held[2][1].cpu().numpy(), all(guards_intact(b, v) for b, v in held) and np.array_equal(held[0][1].cpu().numpy(), p)


# ---------------------------------------------------------------------------------------------
# pb_extract_patches_backward alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_extraction_backward_is_exact(name):
    up, want = extraction_reference(name)
    assert np.abs(want).max() * 64 < 2 ** 24 and np.array_equal(want * 64, np.rint(want * 64))       # (the condition of exactness)
    got, intact = extract_backward(name, up)
    print("%s: largest |grad| * 64 = %g, entries off: %d" % (name, np.abs(want).max() * 64, int((got.astype(np.float64) != want).sum())))
    assert intact and not np.isnan(got).any()                            # (every entry written: the plane was full of NaN)
    assert np.array_equal(got.astype(np.float64), want)


# ---------------------------------------------------------------------------------------------
# pb_overlap_add_backward alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", NAMES)
def test_overlap_add_backward_against_float64(name):
    shape, g = pg.case(name)
    p, w, want, v = ola_reference(name)
    margin, share = min(float(np.abs(v).min()), float(np.abs(v - 1).min())), float(((v < 0) | (v > 1)).mean())
    assert margin >= 1e-3 and 0.05 <= share <= 0.95                      # (the conditions of the comparison)
    got, intact = overlap_add_backward(name, p, w)
    err = pg.rel_error(got, want)
    print("%s: %.3g of max |grad| = %.3g (bound %.3g); margin %.4f, clamped %.3f" % (name, err, np.abs(want).max(), pg.TOL_OLA[name], margin, share))
    assert intact and np.isfinite(got).all()                             # (written everywhere, zeros included)
    assert err <= pg.TOL_OLA[name]
    inside = pg.in_image(g, shape[0], shape[1]).numpy()
    assert not got[~inside].any()                                        # (the cropped pad: exactly 0)
    assert np.array_equal(got == 0, want == 0)                           # (the same samples clamped, the same elements in the pad)


@pytest.mark.parametrize("name", ["a", "e", "g"])
def test_clamp_convention(name):
    """v == 0 exactly passes the gradient (torch.clamp's convention: the mask is inclusive), v == 2 passes nothing"""
    shape, g = pg.case(name)
    p, w, _, _ = ola_reference(name)
    zeros = np.zeros_like(p)
    want, v = pg.ola_gradient(name, zeros, np.array(w), clamp=False)                 # the unmasked formula
    assert not v.any()
    got, _ = overlap_add_backward(name, zeros, w)
    err = pg.rel_error(got, want)
    print("%s, all-zero patches: %.3g from the unmasked formula (bound %.3g)" % (name, err, pg.TOL_OLA[name]))
    assert np.abs(want).max() > 0.1 and err <= pg.TOL_OLA[name]
    got, _ = overlap_add_backward(name, np.full_like(p, 2.0), w)
    assert not got.any() and not np.isnan(got).any()


# ---------------------------------------------------------------------------------------------
# determinism, offsets, arguments
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["a", "c", "g"])
def test_the_same_call_twice_gives_equal_bits(name):
    up = np.random.default_rng(7).standard_normal(extraction_reference(name)[0].shape).astype(np.float32)     # (sums that do round)
    assert np.array_equal(extract_backward(name, up)[0], extract_backward(name, up)[0])
    p, w, _, _ = ola_reference(name)
    assert np.array_equal(overlap_add_backward(name, p, w)[0], overlap_add_backward(name, p, w)[0])


@pytest.mark.parametrize("offset", [1, 3])
@pytest.mark.parametrize("name", ["a", "g"])
def test_every_pointer_at_an_element_offset(name, offset):
    up = np.random.default_rng(8).standard_normal(extraction_reference(name)[0].shape).astype(np.float32)
    twin, ok0 = extract_backward(name, up)
    got, ok = extract_backward(name, up, offset)
    assert ok0 and ok and np.array_equal(twin.view(np.int32), got.view(np.int32))
    p, w, _, _ = ola_reference(name)
    twin, ok0 = overlap_add_backward(name, p, w)
    got, ok = overlap_add_backward(name, p, w, offset)
    assert ok0 and ok and np.array_equal(twin.view(np.int32), got.view(np.int32))


def test_bad_arguments_are_refused_before_any_launch():
    import torch
    shape, g = pg.case("e")
    n = g["n_i"] * g["n_j"] * shape[0]
    gp = torch.rand((n, shape[1], g["ph"], g["pw"]), device="cuda")
    gi, go = torch.full(shape, 7.0, device="cuda"), torch.rand(shape, device="cuda")
    out = torch.full_like(gp, 7.0)
    wy, wx = (cuda(a) for a in windows(g))
    eng = engine()
    bad = [dict(g, ph=1), dict(g, pw=1), dict(g, step_h=0), dict(g, step_w=-1), dict(g, n_i=0), dict(g, n_j=0)]
    for args in [(gp.data_ptr(), gi.data_ptr(), shape, b) for b in bad] + [(None, gi.data_ptr(), shape, g), (gp.data_ptr(), None, shape, g),
                                                                            (gp.data_ptr(), gp.data_ptr(), shape, g), (gp.data_ptr(), gi.data_ptr(), (1, 1, 0, 46), g)]:
        with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):
            eng.extract_patches_backward_ptr(*args)
    good = (gp.data_ptr(), go.data_ptr(), out.data_ptr(), shape, g, wy.data_ptr(), wx.data_ptr())
    for args in [good[:4] + (b,) + good[5:] for b in bad] + [good[:i] + (None,) + good[i + 1:] for i in (0, 1, 2)] + \
                [(gp.data_ptr(), go.data_ptr(), gp.data_ptr()) + good[3:], (gp.data_ptr(), out.data_ptr(), out.data_ptr()) + good[3:]]:
        with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):
            eng.overlap_add_backward_ptr(*args)
    for wys in ((0, wx.data_ptr()), (wy.data_ptr(), 0)):
        with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):
            eng.overlap_add_backward_ptr(*(good[:5] + wys))
    torch.cuda.synchronize()
    assert bool((gi == 7.0).all()) and bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------
# image_to_patches and patches_to_image
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("half", [False, True], ids=["fp32", "fp16"])
@pytest.mark.parametrize("name", ["a", "b", "g"])
def test_public_functions_give_the_engines_bits(name, half):
    import torch
    import polyblur_amd as pa
    full, ps, ov = pg.CASES[name]
    shape, g = pg.case(name)
    dt, pbdt = (torch.float16, capi.PB_F16) if half else (torch.float32, capi.PB_F32)
    x = torch.rand(full, device="cuda", generator=torch.Generator("cuda").manual_seed(11)).to(dt)
    xe = x[..., :shape[2], :shape[3]].contiguous()
    n_p = g["n_i"] * g["n_j"]
    want_p = torch.empty((n_p * shape[0], shape[1], g["ph"], g["pw"]), dtype=dt, device="cuda")
    engine().extract_patches_ptr(xe.data_ptr(), want_p.data_ptr(), pbdt, shape, g, 0, n_p)
    got_p = pa.image_to_patches(x, ps, ov)
    assert got_p.dtype == dt and torch.equal(bits(got_p), bits(want_p))
    restored = (1.6 * got_p - 0.3).contiguous()                           # (beyond [0, 1] in places: the clamp takes part)
    wy, wx = (cuda(a) for a in windows(g))
    want = torch.empty(shape, dtype=dt, device="cuda")
    engine().overlap_add_ptr(restored.data_ptr(), want.data_ptr(), pbdt, shape, g, wy.data_ptr(), wx.data_ptr())
    got = pa.patches_to_image(restored, full[-2:], ps, ov)
    assert got.dtype == dt and tuple(got.shape) == shape and torch.equal(bits(got), bits(want))
    if not half:                                                          # under grad: the same forwards, and the engine's backwards
        xg = x.clone().requires_grad_(True)
        pgr = pa.image_to_patches(xg, ps, ov)
        assert pgr.grad_fn is not None and torch.equal(bits(pgr.detach()), bits(want_p))
        rg = restored.clone().requires_grad_(True)
        og = pa.patches_to_image(rg, full[-2:], ps, ov)
        assert og.grad_fn is not None and torch.equal(bits(og.detach()), bits(want))
        w = torch.rand(shape, device="cuda", generator=torch.Generator("cuda").manual_seed(12)) - 0.5
        og.backward(w)
        want_g = torch.empty_like(restored)
        engine().overlap_add_backward_ptr(restored.data_ptr(), w.data_ptr(), want_g.data_ptr(), shape, g, wy.data_ptr(), wx.data_ptr())
        assert torch.equal(bits(rg.grad), bits(want_g))
        up = torch.rand(pgr.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(13))
        pgr.backward(up)
        want_x = torch.empty(shape, device="cuda")
        engine().extract_patches_backward_ptr(up.data_ptr(), want_x.data_ptr(), shape, g)
        assert tuple(xg.grad.shape) == full
        assert torch.equal(bits(xg.grad[..., :shape[2], :shape[3]].contiguous()), bits(want_x))
        if full != shape:                                                 # (the dropped row and column of an odd side: no gradient)
            assert not xg.grad[..., shape[2]:, :].any() and not xg.grad[..., :, shape[3]:].any()


# ---------------------------------------------------------------------------------------------
# the module under grad
# ---------------------------------------------------------------------------------------------
def composed(x, name, kw, shape_g=None):
    """the module's computation from torch ops around the package's differentiable blind call: F.pad replicate, slices, Kaiser
    overlap-add (patch_grad_ref's own, in float32 on the device), one blind call per patch"""
    import torch
    import polyblur_amd as pa
    shape, g = shape_g or pg.case(name)
    patches = pg.extract(x, g)
    if patches.requires_grad:
        patches.retain_grad()                                             # (summation_slack reads it)
    B = shape[0]
    restored = torch.cat([pa.polyblur_deblurring(patches[n * B:(n + 1) * B].contiguous(), q=0.0, **kw) for n in range(g["n_i"] * g["n_j"])])
    return pg.overlap_add(restored, shape, g)[0], patches


def module_call(x, name, kw, batch_size, case=None):
    import polyblur_amd as pa
    _, ps, ov = case or pg.CASES[name]
    return pa.PolyblurDeblurring(patch_decomposition=True, patch_size=ps, patch_overlap=ov, batch_size=batch_size)(x, q=0.0, **kw)


def summation_slack(shape, g, patch_grad):
    """Per entry of the image gradient, what the order of a float32 sum can change.  The module and the composed computation add the
    same terms of the extraction's adjoint -- the patches' gradients at the padded positions that clamp to the entry -- in different
    orders (the module: the cover, the run of padded rows, the run of padded columns, each in index order; torch: the backward of
    F.pad, in no fixed order).  A float32 sum of N terms is within (N - 1) 2^-24 of the exact one, relative to the sum of the terms'
    magnitudes A, whatever the order (Higham, Accuracy and Stability of Numerical Algorithms, 4.2, to first order).  N and A are
    computed here, per entry, in float64: the adjoint of ones and of |patch_grad|.  Twice that, once for each computation: nothing for
    an entry with one term, three ulps of A under a cover of four patches, and only the pad's corners reach a hundred."""
    import torch
    def adjoint(up):
        x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        pg.extract(x, g).backward(up)
        return x.grad.numpy()
    G = patch_grad.detach().cpu().to(torch.float64).abs()
    N, A = adjoint(torch.ones_like(G)), adjoint(G)
    return 2 * (N - 1) * 2.0 ** -24 * A, int(N.max())


def check_image_gradient(what, gm, gc, tol_ola, slack):
    """|module - composed| per entry within tol_ola x the largest entry + the summation slack of that entry"""
    gm, gc = gm.detach().cpu().numpy().astype(np.float64), gc.detach().cpu().numpy().astype(np.float64)
    diff, big = np.abs(gm - gc), np.abs(gc).max()
    bound = tol_ola * big + slack
    worst = int(np.argmax(diff - bound))
    print("%s: image gradient %.3g of max |grad| = %.3g (overlap-add bound %.3g; summation slack of an entry up to %.3g of it, median %.3g); "
          "nearest to its bound: |diff| %.3g under %.3g" % (what, diff.max() / big, big, tol_ola, slack.max() / big, np.median(slack) / big,
                                                           diff.flat[worst], bound.flat[worst]))
    assert np.isfinite(gm).all() and (diff <= bound).all()


@functools.lru_cache(maxsize=None)
def image_a():
    shape, _ = pg.case("a")
    x, _ = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=23)
    w = np.random.default_rng(31).uniform(0.5, 1.5, size=shape).astype(np.float32)
    x.setflags(write=False), w.setflags(write=False)
    return x, w


def test_module_image_gradient_against_the_composed_computation():
    import torch
    import polyblur_amd as pa
    shape, g = pg.case("a")
    x, w = image_a()
    kw = dict(BLIND, c=pr.BLIND_C, b=pr.BLIND_B)
    wt = cuda(w)
    xc = cuda(x, requires_grad=True)
    yc, patches = composed(xc, "a", kw)
    assert torch.equal(bits(patches.detach()), bits(pa.image_to_patches(cuda(x), 64, 0.25)))      # the same patches, bit for bit
    (yc * wt).sum().backward()
    outs = {}
    for bs in (1, 4, 4):
        xm = cuda(x, requires_grad=True)
        ym = module_call(xm, "a", kw, bs)
        assert ym.grad_fn is not None and tuple(ym.shape) == shape
        (ym * wt).sum().backward()
        assert torch.isfinite(xm.grad).all()
        outs.setdefault(bs, []).append((ym.detach(), xm.grad))
    with torch.no_grad():
        plain = module_call(cuda(x), "a", kw, 4)
    ym, gm = outs[1][0]
    e_fwd, e_plain = float((ym - yc.detach()).abs().max()), float((ym - plain).abs().max())
    slack, longest = summation_slack(shape, g, patches.grad)
    print("output: %.3g from the composed computation, %.3g from the call without grad (TOL_FWD %.3g); longest sum of the extraction's adjoint: %d terms"
          % (e_fwd, e_plain, TOL_FWD, longest))
    # the grouping changes no bit, and neither does a second identical call
    for y2, g2 in (outs[4][0], outs[4][1]):
        assert torch.equal(bits(ym), bits(y2)) and torch.equal(bits(gm), bits(g2))
    assert e_fwd <= TOL_FWD and e_plain <= TOL_FWD * BLIND["n_iter"]
    check_image_gradient("case a", gm, xc.grad, pg.TOL_OLA["a"], slack)


@pytest.mark.parametrize("which", ["c,b", "alpha,beta"])
def test_module_parameter_gradients_against_the_composed_computation(which):
    """the image is data: every parameter gets a gradient, the image none.  Bound, relative to the larger gradient of the pair:
    pr.TOL_FACTOR x the composed computation's own float32 error E against the float64 truth of the same composition
    (pg.composition_param_truth, recorded in pg.PARAM_TRUTH: a minute on a CPU).  E is recorded in pg.E_PARAMS as measured here and
    measured again: the record must lie within a factor of two of it."""
    import torch
    x, w = image_a()
    values = dict(c=pr.BLIND_C, b=pr.BLIND_B, alpha=float(BLIND["alpha"]), beta=float(BLIND["beta"]))
    assert pg.PARAM_SETTING == dict(BLIND, c=pr.BLIND_C, b=pr.BLIND_B, method="fft", case="a")
    names = which.split(",")
    grads = {}
    for how in ("composed", 1, 4, 4):
        ps = {n: torch.tensor(values[n], requires_grad=True) for n in names}          # CPU parameters
        kw = dict(BLIND, **dict(values, **ps))
        xt = cuda(x)
        y = composed(xt, "a", kw)[0] if how == "composed" else module_call(xt, "a", kw, how)
        assert y.grad_fn is not None
        (y * cuda(w)).sum().backward()
        assert xt.grad is None and all(p.grad is not None and p.grad.shape == p.shape and p.grad.dtype == p.dtype and p.grad.device.type == "cpu"
                                       for p in ps.values())
        grads.setdefault(how, []).append(np.array([float(p.grad) for p in ps.values()]))
    truth, composed_g = np.array(pg.PARAM_TRUTH[which]), grads["composed"][0]
    e = pr.rel_error(composed_g, truth)
    bound = pr.TOL_FACTOR * pg.E_PARAMS[which]
    print("d %s: float64 truth %s, composed on the GPU %s: E = %.3g (recorded %.3g, bound %.3g)" % (which, truth, composed_g, e, pg.E_PARAMS[which], bound))
    assert pg.E_PARAMS[which] / 2 <= e <= pg.E_PARAMS[which] * 2
    for bs in (1, 4):
        got = grads[bs][0]
        err = pr.rel_error(got, composed_g)
        print("d %s, batch_size %d: %s, %.3g from the composed computation, %.3g from the float64 truth" % (which, bs, got, err, pr.rel_error(got, truth)))
        assert np.isfinite(got).all() and (got != 0).all()
        assert err <= bound
    # the grouping does not reach a parameter's gradient, and neither does a second identical call
    assert np.array_equal(grads[1][0], grads[4][0]) and np.array_equal(grads[4][0], grads[4][1])


SMALL = ((1, 3, 48, 80), 48, 0.25)                              # one row of two overlapping 48 x 48 patches, pads 0 and 2


@pytest.mark.parametrize("option", ["remove_halo", "edgetaping"])
def test_options_through_patches(option):
    import torch
    full, ps, ov = SMALL
    g = pg.lattice(full, ps, ov)
    assert (g["n_i"], g["n_j"]) == (1, 2) and g["step_w"] < g["pw"]
    x, _ = synthetic_blurry_batch(full[0], full[1], full[2], full[3], seed0=29)
    w = cuda(np.random.default_rng(33).uniform(0.5, 1.5, size=full).astype(np.float32))
    kw = dict(n_iter=1, alpha=6, beta=1, ker_size=13, c=pr.BLIND_C, b=pr.BLIND_B, **{option: True})
    xc, xm = cuda(x, requires_grad=True), cuda(x, requires_grad=True)
    yc, patches = composed(xc, None, kw, shape_g=(full, g))
    ym = module_call(xm, None, kw, 1, case=SMALL)
    (yc * w).sum().backward()
    (ym * w).sum().backward()
    e_fwd = float((ym - yc).detach().abs().max())
    print("%s: output %.3g from the composed computation (TOL_FWD %.3g)" % (option, e_fwd, TOL_FWD))
    assert float(xm.grad.abs().max()) > 0 and e_fwd <= TOL_FWD
    check_image_gradient(option, xm.grad, xc.grad, max(pg.TOL_OLA.values()), summation_slack(full, g, patches.grad)[0])


def test_refusals_on_rocm_tensors():
    """what the blind call refuses under grad stays refused through patches, before a patch is cut; the lattice's errors come first"""
    import torch
    import polyblur_amd as pa
    x = torch.rand(1, 3, 40, 46, device="cuda", requires_grad=True)
    m = pa.PolyblurDeblurring(patch_decomposition=True, patch_size=24, patch_overlap=0.5)
    for what, kw in (("q=0.1", dict(q=0.1)), ("direct_separable", dict(method="direct_separable")), ("ker_size=12", dict(ker_size=12)),
                     ("prefilters are not differentiated", dict(prefiltering=True, prefilter="domain_transform"))):
        with pytest.raises(NotImplementedError, match="has no backward pass") as e:
            m(x, **kw)
        assert what in str(e.value) and "polyblur_deblurring" in str(e.value)
    with pytest.raises(NotImplementedError, match="has no backward pass.*overlap-add"):
        m(x.detach().half().requires_grad_(True))
    with pytest.raises(ValueError, match="holds no patch"):
        pa.PolyblurDeblurring(patch_decomposition=True, patch_size=400, patch_overlap=0.4)(torch.rand(1, 3, 100, 299, device="cuda", requires_grad=True))
    with pytest.raises(TypeError, match="return_info"):
        m(x, return_info=True)
