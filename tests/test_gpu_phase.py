"""The pure-phase filter on the GPU: polyblur_amd.inverse_filtering_nonsymmetric / compute_polynomial and the Engine's
pb_inverse_filter_phase_taps / pb_compute_polynomial_taps against the reference's own outputs
(tests/golden/nonblind_phase.npz) and against the local restatement (tests/phase_ref.py), which tests/test_phase_cpu.py pins
to those goldens and whose inputs it checks for conditioning (complex64 against complex128 <= 2e-6, clamped share <= 1 %).

Tolerances are the project's own for caller-supplied taps: inverse filter and polynomial < 2e-5, fp16 images < 1e-3.
Worst error of each group on an MI355X: not measured.

The shapes are the smallest at which each branch of conv_phase.hip can go wrong (tests/phase_ref.py: CASES): single-stage
plans, multi-stage direct plans, prime sides (Bluestein both ways), Bluestein rows with direct columns and the reverse, a lone
plane / a pair and a lone plane / two pairs, three images with three kernels, one kernel per plane, the extreme kernel shapes,
one mid-size domain (530 x 730) that crosses the column tile's width choice, and two narrow domains with a side of 2190
samples: Bluestein cores of 8192 points, the 1024-thread workgroups and the LDS footprints a 4K image runs with."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import phase_ref as pr
from oracle import polyblur_ref as ref
from polyblur_amd import _capi as capi

TOL_INV, TOL_HALF = 2e-5, 1e-3


@pytest.fixture(scope="module")
def eng():
    from polyblur_amd.engine import get_engine
    return get_engine(0)


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def check(got, want, tol, what, clamped_chain=True):
    """the comparison, behind the clamp condition: at most 1 % of the expected samples at exactly 0 or 1"""
    err = maxabs(got, want)
    clamped = float(np.mean((want == 0) | (want == 1))) if clamped_chain else 0.0
    print(what, "err %.3g" % err, "clamped %.2f %%" % (100 * clamped))
    assert np.all(np.isfinite(got)), what
    assert clamped <= 0.01, (what, clamped)
    assert err < tol, (what, err)


def golden_call(d, name):
    p = name.split("_")
    ab = {"a2b3": (2, 3), "a6b1": (6, 1)}[p[-1]]
    if p[1] == "correlate":
        return d["k_" + p[2]], ab, dict(correlate=True)
    if p[1] == "perchannel":
        return d["k_perchannel_" + p[2]], ab, dict(remove_halo=True)
    full = p[2] == "full"
    return d["k_" + p[1]], ab, dict(remove_halo=full, do_edgetaper=full)


# ---------------------------------------------------------------------------------------------
# the reference's own outputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["numpy", "rocm_tensor"])
def test_chain_against_reference_goldens(golden, where):
    import torch
    from polyblur_amd import inverse_filtering_nonsymmetric
    d, g = golden("nonblind.npz"), golden("nonblind_phase.npz")
    x, n = d["x"], 0
    xin = x if where == "numpy" else torch.from_numpy(x).cuda()
    for name in g.files:
        if not name.startswith("phase_"):
            continue
        k, (alpha, b), kw = golden_call(d, name)
        got = inverse_filtering_nonsymmetric(xin, k if where == "numpy" else torch.from_numpy(k).cuda(), alpha, b, **kw)
        if where != "numpy":
            assert isinstance(got, torch.Tensor) and got.device == xin.device and got.dtype == torch.float32
            got = got.cpu().numpy()
        else:
            assert isinstance(got, np.ndarray) and got.dtype == np.float32
        check(got, g[name], TOL_INV, name)
        n += 1
    assert n == 12


@pytest.mark.parametrize("where", ["numpy", "rocm_tensor"])
def test_polynomial_against_reference_goldens(golden, where):
    import torch
    from polyblur_amd import compute_polynomial
    d, g = golden("nonblind.npz"), golden("nonblind_phase.npz")
    n = 0
    for name in g.files:
        if not name.startswith("poly_"):
            continue
        _, shape, method, flag = name.split("_")
        k = d["k_" + shape]
        xp = ref.replicate_pad(d["x"], k.shape[-1] // 2)
        got = compute_polynomial(xp if where == "numpy" else torch.from_numpy(xp).cuda(), k, 2, 3, method=method, not_symmetric=flag == "ns")
        if where != "numpy":
            assert isinstance(got, torch.Tensor) and got.is_cuda
            got = got.cpu().numpy()
        assert got.shape == xp.shape
        check(got, g[name], TOL_INV, name, clamped_chain=False)
        n += 1
    assert n == 4


# ---------------------------------------------------------------------------------------------
# the restatement, every branch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pr.CASES, ids=lambda c: c[0])
def test_chain_against_restatement(case):
    from polyblur_amd import inverse_filtering_nonsymmetric
    x, k = pr.case_inputs(case)
    alpha, b = case[8]
    for form in case[9]:
        full = form == "full"
        got = inverse_filtering_nonsymmetric(x, k, alpha, b, remove_halo=full, do_edgetaper=full)
        want = pr.inverse_filtering_nonsymmetric(x, k, alpha, b, remove_halo=full, do_edgetaper=full)
        check(got, want, TOL_INV, case[0] + " " + form)
    if k.shape[-2] // 2 > k.shape[-1] // 2:
        with pytest.raises(NotImplementedError):
            inverse_filtering_nonsymmetric(x, k, alpha, b, do_edgetaper=True)


def test_three_kernels_differ_and_correlate():
    """the three kernels of the B = 3 case are different ones, and correlate=True is the rotated kernel"""
    from polyblur_amd import inverse_filtering_nonsymmetric
    case = pr.case_named("three_images_three_kernels")
    x, k = pr.case_inputs(case)
    assert maxabs(k[0], k[1]) > 1e-3 and maxabs(k[1], k[2]) > 1e-3
    got = inverse_filtering_nonsymmetric(x, k, 2, 3, correlate=True)
    check(got, pr.inverse_filtering_nonsymmetric(x, k, 2, 3, correlate=True), TOL_INV, "correlate")
    assert maxabs(got, pr.inverse_filtering_nonsymmetric(x, k, 2, 3)) > 1e-2


def test_grad_img_of_the_caller():
    from polyblur_amd import inverse_filtering_nonsymmetric
    case = pr.case_named("k8x8")
    x, k = pr.case_inputs(case)
    other, _ = pr.case_inputs(("other", x.shape, 8300) + case[3:])
    grad = ref.spectral_gradients(other)
    got = inverse_filtering_nonsymmetric(x, k, 2, 3, remove_halo=True, grad_img=grad)
    check(got, pr.inverse_filtering_nonsymmetric(x, k, 2, 3, remove_halo=True, grad_img=grad), TOL_INV, "grad_img")


@pytest.mark.parametrize("case", pr.FP16_CASES, ids=lambda c: c[0])
def test_fp16_images(case):
    """fp16 in, fp16 out, against the restatement on the fp16-rounded input"""
    from polyblur_amd import inverse_filtering_nonsymmetric
    x, k = pr.case_inputs(case)
    xh = x.astype(np.float16)
    for form in case[9]:
        full = form == "full"
        got = inverse_filtering_nonsymmetric(xh, k, *case[8], remove_halo=full, do_edgetaper=full)
        assert got.dtype == np.float16
        want = pr.inverse_filtering_nonsymmetric(xh.astype(np.float32), k, *case[8], remove_halo=full, do_edgetaper=full)
        check(got.astype(np.float32), want, TOL_HALF, case[0] + " " + form)


@pytest.mark.parametrize("method", ["fft", "direct"])
@pytest.mark.parametrize("shape", [(13, 13), (26, 26), (30, 9), (8, 8)], ids=lambda s: "%dx%d" % s)
def test_plain_polynomial_on_the_domain(golden, shape, method):
    """compute_polynomial(..., not_symmetric=False): the existing reblurring passes over the given domain, against the oracle's
    polynomial on the same domain (30 x 9: taller than wide -- p2o is circular over the domain, so 'fft' takes it too)"""
    from polyblur_amd import compute_polynomial
    x = golden("nonblind.npz")["x"]
    k = pr.make_kernel(shape, 8400 + shape[0])
    xp = ref.replicate_pad(x, shape[1] // 2)
    got = compute_polynomial(xp, k, 2, 3, method=method)
    check(got, ref.polynomial_deconvolution(xp, k, 2, 3, method=method), TOL_INV, "%s %s" % (shape, method), clamped_chain=False)


@pytest.mark.parametrize("pcase", pr.POLY_CASES, ids=lambda c: c[0])
def test_phase_polynomial_on_the_domain(pcase):
    """compute_polynomial(..., not_symmetric=True) with one kernel per plane on an un-padded domain of odd sides"""
    from polyblur_amd import compute_polynomial
    x, k = pr.poly_inputs(pcase)
    got = compute_polynomial(x, k, 2, 3, not_symmetric=True)
    check(got, pr.compute_polynomial_fft(x, k, 2, 3), TOL_INV, pcase[0], clamped_chain=False)


# ---------------------------------------------------------------------------------------------
# bits
# ---------------------------------------------------------------------------------------------
def test_an_image_of_a_batch_equals_the_lone_call():
    from polyblur_amd import inverse_filtering_nonsymmetric
    case = pr.case_named("three_images_three_kernels")
    x, k = pr.case_inputs(case)
    for full in (False, True):
        batch = inverse_filtering_nonsymmetric(x, k, 2, 3, remove_halo=full, do_edgetaper=full)
        for i in range(3):
            lone = inverse_filtering_nonsymmetric(x[i:i + 1], k[i:i + 1], 2, 3, remove_halo=full, do_edgetaper=full)
            assert np.array_equal(batch[i:i + 1], lone), (full, i)


def test_scratch_does_not_collide_with_other_calls(eng, golden):
    """the same call after a plain inverse_filtering_rank3 and a blind polyblur_deblurring on the same engine: the same bits"""
    from polyblur_amd import inverse_filtering_nonsymmetric, inverse_filtering_rank3, polyblur_deblurring
    x = golden("nonblind.npz")["x"]
    k = pr.make_kernel((26, 26), 8500)
    first = inverse_filtering_nonsymmetric(x, k, 2, 3, remove_halo=True, do_edgetaper=True)
    plain = inverse_filtering_rank3(x, k, 2, 3, remove_halo=True, do_edgetaper=True, method="fft")
    other, _ = pr.case_inputs(("other", (1, 3, 96, 80), 8501, (3, 3), 1, 1, 1, "dense"))
    polyblur_deblurring(np.ascontiguousarray(np.moveaxis(other[0], 0, -1)), n_iter=2, edgetaping=True, remove_halo=True)
    again = inverse_filtering_nonsymmetric(x, k, 2, 3, remove_halo=True, do_edgetaper=True)
    assert np.array_equal(first, again)
    assert np.array_equal(plain, inverse_filtering_rank3(x, k, 2, 3, remove_halo=True, do_edgetaper=True, method="fft"))
    assert maxabs(first, plain) > 1e-2                     # (two different filters)
    assert eng.workspace_bytes() > 0


@pytest.mark.parametrize("name", ["bluestein_cols_55x48_c4", "mid_530x730"])
def test_plane_group_loop(name):
    """a budget (Engine.set_phase_budget, per context) of one byte: every group of plane pairs is a single pair -- two groups for
    C = 3 or 4 -- and the bits are those of the default budget, which holds every pair of these images in one group"""
    from polyblur_amd.engine import Engine
    x, k = pr.case_inputs(pr.case_named(name))
    outs, used = [], []
    for budget in (0, 1):
        e = Engine(0)
        e.set_phase_budget(budget)
        try:
            ks = e.set_taps(k[:, 0])
            outs.append(e.inverse_filter_phase_taps(x, ks, 2, 3))
            used.append(e.workspace_bytes())
            ks.free()
        finally:
            e.close()
    assert np.array_equal(outs[0], outs[1])
    # (pb_workspace_bytes reports the scratch: the multiplier's plane and two pairs, or one; buffers are sized in units of 256 bytes)
    plane = 8 * (x.shape[2] + 2 * (k.shape[-1] // 2)) * (x.shape[3] + 2 * (k.shape[-1] // 2))
    up = lambda n: (n + 255) // 256 * 256
    assert used[0] - used[1] == up(2 * plane) - up(plane), (used, plane)
    check(outs[1], pr.inverse_filtering_nonsymmetric(x, k, 2, 3), TOL_INV, name + " in groups of one pair")


def test_c_abi_refusals(eng):
    from polyblur_amd._capi import PolyblurHipError
    x, k = pr.case_inputs(pr.case_named("k21x5"))
    ks = eng.set_taps(k[:, 0])
    try:
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG.*not_symmetric"):
            eng.compute_polynomial_taps(x, ks, 2, 3, capi.PB_ZERO, not_symmetric=True)
        with pytest.raises(PolyblurHipError, match="PB_ERR_UNSUPPORTED.*taller than wide"):
            eng.inverse_filter_phase_taps(x, ks, 2, 3, edgetaping=True)
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
            eng.inverse_filter_phase_taps(x[:, :, :17], ks, 2, 3)                     # 21 rows > 17 + 4 - 1
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
            eng.inverse_filter_phase_taps(np.concatenate([x, x]), ks, 2, 3)           # one kernel, two images
        # the plain calls still work with the same set
        check(eng.inverse_filter_phase_taps(x, ks, 2, 3), pr.inverse_filtering_nonsymmetric(x, k, 2, 3), TOL_INV, "21x5")
    finally:
        ks.free()
    wide = eng.set_taps(pr.make_kernel((3, 13), 8601)[:, 0])
    try:
        with pytest.raises(PolyblurHipError, match="PB_ERR_UNSUPPORTED"):
            eng.inverse_filter_phase_taps(np.full((1, 1, 8, 8200), 0.5, np.float32), wide, 2, 3)      # 8212 samples: not held in LDS
    finally:
        wide.free()
