"""Halo masking on the GPU where the mask can be told from a no-op: halo_kernel, grad_energy_kernel and pb_fold_partials_kernel
(csrc/filters.hip) through pb_halo_mask, the three non-blind C entry points and the Python API, with the caller's gradient
planes built by tests/halo_ref.py -- sparse and reversed against the output's x-derivative, another energy for every plane, so
that z = max(M / (nM + M), 0) covers (0, 1) and the mask moves the output by up to 0.7.

Every comparison is against the float64 restatement (halo_ref.halo_f64 behind halo_ref.chain_f64), and against the reference's
own outputs where tests/golden/halo_strong.npz has them.  Every test asserts the gauge (halo_ref.power) first; tests/test_halo_cpu.py
proves without a GPU that each comparison made here rejects every applicable mutant of halo_ref.MUTANTS by ten tolerances.
Tolerances: four times the error of the fp32 NumPy oracle against float64 on the same inputs (halo_ref.TOL_*).

What reaches what (TX / TOut / TG are halo_kernel's types, VEC its four-samples-per-lane form):
  stage 1x3x32x48 float/float/float VEC; 2x3x33x50, 1x1x8x9, 1x1x2x3 scalar; 1x2x34x50 energy sum VEC, mask scalar;
  1x1x2x4 the smallest VEC plane; 1x1x96x128 2 blocks per plane; 1x1x520x512 65 partial sums (the fold's second trip);
  1x1x1024x1028 the cap of 256 blocks; 16385x4x2x4 the plane loop above gridDim.y
  info_*_taper at W = 48: the pitched x operand, VEC (pitch 72, first sample 876 in); taps_k27 / taps_k29: pitched, scalar although
  W % 4 == 0 (pitch 74; first sample 1078 in); W = 50: pitched, scalar
  half_*: __half/__half/float, VEC at W = 48 (plain: x is the fp16 image itself; taper: float/__half/float on the padded plane)
  test_blind_pipeline_fp32: the image's own gradients; prefiltered: the fused recombination (cur != nullptr, fp32)
Not reached with the gauge met: TG = __half and an fp16 `cur`, which only an fp16 blind call from 512 x 640 builds (halo_ref:
no input of that size can meet the gauge; largest effect found 1.4e-4 against a tolerance of 1e-3), and grad0 = None on
(1,1,8,9) / (1,3,12,16) (tests/test_halo_cpu.py::test_own_gradients_do_not_reach_the_gauge).  See DESIGN.md."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import halo_ref as hr
from polyblur_amd import _capi as capi

BOUNDARY = {"fft": capi.PB_WRAP, "direct": capi.PB_ZERO}


@pytest.fixture(scope="module")
def eng():
    from polyblur_amd.engine import get_engine
    return get_engine(0)


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def check(what, got, s, tol, golden_out=None):
    why = hr.power(s["want"], s["unmasked"], tol, s["z"], s["pole"])
    assert why is None, (what, why)
    err = maxabs(got, s["want"])
    print(what, "err %.3g" % err, "tol %.3g" % tol, "the mask's effect %.3g" % maxabs(s["want"], s["unmasked"]),
          "" if golden_out is None else "golden %.3g" % maxabs(got, golden_out))
    assert err < tol, (what, err)
    if golden_out is not None:
        assert maxabs(got, golden_out) < tol, (what, maxabs(got, golden_out))


# ---------------------------------------------------------------------------------------------
# the stage: Engine.halo_mask -> pb_halo_mask, fp32, no clamp
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hr.STAGE_SHAPES, ids=hr.shape_id)
def test_stage(eng, golden, shape):
    s = hr.stage_set(shape)
    got = eng.halo_mask(s["x"], s["y32"], s["gx"], s["gy"])
    want_ref = golden("halo_strong.npz")["w%d_halo" % shape[-1]] if shape in hr.GOLDEN_SHAPES else None
    check(hr.shape_id(shape), got, s, hr.TOL_STAGE, want_ref)


# ---------------------------------------------------------------------------------------------
# the non-blind entry points with grad0 of the caller
# ---------------------------------------------------------------------------------------------
def run_case(eng, s):
    x, k, grad = s["x"], s["k"], (s["gx"], s["gy"])
    if s["entry"] == "info":
        buf = eng.set_kernels(k[:, 0])
        return eng.inverse_filter(x, buf, hr.ALPHA, hr.BETA, BOUNDARY[s["method"]], edgetaping=s["taper"], remove_halo=True, grad0=grad)
    if s["entry"] in ("taps", "phase"):
        ks = eng.set_taps(k[:, 0])
        try:
            if s["entry"] == "phase":
                return eng.inverse_filter_phase_taps(x, ks, hr.ALPHA, hr.BETA, edgetaping=s["taper"], remove_halo=True, grad0=grad)
            return eng.inverse_filter_taps(x, ks, hr.ALPHA, hr.BETA, BOUNDARY[s["method"]], edgetaping=s["taper"], remove_halo=True, grad0=grad)
        finally:
            ks.free()
    from polyblur_amd import inverse_filtering_rank3, inverse_filtering_nonsymmetric
    if s["entry"] == "rank3":
        return inverse_filtering_rank3(x, k, hr.ALPHA, hr.BETA, remove_halo=True, do_edgetaper=s["taper"], grad_img=grad, method=s["method"])
    return inverse_filtering_nonsymmetric(x, k, hr.ALPHA, hr.BETA, remove_halo=True, do_edgetaper=s["taper"], grad_img=grad)


@pytest.mark.parametrize("name", [c[0] for c in hr.INVERSE_CASES])
def test_inverse_filter_fp32(eng, name):
    s = hr.inverse_set(name)
    got = run_case(eng, s)
    assert got.dtype == np.float32 and got.shape == s["x"].shape
    check(name, got, s, hr.TOL_INV)


@pytest.mark.parametrize("name", [c[0] for c in hr.HALF_CASES])
def test_inverse_filter_fp16_images(eng, name):
    """fp16 in, fp16 out, fp32 gradient planes; the float64 chain on the fp16 image"""
    s = hr.inverse_set(name)
    assert s["x"].dtype == np.float16
    got = run_case(eng, s)
    assert got.dtype == np.float16
    check(name, got, s, hr.TOL_INV_HALF)


@pytest.mark.parametrize("method,taper", hr.GOLDEN_VARIANTS)
@pytest.mark.parametrize("shape", hr.GOLDEN_SHAPES, ids=hr.shape_id)
def test_python_api_against_reference(golden, shape, method, taper):
    """inverse_filtering_rank3(..., grad_img=...) on ndarrays against the reference's own outputs (and float64)"""
    from polyblur_amd import inverse_filtering_rank3
    g, tag = golden("halo_strong.npz"), "w%d" % shape[-1]
    x, k, gx, gy = (g["%s_%s" % (tag, n)] for n in ("image", "k", "igx", "igy"))
    _, xc, y, _ = hr.chain_f64(x, k, taper, method)
    want, z, pole = hr.halo_f64(xc, y, gx, gy, True, parts=True)
    got = inverse_filtering_rank3(x, k, hr.ALPHA, hr.BETA, remove_halo=True, do_edgetaper=taper, grad_img=(gx, gy), method=method)
    check("%s %s %s" % (tag, method, taper), got, dict(want=want, unmasked=np.clip(y, 0, 1), z=z, pole=pole), hr.TOL_INV,
          g["%s_inv_%s_%s" % (tag, method, "taper" if taper else "plain")])


@pytest.mark.parametrize("name", ["rank3_w50_direct", "nonsym_w48", "half_rank3_w48", "half_nonsym_w50"])
def test_python_api_on_device_tensors(name):
    """the same sets with image, kernel and gradient planes as tensors on the GPU: the result stays there, in the image's type.
    (rank3_w50_direct and half_nonsym_w50: three channels of two images, every plane with a gradient scale of its own)"""
    import torch
    from polyblur_amd import inverse_filtering_rank3, inverse_filtering_nonsymmetric
    s = hr.inverse_set(name)
    half = s["x"].dtype == np.float16
    x = torch.from_numpy(np.array(s["x"])).cuda()
    grad = tuple(torch.from_numpy(np.array(g)).cuda() for g in (s["gx"], s["gy"]))
    k = torch.from_numpy(np.array(s["k"])).cuda()
    if s["entry"] == "rank3":
        got = inverse_filtering_rank3(x, k, hr.ALPHA, hr.BETA, remove_halo=True, do_edgetaper=s["taper"], grad_img=grad, method=s["method"])
    else:
        got = inverse_filtering_nonsymmetric(x, k, hr.ALPHA, hr.BETA, remove_halo=True, do_edgetaper=s["taper"], grad_img=grad)
    assert isinstance(got, torch.Tensor) and got.device == x.device and got.dtype == x.dtype
    check(name, got.float().cpu().numpy(), s, hr.TOL_INV_HALF if half else hr.TOL_INV)


# ---------------------------------------------------------------------------------------------
# the blind pipeline: the image's own gradients, an input found so that the gauge holds (halo_ref.pipeline_set)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_tensor", [False, True], ids=["ndarray", "tensor"])
@pytest.mark.parametrize("prefiltering", [False, True], ids=["plain", "prefiltered"])
def test_blind_pipeline_fp32(prefiltering, device_tensor):
    """polyblur_deblurring(..., remove_halo=True) on (1,3,24,40) against the oracle at the project's 2e-5, the gauge at 20
    tolerances, the same theta on both sides.  prefiltered: the halo kernel recombines as it stores (cur != nullptr)."""
    from polyblur_amd import polyblur_deblurring
    s = hr.pipeline_set(prefiltering)
    why = hr.power(s["want"], s["unmasked"], hr.TOL_PIPE, s["z"], s["pole"], factor=20)
    assert why is None, why
    if device_tensor:
        import torch
        out, infos = polyblur_deblurring(torch.from_numpy(np.array(s["x"])).cuda(), prefiltering=prefiltering, return_info=True, **hr.PIPE_KW)
        out = out.cpu().numpy()
    else:                                                     # (an ndarray is one (H,W,C) image)
        out, infos = polyblur_deblurring(np.ascontiguousarray(np.moveaxis(s["x"][0], 0, -1)), prefiltering=prefiltering,
                                         return_info=True, **hr.PIPE_KW)
        out = np.moveaxis(out, -1, 0)[None]
    assert [float(i["theta"][0]) for i in infos] == s["theta"]
    err = maxabs(out, s["oracle"])
    print("prefiltering", prefiltering, "err %.3g" % err, "vs float64 %.3g" % maxabs(out, s["want"]),
          "the mask's effect %.3g" % maxabs(s["want"], s["unmasked"]))
    assert err < hr.TOL_PIPE, err
