"""The pure-phase filter for kernels that are not point-symmetric (reference deblurring.py:141-169, not_symmetric=True), host
side: the public names and signatures, the two C entry points, every refusal -- raised before any device work, so they hold
on a box without a GPU --, the local restatement (tests/phase_ref.py) against the reference's own outputs
(tests/golden/nonblind_phase.npz, written by tests/golden/make_golden_phase.py), and the conditioning of every input
tests/test_gpu_phase.py compares on.

The restatement reproduces every golden within 3e-6 (the figure tests/test_nonblind_cpu.py uses for the oracle); measured:
1.6e-6 at most.

The conditioning condition: 1 / |K| amplifies fp32 roundoff where |K| is small, in the reference as much as in the engine, so a
GPU comparison at 2e-5 means something only where two evaluations of the same formula agree far better than that.  For every
(shape, kernel, alpha, b) of the GPU tests the complex64 and complex128 restatements differ by at most 2e-6 -- one tenth of
the GPU tolerance -- and at most 1 % of the clamped chain's samples sit at exactly 0 or 1.  Measured: 4.9e-7 and 0.04 % at most
over tests/phase_ref.py's cases, 1.2e-6 and 0.65 % over the goldens' inputs; min |K| 5e-5 .. 1.0."""
import inspect

import numpy as np
import pytest

import phase_ref as pr
from oracle import polyblur_ref as ref
from polyblur_amd import _capi as capi

TOL_RESTATEMENT = 3e-6
TOL_CONDITIONING = 2e-6


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def golden_call(d, name):
    """name of a chain golden -> (kernel, alpha, b, keyword arguments)"""
    p = name.split("_")
    ab = {"a2b3": (2, 3), "a6b1": (6, 1)}[p[-1]]
    if p[1] == "correlate":
        return d["k_" + p[2]], ab, dict(correlate=True)
    if p[1] == "perchannel":
        return d["k_perchannel_" + p[2]], ab, dict(remove_halo=True)
    full = p[2] == "full"
    return d["k_" + p[1]], ab, dict(remove_halo=full, do_edgetaper=full)


def test_exports_and_signatures():
    import polyblur_amd
    for name in ("compute_polynomial", "inverse_filtering_nonsymmetric"):
        assert name in polyblur_amd.__all__ and callable(getattr(polyblur_amd, name))
    sig = inspect.signature(polyblur_amd.compute_polynomial)
    assert list(sig.parameters) == ["img", "kernel", "alpha", "b", "method", "not_symmetric"]
    assert sig.parameters["method"].default == "fft" and sig.parameters["not_symmetric"].default is False
    assert sig.parameters["alpha"].default is inspect.Parameter.empty and sig.parameters["b"].default is inspect.Parameter.empty
    sig = inspect.signature(polyblur_amd.inverse_filtering_nonsymmetric)
    assert list(sig.parameters) == ["img", "kernel", "alpha", "b", "correlate", "remove_halo", "do_edgetaper", "grad_img"]
    assert [sig.parameters[n].default for n in list(sig.parameters)[2:]] == [2, 4, False, False, False, None]
    # (the existing function keeps its parameter list)
    assert list(inspect.signature(polyblur_amd.inverse_filtering_rank3).parameters)[-1] == "method"


def test_library_has_the_entry_points():
    lib = capi.load_library()
    for name in ("pb_compute_polynomial_taps", "pb_inverse_filter_phase_taps"):
        assert name in capi.SYMBOLS and hasattr(lib, name)
    from polyblur_amd.engine import Engine
    for name in ("compute_polynomial_taps", "compute_polynomial_taps_ptr", "inverse_filter_phase_taps", "inverse_filter_phase_taps_ptr"):
        assert callable(getattr(Engine, name))
    assert lib.pb_version() == 200


def test_refusals_come_before_any_device_work():
    from polyblur_amd import compute_polynomial, inverse_filtering_nonsymmetric
    x = np.full((1, 3, 40, 50), 0.5, np.float32)
    k = pr.make_kernel((5, 7), 1)
    both = (lambda kk, xx=x: compute_polynomial(xx, kk, 2, 3, not_symmetric=True),
            lambda kk, xx=x: inverse_filtering_nonsymmetric(xx, kk, 2, 3))
    for fn in both:
        with pytest.raises(NotImplementedError):
            fn((k, k))                                                   # tuple kernels
        with pytest.raises(TypeError):
            fn(3.0)                                                      # not an array
        with pytest.raises(ValueError):
            fn(k[0])                                                     # not (B,C,h,w)
        with pytest.raises(ValueError):
            fn(pr.make_kernel((5, 7), 1, batch=2))                       # batch 2 for one image
        with pytest.raises(ValueError):
            fn(pr.make_kernel((5, 7), 1, channels=2))                    # 2 planes for 3 channels
        with pytest.raises(ValueError):
            fn(pr.make_kernel((5, 1), 1))                                # one tap wide
        with pytest.raises(NotImplementedError):
            fn(pr.make_kernel((50, 5), 1))                               # a side above 49
        with pytest.raises(NotImplementedError):
            fn(pr.make_kernel((5, 50), 1))
    with pytest.raises(ValueError):
        compute_polynomial(x[..., :20, :], pr.make_kernel((21, 5), 1), 2, 3, not_symmetric=True)     # 21 rows > 20 - 1
    with pytest.raises(ValueError):
        inverse_filtering_nonsymmetric(x[..., :17, :], pr.make_kernel((21, 5), 1), 2, 3)              # 21 rows > 17 + 4 - 1
    with pytest.raises(ValueError):
        compute_polynomial(x, k, 2, 3, method="direct", not_symmetric=True)
    with pytest.raises(ValueError):
        compute_polynomial(x, k, 2, 3, method="nope")
    with pytest.raises(NotImplementedError):
        compute_polynomial(x, k, 2, 3, method="direct_separable")
    # a padded side whose lines are not held in LDS: 8200 + 2 * 6 = 8212 = 4 * 2053 needs a Bluestein core of 32768 points
    assert capi.load_library().pb_fft_length_supported(8212) == 2
    wide = np.full((1, 1, 8, 8200), 0.5, np.float32)
    with pytest.raises(NotImplementedError):
        inverse_filtering_nonsymmetric(wide, pr.make_kernel((3, 13), 1), 2, 3)
    with pytest.raises(NotImplementedError):
        compute_polynomial(np.full((1, 1, 8, 8212), 0.5, np.float32), pr.make_kernel((3, 13), 1), 2, 3, not_symmetric=True)
    # a kernel taller than wide: with the edgetaper only (its circular pad by the half-width is no circular convolution)
    with pytest.raises(NotImplementedError):
        inverse_filtering_nonsymmetric(x, pr.make_kernel((21, 5), 1), 2, 3, do_edgetaper=True)
    with pytest.raises(ValueError):
        inverse_filtering_nonsymmetric(x, k, 2, 3, remove_halo=True, grad_img=(x,))
    with pytest.raises(ValueError):
        inverse_filtering_nonsymmetric(x, k, 2, 3, remove_halo=True, grad_img=(x[:, :1], x[:, :1]))


def test_restatement_reproduces_the_reference(golden):
    d, g = golden("nonblind.npz"), golden("nonblind_phase.npz")
    x, worst, n = d["x"], 0.0, 0
    for name in g.files:
        if name.startswith("phase_"):
            k, (alpha, b), kw = golden_call(d, name)
            got = pr.inverse_filtering_nonsymmetric(x, k, alpha, b, **kw)
        else:
            _, shape, method, flag = name.split("_")
            k = d["k_" + shape]
            xp = ref.replicate_pad(x, k.shape[-1] // 2)
            if method == "direct":
                got = ref.polynomial_deconvolution(xp, k, 2, 3, method="direct")
            else:
                got = pr.compute_polynomial_fft(xp, k, 2, 3, not_symmetric=flag == "ns")
        err = maxabs(got, g[name])
        print(name, "err %.3g" % err)
        assert err < TOL_RESTATEMENT, (name, err)
        worst, n = max(worst, err), n + 1
    print("worst %.3g" % worst)
    assert n == 16
    # the filter matters: without it the polynomial is somewhere else entirely
    assert maxabs(g["poly_25x24_fft_ns"], g["poly_25x24_fft_sym"]) > 0.1


def check_conditioning(what, x, k, alpha, b, **kw):
    y32 = pr.inverse_filtering_nonsymmetric(x, k, alpha, b, **kw)
    y64 = pr.inverse_filtering_nonsymmetric(x, k, alpha, b, double=True, **kw)
    err, clamped = maxabs(y32, y64), float(np.mean((y32 == 0) | (y32 == 1)))
    print(what, "complex64 vs complex128 %.3g" % err, "clamped %.2f %%" % (100 * clamped))
    assert err <= TOL_CONDITIONING, (what, err)
    assert clamped <= 0.01, (what, clamped)


def check_conditioning_unclamped(what, x, k, alpha, b):
    """compute_polynomial(..., not_symmetric=True) on the given domain: no clamp, so only the first bound"""
    err = maxabs(pr.compute_polynomial_fft(x, k, alpha, b), pr.compute_polynomial_fft(x, k, alpha, b, double=True))
    print(what, "complex64 vs complex128 %.3g" % err)
    assert err <= TOL_CONDITIONING, (what, err)


def test_conditioning_of_the_golden_inputs(golden):
    d, g = golden("nonblind.npz"), golden("nonblind_phase.npz")
    for name in g.files:
        if name.startswith("phase_"):
            k, (alpha, b), kw = golden_call(d, name)
            check_conditioning(name, d["x"], k, alpha, b, **kw)
        elif name.endswith("_ns"):
            k = d["k_" + name.split("_")[1]]
            check_conditioning_unclamped(name, ref.replicate_pad(d["x"], k.shape[-1] // 2), k, 2, 3)


@pytest.mark.parametrize("case", pr.CASES + pr.FP16_CASES, ids=lambda c: c[0])
def test_conditioning_of_the_gpu_cases(case):
    x, k = pr.case_inputs(case)
    if case in pr.FP16_CASES:
        x = x.astype(np.float16).astype(np.float32)
    for form in case[9]:
        full = form == "full"
        check_conditioning(case[0] + " " + form, x, k, *case[8], remove_halo=full, do_edgetaper=full)


@pytest.mark.parametrize("pcase", pr.POLY_CASES, ids=lambda c: c[0])
def test_conditioning_of_the_gpu_polynomial_cases(pcase):
    x, k = pr.poly_inputs(pcase)
    check_conditioning_unclamped(pcase[0], x, k, 2, 3)


def test_conditioning_of_the_correlate_case():
    x, k = pr.case_inputs(pr.case_named("three_images_three_kernels"))
    check_conditioning("correlate", x, k, 2, 3, correlate=True)
