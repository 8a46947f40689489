"""Gradients of the non-blind step, the part that needs no GPU:

  * tests/autograd_ref.py -- the float64 restatement -- against the reference's own autograd (tests/golden/nonblind_grad.npz,
    written by tests/golden/make_golden_autograd.py) to about 1e-12, and its hand-written K^T and L(u, v) against torch.autograd;
  * the new C symbols are declared, exported and bound, and every refusal under grad is raised before any device work;
  * the conditions the GPU test (tests/test_gpu_autograd.py) relies on, asserted here for every one of its cases:
      - the kernel-gradient tolerance ar.TOL_K is 4 x the largest normalised error of the float32 CPU evaluation of the
        restatement against float64 (normalised per lag by sum |u| |v|; measured here: 4.78e-7, on the 49 x 49 rank-3 golden under 'direct');
      - discriminating power: taking every lag one sample off changes the tap gradient by more than 10 x ar.TOL_K in the
        statistic the GPU test asserts (the largest normalised error over the lags);
      - clamp margin: no unclamped float64 output of an inverse_filtering_rank3 case within 1e-3 of 0 or 1, at least 5 % clamped."""
import json
import os
import re

import numpy as np
import pytest
import torch

import autograd_ref as ar
from polyblur_amd import _capi as capi

NEW_SYMBOLS = ["pb_tap_gradient", "pb_convolve2d_taps_backward", "pb_compute_polynomial_taps_backward"]
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden_cases(golden):
    d = golden("nonblind_grad.npz")
    for c in json.loads(str(d["cases"])):
        n = c["name"]
        yield c, d[n + "_x"], d[n + "_w"], d[n + "_k"], d[n + "_gx"], d[n + "_gk"]


@pytest.fixture(scope="module")
def table(golden):
    """per kernel-gradient case (the GPU test's and the goldens'): float64 kernel.grad and its normaliser, the float32 evaluation,
    the gradient with every lag one sample off; per tap-gradient-alone case the same for L(w, x)"""
    rows = []
    todo = [(cid, func, method, x, w, k, ar.ALPHA, ar.BETA, False) for cid, func, method, x, w, k in ar.gpu_cases()]
    todo += [(c["name"], c["func"], c["method"], x, w, k, c["alpha"], c["b"], c["correlate"]) for c, x, w, k, _, _ in golden_cases(golden)]
    for cid, func, method, x, w, k, alpha, b, correlate in todo:
        gk, norm = ar.kernel_grad_parts(func, x, k, w, alpha, b, method, correlate)
        off, _ = ar.kernel_grad_parts(func, x, k, w, alpha, b, method, correlate, shift=True)
        _, _, gk32 = ar.gradients(func, x, k, w, alpha, b, method, correlate, dtype=torch.float32)
        rows.append((cid, ar.normalised_error(gk32, gk, norm), ar.normalised_error(off, gk, norm)))
    for cid, method, x, w, k in ar.tap_cases():
        want, norm = ar.lag(w, x, k.shape, method), ar.lag(np.abs(w), np.abs(x), k.shape, method)
        off = ar.lag(w, ar.shifted(x.astype(np.float64), 0, 1, method), k.shape, method)
        rows.append(("tap-" + cid, ar.normalised_error(ar.lag(w, x, k.shape, method, dtype=torch.float32), want, norm),
                     ar.normalised_error(off, want, norm)))
    return rows


def test_restatement_matches_the_reference(golden):
    n = 0
    for c, x, w, k, gx, gk in golden_cases(golden):
        _, rx, rk = ar.gradients(c["func"], x, k, w, c["alpha"], c["b"], c["method"], c["correlate"])
        ex, ek = np.abs(rx - gx).max() / max(1.0, np.abs(gx).max()), np.abs(rk - gk).max() / max(1.0, np.abs(gk).max())
        print(c["name"], c["func"], c["method"], "grad_x %.2g grad_k %.2g" % (ex, ek))
        assert ex < 1e-12 and ek < 1e-12, (c, ex, ek)
        n += 1
    assert n == 20


@pytest.mark.parametrize("method", ["fft", "direct"])
@pytest.mark.parametrize("kshape", [(2, 1, 3, 3), (2, 3, 5, 9), (1, 1, 1, 5), (1, 1, 7, 3)])
def test_hand_written_adjoint_and_lag_match_autograd(method, kshape):
    rng = np.random.default_rng(11)
    x, w, k = rng.random((2, 3, 10, 13)), rng.uniform(-1, 1, (2, 3, 10, 13)), rng.random(kshape)
    for func in ("convolve2d", "polynomial"):
        _, gx, gk = ar.gradients(func, x, k, w, 6, 1, method)
        hx, hk, norm = ar.hand_gradients(func, x, k, w, 6, 1, method)
        assert np.abs(hx - gx).max() <= 1e-12 * max(1.0, np.abs(gx).max()), (func, method)
        assert ar.normalised_error(hk, gk, norm) < 1e-14, (func, method)
        # ... and the torch statement of the same parts, which the tests use where 2401 lags would be slow by hand
        pk, pnorm = ar.kernel_grad_parts(func, x, k, w, 6, 1, method)
        assert ar.normalised_error(pk, gk, norm) < 1e-14 and np.allclose(pnorm, norm, rtol=1e-12)
        if method == "fft":                                 # (under 'direct' a shifted operand loses its first column: not the same thing at the edge)
            off, _ = ar.kernel_grad_parts(func, x, k, w, 6, 1, method, shift=True)
            _, hoff, _ = ar.hand_gradients(func, x, k, w, 6, 1, method, extra=(0, 1))
            assert ar.normalised_error(off, hoff, norm) < 1e-14
    assert np.abs(ar.hand_k(w, k, method, adjoint=True) - ar.adjoint(w, k, method)).max() < 1e-13
    # <K x, g> == <x, K^T g>
    assert abs(np.vdot(ar.hand_k(x, k, method), w) - np.vdot(x, ar.hand_k(w, k, method, adjoint=True))) < 1e-10


def test_new_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "polyblur_hip.h")).read()
    lib = capi.load_library()
    from polyblur_amd.engine import Engine
    for name in NEW_SYMBOLS:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.SYMBOLS
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) >= 11
    for name in ("tap_gradient_ptr", "convolve2d_taps_backward_ptr", "compute_polynomial_taps_backward_ptr"):
        assert callable(getattr(Engine, name))
    # the header cites what each is the derivative of, and the reference's claim
    assert "fully differentiable" in header and "filters.py:14-37" in header and "deblurring.py:113-169" in header
    assert header.count("#define PB_PROF_NTAGS 10") == 1


def _refusals():
    import polyblur_amd as pa
    x = torch.rand(1, 3, 16, 18)
    k = torch.rand(1, 1, 3, 5)
    xg, kg = x.clone().requires_grad_(True), k.clone().requires_grad_(True)
    even = torch.rand(1, 1, 4, 5)
    return [
        ("float16", lambda: pa.inverse_filtering_rank3(x.half(), kg, 6, 1, method="fft")),
        ("ROCm tensors only", lambda: pa.convolve2d(xg, k, method="fft")),
        ("ROCm tensors only", lambda: pa.compute_polynomial(x, kg, 6, 1, method="direct")),
        ("ROCm tensors only", lambda: pa.inverse_filtering_rank3(xg, kg, 6, 1)),
        ("ROCm tensors only", lambda: pa.compute_polynomial(x.numpy(), kg, 6, 1)),
        ("odd sides only", lambda: pa.convolve2d(xg, even, method="direct")),
        ("odd sides only", lambda: pa.compute_polynomial(xg, torch.rand(1, 1, 3, 4), 6, 1)),
        ("odd sides only", lambda: pa.inverse_filtering_rank3(xg, torch.rand(1, 1, 6, 6), 6, 1)),
        ("halo masking", lambda: pa.inverse_filtering_rank3(xg, k, 6, 1, remove_halo=True)),
        ("edgetaper is not", lambda: pa.inverse_filtering_rank3(xg, k, 6, 1, do_edgetaper=True, method="fft")),
        ("edgetaper has no backward", lambda: pa.edgetaper(xg, k)),
        ("edgetaper has no backward", lambda: pa.edgetaper(x, kg)),
        ("pure-phase", lambda: pa.compute_polynomial(xg, k, 6, 1, method="fft", not_symmetric=True)),
        ("pure-phase", lambda: pa.inverse_filtering_nonsymmetric(xg, k, 6, 1)),
        ("pure-phase", lambda: pa.inverse_filtering_nonsymmetric(x, kg, 6, 1)),
    ]


def test_every_refusal_under_grad_comes_before_any_device_work():
    for pattern, call in _refusals():
        with pytest.raises(NotImplementedError, match=pattern) as e:
            call()
        assert "\n" not in str(e.value)                     # a one-line reason


def test_without_grad_nothing_is_refused_that_was_not_before():
    """the same call under torch.no_grad() gets past the new checks (and then runs, or fails on a missing GPU, as before)"""
    import polyblur_amd as pa
    xg, k = torch.rand(1, 3, 16, 18, requires_grad=True), torch.rand(1, 1, 4, 5)
    with torch.no_grad():
        try:
            y = pa.convolve2d(xg, k, method="direct")
        except NotImplementedError:
            raise
        except Exception:                                   # (no GPU here)
            return
    assert not y.requires_grad and tuple(y.shape) == (1, 3, 16, 18)


def test_kernel_gradient_tolerance_is_four_times_the_fp32_cpu_error(table):
    worst = max(table, key=lambda r: r[1])
    for cid, e32, _ in table:
        print("%-44s fp32 vs float64, normalised: %.3g" % (cid, e32))
    print("largest:", worst[0], worst[1], "-> 4 x = %.3g; ar.TOL_K = %.3g" % (4 * worst[1], ar.TOL_K))
    # the constant was derived from this measurement (4.78e-7); a re-measurement on another CPU sums in another order and must land
    # within a factor 1.5 of it -- beyond that the constant is stale
    assert ar.TOL_K / 1.5 <= 4 * worst[1] <= ar.TOL_K * 1.5


def test_every_kernel_gradient_case_tells_a_lag_one_sample_off(table):
    for cid, _, off in table:
        print("%-44s one sample off: %.3g (needs > %.3g)" % (cid, off, 10 * ar.TOL_K))
        assert off > 10 * ar.TOL_K, (cid, off)


def test_clamp_margin_of_every_rank3_case(golden):
    todo = [(cid, method, x, k, ar.ALPHA, ar.BETA, False) for cid, func, method, x, w, k in ar.gpu_cases() if func == "rank3"]
    todo += [(c["name"], c["method"], x, k, c["alpha"], c["b"], c["correlate"]) for c, x, w, k, _, _ in golden_cases(golden) if c["func"] == "rank3"]
    assert len(todo) == 10 + 9
    for cid, method, x, k, alpha, b, correlate in todo:
        y = ar.rank3_unclamped(torch.tensor(x, dtype=torch.float64), torch.tensor(k, dtype=torch.float64), alpha, b, method, correlate).numpy()
        margin, clamped = ar.clamp_margin(y)
        print("%-36s margin %.2g clamped %.1f %%" % (cid, margin, 100 * clamped))
        assert margin > 1e-3 and clamped >= 0.05, (cid, margin, clamped)
