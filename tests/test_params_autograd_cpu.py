"""Learnable parameters, the part that needs no GPU:

  * tests/params_grad_ref.py -- the float64 restatement of the gradients with respect to alpha, beta, c and b -- against the
    reference's own autograd (tests/golden/params_grad.npz, written by tests/golden/make_golden_params_autograd.py): its float64
    gradients of the polynomial to 1e-10 of the case's larger one, its float32 gradients to the tolerances of params_grad_ref.py;
  * those tolerances lie between 4 E and 8 E of their own setting -- per case for the polynomial, per clamp state for the estimation,
    per (alpha, beta, method) for the blind call --, E the reference's own float32 error against the float64 truth, measured here again;
  * every polynomial case has min(|d alpha|, |d beta|) >= 0.1 max(...): no case tests a near-zero scalar; the estimation cases have
    the clamp states their names say, and the case on which both variances clamp gives exactly (0, 0);
  * mutants -- the 1/2 dropped, the `+ x` of d beta dropped, the clamp's gate ignored, one plane in place of the sum over planes, eps left
    out of d c, the last iteration's contribution alone -- are off by at least 1e-3 of the case's larger gradient wherever they can
    move it;
  * the header's prototypes and scratch names, PB_VERSION 200, the bindings; a NULL context is refused by both entry points;
  * the Python refusals, on CPU tensors, before any device work."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import estimation_grad_ref as er
import params_grad_ref as pr
from frontend_cases import no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases():
    return pr.load_golden()


@pytest.fixture(scope="module")
def poly_rows(cases):
    """per polynomial case: (case, image, weights, kernel, the restatement's rows)"""
    z, cs = cases
    out = []
    for c in cs:
        if c["kind"] != "poly":
            continue
        x, w = pr.smooth_image(c["seed"], tuple(c["xshape"]))
        k = z[c["name"] + "_k"]
        rows = pr.poly_param_rows(x, k, w, c["method"]) if c["func"] == "polynomial" else pr.rank3_param_rows(x, k, w, c["alpha"], c["beta"], c["method"])
        out.append((c, x, w, k, rows))
    return out


@pytest.fixture(scope="module")
def est_rows(cases):
    """per estimation case: (case, the forward's records, weights, the restatement's rows)"""
    z, cs = cases
    out = []
    for c in cs:
        if c["kind"] == "estimation":
            recs = er.estimate(z[c["name"] + "_x"], pr.EST_C, pr.EST_B)
            out.append((c, recs, z[c["name"] + "_w"], pr.estimation_param_rows(recs, z[c["name"] + "_w"])))
    return out


@pytest.fixture(scope="module")
def blind_rows(cases):
    """per blind case: (case, the iterations, weights, the restatement's four gradients)"""
    z, cs = cases
    out = []
    for c in cs:
        if c["kind"] == "blind":
            x, w = z[c["name"] + "_x"], z[c["name"] + "_w"]
            _, steps = er.blind(x, c["n_iter"], c["alpha"], c["beta"], c["method"], pr.BLIND_C, pr.BLIND_B)
            out.append((c, steps, w, pr.blind_param_grads(x, w, c["n_iter"], c["alpha"], c["beta"], c["method"], steps=steps)))
    return out


def test_case_lists_are_the_committed_ones(cases):
    z, cs = cases
    poly = [c for c in cs if c["kind"] == "poly"]
    assert [(c["func"], tuple(c["xshape"]), tuple(c["kshape"]), c["kernel"], c["method"], (c["alpha"], c["beta"])) for c in poly] == pr.POLY
    assert sum(c["kind"] == "estimation" for c in cs) == len(pr.ESTIMATION) and sum(c["kind"] == "blind" for c in cs) == 7
    assert {c["n_iter"] for c in cs if c["kind"] == "blind"} == {1, 2, 3}
    assert os.path.getsize(pr.GOLDEN) < os.path.getsize(os.path.join(os.path.dirname(pr.GOLDEN), "dt_grad.npz"))
    # what the shape list is for: every side, channel count, kernel size and kind, both methods, both settings, both kernel layouts
    assert {c["xshape"][3] for c in poly} == {10, 63, 64, 65, 130} and {c["xshape"][2] for c in poly} == {6, 17, 33}
    assert {c["xshape"][1] for c in poly} == {1, 3, 4} and {tuple(c["kshape"][2:]) for c in poly} == {(3, 3), (5, 9), (25, 25)}
    assert {c["kernel"] for c in poly} == {"rank1", "oblique", "dense"} and {c["method"] for c in poly} == {"fft", "direct"}
    assert {(c["alpha"], c["beta"]) for c in poly} == {(6, 1), (2, 3)} and {c["kshape"][1] > 1 for c in poly} == {True, False}
    assert all(c["xshape"][0] == (1 if c["method"] == "direct" else 2) for c in poly)


def test_polynomial_restatement_against_the_references_float64(cases, poly_rows):
    z, _ = cases
    for c, x, w, k, rows in poly_rows:
        g64 = z[c["name"] + "_g64"]
        e = pr.rel_error(rows.sum(axis=0), g64)
        print("%s %-10s %s restatement vs float64 golden: %.3g" % (c["name"], c["func"], c["method"], e))
        assert e <= 1e-10, (c["name"], e)
        assert np.abs(g64).min() >= 0.1 * np.abs(g64).max(), c["name"]         # no near-zero scalar under test


def test_tolerances_are_held_to_the_references_float32_error(cases, poly_rows, est_rows, blind_rows):
    z, _ = cases
    e_poly = {c["name"]: pr.rel_error(z[c["name"] + "_g32"], z[c["name"] + "_g64"]) for c, *_ in poly_rows}      # per case
    e_est, e_blind = {}, {}
    for c, _, _, rows in est_rows:                                              # per clamp state: the largest over its cases
        if pr.est_setting(c) != "both":
            e_est[pr.est_setting(c)] = max(e_est.get(pr.est_setting(c), 0.0), pr.rel_error(z[c["name"] + "_g32"], rows.sum(axis=0)))
    for c, _, _, g in blind_rows:                                               # per (alpha, beta, method): the largest over n_iter
        e_blind[pr.blind_setting(c)] = max(e_blind.get(pr.blind_setting(c), 0.0), pr.rel_error(z[c["name"] + "_g32"], g))
    for kind, measured, recorded, tols in (("polynomial", e_poly, pr.E_POLY, pr.TOL_POLY), ("estimation", e_est, pr.E_EST, pr.TOL_EST),
                                           ("blind", e_blind, pr.E_BLIND, pr.TOL_BLIND)):
        assert set(measured) == set(recorded) == set(tols), (kind, sorted(measured, key=str))
        for key, e in measured.items():
            print("%-10s %-18s E = %.3g (recorded %.3g), tolerance %.3g = %.2f E" % (kind, key, e, recorded[key], tols[key], tols[key] / e))
            assert abs(e - recorded[key]) <= 0.02 * recorded[key], (kind, key, e)   # the recorded figure is this measurement
            assert 4 * e <= tols[key] <= 8 * e, (kind, key, e, tols[key])


def test_float32_goldens_within_the_tolerances(cases, poly_rows, est_rows, blind_rows):
    z, _ = cases
    for c, x, w, k, rows in poly_rows:
        assert pr.rel_error(z[c["name"] + "_g32"], rows.sum(axis=0)) <= pr.TOL_POLY[c["name"]], c["name"]
    for c, recs, w, rows in est_rows:
        g32 = z[c["name"] + "_g32"]
        if not np.abs(rows).max() > 0:
            assert not g32.any() and not rows.any(), c["name"]
        else:
            assert pr.rel_error(g32, rows.sum(axis=0)) <= pr.TOL_EST[pr.est_setting(c)], c["name"]
    for c, steps, w, g in blind_rows:
        assert pr.rel_error(z[c["name"] + "_g32"], g) <= pr.TOL_BLIND[pr.blind_setting(c)], c["name"]


def test_clamp_states_of_the_estimation_cases(est_rows):
    seen = set()
    for (c, recs, w, rows), (shape, sig, want) in zip(est_rows, pr.ESTIMATION):
        m = er.margins(recs)
        assert er.case_ok(recs), (c["name"], m)
        assert [list(f) for f in m[4]] == c["clamped"] and (want is None or all(f == want for f in m[4])), (c["name"], m[4])
        seen.update(m[4])
        if want == pr.BOTH_CLAMPED:
            # an unblurred noise image: both variances below 0.09, sigma = rho = 0.3, and nothing passes the clamp -- exactly (0, 0)
            assert all(float(v) < 0.09 for r in recs for v in r["v"])
            assert all(abs(float(r["sigma"]) - 0.3) < 1e-15 and abs(float(r["rho"]) - 0.3) < 1e-15 for r in recs)
            assert not rows.any() and rows.dtype == np.float64
    assert {(False, False), (False, True), (True, True)} <= seen


def _moved(got, want):
    return pr.rel_error(got, want)


def test_mutants_of_the_polynomial_are_told_apart(poly_rows):
    for c, x, w, k, rows in poly_rows:
        f = (lambda **m: pr.poly_param_rows(x, k, w, c["method"], **m)) if c["func"] == "polynomial" else \
            (lambda **m: pr.rank3_param_rows(x, k, w, c["alpha"], c["beta"], c["method"], **m))
        want = rows.sum(axis=0)
        assert _moved(f(half=1.0).sum(axis=0), want) >= 1e-3, c["name"]
        assert _moved(f(direct_term=False).sum(axis=0), want) >= 1e-3, c["name"]
        if c["xshape"][1] > 1 and c["kshape"][1] == 1:                          # (one channel, or one image per plane: nothing to sum)
            assert _moved(f(one_plane=True).sum(axis=0), want) >= 1e-3, c["name"]
        else:
            assert _moved(f(one_plane=True).sum(axis=0), want) == 0.0, c["name"]


def test_mutants_of_the_estimation_are_told_apart(est_rows):
    for c, recs, w, rows in est_rows:
        want = rows.sum(axis=0)
        ungated = pr.estimation_param_rows(recs, w, gate=False).sum(axis=0)
        clamped = any(any(f) for f in c["clamped"])
        if clamped:                                                             # (the gate moves only clamped cases)
            assert np.abs(ungated - want).max() >= 1e-3 * max(np.abs(want).max(), np.abs(ungated).max()), c["name"]
        else:
            assert np.array_equal(ungated, want), c["name"]
        if np.abs(want).max() > 0:
            # eps = 1e-8 beside m^2 of 1e-3 .. 1e-1: d c moves by eps / m^2; it must stay in the formula, and the restatement with it
            # left out is told from the truth at the float64 goldens' level, not at 1e-3 (measured: 1e-7 to 3e-7 of the gradient)
            no_eps = pr.estimation_param_rows(recs, w, eps=0.0).sum(axis=0)
            assert no_eps[0] != want[0] and no_eps[1] == want[1], c["name"]
            print("%s eps left out of d c: off by %.3g" % (c["name"], abs(no_eps[0] - want[0]) / np.abs(want).max()))


def test_last_iteration_alone_is_told_apart(cases, blind_rows):
    z, _ = cases
    for c, steps, w, g in blind_rows:
        last = pr.blind_param_grads(z[c["name"] + "_x"], w, c["n_iter"], c["alpha"], c["beta"], c["method"], steps=steps, last_only=True)
        if c["n_iter"] == 1:
            assert np.array_equal(last, g), c["name"]
        else:
            assert _moved(last, g) >= 1e-3, (c["name"], last, g)


# ---------------------------------------------------------------------------------------------
# the C surface
# ---------------------------------------------------------------------------------------------
def _types(proto):
    args = [a.strip() for a in proto.replace("\n", " ").split(",")]
    return [a.rsplit(" ", 1)[0].replace(" *", "*").strip() + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in args]


def test_header_prototypes_scratch_names_and_bindings():
    import polyblur_amd as pa
    from polyblur_amd import _capi as capi
    from polyblur_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "polyblur_hip.h")).read()
    assert "#define PB_VERSION 200" in header and header.count("#define PB_PROF_NTAGS 10") == 1
    m = re.search(r"int pb_compute_polynomial_taps_params_backward\(([^)]*)\);", header)
    assert m and "pb_compute_polynomial_taps_params_backward" in capi.SYMBOLS
    assert _types(m.group(1)) == ["pb_ctx*", "const float*", "const float*", "float*", "int", "int", "int", "int", "const pb_taps*", "float", "float", "int"]
    comment = header[:m.start()].rsplit("/*", 1)[1]
    for word in ('"ppg.u1"', '"ppg.u2"', '"ppg.partial"', "no float atomics", "ODD", "before any"):
        assert word in comment, word
    m = re.search(r"int pb_estimate_blur_params_backward\(([^)]*)\);", header)
    assert m and "pb_estimate_blur_params_backward" in capi.SYMBOLS
    assert _types(m.group(1)) == ["pb_ctx*", "const float*", "int", "int", "int", "int", "const pb_options*", "const pb_blur_info*", "const float*",
                                  "const float*", "int", "float*", "float*"]
    # the old prototypes stand as they were
    assert re.search(r"int pb_estimate_blur_backward\([^)]*int ker_size, float \*grad_in\);", header)
    assert re.search(r"int pb_compute_polynomial_taps_backward\(pb_ctx \*ctx, const float \*x, const float \*grad_out, float \*grad_x, float \*grad_taps,", header)
    build = __import__("polyblur_amd.build", fromlist=["SOURCES"])
    assert "poly_param_grad.hip" in build.SOURCES
    csrc = os.path.join(ROOT, "polyblur_amd", "csrc")
    source = open(os.path.join(csrc, "poly_param_grad.hip")).read()
    api = open(os.path.join(csrc, "api.hip")).read()
    body = api[api.index("int pb_compute_polynomial_taps_params_backward("):api.index("int pb_edgetaper_taps_backward(")]
    assert set(re.findall(r'pb_scratch\(ctx, "([^"]+)"', source + body)) == {"ppg.u1", "ppg.u2", "ppg.partial"}
    assert "atomic" not in source.replace("no float atomics", "")
    assert body.count("taps_pass(") == 1 and "p.scale = -1.f; p.coef = 1.f;" in body                # three Horner steps of the forward's pass, in a loop
    math = open(os.path.join(csrc, "stage_math.h")).read()
    assert "pb_variance_dc" in math and "pb_variance_db" in math
    est = open(os.path.join(csrc, "estimate_grad.hip")).read()
    assert "pb_variance_dc(" in est and "pb_variance_db(" in est and "2.0 * c /" not in est        # the formulas are stated once
    assert list(inspect.signature(Engine.compute_polynomial_taps_params_backward_ptr).parameters) == \
        ["self", "x_ptr", "grad_out_ptr", "grad_params_ptr", "shape", "ks", "alpha", "beta", "boundary"]
    assert list(inspect.signature(Engine.estimate_blur_params_backward_ptr).parameters) == \
        ["self", "in_ptr", "shape", "opts", "info_ptr", "grad_kernel_ptr", "grad_sigma_rho_ptr", "ker_size", "grad_in_ptr", "grad_cb_ptr"]
    if os.path.exists(capi.library_path()):
        lib = capi.load_library()
        fn = lib.pb_compute_polynomial_taps_params_backward
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 4 + [ctypes.c_void_p] + [ctypes.c_float] * 2 + [ctypes.c_int]
        assert fn(None, None, None, None, 1, 1, 8, 8, None, 2.0, 3.0, capi.PB_WRAP) == -1          # a NULL context: PB_ERR_BADARG, no device touched
        fn = lib.pb_estimate_blur_params_backward
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == 13
        assert fn(None, None, 1, 1, 8, 8, None, None, None, None, 25, None, None) == -1
    from polyblur_amd._autograd import EstimationParamsFunction, TapsParamsFunction
    assert issubclass(TapsParamsFunction, torch.autograd.Function) and issubclass(EstimationParamsFunction, torch.autograd.Function)
    assert callable(pa.compute_polynomial)


# ---------------------------------------------------------------------------------------------
# the Python refusals, on CPU tensors: all before any device work
# ---------------------------------------------------------------------------------------------
@pytest.fixture
def no_library():
    with no_device(AssertionError("device work before the refusal")):
        yield


def _p(v=2.0, grad=True, dtype=torch.float32, shape=()):
    return torch.full(shape, v, dtype=dtype, requires_grad=grad)


def test_a_parameter_that_requires_grad_beside_a_cpu_image(no_library):
    import polyblur_amd as pa
    x, k = torch.rand(1, 3, 16, 18), torch.rand(1, 1, 3, 5)
    calls = [
        ("compute_polynomial", "alpha", lambda: pa.compute_polynomial(x, k, _p(), 3)),
        ("compute_polynomial", "b", lambda: pa.compute_polynomial(x, k, 2, _p(3.0, dtype=torch.float64, shape=(1,)))),
        ("compute_polynomial", "alpha", lambda: pa.compute_polynomial(x.numpy(), k, _p(), 3)),
        ("inverse_filtering_rank3", "alpha", lambda: pa.inverse_filtering_rank3(x, k, alpha=_p())),
        ("inverse_filtering_rank3", "b", lambda: pa.inverse_filtering_rank3(x.half(), k, b=_p())),
        ("gaussian_blur_estimation", "c", lambda: pa.gaussian_blur_estimation(x, q=0.0, c=_p(0.362))),
        ("gaussian_blur_estimation", "b", lambda: pa.gaussian_blur_estimation(x, q=0.0, b=_p(0.464))),
        ("polyblur_deblurring", "c", lambda: pa.polyblur_deblurring(x, c=_p(0.352))),
        ("polyblur_deblurring", "b", lambda: pa.polyblur_deblurring(x, b=_p(0.768))),
        ("polyblur_deblurring", "alpha", lambda: pa.polyblur_deblurring(x, alpha=_p(6.0))),
        ("polyblur_deblurring", "beta", lambda: pa.polyblur_deblurring(x.numpy()[0, 0], beta=_p(1.0))),
        ("polyblur_deblurring", "beta", lambda: pa.PolyblurDeblurring()(x, beta=_p(1.0))),
    ]
    for what, name, call in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == "%s has no backward pass: %s requires grad and the image is not a float32 ROCm tensor -- parameter " \
                               "gradients are built for float32 ROCm images only" % (what, name), str(e.value)


def test_a_parameter_of_more_than_one_element(no_library):
    import polyblur_amd as pa
    x, k = torch.rand(1, 3, 16, 18), torch.rand(1, 1, 3, 5)
    two = torch.tensor([2.0, 3.0])
    for grad in (False, True):
        t = two.clone().requires_grad_(grad)
        for call in (lambda: pa.compute_polynomial(x, k, t, 3), lambda: pa.compute_polynomial(x, k, 2, t),
                     lambda: pa.inverse_filtering_rank3(x, k, alpha=t), lambda: pa.inverse_filtering_nonsymmetric(x, k, b=t),
                     lambda: pa.gaussian_blur_estimation(x, c=t), lambda: pa.gaussian_blur_estimation(x, b=t),
                     lambda: pa.polyblur_deblurring(x, c=t), lambda: pa.polyblur_deblurring(x, beta=t),
                     lambda: pa.PolyblurDeblurring()(x, alpha=t)):
            with pytest.raises(ValueError, match="must be a number or a one-element tensor"):
                call()
        with torch.no_grad():
            with pytest.raises(ValueError, match="alpha must be a number or a one-element tensor"):
                pa.compute_polynomial(x, k, t, 3)
    with pytest.raises(ValueError, match="one-element tensor"):
        pa.compute_polynomial(x, k, torch.ones(1, 1), 3)                       # (0-dim or (1,): no other shape)
    with pytest.raises(TypeError, match="float32 or float64"):
        pa.compute_polynomial(x, k, torch.tensor(2), 3)


def test_a_parameter_that_requires_grad_on_the_pure_phase_path(no_library):
    import polyblur_amd as pa
    x, k = torch.rand(1, 3, 16, 18), torch.rand(1, 1, 3, 5)
    reason = "the gradients with respect to alpha and b are not built for the pure-phase filter"
    for what, call in (("compute_polynomial(not_symmetric=True)", lambda: pa.compute_polynomial(x, k, _p(), 3, not_symmetric=True)),
                       ("compute_polynomial(not_symmetric=True)", lambda: pa.compute_polynomial(x, k, 2, _p(3.0), not_symmetric=True)),
                       ("inverse_filtering_nonsymmetric", lambda: pa.inverse_filtering_nonsymmetric(x, k, alpha=_p())),
                       ("inverse_filtering_nonsymmetric", lambda: pa.inverse_filtering_nonsymmetric(x, k, b=_p(4.0)))):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == "%s has no backward pass: %s" % (what, reason)


def test_a_parameter_that_asks_for_nothing_takes_the_existing_path(no_library):
    """a tensor that does not require grad, or any tensor under torch.no_grad(): no refusal -- the call goes on to the device"""
    import polyblur_amd as pa
    x, k = torch.rand(1, 3, 16, 18), torch.rand(1, 1, 3, 5)
    for call in (lambda: pa.compute_polynomial(x, k, _p(grad=False), 3), lambda: pa.inverse_filtering_rank3(x, k, b=_p(4.0, grad=False)),
                 lambda: pa.gaussian_blur_estimation(x, c=_p(0.362, grad=False)), lambda: pa.polyblur_deblurring(x, beta=_p(1.0, grad=False))):
        with pytest.raises(AssertionError, match="device work before the refusal"):
            call()
    with torch.no_grad():
        for call in (lambda: pa.compute_polynomial(x, k, _p(), 3), lambda: pa.gaussian_blur_estimation(x, c=_p(0.362)),
                     lambda: pa.polyblur_deblurring(x, alpha=_p(6.0)), lambda: pa.inverse_filtering_nonsymmetric(x, k, alpha=_p())):
            with pytest.raises(AssertionError, match="device work before the refusal"):
                call()
    with pytest.raises(NotImplementedError, match="overlap-add"):
        pa.PolyblurDeblurring(patch_decomposition=True, patch_size=8)(x, alpha=_p(6.0))
