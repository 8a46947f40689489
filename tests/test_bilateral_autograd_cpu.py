"""The differentiable bilateral prefilter without a GPU: the float64 restatement of the gradient
(tests/bilateral_grad_ref.py) against torch's autograd of the reference's formula and against the reference's goldens
(tests/golden/prefilter_grad.npz), and the proof that tests/test_gpu_bilateral_autograd.py has teeth -- its tolerance is four
times the float32 CPU evaluation's own error over its cases, and at that tolerance its comparison rejects every mutant of the
backward.  Then the symbols, the public names and the refusals that remain."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import bilateral_grad_ref as bg
from frontend_cases import no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REJECT = 10                                                   # a mutant is off by at least this many GPU tolerances
GAUGE = [c for c in bg.CASES if c[0] == bg.TILE and c[1] >= 3]
BLIND = ["p%02d" % n for n in range(len(bg.GOLDEN_BLIND))]


@functools.lru_cache(maxsize=None)
def goldens():
    return np.load(os.path.join(ROOT, "tests", "golden", "prefilter_grad.npz"))


@functools.lru_cache(maxsize=None)
def blind_reference(name):
    d = goldens()
    c = [c for c in json.loads(str(d["cases"])) if c["name"] == name][0]
    x, w = d[name + "_x"], d[name + "_w"]
    _, steps = bg.blind(x, c["n_iter"], c["remove_halo"])
    return c, x, w, d[name + "_dx"], steps, bg.blind_tolerances(x, w, c["n_iter"], c["remove_halo"], steps=steps)


# ---------------------------------------------------------------------------------------------
# the restatement against autograd and against the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in bg.CASES if c[0] != bg.MANY], ids=bg.case_id)
def test_hand_written_backward_is_autograds(case):
    shape, k, (ss, sc) = case
    v, g = bg.case_inputs(shape, sc)
    assert bg.case_error(bg.autograd_backward(v, g, k, ss, sc), bg.case_reference(case)) < 1e-12


def test_hand_written_backward_is_autograds_on_many_planes():
    """the 65 540 planes: autograd on the first and the last hundred"""
    shape, k, (ss, sc) = case = [c for c in bg.CASES if c[0] == bg.MANY][0]
    v, g = bg.case_inputs(shape, sc)
    want = bg.case_reference(case)
    for sl in (slice(0, 100), slice(-100, None)):
        assert bg.case_error(bg.autograd_backward(v[sl], g[sl], k, ss, sc), want[sl]) < 1e-12


def test_restatement_against_the_references_blind_gradients():
    worst = 0.0
    for name in BLIND:
        c, x, w, gref, steps, ref = blind_reference(name)
        assert bg.blind_margins_ok(steps, np.asarray(x, np.float64), c["remove_halo"])        # the generator's margins, still
        worst = max(worst, float(np.max(np.abs(ref["want"] - gref) / bg.hg.image_max(gref))))
    print("restatement vs the reference's float32 blind gradients with prefiltering: %.3g" % worst)
    assert bg.BOUND_GOLDEN_PREFILTER / 8 < worst <= bg.BOUND_GOLDEN_PREFILTER / 4
    assert {(c[1], c[2]) for c in bg.GOLDEN_BLIND} == {(1, False), (2, False), (1, True), (2, True)}


@pytest.mark.parametrize("name", BLIND)
def test_blind_comparison_rejects_a_filter_taken_for_a_constant(name):
    c, x, w, _, steps, ref = blind_reference(name)
    m = bg.blind_gradient(x, w, c["n_iter"], c["remove_halo"], steps=steps, mutant="smooth detached")
    off = float(np.max(np.abs(m - ref["want"]) / ref["tol"]))
    print(name, "the filter taken for a constant: off by %.3g tolerances; upstream of the filter %s" % (off, ref["upstream"]))
    assert off >= REJECT


# ---------------------------------------------------------------------------------------------
# the tolerance: four times the float32 evaluation's error against float64, measured here again
# ---------------------------------------------------------------------------------------------
def test_tolerance_is_four_float32_errors():
    worst, by_ksize = 0.0, {}
    for case in bg.CASES:
        shape, k, (ss, sc) = case
        v, g = bg.case_inputs(shape, sc)
        e = bg.case_error(bg.backward(v, g, k, ss, sc, dtype=np.float32), bg.case_reference(case))
        by_ksize[k] = max(by_ksize.get(k, 0.0), e)
        worst = max(worst, e)
    print("float32 CPU evaluation vs float64, largest by ksize:", {k: "%.3g" % e for k, e in sorted(by_ksize.items())})
    assert bg.TOL_BILATERAL / 8 < worst <= bg.TOL_BILATERAL / 4, worst


# ---------------------------------------------------------------------------------------------
# the gauge, from float64 alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GAUGE, ids=bg.case_id)
def test_mutants_are_rejected(case):
    shape, k, (ss, sc) = case
    v, g = bg.case_inputs(shape, sc)
    want = bg.case_reference(case)
    assert np.abs(g).min() >= 0.25 and np.abs(g).max() < 1
    for name in bg.MUTANTS:
        frac = bg.missed(bg.backward(v, g, k, ss, sc, mutant=name), want, REJECT * bg.TOL_BILATERAL).mean()
        assert frac >= 0.90, (name, frac)
    m = bg.missed(bg.backward(v, g, k, ss, sc, mutant=bg.BORDER_MUTANT), want, REJECT * bg.TOL_BILATERAL)
    ring = np.ones(shape, bool)
    ring[..., 1:-1, 1:-1] = False
    assert m[ring].mean() >= 0.90, m[ring].mean()
    assert not m[~ring].any()
    assert bg.case_error(bg.backward(v, g, k, ss, sc, mutant=bg.BORDER_MUTANT)[..., 1:-1, 1:-1], want[..., 1:-1, 1:-1]) < 1e-12


def test_cases_cover_what_the_kernels_branch_on():
    shapes = {c[0] for c in bg.CASES}
    assert {bg.TINY, bg.TILE, bg.WIDE, bg.MANY} == shapes
    assert bg.TILE[-1] == 64 + 1 and bg.TILE[-2] == 16 + 1 and bg.MANY[0] * bg.MANY[1] > 65535
    assert {(k, s) for sh, k, s in bg.CASES if sh == bg.TILE} == {(k, s) for k in (1, 3, 5, 7, 13, 25) for s in bg.SIGMAS}
    assert {k for sh, k, _ in bg.CASES if sh == bg.TINY} == {1, 3, 25} and {k for sh, k, _ in bg.CASES if sh == bg.WIDE} == {5, 13}


# ---------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------
def test_symbols_names_and_header():
    import ctypes
    import inspect
    import polyblur_amd as pa
    from polyblur_amd import _capi as capi
    from polyblur_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "polyblur_hip.h")).read()
    m = re.search(r"int pb_bilateral_backward\(([^)]*)\);", header)
    assert m and "pb_bilateral_backward" in capi.SYMBOLS
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.rsplit(" ", 1)[0].replace(" *", "*").strip() + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in args] == \
        ["pb_ctx*", "const float*", "const float*", "float*", "int", "int", "int", "int", "int", "float", "float"]
    assert "#define PB_VERSION 200" in header and '"bilg.out"' in header and '"bilg.G"' in header and '"bilg.T"' in header
    assert "bilateral_grad.hip" in __import__("polyblur_amd.build", fromlist=["SOURCES"]).SOURCES
    assert list(inspect.signature(Engine.bilateral_backward_ptr).parameters) == \
        ["self", "in_ptr", "grad_out_ptr", "grad_in_ptr", "shape", "ksize", "sigma_spatial", "sigma_color"]
    if os.path.exists(capi.library_path()):
        fn = capi.load_library().pb_bilateral_backward
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 5 + [ctypes.c_float] * 2
    for name in ("bilateral_filter", "edge_aware_filtering"):
        assert name in pa.__all__ and callable(getattr(pa, name))
    from polyblur_amd._autograd import BilateralFunction
    assert issubclass(BilateralFunction, torch.autograd.Function)


@pytest.fixture
def no_library():
    """any device work raises: a refusal must come first"""
    with no_device(AssertionError("device work before the refusal")):
        yield


def test_refusals_that_remain(no_library):
    import polyblur_amd as pa
    x = torch.rand(1, 3, 16, 18)
    xg, xh = x.clone().requires_grad_(True), x.half().requires_grad_(True)
    filters = " has no backward pass: the edge-aware filters are not differentiated"
    blind = "polyblur_deblurring(prefiltering=True) has no backward pass: the edge-aware prefilters are not differentiated"
    calls = [
        ("bilateral_filter" + filters, lambda: pa.bilateral_filter(xg)),
        ("bilateral_filter" + filters, lambda: pa.bilateral_filter(xh, 7, 3.0, 0.05)),
        ("edge_aware_filtering" + filters, lambda: pa.edge_aware_filtering(xg, 2.0, 0.8)),
        ("edge_aware_filtering" + filters, lambda: pa.edge_aware_filtering(xh, 2.0, 0.8)),
        ("edge_aware_filtering" + filters, lambda: pa.edge_aware_filtering(xg, 2.0, 0.8, prefilter="domain_transform")),
        ("edge_aware_filtering" + filters, lambda: pa.edge_aware_filtering(xg, 2.0, 0.8, prefilter="normalized_convolution")),
        ("recursive_filter" + filters, lambda: pa.recursive_filter(xg)),
        ("recursive_filter" + filters, lambda: pa.recursive_filter(x, joint_image=xg)),
        ("normalized_convolution" + filters, lambda: pa.normalized_convolution(xg)),
        (blind, lambda: pa.polyblur_deblurring(xg, prefiltering=True)),
        (blind, lambda: pa.polyblur_deblurring(xh, prefiltering=True)),
        (blind, lambda: pa.polyblur_deblurring(xg, prefiltering=True, prefilter="domain_transform")),
        (blind, lambda: pa.polyblur_deblurring(xg, prefiltering=True, prefilter="normalized_convolution")),
        (blind, lambda: pa.polyblur_deblurring(xg, prefiltering=True, prefilter="bogus")),      # (a CPU tensor: today's refusal first)
        (blind, lambda: pa.PolyblurDeblurring()(xg, prefiltering=True)),
        (blind, lambda: pa.PolyblurDeblurring()(xh, prefiltering=True)),
        ("polyblur_deblurring(remove_halo=True) has no backward pass: halo masking is differentiated for float32 ROCm tensors only",
         lambda: pa.polyblur_deblurring(xg, prefiltering=True, remove_halo=True)),
        ("polyblur_deblurring(edgetaping=True) has no backward pass: the edgetaper is not differentiated",
         lambda: pa.polyblur_deblurring(xg, prefiltering=True, edgetaping=True)),
    ]
    for message, call in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == message
    with pytest.raises(ValueError, match="prefilter must be"):
        pa.edge_aware_filtering(xg, 2.0, 0.8, prefilter="bogus")
