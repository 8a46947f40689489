"""The differentiable edgetaper without a GPU: the float64 restatement (tests/edgetaper_grad_ref.py) against the
reference's own autograd (tests/golden/edgetaper_grad.npz), its discriminating power (six mutants), the tolerances against the
reference's own float32 error, the C ABI's declaration, and every refusal under grad -- raised before any device work."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import edgetaper_grad_ref as eg
import estimation_grad_ref as er

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [c[0] for c in eg.TAPER_CASES + eg.EXTRA_CASES]


@functools.lru_cache(maxsize=None)
def hand(name, mutant=None):
    c = eg.taper_case(name)
    return eg.backward(c["x"], c["k"], c["w"], c["method"], c["n"], mutant=mutant)


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", eg.GOLDEN_TAPER)
def test_restatement_meets_the_float64_goldens(name):
    d, _, _ = eg.read_golden()
    gx, gk = hand(name)
    ex, ek = eg.rel_error(gx, d[name + "_dx"]), eg.rel_error(gk, d[name + "_dk"])
    print("%-18s image %.3g | kernel %.3g (bound 1e-10)" % (name, ex, ek))
    assert ex <= 1e-10 and ek <= 1e-10


@pytest.mark.parametrize("name", ALL)
def test_hand_backward_meets_torch_autograd(name):
    """on the golden cases and on those the reference cannot serve: one kernel per image, one per plane, no blend"""
    c = eg.taper_case(name)
    y, ax, ak = eg.autograd_gradients(c["x"], c["k"], c["w"], c["method"], c["n"])
    gx, gk = hand(name)
    assert np.abs(y - eg.forward(c["x"], c["k"], c["method"], c["n"])).max() <= 1e-12
    if c["n"] == 0:
        assert np.array_equal(gx, c["w"].astype(np.float64)) and not gk.any() and not ak.any()
        return
    assert eg.rel_error(gx, ax) <= 1e-10 and eg.rel_error(gk, ak) <= 1e-10


@pytest.mark.parametrize("name", [c[0] for c in eg.CHAIN_CASES])
def test_chain_cases_keep_their_margins_and_meet_the_goldens(name):
    d, table, _ = eg.read_golden()
    c = eg.chain_case(name)
    assert eg.chain_ok(c) and table[name]["seed"] == eg.CHAIN_SEEDS[name]
    _, gx, gk = eg.chain_gradients(c)
    assert eg.rel_error(gx, d[name + "_dx"]) <= 1e-10 and eg.rel_error(gk, d[name + "_dk"]) <= 1e-10


def test_blind_restatement_meets_the_float32_goldens():
    d, _, blind = eg.read_golden()
    assert len(blind) == len(eg.BLIND_CASES)
    for c in blind:
        x, w, gx = d[c["name"] + "_x"], d[c["name"] + "_w"], d[c["name"] + "_gx"]
        assert x.shape[0] == 1                                # (the reference's maximum runs over the batch)
        off = eg.rel_error(eg.blind_gradient(x, w, c["n_iter"], c["alpha"], c["beta"], c["method"]), gx)
        print("%s: restatement against the reference's float32 %.3g (bound %.3g)" % (c["name"], off, er.BOUND_GOLDEN))
        assert off <= er.BOUND_GOLDEN


@pytest.mark.parametrize("mutant", eg.MUTANTS)
def test_every_mutant_is_told_from_the_truth(mutant):
    """each deliberate error moves the image or the tap gradient of some golden case by at least 1e-3 of its largest entry"""
    moved = {}
    for name in eg.GOLDEN_TAPER:
        c = eg.taper_case(name)
        if mutant == "x0_for_xi" and c["n"] < 2:
            continue
        gx, gk = hand(name)
        mx, mk = hand(name, mutant)
        moved[name] = max(eg.rel_error(mx, gx), eg.rel_error(mk, gk))
    print(mutant, {n: "%.3g" % v for n, v in moved.items()})
    assert max(moved.values()) >= eg.MUTANT_BOUND


def test_tolerances_are_six_times_the_references_own_error():
    _, table, _ = eg.read_golden()
    for kind, tx, tk in (("taper", eg.TOL_ET_X, eg.TOL_ET_K), ("chain", eg.TOL_CHAIN_X, eg.TOL_CHAIN_K)):
        rows = [t for t in table.values() if t["kind"] == kind]
        ex, ek = max(t["E_x"] for t in rows), max(t["E_k"] for t in rows)
        print("%s: E image %.3g, taps %.3g; tolerances %.3g, %.3g" % (kind, ex, ek, tx, tk))
        assert 4 * ex <= tx <= 8 * ex and 4 * ek <= tk <= 8 * ek
        assert all(t["restatement"] <= 1e-10 for t in rows)
    assert all(c[2][0] == 1 for c in eg.TAPER_CASES + eg.CHAIN_CASES)         # kernel batch 1: the reference's maximum is global


# ---------------------------------------------------------------------------------------------
# the declaration
# ---------------------------------------------------------------------------------------------
def test_header_prototype_comment_and_ctypes_signature():
    from polyblur_amd import _capi as capi
    from polyblur_amd.build import SOURCES
    from polyblur_amd.engine import Engine
    header = open(os.path.join(REPO, "include", "polyblur_hip.h")).read()
    flat = re.sub(r"\s+", " ", header)
    assert ("int pb_edgetaper_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps, "
            "int B, int C, int H, int W, const pb_taps *taps, int boundary, int n_tapers);") in flat
    comment = flat[flat.index("Backward of pb_edgetaper_taps"):flat.index("int pb_edgetaper_taps_backward")]
    for word in ("edgetaper.py:10-33", "etg.u", "etg.ag", "etg.g", "etg.kx", "etg.x", "etg.abar", "etg.vbar", "n_tapers + 3", "no float atomics",
                 "x may be NULL when grad_taps is", "PB_ERR_UNSUPPORTED", "n_tapers == 0"):
        assert word in comment, word
    assert header.count("#define PB_PROF_NTAGS 10") == 1 and "#define PB_VERSION 200" in header
    assert "pb_edgetaper_taps_backward" in capi.SYMBOLS and "edgetaper_grad.hip" in SOURCES
    assert callable(Engine.edgetaper_taps_backward_ptr)
    src = open(os.path.join(REPO, "polyblur_amd", "_capi.py")).read()
    assert '"pb_edgetaper_taps_backward": (ci, [vp, vp, vp, vp, vp, ci, ci, ci, ci, vp, ci, ci])' in src
    kernels = open(os.path.join(REPO, "polyblur_amd", "csrc", "edgetaper_grad.hip")).read()
    assert "atomic" not in kernels.replace("no atomics", "") and "__frcp_rn" in kernels


# ---------------------------------------------------------------------------------------------
# refusals, before any device work
# ---------------------------------------------------------------------------------------------
def _refusals():
    import polyblur_amd as pa
    from polyblur_amd import _frontend as fe
    x, k = torch.rand(1, 3, 16, 18), torch.rand(1, 1, 3, 5)
    xg, kg = x.clone().requires_grad_(True), k.clone().requires_grad_(True)
    taper = "inverse_filtering_rank3(do_edgetaper=True) has no backward pass: " + fe.NO_EDGETAPER
    blind = "polyblur_deblurring(edgetaping=True) has no backward pass: " + fe.NO_EDGETAPER
    return [
        (taper, lambda: pa.inverse_filtering_rank3(xg, k, 6, 1, do_edgetaper=True, method="fft")),
        (taper, lambda: pa.inverse_filtering_rank3(x, kg, 6, 1, do_edgetaper=True, method="direct")),
        (taper, lambda: pa.inverse_filtering_rank3(x.numpy(), kg, 6, 1, do_edgetaper=True)),
        (taper, lambda: pa.inverse_filtering_rank3(x.half(), kg, 6, 1, do_edgetaper=True)),
        (blind, lambda: pa.polyblur_deblurring(xg, edgetaping=True)),
        (blind, lambda: pa.polyblur_deblurring(xg.detach().half().requires_grad_(True), edgetaping=True)),
        (blind, lambda: pa.PolyblurDeblurring()(xg, edgetaping=True)),
        ("edgetaper has no backward", lambda: pa.edgetaper(xg, k)),
        ("edgetaper has no backward", lambda: pa.edgetaper(x, kg)),
        ("edgetaper has no backward", lambda: pa.edgetaper(x.numpy(), kg, method="direct")),
        ("inverse_filtering_nonsymmetric", lambda: pa.inverse_filtering_nonsymmetric(xg, k, 6, 1, do_edgetaper=True)),
        ("odd sides only", lambda: pa.inverse_filtering_rank3(xg, torch.rand(1, 1, 4, 4), 6, 1)),
        ("halo masking", lambda: pa.inverse_filtering_rank3(xg, k, 6, 1, remove_halo=True, do_edgetaper=True)),
        ("polyblur_deblurring(q=0.1)", lambda: pa.polyblur_deblurring(xg, q=0.1)),
        ("patch_decomposition", lambda: pa.PolyblurDeblurring(patch_decomposition=True)(xg, edgetaping=True)),
    ]


def test_every_refusal_comes_before_any_device_work():
    for pattern, call in _refusals():
        with pytest.raises(NotImplementedError) as e:
            call()
        assert pattern in str(e.value), (pattern, str(e.value))
        assert "\n" not in str(e.value)


def test_without_grad_the_new_checks_are_passed():
    """the same calls under torch.no_grad() get past every check (and then run, or fail on a missing GPU, as before)"""
    import polyblur_amd as pa
    xg, kg = torch.rand(1, 3, 16, 18, requires_grad=True), torch.rand(1, 1, 3, 5, requires_grad=True)
    calls = [lambda: pa.edgetaper(xg, kg), lambda: pa.inverse_filtering_rank3(xg, kg, 6, 1, do_edgetaper=True, method="fft"),
             lambda: pa.polyblur_deblurring(xg, edgetaping=True)]
    with torch.no_grad():
        for call in calls:
            try:
                y = call()
            except NotImplementedError:
                raise
            except Exception:                                 # (no GPU here)
                continue
            assert not y.requires_grad


def test_the_autograd_function_is_once_differentiable_and_asks_only_for_what_is_needed():
    src = open(os.path.join(REPO, "polyblur_amd", "_autograd.py")).read()
    body = src[src.index("class EdgetaperFunction"):src.index("class PhaseFunction")]
    assert "@once_differentiable" in body and "needs_input_grad" in body and "_kernel_grad" in body and "ctx.save_for_backward(x)" in body
