"""Halo masking without a GPU: the oracle and the float64 restatement (tests/halo_ref.py) against the reference's own outputs
on inputs where the mask has a strong effect (tests/golden/halo_strong.npz), and the proof that tests/test_gpu_halo.py has teeth
-- for every input set it uses, the gauge (halo_ref.power) holds, the tolerance is four times the fp32 oracle's own error, and
the comparison it makes rejects every applicable mutant of halo_ref.MUTANTS by at least ten times that tolerance."""
import numpy as np
import pytest

from oracle import polyblur_ref as ref
import halo_ref as hr

STAGE_IDS = [hr.shape_id(s) for s in hr.STAGE_SHAPES]
FP32_NAMES = [c[0] for c in hr.INVERSE_CASES]
HALF_NAMES = [c[0] for c in hr.HALF_CASES]


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def set_and_tol(kind, key):
    if kind == "stage":
        return hr.stage_set(key), hr.TOL_STAGE
    return hr.inverse_set(key), (hr.TOL_INV_HALF if key in HALF_NAMES else hr.TOL_INV)


ALL_SETS = [("stage", s) for s in hr.STAGE_SHAPES] + [("inverse", n) for n in FP32_NAMES + HALF_NAMES]
ALL_IDS = STAGE_IDS + FP32_NAMES + HALF_NAMES


# ---------------------------------------------------------------------------------------------
# the reference's own outputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", hr.GOLDEN_SHAPES, ids=hr.shape_id)
def test_halo_masking_against_reference(golden, shape):
    """the bug-compatible formula (gy * gy) where it shows: the gy * oy mutant is ~3e-2 away on these inputs"""
    g, tag = golden("halo_strong.npz"), "w%d" % shape[-1]
    x, y, gx, gy, want = (g["%s_%s" % (tag, k)] for k in ("x", "y", "gx", "gy", "halo"))
    s = hr.stage_set(shape)
    assert all(np.array_equal(a, b) for a, b in ((x, s["x"]), (y, s["y32"]), (gx, s["gx"]), (gy, s["gy"])))   # the builder's, still
    assert hr.power(want, y, hr.TOL_STAGE, s["z"], s["pole"]) is None
    assert maxabs(ref.halo_masking(x, y, (gx, gy)), want) < hr.TOL_STAGE
    assert maxabs(hr.halo_f64(x, y, gx, gy, False), want) < hr.TOL_STAGE
    assert maxabs(hr.MUTANTS["gy * oy"](s), want) > 1e-2


@pytest.mark.parametrize("method,taper", hr.GOLDEN_VARIANTS)
@pytest.mark.parametrize("shape", hr.GOLDEN_SHAPES, ids=hr.shape_id)
def test_inverse_filter_with_grad_img_against_reference(golden, shape, method, taper):
    g, tag = golden("halo_strong.npz"), "w%d" % shape[-1]
    x, k, gx, gy = (g["%s_%s" % (tag, n)] for n in ("image", "k", "igx", "igy"))
    assert all(np.array_equal(a, b) for a, b in zip((x, k, gx, gy), hr.golden_inverse_inputs(shape)))
    want = g["%s_inv_%s_%s" % (tag, method, "taper" if taper else "plain")]
    _, xc, y, _ = hr.chain_f64(x, k, taper, method)
    w64, z, pole = hr.halo_f64(xc, y, gx, gy, True, parts=True)
    assert hr.power(w64, np.clip(y, 0, 1), hr.TOL_INV, z, pole) is None
    got = ref.inverse_filtering_rank3(x, k, hr.ALPHA, hr.BETA, remove_halo=True, grad_img=(gx, gy), do_edgetaper=taper, method=method)
    assert maxabs(got, want) < hr.TOL_INV
    assert maxabs(w64, want) < hr.TOL_INV


# ---------------------------------------------------------------------------------------------
# every input set of tests/test_gpu_halo.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,key", ALL_SETS, ids=ALL_IDS)
def test_gauge_holds(kind, key):
    s, tol = set_and_tol(kind, key)
    assert hr.power(s["want"], s["unmasked"], tol, s["z"], s["pole"]) is None
    if kind == "inverse":                                     # the clamp acts, and hides little
        at = float(np.mean((s["want"] == 0) | (s["want"] == 1)))
        assert 0 < at < 0.12, at


@pytest.mark.parametrize("kind,key", ALL_SETS, ids=ALL_IDS)
def test_mutants_are_rejected(kind, key):
    s, tol = set_and_tol(kind, key)
    applied = []
    for name, mutant in hr.MUTANTS.items():
        out = mutant(s)
        if out is None:
            continue
        applied.append(name)
        assert maxabs(out, s["want"]) >= 10 * tol, (name, maxabs(out, s["want"]))
    must = {"copy of y", "gy * oy", "no max(., 0)", "M / nM"}
    if kind == "inverse":
        must |= {"no final clamp"} | ({"x with pitch W"} if s["taper"] else set())
    if np.prod(s["want"].shape[:2]) > 1:
        must.add("nM of the neighbouring plane")
    if s["want"].shape[1] > 1:
        must.add("nM of the whole image")
    assert must <= set(applied), must - set(applied)


def test_recombination_mutant_is_rejected():
    """the fused recombination (the blind pipeline with a prefilter): float64 arithmetic against its mutant"""
    s = hr.recombined_set()
    assert hr.power(s["want"], s["unmasked"], hr.TOL_PIPE, s["z"], s["pole"], factor=20) is None
    for name in ("recombination without the inner clip", "copy of y", "no max(., 0)", "M / nM", "gy * oy"):
        assert maxabs(hr.MUTANTS[name](s), s["want"]) >= 10 * hr.TOL_PIPE, name
    assert hr.MUTANTS["no final clamp"](s) is None
    # behind the final clamp, which the pipeline always asks for, the inner clip is the identity: nothing to tell apart there
    t = dict(s, clamp=True)
    assert maxabs(hr.MUTANTS["recombination without the inner clip"](t), hr.halo_f64(t["xc"], t["y"], t["gx"], t["gy"], True, t["cur"], t["smooth"])) == 0


@pytest.mark.parametrize("prefiltering", [False, True])
def test_pipeline_input_meets_the_gauge(prefiltering):
    """the blind call's input (the image's own gradients): the gauge at 20 tolerances, the oracle within a tolerance of the
    float64 mask on its own kernel estimate, and the mutants the input can show (behind the final clamp the recombination's
    inner clip is the identity)"""
    s = hr.pipeline_set(prefiltering)
    assert hr.power(s["want"], s["unmasked"], hr.TOL_PIPE, s["z"], s["pole"], factor=20) is None
    assert maxabs(s["oracle"], s["want"]) < hr.TOL_PIPE
    for name in ("copy of y", "gy * oy", "no max(., 0)", "M / nM", "nM of the neighbouring plane", "nM of the whole image"):
        assert maxabs(hr.MUTANTS[name](s), s["want"]) >= 10 * hr.TOL_PIPE, (name, maxabs(hr.MUTANTS[name](s), s["want"]))


@pytest.mark.parametrize("name", [c[0] for c in hr.OWN_CASES])
def test_own_gradients_do_not_reach_the_gauge(name):
    """grad0 = None at (1,1,8,9) and (1,3,12,16): with the image's own gradients the gauge is not met from the reference, so
    tests/test_gpu_halo.py has no such case; this records why (printed)"""
    s = hr.inverse_set(name)
    why = hr.power(s["want"], s["unmasked"], hr.TOL_INV, s["z"], s["pole"])
    print(name, why, "largest effect %.3g" % maxabs(s["want"], s["unmasked"]))
    assert why is not None


# ---------------------------------------------------------------------------------------------
# the tolerances: four times the fp32 oracle's error against float64, measured here again
# ---------------------------------------------------------------------------------------------
def test_stage_tolerance_is_four_oracle_errors():
    worst = 0.0
    for shape in hr.STAGE_SHAPES:
        s = hr.stage_set(shape)
        worst = max(worst, maxabs(ref.halo_masking(s["x"], s["y32"], (s["gx"], s["gy"])), s["want"]))
    print("oracle vs float64, stage: %.3g" % worst)
    assert hr.TOL_STAGE / 8 < worst <= hr.TOL_STAGE / 4


def test_inverse_tolerances_are_four_oracle_errors():
    worst = max(maxabs(hr.oracle_inverse(hr.inverse_set(n)), hr.inverse_set(n)["want"]) for n in FP32_NAMES)
    print("oracle vs float64, fp32 chains: %.3g" % worst)
    assert hr.TOL_INV / 8 < worst <= hr.TOL_INV / 4
    worst = max(maxabs(hr.oracle_inverse(hr.inverse_set(n)).astype(np.float16), hr.inverse_set(n)["want"]) for n in HALF_NAMES)
    print("oracle vs float64, fp16 images: %.3g" % worst)
    assert hr.TOL_INV_HALF / 8 < worst <= hr.TOL_INV_HALF / 4
