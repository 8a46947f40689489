"""Gradients of the polynomial with the pure-phase filter, the part that needs no GPU:

  * tests/phase_grad_ref.py -- the NumPy float64 restatement of the formulas -- against the reference's own float64 autograd
    (tests/golden/nonblind_phase_grad.npz, written by tests/golden/make_golden_phase_autograd.py) within 1e-10 of the largest entry;
    with the mask in the chain the reference's float64 run still takes float32 frequencies for its spectral derivative
    (filters.py:175-178), which the comparison takes too (pg.reference_frequencies) -- with exact ones it is within
    halo_grad_ref.BOUND_GOLDEN_F64, the bound that restatement has held since it was written;
  * each mutant of the restatement is off by at least 1e-3 of the largest entry on a named case;
  * the new C symbol is declared, exported and bound; the new refusals, and the pinned ones unchanged;
  * the conditions the GPU test (tests/test_gpu_phase_autograd.py) relies on, for every one of its cases: the reference's own
    float32 error E stays within pg.E_CAP, pg.TOL is between 4 and 8 times the largest E of its group, and in the chain cases no
    float64 output lies within 1e-4 of the clamp's 0 or 1, at most 1 % sit at them and the mask's kink band is empty."""
import os
import re

import numpy as np
import pytest
import torch

import halo_grad_ref as hg
import phase_grad_ref as pg
from polyblur_amd import _capi as capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOL = "pb_compute_polynomial_phase_taps_backward"
CHAIN_NAMES = [c[0] for c in pg.CHAIN_CASES]


@pytest.fixture(scope="module")
def golden_table():
    return pg.golden()


def chain_gradients(name, **kw):
    c = pg.chain_case(name)
    return pg.chain_backward(c["x"], c["k"], c["w"], c["alpha"], c["b"], c["correlate"], c["remove_halo"], c["grad_img"], **kw)


@pytest.mark.parametrize("name", pg.GOLDEN_POLY)
def test_restatement_matches_the_reference_polynomial(golden_table, name):
    d, _ = golden_table
    gx, gk = pg.poly_want(name)
    ex, ek = pg.rel_error(gx, d[name + "_dx"]), pg.rel_error(gk, d[name + "_dk"])
    print(name, "grad_x %.2g grad_k %.2g" % (ex, ek))
    assert gk.shape == pg.poly_case(name)["k"].shape
    assert ex < 1e-10 and ek < 1e-10, (name, ex, ek)


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_restatement_matches_the_reference_chain(golden_table, name):
    d, _ = golden_table
    pg.chain_case(name)                                     # (its inputs are built with the exact derivative: before the switch)
    with pg.reference_frequencies():
        got = chain_gradients(name)
    exact = pg.chain_want(name)
    assert sorted(got) == sorted(n[len(name) + 2:] for n in d.files if n.startswith(name + "_d"))
    for n in got:
        e, ee = pg.rel_error(got[n], d["%s_d%s" % (name, n)]), pg.rel_error(exact[n], d["%s_d%s" % (name, n)])
        print(name, n, "%.2g (exact frequencies: %.2g)" % (e, ee))
        assert e < 1e-10, (name, n, e)
        assert ee < (hg.BOUND_GOLDEN_F64 if pg.chain_case(name)["remove_halo"] else 1e-10), (name, n, ee)


def test_forward_of_the_restatement_is_phase_ref():
    import phase_ref as pr
    c = pg.poly_case("one_kernel_per_plane")
    assert np.abs(pg.forward(c["x"], c["k"], 2, 3) - pr.compute_polynomial_fft(c["x"], c["k"], 2, 3, True, double=True)).max() < 1e-12


def test_pad_adjoint():
    rng = np.random.default_rng(3)
    x, g = rng.random((1, 2, 5, 6)), rng.random((1, 2, 11, 12))
    assert abs(np.vdot(pg.pad(x, 3), g) - np.vdot(x, pg.pad_adjoint(g, 3))) < 1e-12


# the case each mutant is measured on, and which gradient it moves
MUTANT_CASES = {
    "C constant": ("single_stage_16x24", "k"),
    "conj term dropped": ("single_stage_16x24", "k"),
    "M for conj(M)": ("single_stage_16x24", "x"),
    "roll by (kh - 1) // 2": ("k8x8", "k"),
    "one plane": ("single_stage_16x24", "k"),
    "no 1 / N": ("single_stage_16x24", "k"),
    "flip forgotten": ("chain_correlate_7x9", "k"),
}


@pytest.mark.parametrize("mutant", pg.MUTANTS)
def test_mutants_are_off(mutant):
    name, which = MUTANT_CASES[mutant]
    if name in CHAIN_NAMES:
        want, got = pg.chain_want(name)[which], chain_gradients(name, mutant=mutant)[which]
    else:
        c = pg.poly_case(name)
        want = dict(zip("xk", pg.poly_want(name)))[which]
        got = dict(zip("xk", pg.backward(c["x"], c["k"], c["w"], c["alpha"], c["b"], mutant=mutant)))[which]
    e = pg.rel_error(got, want)
    print("%-24s on %-22s grad_%s off by %.3g of the largest entry" % (mutant, name, which, e))
    assert e >= 1e-3, (mutant, e)
    assert set(MUTANT_CASES) == set(pg.MUTANTS)


# ---------------------------------------------------------------------------------------------
# the conditions of the GPU test's cases
# ---------------------------------------------------------------------------------------------
def test_reference_error_of_every_case_is_within_the_caps(golden_table):
    d, table = golden_table
    assert sorted(table) == sorted(pg.POLY_NAMES + [pg.LONG] + CHAIN_NAMES)
    for name, row in table.items():
        assert row["E_k"] <= pg.E_CAP["k"] and row["E_x"] <= pg.E_CAP["x"], (name, row)
        assert row["restatement"] < 1e-10, (name, row)
    # the stored float32 gradients are what the table's figures were taken from
    for name in pg.GOLDEN_POLY + CHAIN_NAMES:
        for n in ("x", "k"):
            assert pg.rel_error(d["%s_f%s" % (name, n)], d["%s_d%s" % (name, n)]) == pytest.approx(table[name]["E_" + n], rel=1e-6)


def test_tolerances_are_four_to_eight_times_the_reference_error(golden_table):
    _, table = golden_table
    groups = {"poly_x": [r["E_x"] for r in table.values() if r["kind"] == "poly"], "poly_k": [r["E_k"] for r in table.values() if r["kind"] == "poly"],
              "chain_x": [r["E_x"] for r in table.values() if r["kind"] == "chain"], "chain_k": [r["E_k"] for r in table.values() if r["kind"] == "chain"],
              "chain_g": [r[n] for r in table.values() for n in ("E_gx", "E_gy") if n in r]}
    assert sorted(groups) == sorted(pg.TOL) == sorted(pg.E_MAX)
    for g, es in groups.items():
        E = max(es)
        print("%-8s E %.3g (recorded %.3g) TOL %.3g = %.2f E" % (g, E, pg.E_MAX[g], pg.TOL[g], pg.TOL[g] / E))
        assert pg.E_MAX[g] == pytest.approx(E, rel=5e-3), g
        assert 4 * E <= pg.TOL[g] <= 8 * E, (g, E, pg.TOL[g])


@pytest.mark.parametrize("name", CHAIN_NAMES)
def test_chain_cases_stay_clear_of_the_kinks(golden_table, name):
    _, table = golden_table
    c = pg.chain_case(name)
    assert c["seed"] == table[name]["seed"]
    margin, clamped, band_empty, moved = pg.chain_margins(c)
    print(name, "margin %.3g clamped %.2f %% mask moves %.1f %% of the samples" % (margin, 100 * clamped, 100 * moved))
    assert margin > 1e-4 and clamped <= 0.01 and band_empty
    if c["remove_halo"]:
        assert moved >= 0.05                                 # (the mask is no bystander of these cases)
    w = np.abs(c["w"])
    assert w.min() >= 0.25 and w.max() < 1


def test_upstream_weights_of_every_case():
    for name in pg.POLY_NAMES + [pg.LONG]:
        w = np.abs(pg.poly_case(name)["w"])
        assert w.min() >= 0.25 and w.max() < 1, name


# ---------------------------------------------------------------------------------------------
# the symbol and the refusals
# ---------------------------------------------------------------------------------------------
def test_new_symbol_is_declared_exported_and_bound():
    header = open(os.path.join(REPO, "include", "polyblur_hip.h")).read()
    lib = capi.load_library()
    from polyblur_amd.engine import Engine
    assert re.search(r"\bint %s\(" % SYMBOL, header)
    assert SYMBOL in capi.SYMBOLS
    fn = getattr(lib, SYMBOL)
    assert fn.argtypes is not None and len(fn.argtypes) == 12
    assert callable(Engine.compute_polynomial_phase_taps_backward_ptr)
    assert "deblurring.py:141-169" in header and "filters.py:255-273" in header
    assert lib.pb_version() == 200
    from polyblur_amd import build
    assert "conv_phase_grad.hip" in build.SOURCES


def test_pinned_refusals_are_unchanged():
    """no operand on a ROCm device: the text pinned since the forward was built, first"""
    import polyblur_amd as pa
    x, k = torch.rand(1, 3, 16, 18), torch.rand(1, 1, 3, 5)
    xg, kg = x.clone().requires_grad_(True), k.clone().requires_grad_(True)
    calls = [
        ("compute_polynomial(not_symmetric=True)", lambda: pa.compute_polynomial(xg, k, 6, 1, method="fft", not_symmetric=True)),
        ("inverse_filtering_nonsymmetric", lambda: pa.inverse_filtering_nonsymmetric(xg, k, 6, 1)),
        ("inverse_filtering_nonsymmetric", lambda: pa.inverse_filtering_nonsymmetric(x, kg, 6, 1)),
        ("inverse_filtering_nonsymmetric", lambda: pa.inverse_filtering_nonsymmetric(x.half(), kg, 6, 1, do_edgetaper=True)),
        ("inverse_filtering_nonsymmetric", lambda: pa.inverse_filtering_nonsymmetric(xg, torch.rand(1, 1, 4, 6), 6, 1, remove_halo=True)),
    ]
    for what, call in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == "%s has no backward pass: the pure-phase filter is not differentiated" % what


def test_new_refusals_come_before_any_device_work(monkeypatch):
    """beside a ROCm operand (stood in for here: this machine has none) every refusal is one line and raised before the engine
    is touched; tests/test_gpu_phase_autograd.py raises them with real ROCm tensors"""
    import polyblur_amd as pa
    from polyblur_amd import _frontend as fe, nonblind
    monkeypatch.setattr(nonblind, "_any_rocm", lambda *operands: True)
    x, k = torch.rand(1, 3, 16, 18), torch.rand(1, 1, 4, 5)
    xg, kg = x.clone().requires_grad_(True), k.clone().requires_grad_(True)
    calls = [
        (fe.FLOAT32_ONLY, lambda: pa.inverse_filtering_nonsymmetric(x.half(), kg, 6, 1)),
        (fe.CPU_WITH_GRAD % "img", lambda: pa.compute_polynomial(xg, k, 6, 1, not_symmetric=True)),
        (fe.CPU_WITH_GRAD % "kernel", lambda: pa.inverse_filtering_nonsymmetric(x, kg, 6, 1)),
        (fe.NO_EDGETAPER, lambda: pa.inverse_filtering_nonsymmetric(xg, k, 6, 1, do_edgetaper=True)),
        (fe.HALO_ONLY, lambda: pa.inverse_filtering_nonsymmetric(xg, k, 6, 1, remove_halo=True)),
    ]
    for reason, call in calls:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value).endswith("has no backward pass: " + reason) and "\n" not in str(e.value)
