"""CPU checks of tests/stencil_ref.py, the float64 reference, the restated phase-list rule and the case families of
tests/test_gpu_stencil_conformance.py: the reference against the project's fp32 oracle and against tests/window_ref.py, the walk
of the phase list against the reference, what every case claims about its record against the restated rule, the coverage tables,
and -- the evidence that the cases can tell -- seven ways the body could be wrong, each caught by a named case by more than 100
times that case's tolerance.

What today's dense Gaussians cannot see (test_what_the_gaussians_of_the_suite_cannot_see): on the 25 x 25 Gaussian of 66 degrees,
sigma 2.095, rho 1.314 (tests/test_gpu_onepass.py, tests/test_window_ref_cpu.py) dropping the last live phase of any kind group
moves the output by < 1e-13 and evaluating the fillers with the previous phase's taps by < 1e-13, against the suite's 2e-6;
correlation in place of convolution moves a point-symmetric Gaussian by < 1e-14 under either boundary; a rank-1 Gaussian whose
taps underflow beyond radius 10 loses < 1e-20 with the taps beyond 8.  The swapped odd-aligned pair, the clamp in place of the
zero boundary and the wrap period of Wp - 1 are visible on any Gaussian: for those the directed cases add the positions, not the
kind of fault."""
import numpy as np
import pytest

import stencil_ref as sr
import window_ref as wr
from oracle import polyblur_ref as ref

BOUNDARIES = ((sr.ZERO, "direct"), (sr.WRAP, "fft"))
SUITE_TOL = 2e-6                                    # the suite's bound on one reblurring pass (tests/test_gpu_parity.py)


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def _gaussian(deg, sigma, rho):
    f = lambda v: np.array([v], np.float32)
    return ref.gaussian_kernel_2d(f(np.deg2rad(deg)), f(sigma), f(rho))[0]


# ---------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------
ORACLE_CASES = [("dense", lambda: sr.b_cases(12)[-1][1], (40, 44)), ("dense-symmetric", lambda: sr.d_taps(8), (33, 37)),
                ("asymmetric", lambda: sr.geometry_taps("general", 10), (40, 44)), ("small", lambda: sr.b_cases(12)[-1][1], sr.SMALL_DOMAIN),
                ("small-sparse", lambda: sr.geometry_taps("general", 12), sr.SMALL_DOMAIN)]


@pytest.mark.parametrize("boundary,method", BOUNDARIES)
@pytest.mark.parametrize("name,taps,domain", ORACLE_CASES)
def test_correlate64_matches_the_oracle(name, taps, domain, boundary, method):
    """within the oracle's own rounding: an fp32 sum of N products (direct), complex64 transforms (fft: 1e-6 of the peak of S, the
    bound tests/test_window_ref_cpu.py holds the same oracle to)"""
    k = taps()
    x = sr.white((1, 2) + domain, 11)
    want, S = sr.correlate64(x, k[None], boundary)
    got = ref.convolve2d(x, k[None, None], method=method)
    n = int(np.count_nonzero(k))
    d = np.abs(got.astype(np.float64) - want)
    bound = sr.sum_bound(n + 1, S) if method == "direct" else 1e-6 * S.max()
    print("%s %s %s: oracle against correlate64 %.3g (bound %.3g)" % (name, domain, method, d.max(), np.max(bound)))
    assert (d <= bound).all(), (name, method, d.max())
    assert d.max() < 1e-3 * np.abs(want).max()


def test_small_domain_wraps_more_than_once():
    """8 x 9 under wrap: the tap 12 columns away lands 12 mod 9 = 3 columns away"""
    x = sr.white((1, 1) + sr.SMALL_DOMAIN, 3)
    k = np.zeros((1, 25, 25), np.float32)
    k[0, 0, 24] = 1.0
    y, _ = sr.correlate64(x, k, sr.WRAP)
    assert np.array_equal(y[0, 0], np.roll(x[0, 0].astype(np.float64), (-12, 12), axis=(0, 1)))
    y, _ = sr.correlate64(x, k, sr.ZERO)
    assert not y.any()


@pytest.mark.parametrize("taps", [lambda: sr.d_taps(12), lambda: sr.b_cases(8)[-1][1], lambda: sr.geometry_taps("general", 6)])
def test_inverse_filter64_agrees_with_window_ref_under_wrap(taps):
    k = taps()
    x = sr.white((1, 2, 30, 41), 5)
    a = sr.inverse_filter64(x, k[None], wr.ALPHA, wr.BETA, sr.WRAP)
    b = wr.reference64(x, k[None], wr.ALPHA, wr.BETA)
    assert maxabs(a, b) < 1e-12 * max(1.0, float(np.abs(b).max())), maxabs(a, b)


# ---------------------------------------------------------------------------------------------
# the walk and the claims
# ---------------------------------------------------------------------------------------------
def _tolerance(k, x, boundary):
    """the largest per-sample bound of the general body on this case"""
    _, S = sr.correlate64(x, k, boundary)
    return float(np.max(sr.sum_bound(max(int(np.count_nonzero(kk)) for kk in k), S)))


@pytest.mark.parametrize("R", sr.CLASSES)
def test_family_a_walk_claims_and_coverage(R):
    k = sr.a_taps(R)
    pos = sr.a_positions(R)
    assert len(pos) == (2 * R + 1) ** 2 == len(set(pos)) == k.shape[0]
    lists = []
    for n, (i, j) in enumerate(pos):
        assert k[n, i, j] == np.float32(0.6) and np.count_nonzero(k[n]) == 2
        sep, rad, nphase, phases = sr.phase_list(k[n], sr.A_SUPPORT)
        assert (sep, rad) == (0, R), ((i, j), sep, rad)
        assert sr.walked_taps_equal(k[n], R, phases), (R, i, j)
        lists.append(phases)
    x = sr.a_input(R)
    for boundary, _ in BOUNDARIES:
        want, _ = sr.correlate64(x, k, boundary)
        assert np.array_equal(sr.walk64(x, k, lists, boundary, radii=[R] * len(pos)), want)


def test_family_a_visits_every_tap_of_every_class():
    assert sum(len(sr.a_positions(R)) for R in sr.CLASSES) == 1605
    for R in sr.CLASSES:
        assert set(sr.a_positions(R)) == {(i, j) for i in range(25) for j in range(25) if max(abs(i - 12), abs(j - 12)) <= R}


@pytest.mark.parametrize("R", sr.CLASSES)
def test_family_b_walk_claims_and_coverage(R):
    cases = sr.b_cases(R)
    seen_patterns, parities, single, last_slot = set(), set(), False, False
    x = sr.white((1,) + sr.B_SHAPE, 200 + R)
    for name, k, claimed in cases:
        sep, rad, nphase, phases = sr.phase_list(k, sr.B_SUPPORT)
        assert sep == 0 and nphase == claimed, (name, nphase, claimed)
        assert rad == (4 if name == "zero" else R), (name, rad)
        assert len(phases) == sum(nphase) <= 175 + 3 and all(n % 2 == 0 for n in nphase)
        assert sr.walked_taps_equal(k, rad, phases), name
        for boundary, _ in BOUNDARIES:
            want, _ = sr.correlate64(x, k[None], boundary)
            assert np.array_equal(sr.walk64(x, k[None], [phases], boundary, radii=[rad]), want), name
        live = [sum(1 for kind, row, _ in phases if kind == g and row is not None) for g in range(3)]
        if name != "zero":
            seen_patterns.add(tuple(n > 0 for n in live))
            parities |= {(g, n & 1) for g, n in enumerate(live) if n}
            single |= sum(live) == 1
            last_slot |= phases[-1][1] is not None
        if abs(float(k.astype(np.float64).sum()) - 1.0) > 1e-6:
            assert name == "zero", name
    assert seen_patterns == {(a, b, c) for a in (False, True) for b in (False, True) for c in (False, True)} - {(False,) * 3}
    assert parities == {(g, p) for g in range(3) for p in (0, 1)}
    assert single and last_slot
    full = [c for c in cases if c[0].endswith("full")][0]
    assert sum(1 for _, row, _ in sr.phase_list(full[1], sr.B_SUPPORT)[3] if row is not None) == (2 * R + 1) * (R // 2 + 1)
    assert not np.array_equal(full[1], full[1][::-1, ::-1])
    if R == 4:
        assert sr.phase_list(cases[-1][1], sr.B_SUPPORT)[2] == [0, 0, 0]


def test_family_b_columns_are_seen_by_one_chunk():
    assert [sr.b_columns(R) for R in sr.CLASSES] == [(12, 8, 16), (10, 6, 18), (8, 4, 20), (6, 2, 22), (12, 0, 24)]
    for R in sr.CLASSES:
        off, nq = 12 - R, R // 2 + 1
        for kind, col in enumerate(sr.b_columns(R)):
            qs = [q for q in range(nq) if 4 * q + off - 3 <= col <= 4 * q + off + 3]
            assert len(qs) == 1 and (1 if qs[0] == 0 else (2 if qs[0] == nq - 1 else 0)) == kind, (R, kind, col, qs)


def test_family_c_claims_and_coverage():
    templates = set()
    x = sr.white((1,) + sr.C_SHAPE, 300)
    for name, k, sep, rad in sr.c_cases():
        got = sr.phase_list(k, sr.FULL)
        assert got[:2] == (sep, rad), (name, got[:2])
        rho = sr.residual(k)
        assert (rho < 2e-7) if sep else (rho > 1e-3), (name, rho)           # (a margin no fp32 evaluation of the sum crosses)
        if sep:
            templates.add((rad, sr.rank1_template(rad)))
            kx, ky = sr.marginals(k)
            for boundary, _ in BOUNDARIES:
                want, _ = sr.correlate64(x, k[None], boundary)
                assert maxabs(sr.rank1_64(x, kx[None], ky[None], sr.rank1_template(rad), boundary), want) <= rho * 0.6 + 1e-15, name
    assert templates == {(4, 4), (6, 8), (8, 8), (10, 12), (12, 12)}
    names = [c[0] for c in sr.c_cases()]
    assert "rx12-ry1" in names and "rx1-ry12" in names and "rx0-ry0" in names and "asymmetric-marginal" in names


def test_family_d_is_dense_and_point_symmetric():
    for R in sr.RANK1_CLASSES:
        k = sr.d_taps(R)
        assert np.array_equal(k, k[::-1, ::-1]) and np.count_nonzero(k) == (2 * R + 1) ** 2
        sep, rad, nphase, _ = sr.phase_list(k, sr.FULL)
        assert (sep, rad) == (0, R) and sum(nphase) >= (2 * R + 1) * (R // 2 + 1)


def _e_cases():
    return [("gaussian %s" % (g,), _gaussian(*g)) for g in sr.E_GAUSSIANS] + [(n, sr.e_ring(v)) for n, v in sr.E_RINGS]


def test_family_e_walk_and_claims():
    x = sr.white((1,) + sr.E_SHAPE, 400)
    for name, k in _e_cases():
        full, adaptive = sr.phase_list(k, sr.FULL), sr.phase_list(k, sr.ADAPTIVE)
        assert sr.support_margin(k) >= 2.0, (name, sr.support_margin(k))
        if name.startswith("gaussian"):
            assert adaptive[1] < full[1], (name, full[1], adaptive[1])
        else:
            assert adaptive[1] == full[1] == 8
        assert sr.walked_taps_equal(k, full[1], full[3]), name
        dropped = sr.dropped_mass(k, adaptive[1], adaptive[3])
        print("%s: class %d full, %d adaptive; phases %s / %s; dropped mass %.3g" % (name, full[1], adaptive[1], full[2], adaptive[2], dropped))
        assert dropped < 1e-7
        for boundary, _ in BOUNDARIES:
            want, _ = sr.correlate64(x, k[None], boundary)
            assert np.array_equal(sr.walk64(x, k[None], [full[3]], boundary, radii=[full[1]]), want), name
            d = maxabs(sr.walk64(x, k[None], [adaptive[3]], boundary, radii=[adaptive[1]]), want)
            assert d <= dropped * float(x.max()) + 1e-16, (name, d, dropped)
    kept, lost = sr.phase_list(sr.e_ring(2e-10), sr.ADAPTIVE), sr.phase_list(sr.e_ring(5e-11), sr.ADAPTIVE)
    assert sum(kept[2]) > sum(lost[2]) and sr.dropped_mass(sr.e_ring(2e-10), 8, kept[3]) == 0.0
    assert sr.dropped_mass(sr.e_ring(5e-11), 8, lost[3]) > 20 * 5e-11


def test_geometry_records_and_domains():
    for body, R in sr.GEOMETRY_BODIES:
        k = sr.geometry_taps(body, R)
        sep, rad, nphase, phases = sr.phase_list(k, sr.geometry_support(body))
        assert sep == (body == "rank1") and rad == R, (body, R, sep, rad)
        if body == "general":
            assert all(nphase) and not np.array_equal(k, k[::-1, ::-1])
        assert len(sr.convolve_domains(R)) == 5 and len(sr.inverse_shapes(R)) == 7 and len(set(sr.fp16_shapes(R))) == 4
        assert max(max(s) for s in sr.inverse_shapes(R)) + 24 <= 152
    assert sr.interior_pair(12) == ((140, 140), (139, 140)) and sr.interior_pair(12, virtual=True) == ((128, 128), (127, 128))
    # classes 6 and 10 never take the 16-byte path: neither pitch nor first column is a multiple of 4
    for R in sr.CLASSES:
        (n, _), _ = sr.interior_pair(R)
        assert ((n | (64 - R)) & 3 == 0) == (R in (4, 8, 12))


# ---------------------------------------------------------------------------------------------
# the mutants
# ---------------------------------------------------------------------------------------------
def _b_case(R, name):
    return [c for c in sr.b_cases(R) if c[0] == name][0][1]


GENERAL_MUTANTS = [
    (("drop", 0), "R8-321", sr.ZERO), (("drop", 1), "R8-321", sr.ZERO), (("drop", 2), "R8-321", sr.WRAP), (("drop", 0), "R12-100", sr.WRAP),
    ("filler", "R8-111", sr.ZERO), ("filler", "R6-100", sr.WRAP), ("swap", "R10-222", sr.ZERO), ("clamp", "R4-111", sr.ZERO),
    ("period", "R12-111", sr.WRAP), ("flip", "R8-321", sr.ZERO), ("flip", "R8-321", sr.WRAP),
]


@pytest.mark.parametrize("mutant,name,boundary", GENERAL_MUTANTS)
def test_mutants_of_the_general_body_are_caught(mutant, name, boundary):
    R = int(name[1:name.index("-")])
    k = _b_case(R, name)
    x = sr.white((1,) + sr.B_SHAPE, 200 + R)
    phases = sr.phase_list(k, sr.B_SUPPORT)[3]
    want, _ = sr.correlate64(x, k[None], boundary)
    tol = _tolerance(k[None], x, boundary)
    d = maxabs(sr.walk64(x, k[None], [phases], boundary, mutant=mutant, radii=[R]), want)
    print("mutant %s on %s: moves the output by %.3g, tolerance %.3g" % (mutant, name, d, tol))
    assert d > 100 * tol, (mutant, name, d, tol)


def test_the_swapped_pair_is_caught_at_every_position_of_family_a():
    for R in (4, 12):
        k, x = sr.a_taps(R), sr.a_input(R)
        lists = [sr.phase_list(kk, sr.A_SUPPORT)[3] for kk in k]
        want, _ = sr.correlate64(x, k, sr.ZERO)
        got = sr.walk64(x, k, lists, sr.ZERO, mutant="swap", radii=[R] * len(lists))
        d = np.abs(got - want).max(axis=(1, 2, 3))
        assert d.min() > 100 * 3 * sr.U32, (R, d.min())


def test_the_rank1_mutant_is_caught():
    name, k, _, rad = [c for c in sr.c_cases() if c[0] == "rx9-ry10"][0]
    x = sr.white((1,) + sr.C_SHAPE, 300)
    kx, ky = sr.marginals(k)
    want, S = sr.correlate64(x, k[None], sr.ZERO)
    tol = float(np.max(sr.sum_bound(np.count_nonzero(kx) + np.count_nonzero(ky), S))) + sr.residual(k) * float(x.max())
    d = maxabs(sr.rank1_64(x, kx[None], ky[None], 12, sr.ZERO, mutant="r8"), want)
    assert rad == 10 and d > 100 * tol, (d, tol)


def test_what_the_gaussians_of_the_suite_cannot_see():
    k = _gaussian(66.0, 2.095, 1.314)
    x = sr.white((1, 1, 70, 76), 500)
    sep, R, nphase, phases = sr.phase_list(k, sr.FULL)
    assert (sep, R) == (0, 12)
    for boundary, _ in BOUNDARIES:
        want, _ = sr.correlate64(x, k[None], boundary)
        for mutant in (("drop", 0), ("drop", 1), ("drop", 2), "filler", "flip"):
            if mutant == "filler" and all(row is not None for _, row, _ in phases):
                continue
            d = maxabs(sr.walk64(x, k[None], [phases], boundary, mutant=mutant, radii=[R]), want)
            print("the 25 x 25 Gaussian under mutant %s, boundary %d: %.3g" % (mutant, boundary, d))
            assert d < 1e-3 * SUITE_TOL, (mutant, d)
            if mutant == "flip":
                assert d < 1e-13                            # (float64 sums in another order; the oracle's taps are symmetric to an fp32 rounding)
        for mutant in ("swap", "clamp" if boundary == sr.ZERO else "period"):
            d = maxabs(sr.walk64(x, k[None], [phases], boundary, mutant=mutant, radii=[R]), want)
            assert d > 100 * SUITE_TOL, (mutant, d)
    # a rank-1 Gaussian of radius class 10: the taps beyond 8 are below 1e-20
    found = None
    for sigma in (0.70, 0.71, 0.72, 0.73, 0.74, 0.75):
        g = _gaussian(0.0, sigma, 0.5)
        if sr.phase_list(g, sr.FULL)[:2] == (1, 10):
            found = g
            break
    assert found is not None
    kx, ky = sr.marginals(found)
    want, _ = sr.correlate64(x, found[None], sr.ZERO)
    full = sr.rank1_64(x, kx[None], ky[None], 12, sr.ZERO)
    assert maxabs(sr.rank1_64(x, kx[None], ky[None], 12, sr.ZERO, mutant="r8"), full) < 1e-20
    assert maxabs(full, want) < SUITE_TOL
