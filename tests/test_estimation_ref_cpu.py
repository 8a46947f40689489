"""tests/estimation_ref.py is what tests/test_gpu_estimation_planted.py holds the engine to; here, without a GPU:

  * its spectral derivative (numpy.fft) is estimation_grad_ref.deriv_matrix on odd and even lengths, its default grid
    estimation_grad_ref.interp_weights, its forward estimation_grad_ref.estimate at 6 x 30; its weights of every grid are the
    oracle's float32 ones;
  * the forward against the REFERENCE (tests/golden/estimation_planted.npz: direction counts 1 .. 12 x 7 / 30 / 64, quantiles, the
    mask) within er.BOUND_GOLDEN, theta exactly;
  * every case of er.cases() keeps the margins of estimation_grad_ref (arg-max gap, gray-range gap and arg-min gap 1e-3, clamp
    distance 1e-2) and every targeted region holds the maximum of its direction: without it the maximum drops by at least 10
    tolerances (measured: 0.05 to 0.4 of the maximum, the tolerance is 3.0e-6);
  * every mutant of the forward is rejected by its named case (er.KILLERS) by at least 10 tolerances in the named field;
  * er.TOL is 4 x the float32 oracle's error against the forward over exactly those cases.

Cases changed or dropped for missing a gauge (none was loosened):
  * a point-symmetric ridge / wave has two equal maxima per direction (arg-max gap 0): one flank of the ridge is 1.6 x wider, the
    wave's window and phase are offset;
  * a smooth plane's two lowest values are closer than 1e-3 of the range: the lowest pixel of `planted` is lowered by 0.004;
  * ridge angles / noise seeds where the default missed the arg-min gap: er._PHI, er._SEED (the first candidate that passes);
  * DROPPED n_angles = 1 with n_interp = 64: interp = (w0 + w1) m there, the arg-min gap is 8.6e-4 on every image (er.DROPPED_GRIDS);
  * DROPPED theta indices 1 and 29 of 30 and 3 of 7 of `oriented`: er.search_oriented (windowed waves in half-degree steps at five
    sharpnesses) finds no image with its arg-min there and every margin kept -- at n_interp = 7 the rows 3 and 4 both interpolate
    to mags[3] alone, a near-tie below the arg-min gauge; index 0 of 30, 7 and 64 and the last index of 7 and 64 are reached, 28 is
    the highest of 30.  The search's results are kept as data (er.ORIENTED) and every entry is checked here;
  * DROPPED `tied`: the mirror symmetry gives mags[k] = mags[n - k] in exact arithmetic only -- the float32 transforms of a
    mirrored line do not round alike (test_tied_is_not_a_tie_in_float32) -- so the image does not make two entries of interp equal.
    The exact tie that does exist is kept instead: sparse grids (n_angles <= 5 with 7 or 30 interpolated angles) have rows of
    weights that are all zero, interp is exactly 0 there in any arithmetic, and the FIRST such index must win
    (er.gauges: exact_tie; the mutant `last_min` is rejected by a1_i7).  In such a case -- 21 of the `angles` cases -- theta, i_min
    and sigma (4.0, from interp == 0) are fixed by the grid alone: only mags, interp and rho depend on the image there; the clamp
    distance of rho is kept;
  * the quantised cases are exempt from the arg-max and gray-range gaps: ties are what they are for, and a tie changes neither a
    maximum nor a quantile.
"""
import numpy as np
import pytest

import estimation_grad_ref as eg
import estimation_ref as er
from oracle import polyblur_ref as ref

CASES = {c.id: c for c in er.cases()}


@pytest.mark.parametrize("N", [2, 3, 5, 8, 16, 33, 64])
def test_fft_derivative_is_the_derivative_matrix(N):
    x = np.random.default_rng(N).standard_normal((4, N))
    assert np.abs(er.spectral_derivative(x, 1) - x @ eg.deriv_matrix(N).T).max() < 1e-12
    assert np.abs(er.spectral_derivative(x.T, 0) - eg.deriv_matrix(N) @ x.T).max() < 1e-12


def test_default_grid_and_forward_are_estimation_grad_refs():
    assert np.array_equal(er.grid_weights(6, 30), eg.interp_weights())
    x = eg.blurred_noise(3, (2, 3, 33, 47))
    for sat in (False, True):
        a, b = eg.estimate(x, 0.362, 0.464, discard_saturation=sat), er.forward(x, c=0.362, b=0.464, discard_saturation=sat)
        for ra, rb in zip(a, b):
            assert ra["i_min"] == rb["i_min"] and ra["i_ortho"] == rb["i_ortho"] and np.array_equal(ra["arg"], rb["arg"])
            for f in ("mags", "interp", "sigma", "rho", "kernel", "lo", "hi"):
                assert np.abs(np.asarray(ra[f]) - np.asarray(rb[f])).max() < 1e-12, f


@pytest.mark.parametrize("na", range(1, 13))
def test_weights_of_every_grid_are_the_oracles(na):
    for ni in (1, 7, 30, 64):
        th, it = ref.angle_grids(na, ni)
        w32 = ref.keys_cubic_weights(it.astype(np.float32) / np.float32(ni), th.astype(np.float32) / np.float32(ni))
        # (cubics of d <= 2 in float32: a few 1e-7 each, divided by row sums as small as 0.3)
        assert np.abs(er.grid_weights(na, ni) - w32).max() < 1e-5 * max(1.0, np.abs(w32).max()), (na, ni)


def test_forward_against_the_reference(golden):
    g = golden("estimation_planted.npz")
    worst = {}
    for name, case in er.golden_cases():
        assert np.array_equal(g[name + "_x"], er.image(case)), name
        o = case.opts
        assert np.array_equal(g[name + "_opts"], [o["n_angles"], o["n_interp"], o["q"], float(o["discard_saturation"]), o["c"], o["b"]])
        recs = er.run(case)
        for bi, r in enumerate(recs):
            assert abs(r["theta"] - g[name + "_theta"][bi]) < 1e-6, name
            for f, got in (("sigma", r["sigma"]), ("rho", r["rho"]), ("kernel", r["kernel"])):
                want = g[name + "_" + f][bi, 0] if f == "kernel" else g[name + "_" + f][bi]
                e = float(np.abs(got - want).max())
                worst[f] = max(worst.get(f, 0.0), e)
                assert e <= er.BOUND_GOLDEN[f], (name, f, e)
    print("largest |float64 - reference|:", worst)
    # the mask and the quantile change the answer there: the golden pairs differ by far more than the bound
    assert abs(g["saturated_0_sigma"][0] - g["saturated_1_sigma"][0]) > 100 * er.BOUND_GOLDEN["sigma"]


@pytest.mark.parametrize("theme", sorted({c.theme for c in er.cases()}))
def test_every_case_keeps_its_gauges(theme):
    for c in er.cases():
        if c.theme != theme:
            continue
        recs = er.run(c)
        assert er.gauges_ok(c, recs), (c.id, er.gauges(c, recs))
        H, W = recs[0]["shape"][1:]
        for bi, reg, d in c.targets:
            drop = er.loss_without([recs[bi]], er.region(H, W, reg))[0][d]
            assert drop >= 10 * er.TOL["mags"], (c.id, bi, reg, d, drop)
            assert drop >= 0.04, (c.id, bi, reg, d, drop)             # (what the builder is for: the region holds the maximum)
        if theme in ("where", "fixed_narrow", "fixed_wide", "long", "angles") and c.build.func is er.planted:
            # every direction's arg-max lies within 4 px of the image's ridge
            for bi, r in enumerate(recs):
                at = er.WHERE[c.build.args[4][bi]](H, W)
                ys, xs = np.divmod(r["arg"], W)
                dist = np.hypot((ys - at[0] + H / 2) % H - H / 2, (xs - at[1] + W / 2) % W - W / 2)
                assert dist.max() <= 4.0, (c.id, bi, dist)
            # the images of a batch differ: every image's maxima are its own
            if len(recs) > 1:
                assert er.err(recs[-1]["mags"], recs[0]["mags"], "mags") > 10 * er.TOL["mags"], c.id


def test_the_saturated_builder_does_what_it_is_for():
    for c in er.cases():
        if c.theme != "mask":
            continue
        on, off = er.run(c), er.run(c, discard_saturation=False)[0]
        g = on[0]["gray"]
        H, W = g.shape
        assert 0 < on[0]["lo"] and on[0]["hi"] < 1
        raw = g > np.float32(er.SAT)
        norm = (g - on[0]["lo"]) / (on[0]["hi"] - on[0]["lo"]) > np.float32(er.SAT)
        assert raw.sum() > 0 and (norm & ~raw).sum() > 0 and (g == np.float32(er.SAT)).sum() > 0
        assert all(raw[divmod(int(a), W)] for a in off["arg"]), c.id      # without the mask every maximum sits on a masked pixel
        assert er.err(on[0]["mags"], off["mags"], "mags") > 10 * er.TOL["mags"]
        assert abs(on[0]["sigma"] - off["sigma"]) > 10 * er.TOL["sigma"] and abs(on[0]["rho"] - off["rho"]) > 10 * er.TOL["rho"]


def test_the_range_cases_put_the_extremes_where_they_say():
    for c in er.cases():
        if c.theme != "range":
            continue
        B, C, H, W, lo_at, hi_at = c.build.args[:6]
        g = er.gray32(er.image(c))
        for bi in range(B):
            assert np.unravel_index(np.argmin(g[bi]), (H, W)) == (lo_at[0] % H, lo_at[1] % W), c.id
            assert np.unravel_index(np.argmax(g[bi]), (H, W)) == (hi_at[0] % H, hi_at[1] % W), c.id
        if B > 1:
            assert len({float(g[bi].min()) for bi in range(B)}) == B and len({float(g[bi].max()) for bi in range(B)}) == B


def test_the_chain_cases_reach_what_they_say():
    recs = {c.id: er.run(c) for c in er.cases() if c.theme == "chain"}
    for ni, missing in ((30, {1, 29}), (7, {3}), (64, set())):
        got = {r[0]["i_min"] for cid, r in recs.items() if cid.endswith("_of_%d" % ni)}
        want = set(range(30)) if ni == 30 else ({0, 3, 6} if ni == 7 else {0, 1, 31, 32, 63})
        assert got == want - missing == set(er.ORIENTED[ni]), (ni, got)
        for i in er.ORIENTED[ni]:                                                       # every entry of the table gives its index
            assert recs["oriented_i%d_of_%d" % (i, ni)][0]["i_min"] == i
    assert any(r[0]["theta_deg"] >= 90 for r in recs.values()) and any(r[0]["theta_deg"] < 90 for r in recs.values())      # the wrap of (theta + 90) % 180
    v = {cid: recs[cid][0]["v"] for cid in ("clamp_high_sigma", "clamp_high_both", "clamp_low", "clamp_none")}
    assert v["clamp_high_sigma"][0] > 16 and 0.09 < v["clamp_high_sigma"][1] < 16
    assert min(v["clamp_high_both"]) > 16 and max(v["clamp_low"]) < 0.09 and all(0.09 < u < 16 for u in v["clamp_none"])
    assert recs["force_theta"][0]["theta_deg"] == 132 and recs["force_theta"][0]["i_min"] == 22
    assert er.run(CASES["force_theta"], force_theta_deg=None)[0]["i_min"] != 22


def test_the_quantised_cases_are_what_they_say():
    seen_integer = seen_negative = seen_interpolated = False
    for c in er.cases():
        if c.theme != "quantile":
            continue
        x = er.image(c)
        g = np.sort(er.gray32(x).reshape(-1))
        values, counts = np.unique(g, return_counts=True)
        assert len(values) <= 8 and counts.max() >= 0.35 * g.size, c.id                 # heavy ties, one value holds a third and more
        r = np.float32(c.opts["q"]) * np.float32(g.size - 1)
        seen_integer |= float(r) == np.floor(r) and r > 0
        seen_negative |= g[0] < 0
        rec = er.run(c)[0]
        seen_interpolated |= rec["lo"] not in values.astype(np.float64)
        if c.opts["q"] > 0.1:                                                             # the clip of normalize() acts at both ends
            assert (rec["gray"] < rec["lo"]).sum() > 0 and (rec["gray"] > rec["hi"]).sum() > 0, c.id
    assert seen_integer and seen_negative and seen_interpolated


def _power(a, b, field):
    if field == "theta":
        return np.inf if any(x["theta"] != y["theta"] for x, y in zip(a, b)) else 0.0
    return max(er.err(x[field], y[field], field) for x, y in zip(a, b)) / er.TOL[field]


@pytest.mark.parametrize("mutant", er.MUTANTS)
def test_every_mutant_is_rejected(mutant):
    cid, field = er.KILLERS[mutant]
    c = CASES[cid]
    p = _power(er.run(c, mutant=mutant), er.run(c), field)
    print("%s: %s differs by %.3g tolerances in %s" % (mutant, cid, p, field))
    assert p >= 10, (mutant, cid, field, p)


def test_tied_is_not_a_tie_in_float32():
    x = er.tied(32, 48)
    assert np.array_equal(x, x[..., (-np.arange(48)) % 48])
    r = er.forward(x)[0]
    assert np.abs(r["mags"] - r["mags"][::-1]).max() < 1e-12                              # exact arithmetic: the tie is there
    _, info = ref.estimate_gaussian_blur(x, c=0.362, b=0.468, return_info=True)
    assert not np.array_equal(info["mags"][0], info["mags"][0][::-1])                   # float32: it is not


def test_tolerances_are_four_times_the_oracles_error():
    worst = {f: (0.0, None) for f in er.TOL}
    for c in er.cases():
        o = c.opts
        if o.get("force_theta_deg") is not None:
            continue                                                                    # (the oracle takes no forced angle)
        x = er.image(c)
        x32 = x.astype(np.float32) * np.float32(1.0 / 255.0) if x.dtype == np.uint8 else x.astype(np.float32)
        _, info = ref.estimate_gaussian_blur(x32, c=o["c"], b=o["b"], q=o["q"], n_angles=o["n_angles"], n_interpolated_angles=o["n_interp"],
                                             discard_saturation=o["discard_saturation"], return_info=True)
        for bi, r in enumerate(er.run(c)):
            assert int(info["i_min"][bi]) == r["i_min"] and abs(float(info["theta"][bi]) - r["theta"]) < 1e-6, c.id
            for f in er.TOL:
                e = er.err(info[f][bi], r[f], f)
                if e > worst[f][0]:
                    worst[f] = (e, c.id)
    for f, (e, cid) in worst.items():
        print("%-6s float32 oracle vs float64: %.3g (%s) -> 4 x = %.3g; er.TOL = %.3g" % (f, e, cid, 4 * e, er.TOL[f]))
    # sigma and rho are the same function of two entries of interp: which of the two lands on the steep part of c^2 / m^2 - b^2 is
    # an accident of the case, so they share the larger bound
    both = max(worst["sigma"][0], worst["rho"][0])
    for f, e in (("mags", worst["mags"][0]), ("interp", worst["interp"][0]), ("sigma", both), ("rho", both)):
        assert er.TOL[f] / 1.5 <= 4 * e <= er.TOL[f] * 1.5, (f, e)          # (as test_blind_autograd_cpu: another CPU sums in another order)
