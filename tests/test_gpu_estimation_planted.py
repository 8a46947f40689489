"""The blur estimation on inputs whose answer depends on WHERE the maximum sits (csrc/estimate.hip, csrc/lines_fixed.hip), against
the float64 restatement of tests/estimation_ref.py (blur_estimation.py:18-79, deblurring.py:62-63).

Natural images have their arg-max pixels, their gray extremes and their arg-min somewhere in the interior: a kernel that left out
the last row, the unpaired row of an odd height, the last column, the ragged last column tile, or took every image's maxima from
image 0, passed every earlier estimation test.  The cases of er.cases() plant a short ridge, the range's extremes, saturated pixels,
an orientation, a clamp or heavy ties where a path could lose them; tests/test_estimation_ref_cpu.py proves, without a GPU, that
each targeted region holds the maximum it is meant to hold (at least 0.04 of it, the tolerance is 3e-6) and that each one-line
mutant of the forward is rejected by a named case by 10 tolerances and more.

Compared: mags, interp (relative to the image's largest maximum), sigma, rho within er.TOL = 4 x the float32 oracle's error against
float64 over exactly these cases (mags 7.5e-7, interp 8.1e-7, sigma / rho 4.7e-6 -> 3.0e-6, 3.3e-6, 1.9e-5); the kernel within the
1e-5 of test_gpu_parity.py::test_estimate_blur; theta, i_min, gray_min, gray_max exactly.  Every figure is printed before it is
asserted (pytest -s).

That the cases reach the kernels they name was checked by hand on scratch builds with one defect each (none committed): the lane
of an even width's last column dropped in ColsIO::store plus the fold of k < 7 only in blur_params_kernel (81 of 220 cases failed:
the even-width last-column cases of the run-time plan, every PB_COLS_FIXED=0 run of the compiled heights, every n_angles 7 / 12
case); the last row left out of cols_fixed_kernel's fold (all narrow- and wide-tile cases failed, n_angles != 6 at 1080 x 32 did
not); the same in its 1024-thread instances only (exactly the 15 wide-tile cases failed).

Contexts (one per environment setting, made once): default; PB_COLS_FIXED=0 (the run-time-plan column kernel at the heights of the
compiled plans, its 512- and 1024-thread variants); PB_ROWS_FIXED=0; PB_EST_GRAY_ROWS=0 (gray + range in a launch of their own).
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import estimation_ref as er

F32 = np.float32
ENGINE_ENV = {"default": {}, "runtime_cols": {"PB_COLS_FIXED": 0}, "runtime_rows": {"PB_ROWS_FIXED": 0}, "two_launches": {"PB_EST_GRAY_ROWS": 0}}


def _engine(**env):
    from polyblur_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    os.environ.update({k: str(v) for k, v in env.items()})
    try:
        return Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    return {name: _engine(**env) for name, env in ENGINE_ENV.items()}


def opts(case, **over):
    from polyblur_amd.engine import Engine
    o = dict(case.opts, **over)
    kw = dict(c=o["c"], b=o["b"], q=o["q"], n_angles=o["n_angles"], n_interpolated_angles=o["n_interp"], discard_saturation=o["discard_saturation"])
    if o.get("force_theta_deg") is not None:
        kw["force_theta_deg"] = o["force_theta_deg"]
    return Engine.make_options(**kw)


def theta32(rec):
    return F32(rec["theta_deg"]) * F32(np.pi) / F32(180)


def check(tag, info, recs, case, x):
    """one estimation record per image against the float64 forward"""
    na, ni = case.opts["n_angles"] + 1, case.opts["n_interp"]
    gray = er.gray32(x).reshape(len(recs), -1)
    bad = []
    for bi, r in enumerate(recs):
        got = info[bi]
        figures = [(f, er.err(v, r[f], f), er.TOL[f]) for f, v in (("mags", got["mags"][:na]), ("interp", got["interp"][:ni]),
                                                                  ("sigma", got["sigma"]), ("rho", got["rho"]))]
        figures.append(("kernel", er.err(got["kernel"], r["kernel"], "kernel"), er.TOL_KERNEL))
        print("%s image %d: %s" % (tag, bi, "  ".join("%s %.3g / %.3g" % f for f in figures)))
        bad += [(bi,) + f for f in figures if not f[1] <= f[2]]
        if int(got["i_min"]) != r["i_min"] or F32(got["theta"]) != theta32(r):
            bad.append((bi, "theta", int(got["i_min"]), r["i_min"], float(got["theta"]), float(theta32(r))))
        if case.opts["q"] == 0:
            if F32(got["gray_min"]) != gray[bi].min() or F32(got["gray_max"]) != gray[bi].max():
                bad.append((bi, "range", float(got["gray_min"]), float(gray[bi].min()), float(got["gray_max"]), float(gray[bi].max())))
        # (everything past the call's direction counts stays zero: the record is read with the widest strides)
        if np.any(got["mags"][na:] != 0) or np.any(got["interp"][ni:] != 0):
            bad.append((bi, "tail", got["mags"][na:].tolist(), got["interp"][ni:].tolist()))
    assert not bad, (tag, bad)


def run_case(engines, case):
    x = er.image(case)
    recs = er.run(case)
    for name in case.engines:
        check("%s [%s]" % (case.id, name), engines[name].estimate_blur(x, opts(case)), recs, case, x)


def _ids(theme):
    return [c for c in er.cases() if c.theme == theme]


@pytest.mark.parametrize("case", _ids("where"), ids=repr)
def test_where_the_maxima_are_taken_runtime_plan(engines, case):
    """grad_cols_kernel with the run-time plan: odd W (scalar loads), even W (vec2), a ragged last tile (37 x 75, 45 x 70: 16-column
    tiles), one-stage plans and the unfused body (16 x 15, 15 x 16), Bluestein (97 x 101), 2 x 3; B = 1 and 3, C = 1, 3, 2; the ridge in
    the last row (the unpaired one of an odd height), the last column, row 0, column 0 and the bottom right corner, each with and
    without the mask; the images of a batch have their ridges in different places"""
    run_case(engines, case)


@pytest.mark.parametrize("case", _ids("fixed_narrow"), ids=repr)
def test_where_the_maxima_are_taken_compiled_plans_narrow_tile(engines, case):
    """all 19 heights of PB_COLS_PLANS (lines_fixed.hip) at W = 32, B = 2, in their narrow tile -- image 0 with its ridge in the last
    row / row 0, image 1 with it in the last column of the last tile / the bottom right corner -- and the same on PB_COLS_FIXED=0"""
    run_case(engines, case)


@pytest.mark.parametrize("case", _ids("fixed_wide"), ids=repr)
def test_where_the_maxima_are_taken_compiled_plans_wide_tile(engines, case):
    """the 15 heights PB_COLS_PLANS compiles a wide (1024-thread) instance for (er.WIDE_PLANS), B = 8 and W = 25 * (4 << lognb): the
    smallest batch and width with P * (W / (4 << lognb)) >= 200 (line_choice.h: choose_cols), W a multiple of the wide tile; the images have their
    ridges in different places, the last one in its last tile's last column and last row.  Not reached: 1080-point columns (they
    never take a wide tile with the compiled plans: choose_cols keeps 16 columns where W % 16 == 0, and the plan is refused where
    it is not); 1200, 1280 and 2560 (no wide instance is compiled)."""
    B, _, H, W = er.image(case).shape
    narrow, wide = er.WIDE_PLANS[H]
    assert B * (W // (4 << narrow)) >= 200 and W % (2 << wide) == 0    # what the case is for: choose_cols takes the wide tile
    run_case(engines, case)


@pytest.mark.parametrize("case", _ids("long"), ids=repr)
def test_long_lines_and_many_tiles(engines, case):
    """extended radices (3240 x 24, 4320 x 32, also on PB_COLS_FIXED=0: grad_cols_kernel<1, 7, 1024, 24 / 18>), through-memory
    columns (8200 x 10, 20736 x 10: grad_cols_long_kernel<1>), and 8 x 8200: 513 column tiles of 16, the ridge in the last one --
    blur_params_kernel folds them in two batches of 128 uint4"""
    if case.id.endswith("8x8200_last_col"):
        # choose_cols starts from lognb = 3 (16 columns) and only lowers it, but for the wide tile, which needs a plan of two stages
        # and more: 8 is one radix-8 stage.  No tile is wider than 16 columns, so there are at least 513
        assert (8200 + 15) // 16 > 512
    run_case(engines, case)


@pytest.mark.parametrize("case", _ids("angles"), ids=repr)
def test_direction_counts(engines, case):
    """n_angles in {1, 2, 3, 5, 7, 12} x n_interpolated_angles in {7, 30, 64} (less (1, 64): er.DROPPED_GRIDS) on 37 x 75, 64 x 96 and
    1080 x 32, where the compiled plan must refuse (n_angles != 6) and grad_cols_kernel<1, 0> run with the run-time count; 12 at
    3240 x 24 and 5 at 4320 x 32, heights with a radix above 16, whose plan choose_cols' ext_variant then does not choose.  In 21
    of these cases (er.gauges: exact_tie) theta, i_min and sigma are fixed by the grid; mags, interp and rho are not"""
    run_case(engines, case)


def test_direction_counts_in_turn_on_one_context(engines):
    """6, 12, 6, 1, 6 on one context: the weight cache keyed on (n_angles, n_interp) and the reused est.mags scratch (13 rows per
    image whatever the count) crossed in both directions"""
    by_id = {c.id: c for c in er.cases()}
    for cid in ("1x1x37x75_br", "a12_i30_1x1x37x75_br", "1x1x37x75_br", "a1_i30_1x1x37x75_br", "1x1x37x75_br",
                "2x1x1080x32_last_row+last_col", "a12_i64_1x1x1080x32_br", "2x1x1080x32_last_row+last_col", "a1_i7_1x1x1080x32_br",
                "2x1x1080x32_last_row+last_col"):
        run_case(engines, by_id[cid])


@pytest.mark.parametrize("case", _ids("mask"), ids=repr)
def test_saturation_mask(engines, case):
    """er.saturated on the scalar (37 x 75), vec2 (64 x 96), compiled narrow (1080 x 32), extended-radix (3240 x 24) and
    through-memory (8200 x 10) paths: without the mask every maximum sits on a pixel whose raw gray exceeds 0.99, a second
    structure sits at exactly float32(0.99) (`>`, not `>=`; the raw value, not the normalised one)"""
    run_case(engines, case)
    x, off = er.image(case), er.run(case, discard_saturation=False)
    check(case.id + " [mask off]", engines["default"].estimate_blur(x, opts(case, discard_saturation=False)), off, case, x)


@pytest.mark.parametrize("case", _ids("range"), ids=repr)
def test_gray_range(engines, case):
    """er.extremes: the minimum and the maximum at the first pixel, the last pixel, in the unpaired last row, in the last row pair.
    gray_rows_kernel: fp32 at 33 x 45 (45 = 9 x 5: two stages; a prime width such as 47 is Bluestein, which choose_rows
    refuses) with C = 1, 3 and a batch of 3 whose images have different ranges, 34 x 48 with C = 4; the compiled row plans at 33 x
    1920 and 33 x 3840 (and PB_ROWS_FIXED=0).  gray_minmax_kernel: the same fp32 cases on PB_EST_GRAY_ROWS=0, fp16 and u8 with HW %
    4 zero (34 x 48: VEC) and not (33 x 45), C = 1 and 3"""
    run_case(engines, case)


@pytest.mark.parametrize("case", _ids("chain"), ids=repr)
def test_scalar_chain(engines, case):
    """every theta index of er.ORIENTED (28 of 30: all but 1 and 29; 0 and 6 of 7; 0, 1, 31, 32, 63 of 64; blur directions on both
    sides of 90 degrees: the wrap), sigma and rho on each clamp and inside, force_theta_deg"""
    run_case(engines, case)


@pytest.mark.parametrize("case", _ids("quantile"), ids=repr)
def test_quantiles_of_quantised_images(engines, case):
    """heavy ties (at most 8 distinct values, one of them on 40 to 70 % of the pixels), negative values and values above 1, u8
    planes, HW below one histogram block (5 x 5, 5 x 7), a rank that is an integer (5 x 5, q = 0.25): gray_min / gray_max against the
    order statistics as test_gpu_parity.py::test_quantile_normalisation takes them, at its tolerance; the record against the
    float64 forward with the clip of normalize() acting"""
    x = er.image(case)
    info = engines["default"].estimate_blur(x, opts(case))
    flat = np.sort(er.gray32(x).reshape(1, -1), axis=1)
    n1 = F32(flat.shape[1] - 1)
    for qq, key in ((F32(case.opts["q"]), "gray_min"), (F32(1.0 - case.opts["q"]), "gray_max")):
        r = qq * n1
        f = np.floor(r)
        lo_i, hi_i = int(f), int(min(f + 1, n1))
        want = flat[:, lo_i] + F32(r - f) * (flat[:, hi_i] - flat[:, lo_i])
        print(case.id, key, info[key], want)
        assert np.max(np.abs(info[key] - want)) < 2e-7, (key, info[key], want)
    check(case.id, info, er.run(case), case, x)


def test_through_the_python_entry_points(engines):
    """one case per theme through gaussian_blur_estimation (kernel; sigma / rho / theta) and polyblur_deblurring(return_info=True)"""
    import torch
    from polyblur_amd import gaussian_blur_estimation, polyblur_deblurring
    by_id = {c.id: c for c in er.cases()}
    for cid in ("3x3x37x75_tl+last_col+last_row", "2x1x1080x32_last_row+last_col", "a12_i64_1x1x37x75_br", "a1_i7_1x1x64x96_br",
                "saturated_64x96", "extremes_3x3x33x45_float32_-1.-1", "oriented_i27_of_30", "clamp_high_sigma",
                "quantised_float32_97x131_q0.02"):
        case = by_id[cid]
        o, x, recs = case.opts, er.image(case), er.run(case)
        kw = dict(q=o["q"], n_angles=o["n_angles"], n_interpolated_angles=o["n_interp"], c=o["c"], b=o["b"], discard_saturation=o["discard_saturation"])
        kernel = np.asarray(gaussian_blur_estimation(x, **kw))
        sigma, rho, theta = (np.asarray(v).reshape(-1) for v in gaussian_blur_estimation(x, return_2d_filters=False, **kw))
        _, info = polyblur_deblurring(torch.from_numpy(x.copy()), n_iter=1, return_info=True, **kw)
        for bi, r in enumerate(recs):
            figures = (("kernel", er.err(kernel[bi, 0], r["kernel"], "kernel"), er.TOL_KERNEL), ("sigma", er.err(sigma[bi], r["sigma"], "sigma"), er.TOL["sigma"]),
                       ("rho", er.err(rho[bi], r["rho"], "rho"), er.TOL["rho"]),
                       ("mags", er.err(info[0]["mags"][bi], r["mags"], "mags"), er.TOL["mags"]),
                       ("interp", er.err(info[0]["interp"][bi], r["interp"], "interp"), er.TOL["interp"]),
                       ("sigma", er.err(info[0]["sigma"][bi], r["sigma"], "sigma"), er.TOL["sigma"]),
                       ("rho", er.err(info[0]["rho"][bi], r["rho"], "rho"), er.TOL["rho"]))
            print("%s image %d: %s" % (cid, bi, "  ".join("%s %.3g / %.3g" % f for f in figures)))
            assert all(f[1] <= f[2] for f in figures), (cid, bi, figures)
            assert F32(theta[bi]) == theta32(r) and F32(info[0]["theta"][bi]) == theta32(r) and int(info[0]["i_min"][bi]) == r["i_min"], cid
            if o["q"] == 0:
                g = er.gray32(x)[bi]
                assert F32(info[0]["lo"][bi]) == g.min() and F32(info[0]["hi"][bi]) == g.max(), cid
