"""GPU conformance sweep of the polynomial's window passes -- pairs of 64 x 64 windows (csrc/conv_wfft.hip: wave_pair), windows 64
wide and 128 tall (wave_tall), 128 x 128 windows (csrc/conv_w128.hip), and the merged launch that carries all three
(csrc/conv_win.hip) -- against a float64 evaluation of the same filter (tests/window_ref.py: reference64), over EVERY composite
halo pair csrc/khat.h can emit, on spectrally white input.

Everything goes through the C ABI with host-built records of caller taps (Engine.set_kernels + Engine.inverse_filter, full
support, wrap boundary; tests/window_ref.py: dial_taps gives the taps of any halo pair, with a margin no fp32 evaluation of the
halo rule can cross).  Six contexts: `pairs` (PB_POLY1=2, PB_POLY_TALL=0), `w128` (PB_POLY1=3, PB_POLY_TALL=0), `tall` (PB_POLY1=3,
PB_POLY_TALL=2), `three` (PB_POLY1=0: three Horner steps), and `w128_merged` / `tall_merged` (as `w128` / `tall` with
PB_POLY_ONE_LAUNCH=2: host-built records through conv_win_kernel with the exact grid, the branch of
pb_launch_conv_win that is handed the records' selections).  The cost model of csrc/khat.h decides which form an image takes in a context; the tests do not restate
it: they read the form from pb_body_selection (a 64 x 128 window reports as a 64 x 64 pair does: it is told by bits that differ
from a 64 x 64 run of the same image, or by a halo pair that leaves a 64 x 64 window no admissible tile), check whatever ran,
and the coverage tests assert that every halo value and every joint corner each form admits by csrc/common.h's constants was
reached -- less what REFUSED lists with its reason.

Tolerances.  fp32 planes: 5e-6 against clip(reference64) -- the bound of tests/test_gpu_onepass.py and
tests/test_gpu_tall_windows.py, now against float64 --, or 8 x the fp32 oracle's own distance from reference64 on the case where
that is larger (three transforms per axis in windows against one whole-image transform); 8e-6 against the three-step context.
fp16 planes: 6e-4 (tests/test_gpu_onepass.py).  The unclamped route: 5e-6 times the reference's peak magnitude.

Measured on MI355X (largest absolute difference against clip(reference64), every case below):
                       white input   geometry edges   impulses   alpha 2, beta 3   fp16 planes   unclamped / peak
  64 x 64 pairs          4.3e-7         4.1e-7         3.0e-7        6.2e-7          2.4e-4          3.5e-7
  64 x 128 windows       5.9e-7         4.3e-7         2.4e-7        8.7e-7            --              --
  128 x 128 windows      4.4e-7         3.9e-7         2.9e-7        8.3e-7          2.4e-4          3.7e-7
  three steps            7.7e-7 (the sweep's cases no one-pass form takes)
the batches of the merged launch 6.3e-7; any form against the three-step context 1.1e-6.  5e-6 held on every case: no case needed
the oracle's own distance.  The merged launch gave the bits and the selection of the separate launches on every case."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import window_ref as wr
from oracle import polyblur_ref as ref                      # the fp32 oracle: only where a case exceeds 5e-6 (E32)
from polyblur_amd import _capi as capi

TOL, TOL_FACTOR, TOL_THREE, TOL_FP16, TOL_DOMAIN = 5e-6, 8.0, 8e-6, 6e-4, 5e-6
COEF = (wr.ALPHA, wr.BETA)
COEF2 = (wr.ALPHA2, wr.BETA2)
CONTEXTS = {
    "pairs": dict(PB_POLY1=2, PB_POLY_TALL=0),
    "w128": dict(PB_POLY1=3, PB_POLY_TALL=0),
    "tall": dict(PB_POLY1=3, PB_POLY_TALL=2),
    "three": dict(PB_POLY1=0),
    "w128_merged": dict(PB_POLY1=3, PB_POLY_TALL=0, PB_POLY_ONE_LAUNCH=2),
    "tall_merged": dict(PB_POLY1=3, PB_POLY_TALL=2, PB_POLY_ONE_LAUNCH=2),
}
SWEEP_CONTEXTS = ("pairs", "tall", "w128")                  # (each named after the form its sweep shapes are cut for)
MERGED = {"w128": "w128_merged", "tall": "tall_merged"}

# What the cost model of csrc/khat.h gives to another form in every context that could run it -- (form, "hx" / "hy" / "corner",
# value) -> why --: not reached, and said here instead of silently dropped.
REFUSED = {
    # a 128 x 128 window pair is priced at 8 pairs of 64 x 64 windows (PB_POLY_COST128): 8 / (120 x 124) per sample against
    # 1 / (56 x 60) -- at the smallest halos the 64 x 64 pair (the 64 x 128 window where it is forced) is always cheaper
    ("w128", "corner", (4, 2)): "64 x 64 pairs keep 56 x 60 of 64 x 64: cheaper than 120 x 124 of a window priced at 8 pairs",
}
# ... and through the merged launch, which exists only where 128 x 128 windows are admitted (PB_POLY1=3): there a 64 x 64 pair
# whose tile is down to 16 or 20 rows, or to 768 samples, always costs more than the 128 x 128 window (1 / 768 against 8 / (88 x 96)
# at (20, 16)); these halos reach the 64 x 64 form in the `pairs` context only
REFUSED_MERGED = dict(REFUSED)
REFUSED_MERGED.update({("pairs", "hy", 22): "128 x 128 windows are cheaper", ("pairs", "hy", 24): "128 x 128 windows are cheaper",
                       ("pairs", "corner", (4, 24)): "128 x 128 windows are cheaper",
                       ("pairs", "corner", (8, 24)): "128 x 128 windows are cheaper",
                       ("pairs", "corner", (20, 16)): "128 x 128 windows are cheaper"})


def _engine(**env):
    """a context with these environment variables set (handled as tests/test_gpu_one_launch.py::_engine does)"""
    from polyblur_amd.engine import Engine
    old = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        os.environ[k] = str(v)
    try:
        return Engine(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def engines():
    e = {name: _engine(**env) for name, env in CONTEXTS.items()}
    yield e
    for eng in e.values():
        eng.close()


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


_figures = {}              # (form, what) -> the largest difference so far


def _note(form, what, d):
    _figures[(form, what)] = max(_figures.get((form, what), 0.0), d)


def _run(engines, ctx, x, keys, coef=COEF, profile=False):
    """x: (B, C, H, W); keys: the halo pair of each image's tap set -> (output, (B, 6) selection[, conv_fft launches])"""
    eng = engines[ctx]
    taps = np.stack([wr.taps_for(*k) for k in keys])
    # (the planes' buffers first: growing one frees the old one, and pb_free drops what the context knows about host-built records --
    # the call would still be right, but through the launches of records the host has not read)
    eng.buffer("np.in", x.nbytes)
    eng.buffer("np.out", x.nbytes)
    buf = eng.set_kernels(taps, name="conf%d.info" % len(keys))
    out = eng.inverse_filter(x, buf, coef[0], coef[1], capi.PB_WRAP)
    sel = eng.body_selection(len(keys))
    if not profile:
        return out, sel
    eng.profile_begin()
    again = eng.inverse_filter(x, buf, coef[0], coef[1], capi.PB_WRAP)
    launches = eng.profile_end()["conv_fft"][1]
    assert np.array_equal(out, again)
    return out, sel, launches


def _form(engines, ctx, x, key, out, sel, coef=COEF):
    """the form that ran image 0 of this one-image call: 'three', 'pairs', 'tall' or 'w128'"""
    poly = int(sel[0, 3])
    if poly != 1:
        return {0: "three", 2: "w128"}[poly]
    if not ctx.startswith("tall") or x.shape[2] < 128 or x.dtype != np.float32:
        return "pairs"                                      # (the context never takes 64 x 128 windows, or the plane does not admit them)
    h = tuple(int(v) for v in sel[0, 4:6])
    # poly == 1 in a context that takes 64 x 128 windows wherever they are admitted: a 64 x 64 run of the same image has other bits
    for other in ("pairs", "w128"):
        o, s = _run(engines, other, x, [key], coef)
        if s[0, 3] == 1:
            return "pairs" if np.array_equal(o, out) else "tall"
    # no context runs the image on 64 x 64 pairs: none can stand behind poly == 1 where the constants leave them no tile
    assert not wr.admits("pairs", *h), (ctx, key, h, "a 64 x 64 pass cannot be told from a 64 x 128 one here")
    return "tall"


def _bound(x, key, coef, want):
    """the case's bound where 5e-6 is exceeded: 8 x the fp32 oracle's own distance from the float64 reference, at least 5e-6"""
    k = np.stack([wr.taps_for(*kk) for kk in key])[:, None]
    e32 = maxabs(ref.inverse_filtering_rank3(x.astype(np.float32), k, coef[0], coef[1], method="fft"), want)
    return max(TOL, TOL_FACTOR * e32), e32


def _check(engines, ctx, kind, key, shape, coef=COEF, halos=None, what=None):
    """one image with the tap set `key` through `ctx`: the reported halos are the restated rule's, the output is within tolerance
    of clip(reference64) and within 8e-6 of the three-step context's.  -> (form, output, selection)"""
    halos = key if halos is None else halos
    x = wr.case_input(kind, key, shape)
    want = wr.case_reference(kind, key, shape, coef)
    got, sel = _run(engines, ctx, x, [key], coef)
    form = _form(engines, ctx, x, key, got, sel, coef)
    base, sel3 = _run(engines, "three", x, [key], coef)
    d, d3 = maxabs(got, want), maxabs(got, base)
    _note(form, what or kind, d)
    print("%s %s %s %s coef %s: form %s halos %s, reference64 %.3g, three steps %.3g (they against reference64 %.3g)"
          % (ctx, kind, key, shape, coef, form, sel[0, 4:6].tolist(), d, d3, maxabs(base, want)))
    assert (sel3[:, 3] == 0).all(), sel3
    if form != "three":                                     # (three steps report the kernel's own halos)
        assert tuple(sel[0, 4:6]) == tuple(halos), (ctx, key, sel, halos)
    tol = TOL
    if d >= TOL:
        tol, e32 = _bound(x, [key], coef, want)
        print("    above 5e-6: the fp32 oracle is %.3g from reference64, bound %.3g" % (e32, tol))
    assert d < tol, (ctx, kind, key, shape, form, d, tol)
    assert d3 < TOL_THREE, (ctx, kind, key, shape, form, d3)
    return form, got, sel


# ---------------------------------------------------------------------------------------------
# a. the halo sweep, b. the same cases through the merged launch, and what both reached
# ---------------------------------------------------------------------------------------------
_reached = {}              # (context, hx, hy) -> the form that ran the sweep's case
_swept = set()             # (context, hx) whose cases have all run


def _sweep(engines, ctx, hx):
    for _, hy, shape in wr.sweep_cases(ctx, hx):
        assert wr.composite_halos(wr.taps_for(hx, hy), *COEF)[0] == (hx, hy)
        form, _, _ = _check(engines, ctx, "flat", (hx, hy), shape)
        _reached[(ctx, hx, hy)] = form
    _swept.add((ctx, hx))


@pytest.mark.parametrize("hx", wr.HX)
@pytest.mark.parametrize("ctx", SWEEP_CONTEXTS)
def test_halo_sweep(engines, ctx, hx):
    """every row halo at one column halo: two tiles, a ragged third and a wrapping first window on both axes"""
    _sweep(engines, ctx, hx)


def _sweep_merged(engines, ctx, hx):
    for _, hy, shape in wr.sweep_cases(ctx, hx):
        key = (hx, hy)
        x = wr.case_input("flat", key, shape)
        got, sel = _run(engines, ctx, x, [key])
        if sel[0, 3] == 0:
            continue
        form = _form(engines, ctx, x, key, got, sel)
        merged, msel, launches = _run(engines, MERGED[ctx], x, [key], profile=True)
        assert np.array_equal(msel, sel), (ctx, key, sel, msel)
        assert np.array_equal(merged, got), (ctx, key, form, maxabs(merged, got))
        assert launches == 1, (ctx, key, launches)
        _reached[(MERGED[ctx], hx, hy)] = form
    _swept.add((MERGED[ctx], hx))


@pytest.mark.parametrize("hx", wr.HX)
@pytest.mark.parametrize("ctx", sorted(MERGED))
def test_halo_sweep_merged(engines, ctx, hx):
    """every case of the sweep that took a one-pass form, again through the merged launch: the same selection, the same bits, one
    launch of the conv_fft class"""
    _sweep_merged(engines, ctx, hx)


def _assert_covered(reached, refused, where):
    missing, wrongly = [], []
    for form in wr.FORMS:
        pairs = {h for h, f in reached if f == form}
        xs, ys = wr.admitted_values(form)
        found = {("hx", v): any(h[0] == v for h in pairs) for v in xs}
        found.update({("hy", v): any(h[1] == v for h in pairs) for v in ys})
        found.update({("corner", c): c in pairs for c in wr.corners(form)})
        missing += [(form,) + what for what, ok in found.items() if not ok and (form,) + what not in refused]
        wrongly += [(form,) + what for what, ok in found.items() if ok and (form,) + what in refused]
    assert not missing, (where, "not reached", missing)
    assert not wrongly, (where, "listed as refused, but reached", wrongly)


def test_sweep_reached_every_halo_of_every_form(engines):
    """over the three sweep contexts: each form ran at every halo value it admits on either axis and at its joint corners"""
    for ctx in SWEEP_CONTEXTS:
        for hx in wr.HX:
            if (ctx, hx) not in _swept:                     # (this test alone: the sweep has not run)
                _sweep(engines, ctx, hx)
    reached = [((hx, hy), f) for (ctx, hx, hy), f in _reached.items() if ctx in SWEEP_CONTEXTS]
    for form in wr.FORMS:
        print("sweep: form %s ran %d cases" % (form, sum(f == form for _, f in reached)))
    _assert_covered(reached, REFUSED, "the sweep")


def test_merged_launch_reached_every_halo_of_every_form(engines):
    """the same through the merged launch: the 64 x 64 and 128 x 128 forms in `w128_merged`, the 64 x 128 form in `tall_merged`"""
    for ctx in sorted(MERGED):
        for hx in wr.HX:
            if (MERGED[ctx], hx) not in _swept:             # (this test alone: the sweep has not run)
                _sweep_merged(engines, ctx, hx)
    reached = [((hx, hy), f) for (ctx, hx, hy), f in _reached.items() if ctx in MERGED.values()]
    for form in wr.FORMS:
        print("merged launch: form %s ran %d cases" % (form, sum(f == form for _, f in reached)))
    _assert_covered(reached, REFUSED_MERGED, "the merged launch")


# ---------------------------------------------------------------------------------------------
# b. controlled batches through the merged launch
# ---------------------------------------------------------------------------------------------
def _batch(engines, ctx, shape, keys):
    """a batch through a merged context: bit for bit the unmerged context's output and selection, one launch, every image
    within tolerance of clip(reference64) -> (output, selection)"""
    x = wr.flat_image(shape, wr.BATCH_SEED)
    want = np.clip(wr.reference64(x, np.stack([wr.taps_for(*k) for k in keys]), *COEF), 0.0, 1.0)
    base, sel0 = _run(engines, ctx, x, keys)
    got, sel, launches = _run(engines, MERGED[ctx], x, keys, profile=True)
    d = maxabs(got, want)
    _note("merged batch", "flat", d)
    print("merged batch %s in %s: (form, hx, hy) %s, reference64 %.3g, %d launch(es)" % (shape, ctx, sel[:, 3:6].tolist(), d, launches))
    assert np.array_equal(sel, sel0), (sel, sel0)
    assert (sel[:, 3] != 0).all() and sel[:, 4:6].tolist() == [list(k) for k in keys], sel
    assert np.array_equal(got, base), maxabs(got, base)
    assert launches == 1, launches
    tol = TOL if d < TOL else _bound(x, keys, COEF, want)[0]
    assert d < tol, (d, tol)
    return x, got, sel


@pytest.mark.parametrize("ctx", sorted(MERGED))
def test_merged_batch_of_three_forms(engines, ctx):
    """(3, 3, 200, 150): a halo pair only 128 x 128 windows admit, one only 64 x 128 and 128 x 128 windows admit, and a small one --
    128 x 128, 64 x 128, 64 x 128 windows in `tall_merged`, 128 x 128, 128 x 128 and 64 x 64 windows in `w128_merged`: the prefix sum over
    shares of different forms and halos.  Each image gets bit for bit what it gets alone."""
    shape, keys = wr.BATCHES[0]
    keys = list(keys)
    x, got, sel = _batch(engines, ctx, shape, keys)
    forms = []
    for b in range(3):
        alone, s1 = _run(engines, MERGED[ctx], x[b:b + 1], keys[b:b + 1])
        assert np.array_equal(s1[0], sel[b]), (b, s1, sel)
        assert np.array_equal(alone, got[b:b + 1]), (ctx, b, maxabs(alone, got[b:b + 1]))
        forms.append(_form(engines, MERGED[ctx], x[b:b + 1], keys[b], alone, s1))
    assert forms == (["w128", "tall", "tall"] if ctx == "tall" else ["w128", "w128", "pairs"]), forms


@pytest.mark.parametrize("ctx", sorted(MERGED))
def test_merged_batch_of_more_than_64_records(engines, ctx):
    """(70, 1, 72, 80), two records of different forms alternating: the second round of the prefix sum over 64 records"""
    shape, keys = wr.BATCHES[1]
    keys = list(keys)
    x, got, sel = _batch(engines, ctx, shape, keys)
    assert sel[:, 3].tolist() == [2, 1] * 35, sel[:, 3]
    for b in (0, 1, 63, 64, 65, 69):
        alone, _ = _run(engines, MERGED[ctx], x[b:b + 1], keys[b:b + 1])
        assert np.array_equal(alone, got[b:b + 1]), (ctx, b)


# ---------------------------------------------------------------------------------------------
# c. geometry edges, d. impulses
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,key", [(f, k) for f in wr.FORMS for k in wr.EDGE_HALOS[f]])
def test_geometry_edges(engines, form, key):
    """planes smaller than a window, of one tile exactly, one sample more or less, an odd number of tiles, every W mod 4, and one
    with a pair on the all-16-byte path -- in the context named after the form, which must be the form that runs"""
    for h, w in wr.edge_shapes(form, *key):
        got_form, _, _ = _check(engines, form, "flat", key, (1, h, w), what="edges")
        assert got_form == form, (form, key, (h, w), got_form)


@pytest.mark.parametrize("form", list(wr.FORMS))
def test_impulses(engines, form):
    """five impulses on a constant plane: the output is the filter's own response, replicated borders and wrap included"""
    key = wr.IMPULSE_HALOS[form]
    got_form, _, _ = _check(engines, form, "impulses", key, (1,) + wr.sweep_shape(form, *key))
    assert got_form == form, (form, key, got_form)


# ---------------------------------------------------------------------------------------------
# e. fp16 planes, f. the unclamped route, g. other coefficients
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", sorted(wr.FP16_HALOS))
def test_fp16_planes(engines, form):
    """fp16 in and out at the corners and the centre of the form's halo range, against reference64 of the fp16 input; the context
    that takes 64 x 128 windows must not take them for fp16 planes: the bits of the context that never does"""
    for key in wr.FP16_HALOS[form]:
        shape = (1,) + wr.sweep_shape(form, *key)
        x = wr.case_input("flat16", key, shape)
        want = wr.case_reference("flat16", key, shape)
        got, sel = _run(engines, form, x, [key])
        got_form = _form(engines, form, x, key, got, sel)
        d = maxabs(got, want)
        _note(got_form, "fp16", d)
        print("fp16 %s %s %s: form %s halos %s, reference64 %.3g" % (form, key, shape, got_form, sel[0, 4:6].tolist(), d))
        assert got.dtype == np.float16
        assert got_form == form or (form, "corner", key) in REFUSED, (form, key, got_form)
        if got_form != "three":
            assert tuple(sel[0, 4:6]) == key, (key, sel)
        assert d < TOL_FP16, (form, key, d)
        a, sa = _run(engines, "tall", x, [key])
        b, sb = _run(engines, "w128", x, [key])
        assert np.array_equal(sa, sb) and np.array_equal(a, b), (form, key, sa, sb)


@pytest.mark.parametrize("form", sorted(wr.DOMAIN_HALOS))
def test_unclamped_route(engines, form):
    """compute_polynomial on a plane that is the whole domain and spans [0.05, 0.95]: the window bodies without the clamp"""
    eng = engines[form]
    for key in wr.DOMAIN_HALOS[form]:
        shape = (1, 2) + wr.sweep_shape(form, *key)
        x = (0.5 + np.random.default_rng(wr.case_seed(key, shape)).uniform(-0.45, 0.45, shape)).astype(np.float32)
        x[0, 0, 0, 0], x[0, 0, -1, -1] = 0.05, 0.95
        taps = wr.taps_for(*key)
        want = wr.reference64(x, taps[None], *COEF, domain=True)
        eng.buffer("np.in", x.nbytes)                       # (before the records, as in _run)
        eng.buffer("np.out", x.nbytes)
        ks = eng.set_taps(taps[None])
        try:
            got = eng.compute_polynomial_taps(x, ks, COEF[0], COEF[1], capi.PB_WRAP, not_symmetric=False)
            sel = eng.body_selection(1)
        finally:
            ks.free()
        peak = float(np.max(np.abs(want)))
        d = maxabs(got, want)
        _note({1: "pairs", 2: "w128", 0: "three"}[int(sel[0, 3])], "unclamped / peak", d / peak)
        print("unclamped %s %s %s: selection %s, reference64 %.3g (peak %.3g, range [%.3f, %.3f])"
              % (form, key, shape, sel[0, 3:6].tolist(), d, peak, want.min(), want.max()))
        assert want.min() < 0.0 and want.max() > 1.0, "the case must leave [0, 1] to say anything about the clamp"
        assert int(sel[0, 3]) == {"pairs": 1, "w128": 2}[form] and tuple(sel[0, 4:6]) == key, (form, key, sel)
        assert d < TOL_DOMAIN * peak, (form, key, d, peak)


@pytest.mark.parametrize("form", list(wr.FORMS))
def test_other_coefficients(engines, form):
    """the sweep's corners once more under alpha = 2, beta = 3 (a3 = 0): other spectra, and the halos of a composite of degree two"""
    for key in wr.corners(form):
        halos, shape = wr.coef2_case(form, key)
        _check(engines, form, "flat", key, shape, coef=COEF2, halos=halos, what="alpha 2, beta 3")


def test_figures():
    """(last in the file) the largest differences of this run, per form and input"""
    for (form, what), d in sorted(_figures.items()):
        print("largest difference: %-12s %-18s %.3g" % (form, what, d))
