"""GPU conformance sweep of the per-step bodies of the reblurring pass -- the general 2-D stencil and the rank-1 body of
csrc/conv.hip, the workgroup form of the tile-spectrum body (csrc/conv_fft.hip) -- against a float64 evaluation of the same
operation (tests/stencil_ref.py), over directed cases: every tap position of every radius class (A), the structures of the
phase list only sparse lists reach (B), the rank-1 templates (C), dense point-symmetric sets per halo class (D), adaptive support
(E), and the geometry edges of both entry points and of the edgetaper blend.  tests/test_stencil_ref_cpu.py shows on the CPU
that the reference is right and that the cases can tell seven ways the bodies could be wrong.

Everything goes through the C ABI (Engine.set_kernels / make_kernels, convolve2d, inverse_filter, edgetaper).  Every case first
proves what ran: the record read back equals the restated rule (separable, radius, nphase, every descriptor, the filler and the
read-ahead slots, both tap layouts), and a profiled call shows the launches -- the stencil families run under
set_dense_eval("stencil"), where a pass is launches of the `conv` class only (three for pb_inverse_filter: no one-pass form);
family D and the tile-spectrum geometry rows on a second context created under PB_FFT_BODY=wg and set_dense_eval("auto", 0):
without that variable every per-step tile-spectrum pass goes to the wave form (csrc/conv_wfft.hip), which is not this file's
subject.  There pb_body_selection reports the tile-spectrum body and its halo class, the launches are of the `conv_fft` class,
and -- selection and launch class being the same for both forms -- the first case of every such test runs again on the default
context and must give other bits: the two forms round differently.

Tolerances.  General body through pb_convolve2d: per sample (N + 1) 2^-24 1.01 S + 1e-12, N the non-zero taps, S = |K| (*) |x| --
the forward bound of an fp32 sum of N products in any order.  Rank-1 body: the same with N = the non-zero taps of both marginals,
plus rho max|x|, rho = sum |k - ky (x) kx| of the record (asserted < 1e-6).  Adaptive support adds the dropped tap mass times
max|x|.  Tile-spectrum body, pb_inverse_filter and pb_edgetaper: 8 x the fp32 oracle's own distance from the float64 reference
on the case, at least 2e-6 / 5e-6 (against clip(reference)) / 4e-6.  fp16 planes: the input rounded to fp16 first, the fp32
tolerance plus half an fp16 ulp at the reference's value.

pb_convolve2d takes an already padded plane and refuses domains of 24 samples or fewer on a side (the reference's circular pad of
12 refuses them too), so the 8 x 9 domain of the CPU file cannot run here: the refusal is asserted, and the smallest domain both
entry points take, 26 x 27 (a 2 x 3 image for pb_inverse_filter), stands in for every body through pb_convolve2d, pb_inverse_filter
and pb_edgetaper -- a staged tile of 72 to 88 samples or a 64 x 64 window wraps round it three times.

Measured on MI355X (largest absolute difference against the float64 reference | the case's tolerance):
  A tap positions (1605 records x 2 boundaries)      4.2e-8   (per-sample bound about 1e-7)
  B phase lists                                      6.7e-7   (on the dense full lists, whose bound reaches 4e-5; sparse sets 4e-8)
  C rank-1 templates                                 3.7e-7
  D tile spectrum, workgroup form, classes 4 / 8 / 12  2.0e-7 | 2e-6   (1.2e-7 from the wave form's bits)
  E adaptive support                                 3.8e-7
  geometry, pb_convolve2d    general 1.0e-7, rank-1 1.9e-7, tile spectrum (workgroup form) 2.7e-7 | 2e-6
  geometry, pb_inverse_filter  general 3.4e-7, rank-1 7.9e-7, tile spectrum (workgroup form) 5.4e-7 | 5e-6; fp16 planes 2.44e-4 | 2.49e-4
  geometry, pb_edgetaper     general 1.7e-7, rank-1 9.0e-7, tile spectrum (workgroup form) 2.9e-7 | 4e-6
Every record equalled the restated rule, every tile-spectrum case gave other bits than the wave form, no case needed the oracle's
own distance, and no case exposed a fault in the bodies."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import stencil_ref as sr
import window_ref as wr
from oracle import polyblur_ref as ref
from polyblur_amd import _capi as capi
from polyblur_amd._capi import PolyblurHipError

assert (sr.WRAP, sr.ZERO, sr.FULL, sr.ADAPTIVE) == (capi.PB_WRAP, capi.PB_ZERO, capi.PB_SUPPORT_FULL, capi.PB_SUPPORT_ADAPTIVE)
BOUNDARIES = (sr.ZERO, sr.WRAP)
METHOD = {sr.ZERO: "direct", sr.WRAP: "fft"}
FLOOR_CONV, FLOOR_INVERSE, FLOOR_TAPER, TOL_FACTOR = 2e-6, 5e-6, 4e-6, 8.0
ALPHA, BETA = sr.GEOMETRY_COEF
LEAST_DOMAIN = (26, 27)                              # the smallest padded domain both entry points take (H = 2, W = 3)


@pytest.fixture(scope="module")
def eng():
    from polyblur_amd.engine import Engine
    e = Engine(0)
    yield e
    e.set_dense_eval("auto", capi.PB_DENSE_MIN_PHASES)
    e.close()


@pytest.fixture(scope="module")
def wg():
    """a context whose per-step tile-spectrum passes take the WORKGROUP form (csrc/conv_fft.hip): PB_FFT_BODY=wg, read when the
    context is created.  By default every such pass goes to the wave form (csrc/conv_wfft.hip), which is not this file's subject."""
    import os
    from polyblur_amd.engine import Engine
    old = os.environ.get("PB_FFT_BODY")
    os.environ["PB_FFT_BODY"] = "wg"
    try:
        e = Engine(0)
    finally:
        if old is None:
            os.environ.pop("PB_FFT_BODY", None)
        else:
            os.environ["PB_FFT_BODY"] = old
    yield e
    e.set_dense_eval("auto", capi.PB_DENSE_MIN_PHASES)
    e.close()


_figures = {}              # family -> (the largest difference, the tolerance it met)


def _note(family, d, tol):
    if family not in _figures or d > _figures[family][0]:
        _figures[family] = (d, tol)


def _mode(eng, spectrum):
    if spectrum:
        eng.set_dense_eval("auto", 0)                # every dense point-symmetric kernel through the tile-spectrum body
    else:
        eng.set_dense_eval("stencil")                # the stencil bodies, and no one-pass polynomial


# ---------------------------------------------------------------------------------------------
# what ran: the record against the restated rule, the launches against the body the case names
# ---------------------------------------------------------------------------------------------
def _check_records(info, support, taps=None):
    """every record read back equals stencil_ref.phase_list of its own taps -> [(separable, radius, nphase, phases)]"""
    out = []
    for b in range(info.shape[0]):
        k = info["kernel"][b]
        if taps is not None:
            assert np.array_equal(k, taps[b]), b
        sep, R, nphase, phases = sr.phase_list(k, support)
        got = (int(info["separable"][b]), int(info["radius"][b]), info["nphase"][b].tolist())
        assert got == (sep, R, nphase), (b, got, (sep, R, nphase))
        total = sum(nphase)
        want = sr.descriptors(R, phases)
        assert info["phase"][b][:total].tolist() == want, (b, [i for i in range(total) if info["phase"][b][i] != want[i]][:8])
        # (the three slots read ahead past the end: the first descriptor again, or 0 for an empty list)
        assert info["phase"][b][total:total + 3].tolist() == [want[0] if total else 0] * 3, b
        g = np.zeros((26, 33), np.float32)
        g[:25, 3:28] = k
        assert np.array_equal(info["gtaps"][b], g[:, :32]) and np.array_equal(info["gtaps_odd"][b], g[:, 1:]), b
        out.append((sep, R, nphase, phases))
    return out


def _records(eng, taps, support, x):
    """host-built records of caller taps; the planes' buffers first (growing one frees the old one, and pb_free drops what the
    context knows about host-built records) -> (buffer, the records read back, what phase_list says of each)"""
    eng.buffer("np.in", x.nbytes)
    eng.buffer("np.out", x.nbytes)
    buf = eng.set_kernels(taps, support, name="stencil%d.info" % taps.shape[0])
    info = eng.read_info(buf, taps.shape[0])
    return buf, info, _check_records(info, support, taps)


def _profiled(eng, call, spectrum, least=1):
    """call() between profile_begin and profile_end: launches of the stencil class only, or -- spectrum -- at least `least` of the
    tile-spectrum class (a stencil launch beside them finds every tile taken: the selection says by whom)"""
    eng.profile_begin()
    try:
        out = call()
    finally:
        prof = eng.profile_end()
    n_conv, n_fft = prof["conv"][1], prof["conv_fft"][1]
    # (in place of pb_body_selection's column 3 == 0 for the stencil families: under set_dense_eval("stencil") the context builds
    # no selection to read, and every window form -- a one-pass polynomial among them -- is a launch of the conv_fft class)
    if spectrum:
        assert n_fft >= least, (n_conv, n_fft)
    else:
        assert n_conv >= least and n_fft == 0, (n_conv, n_fft)
    return out


def _selection_is_spectrum(eng, B, classes):
    sel = eng.body_selection(B)
    assert (sel[:, 0] == 1).all() and sel[:, 1].tolist() == list(classes) and (sel[:, 3] == 0).all(), sel


def _is_not_the_wave_form(got, again):
    """the same call on the default context, whose tile-spectrum passes are the wave form's: the two forms round differently
    (csrc/conv_wfft.hip rotates the window rows and has per-axis halos), the selection, the launch class and the tolerance
    are the same -- what tells the workgroup form is that its bits are not the wave form's"""
    assert again.shape == got.shape and not np.array_equal(got, again), "the bits of the wave form: csrc/conv_fft.hip did not run"
    return maxabs(got, again)


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# ---------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------
def _closed_bound(info, rules, support, x, S):
    """the per-sample bound of the stencil bodies through pb_convolve2d: (B, 1, 1, 1)-shaped terms broadcast over S"""
    xmax = float(np.max(np.abs(x)))
    n, extra = [], []
    for b, (sep, R, _, phases) in enumerate(rules):
        k = info["kernel"][b].astype(np.float64)
        if sep:
            kx, ky = info["kx"][b].astype(np.float64), info["ky"][b].astype(np.float64)
            rho = float(np.abs(k - np.outer(ky, kx)).sum())
            assert rho < 1e-6, (b, rho)
            T = sr.rank1_template(R)
            box = np.zeros((25, 25), bool)
            box[12 - T:13 + T, 12 - T:13 + T] = True
            dropped = float(np.abs(k[~box]).sum())
            n.append(np.count_nonzero(kx) + np.count_nonzero(ky))
            extra.append((rho + dropped) * xmax)
        else:
            n.append(np.count_nonzero(k))
            extra.append(sr.dropped_mass(k, R, phases) * xmax)
        if (support & 15) == sr.FULL:
            assert extra[-1] == (rho * xmax if sep else 0.0), (b, extra[-1])
    shape = (-1, 1, 1, 1)
    return sr.sum_bound(np.array(n, np.float64).reshape(shape), S) + np.array(extra).reshape(shape)


def _assert_within(family, got, want, bound, what):
    d = np.abs(np.asarray(got, np.float64) - want)
    bound = np.broadcast_to(np.asarray(bound, np.float64), d.shape)
    top, worst = np.unravel_index(np.argmax(d), d.shape), np.unravel_index(np.argmax(d - bound), d.shape)
    print("%s %s: largest difference %.3g (tolerance there %.3g); closest to its tolerance at %s: %.3g of %.3g"
          % (family, what, d[top], bound[top], tuple(int(i) for i in worst), d[worst], bound[worst]))
    _note(family, float(d[top]), float(bound[top]))
    assert (d <= bound).all(), (family, what, worst, float(d[worst]), float(bound[worst]), int((d > bound).sum()))


def _oracle_bound(floor, e32):
    return max(floor, TOL_FACTOR * e32)


# ---------------------------------------------------------------------------------------------
# A. every tap position of every class; B. the structures of the phase list
# ---------------------------------------------------------------------------------------------
def _convolve_stencil(eng, family, x, taps, support, boundary, what):
    _mode(eng, False)
    buf, info, rules = _records(eng, taps, support, x)
    got = _profiled(eng, lambda: eng.convolve2d(x, buf, boundary), False)
    want, S = sr.correlate64(x, taps, boundary)
    _assert_within(family, got, want, _closed_bound(info, rules, support, x, S), what)
    return got, info, rules


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("R", sr.CLASSES)
def test_tap_positions(eng, R, boundary):
    """family A: 0.6 at (i, j) and 0.4 at the anchor that pins the class, for every (i, j) of the class's box, one plane each"""
    taps = sr.a_taps(R)
    _, info, rules = _convolve_stencil(eng, "A tap positions", sr.a_input(R), taps, sr.A_SUPPORT, boundary, "R %d boundary %d" % (R, boundary))
    assert len(rules) == (2 * R + 1) ** 2 and all(r[:2] == (0, R) for r in rules)


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("R", sr.CLASSES)
def test_phase_list_structures(eng, R, boundary):
    """family B: empty groups, odd and even groups, one live phase, a live phase in the last slot, the full list, no list"""
    cases = sr.b_cases(R)
    taps = np.stack([k for _, k, _ in cases])
    x = sr.white((len(cases),) + sr.B_SHAPE, 200 + R)
    got, info, rules = _convolve_stencil(eng, "B phase lists", x, taps, sr.B_SUPPORT, boundary, "R %d boundary %d" % (R, boundary))
    for (name, _, claimed), (sep, rad, nphase, _) in zip(cases, rules):
        assert sep == 0 and nphase == claimed and rad == (4 if name == "zero" else R), (name, sep, rad, nphase)
    if cases[-1][0] == "zero":
        assert not got[-1].any()                     # (nphase == 0: the epilogue of zero)


# ---------------------------------------------------------------------------------------------
# C. the rank-1 body
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_rank1_templates(eng, boundary):
    cases = sr.c_cases()
    taps = np.stack([c[1] for c in cases])
    x = sr.white((len(cases),) + sr.C_SHAPE, 300)
    _, info, rules = _convolve_stencil(eng, "C rank-1", x, taps, sr.FULL, boundary, "boundary %d" % boundary)
    for (name, _, sep, rad), rule in zip(cases, rules):
        assert rule[:2] == (sep, rad), (name, rule[:2])
    assert {sr.rank1_template(r[1]) for r in rules if r[0]} == set(sr.RANK1_CLASSES)


# ---------------------------------------------------------------------------------------------
# D. the tile-spectrum body
# ---------------------------------------------------------------------------------------------
def _spectrum_convolve(eng, family, x, taps, boundary, what, wave=None):
    """eng: the workgroup-form context; wave: the default context, where the case also proves which form ran"""
    _mode(eng, True)
    buf, info, rules = _records(eng, taps, sr.FULL, x)
    got = _profiled(eng, lambda: eng.convolve2d(x, buf, boundary), True)
    _selection_is_spectrum(eng, taps.shape[0], [r[1] for r in rules])
    if wave is not None:
        _mode(wave, True)
        wbuf, _, _ = _records(wave, taps, sr.FULL, x)
        print("%s %s: workgroup form against wave form %.3g" % (family, what, _is_not_the_wave_form(got, wave.convolve2d(x, wbuf, boundary))))
    want, _ = sr.correlate64(x, taps, boundary)
    d = maxabs(got, want)
    tol = FLOOR_CONV
    if d >= tol:
        tol = _oracle_bound(FLOOR_CONV, maxabs(ref.convolve2d(x, taps[:, None], method=METHOD[boundary]), want))
    _assert_within(family, got, want, tol, what)
    return got


@pytest.mark.parametrize("boundary", BOUNDARIES)
def test_tile_spectrum_classes(eng, wg, boundary):
    taps = np.stack([sr.d_taps(R) for R in sr.RANK1_CLASSES])
    x = sr.white((3,) + sr.D_SHAPE, 350)
    _spectrum_convolve(wg, "D tile spectrum", x, taps, boundary, "boundary %d" % boundary, wave=eng)


# ---------------------------------------------------------------------------------------------
# E. adaptive support
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("support", (sr.FULL, sr.ADAPTIVE))
def test_adaptive_support(eng, support, boundary):
    """the reference uses every tap; the tolerance gains the mass the policy drops, as the restated rule computes it"""
    _mode(eng, False)
    g = np.array(sr.E_GAUSSIANS, np.float32)
    x = sr.white((len(g) + len(sr.E_RINGS),) + sr.E_SHAPE, 400)
    eng.buffer("np.in", x.nbytes)
    eng.buffer("np.out", x.nbytes)
    gbuf = eng.make_kernels(g[:, 1], g[:, 2], np.deg2rad(g[:, 0]), support, name="stencilE.gauss")
    ginfo = eng.read_info(gbuf, len(g))
    # (one call: the Gaussians' taps as the device made them, then the two ring kernels)
    taps = np.concatenate([ginfo["kernel"], np.stack([sr.e_ring(v) for _, v in sr.E_RINGS])])
    for k in taps:
        assert sr.support_margin(k) >= 1.5, sr.support_margin(k)
    classes = [sr.phase_list(k, support)[1] for k in ginfo["kernel"]]
    other = [sr.phase_list(k, support ^ 1)[1] for k in ginfo["kernel"]]
    assert all(a != b for a, b in zip(classes, other)), (classes, other)
    grules = _check_records(ginfo, support)
    _, info, rules = _convolve_stencil(eng, "E adaptive support", x, taps, support, boundary, "support %d boundary %d" % (support, boundary))
    assert [r[:3] for r in rules[:len(g)]] == [r[:3] for r in grules]      # (pb_make_kernels and pb_set_kernels: one rule)
    kept, lost = sum(rules[-1][2]), sum(rules[-2][2])
    assert (kept > lost) if support == sr.ADAPTIVE else (kept == lost), (kept, lost)


# ---------------------------------------------------------------------------------------------
# geometry: both entry points and the edgetaper blend, B = 2, C = 3, different records per image
# ---------------------------------------------------------------------------------------------
def _geometry_setup(eng, body, R, x):
    spectrum = body == "spectrum"
    _mode(eng, spectrum)
    taps = sr.geometry_pair(body, R)
    buf, info, rules = _records(eng, taps, sr.geometry_support(body), x)
    assert [r[0] for r in rules] == [int(body == "rank1")] * 2 and rules[0][1] == R, (body, R, rules[0][:2], rules[1][:2])
    return spectrum, taps, buf, info, rules


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("body,R", sr.GEOMETRY_BODIES)
def test_geometry_convolve2d(eng, wg, body, R, boundary):
    """a real padded source, the whole domain written: one tile exactly, a ragged second row and column, a pitch no multiple of 4,
    exactly one interior tile and none, and the smallest domain (a tile or a window wraps round it three times)"""
    for n, domain in enumerate(sr.convolve_domains(R) + [LEAST_DOMAIN]):
        x = sr.white((2, 3) + domain, 1000 + R + domain[0])
        what = "%s R %d %s boundary %d" % (body, R, domain, boundary)
        if body == "spectrum":
            _spectrum_convolve(wg, "geometry convolve2d, tile spectrum", x, sr.geometry_pair(body, R), boundary, what, wave=None if n else eng)
        else:
            _convolve_stencil(eng, "geometry convolve2d, %s" % body, x, sr.geometry_pair(body, R), sr.geometry_support(body), boundary, what)


def test_the_small_domain_is_refused(eng):
    """pb_convolve2d and pb_edgetaper take padded planes: more than 24 samples on a side"""
    x = sr.white((1, 1) + sr.SMALL_DOMAIN, 3)
    buf = eng.set_kernels(sr.geometry_taps("general", 4)[None], sr.FULL | sr.FORCE_GENERAL, name="stencil1.info")
    for call in (eng.convolve2d, eng.edgetaper):
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
            call(x, buf, sr.WRAP)


LEAST_IMAGE = (LEAST_DOMAIN[0] - 2 * sr.PAD, LEAST_DOMAIN[1] - 2 * sr.PAD)      # 2 x 3: the image whose padded domain is LEAST_DOMAIN


def _inverse_cases(R):
    return [(s, np.float32) for s in sr.inverse_shapes(R) + [LEAST_IMAGE]] + [(s, np.float16) for s in sr.fp16_shapes(R) + [LEAST_IMAGE]]


@pytest.mark.parametrize("body,R,boundary", [(body, R, b) for body, R in sr.GEOMETRY_BODIES for b in BOUNDARIES
                                             if not (body == "spectrum" and b == sr.WRAP)])
def test_geometry_inverse_filter(eng, wg, body, R, boundary):
    """a virtual replicate pad, the cropped output, the Horner epilogue with the x operand, the clamp; fp32 planes on every shape,
    fp16 planes on the two smallest and the two largest, both on the 2 x 3 image.  (The tile-spectrum body under PB_WRAP would be
    the one-pass polynomial: it goes through pb_convolve2d there.)"""
    wave, eng = eng, (wg if body == "spectrum" else eng)
    for n, (shape, dtype) in enumerate(_inverse_cases(R)):
        x = (0.5 + 0.2 * (sr.white((2, 3) + shape, 2000 + R + shape[0], np.float64) - 0.5)).astype(dtype)
        spectrum, taps, buf, info, rules = _geometry_setup(eng, body, R, x)
        got = _profiled(eng, lambda: eng.inverse_filter(x, buf, ALPHA, BETA, boundary), spectrum, least=3)
        assert got.dtype == dtype
        if spectrum:
            _selection_is_spectrum(eng, 2, [r[1] for r in rules])
            if n == 0:
                _, _, wbuf, _, _ = _geometry_setup(wave, body, R, x)
                print("inverse_filter %s: workgroup form against wave form %.3g"
                      % (shape, _is_not_the_wave_form(got, wave.inverse_filter(x, wbuf, ALPHA, BETA, boundary))))
        raw = sr.inverse_filter64(x, taps, ALPHA, BETA, boundary)
        want = np.clip(raw, 0.0, 1.0)
        d = maxabs(got, want)
        half = sr.half_ulp16(want) if dtype == np.float16 else 0.0
        tol = FLOOR_INVERSE
        if (np.abs(got.astype(np.float64) - want) > tol + half).any():
            e32 = maxabs(ref.inverse_filtering_rank3(x.astype(np.float32), taps[:, None], ALPHA, BETA, method=METHOD[boundary]), want)
            tol = _oracle_bound(FLOOR_INVERSE, e32)
        clamped = float(np.mean((raw <= 0.0) | (raw >= 1.0)))
        # (the clamp decides few samples: the rest say something about the filter; of the 36 samples of the 2 x 3 image a share says little)
        assert clamped < 0.05 or shape == LEAST_IMAGE, clamped
        _assert_within("geometry inverse_filter, %s%s" % (body, ", fp16" if dtype == np.float16 else ""), got, want, tol + half,
                       "R %d %s boundary %d clamped %.3f" % (R, shape, boundary, clamped))


TAPER_BODIES = (("general", 10), ("rank1", 12), ("spectrum", 8))


@pytest.mark.parametrize("boundary", BOUNDARIES)
@pytest.mark.parametrize("body,R", TAPER_BODIES)
def test_geometry_edgetaper(eng, wg, body, R, boundary):
    """the blend epilogue: three blends with the weights of the record's own autocorrelations (on the smallest domain both ends
    of an axis weigh on every sample)"""
    import edgetaper_grad_ref as egr
    wave, eng = eng, (wg if body == "spectrum" else eng)
    for n, domain in enumerate(sr.convolve_domains(R) + [LEAST_DOMAIN]):
        x = sr.white((2, 3) + domain, 3000 + R + domain[0])
        spectrum, taps, buf, info, rules = _geometry_setup(eng, body, R, x)
        got = _profiled(eng, lambda: eng.edgetaper(x, buf, boundary), spectrum, least=3)
        if spectrum:
            _selection_is_spectrum(eng, 2, [r[1] for r in rules])
            if n == 0:
                _, _, wbuf, _, _ = _geometry_setup(wave, body, R, x)
                print("edgetaper %s: workgroup form against wave form %.3g" % (domain, _is_not_the_wave_form(got, wave.edgetaper(x, wbuf, boundary))))
        want = egr.forward(x, taps[:, None], METHOD[boundary], 3)
        tol = FLOOR_TAPER
        if maxabs(got, want) >= tol:
            tol = _oracle_bound(FLOOR_TAPER, maxabs(ref.edgetaper(x, taps[:, None], 3, METHOD[boundary]), want))
        _assert_within("geometry edgetaper, %s" % body, got, want, tol, "R %d %s boundary %d" % (R, domain, boundary))


def test_figures():
    """(last in the file) the largest differences of this run and the tolerances they met, per family"""
    for family, (d, tol) in sorted(_figures.items()):
        print("largest difference: %-44s %.3g | %.3g" % (family, d, tol))
