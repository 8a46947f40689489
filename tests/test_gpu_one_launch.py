"""GPU checks of the one-launch window pass (csrc/conv_win.hip; env PB_POLY_ONE_LAUNCH).

A polynomial on device-built records (PolySpec.always == 1) used to issue two window launches, one per window form, each
skipping the other's images; conv_win_kernel carries both bodies, a workgroup of four waves running either one 128 x 128
window pair or four one-wave jobs of the 64-wide forms.  Same bodies, same jobs: every output bit and every body selection
must be those of the two launches (PB_POLY_ONE_LAUNCH=0).

Everything here is a whole call through the C ABI, so that the records are built on the device.  Every case runs through the
default context and through a PB_POLY_ONE_LAUNCH=0 context and asserts: identical output bits, identical body selections for
every iteration, the whole call against the NumPy oracle (2e-5 for fp32 and 1e-3 for fp16 planes, as
tests/test_gpu_onepass.py::test_whole_call; 8-bit planes as tests/test_gpu_parity.py::test_uint8_edge: no level off by more
than one, fewer than 2e-3 of them off at all), the launches of the conv_fft class (one per polynomial against two; the zero
boundary's ring steps on top in both contexts), and -- through the body selection -- that the case ran the window form it is
there for.  The 64 x 128 form is not visible in the selection (it reports as poly == 1): a case that is there for it also
asserts that its bits differ from those of a context that never takes the form (PB_POLY_TALL=0).

method='direct': (1, 3, 150, 200) is below the ring form's threshold (PB_ZERO_RING_MIN_PAIRS, 4096 three-step window pairs --
an image of some 13 M samples, whose oracle takes minutes), where the polynomial is three window steps in both contexts; the
same shape runs the ring form -- the merged launch plus three ring steps -- in contexts whose threshold is lowered to 16."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import polyblur_ref as ref                      # the checker (tests only)
from polyblur_amd import _capi as capi
from polyblur_amd.synthetic import synthetic_blurry_image

KW = dict(c=0.362, b=0.468, alpha=6, beta=1)
TOL = {np.dtype(np.float32): 2e-5, np.dtype(np.float16): 1e-3}

# blurs (sigma, rho, theta deg) of the synthetic images.  What decides the form is what the estimation makes of them on these small,
# noisy images -- larger than the blur itself: (estimated sigma, rho) in the comments are the oracle's, iteration 1 / 2
WIDE = (3.5, 2.0, 30.0)           # 2.2 .. 3.3 / 1.7 .. 2.9: composite halos of 20 and more, 128 x 128 windows
MID = (1.66, 1.0, 66.0)           # 1.9 .. 2.5 / 1.5 .. 1.8 on these shapes: 128 x 128 windows too (halos 16 .. 24)
ROWS = (1.1, 0.5, 66.0)           # 1.46 / 0.85 and 1.22 / 0.64 near 66 degrees on (3, 130, 70): row halos of 12 and more, 64 x 128 windows
ROWS90 = (0.7, 0.4, 90.0)         # 1.2 .. 1.3 / 0.75 .. 0.86 at 66 .. 90 degrees: the same where the image is taller than wide
MILD = (0.8, 0.5, 20.0)           # 1.1 .. 1.4 / 0.8 .. 1.05 near 0 .. 30 degrees: halos (12 .. 16, 8 .. 12), 64 x 64 pairs where the tall form is out
SHARP = (0.3, 0.3, 0.0)           # 0.4 .. 0.8 / 0.3 .. 0.6: row halos of 8 and less, 64 x 64 pairs even where the tall form is admitted


def _engine(**env):
    """a context with these environment variables set (handled as tests/test_gpu_tall_windows.py::_engine does)"""
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
    e = {"merged": _engine(), "separate": _engine(PB_POLY_ONE_LAUNCH=0), "flat": _engine(PB_POLY_TALL=0),
         "merged_ring": _engine(PB_ZERO_RING_MIN_PAIRS=16), "separate_ring": _engine(PB_POLY_ONE_LAUNCH=0, PB_ZERO_RING_MIN_PAIRS=16)}
    yield e
    for eng in e.values():
        eng.close()


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


@functools.lru_cache(maxsize=None)
def _images(shape, blurs, dtype):
    B, C, H, W = shape
    x = np.stack([synthetic_blurry_image(C, H, W, 300 + b, blur=blurs[b % len(blurs)])[0] for b in range(B)])
    if dtype == np.uint8:
        x = ref.img_as_ubyte_from_float(x)
    x = np.ascontiguousarray(x.astype(dtype))
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _oracle(shape, blurs, dtype, n_iter, method, edgetaping):
    x = _images(shape, blurs, dtype)
    kw = dict(n_iter=n_iter, method=method, edgetaping=edgetaping, **KW)
    if dtype == np.uint8:
        want = np.stack([np.moveaxis(np.atleast_3d(ref.polyblur_deblurring_uint8(np.ascontiguousarray(np.moveaxis(im, 0, -1)), **kw)), -1, 0)
                         for im in x])
    else:
        want = ref.polyblur_deblurring(x.astype(np.float32), **kw)
    want.setflags(write=False)
    return want


def _call(eng, x, n_iter, method, edgetaping):
    """one unprofiled call (output, selections per iteration) and one profiled (launches of the conv_fft class; same bits)"""
    B = x.shape[0]
    o = eng.make_options(n_iter=n_iter, edgetaping=edgetaping, boundary=capi.PB_ZERO if method == "direct" else capi.PB_WRAP, **KW)
    out = eng.polyblur(x, o)
    sel = [eng.body_selection(B, it) for it in range(n_iter)]
    eng.profile_begin()
    again = eng.polyblur(x, o)
    launches = eng.profile_end()["conv_fft"][1]
    assert np.array_equal(out, again)
    return out, sel, launches


def _check(engines, shape, blurs, forms, dtype=np.float32, n_iter=2, method="fft", edgetaping=False, ring=False, three_steps=False):
    """forms: per image '128', 'tall' or 'pairs' -- the window form some iteration of that image must have run"""
    dtype = np.dtype(dtype).type
    x = _images(shape, blurs, dtype)
    B = shape[0]
    merged, separate = (engines["merged_ring"], engines["separate_ring"]) if ring else (engines["merged"], engines["separate"])
    got, sel, n_merged = _call(merged, x, n_iter, method, edgetaping)
    base, sel0, n_separate = _call(separate, x, n_iter, method, edgetaping)
    want = _oracle(shape, blurs, dtype, n_iter, method, edgetaping)
    print("one launch %s %s %s%s: (form, hx, hy) per iteration %s; conv_fft launches %d merged / %d separate"
          % (shape, np.dtype(dtype).name, method, " edgetaper" if edgetaping else "", [s[:, 3:6].tolist() for s in sel], n_merged, n_separate))
    if dtype == np.uint8:
        d = np.abs(got.astype(np.int32) - want.astype(np.int32))
        print("    against the oracle: %d levels at most, %.3g of the samples off" % (int(d.max()), float(np.mean(d != 0))))
    else:
        print("    against the oracle: %.3g" % maxabs(got, want))
    assert np.array_equal(got, base)
    for it in range(n_iter):
        assert np.array_equal(sel[it], sel0[it]), (it, sel[it], sel0[it])
    if dtype == np.uint8:
        assert d.max() <= 1 and np.mean(d != 0) < 2e-3, (int(d.max()), float(np.mean(d != 0)))
    else:
        assert maxabs(got, want) < TOL[np.dtype(dtype)], maxabs(got, want)
    if three_steps:
        # (the zero boundary below the ring threshold: three window steps per polynomial, whatever the knob)
        assert all((s[:, 3] == 0).all() for s in sel), sel
        assert n_merged == n_separate == 3 * n_iter, (n_merged, n_separate)
        return got
    extra = 3 * n_iter if ring else 0                       # (the ring steps of a zero-boundary polynomial)
    if not edgetaping:                                      # (an edgetaper's blends are launches of the class too, in both contexts)
        assert n_merged == n_iter + extra, n_merged
    assert n_separate - n_merged == n_iter, (n_merged, n_separate)
    # (a 64 x 128 window can stand behind poly == 1 only on fp32 planes of at least 128 rows under the wrap boundary)
    tall_possible = shape[2] >= 128 and dtype == np.float32 and method != "direct"
    never = _call(engines["flat"], x, n_iter, method, edgetaping)[0] if tall_possible else None
    for b in range(B):
        polys = [int(s[b, 3]) for s in sel]
        assert all(p in (1, 2) for p in polys), (b, polys)  # (the class: every image one window pass, every iteration)
        if forms[b] == "128":
            assert 2 in polys, (b, polys)
        elif forms[b] == "pairs":
            assert 1 in polys, (b, polys)
            assert not tall_possible or np.array_equal(got[b], never[b]), (b, polys)
        else:
            assert 1 in polys and tall_possible and not np.array_equal(got[b], never[b]), (b, polys)
    return got


def test_tall_one_window(engines):
    """64 x 128 form, one window that wraps on four sides: one job, three idle waves"""
    _check(engines, (1, 1, 128, 64), (ROWS90,), ["tall"])


def test_tall_ragged(engines):
    """64 x 128 form, ragged right and bottom; 3 planes of a few jobs: the last workgroup of a list has one to three live waves"""
    _check(engines, (1, 3, 130, 70), (ROWS,), ["tall"])


def test_pairs_fewer_than_128_rows(engines):
    """64 x 64 pairs (fewer than 128 rows: the tall form is not admitted)"""
    _check(engines, (1, 3, 100, 150), (MILD,), ["pairs"])


def test_pairs_one_job(engines):
    """64 x 64 pairs, one job, three idle waves"""
    _check(engines, (1, 1, 64, 64), (MILD,), ["pairs"])


def test_w128(engines):
    _check(engines, (1, 3, 200, 136), (WIDE,), ["128"])


def test_w128_one_window(engines):
    _check(engines, (1, 1, 128, 128), (WIDE,), ["128"])


def test_mixed_batch_and_alone(engines):
    """one image per form: the prefix sum in workgroup units, waves of one workgroup in different planes; and image 1 of the batch
    gets bit for bit what it gets alone"""
    shape, blurs = (3, 3, 200, 150), (WIDE, ROWS90, SHARP)
    got = _check(engines, shape, blurs, ["128", "tall", "pairs"])
    x = _images(shape, blurs, np.float32)
    eng = engines["merged"]
    alone = eng.polyblur(x[1:2], eng.make_options(n_iter=2, **KW))
    assert np.array_equal(alone, got[1:2])


def test_more_than_64_images(engines):
    """the prefix sum's second round of 64 records; blurs alternating between two forms"""
    _check(engines, (66, 1, 72, 80), (WIDE, SHARP), ["128", "pairs"] * 33, n_iter=1)


@pytest.mark.parametrize("dtype", [np.float16, np.uint8])
def test_narrow_planes(engines, dtype):
    """fp16 and 8-bit I/O: the tall form is not admitted, the loaders are per-sample"""
    _check(engines, (2, 3, 150, 200), (WIDE, MILD), ["128", "pairs"], dtype=dtype)


def test_direct_below_the_ring_threshold(engines):
    _check(engines, (1, 3, 150, 200), (MID,), ["pairs"], method="direct", three_steps=True)


@pytest.mark.parametrize("blur,form", [(MID, "128"), (MILD, "pairs")])
def test_direct_ring_form(engines, blur, form):
    """method='direct' in its window pass + border ring form: the interior's window pass through the merged launch, either form"""
    _check(engines, (1, 3, 150, 200), (blur,), [form], method="direct", ring=True)


def test_edgetaper_narrow_image(engines):
    """widths 65 - 80: the polynomial behind a blend reads the second set of spectra, and the merged grid is sized under that
    set's spec"""
    _check(engines, (1, 3, 68, 189), (MILD,), ["pairs"], edgetaping=True)
