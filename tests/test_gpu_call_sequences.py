"""A call's result does not depend on what its context did before.

What a reblurring pass wants of the spectra it meets -- the PolySpec, the slot of the selection scratch, the records the host
has read -- is an argument of the launchers (csrc/common.h: PassWant, Spectra), not state of the context that one call could
leave behind for the next.  This file pins the property from outside: one long-lived engine runs a sequence of calls chosen
so that each would go wrong on what its predecessor left (a one-pass spec, slots 0 and 1, a refused call that returns early, the
second set of spectra, the ring form, fp16 planes), and after every step the same call runs on a fresh engine with the same
environment, which is closed at once.  Equal: the output bits, body_selection(B, it) of every iteration of a pipeline call,
body_selection(B, -1), and the launches of the conv_fft class of a profiled repeat (as test_gpu_one_launch.py::_call counts them).

No oracle runs here: what the calls compute is checked in test_gpu_one_launch.py, test_gpu_onepass.py and test_gpu_parity.py.

What a fresh engine runs is the step's call with what that call needs -- for the steps on host-built records (3, 5, 8) the
make_kernels call that builds them.  The launches a call issues do depend on the HINTS a context keeps about such records (what
the host has read back of them: csrc/common.h, rec_cache), and pb_free drops every hint; the engine's upload / download buffers are
therefore sized for the largest image up front on every engine, so that no step frees one and both engines of a step hold the
same hints when its profiled repeat runs: those the step's own calls left.

Before the launchers took what they want as arguments, the library passed every comparison here but one: step 5's
body_selection(B, -1) was [1, 0, 0, 1, 12, 10] on the long-lived engine -- step 4's second-set selection, reported because
nothing cleared sel2_mask after a pipeline call -- against [1, 12, 0, 0, 8, 10] on the fresh one (csrc/conv_fft.hip:
pb_khat_buffers clears the slot's bit now).

At most three contexts are open at a time."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from polyblur_amd import _capi as capi
from polyblur_amd._capi import PolyblurHipError
from test_gpu_one_launch import KW, MID, MILD, _call, _engine, _images

SHAPE = (1, 3, 150, 200)
NARROW = (1, 3, 68, 189)
PAD = capi.PB_KSIZE // 2
LARGEST = 4 * SHAPE[1] * (SHAPE[2] + 2 * PAD) * (SHAPE[3] + 2 * PAD)        # bytes of step 5's padded fp32 image


def _fresh(**env):
    eng = _engine(**env)
    for name in ("np.in", "np.out"):
        eng.buffer(name, LARGEST)
    return eng


def _last(eng, B):
    """body_selection(B, -1), or None where the context holds no selection for B images"""
    try:
        return eng.body_selection(B, -1)
    except PolyblurHipError:
        return None


def _pipeline(eng, x, n_iter, method="fft", edgetaping=False):
    out, sel, launches = _call(eng, x, n_iter, method, edgetaping)
    return dict(out=out, sel=sel, last=_last(eng, x.shape[0]), launches=launches)


def _profiled(eng, call):
    eng.profile_begin()
    again = call()
    return again, eng.profile_end()["conv_fft"][1]


def _records(eng):
    s, r, t = MID
    return eng.make_kernels([s], [r], [np.deg2rad(t)])


def _inverse(eng, x, buf):
    """step 3 / 8: the polynomial on host-built records -- the call that reads their selections back, then the cached path"""
    call = lambda: eng.inverse_filter(x, buf, KW["alpha"], KW["beta"], capi.PB_WRAP)
    out = call()
    assert np.array_equal(out, call())
    last = _last(eng, x.shape[0])
    again, launches = _profiled(eng, call)
    assert np.array_equal(out, again)
    return dict(out=out, sel=[], last=last, launches=launches)


def _plain(eng, xp, buf):
    """step 5: single passes with the same records on a padded image"""
    conv = lambda: eng.convolve2d(xp, buf, capi.PB_WRAP)
    taper = lambda: eng.edgetaper(xp, buf, capi.PB_WRAP)
    a, b = conv(), taper()
    last = _last(eng, xp.shape[0])
    a2, na = _profiled(eng, conv)
    b2, nb = _profiled(eng, taper)
    assert np.array_equal(a, a2) and np.array_equal(b, b2)
    return dict(out=np.stack([a, b]), sel=[], last=last, launches=(na, nb))


def _same(step, long, fresh, failures):
    """every figure is printed before anything is asserted; the sequence goes on after a difference so that one run shows all"""
    bits = np.array_equal(long["out"], fresh["out"])
    sel = len(long["sel"]) == len(fresh["sel"]) and all(np.array_equal(a, b) for a, b in zip(long["sel"], fresh["sel"]))
    last = (long["last"] is None) == (fresh["last"] is None) and (long["last"] is None or np.array_equal(long["last"], fresh["last"]))
    launches = long["launches"] == fresh["launches"]
    print("step %s: bits %s; selections per iteration %s %s / %s; last selection %s %s / %s; conv_fft launches %s %s / %s"
          % (step, bits, sel, [s.tolist() for s in long["sel"]], [s.tolist() for s in fresh["sel"]],
             last, None if long["last"] is None else long["last"].tolist(), None if fresh["last"] is None else fresh["last"].tolist(),
             launches, long["launches"], fresh["launches"]))
    for name, ok in (("output bits", bits), ("body_selection(B, it)", sel), ("body_selection(B, -1)", last), ("conv_fft launches", launches)):
        if not ok:
            failures.append("step %s: %s differ between the long-lived and the fresh engine" % (step, name))


def test_results_do_not_depend_on_earlier_calls():
    x = _images(SHAPE, (MID,), np.float32)
    x16 = _images(SHAPE, (MID,), np.float16)
    narrow = _images(NARROW, (MILD,), np.float32)
    xp = np.pad(x, ((0, 0), (0, 0), (PAD, PAD), (PAD, PAD)), mode="edge")
    failures = []

    def against_fresh(step, long, run, **env):
        fresh = _fresh(**env)
        try:
            _same(step, long, run(fresh), failures)
        finally:
            fresh.close()

    eng, ring = _fresh(), _fresh(PB_ZERO_RING_MIN_PAIRS=16)
    try:
        # 1: the one-pass spec, slots 0 and 1
        step1 = lambda e: _pipeline(e, x, 2)
        against_fresh(1, step1(eng), step1)
        # 2: refused after the pipeline has begun (fp32 planes with half_temporaries): the refusal and nothing else
        with pytest.raises(PolyblurHipError, match="PB_ERR_UNSUPPORTED.*half_temporaries"):
            eng.polyblur(x, eng.make_options(n_iter=2, half_temporaries=True, **KW))
        # 3: host-built records, wrap: the read-back path of the polynomial, then the cached one
        buf = _records(eng)
        against_fresh(3, _inverse(eng, x, buf), lambda e: _inverse(e, x, _records(e)))
        # 4: behind an edgetaper on a narrow image: the estimation builds the second set, the merged grid is sized under its spec
        step4 = lambda e: _pipeline(e, narrow, 2, edgetaping=True)
        against_fresh(4, step4(eng), step4)
        # 5: plain passes with the records of step 3: the spectra of step 4 must not leak into them
        against_fresh(5, _plain(eng, xp, buf), lambda e: _plain(e, xp, _records(e)))
        # 6: the zero boundary's ring form (the second set as the ring's spectra), on a second long-lived engine that has run step 1
        step1(ring)
        step6 = lambda e: _pipeline(e, x, 2, method="direct")
        against_fresh(6, step6(ring), step6, PB_ZERO_RING_MIN_PAIRS=16)
        # 7: fp16 planes, one iteration
        step7 = lambda e: _pipeline(e, x16, 1)
        against_fresh(7, step7(eng), step7)
        # 8: step 3's call once more, on the records the long-lived engine has kept since
        against_fresh(8, _inverse(eng, x, buf), lambda e: _inverse(e, x, _records(e)))
    finally:
        eng.close()
        ring.close()
    assert not failures, failures
