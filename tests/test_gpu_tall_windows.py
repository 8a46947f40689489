"""GPU checks of the one-pass polynomial on windows 64 wide and 128 tall (csrc/conv_wfft.hip: wave_tall; csrc/khat.h: the
spectrum on the 64 x 128 grid and the choice; PolySpec.tall, env PB_POLY_TALL).

A wave holds one REAL window of 64 columns x 128 rows in the 64 complex registers per lane that otherwise hold a pair of
64 x 64 windows (rows 2 n and 2 n + 1 in register n, the real-input split behind the column transform), so the row halo is
paid once per job.  Everything goes through the C ABI with host-built records: one context that takes the form wherever it
is admitted (PB_POLY_TALL=2), one that never does (PB_POLY_TALL=0), checked against the NumPy oracle (reference:
deblurring.py:139-169, filters.py:33-36), against each other, image by image against the same image alone, and repeated.

Tolerances are those of tests/test_gpu_onepass.py::test_polynomial_against_oracle_and_three_steps for fp32: 5e-6 against the
oracle, 8e-6 between two forms.

Measured on MI355X over every shape and record below, before any bound was fixed (largest absolute difference): 8.9e-7
against the oracle (the other forms: 8.9e-7), 7.2e-7 against the 64 x 64 / 128 x 128 forms; the whole call 3.1e-6."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import polyblur_ref as ref                      # the checker (tests only)
from polyblur_amd import _capi as capi
from polyblur_amd.synthetic import synthetic_blurry_batch

ALPHA, BETA = 6.0, 1.0
TOL_ORACLE, TOL_FORMS = 5e-6, 8e-6


def _engine(tall):
    """a context with PB_POLY_TALL=tall (None: the variable unset -- the default context)"""
    from polyblur_amd.engine import Engine
    old = os.environ.get("PB_POLY_TALL")
    if tall is None:
        os.environ.pop("PB_POLY_TALL", None)
    else:
        os.environ["PB_POLY_TALL"] = str(tall)
    try:
        return Engine(0)
    finally:
        if old is None:
            os.environ.pop("PB_POLY_TALL", None)
        else:
            os.environ["PB_POLY_TALL"] = old


@pytest.fixture(scope="module")
def engines():
    tall, flat = _engine(2), _engine(0)
    yield tall, flat
    tall.close()
    flat.close()


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# (theta deg, sigma, rho) -> the composite filter's halos (x, y) under alpha = 6, beta = 1 (csrc/khat.h: the radius beyond which
# the composite's |tap| mass is < 1e-8): the smallest there are, the largest row halo the form admits (36, tiles of 56 rows),
# the largest column halo (20, tiles of 24 columns), and the headline's second and third estimates
RECORDS = [
    ((20.0, 0.3, 0.15), (4, 2)),
    ((10.0, 1.2, 4.0), (16, 36)),
    ((10.0, 1.7, 3.0), (20, 30)),
    ((66.0, 1.66, 1.01), (12, 16)),
    ((66.0, 1.24, 0.63), (8, 12)),
]
# one window that wraps on all four sides; ragged right and bottom, two tiles each way; two images with different records;
# the odd shape of tests/test_gpu_onepass.py
SHAPES = [(1, 1, 128, 64), (1, 1, 130, 70), (2, 3, 200, 150), (1, 3, 301, 517)]


@functools.lru_cache(maxsize=None)
def _image(shape):
    x, _ = synthetic_blurry_batch(*shape, seed0=23)
    x.setflags(write=False)
    return x


def _records_of(shape, i):
    """the records of a batch: image b gets record i + b (different records in one batch)"""
    return [RECORDS[(i + b) % len(RECORDS)] for b in range(shape[0])]


def _run(eng, x, recs, boundary=capi.PB_WRAP, name="np.info"):
    B = x.shape[0]
    sg = [r[0][1] for r in recs]
    rh = [r[0][2] for r in recs]
    th = [np.float32(np.deg2rad(r[0][0])) for r in recs]
    buf = eng.make_kernels(sg, rh, th, support=capi.PB_SUPPORT_FULL, name=name)
    info = eng.read_info(buf, B)
    out = eng.inverse_filter(x, buf, ALPHA, BETA, boundary)
    return out, eng.body_selection(B), info


_figures = {"oracle": 0.0, "forms": 0.0}


@pytest.mark.parametrize("shape", SHAPES)
def test_tall_against_oracle_and_flat(engines, shape):
    """the 64 x 128 form against the oracle (5e-6) and against the 64 x 64 / 128 x 128 forms (8e-6), with the selection it reports"""
    tall, flat = engines
    x = _image(shape)
    for i in range(len(RECORDS)):
        recs = _records_of(shape, i)
        got, sel, info = _run(tall, x, recs)
        base, sel0, _ = _run(flat, x, recs)
        want = ref.inverse_filtering_rank3(x, info["kernel"][:, None], ALPHA, BETA, method="fft")
        d_or, d_fl = maxabs(got, want), maxabs(got, base)
        _figures["oracle"] = max(_figures["oracle"], d_or)
        _figures["forms"] = max(_figures["forms"], d_fl)
        print("tall windows %s record %d: halos %s, oracle %.3g, other form %.3g (that form against the oracle %.3g; all so far %.3g / %.3g)"
              % (shape, i, sel[:, 4:6].tolist(), d_or, d_fl, maxabs(base, want), _figures["oracle"], _figures["forms"]))
        # a tall image is reported as a 64 x 64 one-pass image is, with the composite's halos -- those the other context reports
        assert (sel[:, 3] == 1).all() and (sel[:, 0] == 1).all(), sel
        assert (sel0[:, 3] >= 1).all(), sel0
        assert np.array_equal(sel[:, 4:6], sel0[:, 4:6]), (sel, sel0)
        assert sel[:, 4:6].tolist() == [list(r[1]) for r in recs], (recs, sel)
        # another form did run.  pb_body_selection does not show which: where the other context runs 64 x 64 windows the bits differ
        # from theirs; where it runs 128 x 128 windows the composite's row halo leaves a 64 x 64 window no tile (the model's
        # PB_POLY_MIN_TY = 16 rows), so no silent 64 x 64 pass can stand behind poly == 1
        assert not np.array_equal(got, base)
        for b in range(shape[0]):
            assert sel0[b, 3] == 1 or 64 - 2 * sel[b, 5] < 16, (sel, sel0)
        assert d_or < TOL_ORACLE, (shape, recs, d_or)
        assert d_fl < TOL_FORMS, (shape, recs, d_fl)


def test_alone_and_in_a_batch_and_repeated(engines):
    """every image of the two-image batch gets bit for bit what it gets alone, and ten repetitions give identical bits"""
    tall, _ = engines
    shape = SHAPES[2]
    x = _image(shape)
    for i in (0, 1, 3):
        recs = _records_of(shape, i)
        got, _, _ = _run(tall, x, recs)
        for b in range(shape[0]):
            alone, sel, _ = _run(tall, x[b:b + 1], recs[b:b + 1], name="one.info")
            assert sel[0, 3] == 1
            assert np.array_equal(alone, got[b:b + 1]), (i, b)
    recs = _records_of(shape, 3)
    first, _, _ = _run(tall, x, recs)
    for _ in range(9):
        again, _, _ = _run(tall, x, recs)
        assert np.array_equal(first, again)


def test_not_taken_for_fp16_planes_and_the_zero_boundary(engines):
    """narrower planes and method='direct' must not take the form: bit for bit what the PB_POLY_TALL=0 context gives"""
    tall, flat = engines
    shape = SHAPES[2]
    x = _image(shape)
    recs = _records_of(shape, 3)
    a, _, _ = _run(tall, x.astype(np.float16), recs)
    b, _, _ = _run(flat, x.astype(np.float16), recs)
    assert a.dtype == np.float16 and np.array_equal(a, b)
    a, _, _ = _run(tall, x, recs, boundary=capi.PB_ZERO)
    b, _, _ = _run(flat, x, recs, boundary=capi.PB_ZERO)
    assert np.array_equal(a, b)


def test_default_context_takes_the_form_where_the_model_prices_it_lowest(engines):
    """the default context (PB_POLY_TALL=1): the headline's second and third estimates, row halos 16 and 12, get the bits of the
    context that always takes the form; the smallest composite, row halo 2 -- a 64 x 64 pair keeps 2 x 60 of 64 rows --, the bits of
    the context that never does"""
    tall, flat = engines
    eng = _engine(None)
    try:
        x = _image(SHAPES[3])
        for i, taken in ((3, True), (4, True), (0, False)):
            got, sel, _ = _run(eng, x, [RECORDS[i]])
            want, _, _ = _run(tall if taken else flat, x, [RECORDS[i]])
            other, _, _ = _run(flat if taken else tall, x, [RECORDS[i]])
            assert sel[0, 3] == 1 and np.array_equal(got, want) and not np.array_equal(got, other), (i, sel)
    finally:
        eng.close()


def test_whole_call_default_context(engines):
    """one whole call through the default context (the cost model decides, records built on the device by the estimation's
    short chain) against the oracle; its second and third iteration (row halos of 10 and more) take the form: not the bits of the
    context that never does, and the bits of the one that always does from the iteration on where both run the same forms"""
    tall, flat = engines
    eng = _engine(None)
    try:
        x, _ = synthetic_blurry_batch(1, 3, 256, 320, seed0=17)
        kw = dict(n_iter=3, c=0.362, b=0.468, alpha=6, beta=1)
        got, info = eng.polyblur(x, eng.make_options(**kw), want_info=True)
        want, winfos = ref.polyblur_deblurring(x, return_info=True, **kw)
        assert [[float(t) for t in it["theta"]] for it in winfos] == info["theta"].tolist()
        d = maxabs(got, want)
        print("whole call (1, 3, 256, 320): %.3g against the oracle" % d)
        assert d < 2e-5, d
        never = flat.polyblur(x, flat.make_options(**kw))
        always, ainfo = tall.polyblur(x, tall.make_options(**kw), want_info=True)
        sel = [eng.body_selection(1, it)[0, 3:6].tolist() for it in range(3)]
        print("whole call: (form, hx, hy) per iteration %s; default == always: %s, default == never: %s"
              % (sel, np.array_equal(got, always), np.array_equal(got, never)))
        assert maxabs(always, want) < 2e-5 and np.array_equal(ainfo["theta"], info["theta"])
        assert any(s[0] == 1 and s[2] >= 10 for s in sel), sel      # (an iteration the model gives the form to ...)
        assert not np.array_equal(got, never)                       # (... and it ran there)
    finally:
        eng.close()
