"""The plan pb_debug_poly_plan returns (csrc/poly_choice.h) is what runs.

For a handful of calls the launches of the `conv` class (the stencil kernel) and of the `conv_fft` class (the window kernels) of a
profiled repeat must be the counts of those classes in the plans the query returns for the call's passes and polynomials, with
prof_on set.  The facts are built here from what the test knows of the call: its spec (what api.hip: poly_spec gives these shapes and
options), boundary, fold, and -- for records the host built -- the flags and selections body_selection reports.  What it cannot know
(whether a side stream exists, what the first scratch set holds) is swept, and the set of plans must have one launch count.  A launch
op that carries the known selections issues nothing where no image of the batch is its kind (the window launchers size their grid
from the selections and leave on an empty one): counted as they count.

One more case reaches the side-stream form: PB_POLY_ALWAYS=0 on 16 three-channel 1000 x 1000 images is exactly 12288 stencil tiles.
A profiled run stays on one stream, so the unprofiled run takes the other form: its output must be bit-identical to the profiled
repeat's, and to the same call at PB_POLY1=0.  The images are smooth enough for the estimation to clamp sigma = rho = 4 -- rank-1
kernels whose composite no window admits, so that every image takes three stencil passes under either knob, the side stream's
launches are the ones that do the work, and the two knobs compute the same thing (an image that takes a one-pass form under
PB_POLY1=3 differs from its three steps under PB_POLY1=0 in the last place, by construction: 1.3e-6 on images blurred as MID).
With a temporary counter in the issuing loop the rest of the GPU suite (7046 polynomials, 4711 single passes) was seen to issue
56 plans with a fork, all of them the zero boundary's ring form, and none with stencil launches on the side stream: no other test
reaches this form."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from polyblur_amd import _capi as capi
from polyblur_amd.synthetic import synthetic_image
from test_gpu_one_launch import KW, MID, MILD, _engine, _images
from test_poly_choice_cpu import BASE, FORK, SCRATCH, STENCIL, W128, WAVE, WG, WIN, query

SHAPE = (1, 3, 150, 200)
NARROW = (1, 3, 68, 189)
PAD = capi.PB_KSIZE // 2
ONE_PASS = dict(on=3, always=1, fold=1)                       # the pipeline's polynomial on fp32 planes of these sizes
BLEND = dict(on=0, always=2)                                  # an edgetaper's blend in the pipeline (window form for every image)


def _launches(op, sel):
    """whether the launch op issues a kernel: with the known selections, only where some image is its kind"""
    kind, poly, known = op[0], op[2], op[5]
    if not known:
        return True
    use, one = sel[:, 0] != 0, sel[:, 3]
    if kind == W128:
        return bool(np.any(use & (one == 2)))
    if kind == WIN:
        return bool(np.any(use & (one != 0)))
    return bool(np.any(use & (one != 2) & ((poly == 2) | ((one != 0) == (poly != 0)))))       # (poly_match, conv_fft_common.h)


def _counts(lib, passes, sel=None):
    """(conv, conv_fft) launches of the call: the sum over its passes [(polynomial, facts)], one answer over the unknown facts"""
    total = np.zeros(2, int)
    for polynomial, known in passes:
        answers = set()
        for aux, (_, scratch) in itertools.product((0, 1), SCRATCH):
            plan = query(lib, polynomial, dict(BASE, prof_on=1, aux=aux, **scratch, **known))
            answers.add((sum(op[0] == STENCIL for op in plan), sum(op[0] in (WAVE, WG, W128, WIN) and _launches(op, sel) for op in plan)))
        assert len(answers) == 1, (polynomial, known, answers)
        total += np.array(answers.pop())
    return tuple(int(v) for v in total)


def _profiled(eng, call):
    eng.profile_begin()
    out = call()
    prof = eng.profile_end()
    return out, (prof["conv"][1], prof["conv_fft"][1])


def _records_facts(sel, on):
    use, strip = sel[:, 0] != 0, sel[:, 2] != 0
    return dict(have=1, ksel=int(on != 0), any_fft=int(use.any()), any_fft3=int((use & (sel[:, 3] == 0)).any()), any_other=int((~use).any()),
                any_strip=int((~use & strip).any()), any_tile=int((~use & ~strip).any()))


PIPELINE = {
    "fft": (dict(), SHAPE, MID, dict(), [(1, ONE_PASS)]),
    "direct_ring": (dict(PB_ZERO_RING_MIN_PAIRS=16), SHAPE, MID, dict(boundary=capi.PB_ZERO), [(1, dict(ONE_PASS, zero=1))]),
    "edgetaping": (dict(), NARROW, MILD, dict(edgetaping=True),
                   [(0, BLEND), (0, dict(BLEND, ring=5)), (0, dict(BLEND, ring=4)), (1, ONE_PASS)]),
    "poly_always_0": (dict(PB_POLY_ALWAYS=0), SHAPE, MID, dict(), [(1, dict(on=3, always=0, fold=1))]),
    "one_launch_0": (dict(PB_POLY_ONE_LAUNCH=0), SHAPE, MID, dict(), [(1, dict(ONE_PASS, poly_one_launch=0))]),
}


@pytest.mark.parametrize("name", list(PIPELINE))
def test_pipeline_call(name):
    env, shape, blur, options, per_iteration = PIPELINE[name]
    x = _images(shape, (blur,), np.float32)
    eng = _engine(**env)
    try:
        o = eng.make_options(n_iter=2, **options, **KW)
        out = eng.polyblur(x, o)
        again, got = _profiled(eng, lambda: eng.polyblur(x, o))
        want = _counts(eng.lib, per_iteration * 2)
        print("%s: (conv, conv_fft) launches %s profiled, %s planned" % (name, got, want))
        assert np.array_equal(out, again)
        assert got == want
    finally:
        eng.close()


def test_stage_calls_on_host_built_records():
    x = _images(SHAPE, (MID,), np.float32)
    xp = np.pad(x, ((0, 0), (0, 0), (PAD, PAD), (PAD, PAD)), mode="edge")
    eng = _engine()
    try:
        # (pb_free drops what the context has read of host-built records: the upload / download buffers are sized for the padded
        # image up front, as tests/test_gpu_call_sequences.py does, so that no call below frees one)
        for name in ("np.in", "np.out"):
            eng.buffer(name, xp.nbytes)
        s, r, t = MID
        buf = eng.make_kernels([s], [r], [np.deg2rad(t)])
        inverse = lambda: eng.inverse_filter(x, buf, KW["alpha"], KW["beta"], capi.PB_WRAP)
        first, got_first = _profiled(eng, inverse)                    # (the call that reads the records' selections back)
        sel = eng.body_selection(1, -1)
        later, got_later = _profiled(eng, inverse)
        want = _counts(eng.lib, [(1, dict(on=3, always=0, fold=1, **_records_facts(sel, 3)))], sel)
        print("inverse_filter: selection %s; (conv, conv_fft) launches %s first, %s later, %s planned" % (sel.tolist(), got_first, got_later, want))
        assert np.array_equal(first, later)
        assert got_first == want and got_later == want
        conv, got_conv = _profiled(eng, lambda: eng.convolve2d(xp, buf, capi.PB_WRAP))
        plain = eng.body_selection(1, -1)
        taper, got_taper = _profiled(eng, lambda: eng.edgetaper(xp, buf, capi.PB_WRAP))
        one = [(0, dict(on=0, always=0, **_records_facts(plain, 0)))]
        want_conv, want_taper = _counts(eng.lib, one, plain), _counts(eng.lib, one * 3, plain)
        print("convolve2d: selection %s; launches %s, %s planned; edgetaper: %s, %s planned" % (plain.tolist(), got_conv, want_conv, got_taper, want_taper))
        assert got_conv == want_conv and got_taper == want_taper
    finally:
        eng.close()


def test_side_stream_form():
    B, C, H, W = 16, 3, 1000, 1000
    assert ((H + 2 * PAD + 63) // 64) * ((W + 2 * PAD + 63) // 64) * B * C == 12288
    # (an image so smooth that the estimation clamps sigma = rho = 4: a rank-1 kernel whose composite is too wide for one window pass,
    # so the three stencil launches -- the side stream's -- do the work, under PB_POLY1=0 as well: the two calls can be compared bit
    # for bit.  Images that take a one-pass form differ from their three steps in the last place: 1.3e-6 on MID-blurred ones)
    f = np.fft.fftfreq(H)
    smooth = np.exp(-2 * (np.pi * 8.0) ** 2 * (f[:, None] ** 2 + f[None, :] ** 2))
    one = np.fft.ifft2(np.fft.fft2(synthetic_image(C, H, W, np.random.default_rng(300))) * smooth).real.astype(np.float32)
    x = np.ascontiguousarray(np.stack([np.roll(one, (37 * b, 53 * b), axis=(1, 2)) for b in range(B)]))
    facts = dict(on=3, always=0, fold=1, side_tiles=1)
    eng = _engine(PB_POLY_ALWAYS=0)
    try:
        unprofiled = [query(eng.lib, 1, dict(BASE, aux=1, **scratch, **facts)) for _, scratch in SCRATCH]
        assert all(any(op[0] == FORK for op in plan) and sum(op[0] == STENCIL and op[4] == 1 for op in plan) == 3 for plan in unprofiled)
        o = eng.make_options(n_iter=1, **KW)
        out = eng.polyblur(x, o)
        sel = eng.body_selection(B, 0)
        again, got = _profiled(eng, lambda: eng.polyblur(x, o))
        want = _counts(eng.lib, [(1, facts)])
        assert not sel[:, 0].any(), sel.tolist()                     # (every image on the stencil body)
        print("side stream: (conv, conv_fft) launches %s profiled, %s planned" % (got, want))
        assert got == want
        assert np.array_equal(out, again)
    finally:
        eng.close()
    eng = _engine(PB_POLY_ALWAYS=0, PB_POLY1=0)
    try:
        steps = eng.polyblur(x, eng.make_options(n_iter=1, **KW))
        assert np.array_equal(eng.body_selection(B, 0)[:, :4], sel[:, :4])
    finally:
        eng.close()
    print("side stream: against PB_POLY1=0: %d samples differ, at most %.3g" % (int(np.sum(out != steps)), float(np.max(np.abs(out - steps)))))
    assert np.array_equal(out, steps)
