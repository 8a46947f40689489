"""Operands at any element offset: every entry point of the engine against its aligned twin.

include/polyblur_hip.h asks of an image pointer that it be a device pointer to a contiguous NCHW array, and the front end hands
ROCm tensors to the engine in place (polyblur_amd/_frontend.py: staged; _autograd.py), storage offset included -- so an image cut
out of a pooled buffer, or batch[1:] of a float16 batch with C*H*W % 8 == 4, reaches the kernels at an address that is aligned
for its element type and for nothing more, while the kernels choose their 16-byte paths from pitches and sizes.

Every case here runs one entry point with its pointer operands carved out of poisoned buffers (tests/offset_operands.py): all at
offset 0 (the aligned twin), then each operand alone at each offset of its type (float32: 1 and 2 elements; float16: 1, 2 and 4;
8-bit: 1 and 2), then all operands together at different offsets.  Each run asserts
  (a) the result against the float64 / oracle reference of the entry point's own GPU test, under that test's tolerance;
  (b) the same bits as the twin (where a launcher's scalar path sums in another order, (a) alone: the case says so);
  (c) the poison around every operand, inputs included, untouched;
  (d) the inputs' own bits unchanged;
and, where the body selection shows it, that twin and case ran the same body.  The largest difference from the twin is printed
before anything is asserted.

What the MI355X run found (gfx950, ROCm 7): every 16-byte path is taken for an operand at an element offset exactly as for its
aligned twin -- the predicates look at pitches, and the body selections agree -- and serves the right samples:
  * plain vector loads and stores (pb_ld4 / pb_st4, float4, uint2): worked as is, 0 bits from the twin in every case;
  * buffer loads and stores (raw_buffer_load_b128 / b64 of the window bodies, float16 planes at 2-byte offsets included): worked
    as is, 0 bits;
  * LDS-DMA (global_load_lds of 16 bytes in the stencil body's interior tiles, raw_ptr_buffer_load_lds in the window bodies and
    the compiled column plans): worked as is, 0 bits.
No result was shifted, no guard was written, nothing faulted, and no launcher's predicate had to change.  The only differences
from a twin are the documented ones, where a launcher that looks at addresses takes a scalar kernel that sums in another order:
pb_halo_mask with gx or gy off a 16-byte boundary (grad_energy_kernel's partials): 5.96e-08; pb_halo_mask_backward with any
operand off (halo_grad.hip): 1.91e-06 on (1,3,32,48), 1.53e-05 on (1,1,96,128), gradients of up to some tens; the blind call's
gradient under remove_halo=True with the image off: 2.38e-07.  For those runs (a) alone is asserted.  csrc/conv_strip.hip is not in
the default library (tests/test_gpu_strip.py) and has no case here.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import polyblur_ref as ref                      # the checker (tests only)
from polyblur_amd import _capi as capi
from polyblur_amd.synthetic import synthetic_blurry_batch
from offset_operands import OFFSETS, bits, carve, guards_intact, poisoned

import autograd_ref as ar
import bilateral_grad_ref as bg
import halo_grad_ref as hg
import halo_ref as hr
import estimation_grad_ref as er
import test_gpu_autograd as ga
import test_gpu_blind_autograd as gb
import test_gpu_edge_aware as ea
import test_gpu_halo_autograd as gh
import test_gpu_nonblind as nb
import test_gpu_one_launch as ol
import test_gpu_phase as ph

F32, F16, U8 = torch.float32, torch.float16, torch.uint8
PB = {F32: capi.PB_F32, F16: capi.PB_F16, U8: capi.PB_U8}
NP = {F32: np.float32, F16: np.float16, U8: np.uint8}
BND = {"fft": capi.PB_WRAP, "direct": capi.PB_ZERO}
WORDS = capi.INFO_DTYPE.itemsize // 4                        # an estimation record in float32 words


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# ---------------------------------------------------------------------------------------------
# the engines: the default context, and the contexts whose knobs route a small shape through a form that has a threshold
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def engines():
    e = {"default": ol._engine(),
         "ring": ol._engine(PB_ZERO_RING_MIN_PAIRS=16),     # method='direct' as window pass + border ring on (1,3,150,200)
         "flat": ol._engine(PB_POLY_TALL=0),                # never the 64 x 128 window: what a 'tall' case must differ from
         "coop": ol._engine(PB_DT_COLS_COOP=2)}             # the few-columns column pass of the domain transform at any width
    yield e
    for eng in e.values():
        eng.close()


# ---------------------------------------------------------------------------------------------
# a case: named operands (inputs with their values, outputs poisoned), one call on their pointers, one check of the outputs
# ---------------------------------------------------------------------------------------------
class Case:
    """ins: name -> array; outs: name -> (shape, torch dtype); call(eng, ptrs) -> what shows which body ran (or None), after which
    the stream may still be busy; check(outs as arrays, that value) asserts (a); sums(offsets) -> True where the launcher's scalar
    path sums in another order than its vector path, so that the bits of twin and case may differ"""

    def __init__(self, ins, outs, call, check, engine="default", sums=None, differs_from=None):
        self.ins = {k: torch.from_numpy(np.array(v)) for k, v in ins.items()}       # (copies: the owners' arrays are read-only)
        self.outs, self.call, self.check, self.engine = outs, call, check, engine
        self.sums = sums or (lambda offs: False)
        self.differs_from = differs_from                     # an engine whose twin must give other bits (the 64 x 128 window)

    def operands(self):
        return [(k, v.dtype) for k, v in self.ins.items()] + [(k, dt) for k, (_, dt) in self.outs.items()]

    def plans(self):
        ops = self.operands()
        yield "twin", {}
        for name, dt in ops:
            for off in OFFSETS[dt]:
                yield "%s+%d" % (name, off), {name: off}
        # all together, neighbours at different offsets (the first input +1, the next operand +2, ...)
        yield "all", {name: OFFSETS[dt][i % len(OFFSETS[dt])] for i, (name, dt) in enumerate(ops)}

    def run(self, eng, offs):
        """-> (outputs as arrays, what call returned), after (c) and (d)"""
        held = {}
        for name, v in self.ins.items():
            held[name] = carve(v, offs.get(name, 0))
        for name, (shape, dt) in self.outs.items():
            held[name] = carve(poisoned(shape, dt), offs.get(name, 0))
        torch.cuda.synchronize()
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        seen = self.call(eng, {name: view.data_ptr() for name, (_, view) in held.items()})
        eng.synchronize()
        torch.cuda.synchronize()
        for name, (buffer, view) in held.items():
            assert guards_intact(buffer, view), "the poison around %r was written to" % name                      # (c)
        for name, v in self.ins.items():
            assert torch.equal(bits(held[name][1]).cpu(), bits(v)), "input %r was written to" % name             # (d)
        return {name: held[name][1].cpu().numpy() for name in self.outs}, seen


CASES = {}


def case(name, /, **kw):
    """register builder(**kw) under name: built when its test runs (the references are computed once and cached by their owners)"""
    def deco(builder):
        assert name not in CASES, name
        CASES[name] = functools.partial(builder, **kw)
        return builder
    return deco


def as_int(a):
    return a.view({4: np.int32, 2: np.int16, 1: np.uint8}[a.dtype.itemsize])


def twin_difference(got, twin):
    """largest |case - twin| over the outputs (inf where one side is not finite and the bits differ), and whether every bit agrees"""
    worst, same = 0.0, True
    for name in got:
        a, b = got[name], twin[name]
        if np.array_equal(as_int(a), as_int(b)):
            continue
        same = False
        d = np.abs(a.astype(np.float64) - b.astype(np.float64))
        worst = max(worst, float(np.max(np.where(np.isfinite(d), d, np.inf))))
    return worst, same


def run_case(engines, cid):
    c = CASES[cid]()
    eng = engines[c.engine]
    failures, twin, twin_seen = [], None, None
    for label, offs in c.plans():
        try:
            got, seen = c.run(eng, offs)
            if label == "twin":
                twin, twin_seen = got, seen
            worst, same = twin_difference(got, twin)
            print("%-40s %-14s largest difference from the twin %.3g%s" % (cid, label, worst, "" if same else "  (bits differ)"))
            c.check(got, seen)                                                                                    # (a)
            if not c.sums(offs):
                assert same, "bits differ from the aligned twin's, by up to %.3g" % worst                         # (b)
            assert seen == twin_seen, ("another body than the twin's", seen, twin_seen)
        except AssertionError as e:
            if label == "twin":
                raise
            failures.append("%s: %s" % (label, e))
    if c.differs_from is not None:
        other, _ = c.run(engines[c.differs_from], {})
        assert not twin_difference(other, twin)[1], "the form this case is there for was not taken"
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------
# pb_polyblur_batch: the blind pipeline, n_iter = 2 (shapes, blurs, oracle and tolerances: tests/test_gpu_one_launch.py)
# ---------------------------------------------------------------------------------------------
def _form_check(form, shape, dtype, want):
    def check(outs, sel):
        got = outs["out"]
        if dtype == U8:                                      # (tests/test_gpu_one_launch.py::_check: no level off by more than one)
            d = np.abs(got.astype(np.int32) - want().astype(np.int32))
            assert d.max() <= 1 and np.mean(d != 0) < 2e-3, (int(d.max()), float(np.mean(d != 0)))
        else:
            err = maxabs(got, want())
            assert err < ol.TOL[np.dtype(NP[dtype])], err
        polys = [p for it in sel for p in (row[3] for row in it)]
        if form == "128":
            assert 2 in polys, sel
        elif form in ("pairs", "tall"):
            assert 1 in polys, sel
        elif form == "steps":                                # (the zero boundary below the ring threshold: three window steps)
            assert all(p == 0 for p in polys), sel
    return check


def _polyblur(shape, blurs, dtype=F32, method="fft", edgetaping=False, form=None, engine="default"):
    x = ol._images(shape, blurs, NP[dtype])
    B = shape[0]

    def call(eng, p):
        o = eng.make_options(n_iter=2, edgetaping=edgetaping, boundary=BND[method], **ol.KW)
        eng.polyblur_ptr(p["in"], p["out"], PB[dtype], shape, o)
        eng.synchronize()
        return [eng.body_selection(B, it).tolist() for it in range(2)]

    want = lambda: ol._oracle(shape, blurs, NP[dtype], 2, method, edgetaping)
    return Case(dict(**{"in": x}), dict(out=(shape, dtype)), call, _form_check(form, shape, dtype, want), engine,
                differs_from="flat" if form == "tall" else None)


# conv_wfft_body.h:133,809,824 (the GEN window pair: in_pitch | wxA - lo, and the pair's stores): 64 x 64 pairs, three windows
# down and across, the middle ones interior
case("polyblur-pairs-interior", shape=(1, 3, 100, 152), blurs=(ol.MILD,), form="pairs")(_polyblur)
# conv_wfft_body.h:133: one 64 x 64 job that wraps on four sides
case("polyblur-pairs-one-job", shape=(1, 1, 64, 64), blurs=(ol.MILD,), form="pairs")(_polyblur)
# conv_w128_body.h:213,412: the 128 x 128 window, one window and several
case("polyblur-w128-one-window", shape=(1, 1, 128, 128), blurs=(ol.WIDE,), form="128")(_polyblur)
case("polyblur-w128", shape=(1, 3, 200, 136), blurs=(ol.WIDE,), form="128")(_polyblur)
# conv_wfft_body.h:631,725 (wave_tall: the 64 x 128 window's 16-byte column loads and stores)
case("polyblur-tall", shape=(1, 1, 128, 64), blurs=(ol.ROWS90,), form="tall")(_polyblur)
# conv_wave_common.h:281-326 (the fp16 windows' b64 pair, 8-bit planes per sample), conv_wfft_body.h:797
case("polyblur-fp16", shape=(2, 3, 150, 200), blurs=(ol.WIDE, ol.MILD), dtype=F16)(_polyblur)
case("polyblur-u8", shape=(2, 3, 150, 200), blurs=(ol.WIDE, ol.MILD), dtype=U8)(_polyblur)
# method='direct' below the ring threshold: three window steps per polynomial (conv_wfft_body.h:850, conv_common.h:63,98)
case("polyblur-direct-steps", shape=(1, 3, 150, 200), blurs=(ol.MID,), method="direct", form="steps")(_polyblur)
# the ring form (PB_ZERO_RING_MIN_PAIRS=16): the interior's window pass plus the border ring's steps, either window form
case("polyblur-direct-ring-pairs", shape=(1, 3, 150, 200), blurs=(ol.MILD,), method="direct", form="pairs", engine="ring")(_polyblur)
case("polyblur-direct-ring-128", shape=(1, 3, 150, 200), blurs=(ol.MID,), method="direct", form="128", engine="ring")(_polyblur)
# the edgetaper's blends before the polynomial (conv_tile_common.h:209: the epilogue's x operand and output)
case("polyblur-edgetaper", shape=(1, 3, 68, 192), blurs=(ol.MILD,), edgetaping=True)(_polyblur)
case("polyblur-edgetaper-direct", shape=(1, 3, 68, 192), blurs=(ol.MILD,), edgetaping=True, method="direct")(_polyblur)


@functools.lru_cache(maxsize=None)
def _halo_oracle(prefilter, method, half):
    x = hr.pipeline_image()
    if half:
        x = x.astype(np.float16)
    want = ref.polyblur_deblurring(x.astype(np.float32), prefiltering=True, prefilter=prefilter, method=method, **dict(hr.PIPE_KW, n_iter=2))
    want.setflags(write=False)
    return x, want


_PREFILTER = {"bilateral": capi.PB_PREFILTER_BILATERAL, "domain_transform": capi.PB_PREFILTER_DOMAIN_TRANSFORM,
              "normalized_convolution": capi.PB_PREFILTER_NORMALIZED_CONVOLUTION}


def _polyblur_halo(prefilter, method="fft", dtype=F32):
    """remove_halo=True, prefiltering=True on halo_ref's pipeline image (1,3,24,40), whose mask finds work (tests/test_gpu_halo.py::
    test_blind_pipeline_fp32; hr.TOL_PIPE / TOL_PIPE_HALF): filters.hip: pb_halo_apply (x, out and the recombination operands)
    and pb_grad_energy, and the prefilter's own launches (bilateral.hip, nc.hip; dt.hip: dt_cols_coop_kernel's 16-byte requests,
    which dt_choice.h: choose_dt grants to operands on 16-byte boundaries alone)"""
    x, want = _halo_oracle(prefilter, method, dtype == F16)
    shape = x.shape
    kw = dict(hr.PIPE_KW, n_iter=2)

    def call(eng, p):
        o = eng.make_options(prefilter=_PREFILTER[prefilter], boundary=BND[method], **kw)
        eng.polyblur_ptr(p["in"], p["out"], PB[dtype], shape, o)

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < (hr.TOL_PIPE_HALF if dtype == F16 else hr.TOL_PIPE), err

    return Case(dict(**{"in": x}), dict(out=(shape, dtype)), call, check)


for _p in _PREFILTER:
    case("polyblur-halo-%s" % _p, prefilter=_p)(_polyblur_halo)
case("polyblur-halo-bilateral-direct", prefilter="bilateral", method="direct")(_polyblur_halo)
case("polyblur-halo-domain_transform-fp16", prefilter="domain_transform", dtype=F16)(_polyblur_halo)


# ---------------------------------------------------------------------------------------------
# pb_estimate_blur (the oracle and the tolerances of tests/test_gpu_estimation_paths.py::
# test_extended_radix_plans_against_greedy_and_oracle and tests/test_gpu_parity.py::test_estimate_blur: 5e-6 on the magnitudes, 2e-5
# on sigma and rho)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _estimate_inputs(shape, dtype):
    x, _ = synthetic_blurry_batch(*shape, seed0=31)
    if dtype == U8:
        x = ref.img_as_ubyte_from_float(x)
        xf = ref.img_as_float32_from_ubyte(x)
    else:
        x = x.astype(NP[dtype])
        xf = x.astype(np.float32)
    _, r = ref.estimate_gaussian_blur(xf, c=0.362, b=0.468, return_info=True)
    return x, r


def _estimate(shape, dtype=F32):
    x, r = _estimate_inputs(shape, dtype)
    B = shape[0]

    def call(eng, p):
        eng.estimate_blur_ptr(p["in"], PB[dtype], shape, eng.make_options(c=0.362, b=0.468), p["rec"])

    def check(outs, seen):
        info = np.frombuffer(outs["rec"].tobytes(), capi.INFO_DTYPE)
        assert maxabs(info["mags"][:, :7], r["mags"]) < 5e-6, maxabs(info["mags"][:, :7], r["mags"])
        assert maxabs(info["sigma"], r["sigma"]) < 2e-5 and maxabs(info["rho"], r["rho"]) < 2e-5

    return Case(dict(**{"in": x}), dict(rec=((B, WORDS), F32)), call, check)


# estimate.hip:459 (the fused gray rows' vec = (W & 3) == 0) on a compiled row plan, the smallest being W = 512; three channels and one
case("estimate-rows512-c3", shape=(1, 3, 4, 512))(_estimate)
case("estimate-rows512-c1", shape=(1, 1, 3, 512))(_estimate)
# lines_fixed.hip:95-102 (a buffer resource on the planes, 16-byte LDS-DMA tiles): a compiled column plan, H = 512, W = 16
case("estimate-cols512", shape=(1, 1, 512, 16))(_estimate)
# a run-time-plan row and column (estimate.hip:459,700)
case("estimate-40x40", shape=(2, 3, 40, 40))(_estimate)
# estimate.hip:215 (gray_minmax_kernel<VEC>: pb_ld4 on the caller's image) -- float16 and 8-bit planes take the two-launch sequence
case("estimate-40x40-fp16", shape=(2, 3, 40, 40), dtype=F16)(_estimate)
case("estimate-40x40-u8", shape=(2, 3, 40, 40), dtype=U8)(_estimate)
case("estimate-rows512-fp16", shape=(1, 3, 4, 512), dtype=F16)(_estimate)
case("estimate-rows512-u8", shape=(1, 3, 4, 512), dtype=U8)(_estimate)
# a through-memory line (estimate.hip:1606)
case("estimate-8200", shape=(1, 1, 4, 8200))(_estimate)


# ---------------------------------------------------------------------------------------------
# pb_estimate_blur_backward (tests/test_gpu_blind_autograd.py::test_backward_alone_against_float64: er.TOL_EST)
# ---------------------------------------------------------------------------------------------
def _estimate_backward(cid):
    """estimate_grad.hip:435 ((HW & 3) == 0: the planes walked in 16-byte units): 'ties' (1,3,30,44) and 'saturated' (1,3,36,40)"""
    x, sat = gb.BACKWARD[cid]
    recs, w, want = gb.backward_reference(cid)
    shape, B = x.shape, x.shape[0]
    opts = dict(c=0.362, b=0.464, discard_saturation=sat)

    def call(eng, p):
        o = eng.make_options(**opts)
        eng.estimate_blur_ptr(p["in"], capi.PB_F32, shape, o, p["rec"])
        eng.estimate_blur_backward_ptr(p["in"], shape, o, p["rec"], p["gk"], None, 25, p["gin"])

    def check(outs, seen):
        err = er.per_image_error(outs["gin"], want)
        assert err <= er.TOL_EST, err

    return Case(dict(**{"in": x}, gk=w.reshape(B, 25, 25)), dict(rec=((B, WORDS), F32), gin=(shape, F32)), call, check)


case("estimate-backward-ties", cid="ties")(_estimate_backward)
case("estimate-backward-saturated", cid="saturated")(_estimate_backward)


# ---------------------------------------------------------------------------------------------
# pb_fourier_gradients and its backward
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _planes(shape):
    x = np.random.default_rng(7).random(shape, dtype=np.float32)
    rx, ry = ref.spectral_gradients(x)
    return x, rx, ry, max(1.0, float(np.abs(rx).max()), float(np.abs(ry).max()))


def _fourier(shape, tol=4e-6):
    """tests/test_gpu_parity.py::test_fourier_gradients_sizes (4e-6 x the largest gradient); through-memory lines:
    tests/test_gpu_long_lines.py::test_fourier_gradients_long_lines (6e-6 x)"""
    x, rx, ry, scale = _planes(shape)

    def call(eng, p):
        eng.fourier_gradients_ptr(p["in"], shape, p["gx"], p["gy"])

    def check(outs, seen):
        ex, ey = maxabs(outs["gx"], rx), maxabs(outs["gy"], ry)
        assert ex < tol * scale and ey < tol * scale, (ex, ey, scale)

    return Case(dict(**{"in": x}), dict(gx=(shape, F32), gy=(shape, F32)), call, check)


# estimate.hip:459: compiled row and column plans on planes of 512 (the caller's planes are the row kernel's input, its outputs the
# column kernel's)
case("fourier-512x512", shape=(1, 1, 512, 512))(_fourier)
case("fourier-cols512", shape=(1, 2, 512, 16))(_fourier)
# run-time plans
case("fourier-40x40", shape=(1, 2, 40, 40))(_fourier)
# a through-memory line, (1,1,4,8200) (estimate.hip:1606)
case("fourier-8200", shape=(1, 1, 4, 8200), tol=6e-6)(_fourier)


def _fourier_backward(shape):
    """tests/test_gpu_halo_autograd.py::test_fourier_gradients_backward_against_float64 (hg.TOL_FOURIER), both upstreams: the row
    and column kernels of estimate.hip:459,700 on the caller's two upstream planes, run-time plans"""
    ggx, ggy = hg.fourier_case(shape)
    want = hg.fourier_backward(ggx, ggy)

    def call(eng, p):
        eng.fourier_gradients_backward_ptr(p["ggx"], p["ggy"], shape, p["gin"])

    def check(outs, seen):
        err = hg.plane_error(outs["gin"], want)
        assert err <= hg.TOL_FOURIER, err

    return Case(dict(ggx=ggx, ggy=ggy), dict(gin=(shape, F32)), call, check)


case("fourier-backward-64x48", shape=(1, 1, 64, 48))(_fourier_backward)
case("fourier-backward-9x8", shape=(2, 1, 9, 8))(_fourier_backward)


# ---------------------------------------------------------------------------------------------
# caller taps: pb_convolve2d_taps, pb_edgetaper_taps, pb_compute_polynomial_taps, pb_inverse_filter_taps, pb_inverse_filter_phase_taps
# ---------------------------------------------------------------------------------------------
def _taps_of(k, B):
    """(kb,kc,kh,kw) -> the engine's (B', kh, kw) and whether the image goes in as B*C one-channel images (polyblur_amd/nonblind.py)"""
    kb, kc, kh, kw = k.shape
    return np.ascontiguousarray(np.broadcast_to(k, (B, kc, kh, kw))).reshape(B * kc, kh, kw), kc > 1


def _with_taps(k, B, fn):
    """call(eng, p) that owns a kernel set for the length of the call"""
    taps, planes = _taps_of(k, B)

    def call(eng, p):
        ks = eng.set_taps(taps)
        try:
            fn(eng, p, ks)
            eng.synchronize()
        finally:
            ks.free()
    return call, planes


def _conv_taps(cid):
    """pb_convolve2d_taps on a case of tests/autograd_ref.py (the image is the domain) against the float64 forward of
    tests/test_gpu_autograd.py::reference, at tests/test_gpu_nonblind.py's TOL_CONV.  The kernels are not point-symmetric: the
    stencil body (conv_tile_common.h:65-81,140-156: interior tiles by 16-byte LDS-DMA; :209 and conv_common.h:63,98: its epilogue)"""
    func, method, x, w, k = ga.CASES[cid]
    assert func == "convolve2d"
    want = ga.reference(cid)[0]
    call, planes = _with_taps(k, x.shape[0], lambda eng, p, ks: eng.convolve2d_taps_ptr(p["in"], p["out"], eshape, ks, BND[method]))
    B, C, H, W = x.shape
    eshape = (B * C, 1, H, W) if planes else x.shape

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < nb.TOL_CONV, err

    return Case(dict(**{"in": x}), dict(out=(x.shape, F32)), call, check)


for _c in ("7x7_planes_on_33x40-convolve2d-fft", "7x7_planes_on_33x40-convolve2d-direct", "3x5_broadcast_on_20x24-convolve2d-direct"):
    case("convolve2d-taps-" + _c, cid=_c)(_conv_taps)


def _conv_interior(method):
    """the same entry on (2,1,200,300), autograd_ref's '5x5_on_200x300': several workgroups with interior tiles
    (conv_tile_common.h:140-156), against the oracle's convolve2d at TOL_CONV (tests/test_gpu_nonblind.py::test_every_shape_against_oracle)"""
    x, w, k = ar.case_inputs(510, (2, 1, 200, 300), (2, 1, 5, 5))
    want = ref.convolve2d(x, k, method=method)
    call, _ = _with_taps(k, 2, lambda eng, p, ks: eng.convolve2d_taps_ptr(p["in"], p["out"], x.shape, ks, BND[method]))

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < nb.TOL_CONV, err

    return Case(dict(**{"in": x}), dict(out=(x.shape, F32)), call, check)


case("convolve2d-taps-interior-fft", method="fft")(_conv_interior)
case("convolve2d-taps-interior-direct", method="direct")(_conv_interior)


@functools.lru_cache(maxsize=None)
def _nonblind_image():
    x = nb.rescaled_batch(1, 3, 52, 72, 7400)                # (tests/test_gpu_nonblind.py's image is (1,3,50,70): rounded to W % 8 == 0)
    x.setflags(write=False)
    return x


def _edgetaper_taps(kshape, method):
    """pb_edgetaper_taps on the padded image against the oracle at TOL_TAPER (tests/test_gpu_nonblind.py::test_every_shape_against_oracle)"""
    k = nb.make_kernel(kshape, 7300 + 100 * kshape[0] + kshape[1])
    xp = ref.replicate_pad(_nonblind_image(), kshape[1] // 2)
    want = ref.edgetaper(xp, k, method=method)
    call, _ = _with_taps(k, 1, lambda eng, p, ks: eng.edgetaper_taps_ptr(p["in"], p["out"], xp.shape, ks, BND[method]))

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < nb.TOL_TAPER, err

    return Case(dict(**{"in": xp}), dict(out=(xp.shape, F32)), call, check)


case("edgetaper-taps-13x13-fft", kshape=(13, 13), method="fft")(_edgetaper_taps)         # (52 + 12) x (72 + 12): W % 4 == 0
case("edgetaper-taps-13x13-direct", kshape=(13, 13), method="direct")(_edgetaper_taps)


def _inverse_taps(kshape, method, dtype=F32, full=False):
    """pb_inverse_filter_taps (pad, [edgetaper], polynomial, crop, [mask], clamp) against the oracle at TOL_INV / TOL_HALF
    (tests/test_gpu_nonblind.py::test_every_shape_against_oracle, ::test_fp16_images); 49 x 49: the large-kernel pass (conv_big.hip)"""
    k = nb.make_kernel(kshape, 7300 + 100 * kshape[0] + kshape[1])
    x = _nonblind_image().astype(NP[dtype])
    want = nb.oracle_inverse(x.astype(np.float32), k, method, full)
    call, _ = _with_taps(k, 1, lambda eng, p, ks: eng.inverse_filter_taps_ptr(p["in"], p["out"], PB[dtype], x.shape, ks, nb.ALPHA, nb.BETA,
                                                                              BND[method], full, full))

    def check(outs, seen):
        nb.check_inverse(outs["out"].astype(np.float32), want, nb.TOL_HALF if dtype == F16 else nb.TOL_INV, "inverse_filter_taps")

    return Case(dict(**{"in": x}), dict(out=(x.shape, dtype)), call, check)


case("inverse-taps-13x13-fft", kshape=(13, 13), method="fft")(_inverse_taps)
case("inverse-taps-13x13-direct-full", kshape=(13, 13), method="direct", full=True)(_inverse_taps)
case("inverse-taps-13x13-fft-full-fp16", kshape=(13, 13), method="fft", dtype=F16, full=True)(_inverse_taps)
case("inverse-taps-49x49-fft", kshape=(49, 49), method="fft")(_inverse_taps)


def _polynomial_taps(cid):
    """pb_compute_polynomial_taps against the float64 forward of tests/test_gpu_autograd.py::reference at ga.TOL_FWD"""
    func, method, x, w, k = ga.CASES[cid]
    assert func == "polynomial"
    want = ga.reference(cid)[0]
    B, C, H, W = x.shape
    call, planes = _with_taps(k, B, lambda eng, p, ks: eng.compute_polynomial_taps_ptr(p["in"], p["out"], eshape, ks, ar.ALPHA, ar.BETA, BND[method]))
    eshape = (B * C, 1, H, W) if planes else x.shape

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < ga.TOL_FWD, err

    return Case(dict(**{"in": x}), dict(out=(x.shape, F32)), call, check)


for _c in ("5x5_on_200x300-polynomial-fft", "5x5_on_200x300-polynomial-direct", "25x25_on_64x64-polynomial-fft", "7x7_planes_on_33x40-polynomial-direct"):
    case("polynomial-taps-" + _c, cid=_c)(_polynomial_taps)


def _phase_taps(dtype=F32, full=False):
    """pb_inverse_filter_phase_taps against the restatement of tests/phase_ref.py at ph.TOL_INV / TOL_HALF
    (tests/test_gpu_phase.py::test_chain_against_restatement), on the non-blind image and a kernel that is not point-symmetric"""
    import phase_ref as pr
    k = nb.make_kernel((9, 9), 8100)
    x = _nonblind_image().astype(NP[dtype])
    want = pr.inverse_filtering_nonsymmetric(x.astype(np.float32), k, 2, 3, remove_halo=full, do_edgetaper=full)
    call, _ = _with_taps(k, 1, lambda eng, p, ks: eng.inverse_filter_phase_taps_ptr(p["in"], p["out"], PB[dtype], x.shape, ks, 2, 3, full, full))

    def check(outs, seen):
        ph.check(outs["out"].astype(np.float32), want, ph.TOL_HALF if dtype == F16 else ph.TOL_INV, "inverse_filter_phase_taps")

    return Case(dict(**{"in": x}), dict(out=(x.shape, dtype)), call, check)


case("phase-taps", )(_phase_taps)
case("phase-taps-full-fp16", dtype=F16, full=True)(_phase_taps)


# ---------------------------------------------------------------------------------------------
# the backward passes of the taps entries (tests/test_gpu_autograd.py: ga.check holds TOL_X per sample and ar.TOL_K per lag)
# ---------------------------------------------------------------------------------------------
def _taps_backward(cid):
    func, method, x, w, k = ga.CASES[cid]
    y, gx, gk, norm = ga.reference(cid)
    B, C, H, W = x.shape
    kb, kc, kh, kw = k.shape
    taps, planes = _taps_of(k, B)
    eshape = (B * C, 1, H, W) if planes else x.shape

    def call(eng, p):
        ks = eng.set_taps(taps)
        try:
            if func == "convolve2d":
                eng.convolve2d_taps_backward_ptr(p["x"], p["g"], p["gx"], p["gk"], eshape, ks, BND[method])
            else:
                eng.compute_polynomial_taps_backward_ptr(p["x"], p["g"], p["gx"], p["gk"], eshape, ks, ar.ALPHA, ar.BETA, BND[method])
            eng.synchronize()
        finally:
            ks.free()

    def check(outs, seen):
        g = outs["gk"].astype(np.float64).reshape(B, kc, kh, kw)
        g = g.sum(0, keepdims=True) if kb == 1 else g
        ga.check(cid, func, (y, outs["gx"], g), (y, gx, gk), norm, kw)

    return Case(dict(x=x, g=w), dict(gx=(x.shape, F32), gk=(taps.shape, F32)), call, check)


for _c in ("7x7_planes_on_33x40-convolve2d-fft", "3x5_broadcast_on_20x24-convolve2d-direct", "5x5_on_200x300-polynomial-fft",
           "5x5_on_200x300-polynomial-direct", "25x25_on_64x64-polynomial-direct"):
    case("taps-backward-" + _c, cid=_c)(_taps_backward)


def _tap_gradient(cid):
    """pb_tap_gradient alone (tests/test_gpu_autograd.py::test_tap_gradient_alone: ar.TOL_K per lag, normalised)"""
    method, x, w, k = ga.TAP_CASES[cid]
    B, C, H, W = x.shape
    kb, kc, kh, kw = k.shape
    want, norm = ar.lag(w, x, k.shape, method), ar.lag(np.abs(w), np.abs(x), k.shape, method)
    eshape = (B * C, 1, H, W) if kc > 1 else (B, C, H, W)

    def call(eng, p):
        eng.tap_gradient_ptr(p["u"], p["v"], eshape, kh, kw, BND[method], p["grad"])

    def check(outs, seen):
        g = outs["grad"].astype(np.float64).reshape(B, kc, kh, kw)
        g = g.sum(0, keepdims=True) if kb == 1 else g
        err = ar.normalised_error(g, want, norm)
        assert err <= ar.TOL_K, err

    return Case(dict(u=w, v=x), dict(grad=((eshape[0], kh, kw), F32)), call, check)


for _c in ("5x5_on_200x300-fft", "7x7_planes_on_33x40-direct", "25x25_on_64x64-fft"):
    case("tap-gradient-" + _c, cid=_c)(_tap_gradient)


# ---------------------------------------------------------------------------------------------
# pb_halo_mask and its backward
# ---------------------------------------------------------------------------------------------
def _halo_mask(shape):
    """each of its five pointers (tests/test_gpu_halo.py::test_stage: hr.TOL_STAGE against float64).  filters.hip: pb_grad_energy takes
    grad_energy_kernel's scalar form where gx or gy is off a 16-byte boundary, and its partial sums then add up in another order:
    for those runs (a) stands alone"""
    s = hr.stage_set(shape)

    def call(eng, p):
        eng.halo_mask_ptr(p["x"], p["y"], p["gx"], p["gy"], p["out"], shape)

    def check(outs, seen):
        err = maxabs(outs["out"], s["want"])
        assert err < hr.TOL_STAGE, err

    return Case(dict(x=s["x"], y=s["y32"], gx=s["gx"], gy=s["gy"]), dict(out=(shape, F32)), call, check,
                sums=lambda offs: bool(offs.get("gx") or offs.get("gy")))


case("halo-mask-32x48", shape=(1, 3, 32, 48))(_halo_mask)              # four samples per lane (filters.hip: pb_halo_apply)
case("halo-mask-96x128", shape=(1, 1, 96, 128))(_halo_mask)            # more than one block per plane in the energy sum


def _halo_mask_backward(shape):
    """tests/test_gpu_halo_autograd.py::test_stage_backward_against_float64 (hg.stage_tolerance).  halo_grad.hip:192,244 looks at
    every operand and takes its scalar kernels where one is off a 16-byte boundary; their plane sums add up in another order, so
    (a) stands alone for every run but the twin"""
    s = hg.repaired_set(shape)
    tol = hg.stage_tolerance(shape)

    def call(eng, p):
        eng.halo_mask_backward_ptr(p["x"], p["y"], p["gx"], p["gy"], p["g"], p["dx"], p["dy"], p["dgx"], p["dgy"], shape)

    def check(outs, seen):
        errs = {n: hg.plane_error(outs["d" + n], s["want"][n]) for n in hg.NAMES}
        assert all(np.isfinite(outs["d" + n]).all() for n in hg.NAMES)
        assert all(errs[n] <= tol[n] for n in hg.NAMES), errs

    return Case({n: s[n] for n in ("x", "y", "gx", "gy", "g")}, {"d" + n: (shape, F32) for n in hg.NAMES}, call, check,
                sums=lambda offs: bool(offs))


case("halo-mask-backward-32x48", shape=(1, 3, 32, 48))(_halo_mask_backward)
case("halo-mask-backward-96x128", shape=(1, 1, 96, 128))(_halo_mask_backward)


# ---------------------------------------------------------------------------------------------
# the edge-aware filters
# ---------------------------------------------------------------------------------------------
EDGE_SHAPE = (1, 2, 33, 136)                                 # tests/test_gpu_edge_aware.py's ragged (1,2,33,130), W rounded to a multiple of 8


def _bilateral(ksize, dtype=F32):
    """tests/test_gpu_edge_aware.py::test_bilateral_parity (the float64 restatement, the case's own bound) and ::test_float16_images
    (the oracle on the fp16 image, 1e-3); ksize 5 is filters.hip's 5 x 5 kernel, 7 bilateral.hip's.  Both stage a 64 x 16 tile with
    its halo sample by sample and store per sample: no 16-byte path of their own -- the cases hold the entry points to the contract"""
    x = ea.image(EDGE_SHAPE)

    def call(eng, p):
        eng.bilateral_ptr(p["in"], p["out"], PB[dtype], EDGE_SHAPE, ksize, 5.0, 0.1)

    if dtype == F16:
        x = x.astype(np.float16)
        want, bound = ref.bilateral_filter(x.astype(np.float32), ksize), 1e-3
    else:
        want, bound = ea.yardstick(EDGE_SHAPE, ksize, 5.0, 0.1)

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < bound, (err, bound)

    return Case(dict(**{"in": x}), dict(out=(EDGE_SHAPE, dtype)), call, check)


for _k in (5, 7):
    case("bilateral-k%d" % _k, ksize=_k)(_bilateral)
    case("bilateral-k%d-fp16" % _k, ksize=_k, dtype=F16)(_bilateral)


def _bilateral_backward(ksize):
    """tests/test_gpu_bilateral_autograd.py::test_backward_alone_against_float64 (bg.TOL_BILATERAL)"""
    cs = ((1, 2, 33, 132), ksize, bg.SIGMAS[0])              # bilateral_grad_ref.WIDE (1,2,33,130), W rounded to a multiple of 4
    shape, k, (ss, sc) = cs
    v, g = bg.case_inputs(shape, sc)
    want = bg.case_reference(cs)

    def call(eng, p):
        eng.bilateral_backward_ptr(p["v"], p["g"], p["gin"], shape, k, ss, sc)

    def check(outs, seen):
        assert np.isfinite(outs["gin"]).all()
        err = bg.case_error(outs["gin"], want)
        assert err <= bg.TOL_BILATERAL, err

    return Case(dict(v=v, g=g), dict(gin=(shape, F32)), call, check)


case("bilateral-backward-k5", ksize=5)(_bilateral_backward)
case("bilateral-backward-k7", ksize=7)(_bilateral_backward)


def _recursive(shape, dtype=F32, joint=False, engine="default", n=2):
    """pb_dt_recursive_filter against the oracle: 5e-6, float16 images 1e-3 (tests/test_gpu_edge_aware.py::test_recursive_filter,
    ::test_recursive_filter_joint_image).  C = 1 and 3 run the fused kernels (dt.hip: dt_filter_fused, in the forms dt_choice.h chooses), C = 4 the domain planes"""
    x = ea.image(shape, seed=17).astype(NP[dtype])
    j = ea.image(shape, seed=6).astype(NP[dtype]) if joint else None
    want = ref.recursive_filter(x.astype(np.float32), 6.0, 0.4, n, None if j is None else j.astype(np.float32))

    def call(eng, p):
        eng.dt_recursive_filter_ptr(p["in"], p.get("joint"), p["out"], PB[dtype], shape, 6.0, 0.4, n)

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < (1e-3 if dtype == F16 else 5e-6), err

    ins = dict(**{"in": x})
    if joint:
        ins["joint"] = j
    return Case(ins, dict(out=(shape, dtype)), call, check, engine)


for _sh, _n in (((1, 1, 33, 72), "c1"), ((2, 3, 21, 64), "c3"), ((1, 4, 21, 64), "c4")):
    for _dt, _t in ((F32, ""), (F16, "-fp16")):
        case("recursive-%s%s" % (_n, _t), shape=_sh, dtype=_dt)(_recursive)
        case("recursive-%s-joint%s" % (_n, _t), shape=_sh, dtype=_dt, joint=True)(_recursive)
        if _n != "c4":
            # dt.hip: dtc_dma16, dt_choice.h: choose_dt's aligned16 (dt_cols_coop_kernel, PB_DT_COLS_COOP=2: the column pass whose lanes fetch J by 16-byte LDS-DMA)
            case("recursive-%s-coop%s" % (_n, _t), shape=_sh, dtype=_dt, engine="coop")(_recursive)
            case("recursive-%s-coop-joint%s" % (_n, _t), shape=_sh, dtype=_dt, joint=True, engine="coop")(_recursive)


@functools.lru_cache(maxsize=None)
def _nc_reference(shape, half):
    x = ea.image(shape, seed=17)
    if half:
        x = x.astype(np.float16)
    return x, ref.normalized_convolution(x.astype(np.float32), 6.0, 0.4, 2)


def _normalized_convolution(shape, dtype=F32):
    """pb_dt_normalized_convolution (nc.hip) against the oracle at the golden's 1e-6 (tests/test_gpu_edge_aware.py::
    test_normalized_convolution_golden); float16 images 1e-3, the project's bound for them"""
    x, want = _nc_reference(shape, dtype == F16)

    def call(eng, p):
        eng.dt_normalized_convolution_ptr(p["in"], p["out"], PB[dtype], shape, 6.0, 0.4, 2)

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < (1e-3 if dtype == F16 else 1e-6), err

    return Case(dict(**{"in": x}), dict(out=(shape, dtype)), call, check)


case("normalized-convolution-c3", shape=(2, 3, 21, 64))(_normalized_convolution)
case("normalized-convolution-c1", shape=(1, 1, 33, 72))(_normalized_convolution)
case("normalized-convolution-c3-fp16", shape=(2, 3, 21, 64), dtype=F16)(_normalized_convolution)


# ---------------------------------------------------------------------------------------------
# the patch lattice: pb_extract_patches, pb_overlap_add (no GPU test of their own: tests/test_gpu_parity.py::test_patch_decomposition
# runs them inside the whole call; float64 restatements of oracle/polyblur_ref.py::patchwise_deblurring's two
# ends; both kernels copy or blend samples: float32 results within 1e-6 of float64 -- two roundings of values in [0, 1] and of a
# quotient of window sums --, float16 within half a step below 1, 2.5e-4, on top)
# ---------------------------------------------------------------------------------------------
def _lattice(shape):
    from polyblur_amd.deblurring import kaiser_window_periodic, patch_grid
    g = patch_grid(shape[2], shape[3], (32, 32), 0.25)
    return g, kaiser_window_periodic(g["ph"]).astype(np.float32), kaiser_window_periodic(g["pw"]).astype(np.float32)


def _padded(x, g):
    H, W = x.shape[-2:]
    return np.pad(x, ((0, 0), (0, 0), (g["pad_top"], g["new_h"] - H - g["pad_top"]), (g["pad_left"], g["new_w"] - W - g["pad_left"])), mode="edge")


def _extract(shape, dtype=F32):
    g, _, _ = _lattice(shape)
    x = ea.image(shape, seed=23).astype(NP[dtype])
    B, C = shape[:2]
    n_p = g["n_i"] * g["n_j"]
    xp = _padded(x, g)
    want = np.empty((n_p, B, C, g["ph"], g["pw"]), x.dtype)
    for i in range(g["n_i"]):
        for j in range(g["n_j"]):
            want[i * g["n_j"] + j] = xp[..., i * g["step_h"]:i * g["step_h"] + g["ph"], j * g["step_w"]:j * g["step_w"] + g["pw"]]
    want = want.reshape(n_p * B, C, g["ph"], g["pw"])

    def call(eng, p):
        eng.extract_patches_ptr(p["in"], p["patches"], PB[dtype], shape, g, 0, n_p)

    def check(outs, seen):
        assert np.array_equal(outs["patches"], want)         # (copies: exact)

    return Case(dict(**{"in": x}), dict(patches=(want.shape, dtype)), call, check)


def _overlap_add(shape, dtype=F32):
    g, wy, wx = _lattice(shape)
    B, C, H, W = shape
    n_p = g["n_i"] * g["n_j"]
    patches = ea.image((n_p * B, C, g["ph"], g["pw"]), seed=29).astype(NP[dtype])
    win = np.outer(wy.astype(np.float64), wx.astype(np.float64))
    n_h, n_w = g["new_h"], g["new_w"]
    acc, norm = np.zeros((B, C, n_h, n_w)), np.zeros((n_h, n_w))
    pv = patches.astype(np.float64).reshape(n_p, B, C, g["ph"], g["pw"])
    for i in range(g["n_i"]):
        for j in range(g["n_j"]):
            ys, xs = slice(i * g["step_h"], i * g["step_h"] + g["ph"]), slice(j * g["step_w"], j * g["step_w"] + g["pw"])
            acc[..., ys, xs] += pv[i * g["n_j"] + j] * win
            norm[ys, xs] += win
    want = np.clip(acc / (norm + 1e-8), 0, 1)[..., g["pad_top"]:g["pad_top"] + H, g["pad_left"]:g["pad_left"] + W]

    def call(eng, p):
        eng.overlap_add_ptr(p["patches"], p["out"], PB[dtype], shape, g, p["wy"], p["wx"])

    def check(outs, seen):
        err = maxabs(outs["out"], want)
        assert err < (1e-6 + (2.5e-4 if dtype == F16 else 0.0)), err

    return Case(dict(patches=patches, wy=wy, wx=wx), dict(out=(shape, dtype)), call, check)


for _dt, _t in ((F32, ""), (F16, "-fp16")):
    case("extract-patches" + _t, shape=(2, 3, 40, 72), dtype=_dt)(_extract)
    case("overlap-add" + _t, shape=(2, 3, 40, 72), dtype=_dt)(_overlap_add)


# ---------------------------------------------------------------------------------------------
# the table, one test per case
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(CASES))
def test_offsets(engines, cid):
    run_case(engines, cid)


# ---------------------------------------------------------------------------------------------
# the public functions: in-place use through the front end (polyblur_amd/_frontend.py::staged, _autograd.py)
# ---------------------------------------------------------------------------------------------
def _carved(values, offset, grad=False):
    buffer, view = carve(values, offset)
    if grad:
        view = view.detach().requires_grad_(True)            # (a leaf that shares the carved storage: its data_ptr is the view's)
    return buffer, view


def _public(fn, inputs, check, offsets=None):
    """fn(**tensors) on carved views of `inputs`: the twin, then each input at each offset, then all; (a) by `check`, (b), (c), (d)"""
    names = list(inputs)
    vals = {n: torch.from_numpy(np.array(v)) for n, v in inputs.items()}
    plans = [("twin", {})]
    for n in names:
        plans += [("%s+%d" % (n, off), {n: off}) for off in (offsets or OFFSETS[vals[n].dtype])]
    plans.append(("all", {n: OFFSETS[vals[n].dtype][i % len(OFFSETS[vals[n].dtype])] for i, n in enumerate(names)}))
    twin, failures = None, []
    for label, offs in plans:
        held = {n: carve(vals[n], offs.get(n, 0)) for n in names}
        out = fn(**{n: v for n, (_, v) in held.items()})
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        try:
            for n, (buffer, view) in held.items():
                assert guards_intact(buffer, view), "the poison around %r was written to" % n
                assert torch.equal(bits(view).cpu(), bits(vals[n])), "input %r was written to" % n
            if twin is None:
                twin = got
            worst, same = twin_difference(dict(out=got), dict(out=twin))
            print("%-14s largest difference from the twin %.3g" % (label, worst))
            check(got)
            assert same, "bits differ from the aligned twin's, by up to %.3g" % worst
        except AssertionError as e:
            if label == "twin":
                raise
            failures.append("%s: %s" % (label, e))
    assert not failures, "\n".join(failures)


def test_public_polyblur_deblurring():
    """polyblur_deblurring on a carved view: tests/test_gpu_one_launch.py's (1,3,100,150) at W = 152, its oracle and tolerance"""
    import polyblur_amd as pa
    shape, blurs = (1, 3, 100, 152), (ol.MILD,)
    want = ol._oracle(shape, blurs, np.float32, 2, "fft", False)
    _public(lambda img: pa.polyblur_deblurring(img, n_iter=2, **ol.KW), dict(img=ol._images(shape, blurs, np.float32)),
            lambda got: maxabs(got, want) < ol.TOL[np.dtype(np.float32)] or pytest.fail("against the oracle: %.3g" % maxabs(got, want)))


def test_public_bilateral_filter():
    import polyblur_amd as pa
    for ksize in (5, 7):
        want, bound = ea.yardstick(EDGE_SHAPE, ksize, 5.0, 0.1)
        _public(lambda img: pa.bilateral_filter(img, ksize), dict(img=ea.image(EDGE_SHAPE)),
                lambda got: maxabs(got, want) < bound or pytest.fail("against float64: %.3g (bound %.3g)" % (maxabs(got, want), bound)))


def test_public_recursive_filter_with_a_carved_joint_image():
    import polyblur_amd as pa
    shape = (2, 3, 21, 64)
    x, j = ea.image(shape, seed=17), ea.image(shape, seed=6)
    want = ref.recursive_filter(x, 6.0, 0.4, 2, j)
    _public(lambda img, joint: pa.recursive_filter(img, 6.0, 0.4, 2, joint_image=joint), dict(img=x, joint=j),
            lambda got: maxabs(got, want) < 5e-6 or pytest.fail("against the oracle: %.3g" % maxabs(got, want)))


def test_public_gaussian_blur_estimation():
    """tests/test_gpu_blind_autograd.py::test_forward_of_arrays_and_cpu_tensors_and_against_float64: gb.TOL_KERNEL per tap"""
    import polyblur_amd as pa
    x = er.blurred_noise(12, (2, 3, 40, 48))
    want = er.kernels(er.estimate(x))
    _public(lambda img: pa.gaussian_blur_estimation(img, q=0.0), dict(img=x),
            lambda got: maxabs(got, want) <= gb.TOL_KERNEL or pytest.fail("against float64: %.3g" % maxabs(got, want)))


def test_float16_batch_tail():
    """batch[1:] of a float16 (3,1,9,12) batch: C*H*W % 8 == 4, so the tail starts 8 bytes off a 16-byte boundary; against the same
    images in a tensor of their own"""
    import polyblur_amd as pa
    x = torch.from_numpy(ea.image((3, 1, 9, 12), seed=31).astype(np.float16)).cuda()
    assert x.data_ptr() % 256 == 0
    tail = x[1:]
    assert tail.is_contiguous() and tail.data_ptr() % 16 == 8
    own = tail.clone()
    assert own.data_ptr() % 256 == 0
    before = x.clone()
    for what, fn in (("polyblur_deblurring", lambda t: pa.polyblur_deblurring(t, n_iter=2, **ol.KW)),
                     ("bilateral_filter", lambda t: pa.bilateral_filter(t, 5)), ("bilateral_filter 7", lambda t: pa.bilateral_filter(t, 7)),
                     ("recursive_filter", lambda t: pa.recursive_filter(t, 6.0, 0.4, 2)),
                     ("normalized_convolution", lambda t: pa.normalized_convolution(t, 6.0, 0.4, 2)),
                     ("gaussian_blur_estimation", lambda t: pa.gaussian_blur_estimation(t, q=0.0))):
        a, b = fn(tail), fn(own)
        torch.cuda.synchronize()
        d = (a.float() - b.float()).abs().max().item()
        print("%-26s largest difference from the aligned copy %.3g" % (what, d))
        assert torch.equal(a, b), (what, d)
    assert torch.equal(bits(x), bits(before))
    want = ref.polyblur_deblurring(tail.float().cpu().numpy(), n_iter=2, **ol.KW)
    assert maxabs(pa.polyblur_deblurring(tail, n_iter=2, **ol.KW).float().cpu().numpy(), want) < ol.TOL[np.dtype(np.float16)]


def _backward_case(forward, x, w, check, sums=lambda ox, og: False):
    """one backward pass with a carved leaf and y.backward(gradient=<carved view>): the twin (offsets 0, 0), then the input and the
    upstream at +1 and +2 each, then both.  sums(ox, og): the backward sums in another order for these offsets, (a) stands alone"""
    twin, failures = None, []
    for label, ox, og in (("twin", 0, 0), ("x+1", 1, 0), ("x+2", 2, 0), ("g+1", 0, 1), ("g+2", 0, 2), ("all", 1, 2)):
        bx, xt = _carved(x, ox, grad=True)
        bgr, gt = carve(w, og)
        y = forward(xt)
        y.backward(gradient=gt)
        torch.cuda.synchronize()
        got = xt.grad.cpu().numpy()
        try:
            assert guards_intact(bx, xt.detach()) and guards_intact(bgr, gt), "the poison around an operand was written to"
            assert torch.equal(bits(xt.detach()).cpu(), bits(torch.as_tensor(x))) and torch.equal(bits(gt).cpu(), bits(torch.as_tensor(w)))
            if twin is None:
                twin = got
            worst, same = twin_difference(dict(g=got), dict(g=twin))
            print("%-6s largest difference of x.grad from the twin %.3g" % (label, worst))
            check(got)
            assert same or sums(ox, og), "bits differ from the aligned twin's, by up to %.3g" % worst
        except AssertionError as e:
            if label == "twin":
                raise
            failures.append("%s: %s" % (label, e))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("cid", ["7x7_planes_on_33x40-convolve2d-fft", "5x5_on_200x300-polynomial-direct"])
def test_public_backward_of_the_taps_functions(cid):
    """convolve2d / compute_polynomial under autograd (tests/test_gpu_autograd.py::test_gradients_against_float64: TOL_X per sample)"""
    func, method, x, w, k = ga.CASES[cid]
    _, gx, _, _ = ga.reference(cid)
    kt = torch.tensor(k, device="cuda")

    def check(got):
        ex = float(np.max(np.abs(got - gx) / ga.image_tolerance(func, got.shape, k.shape[-1])))
        assert ex <= 1.0, ex

    _backward_case(lambda xt: ga.engine_call(func, xt, kt, ar.ALPHA, ar.BETA, method), x, w, check)


def test_public_backward_of_bilateral_filter():
    import polyblur_amd as pa
    cs = ((1, 2, 33, 132), 7, bg.SIGMAS[0])
    v, g = bg.case_inputs(cs[0], cs[2][1])
    want = bg.case_reference(cs)

    def check(got):
        assert bg.case_error(got, want) <= bg.TOL_BILATERAL, bg.case_error(got, want)

    _backward_case(lambda xt: pa.bilateral_filter(xt, 7, *cs[2]), v, g, check)


def test_public_backward_of_polyblur_deblurring_with_remove_halo():
    """the blind call under grad with remove_halo=True on the golden's (2,3,20,24) case (tests/test_gpu_halo_autograd.py::
    test_blind_gradients_against_the_goldens_and_float64: the float64 gradient, hg.blind_tolerances per sample).  The image is an
    operand of pb_halo_mask_backward, whose launcher (halo_grad.hip:244) takes its scalar kernels for an image off a 16-byte
    boundary; their plane sums add up in another order, so for those runs (a) stands alone"""
    import polyblur_amd as pa
    c, x, w, _, r = gh.blind_reference("b00")
    want, tol, n_iter = r["want"], r["tol"], c["n_iter"]

    def check(got):
        e = float(np.max(np.abs(got - want) / tol))
        assert e <= 1.0, e

    _backward_case(lambda xt: pa.polyblur_deblurring(xt, **dict(hr.PIPE_KW, n_iter=n_iter)), x, w, check, sums=lambda ox, og: ox != 0)
