"""The edge-aware filters as public functions on the GPU: the bilateral filter of any odd window against the float64 restatement
(tests/filters_ref.py) with a bound worked out per case from the fp32 oracle's own error, the routing of ksize == 5, the three
kinds of operand, and recursive_filter / normalized_convolution / edge_aware_filtering against the oracle and the goldens.
Shapes are the smallest that can go wrong with a 64 x 16 tile and a radius of up to 12."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import polyblur_ref as ref                      # the checker (tests only)
import polyblur_amd as pa
import filters_ref as fr
from filters_ref import maxabs

SHAPES = [(1, 1, 2, 3),          # smaller than the radius: every tap is a clamped one
          (2, 3, 17, 65),        # one tile plus one row and one column, several planes
          (1, 2, 33, 130)]       # ragged tiles in both directions
WINDOWS = [(1, 5.0, 0.1), (3, 1.5, 0.02), (7, 5.0, 0.1), (13, 3.0, 0.05), (25, 5.0, 0.1), (25, 12.0, 0.5)]
WIDE = (1, 1, 33, 130)


@functools.lru_cache(maxsize=None)
def image(shape, seed=3):
    x = np.random.default_rng(seed).random(shape, dtype=np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def yardstick(shape, ksize, ss, sc):
    """(the float64 result, the parity bound of this very case: four times the fp32 oracle's own error, 3e-6 at least)"""
    x = image(shape)
    want = fr.bilateral_f64(x, ksize, ss, sc)
    want.setflags(write=False)
    return want, max(3e-6, 4 * maxabs(ref.bilateral_filter(x, ksize, ss, sc), want))


@pytest.fixture(scope="module")
def eng():
    from polyblur_amd.engine import get_engine
    return get_engine(0)


# ---------------------------------------------------------------------------------------------
# the bilateral filter
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ksize,ss,sc", WINDOWS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_bilateral_parity(shape, ksize, ss, sc):
    want, bound = yardstick(shape, ksize, ss, sc)
    got = pa.bilateral_filter(image(shape), ksize, ss, sc)
    err = maxabs(got, want)
    print("bilateral %r ksize %d sigma %g / %g: %.3g against a bound of %.3g" % (shape, ksize, ss, sc, err, bound))
    assert got.dtype == np.float32 and got.shape == shape
    assert err < bound, (err, bound)


def test_defaults_are_the_5x5_kernel_bit_for_bit(eng, golden):
    x = image((2, 3, 17, 65))
    got = pa.bilateral_filter(x)
    assert np.array_equal(got, eng.bilateral5(x))
    assert np.array_equal(got, pa.bilateral_filter(x, 5, 5.0, 0.1))
    g = golden("stages_A.npz")
    assert maxabs(pa.bilateral_filter(g["x"]), g["bilateral"]) < 3e-6


def test_abi_refuses_bad_arguments(eng):
    """pb_bilateral itself: PB_ERR_BADARG before any launch, the output untouched"""
    from polyblur_amd import _capi as capi
    x = torch.rand(1, 2, 8, 9, device="cuda")
    out = torch.full_like(x, -1.0)
    torch.cuda.synchronize()
    bad = [dict(ksize=0), dict(ksize=4), dict(ksize=27), dict(ksize=-3), dict(ss=0.0), dict(sc=-0.1), dict(sc=float("nan")), dict(ss=float("inf")),
           dict(sc=1e-30), dict(dtype=capi.PB_U8), dict(shape=(1, 2, 1, 9)), dict(shape=(0, 2, 8, 9)), dict(alias=True)]
    for kw in bad:
        with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):
            eng.bilateral_ptr(x.data_ptr(), x.data_ptr() if kw.get("alias") else out.data_ptr(), kw.get("dtype", capi.PB_F32),
                              kw.get("shape", x.shape), kw.get("ksize", 7), kw.get("ss", 5.0), kw.get("sc", 0.1))
    eng.synchronize()
    assert bool((out == -1.0).all())


def test_ksize_5_takes_the_callers_sigma():
    """the 5 x 5 kernel with sigma other than its defaults"""
    for ss, sc in ((1.0, 0.1), (5.0, 0.02), (0.7, 0.3)):
        want, bound = yardstick(WIDE, 5, ss, sc)
        assert maxabs(pa.bilateral_filter(image(WIDE), 5, ss, sc), want) < bound


@pytest.mark.parametrize("kw", [dict(ksize=7), dict(sigma_color=0.02), dict(sigma_spatial=1.0)], ids=lambda kw: "%s=%s" % next(iter(kw.items())))
def test_arguments_are_honoured(kw):
    """each moves the result away from the default one by more than ten parity bounds (the oracle alone shows it:
    tests/test_edge_aware_cpu.py::test_arguments_show_in_the_oracle)"""
    x = image(WIDE, seed=7)
    args = dict(dict(ksize=5, sigma_spatial=5.0, sigma_color=0.1), **kw)
    want = fr.bilateral_f64(x, **args)
    bound = max(3e-6, 4 * maxabs(ref.bilateral_filter(x, **args), want))
    got = pa.bilateral_filter(x, **kw)
    assert maxabs(got, want) < bound
    assert maxabs(got, pa.bilateral_filter(x)) > 10 * bound


def test_step_edge_is_kept():
    """what separates a bilateral filter from a blur: a step of 0.6 under sigma_color = 0.02 comes back as it went in (the 1e-5
    in the denominator included); with sigma_color = 1e3 the same window smears it.  The step sits on a tile boundary."""
    x = np.full((1, 1, 20, 130), 0.2, np.float32)
    x[..., 64:] = 0.8
    kept = pa.bilateral_filter(x, ksize=13, sigma_color=0.02)
    assert maxabs(kept, x) < 1e-5
    smeared = pa.bilateral_filter(x, ksize=13, sigma_color=1e3)
    assert np.abs(smeared - x)[..., 63:65].min() > 0.05
    assert maxabs(smeared[..., :58], x[..., :58]) < 1e-5 and maxabs(smeared[..., 71:], x[..., 71:]) < 1e-5


@pytest.mark.parametrize("ksize", [5, 7, 25])
def test_float16_images(ksize):
    xh = image((2, 3, 17, 65)).astype(np.float16)
    got = pa.bilateral_filter(xh, ksize)
    assert got.dtype == np.float16 and got.shape == xh.shape
    assert maxabs(got, ref.bilateral_filter(xh.astype(np.float32), ksize)) < 1e-3


@pytest.mark.parametrize("ksize", [5, 7])
def test_operand_kinds(ksize):
    x = image((1, 2, 33, 130))
    want = pa.bilateral_filter(x, ksize)
    assert isinstance(want, np.ndarray)
    on_cpu = pa.bilateral_filter(torch.from_numpy(x.copy()), ksize)
    assert isinstance(on_cpu, torch.Tensor) and on_cpu.device.type == "cpu" and on_cpu.dtype == torch.float32
    assert np.array_equal(on_cpu.numpy(), want)
    xg = torch.from_numpy(x.copy()).cuda()
    on_gpu = pa.bilateral_filter(xg, ksize)
    assert on_gpu.is_cuda and on_gpu.device == xg.device and on_gpu.dtype == torch.float32
    assert np.array_equal(on_gpu.cpu().numpy(), want)
    # a view with other strides: the result of its contiguous copy
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 1, 3, 2))).cuda().transpose(-1, -2)
    assert not xt.is_contiguous() and tuple(xt.shape) == x.shape
    assert np.array_equal(pa.bilateral_filter(xt, ksize).cpu().numpy(), want)
    # on a side stream, read on that stream
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = pa.bilateral_filter(xg, ksize)
        host = y.cpu()
    assert np.array_equal(host.numpy(), want)
    torch.cuda.current_stream().wait_stream(side)
    # half tensors keep their dtype; a tensor that requires grad runs under no_grad
    assert pa.bilateral_filter(xg.half(), ksize).dtype == torch.float16
    with torch.no_grad():
        assert np.array_equal(pa.bilateral_filter(xg.clone().requires_grad_(True), ksize).cpu().numpy(), want)


# ---------------------------------------------------------------------------------------------
# the domain transform
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("shape", [(1, 1, 33, 70), (1, 4, 21, 64), (3, 3, 2, 90)], ids=lambda s: "x".join(map(str, s)))
def test_recursive_filter(shape, n):
    x = image(shape, seed=17)
    want = ref.recursive_filter(x, 6.0, 0.4, n)
    assert maxabs(pa.recursive_filter(x, 6.0, 0.4, n), want) < 5e-6
    got = pa.recursive_filter(torch.from_numpy(x.copy()).cuda(), sigma_s=6.0, sigma_r=0.4, num_iterations=n)
    assert got.is_cuda and maxabs(got.cpu().numpy(), want) < 5e-6


def test_recursive_filter_joint_image():
    """the joint image goes in as the image's dtype whatever it comes as, for host and for device operands"""
    x, j = image((2, 3, 37, 203), seed=5), image((2, 3, 37, 203), seed=6)
    want = ref.recursive_filter(x, 8.0, 0.5, 2, j)
    assert maxabs(want, ref.recursive_filter(x, 8.0, 0.5, 2)) > 1e-2           # (the guide matters)
    xg, jg = torch.from_numpy(x.copy()).cuda(), torch.from_numpy(j.copy()).cuda()
    for got in (pa.recursive_filter(x, 8.0, 0.5, 2, j), pa.recursive_filter(x, 8.0, 0.5, 2, joint_image=torch.from_numpy(j.copy())),
                pa.recursive_filter(xg, 8.0, 0.5, 2, jg).cpu().numpy(), pa.recursive_filter(xg, 8.0, 0.5, 2, j.copy()).cpu().numpy()):
        assert got.dtype == np.float32 and maxabs(got, want) < 5e-6
    xh, jh = x.astype(np.float16), j.astype(np.float16)
    wanth = ref.recursive_filter(xh.astype(np.float32), 8.0, 0.5, 2, jh.astype(np.float32))
    for got in (pa.recursive_filter(xh, 8.0, 0.5, 2, j), pa.recursive_filter(xh, 8.0, 0.5, 2, jh),
                pa.recursive_filter(xg.half(), 8.0, 0.5, 2, jg).cpu().numpy(), pa.recursive_filter(xg.half(), 8.0, 0.5, 2, jg.half()).cpu().numpy()):
        assert got.dtype == np.float16 and maxabs(got, wanth) < 1e-3


def test_normalized_convolution_golden(golden):
    g = golden("native_dt.npz")
    ss, sr, n = g["p_a"]
    assert maxabs(pa.normalized_convolution(g["x_a"], ss, sr, int(n)), g["nc_a"]) < 1e-6
    got = pa.normalized_convolution(torch.from_numpy(g["x_a"]).cuda(), float(ss), float(sr), int(n))
    assert got.is_cuda and maxabs(got.cpu().numpy(), g["nc_a"]) < 1e-6


# ---------------------------------------------------------------------------------------------
# edge_aware_filtering
# ---------------------------------------------------------------------------------------------
def test_edge_aware_filtering_bilateral():
    shape = (2, 3, 17, 65)
    x = image(shape)
    want, bound = yardstick(shape, 5, 5.0, 0.1)
    smooth, noise = pa.edge_aware_filtering(x, 2.0, 0.8)
    assert np.array_equal(smooth, pa.bilateral_filter(x))                      # sigma_s / sigma_r unused, deblurring.py:107-108
    assert maxabs(smooth, want) < bound and maxabs(noise, x - want) < bound + 1e-7
    o_smooth, o_noise = ref.edge_aware_filtering(x, 2.0, 0.8, "bilateral")
    assert maxabs(smooth, o_smooth) < 3e-6 and maxabs(noise, o_noise) < 3e-6
    assert noise.dtype == np.float32 and maxabs(smooth + noise, x) < 1e-6
    sg, ng = pa.edge_aware_filtering(torch.from_numpy(x.copy()).cuda(), 2.0, 0.8, prefilter="bilateral")
    assert sg.is_cuda and ng.is_cuda and np.array_equal(sg.cpu().numpy(), smooth) and np.array_equal(ng.cpu().numpy(), noise)
    sh, nh = pa.edge_aware_filtering(x.astype(np.float16), 2.0, 0.8)
    assert sh.dtype == np.float16 and nh.dtype == np.float16


def test_edge_aware_filtering_domain_transform():
    x = image((2, 3, 17, 65))
    smooth, noise = pa.edge_aware_filtering(x, 2.0, 0.8, prefilter="domain_transform")
    o_smooth, o_noise = ref.edge_aware_filtering(x, 2.0, 0.8, "domain_transform")
    assert maxabs(smooth, o_smooth) < 5e-6 and maxabs(noise, o_noise) < 5e-6
    assert maxabs(smooth, pa.bilateral_filter(x)) > 1e-3                       # (not the bilateral filter)
    assert maxabs(smooth + noise, x) < 1e-6


def test_edge_aware_filtering_normalized_convolution(golden):
    g = golden("native_dt.npz")                                                # case a: sigma 2 / 0.8, one iteration
    x = g["x_a"]
    assert np.allclose(g["p_a"], (2.0, 0.8, 1.0))
    smooth, noise = pa.edge_aware_filtering(x, 2.0, 0.8, prefilter="normalized_convolution")
    o_smooth, o_noise = ref.edge_aware_filtering(x, 2.0, 0.8, "normalized_convolution")
    assert maxabs(smooth, g["nc_a"]) < 1e-6 and maxabs(smooth, o_smooth) < 1e-6 and maxabs(noise, o_noise) < 1e-6
    assert maxabs(smooth + noise, x) < 1e-6
