"""GPU parity: the HIP engine (through the C ABI) against the reference's golden vectors and
against the CPU oracle on the same seeded inputs.  Tolerances are fp32 (stated per check);
the north star asks for end-to-end agreement with the reference's NumPy path within a stated
fp32 tolerance: 2e-5 max-abs after n_iter=3 with the identical theta sequence."""
import functools
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import polyblur_ref as ref                      # the checker (tests only)
from polyblur_amd import _capi as capi
from polyblur_amd.synthetic import synthetic_blurry_batch

KW = dict(c=0.362, b=0.468, alpha=6, beta=1)


@pytest.fixture(scope="module")
def eng():
    from polyblur_amd.engine import get_engine
    return get_engine(0)


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


# ---------------------------------------------------------------------------------------------
# stages
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["stages_A.npz", "stages_B.npz", "stages_C.npz"])
def test_fourier_gradients(eng, golden, name):
    g = golden(name)
    gx, gy = eng.fourier_gradients(g["x"])
    assert maxabs(gx, g["grad_x"]) < 5e-6, maxabs(gx, g["grad_x"])
    assert maxabs(gy, g["grad_y"]) < 5e-6, maxabs(gy, g["grad_y"])


@pytest.mark.parametrize("shape", [(1, 1, 64, 64), (1, 2, 50, 70), (2, 1, 121, 77), (1, 1, 97, 101), (1, 1, 360, 480),
                                   (1, 1, 2, 3), (1, 1, 1080, 1920), (1, 1, 45, 75), (2, 1, 135, 63), (1, 1, 16, 15)])
def test_fourier_gradients_sizes(eng, shape):
    """mixed radix (2,3,4,5,7), Bluestein (prime factors > 7, e.g. 97, 101, 121=11^2), tiny sizes, one-stage plans
    (16, 15), and odd lengths on the multi-stage (fused) plans: an unpaired last row / last column"""
    rng = np.random.default_rng(7)
    x = rng.random(shape, dtype=np.float32)
    gx, gy = eng.fourier_gradients(x)
    rx, ry = ref.spectral_gradients(x)
    scale = max(1.0, float(np.abs(rx).max()))
    assert maxabs(gx, rx) < 4e-6 * scale and maxabs(gy, ry) < 4e-6 * scale


@pytest.mark.parametrize("shape", [(1, 1, 4320, 40), (1, 1, 40, 7680), (2, 1, 3240, 24), (1, 1, 33, 4320), (1, 1, 7680, 18),
                                   (1, 1, 12, 6480), (1, 1, 5400, 16)])
def test_fourier_gradients_extended_radices(eng, shape):
    """lines whose plan takes radices 18 / 20 / 24 to save a stage (4320 = 16 x 15 x 18, 7680 = 16 x 20 x 24 -- the 8K sides --,
    3240, 5400, 6480): the 512-thread row variant and the 1024-thread column variants (csrc/line_choice.h: factorize,
    plan_ext); the other kernel variants keep the greedy plan of the same length"""
    rng = np.random.default_rng(13)
    x = rng.random(shape, dtype=np.float32)
    gx, gy = eng.fourier_gradients(x)
    rx, ry = ref.spectral_gradients(x)
    scale = max(1.0, float(np.abs(rx).max()), float(np.abs(ry).max()))
    assert maxabs(gx, rx) < 4e-6 * scale and maxabs(gy, ry) < 4e-6 * scale


def opts(**kw):
    from polyblur_amd.engine import Engine
    return Engine.make_options(**kw)


@pytest.mark.parametrize("name", ["stages_A.npz", "stages_B.npz", "stages_C.npz"])
def test_estimate_blur(eng, golden, name):
    g = golden(name)
    info = eng.estimate_blur(g["x"], opts(c=0.362, b=0.468))
    assert maxabs(info["mags"][:, :7], g["mags"]) < 5e-6
    assert maxabs(info["interp"][:, :30], g["interp"]) < 5e-6
    assert np.array_equal(info["theta"], g["theta"])
    assert maxabs(info["sigma"], g["sigma"]) < 2e-5 and maxabs(info["rho"], g["rho"]) < 2e-5
    assert maxabs(info["kernel"], g["kernel"]) < 1e-5
    assert maxabs(info["gray_min"], g["gray"].reshape(g["gray"].shape[0], -1).min(1)) == 0
    assert maxabs(info["gray_max"], g["gray"].reshape(g["gray"].shape[0], -1).max(1)) == 0


@pytest.mark.parametrize("shape,q", [((2, 3, 160, 224), 1e-4), ((1, 1, 97, 131), 0.01), ((1, 3, 1080, 1920), 1e-4)])
def test_quantile_normalisation(eng, shape, q):
    """q > 0: the clip values are torch.quantile's (linear interpolation between exact order statistics)"""
    x, _ = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=55)
    info = eng.estimate_blur(x, opts(c=0.362, b=0.468, q=q))
    gray = x.mean(axis=1, dtype=np.float32) if shape[1] == 3 else x[:, 0]
    flat = np.sort(gray.reshape(shape[0], -1), axis=1)
    n1 = np.float32(flat.shape[1] - 1)
    for which, qq, key in ((0, np.float32(q), "gray_min"), (1, np.float32(1.0 - q), "gray_max")):
        r = qq * n1
        f = np.floor(r)
        lo_i, hi_i = int(f), int(min(f + 1, n1))
        w = np.float32(r - f)
        want = flat[:, lo_i] + w * (flat[:, hi_i] - flat[:, lo_i])
        assert maxabs(info[key], want) < 2e-7, (which, info[key], want)


def test_make_kernels_grid(eng, golden):
    g = golden("kernel_grid.npz")
    buf = eng.make_kernels(g["sigma"], g["rho"], g["theta"])
    info = eng.read_info(buf, g["sigma"].size)
    assert maxabs(info["kernel"], g["kernels"]) < 5e-7
    sep_expected = (np.isin(np.round(np.rad2deg(g["theta"])).astype(int) % 90, [0])) | (g["sigma"] == g["rho"])
    assert np.array_equal(info["separable"].astype(bool), sep_expected)
    # full support: the radius class covers every tap that is not exactly 0.0f
    k = info["kernel"].reshape(-1, 25, 25) != 0
    d = np.abs(np.arange(25) - 12)
    ext = np.maximum((k.any(axis=1) * d).max(axis=1), (k.any(axis=2) * d).max(axis=1))
    assert np.array_equal(info["radius"], np.where(ext <= 4, 4, np.where(ext <= 6, 6, np.where(ext <= 8, 8, np.where(ext <= 10, 10, 12)))))
    assert np.all(info["radius"][np.maximum(g["sigma"], g["rho"]) >= 1.0] == 12)
    # adaptive support: radius class follows the wider std
    buf = eng.make_kernels(g["sigma"], g["rho"], g["theta"], support=capi.PB_SUPPORT_ADAPTIVE)
    info = eng.read_info(buf, g["sigma"].size)
    smax = np.maximum(g["sigma"], g["rho"])
    assert np.all(info["radius"][smax <= 0.55] == 4)
    assert np.all(info["radius"][smax >= 4.0] == 12)
    assert set(np.unique(info["radius"])) <= {4, 6, 8, 10, 12}
    # the phase lists of the general body: even per-kind counts, full rows under the full policy at sigma = 4, and
    # under the adaptive policy only the segments inside the Gaussian's ellipse
    gen = info["separable"] == 0
    assert np.all(info["nphase"] % 2 == 0) and np.all(info["nphase"].sum(axis=1)[gen] > 0)
    full = eng.read_info(eng.make_kernels(g["sigma"], g["rho"], g["theta"]), g["sigma"].size)
    wide = gen & (np.minimum(g["sigma"], g["rho"]) >= 2.0)
    assert np.all(full["nphase"].sum(axis=1)[wide] == 178)          # 25 rows x 7 chunks (+1 filler per kind)
    na, nf = info["nphase"].sum(axis=1), full["nphase"].sum(axis=1)
    assert np.all(na[gen] <= nf[gen]) and np.any(na[gen] < 0.7 * nf[gen])
    thin = gen & (smax >= 2.0) & (np.minimum(g["sigma"], g["rho"]) <= 0.55)
    assert thin.any() and np.all(nf[thin] < 178)                   # taps that underflowed to 0.0f are skipped even when "full"


@pytest.mark.parametrize("name", ["stages_A.npz", "stages_B.npz"])
@pytest.mark.parametrize("boundary,key", [(capi.PB_WRAP, "conv_fft_kwide"), (capi.PB_ZERO, "conv_direct_kwide")])
def test_convolve2d(eng, golden, name, boundary, key):
    g = golden(name)
    xp = ref.replicate_pad(g["x"], 12)
    buf = eng.set_kernels(g["kwide"])
    out = eng.convolve2d(xp, buf, boundary)
    assert maxabs(out, g[key]) < 2e-6


def _odd_kernels():
    """caller-supplied taps that are NOT point-symmetric: a shifted delta pair, a one-sided motion streak, an off-centre blob"""
    K = capi.PB_KSIZE; c = K // 2
    k = np.zeros((3, K, K), np.float64)
    k[0, c + 3, c - 2] = 0.8; k[0, c, c] = 0.2
    for t in range(9): k[1, c - t // 2, c + t] += 1.0 + 0.1 * t
    yy, xx = np.mgrid[-c:c + 1, -c:c + 1].astype(np.float64)
    k[2] = np.exp(-0.5 * ((xx - 2.5) ** 2 / 4.0 + (yy + 1.5) ** 2 / 1.5)) * (1.0 + 0.05 * xx).clip(0.1)
    return (k / k.sum(axis=(1, 2), keepdims=True)).astype(np.float32)


@pytest.mark.parametrize("method,boundary", [("fft", capi.PB_WRAP), ("direct", capi.PB_ZERO)])
def test_caller_kernels_that_are_not_point_symmetric(eng, method, boundary):
    """the reference CORRELATES under method='direct' (F.conv2d, filters.py:40-49) and CONVOLVES under method='fft'
    (K = p2o(kernel), filters.py:33-36): for taps that are not point-symmetric the two differ by a reflection, and the stage
    entry points follow the reference in both (found by tools/sweep_random_kernels.py: the wrap boundary correlated too).
    convolve2d, the edgetaper, the inverse filter with and without the edgetaper, a batch that mixes such kernels with a
    Gaussian -- against the oracle, which is pinned to the reference on exactly this (tests/test_oracle_golden.py)"""
    # (a smaller call with a point-symmetric kernel first: the buffers that grow for the next call are freed in between, and which
    #  record sets hold taps that are not point-symmetric has to outlive that -- it is not one of the context's disposable hints)
    g1 = np.asarray(ref.gaussian_kernel_2d(np.float32([0.3]), np.float32([1.5]), np.float32([1.0])), np.float32).reshape(1, capi.PB_KSIZE, capi.PB_KSIZE)
    x1, _ = synthetic_blurry_batch(1, 3, 96, 128, seed0=40)
    xp1 = ref.replicate_pad(x1, capi.PB_KSIZE // 2)
    assert maxabs(eng.convolve2d(xp1, eng.set_kernels(g1), boundary), ref.convolve2d(xp1, g1[:, None], method=method)) < 2e-6
    ks = np.concatenate([_odd_kernels(), np.asarray(ref.gaussian_kernel_2d(np.float32([0.7]), np.float32([2.0]), np.float32([1.0])), np.float32).reshape(1, capi.PB_KSIZE, capi.PB_KSIZE)])
    B = ks.shape[0]
    x, _ = synthetic_blurry_batch(B, 3, 150, 210, seed0=41)
    buf = eng.set_kernels(ks)
    xp = ref.replicate_pad(x, capi.PB_KSIZE // 2)
    assert maxabs(eng.convolve2d(xp, buf, boundary), ref.convolve2d(xp, ks[:, None], method=method)) < 2e-6
    assert maxabs(eng.edgetaper(xp, buf, boundary), ref.edgetaper(xp, ks[:, None], method=method)) < 4e-6
    for taper in (False, True):
        got = eng.inverse_filter(x, buf, 6.0, 1.0, boundary, edgetaping=taper)
        assert maxabs(got, ref.inverse_filtering_rank3(x, ks[:, None], 6.0, 1.0, do_edgetaper=taper, method=method)) < 2e-5
    # the records themselves are untouched: the other boundary model right after, and the first again
    other = capi.PB_ZERO if boundary == capi.PB_WRAP else capi.PB_WRAP
    om = "direct" if method == "fft" else "fft"
    assert maxabs(eng.convolve2d(xp, buf, other), ref.convolve2d(xp, ks[:, None], method=om)) < 2e-6
    assert maxabs(eng.convolve2d(xp, buf, boundary), ref.convolve2d(xp, ks[:, None], method=method)) < 2e-6


def test_not_point_symmetric_kernels_outlive_set_dense_eval(eng):
    """which record sets hold taps that are not point-symmetric is a fact about the caller's data, not one of the context's
    disposable hints: pb_set_dense_eval drops the hints (which body each cached record takes has changed) and must leave that
    fact alone -- it used to clear it, and the wrap boundary then correlated again.  The oracle's true convolution
    (method='fft', filters.py:33-36) after each switch of the evaluation mode"""
    ks = _odd_kernels()
    x, _ = synthetic_blurry_batch(ks.shape[0], 3, 150, 210, seed0=42)
    xp = ref.replicate_pad(x, capi.PB_KSIZE // 2)
    want = ref.convolve2d(xp, ks[:, None], method="fft")
    buf = eng.set_kernels(ks)
    try:
        eng.set_dense_eval("stencil")
        assert maxabs(eng.convolve2d(xp, buf, capi.PB_WRAP), want) < 2e-6
        eng.set_dense_eval("auto", capi.PB_DENSE_MIN_PHASES)
        assert maxabs(eng.convolve2d(xp, buf, capi.PB_WRAP), want) < 2e-6
    finally:
        eng.set_dense_eval("auto", capi.PB_DENSE_MIN_PHASES)


@pytest.mark.parametrize("name", ["stages_A.npz", "stages_B.npz", "stages_C.npz"])
@pytest.mark.parametrize("kname", ["kest", "kwide"])
def test_inverse_filter_fft(eng, golden, name, kname):
    g = golden(name)
    k = g["kernel" if kname == "kest" else "kwide"]
    buf = eng.set_kernels(k)
    out = eng.inverse_filter(g["x"], buf, 6.0, 1.0, capi.PB_WRAP)
    assert maxabs(out, g["inv_fft_" + kname]) < 1e-5
    # the un-clamped polynomial on the padded domain, cropped (golden poly_* is the padded result)
    want = np.clip(ref.crop(g["poly_fft_" + kname], 12), 0, 1)
    assert maxabs(out, want) < 1e-5


@pytest.mark.parametrize("name", ["stages_A.npz", "stages_B.npz"])
def test_inverse_filter_direct(eng, golden, name):
    g = golden(name)
    for kname in ("kest", "kwide"):
        buf = eng.set_kernels(g["kernel" if kname == "kest" else "kwide"])
        out = eng.inverse_filter(g["x"], buf, 6.0, 1.0, capi.PB_ZERO)
        want = np.clip(ref.crop(g["poly_direct_" + kname], 12), 0, 1)
        assert maxabs(out, want) < 1e-5


@pytest.mark.parametrize("name", ["stages_A.npz", "stages_B.npz"])
@pytest.mark.parametrize("boundary,key", [(capi.PB_WRAP, "taper_fft_kwide"), (capi.PB_ZERO, "taper_direct_kwide")])
def test_edgetaper(eng, golden, name, boundary, key):
    g = golden(name)
    xp = ref.replicate_pad(g["x"], 12)
    buf = eng.set_kernels(g["kwide"])
    out = eng.edgetaper(xp, buf, boundary)
    assert maxabs(out, g[key]) < 4e-6
    # the closed-form alpha equals the reference's FFT autocorrelation
    info = eng.read_info(buf, 1)
    Hp, Wp = xp.shape[-2:]
    def v(ac, n):
        p = np.arange(n); m = np.minimum(p, n - 1 - p)
        z = np.where(m < 25, ac[np.minimum(m, 24)], 0.0)
        return 1 - z / ac[0]
    alpha = v(info["acorr_y"][0], Hp)[:, None] * v(info["acorr_x"][0], Wp)[None, :]
    assert maxabs(alpha, g["taper_alpha_kwide"][0, 0]) < 2e-6


@pytest.mark.parametrize("name", ["stages_A.npz", "stages_B.npz"])
def test_halo_mask(eng, golden, name):
    """(on these goldens the mask moves the output by 6e-7: the checks that can tell it from a no-op are tests/test_gpu_halo.py)"""
    g = golden(name)
    y = g["inv_fft_kwide"]
    out = eng.halo_mask(g["x"], y, g["grad_x"], g["grad_y"])
    assert maxabs(out, g["halo_kwide"]) < 1e-5


@pytest.mark.parametrize("name", ["stages_A.npz", "stages_B.npz", "stages_C.npz"])
def test_edge_aware_filters(eng, golden, name):
    g = golden(name)
    assert maxabs(eng.bilateral5(g["x"]), g["bilateral"]) < 3e-6
    assert maxabs(eng.dt_recursive_filter(g["x"], 2.0, 0.8, 1), g["rf_n1"]) < 3e-6
    assert maxabs(eng.dt_recursive_filter(g["x"], 60.0, 0.4, 3), g["rf_n3"]) < 1e-5


@pytest.mark.parametrize("case", list("abcde"))
def test_normalized_convolution_goldens(eng, golden, case):
    """NC.cpp compiled from the reference's source (tests/golden/make_golden_native.py) vs the HIP kernels"""
    g = golden("native_dt.npz")
    ss, sr, n = g["p_" + case]
    got = eng.dt_normalized_convolution(g["x_" + case], ss, sr, int(n))
    assert maxabs(got, g["nc_" + case]) < 1e-6, maxabs(got, g["nc_" + case])


@pytest.mark.parametrize("shape,ss,sr,n", [((2, 3, 130, 250), 2.0, 0.8, 1), ((1, 1, 77, 301), 20.0, 0.3, 3),
                                           ((1, 4, 64, 1000), 5.0, 0.2, 2), ((1, 3, 1080, 1920), 2.0, 0.8, 1)])
def test_normalized_convolution_sizes(eng, shape, ss, sr, n):
    """batches (per-image semantics), C != 3, long rows; fp16 I/O"""
    x, _ = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=31)
    want = ref.normalized_convolution(x, ss, sr, n)
    got = eng.dt_normalized_convolution(x, ss, sr, n)
    # box limits are exact float comparisons: a last-bit difference in a prefix sum can move one limit by a sample
    d = np.abs(got - want)
    assert np.mean(d > 1e-5) < 1e-4 and d.max() < 5e-2, (float(d.max()), float(np.mean(d > 1e-5)))
    if shape[2] <= 130:
        xh = x.astype(np.float16)
        goth = eng.dt_normalized_convolution(xh, ss, sr, n)
        wanth = ref.normalized_convolution(xh.astype(np.float32), ss, sr, n)
        assert goth.dtype == np.float16 and np.mean(np.abs(goth.astype(np.float32) - wanth) > 2e-3) < 1e-3


@pytest.mark.parametrize("body", ["auto", "stencil"])
@pytest.mark.parametrize("seed", [41, 43])
def test_pipeline_with_normalized_convolution_prefilter(eng, body, seed):
    """Iteration by iteration on IDENTICAL inputs -- the engine's output of iteration k is what both sides deblur in
    iteration k + 1 -- so that a box limit of the (discontinuous) NC filter that flips on a last-bit difference cannot
    compound across iterations: every iteration is held to the plain fp32 tolerance, through both dense bodies
    (measured, tools/nc_check2.py: <= 1.3e-6 through the tile-spectrum body, <= 5.2e-6 through the stencil body)."""
    import torch
    from polyblur_amd import polyblur_deblurring
    x, _ = synthetic_blurry_batch(2, 3, 96, 140, seed0=seed)
    kw = dict(n_iter=1, prefiltering=True, sigma_s=2.0, sigma_r=0.8, **KW)
    eng.set_dense_eval(body, 0)
    try:
        cur = x
        for _ in range(3):
            got = polyblur_deblurring(torch.from_numpy(cur), prefilter="normalized_convolution", **kw).numpy()
            want = ref.polyblur_deblurring(cur, prefilter="normalized_convolution", **kw)
            assert maxabs(got, want) < 2e-5
            cur = got
        # the chained call is the same three iterations (the prefilter's split and recombination included)
        chained = polyblur_deblurring(torch.from_numpy(x), prefilter="normalized_convolution", **dict(kw, n_iter=3)).numpy()
        assert maxabs(chained, cur) < 1e-6
    finally:
        eng.set_dense_eval("auto", capi.PB_DENSE_MIN_PHASES)


def test_dt_filter_joint_and_wide(eng):
    rng = np.random.default_rng(5)
    x = rng.random((2, 3, 37, 203), dtype=np.float32)          # W spans several 64-wide scan chunks, ragged tail
    j = rng.random((2, 3, 37, 203), dtype=np.float32)
    assert maxabs(eng.dt_recursive_filter(x, 8.0, 0.5, 2, joint=j), ref.recursive_filter(x, 8.0, 0.5, 2, j)) < 5e-6


@pytest.mark.parametrize("shape,n", [((1, 1, 33, 70), 1), ((2, 1, 65, 129), 3), ((1, 2, 40, 130), 2), ((1, 4, 21, 64), 1),
                                     ((3, 3, 2, 90), 1), ((1, 3, 90, 2), 2)])
def test_dt_filter_channel_counts(eng, shape, n):
    """1 and 3 channels take the kernels that recompute the domain weights in place, any other count the ones that
    read them from domain planes; two-row / two-column images; fp16 input"""
    rng = np.random.default_rng(17)
    x = rng.random(shape, dtype=np.float32)
    assert maxabs(eng.dt_recursive_filter(x, 6.0, 0.4, n), ref.recursive_filter(x, 6.0, 0.4, n)) < 5e-6
    xh = x.astype(np.float16)
    got = eng.dt_recursive_filter(xh, 6.0, 0.4, n)
    assert got.dtype == np.float16
    assert maxabs(got, ref.recursive_filter(xh.astype(np.float32), 6.0, 0.4, n)) < 1e-3


# ---------------------------------------------------------------------------------------------
# rank-1 (separable) kernels and support policy
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sigma,rho,deg", [(2.5, 1.0, 0.0), (1.0, 3.0, 90.0), (1.7, 1.7, 36.0), (0.5, 0.3, 0.0),
                                           (4.0, 0.3, 90.0)])
@pytest.mark.parametrize("boundary,method", [(capi.PB_WRAP, "fft"), (capi.PB_ZERO, "direct")])
def test_separable_path(eng, sigma, rho, deg, boundary, method):
    x, _ = synthetic_blurry_batch(1, 3, 150, 210, seed0=11)
    th = np.float32(deg) * np.float32(np.pi) / np.float32(180)
    k = ref.gaussian_kernel_2d([th], [sigma], [rho])
    buf = eng.make_kernels([sigma], [rho], [th])
    info = eng.read_info(buf, 1)
    assert info["separable"][0] == 1
    assert maxabs(info["kernel"], k) < 3e-7
    out = eng.inverse_filter(x, buf, 6.0, 1.0, boundary)
    want = ref.inverse_filtering_rank3(x, k[:, None], 6.0, 1.0, method=method)
    assert maxabs(out, want) < 1e-5
    # same taps through the general 2-D stencil (rank-1 detection disabled)
    buf2 = eng.set_kernels(k, support=capi.PB_SUPPORT_FULL | 16, name="np.info2")
    assert eng.read_info(buf2, 1)["separable"][0] == 0
    out2 = eng.inverse_filter(x, buf2, 6.0, 1.0, boundary)
    assert maxabs(out, out2) < 5e-6


@pytest.mark.parametrize("sigma,rho,deg", [(0.6, 0.4, 24.0), (1.3, 0.8, 60.0), (1.0, 0.5, 0.0), (3.0, 2.0, 12.0)])
def test_adaptive_support_matches_full(eng, sigma, rho, deg):
    x, _ = synthetic_blurry_batch(2, 3, 100, 140, seed0=21)
    th = np.deg2rad(np.float32(deg))
    full = eng.make_kernels([sigma] * 2, [rho] * 2, [th] * 2, support=capi.PB_SUPPORT_FULL)
    a = eng.inverse_filter(x, full, 6.0, 1.0, capi.PB_WRAP)
    adap = eng.make_kernels([sigma] * 2, [rho] * 2, [th] * 2, support=capi.PB_SUPPORT_ADAPTIVE, name="np.info2")
    assert eng.read_info(adap, 2)["radius"][0] in ((4, 6, 8, 10, 12) if sigma < 1.5 else (10, 12))
    b = eng.inverse_filter(x, adap, 6.0, 1.0, capi.PB_WRAP)
    # (fp32 rounding of the Horner temporaries, which reach 9x the image range; the two policies may also put the image
    # on different bodies -- tile-spectrum for the full box, stencil for the trimmed one: 2.0e-6 measured then, 1e-6 otherwise)
    assert maxabs(a, b) < 4e-6


# ---------------------------------------------------------------------------------------------
# whole pipeline against the reference's goldens
# ---------------------------------------------------------------------------------------------
def check_iterations(g, prefix, infos, n):
    for it in range(n):
        p = "%s/it%d/" % (prefix, it)
        assert np.array_equal(infos[it]["theta"], g[p + "theta"]), (it, infos[it]["theta"], g[p + "theta"])
        assert maxabs(infos[it]["mags"], g[p + "mags"]) < 3e-5, (it, "mags")
        assert maxabs(infos[it]["sigma"], g[p + "sigma"]) < 1e-4, (it, "sigma")
        assert maxabs(infos[it]["rho"], g[p + "rho"]) < 1e-4, (it, "rho")
        assert maxabs(infos[it]["kernel"], g[p + "kernel"]) < 3e-5, (it, "kernel")


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_pipeline_peacock(golden, method):
    """BASELINE config 1: the reference's own demo image, n_iter=3, alpha=6, beta=1."""
    from PIL import Image
    from polyblur_amd import polyblur_deblurring
    g = golden("pipeline_peacock.npz")
    img = np.asarray(Image.open(os.path.join(os.path.dirname(__file__), "golden", "peacock_defocus.png")))
    img = img[..., :3].astype(np.float32) / 255.0
    out, infos = polyblur_deblurring(img, n_iter=3, method=method, return_info=True, **KW)
    assert out.shape == img.shape and out.dtype == np.float32
    check_iterations(g, method, infos, 3)
    gold = np.moveaxis(g[method + "/out"][0], 0, 2)
    assert maxabs(out, gold) < 2e-5, maxabs(out, gold)
    # SURVEY Appendix A known-good values
    assert [int(round(np.rad2deg(i["theta"][0]))) for i in infos] == [0, 24, 30]
    assert abs(float(infos[0]["sigma"][0]) - 0.96224) < 1e-4 and abs(float(infos[0]["rho"][0]) - 0.55467) < 1e-4


VARIANTS = [("plain", {}), ("edgetaping", dict(edgetaping=True)), ("remove_halo", dict(remove_halo=True)),
            ("prefiltering", dict(prefiltering=True)), ("discard_saturation", dict(discard_saturation=True)),
            ("q1e-4", dict(q=1e-4)), ("all", dict(edgetaping=True, remove_halo=True, prefiltering=True))]


@pytest.mark.parametrize("variant,o", VARIANTS)
@pytest.mark.parametrize("method", ["fft", "direct"])
def test_pipeline_variants(golden, variant, o, method):
    import torch
    from polyblur_amd import polyblur_deblurring
    g = golden("pipeline_variants.npz")
    x = torch.from_numpy(g["x"]).cuda()
    out, infos = polyblur_deblurring(x, n_iter=3, method=method, return_info=True, **KW, **o)
    assert out.is_cuda and out.shape == x.shape and out.dtype == x.dtype
    check_iterations(g, "%s/%s" % (variant, method), infos, 3)
    assert maxabs(out.cpu().numpy(), g["%s/%s/out" % (variant, method)]) < 3e-5


def test_pipeline_misc(golden):
    from polyblur_amd import polyblur_deblurring, PolyblurDeblurring
    g = golden("pipeline_variants.npz")
    out, infos = polyblur_deblurring(g["x_sat"][0].transpose(1, 2, 0), n_iter=2, discard_saturation=True,
                                     return_info=True, **KW)
    check_iterations(g, "sat/fft", infos, 2)
    assert maxabs(out.transpose(2, 0, 1)[None], g["sat/fft/out"]) < 3e-5
    xg = np.ascontiguousarray(g["x"][0, 1])                                  # (H,W) gray ndarray
    out = polyblur_deblurring(xg, n_iter=2, **KW)
    assert out.shape == xg.shape and maxabs(out, g["gray/fft/out"][0, 0]) < 3e-5
    out = polyblur_deblurring(xg, n_iter=1, **KW)
    assert maxabs(out, g["gray_ndarray_hw"]) < 2e-5
    import torch
    xt = torch.from_numpy(g["x"])                                            # CPU tensor in -> CPU tensor out
    o = polyblur_deblurring(xt)
    assert not o.is_cuda and maxabs(o.numpy(), g["defaults/functional"]) < 2e-5
    m = PolyblurDeblurring()
    assert maxabs(m(xt.cuda()).cpu().numpy(), g["defaults/module"]) < 2e-5
    assert maxabs(m(xt.cuda(), n_iter=2, alpha=6, beta=1).cpu().numpy(), g["module_n2"]) < 2e-5


EXTRA = {"a6_i45": dict(n_iter=2, n_interpolated_angles=45), "a6_i12": dict(n_iter=2, n_interpolated_angles=12),
         "a6_i60": dict(n_iter=1, n_interpolated_angles=60), "a6_i7": dict(n_iter=2, n_interpolated_angles=7)}


@pytest.mark.parametrize("name", sorted(EXTRA))
@pytest.mark.parametrize("method", ["fft", "direct"])
def test_pipeline_extra_interpolation_grids(golden, name, method):
    """other interpolation grids than 30 (tests/golden/make_golden_extra.py ran the reference on them)"""
    import torch
    from polyblur_amd import polyblur_deblurring
    g = golden("pipeline_extra.npz")
    out = polyblur_deblurring(torch.from_numpy(g["x"]).cuda(), method=method, **KW, **EXTRA[name]).cpu().numpy()
    assert maxabs(out, g["%s_%s" % (name, method)]) < 2e-5


def test_pipeline_extra_defaults_and_odd_batch(golden):
    import torch
    from polyblur_amd import polyblur_deblurring, PolyblurDeblurring
    g = golden("pipeline_extra.npz")
    out = polyblur_deblurring(torch.from_numpy(g["y"]).cuda(), n_iter=3, method="fft", **KW).cpu().numpy()
    assert maxabs(out, g["odd_batch_fft"]) < 2e-5
    out = PolyblurDeblurring()(torch.from_numpy(g["x"]).cuda(), n_iter=3).cpu().numpy()
    assert maxabs(out, g["module_defaults_n3"]) < 2e-5
    out = polyblur_deblurring(torch.from_numpy(g["x"]).cuda(), n_iter=2).cpu().numpy()
    assert maxabs(out, g["functional_defaults_n2"]) < 2e-5


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_pipeline_strongblur(golden, method):
    """sigma ~ 3.5 blur: fft and direct differ by 3.6e-2 at the border -- each must match its own golden"""
    from polyblur_amd import polyblur_deblurring
    import torch
    g = golden("pipeline_strongblur.npz")
    out, infos = polyblur_deblurring(torch.from_numpy(g["x"]).cuda(), n_iter=3, method=method, return_info=True, **KW)
    check_iterations(g, method, infos, 3)
    assert maxabs(out.cpu().numpy(), g[method + "/out"]) < 3e-5
    assert maxabs(g["fft/out"], g["direct/out"]) > 1e-3


def test_pipeline_batch(golden):
    from polyblur_amd import polyblur_deblurring
    import torch
    g = golden("pipeline_batch.npz")
    x = torch.from_numpy(g["x"]).cuda()
    out, infos = polyblur_deblurring(x, n_iter=3, return_info=True, **KW)
    check_iterations(g, "fft", infos, 3)
    assert maxabs(out.cpu().numpy(), g["fft/out"]) < 3e-5
    # independence of images: any sub-batch gives bit-identical rows
    out1 = polyblur_deblurring(x[1:2].contiguous(), n_iter=3, **KW)
    assert torch.equal(out1, out[1:2])
    # adaptive support stays within rounding of the full-support result
    out_a = polyblur_deblurring(x, n_iter=3, support="adaptive", **KW)
    assert maxabs(out_a.cpu().numpy(), out.cpu().numpy()) < 1e-5


def test_pipeline_fp16(golden):
    """fp16 I/O (configs 3 and 5): inputs rounded to fp16, fp32 oracle on those inputs.
    Estimation, all temporaries and the images between iterations stay fp32; only the final store rounds:
    tolerance = 1 fp16 ulp at 1.0 (SURVEY 8c asks for <= 2e-3)."""
    from polyblur_amd import polyblur_deblurring
    import torch
    g = golden("pipeline_fp16in.npz")
    x = torch.from_numpy(g["x"]).cuda().half()
    out, infos = polyblur_deblurring(x, n_iter=1, return_info=True, **KW)
    assert out.dtype == torch.float16
    check_iterations(g, "fft", infos, 1)
    out3, infos3 = polyblur_deblurring(x, n_iter=3, return_info=True, **KW)
    assert [float(i["theta"][0]) for i in infos3] == [float(g["fft/it%d/theta" % k][0]) for k in range(3)]
    assert maxabs(out3.float().cpu().numpy(), g["fft/out"]) < 1e-3


def test_argument_errors():
    from polyblur_amd import polyblur_deblurring, PolyblurDeblurring
    x = np.zeros((32, 32, 3), np.float32)
    with pytest.raises(ValueError):
        polyblur_deblurring(x, method="nope")
    with pytest.raises(ValueError):
        polyblur_deblurring(x, q=0.7)
    with pytest.raises(ValueError):
        PolyblurDeblurring(patch_decomposition=True)(x)               # the patch branch needs a (B,C,H,W) tensor
    with pytest.raises(ValueError):
        polyblur_deblurring(np.zeros((2, 2, 2, 2, 2), np.float32))


# ---------------------------------------------------------------------------------------------
# full-size properties (BASELINE config 2: one 4K image) -- no oracle run at this size
# ---------------------------------------------------------------------------------------------
def test_4k_properties(eng):
    import torch
    from polyblur_amd import polyblur_deblurring
    H, W = 2160, 3840
    x, _ = synthetic_blurry_batch(1, 3, 270, 480, seed0=33)
    x = torch.from_numpy(x).cuda()
    x = torch.nn.functional.interpolate(x, size=(H, W), mode="bicubic", align_corners=False).clamp(0, 1).contiguous()
    # (1) a constant image is a fixed point of the polynomial (coefficients sum to 1, kernel sums to 1)
    const = torch.full((1, 3, H, W), 0.37, device="cuda")
    th = np.deg2rad(np.float32(30.0))
    buf = eng.make_kernels([2.0], [1.0], [th])
    outc = torch.empty_like(const)
    rc = eng.lib.pb_inverse_filter(eng.ctx, const.data_ptr(), outc.data_ptr(), capi.PB_F32, 1, 3, H, W, buf.ptr, 6.0, 1.0,
                                   capi.PB_WRAP, 0, 0, None, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert float((outc - 0.37).abs().max()) < 2e-6
    # (2) rank-1 kernel: separable path == general path at full size
    k = ref.gaussian_kernel_2d([np.float32(0)], [2.5], [1.2])
    outs = []
    for flag, name in ((0, "np.info"), (16, "np.info2")):
        b = eng.set_kernels(k, support=capi.PB_SUPPORT_FULL | flag, name=name)
        o = torch.empty_like(x)
        assert eng.lib.pb_inverse_filter(eng.ctx, x.data_ptr(), o.data_ptr(), capi.PB_F32, 1, 3, H, W, b.ptr, 6.0, 1.0,
                                         capi.PB_WRAP, 0, 0, None, None) == 0
        outs.append(o)
    torch.cuda.synchronize()
    assert float((outs[0] - outs[1]).abs().max()) < 1e-5
    # (3) the pipeline at 4K: a down-sampled oracle is not comparable, so check invariants:
    #     range, determinism, and adaptive == full support
    a, infos = polyblur_deblurring(x, n_iter=3, return_info=True, **KW)
    b = polyblur_deblurring(x, n_iter=3, **KW)
    assert torch.equal(a, b)
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0
    c = polyblur_deblurring(x, n_iter=3, support="adaptive", **KW)
    assert float((a - c).abs().max()) < 1e-5
    assert all(0.3 <= float(i["sigma"][0]) <= 4.0 for i in infos)


def test_large_batch_is_per_image(eng):
    """BASELINE configs 3/4 in miniature: a 1080p batch (fp16 I/O, halo masking, domain-transform prefilter; and
    plain fp32) gives every image exactly what it gets alone -- every reduction of the pipeline is per image"""
    import torch
    from polyblur_amd import polyblur_deblurring
    small, _ = synthetic_blurry_batch(6, 3, 135, 240, seed0=90)
    x = torch.nn.functional.interpolate(torch.from_numpy(small).cuda(), size=(1080, 1920), mode="bicubic",
                                        align_corners=False).clamp(0, 1).contiguous()
    for xx, kw in ((x.half(), dict(remove_halo=True, prefiltering=True, prefilter="domain_transform")), (x, dict())):
        full, infos = polyblur_deblurring(xx, n_iter=3, return_info=True, **KW, **kw)
        for i in (0, 3, 5):
            one = polyblur_deblurring(xx[i:i + 1].contiguous(), n_iter=3, **KW, **kw)
            assert torch.equal(full[i:i + 1], one), i
        assert len({float(i_["theta"][k]) for i_ in infos for k in range(6)}) > 1      # the images do differ


def test_8k_fp16_properties(eng):
    """BASELINE config 5's per-GPU share: one 7680x4320 fp16 image, n_iter=5 (longest FFT lines, largest grid)"""
    import torch
    from polyblur_amd import polyblur_deblurring
    H, W = 4320, 7680
    small, _ = synthetic_blurry_batch(1, 3, 270, 480, seed0=34)
    x = torch.nn.functional.interpolate(torch.from_numpy(small).cuda(), size=(H, W), mode="bicubic",
                                        align_corners=False).clamp(0, 1).half().contiguous()
    a, infos = polyblur_deblurring(x, n_iter=5, return_info=True, **KW)
    b = polyblur_deblurring(x, n_iter=5, **KW)
    assert torch.equal(a, b) and a.dtype == torch.float16
    assert float(a.min()) >= 0.0 and float(a.max()) <= 1.0 and bool(torch.isfinite(a).all())
    assert all(0.3 <= float(i["sigma"][0]) <= 4.0 and 0.3 <= float(i["rho"][0]) <= 4.0 for i in infos)
    # the spectral gradient at these lengths (7680 = 2^9*15, 4320 = 2^5*135) against the FFT definition on one plane
    g = x[0, 0].float()
    gx, gy = eng.fourier_gradients(g[None, None].cpu().numpy())
    G = torch.fft.fft2(g.double())
    fx = torch.fft.fftfreq(W, dtype=torch.float64, device="cuda") * W
    fy = torch.fft.fftfreq(H, dtype=torch.float64, device="cuda") * H
    fx[W // 2] = 0
    fy[H // 2] = 0
    rx = torch.fft.ifft2(G * (2j * np.pi * fx / W)[None, :]).real.cpu().numpy()
    ry = torch.fft.ifft2(G * (2j * np.pi * fy / H)[:, None]).real.cpu().numpy()
    scale = max(1.0, float(np.abs(rx).max()), float(np.abs(ry).max()))
    assert maxabs(gx[0, 0], rx) < 1e-5 * scale and maxabs(gy[0, 0], ry) < 1e-5 * scale


# ---------------------------------------------------------------------------------------------
# edge cases: ragged / tiny sizes, mixed batches, degenerate inputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 3, 8, 8), (1, 1, 16, 20), (2, 3, 33, 130), (1, 3, 65, 63), (1, 2, 40, 44),
                                   (1, 3, 45, 75)])
@pytest.mark.parametrize("method", ["fft", "direct"])
def test_small_and_ragged_sizes(shape, method):
    """images smaller than the 25x25 support (the wrap boundary wraps more than once), widths that are
    not multiples of 4 (no 16-byte path), tile-edge sizes, and a 2-channel input (gray = mean over C)"""
    from polyblur_amd import polyblur_deblurring
    import torch
    x, _ = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=91)
    out, infos = polyblur_deblurring(torch.from_numpy(x).cuda(), n_iter=2, method=method, return_info=True, **KW)
    want, winfos = ref.polyblur_deblurring(x, n_iter=2, method=method, return_info=True, **KW)
    for a, b in zip(infos, winfos):
        assert np.array_equal(a["theta"], b["theta"])
    assert maxabs(out.cpu().numpy(), want) < 3e-5


def _random_case(i):
    rng = np.random.default_rng(9000 + i)
    B, C = int(rng.integers(1, 4)), int(rng.choice([1, 3]))
    H, W = int(rng.integers(26, 190)), int(rng.integers(26, 230))
    kw = dict(n_iter=int(rng.integers(1, 4)), method=str(rng.choice(["fft", "direct"])),
              remove_halo=bool(rng.integers(0, 2)), edgetaping=bool(rng.integers(0, 2)),
              prefiltering=bool(rng.integers(0, 2)), discard_saturation=bool(rng.integers(0, 2)),
              q=float(rng.choice([0.0, 0.0, 1e-3, 0.02])))
    if kw["prefiltering"]:
        kw["prefilter"] = str(rng.choice(["bilateral", "domain_transform"]))
    coef = dict(c=float(rng.uniform(0.3, 0.4)), b=float(rng.uniform(0.4, 0.8)), alpha=float(rng.choice([2, 4, 6])),
                beta=float(rng.choice([1, 3, 4])))
    return (B, C, H, W), kw, coef


@pytest.mark.parametrize("i", range(24))
def test_random_configurations(i):
    """seeded sweep over shapes x options x coefficients against the oracle (the goldens pin the oracle; this pins the
    engine on combinations the goldens do not enumerate)"""
    import torch
    from polyblur_amd import polyblur_deblurring
    (B, C, H, W), kw, coef = _random_case(i)
    x, _ = synthetic_blurry_batch(B, C, H, W, seed0=500 + 7 * i)
    got, infos = polyblur_deblurring(torch.from_numpy(x).cuda(), return_info=True, **kw, **coef)
    want, winfos = ref.polyblur_deblurring(x, return_info=True, **kw, **coef)
    same_theta = all(np.array_equal(a["theta"], b["theta"]) for a, b in zip(infos, winfos))
    err = maxabs(got.cpu().numpy(), want)
    # identical direction decisions -> rounding-level agreement; a near-tie in the argmin (possible on random data)
    # shows up as a different theta and is reported as such rather than hidden behind a loose tolerance
    assert same_theta, (kw, [(float(a["theta"][0]), float(b["theta"][0])) for a, b in zip(infos, winfos)])
    assert err < 5e-5, (err, kw, coef, (B, C, H, W))


def test_many_small_images_and_many_iterations():
    """grid sizing with B far above the CU count, and a long iteration chain"""
    import torch
    from polyblur_amd import polyblur_deblurring
    x, _ = synthetic_blurry_batch(4, 3, 40, 52, seed0=123)
    big = np.concatenate([x] * 75)                                    # B = 300
    out = polyblur_deblurring(torch.from_numpy(big).cuda(), n_iter=2, **KW).cpu().numpy()
    want = ref.polyblur_deblurring(x, n_iter=2, **KW)
    for i in (0, 1, 150, 299):
        assert maxabs(out[i], want[i % 4]) < 2e-5
    assert np.array_equal(out[:4], out[296:])
    # each iteration is polyblur applied to the previous result: 6 at once == 4 followed by 2, bit for bit
    xs = torch.from_numpy(x[:1]).cuda()
    six, infos = polyblur_deblurring(xs, n_iter=6, return_info=True, **KW)
    assert torch.equal(six, polyblur_deblurring(polyblur_deblurring(xs, n_iter=4, **KW), n_iter=2, **KW))
    want6, winfos = ref.polyblur_deblurring(x[:1], n_iter=6, return_info=True, **KW)
    # six sharpening passes (17 % of the samples end up clipped): the same six directions, and the fp32 tolerance
    # still holds (measured 4.4e-6; 5e-7 after one pass)
    assert [float(i["theta"][0]) for i in infos] == [float(i["theta"][0]) for i in winfos]
    assert maxabs(six.cpu().numpy(), want6) < 2e-5


def test_mixed_batch_rank1_and_general(eng):
    """one launch, images with different bodies and support classes (device-side dispatch per image)"""
    x, _ = synthetic_blurry_batch(5, 3, 140, 200, seed0=17)
    sig = [2.5, 0.6, 1.3, 3.0, 0.4]
    rho = [1.0, 0.6, 0.8, 3.0, 0.3]
    deg = [0.0, 48.0, 60.0, 12.0, 90.0]
    th = np.deg2rad(np.array(deg, np.float32)).astype(np.float32)
    for support in (capi.PB_SUPPORT_FULL, capi.PB_SUPPORT_ADAPTIVE):
        buf = eng.make_kernels(sig, rho, th, support=support)
        info = eng.read_info(buf, 5)
        assert list(info["separable"]) == [1, 1, 0, 1, 1]
        out = eng.inverse_filter(x, buf, 6.0, 1.0, capi.PB_WRAP)
        k = ref.gaussian_kernel_2d(th, np.array(sig, np.float32), np.array(rho, np.float32))
        want = ref.inverse_filtering_rank3(x, k[:, None], 6.0, 1.0, method="fft")
        assert maxabs(out, want) < 1e-5, support


def test_constant_image_is_guarded():
    """the reference returns NaN for a constant image (0/0 in normalize); the engine's
    clamp maps the NaN to 0, the estimate saturates at sigma = rho = 4 and the image is returned unchanged"""
    from polyblur_amd import polyblur_deblurring
    x = np.full((48, 64, 3), 0.5, np.float32)
    out = polyblur_deblurring(x, n_iter=2, **KW)
    assert np.isfinite(out).all() and maxabs(out, x) < 1e-6


def _strided(t):
    """the same values as a strided view of transposed storage"""
    v = t.transpose(-1, -2).contiguous().transpose(-1, -2)
    assert not v.is_contiguous() and v.shape == t.shape
    return v


@functools.lru_cache(maxsize=None)
def _front_end_cases():
    """name -> (operands as arrays, call(polyblur_amd, operands as tensors), the operands to differentiate): every public function,
    the differentiable ones with their gradients.  (2,3,24,40) images and a (1,1,5,7) kernel -- small, odd against every tile, more than
    one plane and image -- but for the first case, which is the one this test began with."""
    rng = np.random.default_rng(29)
    big, _ = synthetic_blurry_batch(2, 3, 64, 96, seed0=3)
    img, _ = synthetic_blurry_batch(2, 3, 24, 40, seed0=5)
    other = np.clip(img + rng.normal(0, 0.05, img.shape), 0, 1).astype(np.float32)
    gx, gy = (rng.normal(0, 0.1, img.shape).astype(np.float32) for _ in range(2))
    k = rng.random((1, 1, 5, 7)).astype(np.float32)
    k /= k.sum()
    ik = dict(img=img, kernel=k)
    halo = dict(img=img, kernel=k, gx=gx, gy=gy)
    blind = dict(n_iter=1, **KW)
    return {
        "polyblur_deblurring": (dict(img=big), lambda pa, o: pa.polyblur_deblurring(o["img"], **blind), None),
        "polyblur_deblurring-small": (dict(img=img), lambda pa, o: pa.polyblur_deblurring(o["img"], **blind), None),
        "polyblur_deblurring-float16": (dict(img=img.astype(np.float16)), lambda pa, o: pa.polyblur_deblurring(o["img"], **blind), None),
        "polyblur_deblurring_uint8": (dict(img=(img * 255).astype(np.uint8)), lambda pa, o: pa.polyblur_deblurring_uint8(o["img"], **blind), None),
        "PolyblurDeblurring": (dict(img=img), lambda pa, o: pa.PolyblurDeblurring()(o["img"], **blind), None),
        "PolyblurDeblurring-patches": (dict(img=img), lambda pa, o: pa.PolyblurDeblurring(True, 16, 0.25, 2)(o["img"], **blind), None),
        "polyblur_deblurring-n_iter=2-remove_halo": (dict(img=img), lambda pa, o: pa.polyblur_deblurring(o["img"], n_iter=2, remove_halo=True, **KW), ("img",)),
        "convolve2d": (ik, lambda pa, o: pa.convolve2d(o["img"], o["kernel"], method="direct"), ("img", "kernel")),
        "edgetaper": (ik, lambda pa, o: pa.edgetaper(o["img"], o["kernel"]), None),
        "compute_polynomial": (ik, lambda pa, o: pa.compute_polynomial(o["img"], o["kernel"], 6, 1), ("img", "kernel")),
        "compute_polynomial-not_symmetric": (ik, lambda pa, o: pa.compute_polynomial(o["img"], o["kernel"], 6, 1, not_symmetric=True), None),
        "inverse_filtering_rank3": (ik, lambda pa, o: pa.inverse_filtering_rank3(o["img"], o["kernel"], 6, 1, method="fft"), ("img", "kernel")),
        "inverse_filtering_rank3-remove_halo": (halo, lambda pa, o: pa.inverse_filtering_rank3(o["img"], o["kernel"], 6, 1, remove_halo=True,
                                                                                             grad_img=(o["gx"], o["gy"])), ("img", "kernel", "gx", "gy")),
        "inverse_filtering_rank3-do_edgetaper": (ik, lambda pa, o: pa.inverse_filtering_rank3(o["img"], o["kernel"], 6, 1, do_edgetaper=True, method="fft"), None),
        "inverse_filtering_nonsymmetric": (halo, lambda pa, o: pa.inverse_filtering_nonsymmetric(o["img"], o["kernel"], 6, 1, remove_halo=True,
                                                                                               grad_img=(o["gx"], o["gy"])), None),
        "gaussian_blur_estimation": (dict(img=img), lambda pa, o: pa.gaussian_blur_estimation(o["img"], q=0), ("img",)),
        "gaussian_blur_estimation-parameters": (dict(img=img), lambda pa, o: pa.gaussian_blur_estimation(o["img"], q=0, return_2d_filters=False), ("img",)),
        "fourier_gradients": (dict(img=img), lambda pa, o: pa.fourier_gradients(o["img"]), ("img",)),
        "halo_masking": (dict(img=img, imout=other, gx=gx, gy=gy), lambda pa, o: pa.halo_masking(o["img"], o["imout"], (o["gx"], o["gy"])),
                         ("img", "imout", "gx", "gy")),
        "halo_masking-own-gradients": (dict(img=img, imout=other), lambda pa, o: pa.halo_masking(o["img"], o["imout"]), ("img", "imout")),
    }


_FRONT_END = ["polyblur_deblurring", "polyblur_deblurring-small", "polyblur_deblurring-float16", "polyblur_deblurring_uint8", "PolyblurDeblurring",
              "PolyblurDeblurring-patches", "polyblur_deblurring-n_iter=2-remove_halo", "convolve2d", "edgetaper", "compute_polynomial",
              "compute_polynomial-not_symmetric", "inverse_filtering_rank3", "inverse_filtering_rank3-remove_halo",
              "inverse_filtering_rank3-do_edgetaper", "inverse_filtering_nonsymmetric", "gaussian_blur_estimation",
              "gaussian_blur_estimation-parameters", "fourier_gradients", "halo_masking", "halo_masking-own-gradients"]


def test_the_front_end_table_is_whole():
    assert sorted(_front_end_cases()) == sorted(_FRONT_END)


@pytest.mark.parametrize("name", _FRONT_END)
def test_non_contiguous_and_stream(eng, name):
    """every public function gives the same bits -- outputs and, where it is differentiable, every input gradient under a fixed
    upstream weight -- for contiguous ROCm tensors on the default stream, for strided views of transposed storage (image, kernel,
    imout and grad_img alike) and for contiguous tensors under torch.cuda.stream(side)"""
    import torch
    import polyblur_amd as pa
    arrays, call, leaves = _front_end_cases()[name]
    side = torch.cuda.Stream()

    def run(variant, grad):
        ops = {n: torch.from_numpy(a).cuda() for n, a in arrays.items()}
        if variant == "strided":
            ops = {n: _strided(t) for n, t in ops.items()}
        for n in (leaves if grad else ()):
            ops[n].requires_grad_(True)
        torch.cuda.synchronize()
        with torch.cuda.stream(side if variant == "stream" else torch.cuda.current_stream()), torch.set_grad_enabled(grad):
            out = call(pa, ops)
            outs = list(out) if isinstance(out, (tuple, list)) else [out]
            if grad:
                live = [o for o in outs if o.requires_grad]
                assert live and all(o.grad_fn is not None for o in live)
                rng = np.random.default_rng(31)                                  # (the same upstream weights for every variant)
                sum((o * torch.from_numpy(rng.uniform(-1, 1, tuple(o.shape)).astype(np.float32)).cuda()).sum() for o in live).backward()
        torch.cuda.synchronize()
        return [o.detach() for o in outs] + ([ops[n].grad for n in leaves] if grad else [])

    for grad in ((False, True) if leaves else (False,)):
        base = run("contiguous", grad)
        assert all(t is not None and bool(torch.isfinite(t.float()).all()) for t in base)
        for variant in ("strided", "stream"):
            got = run(variant, grad)
            assert len(got) == len(base)
            for i, (a, b) in enumerate(zip(base, got)):
                assert torch.equal(a, b), (name, variant, "grad" if grad else "no grad", i)


# ---------------------------------------------------------------------------------------------
# patch decomposition + Kaiser overlap-add (fix-forward of deblurring.py:269-340)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,ps,bs", [((2, 3, 150, 210), 64, 4), ((1, 3, 151, 211), 80, 1), ((1, 1, 90, 60), 100, 20)])
def test_patch_decomposition(shape, ps, bs):
    """the reference's patch branch raises NameError, so this is checked against the oracle's
    fix-forward restatement only ("unpinned"): lattice, replicate padding, periodic Kaiser window,
    normalised overlap-add, odd sizes cropped to even, image smaller than one patch"""
    import torch
    from polyblur_amd import PolyblurDeblurring
    x, _ = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=23)
    kw = dict(n_iter=2, c=0.362, b=0.468, alpha=6, beta=1)
    got = PolyblurDeblurring(patch_decomposition=True, patch_size=ps, patch_overlap=0.25, batch_size=bs)(
        torch.from_numpy(x).cuda(), **kw)
    want = ref.PolyblurDeblurring(patch_decomposition=True, patch_size=ps, patch_overlap=0.25)(x, **kw)
    assert tuple(got.shape) == want.shape == (shape[0], shape[1], shape[2] // 2 * 2, shape[3] // 2 * 2)
    assert maxabs(got.cpu().numpy(), want) < 3e-5
    # patches are independent images: grouping them differently must not change a bit
    got2 = PolyblurDeblurring(patch_decomposition=True, patch_size=ps, patch_overlap=0.25, batch_size=1)(
        torch.from_numpy(x).cuda(), **kw)
    assert torch.equal(got, got2)


# ---------------------------------------------------------------------------------------------
# 8-bit file edge (main.py:80-82,146): uint8 -> img_as_float32 -> polyblur -> img_as_ubyte, fused
# ---------------------------------------------------------------------------------------------
def _u8_image(c, h, w, seed):
    x, _ = synthetic_blurry_batch(1, c, h, w, seed0=seed)
    img = np.ascontiguousarray(ref.img_as_ubyte_from_float(np.moveaxis(x[0], 0, -1)))
    return np.ascontiguousarray(img[..., 0]) if c == 1 else img


@pytest.mark.parametrize("extra", [dict(n_iter=1), dict(n_iter=2), dict(n_iter=3), dict(n_iter=4, method="direct"),
                                   dict(n_iter=3, edgetaping=True), dict(n_iter=2, remove_halo=True),
                                   dict(n_iter=2, prefiltering=True), dict(n_iter=0)])
@pytest.mark.parametrize("c,h,w", [(3, 120, 164), (1, 97, 131)])
def test_uint8_edge(extra, c, h, w):
    from polyblur_amd import polyblur_deblurring, polyblur_deblurring_uint8
    img = _u8_image(c, h, w, seed=77)
    got = polyblur_deblurring_uint8(img, **KW, **extra)
    assert got.dtype == np.uint8 and got.shape == img.shape
    # (i) the fused byte load / store computes exactly what the float pipeline computes between host conversions
    via_float = ref.img_as_ubyte_from_float(polyblur_deblurring(ref.img_as_float32_from_ubyte(img), **KW, **extra))
    assert np.array_equal(got, via_float)
    # (ii) against the CPU restatement: a float difference of <= 2e-5 flips a rounding only next to a half level
    want = ref.polyblur_deblurring_uint8(img, **KW, **extra)
    d = np.abs(got.astype(np.int32) - want.astype(np.int32))
    assert d.max() <= 1 and np.mean(d != 0) < 2e-3, (int(d.max()), float(np.mean(d != 0)))


def test_uint8_planar_tensor_and_layout(eng):
    import torch
    from polyblur_amd import polyblur_deblurring_uint8
    imgs = np.stack([_u8_image(3, 90, 132, seed=s) for s in (5, 6)])                 # (B,H,W,C)
    planar = torch.from_numpy(np.ascontiguousarray(np.moveaxis(imgs, -1, 1))).cuda()    # (B,C,H,W) uint8
    out = polyblur_deblurring_uint8(planar, n_iter=3, **KW)
    assert out.dtype == torch.uint8 and out.is_cuda and out.shape == planar.shape
    for i in range(2):
        one = polyblur_deblurring_uint8(imgs[i], n_iter=3, **KW)
        assert np.array_equal(np.moveaxis(out[i].cpu().numpy(), 0, -1), one)
    # interleave / de-interleave round trip through the C ABI
    hwc = torch.from_numpy(imgs).cuda()
    chw, back = torch.empty_like(planar), torch.empty_like(hwc)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng._check(eng.lib.pb_u8_deinterleave(eng.ctx, hwc.data_ptr(), chw.data_ptr(), 2, 3, 90, 132))
    eng._check(eng.lib.pb_u8_interleave(eng.ctx, chw.data_ptr(), back.data_ptr(), 2, 3, 90, 132))
    torch.cuda.synchronize()
    assert torch.equal(chw, planar)
    assert torch.equal(back, hwc)
    with pytest.raises(TypeError):
        polyblur_deblurring_uint8(imgs[0].astype(np.float32))


@pytest.mark.parametrize("shape", [(1, 1, 8, 9), (1, 3, 16, 12), (1, 1, 20, 40), (2, 3, 25, 24)])
@pytest.mark.parametrize("boundary,method", [(capi.PB_WRAP, "fft"), (capi.PB_ZERO, "direct")])
def test_edgetaper_tiny_images(eng, shape, boundary, method):
    """padded axes shorter than 49 samples: the circular autocorrelation behind edgetaper's alpha (period n-1,
    edgetaper.py:11-15) wraps onto itself, z[p] = ac[p] + ac[n-1-p] -- both terms count"""
    rng = np.random.default_rng(3)
    x = rng.random(shape, dtype=np.float32)
    k = ref.gaussian_kernel_2d([np.float32(0.5)] * shape[0], [4.0] * shape[0], [2.0] * shape[0])
    xp = ref.replicate_pad(x, 12)
    buf = eng.set_kernels(k)
    out = eng.edgetaper(xp, buf, boundary)
    want = ref.edgetaper(xp, k[:, None], method=method)
    assert maxabs(out, want) < 1e-5, maxabs(out, want)


def test_verbose_prints_stage_times(eng, capsys):
    from polyblur_amd import polyblur_deblurring
    x, _ = synthetic_blurry_batch(1, 3, 96, 128, seed0=5)
    polyblur_deblurring(x[0].transpose(1, 2, 0), n_iter=2, verbose=True, **KW)
    text = capsys.readouterr().out
    assert "-- blur estimation:" in text and "-- deblurring:" in text and "stencil passes" in text


def test_streams_and_threads_do_not_share_scratch(eng):
    """two torch streams alternate on one engine (pb_set_stream orders the scratch hand-over), and a second host
    thread gets its own context: results equal the single-stream ones bit for bit"""
    import threading
    import torch
    from polyblur_amd import polyblur_deblurring
    from polyblur_amd.engine import get_engine
    xs = [torch.from_numpy(synthetic_blurry_batch(1, 3, 200, 264, seed0=s)[0]).cuda() for s in (1, 2, 3, 4)]
    want = [polyblur_deblurring(x, n_iter=2, **KW) for x in xs]
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    got = [None] * 4
    for rep in range(3):
        for i, x in enumerate(xs):
            with torch.cuda.stream(s1 if i % 2 == 0 else s2):
                got[i] = polyblur_deblurring(x, n_iter=2, **KW)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(got, want))
    res = {}

    def worker():
        res["eng"] = get_engine(0)
        res["out"] = polyblur_deblurring(xs[0], n_iter=2, **KW)
        torch.cuda.synchronize()
    t = threading.Thread(target=worker)
    t.start()
    other = [polyblur_deblurring(x, n_iter=2, **KW) for x in xs[1:]]
    t.join()
    torch.cuda.synchronize()
    assert res["eng"] is not eng and torch.equal(res["out"], want[0])
    assert all(torch.equal(a, b) for a, b in zip(other, want[1:]))


@pytest.mark.parametrize("k", [5, 13, 21, 4, 12, 24, 31, 36, 49])
@pytest.mark.parametrize("method", ["fft", "direct"])
def test_kernel_sizes_against_reference_goldens(golden, k, method):
    """ker_size != 25 (deblurring.py:23): the estimated Gaussian is k x k and the replicate pad k // 2, so the wrap /
    zero boundary of the three reblurring passes sits closer to the image (or further: sizes above 25 take the
    large-kernel pass, csrc/conv_big.hip)"""
    import torch
    from polyblur_amd import polyblur_deblurring
    g = golden("pipeline_kersize.npz")
    out = polyblur_deblurring(torch.from_numpy(g["x"]).cuda(), n_iter=2, ker_size=k, method=method, **KW).cpu().numpy()
    assert maxabs(out, g["k%d_%s" % (k, method)]) < 2e-5
    if k == 13 and method == "fft":
        out = polyblur_deblurring(torch.from_numpy(g["x"]).cuda(), n_iter=2, ker_size=13, edgetaping=True, remove_halo=True,
                                  **KW).cpu().numpy()
        assert maxabs(out, g["k13_fft_taper_halo"]) < 2e-5


@pytest.mark.parametrize("k", [4, 12, 24, 36])
@pytest.mark.parametrize("method", ["fft", "direct"])
def test_even_kernel_sizes_link_by_link(golden, k, method):
    """the ill-conditioned corner: even ker_size, three iterations.  The off-centre Gaussian's 'fft' transform
    carries a half-sample phase (blur_estimation.py:221-223, filters.py:255-273) and every iteration amplifies the rounding
    differences of the earlier ones 5-10 x, so the engine is held link by link -- one iteration on the REFERENCE's input of
    that iteration -- to the plain fp32 tolerance, and the chained call to 3e-4 (tests/golden/make_golden_kersize_chain.py)."""
    import torch
    from polyblur_amd import polyblur_deblurring
    g = golden("pipeline_kersize_chain.npz")
    kw = dict(ker_size=k, method=method, **KW)
    xs = [g["x0"]] + [g["k%d_%s_x%d" % (k, method, i)] for i in (1, 2, 3)]
    for i in range(3):
        out = polyblur_deblurring(torch.from_numpy(xs[i]).cuda(), n_iter=1, **kw).cpu().numpy()
        assert maxabs(out, xs[i + 1]) < 2e-5, (k, method, i, maxabs(out, xs[i + 1]))
    out = polyblur_deblurring(torch.from_numpy(xs[0]).cuda(), n_iter=3, **kw).cpu().numpy()
    assert maxabs(out, xs[3]) < 3e-4


@pytest.mark.parametrize("k", [4, 12, 24])
@pytest.mark.parametrize("method", ["fft", "direct"])
def test_even_kernel_sizes_with_edgetaping(golden, k, method):
    """the reference's edgetaper takes a kernel of any size (edgetaper.py:10-23); an even ker_size with
    edgetaping=True raised PB_ERR_UNSUPPORTED until round 6 (the record's autocorrelations were those of SYMMETRISED projections,
    and an even size sits off-centre).  Link by link against the reference's own outputs (tests/golden/make_golden_even_taper.py),
    the two links chained, and the oracle on another image."""
    import torch
    from polyblur_amd import polyblur_deblurring
    g = golden("pipeline_even_taper.npz")
    kw = dict(ker_size=k, method=method, edgetaping=True, **KW)
    xs = [g["x0"]] + [g["k%d_%s_x%d" % (k, method, i)] for i in (1, 2)]
    for i in range(2):
        out = polyblur_deblurring(torch.from_numpy(xs[i]).cuda(), n_iter=1, **kw).cpu().numpy()
        assert maxabs(out, xs[i + 1]) < 2e-5, (k, method, i, maxabs(out, xs[i + 1]))
    out = polyblur_deblurring(torch.from_numpy(xs[0]).cuda(), n_iter=2, **kw).cpu().numpy()
    assert maxabs(out, xs[2]) < 1e-4
    x, _ = synthetic_blurry_batch(2, 3, 150, 200, seed0=63)
    out = polyblur_deblurring(torch.from_numpy(x).cuda(), n_iter=1, **kw).cpu().numpy()
    assert maxabs(out, ref.polyblur_deblurring(x, n_iter=1, **kw)) < 2e-5


@pytest.mark.parametrize("k", [31, 48])
@pytest.mark.parametrize("method", ["fft", "direct"])
def test_large_kernel_sizes_with_edgetaping(golden, k, method):
    """a ker_size above 25 with edgetaping=True (the reference's edgetaper takes any size, edgetaper.py:10-23):
    the blends run through csrc/conv_big.hip with the weights of the large kernel's own autocorrelations.  Link by link against
    the reference's outputs (tests/golden/make_golden_big_taper.py), the two links chained, and the oracle on a batch with
    other dtypes' worth of options (halo masking behind the polynomial)."""
    import torch
    from polyblur_amd import polyblur_deblurring
    g = golden("pipeline_big_taper.npz")
    kw = dict(ker_size=k, method=method, edgetaping=True, **KW)
    xs = [g["x0"]] + [g["k%d_%s_x%d" % (k, method, i)] for i in (1, 2)]
    for i in range(2):
        out = polyblur_deblurring(torch.from_numpy(xs[i]).cuda(), n_iter=1, **kw).cpu().numpy()
        assert maxabs(out, xs[i + 1]) < 2e-5, (k, method, i, maxabs(out, xs[i + 1]))
    out = polyblur_deblurring(torch.from_numpy(xs[0]).cuda(), n_iter=2, **kw).cpu().numpy()
    assert maxabs(out, xs[2]) < (1e-4 if k % 2 == 0 else 3e-5)
    x, _ = synthetic_blurry_batch(2, 3, 130, 170, seed0=65)
    out = polyblur_deblurring(torch.from_numpy(x).cuda(), n_iter=1, remove_halo=True, **kw).cpu().numpy()
    assert maxabs(out, ref.polyblur_deblurring(x, n_iter=1, remove_halo=True, **kw)) < 2e-5


@pytest.mark.parametrize("k,shape", [(3, (1, 1, 9, 11)), (9, (2, 3, 40, 33)), (23, (1, 3, 70, 64)), (2, (1, 3, 20, 17)), (8, (2, 1, 33, 40)), (22, (1, 3, 64, 70)),
                                     (27, (2, 3, 70, 133)), (26, (1, 1, 40, 33)), (48, (1, 3, 150, 97)), (49, (2, 1, 20, 30)), (35, (1, 3, 300, 517))])
def test_kernel_sizes_against_oracle(k, shape):
    import torch
    from polyblur_amd import polyblur_deblurring
    x, _ = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=61)
    for method in ("fft", "direct"):
        out, infos = polyblur_deblurring(torch.from_numpy(x).cuda(), n_iter=2, ker_size=k, method=method, return_info=True, **KW)
        want, winfos = ref.polyblur_deblurring(x, n_iter=2, ker_size=k, method=method, return_info=True, **KW)
        assert [float(i["theta"][0]) for i in infos] == [float(i["theta"][0]) for i in winfos]
        assert maxabs(out.cpu().numpy(), want) < 2e-5, (k, method)


# ---------------------------------------------------------------------------------------------
# method='direct_separable': the opt-in x-t separable APPROXIMATION (intent of separable_gaussian2d.cpp:91-183).
# Parity is against the oracle's restatement of the same approximation (unpinned: the reference's own code for this path
# does not run); its distance to the exact 'direct' result is the method's stated tolerance.
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,seed", [((1, 3, 96, 128), 3), ((2, 1, 70, 90), 8), ((1, 3, 200, 264), 12)])
def test_direct_separable_matches_its_oracle(shape, seed):
    import torch
    from polyblur_amd import polyblur_deblurring
    x, _ = synthetic_blurry_batch(shape[0], shape[1], shape[2], shape[3], seed0=seed)
    out, infos = polyblur_deblurring(torch.from_numpy(x).cuda(), n_iter=3, method="direct_separable", return_info=True, **KW)
    want, winfos = ref.polyblur_deblurring(x, n_iter=3, method="direct_separable", return_info=True, **KW)
    for k in range(shape[0]):
        assert [float(i["theta"][k]) for i in infos] == [float(i["theta"][k]) for i in winfos]
    assert maxabs(out.cpu().numpy(), want) < 3e-5
    # stated tolerance of the approximation itself: within 5e-2 of the exact zero-boundary result, 5e-3 on average
    exact = polyblur_deblurring(torch.from_numpy(x).cuda(), n_iter=3, method="direct", **KW).cpu().numpy()
    d = np.abs(out.cpu().numpy() - exact)
    assert d.max() < 5e-2 and d.mean() < 5e-3, (d.max(), d.mean())


def test_direct_separable_mixed_batch_default_build():
    """the default library runs method='direct_separable' as two launches of the general body (the one-launch
    csrc/conv_xt.hip is in the --experimental build only), which has no pass of its own for images whose exact kernel is
    rank-1.  A batch that mixes a rank-1 blur (theta = 0), an oblique one and an isotropic one: against the oracle's x-t
    restatement (intent of separable_gaussian2d.cpp:91-183), identical theta sequences, and every image bit for bit what it
    gets alone."""
    import torch
    from polyblur_amd import polyblur_deblurring
    from polyblur_amd.synthetic import synthetic_blurry_image
    x = np.stack([synthetic_blurry_image(3, 150, 210, 500 + i, blur=b)[0]
                  for i, b in enumerate([(2.0, 1.0, 0.0), (2.0, 1.0, 30.0), (1.5, 1.5, 0.0), (2.5, 0.8, 90.0)])]).astype(np.float32)
    kw = dict(n_iter=2, method="direct_separable", **KW)
    out, infos = polyblur_deblurring(torch.from_numpy(x).cuda(), return_info=True, **kw)
    want, winfos = ref.polyblur_deblurring(x, return_info=True, **kw)
    for k in range(x.shape[0]):
        assert [float(i["theta"][k]) for i in infos] == [float(i["theta"][k]) for i in winfos]
        alone = polyblur_deblurring(torch.from_numpy(x[k:k + 1]).cuda(), **kw)
        assert torch.equal(alone, out[k:k + 1]), k
    assert maxabs(out.cpu().numpy(), want) < 3e-5


@pytest.mark.parametrize("sigma,rho,deg", [(2.0, 1.0, 30.0), (4.0, 0.3, 42.0), (0.74, 0.4, 24.0), (3.0, 2.0, 66.0), (2.0, 1.0, 0.0),
                                           (3.5, 0.5, 96.0), (1.5, 1.5, 48.0)])
def test_direct_separable_records(eng, sigma, rho, deg):
    """the two 1-D kernels built on the device equal the oracle's; both run as short phase lists of the general body"""
    import ctypes as C
    th = np.deg2rad(np.float32(deg))
    base = eng.make_kernels([sigma], [rho], [th])
    sep = eng.info_buffer("np.sep", 2)
    eng._check(eng.lib.pb_make_separable_kernels(eng.ctx, 1, C.c_void_p(base.ptr), C.c_void_p(sep.ptr), capi.PB_SUPPORT_FULL, 25))
    rec = eng.read_info(sep, 2)
    k1, k2 = ref.separable_xt_kernels([th], [sigma], [rho])
    assert maxabs(rec["kernel"][0], k1[0]) < 1e-6 and maxabs(rec["kernel"][1], k2[0]) < 2e-6
    assert rec["separable"][0] == 0 and rec["nphase"][0].sum() <= 26     # the 1-D pass: one kernel row (7 phases) or one column (25), + filler
    if deg % 90 != 0 and sigma != rho:
        assert rec["separable"][1] == 0 and 0 < rec["nphase"][1].sum() <= 80


def test_half_temporaries_option():
    """fp16 images with fp16 Horner temporaries (opt-in).  The temporaries reach |a2| = 9 times the image range, where an
    fp16 ulp is 7.8e-3: stated tolerance 8e-3 against the fp32 oracle on the fp16-rounded input (the default, fp32
    temporaries, holds 1e-3), same theta sequence; also with halo + domain-transform prefilter"""
    import torch
    from polyblur_amd import polyblur_deblurring
    x16 = synthetic_blurry_batch(2, 3, 150, 200, seed0=71)[0].astype(np.float16)
    xt = torch.from_numpy(x16).cuda()
    for kw in (dict(), dict(remove_halo=True, prefiltering=True, prefilter="domain_transform")):
        a, ia = polyblur_deblurring(xt, n_iter=3, return_info=True, **KW, **kw)
        b, ib = polyblur_deblurring(xt, n_iter=3, return_info=True, temporaries="fp16", **KW, **kw)
        want = ref.polyblur_deblurring(x16.astype(np.float32), n_iter=3, **KW, **kw)
        assert [float(i["theta"][0]) for i in ia] == [float(i["theta"][0]) for i in ib]
        assert maxabs(a.float().cpu().numpy(), want) < 1e-3
        assert maxabs(b.float().cpu().numpy(), want) < 8e-3
    with pytest.raises(ValueError):
        polyblur_deblurring(xt.float(), temporaries="fp16", **KW)


def test_direct_separable_fp16_and_kernel_size():
    """the one-launch x-t pass with fp16 images (fp16 window / operand loads, fp16 store) and with a 13 x 13 kernel
    (replicate pad 6: the patch of the intermediate image is cleared outside a smaller padded domain)"""
    import torch
    from polyblur_amd import polyblur_deblurring
    x = synthetic_blurry_batch(2, 3, 120, 150, seed0=14)[0]
    x16 = x.astype(np.float16)
    out = polyblur_deblurring(torch.from_numpy(x16).cuda(), n_iter=3, method="direct_separable", **KW)
    want = ref.polyblur_deblurring(x16.astype(np.float32), n_iter=3, method="direct_separable", **KW)
    assert out.dtype == torch.float16 and maxabs(out.float().cpu().numpy(), want) < 1e-3
    out = polyblur_deblurring(torch.from_numpy(x).cuda(), n_iter=2, method="direct_separable", ker_size=13, **KW)
    want = ref.polyblur_deblurring(x, n_iter=2, method="direct_separable", ker_size=13, **KW)
    assert maxabs(out.cpu().numpy(), want) < 3e-5
    # tiny image: every tile is a border tile
    xs = synthetic_blurry_batch(1, 1, 20, 30, seed0=15)[0]
    out = polyblur_deblurring(torch.from_numpy(xs).cuda(), n_iter=2, method="direct_separable", **KW)
    want = ref.polyblur_deblurring(xs, n_iter=2, method="direct_separable", **KW)
    assert maxabs(out.cpu().numpy(), want) < 3e-5


def test_large_kernel_size_with_options_and_dtypes():
    """ker_size above 25 with halo removal, a prefilter, quantiles, fp16 and 8-bit images (every dtype combination of the
    large-kernel pass); 'direct_separable' is not built for it"""
    import torch
    from polyblur_amd import polyblur_deblurring, polyblur_deblurring_uint8
    x, _ = synthetic_blurry_batch(2, 3, 120, 176, seed0=62)
    kw = dict(n_iter=2, ker_size=33, remove_halo=True, prefiltering=True, q=1e-3, **KW)
    out = polyblur_deblurring(torch.from_numpy(x).cuda(), **kw).cpu().numpy()
    assert maxabs(out, ref.polyblur_deblurring(x, **kw)) < 3e-5
    kw = dict(n_iter=2, ker_size=29, **KW)
    want = ref.polyblur_deblurring(x, **kw)
    out16 = polyblur_deblurring(torch.from_numpy(x).cuda().half(), **kw).float().cpu().numpy()
    assert maxabs(out16, ref.polyblur_deblurring(x.astype(np.float16).astype(np.float32), **kw)) < 1e-3
    outh = polyblur_deblurring(torch.from_numpy(x).cuda().half(), temporaries="fp16", **kw).float().cpu().numpy()
    assert maxabs(outh, want) < 8e-3
    u8 = np.ascontiguousarray((x[0].transpose(1, 2, 0) * 255).round().astype(np.uint8))
    got = polyblur_deblurring_uint8(u8, **kw)
    wantu = ref.polyblur_deblurring_uint8(u8, **kw)
    assert np.mean(got != wantu) < 2e-3 and np.abs(got.astype(int) - wantu.astype(int)).max() <= 1
    hwc = np.ascontiguousarray(x[0].transpose(1, 2, 0))
    with pytest.raises(NotImplementedError):
        polyblur_deblurring(hwc, ker_size=31, method="direct_separable")
    with pytest.raises(NotImplementedError):
        polyblur_deblurring(hwc, ker_size=51)

