"""CPU checks of tests/window_ref.py, the float64 reference and the case tables of tests/test_gpu_window_conformance.py: the
restated halo rule against the halo pairs the GPU tests pin, the margin of every tap set the sweeps dial, and -- for every
(input, taps, coefficients) the GPU file compares on -- that the clamp is out of the picture and that the reference agrees
with the project's fp32 oracle.

Measured over the cases below: the fp32 oracle (complex64 after every transform) against clip(reference64) 8.1e-7 at most;
no sample of any reference at or beyond the clamp (range [0.08, 0.91])."""
import numpy as np
import pytest

import window_ref as wr
from oracle import polyblur_ref as ref

# (theta deg, sigma, rho) -> composite halos under alpha = 6, beta = 1, as tests/test_gpu_onepass.py::KERNELS and
# tests/test_gpu_tall_windows.py::RECORDS pin them on the GPU
PINNED = [
    ((66.0, 2.095, 1.314), (16, 20)), ((66.0, 1.656, 1.009), (12, 16)), ((66.0, 1.240, 0.625), (8, 12)),
    ((0.0, 1.4, 0.9), (16, 10)), ((30.0, 0.65, 0.40), (8, 6)), ((0.0, 0.3, 0.3), (4, 4)), ((90.0, 1.2, 0.5), (8, 12)),
    ((45.0, 3.0, 1.0), (24, 24)), ((20.0, 0.3, 0.15), (4, 2)), ((10.0, 1.2, 4.0), (16, 36)), ((10.0, 1.7, 3.0), (20, 30)),
]
TOL_ORACLE = 1e-6
CLAMP_SHARE = 1e-3


@pytest.mark.parametrize("record,want", PINNED)
def test_composite_halos_of_the_pinned_gaussians(record, want):
    deg, sigma, rho = record
    f = lambda v: np.array([v], np.float32)
    k = ref.gaussian_kernel_2d(f(np.deg2rad(deg)), f(sigma), f(rho))[0]
    got, _ = wr.composite_halos(k, wr.ALPHA, wr.BETA)
    assert got == want, (record, got)


def test_every_halo_pair_is_dialled_with_margin():
    """the whole grid: the tap set the sweeps take for (hx, hy) has these halos under the restated rule, with the margin an fp32
    evaluation of the rule cannot cross, under both coefficient pairs the GPU file uses"""
    for hx in wr.HX:
        for hy in wr.HY:
            k = wr.taps_for(hx, hy)                         # (dial_taps asserts the margin under alpha = 6, beta = 1)
            assert k.dtype == np.float32 and k.shape == (25, 25) and (k >= 0).all() and np.array_equal(k, k[::-1, ::-1])
            assert abs(float(k.astype(np.float64).sum()) - 1.0) < 1e-6
            got, margins = wr.composite_halos(k, wr.ALPHA, wr.BETA)
            assert got == (hx, hy), (hx, hy, got)
            assert all(i >= 10.0 and a <= 0.1 for i, a in margins), (hx, hy, margins)
            _, margins = wr.composite_halos(k, wr.ALPHA2, wr.BETA2)
            assert all(i >= 10.0 and a <= 0.1 for i, a in margins), (hx, hy, margins)


def test_hard_and_soft_radii():
    """a hard box has composite radius 3 r, a soft ring 3 r - 2 (2 r and 2 r - 1 where a3 = 0)"""
    for r in range(2, 13):
        for soft, raw3, raw2 in ((False, 3 * r, 2 * r), (True, 3 * r - 2, 2 * r - 1)):
            k = wr.dial_taps(r, r, soft, 5)
            for coef, raw in (((wr.ALPHA, wr.BETA), raw3), ((wr.ALPHA2, wr.BETA2), raw2)):
                assert wr.composite_halos(k, *coef)[0] == (max(4, (raw + 3) // 4 * 4), max(2, (raw + 1) // 2 * 2)), (r, soft, coef)


def test_forms_admit_what_the_constants_say():
    assert wr.admitted_values("pairs") == (tuple(range(4, 21, 4)), tuple(range(2, 25, 2)))
    assert wr.admitted_values("tall") == (tuple(range(4, 21, 4)), wr.HY)
    assert wr.admitted_values("w128") == (wr.HX, wr.HY)
    assert not wr.admits("pairs", 20, 24) and wr.admits("pairs", 20, 16) and not wr.admits("pairs", 20, 18)
    assert wr.admits("tall", 20, 32) and not wr.admits("tall", 20, 34) and wr.admits("tall", 16, 36)


def test_inputs():
    x = wr.flat((1, 3, 64, 64), 3)
    assert 0.4 <= x.min() and x.max() <= 0.6 and abs(x.std() - 0.2 / np.sqrt(12)) < 2e-3
    y = wr.impulses((1, 1, 40, 60))
    assert y[0, 0, 0, 0] == 0.8 and (y == 0.8).sum() == 5 and ((y == 0.5) | (y == 0.8)).all()


def _cases():
    seen, out = set(), []
    for key, coef, kind, shape in wr.all_fp32_cases():
        if (key, coef, kind, shape) not in seen:
            seen.add((key, coef, kind, shape))
            out.append((key, coef, kind, shape))
    return out


@pytest.mark.parametrize("part", range(8))
def test_clamp_share_and_oracle_distance(part):
    """every case of the GPU file: at most 0.1 % of the float64 reference's samples at or beyond the clamp (so the comparison sees
    the filter, not the clamp), and clip(reference64) within 1e-6 of the fp32 oracle"""
    worst, lo, hi = 0.0, 1.0, 0.0
    for key, coef, kind, shape in _cases()[part::8]:
        x = wr.case_input(kind, key, shape)
        k = wr.taps_for(*key)
        y = wr.reference64(x, k[None], *coef)
        share = float(np.mean((y <= 0.0) | (y >= 1.0)))
        assert share <= CLAMP_SHARE, (key, coef, kind, shape, share)
        want = ref.inverse_filtering_rank3(x.astype(np.float32), k[None, None], coef[0], coef[1], method="fft")
        d = float(np.max(np.abs(np.clip(y, 0.0, 1.0) - want)))
        worst, lo, hi = max(worst, d), min(lo, float(y.min())), max(hi, float(y.max()))
        assert d < TOL_ORACLE, (key, coef, kind, shape, d)
    print("window_ref part %d: oracle against clip(reference64) %.3g at most, reference range [%.3f, %.3f]" % (part, worst, lo, hi))


def test_clamp_share_and_oracle_distance_of_the_batches():
    for shape, keys in wr.BATCHES:
        x = wr.flat_image(shape, wr.BATCH_SEED)
        k = np.stack([wr.taps_for(*key) for key in keys])
        y = wr.reference64(x, k, wr.ALPHA, wr.BETA)
        assert float(np.mean((y <= 0.0) | (y >= 1.0))) <= CLAMP_SHARE, shape
        want = ref.inverse_filtering_rank3(x, k[:, None], wr.ALPHA, wr.BETA, method="fft")
        assert float(np.max(np.abs(np.clip(y, 0.0, 1.0) - want))) < TOL_ORACLE, shape


def test_domain_variant():
    """domain=True is the same filter on the plane as given: equal to the padded form on a plane that is its own replicate pad"""
    k = wr.taps_for(12, 8)
    x = wr.flat((1, 1, 40, 52), 11)
    y = wr.reference64(x, k[None], 6.0, 1.0, domain=True)
    Y = np.fft.fft2(x)
    K = np.fft.fft2(np.roll(np.pad(k.astype(np.float64), [(0, 15), (0, 27)]), (-12, -12), axis=(0, 1)))
    t = np.fft.ifft2(K * Y).real
    want = 4.0 * np.fft.ifft2(K * K * K * Y).real - 9.0 * np.fft.ifft2(K * K * Y).real + 5.0 * t + x
    assert np.max(np.abs(y - want)) < 1e-13
    # against a direct circular correlation at a few samples
    kk = k.astype(np.float64)
    for (r, c) in ((0, 0), (17, 30), (39, 51)):
        s = sum(kk[i, j] * x[0, 0, (r + i - 12) % 40, (c + j - 12) % 52] for i in range(25) for j in range(25))
        assert abs(s - t[0, 0, r, c]) < 1e-13
