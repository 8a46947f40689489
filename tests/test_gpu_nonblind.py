"""The non-blind entry points with a kernel of the caller's -- any kh x kw with 1 <= kh <= 49, 2 <= kw <= 49 -- on the GPU:
polyblur_amd.inverse_filtering_rank3 / convolve2d / edgetaper and the Engine's kernel sets (pb_taps) against the reference's
own outputs (tests/golden/nonblind*.npz) and against the CPU oracle, which tests/test_nonblind_cpu.py pins to those goldens.

Tolerances are the project's own for caller-supplied taps (test_caller_kernels_that_are_not_point_symmetric): convolve2d
< 2e-6, edgetaper < 4e-6, inverse filter < 2e-5, fp16 images < 1e-3.  For scale: on the goldens' inputs the reference and the
oracle -- two independent fp32 evaluations -- differ by at most 5.4e-7 (convolve2d), 4.5e-7 (edgetaper) and 1.3e-6 (inverse
filter, the 2401-tap dense kernels, taper and halo included), as tests/golden/make_golden_nonblind.py prints; over the full
list of shapes below the issue that asked for this measured 6.3e-7, 6.9e-7 and 1.5e-6.
Measured on an MI355X over every case of this file: convolve2d <= 1.5e-6, edgetaper <= 1.2e-6, inverse filter <= 3.2e-6, fp16
images <= 2.5e-4 (half an fp16 ulp at 0.5).

The final clamp must not hide errors: every inverse-filter comparison asserts that at most 1 % of the oracle's samples sit at
exactly 0 or 1 (the images are rescaled to 0.3 + 0.4 x for that; the goldens' worst case is 0.09 %).

Kernels: rng.random(shape) ** 3, normalised -- dense and not point-symmetric, so a misplaced or unreflected tap shows."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from oracle import polyblur_ref as ref                      # the checker (tests only)
from polyblur_amd import _capi as capi
from polyblur_amd.synthetic import synthetic_blurry_batch

ALPHA, BETA = 2, 3
TOL_CONV, TOL_TAPER, TOL_INV, TOL_HALF = 2e-6, 4e-6, 2e-5, 1e-3
SHAPES = [(49, 49), (26, 26), (3, 49), (49, 3), (27, 5), (8, 8), (1, 2), (25, 24), (13, 13), (48, 31)]


@pytest.fixture(scope="module")
def eng():
    from polyblur_amd.engine import get_engine
    return get_engine(0)


@pytest.fixture(scope="module")
def image(golden):
    return golden("nonblind.npz")["x"]                      # (1,3,50,70), already 0.3 + 0.4 x


def maxabs(a, b):
    return float(np.max(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))))


def make_kernel(shape, seed, batch=1, channels=1):
    k = np.random.default_rng(seed).random((batch, channels) + tuple(shape)) ** 3
    return (k / k.sum(axis=(-2, -1), keepdims=True)).astype(np.float32)


def rescaled_batch(b, c, h, w, seed0):
    x, _ = synthetic_blurry_batch(b, c, h, w, seed0=seed0)
    return (0.3 + 0.4 * x).astype(np.float32)


def check_inverse(got, want, tol, what):
    """the comparison, behind the clamp condition: at most 1 % of the oracle's samples at exactly 0 or 1"""
    clamped = float(np.mean((want == 0) | (want == 1)))
    err = maxabs(got, want)
    print(what, "err %.3g" % err, "clamped %.2f %%" % (100 * clamped))
    assert clamped <= 0.01, (what, clamped)
    assert err < tol, (what, err)


def oracle_inverse(x, k, method, full):
    """the oracle, channel by channel where the kernel has one plane per channel"""
    kw = dict(method=method, do_edgetaper=full, remove_halo=full)
    if k.shape[1] == 1:
        return ref.inverse_filtering_rank3(x, np.broadcast_to(k, (x.shape[0],) + k.shape[1:]), ALPHA, BETA, **kw)
    kb = np.broadcast_to(k, (x.shape[0],) + k.shape[1:])
    return np.concatenate([ref.inverse_filtering_rank3(x[:, c:c + 1], kb[:, c:c + 1], ALPHA, BETA, **kw) for c in range(k.shape[1])], axis=1)


# ---------------------------------------------------------------------------------------------
# the reference's own outputs
# ---------------------------------------------------------------------------------------------
def test_inverse_filter_against_reference_goldens(golden):
    from polyblur_amd import inverse_filtering_rank3
    d = golden("nonblind.npz")
    x, n = d["x"], 0
    for name in d.files:
        if not name.startswith("inv_"):
            continue
        p = name.split("_")
        if p[1] == "correlate":
            got = inverse_filtering_rank3(x, d["k_" + p[2]], ALPHA, BETA, correlate=True, method=p[3])
        elif p[1] == "perchannel":
            got = inverse_filtering_rank3(x, d["k_perchannel_" + p[2]], ALPHA, BETA, remove_halo=True, method=p[3])
        else:
            full = p[3] == "full"
            got = inverse_filtering_rank3(x, d["k_" + p[1]], ALPHA, BETA, remove_halo=full, do_edgetaper=full, method=p[2])
        check_inverse(got, d[name], TOL_INV, name)
        n += 1
    assert n == 18


def test_stages_against_reference_goldens(golden):
    from polyblur_amd import convolve2d, edgetaper
    d = golden("nonblind.npz")
    for fname, fn, tol in (("nonblind_conv.npz", convolve2d, TOL_CONV), ("nonblind_taper.npz", edgetaper, TOL_TAPER)):
        s = golden(fname)
        assert len(s.files) == 4
        for name in s.files:
            _, shape, method = name.split("_")
            k = d["k_" + shape]
            got = fn(ref.replicate_pad(d["x"], k.shape[-1] // 2), k, method=method)
            err = maxabs(got, s[name])
            print(name, "err %.3g" % err)
            assert err < tol, (name, err)


# ---------------------------------------------------------------------------------------------
# the oracle, every shape
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("method", ["fft", "direct"])
@pytest.mark.parametrize("shape", SHAPES + [(11, 6)], ids=lambda s: "%dx%d" % s)       # (11 x 6: taller than wide within 25 x 25)
def test_every_shape_against_oracle(image, shape, method):
    from polyblur_amd import inverse_filtering_rank3, convolve2d, edgetaper
    x = image
    k = make_kernel(shape, 7300 + 100 * shape[0] + shape[1])
    # a kernel taller than wide under 'fft': the plain polynomial only (the stages' circular pad by the half-width is refused)
    stages = not (method == "fft" and shape[0] // 2 > shape[1] // 2)
    if stages:
        xp = ref.replicate_pad(x, shape[1] // 2)
        err = maxabs(convolve2d(xp, k, method=method), ref.convolve2d(xp, k, method=method))
        print("convolve2d err %.3g" % err)
        assert err < TOL_CONV, err
        err = maxabs(edgetaper(xp, k, method=method), ref.edgetaper(xp, k, method=method))
        print("edgetaper err %.3g" % err)
        assert err < TOL_TAPER, err
    else:
        with pytest.raises(NotImplementedError):
            convolve2d(x, k, method=method)
        with pytest.raises(NotImplementedError):
            inverse_filtering_rank3(x, k, ALPHA, BETA, do_edgetaper=True, method=method)
    check_inverse(inverse_filtering_rank3(x, k, ALPHA, BETA, method=method), oracle_inverse(x, k, method, False), TOL_INV, "plain")
    if stages:
        check_inverse(inverse_filtering_rank3(x, k, ALPHA, BETA, remove_halo=True, do_edgetaper=True, method=method),
                      oracle_inverse(x, k, method, True), TOL_INV, "taper + halo")


# ---------------------------------------------------------------------------------------------
# batches, planes, tiles, types
# ---------------------------------------------------------------------------------------------
def test_two_images_two_kernels():
    """B = 2, C = 3, two different 31 x 9 kernels: image and plane indexing of the large-kernel pass (taller than wide: every
    call under 'direct', the plain polynomial under 'fft')"""
    from polyblur_amd import inverse_filtering_rank3, convolve2d, edgetaper
    x = rescaled_batch(2, 3, 41, 53, 7400)
    k = make_kernel((31, 9), 7401, batch=2)
    assert maxabs(k[0], k[1]) > 1e-3
    xp = ref.replicate_pad(x, 4)
    assert maxabs(convolve2d(xp, k, method="direct"), ref.convolve2d(xp, k, method="direct")) < TOL_CONV
    assert maxabs(edgetaper(xp, k, method="direct"), ref.edgetaper(xp, k, method="direct")) < TOL_TAPER
    check_inverse(inverse_filtering_rank3(x, k, ALPHA, BETA, remove_halo=True, do_edgetaper=True, method="direct"),
                  oracle_inverse(x, k, "direct", True), TOL_INV, "direct, taper + halo")
    check_inverse(inverse_filtering_rank3(x, k, ALPHA, BETA, method="fft"), oracle_inverse(x, k, "fft", False), TOL_INV, "fft, plain")


@pytest.mark.parametrize("shape", [(7, 10), (30, 33)], ids=lambda s: "%dx%d" % s)
def test_batch_one_kernel_broadcasts(shape):
    from polyblur_amd import inverse_filtering_rank3
    x = rescaled_batch(2, 2, 40, 52, 7410)
    k = make_kernel(shape, 7411)
    for method in ("fft", "direct"):
        check_inverse(inverse_filtering_rank3(x, k, ALPHA, BETA, remove_halo=True, do_edgetaper=True, method=method),
                      oracle_inverse(x, k, method, True), TOL_INV, method)


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_one_kernel_per_plane(method):
    """(2,3,9,12): one kernel per plane, against the oracle applied channel by channel (taper weights normalised per plane)"""
    from polyblur_amd import inverse_filtering_rank3, convolve2d
    x = rescaled_batch(2, 3, 40, 52, 7420)
    k = make_kernel((9, 12), 7421, batch=2, channels=3)
    xp = ref.replicate_pad(x, 6)
    want = np.concatenate([ref.convolve2d(xp[:, c:c + 1], k[:, c:c + 1], method=method) for c in range(3)], axis=1)
    assert maxabs(convolve2d(xp, k, method=method), want) < TOL_CONV
    for full in (False, True):
        check_inverse(inverse_filtering_rank3(x, k, ALPHA, BETA, remove_halo=full, do_edgetaper=full, method=method),
                      oracle_inverse(x, k, method, full), TOL_INV, "full" if full else "plain")


@pytest.mark.parametrize("method", ["fft", "direct"])
def test_single_partial_tile(method):
    """a (1,1,9,11) image with a 5 x 26 kernel: one workgroup, most of its tile outside the 35 x 37 padded domain"""
    from polyblur_amd import inverse_filtering_rank3
    x = rescaled_batch(1, 1, 9, 11, 7430)
    k = make_kernel((5, 26), 7431)
    for full in (False, True):
        check_inverse(inverse_filtering_rank3(x, k, ALPHA, BETA, remove_halo=full, do_edgetaper=full, method=method),
                      oracle_inverse(x, k, method, full), TOL_INV, "full" if full else "plain")


@pytest.mark.parametrize("shape", [(9, 9), (30, 30)], ids=lambda s: "%dx%d" % s)
def test_n_tapers(image, shape):
    from polyblur_amd import edgetaper
    k = make_kernel(shape, 7440)
    xp = ref.replicate_pad(image, shape[1] // 2)
    assert np.array_equal(edgetaper(xp, k, n_tapers=0), xp)
    for n in (1, 2):
        for method in ("fft", "direct"):
            assert maxabs(edgetaper(xp, k, n_tapers=n, method=method), ref.edgetaper(xp, k, n_tapers=n, method=method)) < TOL_TAPER


@pytest.mark.parametrize("shape", [(12, 15), (29, 40)], ids=lambda s: "%dx%d" % s)
def test_fp16_images(image, shape):
    """fp16 in, fp16 out, against the oracle on the fp16-rounded input"""
    from polyblur_amd import inverse_filtering_rank3
    k = make_kernel(shape, 7450)
    xh = image.astype(np.float16)
    for method in ("fft", "direct"):
        for full in (False, True):
            got = inverse_filtering_rank3(xh, k, ALPHA, BETA, remove_halo=full, do_edgetaper=full, method=method)
            assert got.dtype == np.float16
            check_inverse(got.astype(np.float32), oracle_inverse(xh.astype(np.float32), k, method, full), TOL_HALF, method)


def test_grad_img_of_the_caller(image):
    """grad_img given: the halo mask uses the caller's gradients (here: of another image), not the image's own"""
    from polyblur_amd import inverse_filtering_rank3
    k = make_kernel((28, 28), 7460)
    other = rescaled_batch(1, 3, 50, 70, 7461)
    grad = ref.spectral_gradients(other)
    got = inverse_filtering_rank3(image, k, ALPHA, BETA, remove_halo=True, grad_img=grad, method="fft")
    want = ref.inverse_filtering_rank3(image, k, ALPHA, BETA, remove_halo=True, grad_img=grad, method="fft")
    assert maxabs(want, oracle_inverse(image, k, "fft", False)) > 1e-4          # (the mask does something here)
    check_inverse(got, want, TOL_INV, "grad_img")


def test_type_and_device_follow_the_input(image):
    import torch
    from polyblur_amd import inverse_filtering_rank3, convolve2d, edgetaper
    k = make_kernel((6, 30), 7470)
    want = oracle_inverse(image, k, "direct", False)
    got = inverse_filtering_rank3(image, k, ALPHA, BETA)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == image.shape
    check_inverse(got, want, TOL_INV, "ndarray")
    t = torch.from_numpy(image)
    got = inverse_filtering_rank3(t, torch.from_numpy(k), ALPHA, BETA)
    assert isinstance(got, torch.Tensor) and got.device.type == "cpu" and got.dtype == torch.float32
    check_inverse(got.numpy(), want, TOL_INV, "cpu tensor")
    tg = t.cuda()
    for kk in (torch.from_numpy(k).cuda(), k):              # (the kernel may live anywhere: its taps go through the host)
        got = inverse_filtering_rank3(tg, kk, ALPHA, BETA)
        assert isinstance(got, torch.Tensor) and got.device == tg.device and got.dtype == torch.float32
        check_inverse(got.cpu().numpy(), want, TOL_INV, "gpu tensor")
    got = inverse_filtering_rank3(tg.half(), k, ALPHA, BETA)
    assert got.device == tg.device and got.dtype == torch.float16
    for fn, oracle_fn, tol in ((convolve2d, ref.convolve2d, TOL_CONV), (edgetaper, ref.edgetaper, TOL_TAPER)):
        got = fn(tg, k, method="direct")
        assert isinstance(got, torch.Tensor) and got.device == tg.device
        assert maxabs(got.cpu().numpy(), oracle_fn(image, k, method="direct")) < tol
    # halo masking with the caller's gradients on the device
    grad = ref.spectral_gradients(image)
    got = inverse_filtering_rank3(tg, k, ALPHA, BETA, remove_halo=True, grad_img=tuple(torch.from_numpy(g).cuda() for g in grad))
    check_inverse(got.cpu().numpy(), ref.inverse_filtering_rank3(image, k, ALPHA, BETA, remove_halo=True, grad_img=grad), TOL_INV, "gpu grads")


# ---------------------------------------------------------------------------------------------
# the set is the caller's, not scratch
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(13, 13), (49, 49)], ids=lambda s: "%dx%d" % s)
def test_kernel_set_outlives_other_calls(eng, image, shape):
    """the same set gives the same answer after an unrelated blind call on the same engine -- one with a ker_size above 25, whose
    own tap tables are context scratch -- and under the other boundary in between"""
    from polyblur_amd import polyblur_deblurring
    k = make_kernel(shape, 7480)
    ks = eng.set_taps(k[:, 0])
    try:
        first = eng.inverse_filter_taps(image, ks, ALPHA, BETA, capi.PB_WRAP, edgetaping=True, remove_halo=True)
        check_inverse(first, oracle_inverse(image, k, "fft", True), TOL_INV, "first")
        other = rescaled_batch(1, 3, 96, 80, 7481)
        polyblur_deblurring(np.ascontiguousarray(np.moveaxis(other[0], 0, -1)), n_iter=2, ker_size=31, edgetaping=True)
        polyblur_deblurring(np.ascontiguousarray(np.moveaxis(other[0], 0, -1)), n_iter=1)
        check_inverse(eng.inverse_filter_taps(image, ks, ALPHA, BETA, capi.PB_ZERO), oracle_inverse(image, k, "direct", False), TOL_INV, "direct")
        again = eng.inverse_filter_taps(image, ks, ALPHA, BETA, capi.PB_WRAP, edgetaping=True, remove_halo=True)
        assert np.array_equal(first, again)
    finally:
        ks.free()


def test_free_then_a_set_of_another_shape(eng, image):
    for shape, nxt in (((10, 10), (40, 7)), ((40, 7), (10, 10)), ((10, 10), (9, 12))):
        k = make_kernel(shape, 7490)
        ks = eng.set_taps(k[:, 0])
        check_inverse(eng.inverse_filter_taps(image, ks, ALPHA, BETA, capi.PB_ZERO), oracle_inverse(image, k, "direct", False), TOL_INV, shape)
        ks.free()
        ks.free()                                           # (idempotent)
        k2 = make_kernel(nxt, 7491)
        ks2 = eng.set_taps(k2[:, 0])
        try:
            check_inverse(eng.inverse_filter_taps(image, ks2, ALPHA, BETA, capi.PB_ZERO), oracle_inverse(image, k2, "direct", False), TOL_INV, nxt)
            xp = ref.replicate_pad(image, nxt[1] // 2)
            assert maxabs(eng.convolve2d_taps(xp, ks2, capi.PB_ZERO), ref.convolve2d(xp, k2, method="direct")) < TOL_CONV
        finally:
            ks2.free()


def test_c_abi_refusals(eng, image):
    """what the Python layer refuses the C ABI refuses too, with a message"""
    from polyblur_amd._capi import PolyblurHipError
    with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
        eng.set_taps(np.ones((1, 5, 1), np.float32))
    with pytest.raises(PolyblurHipError, match="PB_ERR_UNSUPPORTED"):
        eng.set_taps(np.ones((1, 50, 5), np.float32))
    ks = eng.set_taps(make_kernel((21, 5), 7495)[:, 0])
    try:
        with pytest.raises(PolyblurHipError, match="PB_ERR_UNSUPPORTED.*taller than wide"):
            eng.convolve2d_taps(image, ks, capi.PB_WRAP)
        with pytest.raises(PolyblurHipError, match="PB_ERR_UNSUPPORTED"):
            eng.inverse_filter_taps(image, ks, ALPHA, BETA, capi.PB_WRAP, edgetaping=True)
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
            eng.inverse_filter_taps(image[:, :, :17], ks, ALPHA, BETA, capi.PB_ZERO)      # 21 rows > 17 + 4 - 1
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
            eng.inverse_filter_taps(np.concatenate([image, image]), ks, ALPHA, BETA, capi.PB_ZERO)   # one kernel, two images
        with pytest.raises(PolyblurHipError, match="PB_ERR_BADARG"):
            eng.edgetaper_taps(image, ks, capi.PB_ZERO, n_tapers=-1)
    finally:
        ks.free()
