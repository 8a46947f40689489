"""The non-blind entry points with a kernel of the caller's, as far as they can be checked without a GPU: they are exported,
the library has their symbols, every refused case raises before any device work (on a box without a GPU any device work
raises PolyblurHipError instead), and the oracle the GPU tests compare with reproduces the reference's own outputs
(tests/golden/nonblind*.npz, written by tests/golden/make_golden_nonblind.py) within 3e-6."""
import os

import numpy as np
import pytest

from oracle import polyblur_ref as oracle

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ALPHA, BETA = 2, 3


def test_public_functions_are_exported():
    import polyblur_amd
    from polyblur_amd import inverse_filtering_rank3, convolve2d, edgetaper  # noqa: F401
    import inspect
    for name in ("inverse_filtering_rank3", "convolve2d", "edgetaper"):
        assert name in polyblur_amd.__all__
    # the reference's signatures (deblurring.py:211-212, filters.py:14 without ksize / padding, edgetaper.py:26)
    p = inspect.signature(inverse_filtering_rank3).parameters
    assert list(p) == ["img", "kernel", "alpha", "b", "correlate", "remove_halo", "do_edgetaper", "grad_img", "method"]
    assert (p["alpha"].default, p["b"].default, p["correlate"].default, p["remove_halo"].default, p["do_edgetaper"].default,
            p["grad_img"].default, p["method"].default) == (2, 4, False, False, False, None, "direct")
    p = inspect.signature(convolve2d).parameters
    assert list(p) == ["img", "kernel", "method"] and p["method"].default == "direct"
    p = inspect.signature(edgetaper).parameters
    assert list(p) == ["img", "kernel", "n_tapers", "method"] and (p["n_tapers"].default, p["method"].default) == (3, "fft")


def test_library_exports_the_kernel_set_symbols():
    from polyblur_amd import _capi as capi
    if not os.path.exists(capi.library_path()):
        from polyblur_amd.build import build
        build(verbose=False)
    lib = capi.load_library()
    for name in ("pb_taps_create", "pb_taps_free", "pb_convolve2d_taps", "pb_edgetaper_taps", "pb_inverse_filter_taps"):
        assert name in capi.SYMBOLS and hasattr(lib, name), name
    from polyblur_amd.engine import Engine
    for name in ("set_taps", "convolve2d_taps", "edgetaper_taps", "inverse_filter_taps"):
        assert hasattr(Engine, name), name


def test_refusals_before_any_device_work():
    from polyblur_amd import inverse_filtering_rank3, convolve2d, edgetaper
    x = np.full((1, 3, 16, 20), 0.5, np.float32)
    k = lambda h, w, b=1, c=1: np.full((b, c, h, w), 1.0 / (h * w), np.float32)   # noqa: E731
    calls = (lambda kk, **kw: inverse_filtering_rank3(x, kk, **kw), lambda kk, **kw: convolve2d(x, kk, **kw),
             lambda kk, **kw: edgetaper(x, kk, **kw))
    for f in calls:
        with pytest.raises(ValueError):
            f(k(5, 1))                                       # one tap wide: the reference's crop [0:-0] is empty
        with pytest.raises(NotImplementedError):
            f(k(5, 51))                                      # sides above 49
        with pytest.raises(NotImplementedError):
            f(k(50, 5))
        with pytest.raises(NotImplementedError):
            f(k(5, 5), method="direct_separable")
        with pytest.raises(NotImplementedError):
            f((np.ones((1, 1), np.float32),) * 3)            # the tuple form
        with pytest.raises(ValueError):
            f(k(5, 5), method="nope")
        with pytest.raises(ValueError):
            f(k(5, 5, b=2))                                  # kernel batch is neither 1 nor B
        with pytest.raises(ValueError):
            f(k(5, 5, c=2))                                  # kernel channels are neither 1 nor C
        with pytest.raises(ValueError):
            f(np.ones((5, 5), np.float32))                   # not (B,C,h,w)
    # a kernel taller than the domain minus one: padded height 16 + 2 * 1 = 18 for the inverse filter, 16 for the stages
    with pytest.raises(ValueError):
        inverse_filtering_rank3(x, k(18, 3))
    with pytest.raises(ValueError):
        convolve2d(x, k(16, 3))
    with pytest.raises(ValueError):
        edgetaper(x, k(16, 3), method="direct")
    # taller than wide under 'fft': refused in the stages and with do_edgetaper
    with pytest.raises(NotImplementedError):
        convolve2d(x, k(9, 3), method="fft")
    with pytest.raises(NotImplementedError):
        edgetaper(x, k(9, 3), method="fft")
    with pytest.raises(NotImplementedError):
        inverse_filtering_rank3(x, k(9, 3), method="fft", do_edgetaper=True)
    with pytest.raises(ValueError):
        edgetaper(x, k(3, 3), n_tapers=-1)
    # images
    with pytest.raises(ValueError):
        inverse_filtering_rank3(np.zeros((16, 20), np.float32), k(3, 3))
    with pytest.raises(TypeError):
        convolve2d([[0.0]], k(3, 3))
    import torch
    with pytest.raises(TypeError):
        convolve2d(torch.zeros(1, 1, 16, 20, dtype=torch.float16), k(3, 3))        # fp16: the inverse filter only
    with pytest.raises(TypeError):
        inverse_filtering_rank3(torch.zeros(1, 1, 16, 20, dtype=torch.float64), k(3, 3))
    with pytest.raises(ValueError):
        inverse_filtering_rank3(x, k(3, 3), remove_halo=True, grad_img=(x, x[:, :1]))


def _each_inverse_case(d):
    x = d["x"]
    for name in d.files:
        if not name.startswith("inv_"):
            continue
        p = name.split("_")
        if p[1] == "correlate":
            yield name, x, np.ascontiguousarray(d["k_" + p[2]][..., ::-1, ::-1]), dict(method=p[3])
        elif p[1] == "perchannel":
            yield name, x, d["k_perchannel_" + p[2]], dict(method=p[3], remove_halo=True)
        else:
            full = p[3] == "full"
            yield name, x, d["k_" + p[1]], dict(method=p[2], do_edgetaper=full, remove_halo=full)


def test_oracle_reproduces_the_reference_goldens():
    d = np.load(os.path.join(GOLDEN, "nonblind.npz"))
    n = 0
    for name, x, k, kw in _each_inverse_case(d):
        if k.shape[1] > 1:       # one kernel per plane: the oracle channel by channel
            y = np.concatenate([oracle.inverse_filtering_rank3(x[:, c:c + 1], k[:, c:c + 1], ALPHA, BETA, **kw)
                                for c in range(k.shape[1])], axis=1)
        else:
            y = oracle.inverse_filtering_rank3(x, k, ALPHA, BETA, **kw)
        err = float(np.abs(y - d[name]).max())
        print(name, err)
        assert err < 3e-6, (name, err)
        n += 1
    assert n == 18
    x = d["x"]
    for fname, fn in (("nonblind_conv.npz", oracle.convolve2d), ("nonblind_taper.npz", oracle.edgetaper)):
        s = np.load(os.path.join(GOLDEN, fname))
        assert len(s.files) == 4
        for name in s.files:
            _, shape, method = name.split("_")
            k = d["k_" + shape]
            y = fn(oracle.replicate_pad(x, k.shape[-1] // 2), k, method=method)
            err = float(np.abs(y - s[name]).max())
            print(name, err)
            assert err < 3e-6, (name, err)
