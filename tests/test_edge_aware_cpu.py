"""The edge-aware filters as public functions, without a GPU: the names, the ABI entry, the reference's signatures, every refusal
before any device work, and the float64 yardstick of tests/test_gpu_edge_aware.py against the fp32 oracle."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import polyblur_amd as pa
from polyblur_amd import _capi as capi
from polyblur_amd.edge_aware import bilateral_filter, edge_aware_filtering, normalized_convolution, recursive_filter
from oracle import polyblur_ref as ref
import filters_ref as fr
import frontend_cases as fc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bilateral_filter", "recursive_filter", "normalized_convolution", "edge_aware_filtering")
IMAGE = (1, 3, 16, 18)
NO_BACKWARD = " has no backward pass: the edge-aware filters are not differentiated"


def image(grad=False, dtype=torch.float32, shape=IMAGE):
    return torch.rand(shape).to(dtype).requires_grad_(grad)


def test_names_are_public():
    for name in NAMES:
        assert name in pa.__all__ and callable(getattr(pa, name)), name


def test_abi_entry_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "polyblur_hip.h")).read()
    assert "int pb_bilateral(" in hdr and "filters.py:107-148" in hdr
    assert "#define PB_PROF_NTAGS 10" in hdr and "#define PB_VERSION 200" in hdr
    assert "pb_bilateral" in capi.SYMBOLS
    if not os.path.exists(capi.library_path()):
        from polyblur_amd.build import build
        build(verbose=False)
    assert hasattr(ctypes.CDLL(capi.library_path()), "pb_bilateral")
    lib = capi.load_library()
    assert lib.pb_bilateral.argtypes == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 6 + [ctypes.c_float] * 2
    # no context: refused without touching a device
    assert lib.pb_bilateral(None, None, None, capi.PB_F32, 1, 1, 4, 4, 7, 5.0, 0.1) == -1


def test_signatures_are_the_references():
    def params(f):
        return [(p.name, p.default) for p in inspect.signature(f).parameters.values()]
    none = inspect.Parameter.empty
    assert params(pa.bilateral_filter) == [("I", none), ("ksize", 5), ("sigma_spatial", 5.0), ("sigma_color", 0.1)]
    assert params(pa.recursive_filter) == [("I", none), ("sigma_s", 60), ("sigma_r", 0.4), ("num_iterations", 3), ("joint_image", None)]
    assert params(pa.normalized_convolution) == [("I", none), ("sigma_s", 60), ("sigma_r", 0.4), ("num_iterations", 3)]
    sig = inspect.signature(pa.edge_aware_filtering).parameters
    assert [(p.name, p.default) for p in sig.values()] == [("img", none), ("sigma_s", none), ("sigma_r", none), ("prefilter", "bilateral")]
    assert sig["prefilter"].kind is inspect.Parameter.KEYWORD_ONLY


CALLS = {
    "bilateral_filter": lambda x: bilateral_filter(x),
    "recursive_filter": lambda x: recursive_filter(x),
    "normalized_convolution": lambda x: normalized_convolution(x),
    "edge_aware_filtering": lambda x: edge_aware_filtering(x, 2.0, 0.8),
    "edge_aware_filtering/domain_transform": lambda x: edge_aware_filtering(x, 2.0, 0.8, prefilter="domain_transform"),
    "edge_aware_filtering/normalized_convolution": lambda x: edge_aware_filtering(x, 2.0, 0.8, prefilter="normalized_convolution"),
}

# (id, call, exception, a piece of its message)
REFUSALS = [
    ("ksize=2.5", lambda: bilateral_filter(image(), ksize=2.5), TypeError, "ksize must be an integer"),
    ("ksize='5'", lambda: bilateral_filter(image(), ksize="5"), TypeError, "ksize must be an integer"),
    ("ksize=4", lambda: bilateral_filter(image(), ksize=4), NotImplementedError, "even ksize"),
    ("ksize=0", lambda: bilateral_filter(image(), ksize=0), NotImplementedError, "even ksize"),
    ("ksize=-1", lambda: bilateral_filter(image(), ksize=-1), NotImplementedError, "from 1 to 25"),
    ("ksize=27", lambda: bilateral_filter(image(), ksize=27), NotImplementedError, "from 1 to 25"),
    ("sigma_spatial=0", lambda: bilateral_filter(image(), sigma_spatial=0), ValueError, "sigma_spatial"),
    ("sigma_color=-0.1", lambda: bilateral_filter(image(), sigma_color=-0.1), ValueError, "sigma_color"),
    ("sigma_color=nan", lambda: bilateral_filter(image(), sigma_color=float("nan")), ValueError, "sigma_color"),
    ("sigma_spatial=inf", lambda: bilateral_filter(image(), sigma_spatial=float("inf")), ValueError, "sigma_spatial"),
    ("sigma_color=1e-30", lambda: bilateral_filter(image(), sigma_color=1e-30), ValueError, "sigma_color"),
    ("rf/sigma_s=0", lambda: recursive_filter(image(), sigma_s=0), ValueError, "sigma_s"),
    ("rf/sigma_r=-1", lambda: recursive_filter(image(), sigma_r=-1), ValueError, "sigma_r"),
    ("rf/num_iterations=0", lambda: recursive_filter(image(), num_iterations=0), ValueError, "num_iterations"),
    ("rf/num_iterations=1.5", lambda: recursive_filter(image(), num_iterations=1.5), TypeError, "num_iterations"),
    ("rf/joint=other-shape", lambda: recursive_filter(image(), joint_image=torch.rand(1, 3, 16, 20)), ValueError, "joint_image must have the image's shape"),
    ("rf/joint=rank3", lambda: recursive_filter(image(), joint_image=torch.rand(3, 16, 18)), ValueError, "joint_image must have the image's shape"),
    ("rf/joint=list", lambda: recursive_filter(image(), joint_image=[[1.0]]), TypeError, "joint_image"),
    ("rf/joint=float64", lambda: recursive_filter(image(), joint_image=image(dtype=torch.float64)), TypeError, "joint_image"),
    ("rf/joint+grad", lambda: recursive_filter(image(), joint_image=image(True)), NotImplementedError, "recursive_filter" + NO_BACKWARD),
    ("rf/joint+grad/img=ndarray", lambda: recursive_filter(image().numpy(), joint_image=image(True)), NotImplementedError, "recursive_filter" + NO_BACKWARD),
    ("nc/sigma_s=0", lambda: normalized_convolution(image(), sigma_s=0), ValueError, "sigma_s"),
    ("nc/sigma_r=0", lambda: normalized_convolution(image(), sigma_r=0), ValueError, "sigma_r"),
    ("nc/num_iterations=0", lambda: normalized_convolution(image(), num_iterations=0), ValueError, "num_iterations"),
    ("nc/W=8191", lambda: normalized_convolution(torch.zeros(1, 1, 2, 8191)), NotImplementedError, "8190"),
    ("nc/H=8191", lambda: normalized_convolution(np.zeros((1, 1, 8191, 2), np.float32)), NotImplementedError, "8190"),
    ("eaf/prefilter=bogus", lambda: edge_aware_filtering(image(), 2.0, 0.8, prefilter="bogus"), ValueError,
     "prefilter must be 'bilateral', 'domain_transform' or 'normalized_convolution'"),
    ("eaf/dt/sigma_s=0", lambda: edge_aware_filtering(image(), 0.0, 0.8, prefilter="domain_transform"), ValueError, "sigma_s"),
    ("eaf/nc/sigma_r=0", lambda: edge_aware_filtering(image(), 2.0, 0.0, prefilter="normalized_convolution"), ValueError, "sigma_r"),
]


@pytest.mark.parametrize("call,error,text", [r[1:] for r in REFUSALS], ids=[r[0] for r in REFUSALS])
def test_argument_refusals_come_before_any_device_work(call, error, text):
    with fc.no_device(AssertionError("the call went for an engine")):
        with pytest.raises(error, match=re.escape(text)) as e:
            call()
    assert type(e.value) is error


@pytest.mark.parametrize("name", list(CALLS))
def test_image_refusals_are_check_images(name):
    """not a 4-D float32 or float16 image: what check_image(..., allow_half=True) raises, for every function"""
    call = CALLS[name]
    bad = [(torch.rand(IMAGE[1:]), ValueError, "expected a (B,C,H,W) tensor"), (image(dtype=torch.float64), TypeError, "tensor dtype must be float32 or float16"),
           (np.zeros(IMAGE[1:], np.float32), ValueError, "expected a (B,C,H,W) array"), ([[0.5]], TypeError, "img must be a numpy.ndarray or a torch.Tensor"),
           (torch.rand(1, 1, 1, 8), ValueError, "bad image shape")]
    with fc.no_device(AssertionError("the call went for an engine")):
        for x, error, text in bad:
            with pytest.raises(error) as e:
                call(x)
            assert text in str(e.value)


@pytest.mark.parametrize("name", list(CALLS))
@pytest.mark.parametrize("dtype", [torch.float32, torch.float16], ids=["float32", "float16"])
def test_grad_is_refused_and_no_grad_reaches_the_device(name, dtype):
    call = CALLS[name]
    with fc.no_device(AssertionError("the call went for an engine")):
        with pytest.raises(NotImplementedError) as e:
            call(image(True, dtype))
    assert str(e.value) == name.split("/")[0] + NO_BACKWARD
    for make in (lambda: image(False, dtype), lambda: image(False, dtype).numpy()):
        with pytest.raises(fc.DeviceReached):
            with fc.no_device(fc.DeviceReached()):
                call(make())
    with pytest.raises(fc.DeviceReached):
        with fc.no_device(fc.DeviceReached()), torch.no_grad():
            call(image(True, dtype))


def test_accepted_arguments_reach_the_device():
    """the edges of what is taken: every odd ksize from 1 to 25, NumPy integers, a joint image of another kind and dtype"""
    ok = [lambda k=k: bilateral_filter(image(), ksize=k) for k in range(1, 26, 2)]
    ok += [lambda: bilateral_filter(image(), ksize=np.int64(7), sigma_spatial=1, sigma_color=np.float32(0.02)),
           lambda: recursive_filter(image(), num_iterations=np.int32(1), joint_image=np.zeros(IMAGE)),
           lambda: recursive_filter(image(dtype=torch.float16), joint_image=image()),
           lambda: normalized_convolution(torch.zeros(1, 1, 2, 8190))]
    for call in ok:
        with pytest.raises(fc.DeviceReached):
            with fc.no_device(fc.DeviceReached()):
                call()


def test_blind_prefiltering_keeps_its_refusal():
    with fc.no_device(AssertionError("the call went for an engine")):
        with pytest.raises(NotImplementedError, match="the edge-aware prefilters are not differentiated"):
            pa.polyblur_deblurring(image(True), prefiltering=True)


@pytest.mark.parametrize("ksize", [1, 3, 5, 7, 13, 25])
def test_float64_yardstick_agrees_with_the_oracle(ksize):
    """3e-6 is what the 5 x 5 kernel is allowed against the reference's golden; the oracle's fp32 sums of up to 625 weights are
    within it (printed)"""
    x = np.random.default_rng(ksize).random((2, 3, 17, 65), dtype=np.float32)
    for ss, sc in ((5.0, 0.1), (1.5, 0.02), (12.0, 0.5)):
        err = fr.maxabs(ref.bilateral_filter(x, ksize, ss, sc), fr.bilateral_f64(x, ksize, ss, sc))
        print("ksize %d sigma %g / %g: oracle against float64 %.3g" % (ksize, ss, sc, err))
        assert err < 3e-6
    if ksize == 1:                                            # one tap: x / (1 + 1e-5)
        assert fr.maxabs(fr.bilateral_f64(x, 1), x.astype(np.float64) / (1 + 1e-5)) < 1e-15


def test_arguments_show_in_the_oracle():
    """the three changes of argument tests/test_gpu_edge_aware.py asks the engine to honour move the oracle's result by far more
    than ten parity bounds (6.4e-5 at most)"""
    x = np.random.default_rng(7).random((1, 1, 33, 130), dtype=np.float32)
    base = ref.bilateral_filter(x)
    for kw in (dict(ksize=7), dict(sigma_color=0.02), dict(sigma_spatial=1.0)):
        moved = fr.maxabs(ref.bilateral_filter(x, **kw), base)
        print(kw, "%.3g" % moved)
        assert moved > 1e-3
