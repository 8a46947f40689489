"""The differentiable recursive filter without a GPU: the float64 restatement of its gradients
(tests/dt_grad_ref.py) against the reference's own autograd (tests/golden/dt_grad.npz), the proof that the comparison of
tests/test_gpu_dt_autograd.py has teeth -- every mutant of the backward misses the golden by parts in a thousand, and the GPU
tolerances are four to eight times the reference's own float32 error --, then the symbols, the binding and the refusals that remain."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import dt_grad_ref as dg
from frontend_cases import no_device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c["name"] for c in dg.golden()[1]]
PAIRS = (("dx64", 0), ("dj64", 1))


def test_golden_holds_the_cases_it_should():
    _, cases = dg.golden()
    plain = [c for c in cases if not c["quantised"]]
    assert [(tuple(c["shape"]), dg.setting_of(c), c["joint"]) for c in plain] == \
        [(s, st, j) for s, st in zip([(2, 3, 17, 65), (1, 1, 33, 130), (2, 4, 5, 7)], dg.SETTINGS) for j in (False, True)]
    (q,) = [c for c in cases if c["quantised"]]
    assert q["joint"] and dg.setting_of(q) in dg.SETTINGS
    for name in NAMES:
        c, x, j, w, grads = dg.golden_case(name)
        assert x.dtype == w.dtype == np.float32 and x.shape == w.shape == tuple(c["shape"])
        assert 0.25 <= np.abs(w).min() and np.abs(w).max() < 1.0 and (w < 0).any() and (w > 0).any()
        assert set(grads) == ({"dx64", "dx32", "dj64", "dj32"} if c["joint"] else {"dx64", "dx32"})
        assert grads["dx64"].dtype == np.float64 and grads["dx32"].dtype == np.float32
        if c["quantised"]:
            assert np.array_equal(j * 8, np.round(j * 8))
            equal = np.mean(np.diff(j, axis=-1) == 0)
            assert 0.05 < equal < 0.3, equal                     # many equal neighbours, and many that differ
    assert os.path.getsize(dg.GOLDEN) < 1 << 20


@pytest.mark.parametrize("name", NAMES)
def test_restatement_is_the_references_float64_gradient(name):
    c, x, j, w, grads = dg.golden_case(name)
    got = dg.backward(x, j, w, *dg.setting_of(c))
    for key, k in PAIRS:
        if key in grads:
            err = dg.rel_error(got[k], grads[key])
            print("%s %s: restatement off by %.3g of max |grad| = %.3g" % (name, key, err, np.abs(grads[key]).max()))
            assert err <= 1e-10, (name, key, err)
    assert c["joint"] or got[1] is None


# What a mutant cannot move: "one a" needs a second iteration (the cases of setting 0 have one); "vbar one channel" needs a second
# channel (s1i, s1j have one) and, like "weights constant", moves nothing but the guide's path -- the image's gradient of a case with
# a joint image stays exact; "sign of zero is one" needs equal neighbours in the guide, which only the quantised case has (uniform
# float32 samples have none), and there again moves the guide's gradient alone.
MOVES = {
    "weights constant": lambda c: True,
    "ends dropped": lambda c: True,
    "one a": lambda c: c["num_iterations"] > 1,
    "vbar one channel": lambda c: c["shape"][1] > 1,
    "sign of zero is one": lambda c: c["quantised"],
}


@pytest.mark.parametrize("mutant", dg.MUTANTS)
def test_mutants_miss_the_golden(mutant):
    assert set(MOVES) == set(dg.MUTANTS)
    moved = []
    for name in NAMES:
        c, x, j, w, grads = dg.golden_case(name)
        got = dg.backward(x, j, w, *dg.setting_of(c), mutant=mutant)
        errs = {key: dg.rel_error(got[k], grads[key]) for key, k in PAIRS if key in grads}
        print("%s, %s: off by %s" % (mutant, name, ", ".join("%s %.3g" % kv for kv in errs.items())))
        if MOVES[mutant](c):
            assert max(errs.values()) > 1e-3, (mutant, name, errs)
            moved.append(name)
        else:
            assert max(errs.values()) <= 1e-10, (mutant, name, errs)
        if c["joint"] and mutant in ("weights constant", "vbar one channel", "sign of zero is one"):
            assert errs["dx64"] <= 1e-10                          # (the guide's path alone)
    assert moved


def measured_float32_error():
    """per setting, the largest error of the reference's float32 gradients against its float64 ones, relative to the gradient's
    largest entry, over the setting's cases and both gradients"""
    E = {s: 0.0 for s in dg.SETTINGS}
    for name in NAMES:
        c, _, _, _, grads = dg.golden_case(name)
        for key in ("dx", "dj"):
            if key + "64" in grads:
                E[dg.setting_of(c)] = max(E[dg.setting_of(c)], dg.rel_error(grads[key + "32"], grads[key + "64"]))
    return E


def test_tolerances_are_four_to_eight_float32_errors():
    E = measured_float32_error()
    assert set(dg.TOL_DT) == set(dg.SETTINGS)
    for s in dg.SETTINGS:
        print("setting %r: E = %.3g, TOL_DT = %.3g = %.2f E" % (s, E[s], dg.TOL_DT[s], dg.TOL_DT[s] / E[s]))
        assert 1e-8 < E[s] < 1e-5
        assert 4 * E[s] <= dg.TOL_DT[s] <= 8 * E[s], (s, E[s])


# ---------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------
def test_symbols_binding_and_header():
    import polyblur_amd as pa
    from polyblur_amd import _capi as capi
    from polyblur_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "polyblur_hip.h")).read()
    m = re.search(r"int pb_dt_recursive_filter_backward\(([^)]*)\);", header)
    assert m and "pb_dt_recursive_filter_backward" in capi.SYMBOLS
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert [a.rsplit(" ", 1)[0].replace(" *", "*").strip() + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in args] == \
        ["pb_ctx*", "const float*", "const float*", "const float*", "float*", "float*", "int", "int", "int", "int", "float", "float", "int"]
    comment = header[:m.start()].rsplit("/*", 1)[1]
    for word in ("domain_transform.py:6-85", '"dtg.x"', '"dtg.f"', '"dtg.p"', '"dtg.g"', '"dtg.dx"', '"dtg.dy"', "PB_PROF_PREFILTER"):
        assert word in comment, word
    assert "#define PB_VERSION 200" in header and header.count("#define PB_PROF_NTAGS 10") == 1
    assert "dt_grad.hip" in __import__("polyblur_amd.build", fromlist=["SOURCES"]).SOURCES
    source = open(os.path.join(ROOT, "polyblur_amd", "csrc", "dt_grad.hip")).read()
    assert set(re.findall(r'pb_scratch\(ctx, "([^"]+)"', source)) == {"dtg.x", "dtg.f", "dtg.p", "dtg.g", "dtg.dx", "dtg.dy"}
    assert "atomic" not in source.replace("no float atomics", "")
    assert list(inspect.signature(Engine.dt_recursive_filter_backward_ptr).parameters) == \
        ["self", "in_ptr", "joint_ptr", "grad_out_ptr", "grad_in_ptr", "grad_joint_ptr", "shape", "sigma_s", "sigma_r", "num_iterations"]
    if os.path.exists(capi.library_path()):
        fn = capi.load_library().pb_dt_recursive_filter_backward              # (load_library: every symbol of SYMBOLS is exported)
        assert fn.restype is ctypes.c_int
        assert list(fn.argtypes) == [ctypes.c_void_p] * 6 + [ctypes.c_int] * 4 + [ctypes.c_float] * 2 + [ctypes.c_int]
        assert fn(None, None, None, None, None, None, 1, 1, 4, 4, 2.0, 0.8, 1) == -1      # a NULL context: PB_ERR_BADARG, no device touched
    assert "recursive_filter" in pa.__all__
    from polyblur_amd._autograd import RecursiveFilterFunction
    assert issubclass(RecursiveFilterFunction, torch.autograd.Function)


@pytest.fixture
def no_library():
    """any device work raises: a refusal must come first"""
    with no_device(AssertionError("device work before the refusal")):
        yield


class FakeRocm:
    """stands in for a ROCm tensor where there is no GPU: what the refusals look at, and nothing a device call could use"""

    def __init__(self, like, dtype=torch.float32, index=0, requires_grad=False):
        self.shape, self.dtype, self.device, self.requires_grad = like.shape, dtype, torch.device("cuda", index), requires_grad
        self.is_cuda = True

    def dim(self):
        return len(self.shape)

    def data_ptr(self):
        raise AssertionError("device work before the refusal")


FakeRocm.__module__ = "torch"


def test_refusals_that_remain(no_library):
    import polyblur_amd as pa
    x = torch.rand(1, 3, 16, 18)
    xg = x.clone().requires_grad_(True)
    pinned = "recursive_filter has no backward pass: the edge-aware filters are not differentiated"
    for call in (lambda: pa.recursive_filter(xg), lambda: pa.recursive_filter(xg, joint_image=x),
                 lambda: pa.recursive_filter(x, joint_image=xg), lambda: pa.recursive_filter(x.numpy(), joint_image=xg)):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == pinned
    for name, call in (("edge_aware_filtering", lambda: pa.edge_aware_filtering(xg, 2.0, 0.8, prefilter="domain_transform")),
                       ("normalized_convolution", lambda: pa.normalized_convolution(xg))):
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value) == name + " has no backward pass: the edge-aware filters are not differentiated"
    # operands of which one is a ROCm tensor: what is required is said, before any device work
    rg, r = FakeRocm(x, requires_grad=True), FakeRocm(x)
    mixed = [
        lambda: pa.recursive_filter(FakeRocm(x, torch.float16, requires_grad=True)),                # float16 under grad
        lambda: pa.recursive_filter(rg, joint_image=FakeRocm(x, torch.float16)),
        lambda: pa.recursive_filter(rg, joint_image=x),                                             # a CPU guide beside a ROCm image
        lambda: pa.recursive_filter(rg, joint_image=x.numpy()),                                     # an array beside a tensor that requires grad
        lambda: pa.recursive_filter(x.numpy(), joint_image=rg),
        lambda: pa.recursive_filter(r, joint_image=xg),                                             # a CPU guide that requires grad
        lambda: pa.recursive_filter(rg, joint_image=FakeRocm(x, index=1)),                          # two devices
        lambda: pa.recursive_filter(r, joint_image=FakeRocm(x, index=1, requires_grad=True)),
    ]
    for call in mixed:
        with pytest.raises(NotImplementedError) as e:
            call()
        assert str(e.value).startswith("recursive_filter has no backward pass: gradients are built for float32 ROCm tensors on one "
                                       "device, I and joint_image alike (got I: "), str(e.value)
    with torch.no_grad():                                                                       # nothing is refused without grad: the call reaches the device
        with pytest.raises(AssertionError, match="device work before the refusal"):
            pa.recursive_filter(xg)
