"""The differentiable recursive filter on the GPU: pb_dt_recursive_filter_backward alone and
polyblur_amd.recursive_filter under torch.autograd -- against the float64 restatement (tests/dt_grad_ref.py, which
tests/test_dt_autograd_cpu.py pins to the reference's own float64 autograd and proves discriminating) and against the reference's
goldens (tests/golden/dt_grad.npz).

Tolerance: per gradient, dg.TOL_DT[setting] x its largest entry -- four to eight times the error of the reference's own float32
gradients against its float64 ones at that setting.  The margin covers a scan that associates its products differently and the
device's expf; nothing else should differ.  Equalities (a NULL output, the same call twice, operands at an element offset, the
forward under grad, a chain of two calls) are of bits."""
import os
import re

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import dt_grad_ref as dg
import offset_operands as oo
from polyblur_amd import _capi as capi

DTG_U = 4                                                    # rows a thread of the column kernel requests together (csrc/dt_grad.hip)
S0, S1, S2 = dg.SETTINGS
SEED = 4131


def cuda(a, **kw):
    import torch
    return torch.tensor(np.asarray(a), device="cuda", **kw)


def run(eng, x, j, w, setting, want_x=True, want_j=True):
    """pb_dt_recursive_filter_backward through `eng` on device tensors, into planes full of NaN: written, not accumulated"""
    import torch
    gx = torch.full_like(x, float("nan")) if want_x else None
    gj = torch.full_like(x, float("nan")) if want_j and j is not None else None
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.dt_recursive_filter_backward_ptr(x.data_ptr(), None if j is None else j.data_ptr(), w.data_ptr(),
                                         None if gx is None else gx.data_ptr(), None if gj is None else gj.data_ptr(), x.shape, *setting)
    torch.cuda.current_stream().synchronize()
    return gx, gj


def engine_backward(x, j, w, setting, **kw):
    from polyblur_amd.engine import get_engine
    gx, gj = run(get_engine(0), cuda(x), None if j is None else cuda(j), cuda(w), setting, **kw)
    return None if gx is None else gx.cpu().numpy(), None if gj is None else gj.cpu().numpy()


def check(shape, setting, joint, seed=SEED, quantised=False):
    x, j, w, dI, dJ = dg.reference(shape, setting, seed, joint, quantised)
    gx, gj = engine_backward(x, j, w, setting)
    tol = dg.TOL_DT[setting]
    for what, got, want in (("image", gx, dI), ("guide", gj, dJ)):
        if want is None:
            assert got is None
            continue
        err = dg.rel_error(got, want)
        print("%r %r joint=%s, %s: %.3g of max |grad| = %.3g (tolerance %.3g)" % (shape, setting, joint, what, err, np.abs(want).max(), tol))
        assert np.isfinite(got).all()
        assert err <= tol, (shape, setting, joint, what, err)


# ---------------------------------------------------------------------------------------------
# pb_dt_recursive_filter_backward alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("joint", [False, True], ids=["self", "joint"])
@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 130])
def test_lines(W, joint):
    """the edge of a wave's chunk of 64 samples, and the lone sample that has no neighbour"""
    check((1, 3, 5, W), S1, joint)


def test_the_column_block_is_the_kernels():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "polyblur_amd", "csrc", "dt_grad.hip")).read()
    assert int(re.search(r"constexpr int DTG_U = (\d+);", src).group(1)) == DTG_U


# the top-to-bottom sweep takes rows 1 .. DTG_U, DTG_U + 1 .. 2 DTG_U, ...; the bottom-to-top sweep rows H - 1 .. H - DTG_U, ...:
# H one short of, equal to and one past k DTG_U and k DTG_U + 1, for the first two blocks
COLUMN_HEIGHTS = sorted({1, 2, 17, 33} | {k * DTG_U + e + d for k in (1, 2) for e in (0, 1) for d in (-1, 0, 1)})


@pytest.mark.parametrize("joint", [False, True], ids=["self", "joint"])
@pytest.mark.parametrize("H", COLUMN_HEIGHTS)
def test_columns(H, joint):
    check((1, 3, H, 7), S1, joint)


@pytest.mark.parametrize("joint", [False, True], ids=["self", "joint"])
@pytest.mark.parametrize("setting", dg.SETTINGS, ids=lambda s: "s%g-r%g-n%d" % s)
@pytest.mark.parametrize("C", [1, 3, 4])
def test_channels_batch_and_settings(C, setting, joint):
    """plane and batch strides; one and three channels share the map's slope, four run channel by channel"""
    check((2, C, 17, 65), setting, joint)


def test_quantised_guide():
    """many equal neighbours (sign(0) = 0), and differences that are exact"""
    check((1, 3, 9, 70), S1, True, quantised=True)


@pytest.mark.parametrize("C", [3, 4])
def test_a_null_output_changes_no_bit_of_the_other(C):
    x, j, w, _, _ = dg.reference((2, C, 17, 65), S1, SEED, True)
    gx, gj = engine_backward(x, j, w, S1)
    only_x = engine_backward(x, j, w, S1, want_j=False)
    only_j = engine_backward(x, j, w, S1, want_x=False)
    assert only_x[1] is None and only_j[0] is None
    assert np.array_equal(only_x[0], gx) and np.array_equal(only_j[1], gj)


def test_the_same_call_twice_gives_equal_bits():
    for shape, setting, joint in (((2, 3, 17, 65), S2, True), ((2, 4, 17, 65), S1, False), ((1, 1, 33, 130), S1, True)):
        x, j, w, _, _ = dg.reference(shape, setting, SEED, joint)
        a, b = engine_backward(x, j, w, setting), engine_backward(x, j, w, setting)
        for p, q in zip(a, b):
            assert (p is None and q is None) or np.array_equal(p, q)


@pytest.mark.parametrize("C", [3, 4])
def test_operands_at_odd_element_offsets(C):
    """every operand carved one or three elements off a 16-byte boundary: the bits of the aligned call, the guards untouched"""
    import torch
    from polyblur_amd.engine import get_engine
    shape = (2, C, 17, 65)
    x, j, w, _, _ = dg.reference(shape, S1, SEED, True)
    eng = get_engine(0)

    def call(offsets):
        bufs = [oo.carve(a, o) for a, o in zip((x.copy(), j.copy(), w.copy(), oo.poisoned(shape, torch.float32), oo.poisoned(shape, torch.float32)), offsets)]
        xv, jv, wv, gx, gj = (v for _, v in bufs)
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.dt_recursive_filter_backward_ptr(xv.data_ptr(), jv.data_ptr(), wv.data_ptr(), gx.data_ptr(), gj.data_ptr(), shape, *S1)
        torch.cuda.current_stream().synchronize()
        assert all(oo.guards_intact(b, v) for b, v in bufs)
        return oo.bits(gx).cpu().numpy(), oo.bits(gj).cpu().numpy()

    aligned = call((0, 0, 0, 0, 0))
    for offsets in ((1, 3, 1, 3, 1), (3, 1, 1, 1, 3)):
        got = call(offsets)
        assert np.array_equal(got[0], aligned[0]) and np.array_equal(got[1], aligned[1]), offsets
    assert not (aligned[0] == oo.POISON[torch.float32][1]).any() and not (aligned[1] == oo.POISON[torch.float32][1]).any()


def test_consecutive_calls_of_different_shapes_and_the_scratch():
    """a small call, a larger one with more iterations, the small one again on ONE engine: the scratch is re-sized, the first result
    comes back bit for bit, and the workspace grows by the documented figure: 2 N + 2 plane sets and two (B,H,W) planes"""
    import torch
    from polyblur_amd.engine import Engine
    small, big = ((1, 3, 5, 7), S0, True), ((2, 3, 17, 65), S2, True)
    r256 = lambda n: (n + 255) // 256 * 256
    eng = Engine(0)
    try:
        results = []
        before = eng.workspace_bytes()
        for shape, setting, joint in (small, big, small):
            x, j, w, dI, dJ = dg.reference(shape, setting, SEED, joint)
            gx, gj = run(eng, cuda(x), cuda(j), cuda(w), setting)
            assert dg.rel_error(gx.cpu().numpy(), dI) <= dg.TOL_DT[setting] and dg.rel_error(gj.cpu().numpy(), dJ) <= dg.TOL_DT[setting]
            results.append((gx, gj))
        assert torch.equal(results[0][0], results[2][0]) and torch.equal(results[0][1], results[2][1])
        (B, C, H, W), N = big[0], big[1][2]
        assert eng.workspace_bytes() - before == r256(4 * B * C * H * W * (2 * N - 1)) + 3 * r256(4 * B * C * H * W) + 2 * r256(4 * B * H * W)
    finally:
        eng.close()


def test_bad_arguments_are_refused_before_any_launch():
    """no output, a guide gradient without a guide, an output that aliases an input or the other output, a sigma of 0 or inf,
    no iteration, an empty shape: PB_ERR_BADARG, nothing written"""
    import torch
    from polyblur_amd.engine import get_engine
    eng = get_engine(0)
    shape = (1, 2, 8, 9)
    x, j, w = (torch.rand(shape, device="cuda") for _ in range(3))
    gx, gj = torch.full(shape, 7.0, device="cuda"), torch.full(shape, 7.0, device="cuda")
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    X, J, Wp, GX, GJ = (t.data_ptr() for t in (x, j, w, gx, gj))
    for args in ((X, J, Wp, None, None, shape, 2.0, 0.8, 1), (X, None, Wp, GX, GJ, shape, 2.0, 0.8, 1), (X, None, Wp, None, GJ, shape, 2.0, 0.8, 1),
                 (X, J, Wp, X, GJ, shape, 2.0, 0.8, 1), (X, J, Wp, GX, J, shape, 2.0, 0.8, 1), (X, J, Wp, Wp, GJ, shape, 2.0, 0.8, 1),
                 (X, J, Wp, GX, GX, shape, 2.0, 0.8, 1), (X, J, Wp, GX, GJ, shape, 0.0, 0.8, 1), (X, J, Wp, GX, GJ, shape, 2.0, 0.0, 1),
                 (X, J, Wp, GX, GJ, shape, float("inf"), 0.8, 1), (X, J, Wp, GX, GJ, shape, 2.0, float("nan"), 1),
                 (X, J, Wp, GX, GJ, shape, 2.0, 0.8, 0), (X, J, Wp, GX, GJ, (1, 2, 0, 9), 2.0, 0.8, 1), (None, J, Wp, GX, GJ, shape, 2.0, 0.8, 1),
                 (X, J, None, GX, GJ, shape, 2.0, 0.8, 1)):
        with pytest.raises(capi.PolyblurHipError, match="PB_ERR_BADARG"):
            eng.dt_recursive_filter_backward_ptr(*args)
    torch.cuda.current_stream().synchronize()
    assert bool((gx == 7.0).all()) and bool((gj == 7.0).all())


# ---------------------------------------------------------------------------------------------
# recursive_filter under autograd
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [c["name"] for c in dg.golden()[1]])
def test_recursive_filter_function_against_the_goldens(name):
    import torch
    import polyblur_amd as pa
    c, x, j, w, grads = dg.golden_case(name)
    ss, sr, n = setting = dg.setting_of(c)
    xt = cuda(x, requires_grad=True)
    jt = None if j is None else cuda(j, requires_grad=True)
    y = pa.recursive_filter(xt, ss, sr, n, joint_image=jt)
    assert y.requires_grad and y.grad_fn is not None
    (y * cuda(w)).sum().backward()
    for what, t, key in (("x.grad", xt, "dx64"), ("joint_image.grad", jt, "dj64")):
        if t is None:
            continue
        assert t.grad.shape == t.shape and t.grad.dtype == torch.float32 and t.grad.is_cuda
        err = dg.rel_error(t.grad.cpu().numpy(), grads[key])
        print("%s %s: %.3g of max |grad| = %.3g (tolerance %.3g)" % (name, what, err, np.abs(grads[key]).max(), dg.TOL_DT[setting]))
        assert err <= dg.TOL_DT[setting], (name, what, err)
    # the forward is pb_dt_recursive_filter whatever the mode: the bits under torch.no_grad() and of tensors that ask for nothing
    with torch.no_grad():
        quiet = pa.recursive_filter(xt, ss, sr, n, joint_image=jt)
    plain = pa.recursive_filter(cuda(x), ss, sr, n, joint_image=None if j is None else cuda(j))
    assert not quiet.requires_grad and not plain.requires_grad and quiet.grad_fn is None
    assert torch.equal(y.detach(), quiet) and torch.equal(quiet, plain)
    assert float(np.abs(plain.cpu().numpy() - dg.forward(x, j, ss, sr, n)).max()) <= 5e-6      # (tests/test_gpu_edge_aware.py's bound)


def test_only_the_operand_that_asks_gets_a_gradient():
    import polyblur_amd as pa
    c, x, j, w, grads = dg.golden_case("s0j")
    ss, sr, n = setting = dg.setting_of(c)
    for want_x in (True, False):
        xt, jt = cuda(x, requires_grad=want_x), cuda(j, requires_grad=not want_x)
        y = pa.recursive_filter(xt, ss, sr, n, joint_image=jt)
        assert y.grad_fn is not None
        y.backward(cuda(w))
        asked, other, key = (xt, jt, "dx64") if want_x else (jt, xt, "dj64")
        assert other.grad is None
        assert dg.rel_error(asked.grad.cpu().numpy(), grads[key]) <= dg.TOL_DT[setting]


def test_an_upstream_gradient_that_is_not_contiguous():
    import polyblur_amd as pa
    c, x, j, w, grads = dg.golden_case("s0i")
    ss, sr, n = setting = dg.setting_of(c)
    xt = cuda(x, requires_grad=True)
    wide = cuda(np.repeat(w, 2, axis=-1))[..., ::2]
    assert not wide.is_contiguous() and np.array_equal(wide.cpu().numpy(), w)
    pa.recursive_filter(xt, ss, sr, n).backward(wide)
    assert dg.rel_error(xt.grad.cpu().numpy(), grads["dx64"]) <= dg.TOL_DT[setting]


def test_two_filters_in_a_row_compose():
    """torch.autograd.grad through recursive_filter(recursive_filter(x)) is the engine's backward of the second call handed to the
    engine's backward of the first: the same kernels on the same operands, so the same bits"""
    import torch
    import polyblur_amd as pa
    c, x, _, w, _ = dg.golden_case("s1i")
    ss, sr, n = setting = dg.setting_of(c)
    xt = cuda(x, requires_grad=True)
    mid = pa.recursive_filter(xt, ss, sr, n)
    out = pa.recursive_filter(mid, ss, sr, n)
    assert mid.grad_fn is not None and out.grad_fn is not None
    (g,) = torch.autograd.grad((out * cuda(w)).sum(), xt)
    g1, _ = engine_backward(mid.detach().cpu().numpy(), None, w, setting)
    g0, _ = engine_backward(x, None, g1, setting)
    assert np.isfinite(g0).all() and np.abs(g0).max() > 0
    assert np.array_equal(g.cpu().numpy(), g0)


def test_refusals_on_rocm_tensors():
    import polyblur_amd as pa
    x = cuda(np.random.default_rng(5).random((1, 3, 16, 18), dtype=np.float32))
    xg = x.clone().requires_grad_(True)
    needs = "recursive_filter has no backward pass: gradients are built for float32 ROCm tensors on one device"
    for call in (lambda: pa.recursive_filter(x.half().requires_grad_(True)),                    # float16 under grad
                 lambda: pa.recursive_filter(xg, joint_image=x.cpu()),                          # a CPU guide beside a ROCm image
                 lambda: pa.recursive_filter(x, joint_image=x.cpu().requires_grad_(True)),
                 lambda: pa.recursive_filter(xg, joint_image=x.cpu().numpy())):
        with pytest.raises(NotImplementedError, match=needs):
            call()
    with pytest.raises(NotImplementedError, match="edge_aware_filtering has no backward pass: the edge-aware filters are not differentiated"):
        pa.edge_aware_filtering(xg, 2.0, 0.8, prefilter="domain_transform")
