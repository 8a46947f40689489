"""Differentiable halo masking without a GPU: the float64 restatement of the gradients (tests/halo_grad_ref.py) by
hand against torch's autograd and against the reference's own gradients (tests/golden/halo_grad.npz), and the proof that
tests/test_gpu_halo_autograd.py has teeth -- for every case it uses the gauge holds from the float64 reference alone, its comparison
rejects every applicable mutant of the backward, and its tolerances are four times the float32 NumPy evaluation's own error.
Then the symbols, the public names and the refusals that remain."""
import functools
import os

import numpy as np
import pytest
import torch

import autograd_ref as ar
from frontend_cases import no_device
import halo_grad_ref as hg
import halo_ref as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE = hg.stage_cases()
STAGE_IDS = [c[0] for c in STAGE]
CHAIN, BLIND = ["c00", "c01", "c02", "c03"], ["b00", "b01"]
REJECT = 10                                                   # a mutant is off by at least this many GPU tolerances


@functools.lru_cache(maxsize=None)
def goldens():
    return np.load(os.path.join(ROOT, "tests", "golden", "halo_grad.npz"))


def case(name):
    d = goldens()
    return [c for c in hg.golden_cases(d) if c["name"] == name][0], {k[len(name) + 1:]: d[k] for k in d.files if k.startswith(name + "_")}


@functools.lru_cache(maxsize=None)
def chain_reference(name):
    c, d = case(name)
    grad_img = None if c["own"] else (d["gx"], d["gy"])
    return c, d, grad_img, hg.chain_tolerances(d["x"], d["k"], grad_img, d["w"], c["alpha"], c["beta"], c["method"])


@functools.lru_cache(maxsize=None)
def blind_reference(name):
    c, d = case(name)
    _, steps = hg.blind(d["x"], c["n_iter"], hr.PIPE_KW)
    return c, d, steps, hg.blind_tolerances(d["x"], d["w"], c["n_iter"], hr.PIPE_KW)


# ---------------------------------------------------------------------------------------------
# the restatement: by hand against autograd, both against the reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,shape,zeros", STAGE, ids=STAGE_IDS)
def test_hand_written_backward_is_autograds(cid, shape, zeros):
    s = hg.repaired_set(shape, zeros)
    auto = hg.autograd_backward(s["x"], s["y"], s["gx"], s["gy"], s["g"])
    assert max(hg.plane_error(auto[n], s["want"][n]) for n in hg.NAMES) < 1e-12


def test_fourier_backward_is_autograds():
    for shape in hg.FOURIER_SHAPES:
        ggx, ggy = hg.fourier_case(shape)
        x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
        gx, gy = hg.fourier_gradients_torch(x)
        ((gx * torch.tensor(ggx, dtype=torch.float64)).sum() + (gy * torch.tensor(ggy, dtype=torch.float64)).sum()).backward()
        assert hg.plane_error(hg.fourier_backward(ggx, ggy), x.grad.numpy()) < 1e-12


def test_restatement_against_the_references_float64_gradients():
    d, worst = goldens(), 0.0
    for c in hg.golden_cases(d):
        if c["kind"] == "stage":
            s = hg.repaired_set(tuple(c["shape"]), c["zeros"])
            assert all(np.array_equal(d[c["name"] + "_" + k], s[k]) for k in hg.NAMES + ("g",))      # the builder's, still
            worst = max([worst] + [hg.plane_error(s["want"][n], d[c["name"] + "_d" + n]) for n in hg.NAMES])
        elif c["kind"] == "chain":
            _, g, _, ref = chain_reference(c["name"])
            worst = max([worst] + [float(np.abs(ref["want"][n] - g["d" + n]).max() / np.abs(g["d" + n]).max()) for n in ref["want"]])
            assert float(np.abs(ref["gk"] - ref["want"]["k"]).max()) < 1e-10 * float(np.abs(ref["want"]["k"]).max())   # the lag form
    print("restatement vs the reference's float64 gradients: %.3g" % worst)
    assert hg.BOUND_GOLDEN_F64 / 8 < worst <= hg.BOUND_GOLDEN_F64 / 4


def test_restatement_against_the_references_blind_gradients():
    worst = 0.0
    for name in BLIND:
        _, d, _, ref = blind_reference(name)
        worst = max(worst, float(np.max(np.abs(ref["want"] - d["dx"]) / hg.image_max(d["dx"]))))
    print("restatement vs the reference's float32 blind gradients: %.3g" % worst)
    assert hg.BOUND_GOLDEN_BLIND / 8 < worst <= hg.BOUND_GOLDEN_BLIND / 4


# ---------------------------------------------------------------------------------------------
# the gauge, from the float64 reference alone
# ---------------------------------------------------------------------------------------------
def z_and_pole_ok(z, pole):
    return np.mean(z > 0) >= 0.10 and np.mean(z == 0) >= 0.10 and pole.min() >= 0.25


@pytest.mark.parametrize("cid,shape,zeros", STAGE, ids=STAGE_IDS)
def test_stage_gauge_holds(cid, shape, zeros):
    s = hg.repaired_set(shape, zeros)
    tol = hg.stage_tolerance(shape)
    for n in hg.NAMES:
        moved = hg.plane_fraction(s["want"][n], s["unmasked"][n], 50 * tol[n])
        assert moved >= 0.05, (n, moved)
    assert z_and_pole_ok(s["z"], s["pole"])
    assert not hg.kink_band(s["y"], s["gx"], s["gy"])[0].any() and hg.active_sets_agree(s)
    if zeros:
        assert np.mean((s["gx"] == 0) & (s["gy"] == 0)) > 0.05 and np.mean(s["r"] == 0) > 0.05


def chain_forward(x, k, grad_img, c):
    y = ar.rank3_unclamped(torch.tensor(np.asarray(x, np.float64)), torch.tensor(np.asarray(k, np.float64)), c["alpha"], c["beta"], c["method"]).numpy()
    gx, gy = (hg.dx(x), hg.dy(x)) if grad_img is None else grad_img
    _, nM, M, r, z = hg.forward_parts(x, y, gx, gy)
    return y, gx, gy, r, z, np.abs(nM + M) / nM


@pytest.mark.parametrize("name", CHAIN)
def test_chain_gauge_holds(name):
    c, d, grad_img, ref = chain_reference(name)
    _, plain = hg.chain_gradients(d["x"], d["k"], grad_img, d["w"], c["alpha"], c["beta"], c["method"], mask=False)
    moved = (np.abs(ref["want"]["x"] - plain["x"]) >= 50 * ref["tol"]["x"]).mean(axis=(-2, -1))
    print(name, "the mask moves the image gradient by 50 tolerances on %.1f %% of a plane at least" % (100 * moved.min()))
    assert moved.min() >= 0.05
    y, gx, gy, r, z, pole = chain_forward(d["x"], d["k"], grad_img, c)
    assert z_and_pole_ok(z, pole)
    assert not hg.kink_band(y, gx, gy)[0].any()
    r32 = hg.forward_parts(d["x"], y, gx, gy, np.float32)[3]
    assert np.array_equal(r32 >= 0, r >= 0)
    margin, clamped = ar.clamp_margin(ref["out"])
    assert margin > 1e-3 and clamped >= 0.05


@pytest.mark.parametrize("name", BLIND)
def test_blind_gauge_holds(name):
    c, d, steps, ref = blind_reference(name)
    moved = hg.blind_moved(d["x"], d["w"], c["n_iter"], steps, ref)
    print(name, "the mask moves the blind gradient by 50 tolerances on %.1f %% of a plane at least" % (100 * moved))
    assert moved >= 0.05
    gx, gy = hg.dx(d["x"]), hg.dy(d["x"])
    assert hg.blind_margins_ok(steps, gx, gy)
    zs, poles = [], []
    for xi, _, _, yu in steps:
        _, nM, M, r, z = hg.forward_parts(xi, yu, gx, gy)
        zs.append(z)
        poles.append(np.abs(nM + M) / nM)
        assert np.array_equal(hg.forward_parts(xi, yu, gx, gy, np.float32)[3] >= 0, r >= 0)
    # over the case's iterations together: the second iteration's input is deblurred already, and the mask finds little there
    # (b01: z > 0 on 59 % of the samples of the first iteration, on 2 % of the second)
    assert z_and_pole_ok(np.stack(zs), np.stack(poles))


# ---------------------------------------------------------------------------------------------
# mutants of the float64 backward, each wrong in one way
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,shape,zeros", STAGE, ids=STAGE_IDS)
def test_stage_mutants_are_rejected(cid, shape, zeros):
    s = hg.repaired_set(shape, zeros)
    tol = hg.stage_tolerance(shape)
    applied = []
    for name in hg.MUTANTS:
        m = hg.stage_mutant(name, s)
        if m is None:
            continue
        applied.append(name)
        off = max(hg.plane_error(m[n], s["want"][n]) / tol[n] for n in hg.NAMES)
        assert off >= REJECT, (name, off)
    must = {"z detached", "S dropped", "+D for -D", "gy * oy", "Dy for Dx"}
    if np.prod(shape[:2]) > 1:
        must.add("nM of the neighbouring plane")
    if zeros:
        must.add("open side at r == 0")
    assert must <= set(applied)


@pytest.mark.parametrize("name", CHAIN)
def test_chain_mutants_are_rejected(name):
    c, d, grad_img, ref = chain_reference(name)
    for mutant in ("z detached",) + (("grad_img detached",) if grad_img is None else ()):
        _, m = hg.chain_gradients(d["x"], d["k"], grad_img, d["w"], c["alpha"], c["beta"], c["method"], mutant=mutant)
        off = float(np.max(np.abs(m["x"] - ref["want"]["x"]) / ref["tol"]["x"]))
        assert off >= REJECT, (mutant, off)


@pytest.mark.parametrize("name", BLIND)
def test_blind_mutants_are_rejected(name):
    c, d, steps, ref = blind_reference(name)
    for mutant in ("z detached", "grad_img detached"):
        m = hg.blind_gradient(d["x"], d["w"], c["n_iter"], hr.PIPE_KW, steps=steps, mutant=mutant)
        off = float(np.max(np.abs(m - ref["want"]) / ref["tol"]))
        assert off >= REJECT, (mutant, off)


# ---------------------------------------------------------------------------------------------
# the tolerances: four times the float32 NumPy evaluation's error against float64, measured here again
# ---------------------------------------------------------------------------------------------
def test_stage_tolerances_are_four_float32_errors():
    worst = {False: dict.fromkeys(hg.NAMES, 0.0), True: dict.fromkeys(hg.NAMES, 0.0)}
    for _, shape, zeros in STAGE:
        s = hg.repaired_set(shape, zeros)
        f = hg.hand_backward(s["x"], s["y"], s["gx"], s["gy"], s["g"], dtype=np.float32)
        w = worst[tuple(shape) == hg.MANY]
        for n in hg.NAMES:
            w[n] = max(w[n], hg.plane_error(f[n], s["want"][n]))
    print("float32 NumPy vs float64:", worst)
    for many, tol in ((False, hg.TOL_STAGE), (True, hg.TOL_STAGE_MANY)):
        for n in hg.NAMES:
            assert tol[n] / 8 < worst[many][n] <= tol[n] / 4, (many, n, worst[many][n])


def test_fourier_tolerance_is_four_float32_errors():
    worst = 0.0
    for shape in hg.FOURIER_SHAPES:
        ggx, ggy = hg.fourier_case(shape)
        for a, b in ((ggx, ggy), (ggx, None), (None, ggy)):
            worst = max(worst, hg.plane_error(hg.fourier_backward(a, b, np.float32), hg.fourier_backward(a, b)))
    print("float32 NumPy vs float64, the spectral derivative's backward: %.3g" % worst)
    assert hg.TOL_FOURIER / 8 < worst <= hg.TOL_FOURIER / 4


# ---------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------
def test_symbols_names_and_header():
    import polyblur_amd as pa
    from polyblur_amd import _capi as capi
    header = open(os.path.join(ROOT, "include", "polyblur_hip.h")).read()
    for name in ("pb_fourier_gradients_backward", "pb_halo_mask_backward"):
        assert "int %s(" % name in header and name in capi.SYMBOLS
    assert "deblurring.py:173-208" in header and "filters.py:159-186" in header
    assert "#define PB_VERSION 200" in header and header.count("#define PB_PROF_NTAGS 10") == 1
    for name in ("fourier_gradients", "halo_masking"):
        assert name in pa.__all__ and callable(getattr(pa, name))
    if os.path.exists(capi.library_path()):
        lib = capi.load_library()
        assert hasattr(lib, "pb_fourier_gradients_backward") and hasattr(lib, "pb_halo_mask_backward")
    assert "halo_grad.hip" in __import__("polyblur_amd.build", fromlist=["SOURCES"]).SOURCES


@pytest.fixture
def no_library():
    """any device work raises: a refusal must come first"""
    with no_device(AssertionError("device work before the refusal")):
        yield


def test_refusals_that_remain(no_library):
    import polyblur_amd as pa
    x, k = torch.rand(1, 3, 16, 18), torch.rand(1, 1, 3, 5)
    xg = x.clone().requires_grad_(True)
    planes = (torch.rand(1, 3, 16, 18), torch.rand(1, 3, 16, 18, requires_grad=True))
    calls = [
        ("halo masking is differentiated for float32 ROCm tensors only", lambda: pa.inverse_filtering_rank3(xg, k, 6, 1, remove_halo=True)),
        ("halo masking is differentiated for float32 ROCm tensors only", lambda: pa.inverse_filtering_rank3(x, k, 6, 1, remove_halo=True, grad_img=planes)),
        ("halo masking is differentiated for float32 ROCm tensors only", lambda: pa.inverse_filtering_rank3(x.half().requires_grad_(True), k, 6, 1, remove_halo=True)),
        ("has no backward pass.*halo masking is differentiated", lambda: pa.polyblur_deblurring(xg, remove_halo=True)),
        ("has no backward pass.*halo masking is differentiated", lambda: pa.PolyblurDeblurring()(xg, remove_halo=True)),
        ("halo masking is differentiated", lambda: pa.halo_masking(xg, x)),
        ("halo masking is differentiated", lambda: pa.halo_masking(x, xg, planes)),
        ("halo masking is differentiated", lambda: pa.halo_masking(x, x, planes)),
        ("spectral derivative is differentiated", lambda: pa.fourier_gradients(xg)),
        ("edgetaper is not", lambda: pa.inverse_filtering_rank3(xg, k, 6, 1, remove_halo=False, do_edgetaper=True, method="fft")),
        ("edgetaper", lambda: pa.polyblur_deblurring(xg, edgetaping=True)),
        ("prefilter", lambda: pa.polyblur_deblurring(xg, prefiltering=True)),
        ("pure-phase", lambda: pa.inverse_filtering_nonsymmetric(xg, k, 6, 1, remove_halo=True)),
        ("float32", lambda: pa.polyblur_deblurring(x.half().requires_grad_(True))),
        ("patch", lambda: pa.PolyblurDeblurring(patch_decomposition=True)(xg, remove_halo=True)),
    ]
    for pattern, call in calls:
        with pytest.raises(NotImplementedError, match=pattern) as e:
            call()
        assert "\n" not in str(e.value)                       # a one-line reason
    with pytest.raises(ValueError):
        pa.halo_masking(x, torch.rand(1, 3, 16, 20))
    with pytest.raises(ValueError):
        pa.halo_masking(x, x, (x,))
    with pytest.raises(TypeError):
        pa.halo_masking(x.half(), x)
