"""The differentiable patch decomposition without a GPU: the float64 restatement of the branch's two ends
(tests/patch_grad_ref.py) against the oracle's overlap-add and under gradcheck, the conditions the GPU test's inputs must meet and
the figures its bound comes from, then the symbols, the public names and the refusals that remain."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest
import torch

import patch_grad_ref as pg
from frontend_cases import no_device
from oracle import polyblur_ref as ref                       # the checker (tests only)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(pg.CASES))
def test_forward_is_the_oracles_overlap_add(name, monkeypatch):
    """the oracle's patch branch with the blind call replaced by a fixed map of each patch: the same patches go through both
    overlap-adds.  The oracle works in float32: its result lies within float32 roundoff of the float64 restatement (a quotient of
    two sums of at most 16 terms of size <= 2: 2e-6), and the patches themselves -- copies -- are equal."""
    full, ps, ov = pg.CASES[name]
    shape, g = pg.case(name)
    rng = np.random.default_rng(5)
    x = rng.random(full, dtype=np.float32)
    seen = []

    def remap(p, **kw):
        seen.append(np.array(p))
        return (1.6 * p - 0.3).astype(np.float32)                        # (some of it beyond [0, 1]: the clamp takes part)
    monkeypatch.setattr(ref, "polyblur_deblurring", remap)
    want = ref.patchwise_deblurring(x, (ps, ps), ov)
    xe = torch.from_numpy(x[..., :shape[2], :shape[3]].astype(np.float64))
    patches = pg.extract(xe, g)
    B = shape[0]
    assert len(seen) == g["n_i"] * g["n_j"]
    for n, p in enumerate(seen):
        assert np.array_equal(p, patches[n * B:(n + 1) * B].numpy().astype(np.float32))
    got, v = pg.overlap_add(1.6 * patches - 0.3, shape, g)
    assert got.shape == want.shape == shape
    assert float(np.abs(got.numpy() - want).max()) < 2e-6
    assert float(v.min()) < 0 and float(v.max()) > 1


def test_lattice_and_window_are_the_packages():
    from polyblur_amd.patches import kaiser_window_periodic, patch_grid
    for name, (full, ps, ov) in pg.CASES.items():
        shape, g = pg.case(name)
        mine = patch_grid(shape[2], shape[3], (ps, ps), ov)
        assert all(mine[k] == g[k] for k in mine), name
        assert np.array_equal(pg.window(ps, torch.float32).numpy(), kaiser_window_periodic(ps))
        assert np.array_equal(pg.window(ps, torch.float32).numpy(), ref.kaiser_window_periodic(ps))


def test_gradcheck_of_the_restatement():
    shape, g = pg.case("e")
    x = torch.rand(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(3), requires_grad=True)
    assert torch.autograd.gradcheck(lambda t: pg.extract(t, g), (x,), eps=1e-6, atol=1e-7, fast_mode=True)
    p, _ = pg.ola_inputs("e")                                             # (no value within 0.03 of the clamp's kinks)
    pt = torch.from_numpy(p.astype(np.float64)).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: pg.overlap_add(t, shape, g)[0], (pt,), eps=1e-6, atol=1e-7, fast_mode=True)


@pytest.mark.parametrize("name", sorted(pg.CASES))
def test_conditions_and_figures_of_the_gpu_test(name):
    """what tests/test_gpu_patch_autograd.py relies on: no float64 value before the clamp within 1e-3 of 0 or 1, between 5 % and 95 %
    of the samples clamped, exactly representable partial sums of the extraction's backward, and the recorded float32 error E of the
    restatement -- the bound is 6 E -- within a factor of two of the one measured here"""
    shape, g = pg.case(name)
    p, w = pg.ola_inputs(name)
    grad, v = pg.ola_gradient(name, p, w)
    margin = min(float(np.abs(v).min()), float(np.abs(v - 1).min()))
    share = float(((v < 0) | (v > 1)).mean())
    e = pg.measure_e(name)
    inside = pg.in_image(g, shape[0], shape[1]).numpy()
    up = pg.dyadic_upstream(name)
    ge = pg.extraction_gradient(name, up)
    print("%s: margin %.4f, clamped %.3f, E %.3g (recorded %.3g), largest |extraction gradient| * 64 = %g" %
          (name, margin, share, e, pg.E_OLA[name], np.abs(ge).max() * 64))
    assert margin >= 1e-3 and 0.05 <= share <= 0.95
    assert pg.E_OLA[name] / 2 <= e <= pg.E_OLA[name] * 2 and pg.TOL_OLA[name] == 6 * pg.E_OLA[name]
    assert not grad[~inside].any()                                       # (the cropped pad: exactly 0)
    assert np.abs(up * 64).max() <= 64 and np.array_equal(up * 64, np.rint(up * 64)) and np.abs(ge).max() * 64 < 2 ** 24
    assert np.array_equal(ge * 64, np.rint(ge * 64)) and np.array_equal(ge.astype(np.float32).astype(np.float64), ge)
    assert abs(ge.sum() - up.astype(np.float64).sum()) < 1e-9           # (the adjoint of a gather keeps the total)


# ---------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------
def _types(header, name):
    m = re.search(r"int %s\(([^)]*)\);" % name, header)
    assert m, name
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    return [a.rsplit(" ", 1)[0].replace(" *", "*").strip() + ("*" if a.rsplit(" ", 1)[1].startswith("*") else "") for a in args]


def test_symbols_names_and_header():
    import polyblur_amd as pa
    from polyblur_amd import _capi as capi
    from polyblur_amd.engine import Engine
    header = open(os.path.join(ROOT, "include", "polyblur_hip.h")).read()
    assert _types(header, "pb_extract_patches_backward") == ["pb_ctx*", "const float*", "float*"] + ["int"] * 12
    assert _types(header, "pb_overlap_add_backward") == ["pb_ctx*", "const float*", "const float*", "float*"] + ["int"] * 12 + ["const float*"] * 2
    assert all(s in header for s in ('"patchg.P"', '"patchg.R"', '"patchg.S"'))
    assert {"pb_extract_patches_backward", "pb_overlap_add_backward"} <= set(capi.SYMBOLS)
    assert "patch_grad.hip" in __import__("polyblur_amd.build", fromlist=["SOURCES"]).SOURCES
    assert list(inspect.signature(Engine.extract_patches_backward_ptr).parameters) == ["self", "grad_patches_ptr", "grad_img_ptr", "shape", "grid"]
    assert list(inspect.signature(Engine.overlap_add_backward_ptr).parameters) == \
        ["self", "patches_ptr", "grad_out_ptr", "grad_patches_ptr", "shape", "grid", "wy_ptr", "wx_ptr"]
    if not os.path.exists(capi.library_path()):                           # (as tests/test_frontend_cpu.py: the library needs no GPU)
        from polyblur_amd.build import build
        build(verbose=False)
    lib = capi.load_library()                                             # (AttributeError where the library does not export a symbol)
    assert list(lib.pb_extract_patches_backward.argtypes) == [ctypes.c_void_p] * 3 + [ctypes.c_int] * 12
    assert list(lib.pb_overlap_add_backward.argtypes) == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 12 + [ctypes.c_void_p] * 2
    for name in ("image_to_patches", "patches_to_image"):
        assert name in pa.__all__ and callable(getattr(pa, name))
    assert [p for p in inspect.signature(pa.image_to_patches).parameters] == ["images", "patch_size", "patch_overlap"]
    assert [p for p in inspect.signature(pa.patches_to_image).parameters] == ["patches", "image_size", "patch_size", "patch_overlap"]
    assert inspect.signature(pa.image_to_patches).parameters["patch_size"].default == 400
    assert inspect.signature(pa.patches_to_image).parameters["patch_overlap"].default == 0.25
    from polyblur_amd._autograd import ExtractPatchesFunction, OverlapAddFunction
    assert issubclass(ExtractPatchesFunction, torch.autograd.Function) and issubclass(OverlapAddFunction, torch.autograd.Function)
    # one statement of the cover sum: the forward kernel and the backward's first launch call the header's function
    csrc = os.path.join(ROOT, "polyblur_amd", "csrc")
    for f in ("filters.hip", "patch_grad.hip"):
        assert "patch_cover(" in open(os.path.join(csrc, f)).read() and "patch_cover_value(" in open(os.path.join(csrc, f)).read()


@pytest.fixture
def no_library():
    """any device work raises: a refusal must come first"""
    with no_device(AssertionError("device work before the refusal")):
        yield


def test_refusals_that_remain(no_library):
    import polyblur_amd as pa
    x = torch.rand(1, 3, 16, 18)
    xg, xh = x.clone().requires_grad_(True), x.half().requires_grad_(True)
    p = torch.tensor(0.4, requires_grad=True)
    module = pa.PolyblurDeblurring(patch_decomposition=True, patch_size=8)
    for call in (lambda: module(xg), lambda: module(xh), lambda: module(x, c=p), lambda: module(x, alpha=p), lambda: module(xg, remove_halo=True),
                 lambda: module(xg, edgetaping=True), lambda: module(x.half(), b=p)):
        with pytest.raises(NotImplementedError, match="has no backward pass.*overlap-add") as e:
            call()
        assert "patch_decomposition" in str(e.value) and "\n" not in str(e.value)
    for f, t in ((pa.image_to_patches, xg), (pa.image_to_patches, xh)):
        with pytest.raises(NotImplementedError, match="has no backward pass"):
            f(t, 8)
    patches = torch.rand(2 * 3, 3, 8, 8)                                  # (16 x 18 under 8 / 0.25: pads to 20 x 20, 3 x 3 patches)
    assert pg.lattice((1, 3, 16, 18), 8, 0.25)["n_i"] * pg.lattice((1, 3, 16, 18), 8, 0.25)["n_j"] == 9
    with pytest.raises(ValueError, match="are not the"):
        pa.patches_to_image(patches, (16, 18), 8)
    with pytest.raises(NotImplementedError, match="has no backward pass"):
        pa.patches_to_image(torch.rand(9, 3, 8, 8, requires_grad=True), (16, 18), 8)
    # the lattice's errors come as they do without grad
    with pytest.raises(ValueError, match="holds no patch"):
        pa.image_to_patches(x, 400, 0.4)
    with pytest.raises(ValueError, match="positive step"):
        pa.image_to_patches(x, 1, 0.5)
    with pytest.raises(ValueError, match="positive step"):
        pa.patches_to_image(patches, (16, 18), 8, 0.95)
    with pytest.raises(TypeError, match="float32 or float16"):
        pa.image_to_patches(x.double(), 8)
    with pytest.raises(ValueError, match="4-D"):
        pa.image_to_patches(x[0], 8)
