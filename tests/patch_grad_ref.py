"""A float64 restatement of the patch branch's two ends, written from the reference's deblurring.py:269-340 with the
fix-forward of oracle/polyblur_ref.py::patchwise_deblurring (no saturation branch, patches of a batch per image): F.pad replicate,
slices, the periodic Kaiser(beta=5) window, +=, divide by the summed window + 1e-8, clamp, crop.  Its gradients are torch
autograd's -- the clamp's is torch.clamp's: 1 on [0, 1], both ends included.  Nothing here reads a GPU or a file.

tests/test_patch_autograd_cpu.py pins the forward to the oracle's overlap-add and gradchecks it; tests/test_gpu_patch_autograd.py
holds pb_extract_patches_backward and pb_overlap_add_backward to it."""
import math

import numpy as np
import torch
import torch.nn.functional as F

# (shape, patch_size, overlap)
CASES = {
    "a": ((2, 3, 150, 210), 64, 0.25),       # pads 5 and 23, 3 x 5 patches, batch > 1
    "b": ((1, 3, 151, 211), 80, 0.25),       # odd sizes cropped
    "c": ((1, 1, 90, 60), 100, 0.25),        # image smaller than one patch, pads 5 / 20
    "d": ((1, 2, 70, 96), 32, 0.5),          # no pad along x, cover 2 x 2
    "e": ((1, 1, 40, 46), 24, 0.75),         # cover 4 x 4, pad 1
    "g": ((2, 1, 60, 80), 33, 0.25),         # odd pad total: top 10 / bottom 11, left 0 / right 1
}


def lattice(shape, patch_size, overlap):
    """deblurring.py:273-299 on the even part of the image: the engine's lattice arguments, and the pads of all four sides"""
    h, w = shape[-2] // 2 * 2, shape[-1] // 2 * 2
    ph = pw = int(patch_size)
    step_h, step_w = int(ph * (1 - overlap)), int(pw * (1 - overlap))
    new_h = int(math.ceil((h - ph) / step_h) * step_h) + ph
    new_w = int(math.ceil((w - pw) / step_w) * step_w) + pw
    pad_top, pad_left = (new_h - h) // 2, (new_w - w) // 2
    return dict(ph=ph, pw=pw, step_h=step_h, step_w=step_w, new_h=new_h, new_w=new_w, pad_top=pad_top, pad_left=pad_left,
                pad_bottom=new_h - h - pad_top, pad_right=new_w - w - pad_left, n_i=len(range(0, new_h - ph + 1, step_h)),
                n_j=len(range(0, new_w - pw + 1, step_w)), h=h, w=w)


def case(name):
    """-> (the even-sized shape, the lattice)"""
    shape, ps, ov = CASES[name]
    g = lattice(shape, ps, ov)
    return (shape[0], shape[1], g["h"], g["w"]), g


def window(n, dtype=torch.float64):
    """torch.kaiser_window(n, periodic=True, beta=5) (deblurring.py:352), rounded to the float32 the engine is handed"""
    return torch.kaiser_window(n, periodic=True, beta=5.0, dtype=torch.float64).to(torch.float32).to(dtype)


def corners(g):
    return [(i0, j0) for i0 in range(0, g["new_h"] - g["ph"] + 1, g["step_h"]) for j0 in range(0, g["new_w"] - g["pw"] + 1, g["step_w"])]


def extract(x, g):
    """(B,C,h,w), even-sized -> (n*B, C, ph, pw), patch n of image b at [n*B + b]"""
    xp = F.pad(x, (g["pad_left"], g["pad_right"], g["pad_top"], g["pad_bottom"]), mode="replicate")
    return torch.cat([xp[..., i0:i0 + g["ph"], j0:j0 + g["pw"]] for i0, j0 in corners(g)], dim=0)


def slices_of(plane, g):
    """the patches of an already padded (B,C,new_h,new_w) plane"""
    return torch.cat([plane[..., i0:i0 + g["ph"], j0:j0 + g["pw"]] for i0, j0 in corners(g)], dim=0)


def overlap_add(patches, shape, g, wy=None, wx=None, clamp=True):
    """-> (the image, the value before the clamp), both cropped to shape's h x w; computed in patches' dtype"""
    B, C = shape[:2]
    dt = patches.dtype
    dev = patches.device                                     # (the GPU test composes the module from these same ops on the device)
    wy = (window(g["ph"], dt) if wy is None else wy.to(dt)).to(dev)
    wx = (window(g["pw"], dt) if wx is None else wx.to(dt)).to(dev)
    win = wy[:, None] * wx[None, :]
    acc = torch.zeros((B, C, g["new_h"], g["new_w"]), dtype=dt, device=dev)
    wsum = torch.zeros((g["new_h"], g["new_w"]), dtype=dt, device=dev)
    for n, (i0, j0) in enumerate(corners(g)):
        acc[..., i0:i0 + g["ph"], j0:j0 + g["pw"]] += patches[n * B:(n + 1) * B] * win
        wsum[i0:i0 + g["ph"], j0:j0 + g["pw"]] += win
    v = acc / (wsum + torch.tensor(1e-8, dtype=dt, device=dev))
    crop = (Ellipsis, slice(g["pad_top"], g["pad_top"] + g["h"]), slice(g["pad_left"], g["pad_left"] + g["w"]))
    return (v.clamp(0.0, 1.0) if clamp else v)[crop], v[crop]


def in_image(g, B, C):
    """(n*B, C, ph, pw) bool: the patch elements that lie inside the h x w image (False: in the cropped pad)"""
    m = torch.zeros((g["new_h"], g["new_w"]), dtype=torch.bool)
    m[g["pad_top"]:g["pad_top"] + g["h"], g["pad_left"]:g["pad_left"] + g["w"]] = True
    return slices_of(m[None, None].expand(B, C, -1, -1), g)


# ---------------------------------------------------------------------------------------------
# the inputs of the GPU tests
# ---------------------------------------------------------------------------------------------
def dyadic_upstream(name, seed=0):
    """k / 64 with integer |k| <= 64, in the patches' shape: every partial sum of the extraction's backward is a multiple of 1/64
    below 2^24 / 64, so float32 adds them without rounding in any order"""
    shape, g = case(name)
    rng = np.random.default_rng(1000 + seed + ord(name))
    k = rng.integers(-64, 65, size=(g["n_i"] * g["n_j"] * shape[0], shape[1], g["ph"], g["pw"]))
    return (k / 64.0).astype(np.float32)


def extraction_gradient(name, upstream):
    """float64 d sum(upstream * extract(x)) / d x by autograd"""
    shape, g = case(name)
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    extract(x, g).backward(torch.as_tensor(upstream, dtype=torch.float64))
    return x.grad.numpy()


def ola_inputs(name, seed=0):
    """-> (patches, upstream) float32 arrays.  The patches are the slices of one padded plane whose samples come from three bands,
    [-0.35, -0.05], [0.05, 0.95] and [1.05, 1.35], chosen per sample, plus uniform noise of +-0.02 per patch element: the value
    before the clamp, a convex combination of such elements, stays 0.03 away from 0 and 1, and two thirds of the samples are clamped"""
    shape, g = case(name)
    rng = np.random.default_rng(2000 + seed + ord(name))
    full = (shape[0], shape[1], g["new_h"], g["new_w"])
    band = rng.integers(0, 3, size=full)
    lo = np.array([-0.35, 0.05, 1.05])[band]
    hi = np.array([-0.05, 0.95, 1.35])[band]
    plane = lo + (hi - lo) * rng.random(full)
    p = slices_of(torch.from_numpy(plane), g).numpy()
    p = p + rng.uniform(-0.02, 0.02, size=p.shape)
    w = rng.uniform(-1.0, 1.0, size=shape)
    return p.astype(np.float32), w.astype(np.float32)


def ola_gradient(name, patches, upstream, dtype=torch.float64, clamp=True):
    """-> (d sum(upstream * overlap_add(patches)) / d patches, the value before the clamp), computed in `dtype`"""
    shape, g = case(name)
    p = torch.as_tensor(patches).to(dtype).requires_grad_(True)
    out, v = overlap_add(p, shape, g, clamp=clamp)
    out.backward(torch.as_tensor(upstream).to(dtype))
    return p.grad.numpy(), v.detach().numpy()


def rel_error(got, want):
    """largest |got - want| relative to the largest float64 entry"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())


# The bound of pb_overlap_add_backward against float64, relative to the case's largest entry: 6 x the restatement's own float32
# error E on that case's inputs (ola_inputs, seed 0) -- the factor of params_grad_ref.py and edgetaper_grad_ref.py --, recorded as
# measured on the CPU; tests/test_patch_autograd_cpu.py measures every E again and holds it to within a factor of two.
TOL_FACTOR = 6.0
E_OLA = {"a": 1.41e-7, "b": 1.13e-7, "c": 9.22e-8, "d": 1.17e-7, "e": 9.41e-8, "g": 1.11e-7}
TOL_OLA = {k: TOL_FACTOR * e for k, e in E_OLA.items()}


def measure_e(name):
    p, w = ola_inputs(name)
    g64, _ = ola_gradient(name, p, w)
    g32, _ = ola_gradient(name, p, w, dtype=torch.float32)
    return rel_error(g32, g64)


# ---------------------------------------------------------------------------------------------
# the module's parameter gradients: the float64 truth of the composition
# ---------------------------------------------------------------------------------------------
def composition_param_truth(x, w, name, n_iter, alpha, beta, method, c, b, ker_size):
    """float64 d sum(w * module(x)) / d (c, b, alpha, beta) of the patch branch on case `name`'s lattice, composed of this file's two
    ends around the float64 restatement of the blind call (estimation_grad_ref.blind, params_grad_ref.blind_param_grads): every
    patch is deblurred on its own, the overlap-add's float64 backward hands each patch its upstream gradient, and the four
    gradients are summed over the patches.  -> (the four gradients, the output)"""
    import estimation_grad_ref as er
    import params_grad_ref as pr
    shape, g = case(name)
    B = shape[0]
    patches = extract(torch.as_tensor(np.array(x, np.float64)), g).numpy()
    runs = [er.blind(patches[n * B:(n + 1) * B], n_iter, alpha, beta, method, c, b, ker_size) for n in range(g["n_i"] * g["n_j"])]
    restored = torch.tensor(np.concatenate([out for out, _ in runs]), requires_grad=True)
    out, _ = overlap_add(restored, shape, g)
    out.backward(torch.as_tensor(np.array(w, np.float64)))
    up = restored.grad.numpy()
    total = np.zeros(4)
    for n, (_, steps) in enumerate(runs):
        total += pr.blind_param_grads(patches[n * B:(n + 1) * B], up[n * B:(n + 1) * B], n_iter, alpha, beta, method, c, b, steps=steps)
    return total, out.detach().numpy()


# The module's parameter test (tests/test_gpu_patch_autograd.py): case a's image (synthetic_blurry_batch(2, 3, 150, 210, seed0=23)) under
# the upstream weights default_rng(31).uniform(0.5, 1.5), the image as data.  PARAM_TRUTH is composition_param_truth of that setting,
# recorded (a minute on a CPU: too long for a test).  E_PARAMS is the error of the same composition run in float32 on the GPU -- torch
# ops around the package's polyblur_deblurring, one call per patch -- against it, relative to the larger gradient of the pair, as the
# GPU test measured it; the test measures it again and holds the record to within a factor of two, and its bound is TOL_FACTOR x E.
# d c and d b come through sixty estimations of 64 x 64 patches of a real image, twice each: E is a thousand times
# params_grad_ref.E_BLIND, whose images were searched for their margins from every tie and clamp of the estimation.
PARAM_SETTING = dict(case="a", n_iter=2, alpha=6, beta=1, ker_size=13, method="fft", c=0.352, b=0.768)
PARAM_TRUTH = {"c,b": [-11.18996590920141, 5.886422327441088], "alpha,beta": [0.10388099767806125, -1.159531798255557]}
E_PARAMS = {"c,b": 4.65e-3, "alpha,beta": 5.27e-5}
