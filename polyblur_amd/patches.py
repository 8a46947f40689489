"""The two ends of ``PolyblurDeblurring(patch_decomposition=True)`` as public functions (reference deblurring.py:269-340,
fix-forward): ``image_to_patches`` cuts a (B,C,H,W) image into the overlapping patches of the reference's lattice,
``patches_to_image`` blends them back with the periodic Kaiser(beta=5) window.

    patches = image_to_patches(images, patch_size=400, patch_overlap=0.25)        # (n_i*n_j*B, C, ph, pw), patch n of image b at [n*B + b]
    images  = patches_to_image(patches, (H, W), patch_size=400, patch_overlap=0.25)

Both take float32 or float16 tensors; a ROCm tensor is used in place on torch's current stream, a CPU tensor goes through the GPU.
The kernels are those of the module's patch branch (pb_extract_patches, pb_overlap_add): the same bits.  A float32 ROCm tensor
that requires grad takes the two autograd.Functions of _autograd.py, whose backward passes are the engine's
(pb_extract_patches_backward, pb_overlap_add_backward); their forwards are the same two calls.  No gradient with respect to the
window or the lattice; float16 and CPU tensors are refused under grad.
"""
from __future__ import annotations

import numpy as np

from . import _capi as capi
from ._frontend import CPU_WITH_GRAD, FLOAT32_ONLY, bound_engine, is_tensor, refuse_under_grad, wants_grad


def kaiser_window_periodic(n: int, beta: float = 5.0) -> np.ndarray:
    """torch.kaiser_window(n, periodic=True, beta) (deblurring.py:352): the symmetric window of
    length n+1 without its last sample."""
    if n == 1:
        return np.ones(1, np.float32)
    k = np.arange(n, dtype=np.float64)
    r = 2.0 * k / n - 1.0
    return (np.i0(beta * np.sqrt(np.maximum(0.0, 1.0 - r * r))) / np.i0(beta)).astype(np.float32)


def patch_grid(h: int, w: int, patch_size, overlap: float):
    """The reference's patch lattice (deblurring.py:281-299): steps, padded size, pads, counts."""
    ph, pw = patch_size
    step_h, step_w = int(ph * (1 - overlap)), int(pw * (1 - overlap))
    new_h = int(np.ceil((h - ph) / step_h) * step_h) + ph
    new_w = int(np.ceil((w - pw) / step_w) * step_w) + pw
    pad_top, pad_left = int(np.floor((new_h - h) / 2)), int(np.floor((new_w - w) / 2))
    n_i = len(range(0, new_h - ph + 1, step_h))
    n_j = len(range(0, new_w - pw + 1, step_w))
    return dict(ph=ph, pw=pw, step_h=step_h, step_w=step_w, new_h=new_h, new_w=new_w, pad_top=pad_top,
                pad_left=pad_left, n_i=n_i, n_j=n_j)


def check_lattice(h, w, patch_size, overlap):
    """-> patch_grid of the even part of an h x w image; a plain error for what the reference's arithmetic leaves without a single
    patch -- an image shorter than patch_size - step along an axis gives new_h < patch_size at deblurring.py:284-285 and an empty
    I_coords at :294: the reference's branch, could it run, would return zeros there"""
    if min(patch_size) < 2 or int(patch_size[0] * (1 - overlap)) < 1 or int(patch_size[1] * (1 - overlap)) < 1:
        raise ValueError("patch size / overlap incompatible: patches of at least 2x2 with a positive step are needed")
    g = patch_grid(h // 2 * 2, w // 2 * 2, patch_size, overlap)
    if g["n_i"] < 1 or g["n_j"] < 1:
        raise ValueError("image %dx%d is smaller than patch_size - step along an axis: the reference's lattice (deblurring.py:284-295) "
                         "holds no patch for it -- use a smaller patch_size or patch_decomposition=False" % (h, w))
    return g


def _pair(patch_size):
    return (int(patch_size), int(patch_size)) if isinstance(patch_size, (int, np.integer)) else tuple(int(v) for v in patch_size)


def _check(t, what):
    import torch
    if not is_tensor(t) or t.dim() != 4:
        raise ValueError("%s expects a 4-D tensor" % what)
    if t.dtype not in (torch.float32, torch.float16):
        raise TypeError("tensor dtype must be float32 or float16")


def _refuse(t, what):
    """under grad, anything but a float32 ROCm tensor"""
    import torch
    if t.dtype != torch.float32:
        refuse_under_grad(what + " of a float16 tensor", FLOAT32_ONLY)
    if not t.is_cuda:
        refuse_under_grad(what, CPU_WITH_GRAD % "the tensor")


def even_part(x):
    """deblurring.py:273-279 make the size even: the last row / column of an odd side is dropped"""
    h, w = x.shape[-2:]
    if h % 2 == 1:
        x = x[..., :-1, :]
    if w % 2 == 1:
        x = x[..., :, :-1]
    return x.contiguous()


def windows(grid, device):
    """the periodic Kaiser(beta=5) window of each axis, float32 on `device` (deblurring.py:352)"""
    import torch
    return (torch.from_numpy(kaiser_window_periodic(grid["ph"])).to(device), torch.from_numpy(kaiser_window_periodic(grid["pw"])).to(device))


def extract(x, grid):
    """all patches of the even-sized, contiguous ROCm tensor x -- under grad through the Function"""
    import torch
    if wants_grad(x):
        from ._autograd import ExtractPatchesFunction
        return ExtractPatchesFunction.apply(x, grid)
    B, Cc = x.shape[:2]
    n_p = grid["n_i"] * grid["n_j"]
    patches = torch.empty((n_p * B, Cc, grid["ph"], grid["pw"]), dtype=x.dtype, device=x.device)
    with bound_engine(x) as eng:
        eng.extract_patches_ptr(x.data_ptr(), patches.data_ptr(), capi.PB_F32 if x.dtype == torch.float32 else capi.PB_F16, x.shape, grid, 0, n_p)
    return patches


def blend(patches, shape, grid):
    """the overlap-add of the contiguous ROCm patches into an image of `shape` -- under grad through the Function"""
    import torch
    wy, wx = windows(grid, patches.device)
    if wants_grad(patches):
        from ._autograd import OverlapAddFunction
        return OverlapAddFunction.apply(patches, tuple(int(v) for v in shape), grid, wy, wx)
    out = torch.empty(tuple(shape), dtype=patches.dtype, device=patches.device)
    with bound_engine(patches) as eng:
        eng.overlap_add_ptr(patches.data_ptr(), out.data_ptr(), capi.PB_F32 if patches.dtype == torch.float32 else capi.PB_F16, shape, grid,
                            wy.data_ptr(), wx.data_ptr())        # (wy / wx are torch's: the allocator keeps them until the stream has passed)
    return out


def image_to_patches(images, patch_size=400, patch_overlap=0.25):
    """(B,C,H,W) -> (n_i*n_j*B, C, ph, pw): the image, its odd sides made even, replicate-padded to the lattice of ``patch_size``
    (a number or (ph, pw)) and ``patch_overlap`` and cut; patch n = ki*n_j + kj of image b lies at [n*B + b]."""
    _check(images, "image_to_patches")
    ps = _pair(patch_size)
    g = check_lattice(images.shape[-2], images.shape[-1], ps, patch_overlap)
    if wants_grad(images):
        _refuse(images, "image_to_patches")
    x = even_part(images if images.is_cuda else images.cuda())
    patches = extract(x, g)
    return patches if images.is_cuda else patches.cpu()


def patches_to_image(patches, image_size, patch_size=400, patch_overlap=0.25):
    """(n_i*n_j*B, C, ph, pw) -> (B,C,H,W), H x W the even part of ``image_size`` (the last two of any longer shape): every patch
    weighted by the periodic Kaiser(beta=5) window, summed, divided by the summed window + 1e-8, clamped to [0, 1] and cropped of
    the lattice's pad.  Under grad the clamp passes the gradient where the value lies in [0, 1], both ends included."""
    _check(patches, "patches_to_image")
    ps = _pair(patch_size)
    h, w = (int(v) for v in tuple(image_size)[-2:])
    g = check_lattice(h, w, ps, patch_overlap)
    n_p = g["n_i"] * g["n_j"]
    if tuple(patches.shape[-2:]) != ps or patches.shape[0] % n_p != 0:
        raise ValueError("patches of shape %r are not the %d x %d patches of %dx%d of a %dx%d image" %
                         (tuple(patches.shape), g["n_i"], g["n_j"], ps[0], ps[1], h, w))
    if wants_grad(patches):
        _refuse(patches, "patches_to_image")
    p = (patches if patches.is_cuda else patches.cuda()).contiguous()
    out = blend(p, (p.shape[0] // n_p, p.shape[1], h // 2 * 2, w // 2 * 2), g)
    return out if patches.is_cuda else out.cpu()
