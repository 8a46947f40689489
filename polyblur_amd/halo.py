"""Halo masking and the spectral derivative as public, differentiable functions (reference deblurring.py:193-208,
filters.py:159-186):

    from polyblur_amd import fourier_gradients, halo_masking

``fourier_gradients(img)`` -> ``(grad_x, grad_y)``; ``halo_masking(img, imout, grad_img=None)`` -> the masked image, unclamped.
Same names and arguments as the reference's; bug-compatible with it (M = -grad_x * gout_x - grad_y * grad_y, deblurring.py:174).
The operands are (B,C,H,W) float32 ``torch.Tensor`` s -- on a ROCm device (used in place, on torch's current stream) or on the
CPU (staged through the GPU) -- or ``np.ndarray`` s; the result has the kind of ``img``.

Gradients: with autograd enabled and an operand that requires grad both return tensors with a ``grad_fn`` --
``halo_masking`` with respect to ``img``, ``imout`` and both planes of ``grad_img`` (with ``grad_img=None`` these are
``fourier_gradients(img)``, inside the graph).  The backward passes are the engine's (pb_halo_mask_backward,
pb_fourier_gradients_backward); no double backward.  Under grad: float32 ROCm tensors only (NotImplementedError before any
device work).  ``inverse_filtering_rank3(remove_halo=True)`` and the blind driver compose these under grad.

The arithmetic is the HIP engine's; nothing runs on the CPU.
"""
from __future__ import annotations

import numpy as np

from ._frontend import (HALO_ONLY, check_grad_img, check_image, check_image_size, is_rocm_float32, refuse_under_grad, staged,
                        wants_grad)

_GRAD_ONLY = "the spectral derivative is differentiated for float32 ROCm tensors only"


def _gradients(img):
    shape = tuple(img.shape)
    return staged(img, np.float32, lambda eng, i, o, ex: eng.fourier_gradients_ptr(i, shape, o[0], o[1]), outputs=("np.gx", "np.gy"))[0]


def _mask(img, imout, gx, gy):
    shape = tuple(img.shape)
    return staged(img, np.float32, lambda eng, i, o, ex: eng.halo_mask_ptr(i, ex[0], ex[1], ex[2], o[0], shape),
                  (("np.y", imout), ("np.g0x", gx), ("np.g0y", gy)))[0][0]


def fourier_gradients(img):
    """filters.fourier_gradients (filters.py:159-186): the spectral derivatives of ``img`` along x (columns) and y (rows)."""
    shape, dt = check_image(img, allow_half=False)
    if wants_grad(img):
        if not is_rocm_float32(img):
            refuse_under_grad("fourier_gradients", _GRAD_ONLY)
        check_image_size(*shape[-2:])
        from ._autograd import FourierGradientsFunction
        return FourierGradientsFunction.apply(img, _gradients)
    check_image_size(*shape[-2:])
    gx, gy = _gradients(img)
    return gx, gy


def halo_masking(img, imout, grad_img=None):
    """deblurring.halo_masking (deblurring.py:193-208), unclamped: imout + z (img - imout) with z = max(M / (nM + M), 0).
    ``grad_img``: (grad_x, grad_y) of the original image, or None for ``fourier_gradients(img)``."""
    shape, dt = check_image(img, allow_half=False)
    oshape, _ = check_image(imout, allow_half=False)
    if oshape != shape:
        raise ValueError("imout must have the image's shape %r, got %r" % (shape, oshape))
    if grad_img is not None:
        check_grad_img(grad_img, shape)
    operands = (img, imout) + (tuple(grad_img) if grad_img is not None else ())
    if wants_grad(*operands):
        if not all(is_rocm_float32(t) for t in operands):
            refuse_under_grad("halo_masking", HALO_ONLY)
        check_image_size(*shape[-2:])
        gx, gy = fourier_gradients(img) if grad_img is None else grad_img
        from ._autograd import HaloMaskingFunction
        return HaloMaskingFunction.apply(img, imout, gx, gy, _mask)
    check_image_size(*shape[-2:])
    gx, gy = fourier_gradients(img) if grad_img is None else grad_img
    return _mask(img, imout, gx, gy)
