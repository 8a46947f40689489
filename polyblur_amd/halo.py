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

from .deblurring import _check_image_size, _is_torch_tensor
from .engine import get_engine
from .nonblind import _check_image, _host_array, _refuse_under_grad

_HALO_ONLY = "halo masking is differentiated for float32 ROCm tensors only"
_GRAD_ONLY = "the spectral derivative is differentiated for float32 ROCm tensors only"


def _requires_grad(*ts):
    ts = [t for t in ts if _is_torch_tensor(t)]
    if not ts:
        return False
    import torch
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _rocm_float32(t):
    if not _is_torch_tensor(t):
        return False
    import torch
    return t.is_cuda and t.dtype == torch.float32


def _engine_of(t):
    import torch
    dev = t.device.index if t.device.index is not None else torch.cuda.current_device()
    return dev, get_engine(dev)


_FUNCTIONS = None


def _functions():
    """the two autograd.Functions (made on first use: torch is imported lazily in this module)"""
    global _FUNCTIONS
    if _FUNCTIONS is not None:
        return _FUNCTIONS
    import torch
    from torch.autograd.function import once_differentiable

    class FourierGradientsFunction(torch.autograd.Function):
        """fourier_gradients of a ROCm float32 tensor: linear, nothing is saved"""

        @staticmethod
        def forward(ctx, img):
            x = img.detach().contiguous()
            gx, gy = torch.empty_like(x), torch.empty_like(x)
            dev, eng = _engine_of(x)
            with torch.cuda.device(dev):
                eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
                eng.fourier_gradients_ptr(x.data_ptr(), x.shape, gx.data_ptr(), gy.data_ptr())
            ctx.set_materialize_grads(False)                  # (an output the loss does not reach: None, and no transform for it)
            return gx, gy

        @staticmethod
        @once_differentiable
        def backward(ctx, ggx, ggy):
            if ggx is None and ggy is None:
                return None
            ggx, ggy = (None if g is None else g.detach().to(torch.float32).contiguous() for g in (ggx, ggy))
            like = ggx if ggx is not None else ggy
            gin = torch.empty_like(like)
            dev, eng = _engine_of(like)
            with torch.cuda.device(dev):
                eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
                eng.fourier_gradients_backward_ptr(None if ggx is None else ggx.data_ptr(), None if ggy is None else ggy.data_ptr(),
                                                   like.shape, gin.data_ptr())
            return gin

    class HaloMaskingFunction(torch.autograd.Function):
        """halo_masking of ROCm float32 tensors with given gradient planes"""

        @staticmethod
        def forward(ctx, img, imout, gx, gy):
            x, y, a, b = (t.detach().contiguous() for t in (img, imout, gx, gy))
            out = torch.empty_like(x)
            dev, eng = _engine_of(x)
            with torch.cuda.device(dev):
                eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
                eng.halo_mask_ptr(x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), out.data_ptr(), x.shape)
            ctx.save_for_backward(x, y, a, b)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_out):
            x, y, a, b = ctx.saved_tensors
            g = grad_out.detach().to(torch.float32).contiguous()
            outs = [torch.empty_like(x) if need else None for need in ctx.needs_input_grad[:4]]
            dev, eng = _engine_of(x)
            with torch.cuda.device(dev):
                eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
                eng.halo_mask_backward_ptr(x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), g.data_ptr(),
                                           *[o.data_ptr() if o is not None else None for o in outs], x.shape)
            return tuple(outs)

    _FUNCTIONS = (FourierGradientsFunction, HaloMaskingFunction)
    return _FUNCTIONS


def fourier_gradients(img):
    """filters.fourier_gradients (filters.py:159-186): the spectral derivatives of ``img`` along x (columns) and y (rows)."""
    tensor, shape, dt = _check_image(img, allow_half=False)
    if _requires_grad(img):
        if not _rocm_float32(img):
            _refuse_under_grad("fourier_gradients", _GRAD_ONLY)
        _check_image_size(*shape[-2:])
        return _functions()[0].apply(img)
    _check_image_size(*shape[-2:])
    if tensor and img.is_cuda:
        import torch
        x = img.detach().contiguous()
        gx, gy = torch.empty_like(x), torch.empty_like(x)
        dev, eng = _engine_of(x)
        with torch.cuda.device(dev):
            eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            eng.fourier_gradients_ptr(x.data_ptr(), x.shape, gx.data_ptr(), gy.data_ptr())
        return gx, gy
    eng = get_engine(0)
    eng.set_stream(0)
    gx, gy = eng.fourier_gradients(np.ascontiguousarray(_host_array(img), np.float32))
    if tensor:
        import torch
        return torch.from_numpy(gx), torch.from_numpy(gy)
    return gx, gy


def _check_grad_img(grad_img, shape):
    if not isinstance(grad_img, (tuple, list)) or len(grad_img) != 2:
        raise ValueError("grad_img must be (grad_x, grad_y)")
    for gpart in grad_img:
        if not (_is_torch_tensor(gpart) or isinstance(gpart, np.ndarray)):
            raise TypeError("grad_img planes must be numpy.ndarrays or torch.Tensors")
        if tuple(int(v) for v in gpart.shape) != shape:
            raise ValueError("grad_img planes must have the image's shape %r" % (shape,))


def halo_masking(img, imout, grad_img=None):
    """deblurring.halo_masking (deblurring.py:193-208), unclamped: imout + z (img - imout) with z = max(M / (nM + M), 0).
    ``grad_img``: (grad_x, grad_y) of the original image, or None for ``fourier_gradients(img)``."""
    tensor, shape, dt = _check_image(img, allow_half=False)
    _, oshape, _ = _check_image(imout, allow_half=False)
    if oshape != shape:
        raise ValueError("imout must have the image's shape %r, got %r" % (shape, oshape))
    if grad_img is not None:
        _check_grad_img(grad_img, shape)
    operands = (img, imout) + (tuple(grad_img) if grad_img is not None else ())
    if _requires_grad(*operands):
        if not all(_rocm_float32(t) for t in operands):
            _refuse_under_grad("halo_masking", _HALO_ONLY)
        _check_image_size(*shape[-2:])
        gx, gy = fourier_gradients(img) if grad_img is None else grad_img
        return _functions()[1].apply(img, imout, gx, gy)
    _check_image_size(*shape[-2:])
    if tensor and img.is_cuda:
        import torch
        x = img.detach().contiguous()
        y = torch.as_tensor(imout, dtype=torch.float32, device=x.device).detach().contiguous()
        if grad_img is None:
            gx, gy = fourier_gradients(x)
        else:
            gx, gy = (torch.as_tensor(g, dtype=torch.float32, device=x.device).detach().contiguous() for g in grad_img)
        out = torch.empty_like(x)
        dev, eng = _engine_of(x)
        with torch.cuda.device(dev):
            eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            eng.halo_mask_ptr(x.data_ptr(), y.data_ptr(), gx.data_ptr(), gy.data_ptr(), out.data_ptr(), x.shape)
        return out
    eng = get_engine(0)
    eng.set_stream(0)
    x = np.ascontiguousarray(_host_array(img), np.float32)
    if grad_img is None:
        gx, gy = eng.fourier_gradients(x)
    else:
        gx, gy = (_host_array(g) for g in grad_img)
    out = eng.halo_mask(x, _host_array(imout), gx, gy)
    if tensor:
        import torch
        return torch.from_numpy(out)
    return out
