"""The reference's blur estimation as a public, differentiable function (blur_estimation.py:18-79):

    from polyblur_amd import gaussian_blur_estimation

Same name, arguments and defaults.  ``imgc`` is a (B,C,H,W) ``torch.Tensor`` -- on a ROCm device (used in place, on torch's
current stream) or on the CPU (staged through the GPU) -- or an ``np.ndarray`` of that shape; float32 or float16.  The result is
the float32 (B,1,k,k) Gaussian kernel of every image, of the input's kind and device: the very taps the blind driver deblurs
with (``polyblur_deblurring(..., n_iter=1, return_info=True)`` reports the same bits for the same image and options).

``return_2d_filters=False`` returns ``(sigmas, rhos, thetas)``, each (B,1), thetas in radians.  The reference's own branch dies
on an undefined name (blur_estimation.py:77, ``theta``); it is built fix-forward here: the direction is the ``thetas`` that
find_maximal_blur_direction returned.

What is refused: with ``return_2d_filters=True`` an even ``ker_size`` or one above 25 (NotImplementedError: the function takes no
``method``, on which the placement of an even grid depends, and larger kernels do not live in the estimation record);
``thetas`` / ``interpolated_thetas`` other than ``None`` or the grids that ``n_angles`` / ``n_interpolated_angles`` imply
(ValueError: the engine's directions are those grids); ``multichannel=True`` with C not in {1, 3} (NotImplementedError, as the
blind driver; for C in {1, 3} the reference estimates on the gray image either way).

Gradients (the reference's README: "fully differentiable"): when autograd is enabled and ``imgc`` requires grad the result has
a ``grad_fn``; the backward pass is the engine's (pb_estimate_blur_backward) -- through the taps, sigma and rho,
the affine model, the cubic interpolation, the directional maxima (to the arg-max pixel, as torch.amax), the spectral derivative
and the min / max normalisation (shared among ties, as torch.amin / amax).  Under grad: float32 ROCm tensors and ``q=0`` only
(``q=0`` is what the blind driver defaults to; the backward of torch.quantile is not built) -- NotImplementedError before any
device work otherwise.  No double backward.  Without grad nothing is recorded and ``q`` is free.
"""
from __future__ import annotations

import numpy as np

from . import _capi as capi
from .deblurring import _build_options, _check_image_size, _is_torch_tensor
from .engine import get_engine
from .nonblind import _check_image, _host_array, _refuse_under_grad

_F32 = capi.INFO_DTYPE.itemsize // 4                          # a record in float32 words
_OFF = {name: capi.INFO_DTYPE.fields[name][1] // 4 for name in ("kernel", "sigma", "rho", "theta")}


def _check_grid(given, want, name):
    if given is None:
        return
    g = np.asarray(_host_array(given), np.float64).reshape(-1)
    if g.shape != want.shape or not np.allclose(g, want, rtol=0, atol=1e-4):
        raise ValueError("%s must be None or the grid its count implies (%d values from %g in steps of %g): the engine's "
                         "directions are fixed" % (name, want.size, want[0], want[1] - want[0] if want.size > 1 else 0.0))


def _crop(kernel25, k):
    r0 = capi.PB_KSIZE // 2 - k // 2
    return kernel25[..., r0:r0 + k, r0:r0 + k]


_ESTIMATION_FUNCTION = None


def _estimation_function():
    """the autograd.Function of the estimation (made on first use: torch is imported lazily in this module)"""
    global _ESTIMATION_FUNCTION
    if _ESTIMATION_FUNCTION is not None:
        return _ESTIMATION_FUNCTION
    import torch
    from torch.autograd.function import once_differentiable

    class EstimationFunction(torch.autograd.Function):
        """gaussian_blur_estimation of a ROCm float32 image with q = 0; the records stay on the device for the backward"""

        @staticmethod
        def forward(ctx, img, opts, ker_size, filters):
            x = img.detach().contiguous()
            rec = _estimate_device(x, capi.PB_F32, opts)
            ctx.save_for_backward(x, rec)
            ctx.pb = (opts, int(ker_size), bool(filters))
            if filters:
                return _kernel_of(rec, ker_size)
            sigma, rho, theta = _params_of(rec)
            ctx.mark_non_differentiable(theta)                # (it comes from integer tensors: blur_estimation.py:160-167)
            return sigma, rho, theta

        @staticmethod
        @once_differentiable
        def backward(ctx, *grads):
            x, rec = ctx.saved_tensors
            opts, ker_size, filters = ctx.pb
            dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
            eng = get_engine(dev)
            gk = gsr = None
            if filters:
                gk = grads[0].detach().to(torch.float32).contiguous()
            else:
                gsr = torch.cat([grads[0].detach().to(torch.float32).reshape(-1, 1), grads[1].detach().to(torch.float32).reshape(-1, 1)], dim=1).contiguous()
            gin = torch.empty_like(x)
            with torch.cuda.device(dev):
                eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
                eng.estimate_blur_backward_ptr(x.data_ptr(), x.shape, opts, rec.data_ptr(), gk.data_ptr() if filters else None,
                                               None if filters else gsr.data_ptr(), ker_size if filters else capi.PB_KSIZE, gin.data_ptr())
            return gin, None, None, None

    _ESTIMATION_FUNCTION = EstimationFunction
    return EstimationFunction


def _estimate_device(x, dtype, opts):
    """B estimation records of the contiguous ROCm tensor x, as a (B, words) float32 tensor on its device"""
    import torch
    dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
    eng = get_engine(dev)
    rec = torch.empty((x.shape[0], _F32), dtype=torch.float32, device=x.device)
    with torch.cuda.device(dev):
        eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        eng.estimate_blur_ptr(x.data_ptr(), dtype, x.shape, opts, rec.data_ptr())
    return rec


def _kernel_of(rec, k):
    B = rec.shape[0]
    k25 = rec[:, _OFF["kernel"]:_OFF["kernel"] + capi.PB_KSIZE * capi.PB_KSIZE].view(B, 1, capi.PB_KSIZE, capi.PB_KSIZE)
    return _crop(k25, k).clone()                              # (never a view of the records)


def _params_of(rec):
    return tuple(rec[:, _OFF[n]:_OFF[n] + 1].clone() for n in ("sigma", "rho", "theta"))


def gaussian_blur_estimation(imgc, q=0.0001, n_angles=6, n_interpolated_angles=30, c=0.362, b=0.464, ker_size=25,
                             discard_saturation=False, multichannel=False, thetas=None, interpolated_thetas=None,
                             return_2d_filters=True):
    """blur_estimation.gaussian_blur_estimation (blur_estimation.py:18-79) -- see the module docstring.  With
    ``return_2d_filters=False`` the tuple (sigmas, rhos, thetas) is built fix-forward: the reference's branch raises NameError
    (blur_estimation.py:77)."""
    tensor, shape, dt = _check_image(imgc, allow_half=True)
    if return_2d_filters and isinstance(ker_size, (int, np.integer)) and 2 <= ker_size <= capi.PB_KSIZE_MAX and \
            (ker_size % 2 == 0 or ker_size > capi.PB_KSIZE):
        raise NotImplementedError("gaussian_blur_estimation returns odd kernels of 3 to 25 taps a side: an even grid's placement depends on "
                                  "the method, which this function does not take, and larger kernels do not live in the estimation record")
    want_grad = False
    if tensor:
        import torch
        want_grad = torch.is_grad_enabled() and imgc.requires_grad
    if want_grad:
        what = "gaussian_blur_estimation"
        if imgc.dtype == torch.float16:
            _refuse_under_grad(what + " of a float16 image", "gradients are built for float32 images")
        if q > 0:
            _refuse_under_grad(what + "(q=%g)" % q, "the backward of torch.quantile is not built -- pass q=0, which is what the blind driver defaults to")
        if not imgc.is_cuda:
            _refuse_under_grad(what, "imgc requires grad and is a CPU tensor -- gradients are built for ROCm tensors only")
    opts = _build_options(shape[1], 1, c, b, 2, 3, 0.8, 2.0, ker_size, q, n_angles, n_interpolated_angles, False, False, False,
                          discard_saturation, multichannel, "fft", "full", "bilateral")
    _check_grid(thetas, np.linspace(0, 180, n_angles + 1), "thetas")
    _check_grid(interpolated_thetas, np.arange(n_interpolated_angles) * (180 / n_interpolated_angles), "interpolated_thetas")
    _check_image_size(*shape[-2:])
    k = int(ker_size)
    if want_grad:
        return _estimation_function().apply(imgc, opts, k, bool(return_2d_filters))
    if tensor and imgc.is_cuda:
        rec = _estimate_device(imgc.detach().contiguous(), capi.PB_F16 if dt == np.float16 else capi.PB_F32, opts)
        return _kernel_of(rec, k) if return_2d_filters else _params_of(rec)
    eng = get_engine(0)
    eng.set_stream(0)
    info = eng.estimate_blur(np.ascontiguousarray(_host_array(imgc), dtype=dt), opts)
    if return_2d_filters:
        out = (np.ascontiguousarray(_crop(info["kernel"], k))[:, None],)
    else:
        out = tuple(np.ascontiguousarray(info[n], np.float32)[:, None] for n in ("sigma", "rho", "theta"))
    if tensor:
        import torch
        out = tuple(torch.from_numpy(o) for o in out)
    return out[0] if return_2d_filters else out
