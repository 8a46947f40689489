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

Learnable parameters: ``c`` and ``b`` of the affine model sigma^2 = c^2 / (m^2 + 1e-8) - b^2 are Python numbers or
one-element tensors (0-dim or of shape (1,), float32 or float64, on the CPU or on the image's device; more elements: ValueError).
A tensor's value is read once per call with ``float(t)`` -- one synchronisation where it lives on a device -- and the forward is the
forward with that float, bit for bit.  Where autograd is on and a parameter requires grad the result has a ``grad_fn`` -- a parameter
alone is enough: the calibration case, an image that is data, computes no image gradient -- and its ``.grad`` comes from the same
backward call (pb_estimate_blur_params_backward: d c = sum_e dv_e 2 c / (m_e^2 + 1e-8), d b = -2 b sum_e dv_e per image; a clamped
sigma^2 or rho^2 contributes exactly 0), summed over the images in index order in float64, in the parameter's shape, dtype and
device.  Such a parameter beside an image that is not a float32 ROCm tensor: NotImplementedError before any device work.
"""
from __future__ import annotations

import numpy as np

from . import _capi as capi
from ._frontend import (CPU_WITH_GRAD, DTYPES, FLOAT32_ONLY, NO_QUANTILE, build_options, check_image, check_image_size, check_param,
                        host_array, is_tensor, param_value, refuse_params, refuse_under_grad, staged, wants_grad)

_F32 = capi.INFO_DTYPE.itemsize // 4                          # a record in float32 words
_OFF = {name: capi.INFO_DTYPE.fields[name][1] // 4 for name in ("kernel", "sigma", "rho", "theta")}


def _check_grid(given, want, name):
    if given is None:
        return
    g = np.asarray(host_array(given), np.float64).reshape(-1)
    if g.shape != want.shape or not np.allclose(g, want, rtol=0, atol=1e-4):
        raise ValueError("%s must be None or the grid its count implies (%d values from %g in steps of %g): the engine's "
                         "directions are fixed" % (name, want.size, want[0], want[1] - want[0] if want.size > 1 else 0.0))


def _records(img, dt, opts):
    """the B estimation records of img as (B, words) float32, in its kind"""
    shape = tuple(img.shape)
    return staged(img, dt, lambda eng, i, o, ex: eng.estimate_blur_ptr(i, DTYPES[dt], shape, opts, o[0]),
                  outputs=(("np.info", (shape[0], _F32)),))[0][0]


def _copy(a):
    return a.clone() if is_tensor(a) else a.copy()            # (never a view of the records)


def _kernel_of(rec, k):
    """the (B,1,k,k) kernels of B records -- a (B, words) float32 tensor or array --, cropped about the centre of their 25 x 25"""
    k25 = rec[:, _OFF["kernel"]:_OFF["kernel"] + capi.PB_KSIZE * capi.PB_KSIZE].reshape(rec.shape[0], 1, capi.PB_KSIZE, capi.PB_KSIZE)
    r0 = capi.PB_KSIZE // 2 - k // 2
    return _copy(k25[..., r0:r0 + k, r0:r0 + k])


def _params_of(rec):
    return tuple(_copy(rec[:, _OFF[n]:_OFF[n] + 1]) for n in ("sigma", "rho", "theta"))


def gaussian_blur_estimation(imgc, q=0.0001, n_angles=6, n_interpolated_angles=30, c=0.362, b=0.464, ker_size=25,
                             discard_saturation=False, multichannel=False, thetas=None, interpolated_thetas=None,
                             return_2d_filters=True):
    """blur_estimation.gaussian_blur_estimation (blur_estimation.py:18-79) -- see the module docstring.  With
    ``return_2d_filters=False`` the tuple (sigmas, rhos, thetas) is built fix-forward: the reference's branch raises NameError
    (blur_estimation.py:77)."""
    shape, dt = check_image(imgc, allow_half=True)
    if return_2d_filters and isinstance(ker_size, (int, np.integer)) and 2 <= ker_size <= capi.PB_KSIZE_MAX and \
            (ker_size % 2 == 0 or ker_size > capi.PB_KSIZE):
        raise NotImplementedError("gaussian_blur_estimation returns odd kernels of 3 to 25 taps a side: an even grid's placement depends on "
                                  "the method, which this function does not take, and larger kernels do not live in the estimation record")
    params = (check_param(c, "c", imgc), check_param(b, "b", imgc))
    refuse_params("gaussian_blur_estimation", imgc, c=params[0], b=params[1])
    want_grad = wants_grad(imgc, *params)
    if want_grad:
        what = "gaussian_blur_estimation"
        if dt == np.float16:
            refuse_under_grad(what + " of a float16 image", FLOAT32_ONLY)
        if q > 0:
            refuse_under_grad(what + "(q=%g)" % q, NO_QUANTILE)
        if not imgc.is_cuda:
            refuse_under_grad(what, CPU_WITH_GRAD % "imgc")
    c, b = param_value(c), param_value(b)                     # (a device parameter is read here, behind the refusals under grad)
    opts = build_options(shape[1], 1, c, b, 2, 3, 0.8, 2.0, ker_size, q, n_angles, n_interpolated_angles, False, False, False,
                         discard_saturation, multichannel, "fft", "full", "bilateral")
    _check_grid(thetas, np.linspace(0, 180, n_angles + 1), "thetas")
    _check_grid(interpolated_thetas, np.arange(n_interpolated_angles) * (180 / n_interpolated_angles), "interpolated_thetas")
    check_image_size(*shape[-2:])
    k = int(ker_size)
    if params[0] is not None or params[1] is not None:
        from ._autograd import EstimationParamsFunction
        return EstimationParamsFunction.apply(imgc, params[0], params[1], opts, k, bool(return_2d_filters), lambda x: _records(x, dt, opts),
                                              (lambda rec: _kernel_of(rec, k)) if return_2d_filters else _params_of)
    if want_grad:
        from ._autograd import EstimationFunction
        return EstimationFunction.apply(imgc, opts, k, bool(return_2d_filters), lambda x: _records(x, dt, opts),
                                        (lambda rec: _kernel_of(rec, k)) if return_2d_filters else _params_of)
    rec = _records(imgc, dt, opts)
    return _kernel_of(rec, k) if return_2d_filters else _params_of(rec)
