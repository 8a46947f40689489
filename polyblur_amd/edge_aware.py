"""The edge-aware smoothing behind ``prefiltering=True`` as public functions (reference filters.py:107-148,
domain_transform.py:6-85, deblurring.py:99-110):

    from polyblur_amd import bilateral_filter, recursive_filter, normalized_convolution, edge_aware_filtering

``bilateral_filter(I, ksize=5, sigma_spatial=5.0, sigma_color=0.1)``, ``recursive_filter(I, sigma_s=60, sigma_r=0.4,
num_iterations=3, joint_image=None)`` and ``normalized_convolution(I, sigma_s=60, sigma_r=0.4, num_iterations=3)`` have the
reference's names, arguments and defaults; ``edge_aware_filtering(img, sigma_s, sigma_r, *, prefilter='bilateral')`` ->
``(img_smoothed, img_noise)`` with the three values of ``prefilter`` that ``polyblur_deblurring`` takes.  ``I`` is a (B,C,H,W)
float32 or float16 ``torch.Tensor`` -- on a ROCm device (used in place, on torch's current stream) or on the CPU (staged through
the GPU) -- or ``np.ndarray``; the result has the kind, device and dtype of ``I``.

The bilateral window is any odd ``ksize`` from 1 to 25 (an even one is refused: the reference puts an even window's spatial
weights one sample off its taps, filters.py:109 against utils.pad_with_kernel).

Gradients: with autograd on and ``I`` a float32 ROCm tensor that requires grad, ``bilateral_filter`` returns a
tensor with a ``grad_fn`` -- the same bits as under ``torch.no_grad()``; the backward pass is the engine's
(pb_bilateral_backward), with respect to the image, no double backward -- and ``edge_aware_filtering(prefilter='bilateral')``
returns ``(img_smoothed, img - img_smoothed)``, both in the graph.  ``recursive_filter`` is differentiable with
respect to ``I`` and to ``joint_image``: when either requires grad and both are float32 ROCm tensors on one device it returns a
tensor with a ``grad_fn`` -- again the bits of ``torch.no_grad()``; the backward pass is the engine's
(pb_dt_recursive_filter_backward), a gradient for each operand that asks for one (guided by itself, ``I.grad`` holds both
paths), none with respect to ``sigma_s`` / ``sigma_r``, no double backward.  Every other operand that requires grad -- a CPU or
float16 tensor, an array beside a tensor that requires grad, operands on two devices, ``normalized_convolution``, the other two
values of ``prefilter`` -- is refused before any device work; under ``torch.no_grad()`` the call runs.
``edge_aware_filtering(prefilter='domain_transform')`` and ``polyblur_deblurring(prefiltering=True,
prefilter='domain_transform')`` are still refused under grad (the follow-up); until then compose
``smooth = recursive_filter(x, sigma_s, sigma_r, 1); noise = x - smooth``.

The filters are the HIP engine's (pb_bilateral, pb_dt_recursive_filter, pb_dt_normalized_convolution); ``img_noise`` is the
subtraction ``img - img_smoothed`` in the image's own kind, as the reference writes it.
"""
from __future__ import annotations

import math

import numpy as np

from . import _capi as capi
from ._frontend import _PREFILTER, DTYPES, check_image, is_rocm_float32, is_tensor, refuse_under_grad, staged, wants_grad

_NO_GRAD = "the edge-aware filters are not differentiated"
_NC_MAX_SIDE = 8190                                # pb_dt_normalized_convolution: H, W <= 8190
_SIGMA_MIN = 1e-18                                 # below it -1 / (2 sigma^2) is not a float32


def _positive(name, v, least=0.0):
    v = float(v)
    if not (v > 0 and math.isfinite(v)):
        raise ValueError("%s must be positive and finite, got %r" % (name, v))
    if v < least:
        raise ValueError("%s must be at least %g, got %r" % (name, least, v))
    return v


def _iterations(n):
    if isinstance(n, bool) or not isinstance(n, (int, np.integer)):
        raise TypeError("num_iterations must be an integer, got %r" % (n,))
    if n < 1:
        raise ValueError("num_iterations must be at least 1, got %d" % n)
    return int(n)


def _bilateral(I, ksize, ss, sc, dt=np.dtype(np.float32)):
    """the one call of pb_bilateral: the public function's forward, and BilateralFunction's"""
    shape = tuple(I.shape)
    return staged(I, dt, lambda eng, i, o, ex: eng.bilateral_ptr(i, o[0], DTYPES[dt], shape, int(ksize), ss, sc))[0][0]


def bilateral_filter(I, ksize=5, sigma_spatial=5.0, sigma_color=0.1):
    """filters.bilateral_filter (filters.py:107-148): per plane, replicate pad of ``ksize // 2``, the weight of a tap
    exp(-(dx^2 + dy^2) / (2 sigma_spatial^2)) exp(-(v - centre)^2 / (2 sigma_color^2)), sum w v / (sum w + 1e-5).
    Differentiable with respect to ``I`` when it is a float32 ROCm tensor that requires grad (the module docstring)."""
    _, dt = check_image(I, allow_half=True)
    if isinstance(ksize, bool) or not isinstance(ksize, (int, np.integer)):
        raise TypeError("ksize must be an integer, got %r" % (ksize,))
    if ksize % 2 == 0:
        raise NotImplementedError("an even ksize is not built: the reference's even window puts its spatial weights one sample "
                                  "off its taps (got %d)" % ksize)
    if not 1 <= ksize <= capi.PB_KSIZE:
        raise NotImplementedError("ksize must be odd, from 1 to %d (got %d)" % (capi.PB_KSIZE, ksize))
    ss, sc = _positive("sigma_spatial", sigma_spatial, _SIGMA_MIN), _positive("sigma_color", sigma_color, _SIGMA_MIN)
    if wants_grad(I):
        if not is_rocm_float32(I):
            refuse_under_grad("bilateral_filter", _NO_GRAD)
        from ._autograd import BilateralFunction
        return BilateralFunction.apply(I, int(ksize), ss, sc, _bilateral)
    return _bilateral(I, int(ksize), ss, sc, dt)


def _recursive(I, joint_image, ss, sr, n, dt=np.dtype(np.float32)):
    """the one call of pb_dt_recursive_filter: the public function's forward, and RecursiveFilterFunction's"""
    shape = tuple(I.shape)
    extra = () if joint_image is None else (("np.joint", joint_image, dt.type),)
    return staged(I, dt, lambda eng, i, o, ex: eng.dt_recursive_filter_ptr(i, ex[0] if ex else None, o[0], DTYPES[dt], shape, ss, sr, n),
                  extra)[0][0]


def _describe(t):
    if not is_tensor(t):
        return type(t).__module__.split(".")[0] + "." + type(t).__name__
    return "%s tensor on %s" % (str(t.dtype).replace("torch.", ""), t.device)


def _recursive_grad_refusal(I, joint_image):
    """why ``recursive_filter`` cannot differentiate these operands, or None: both must be float32 ROCm tensors on one device"""
    operands = [I] if joint_image is None else [I, joint_image]
    if all(is_rocm_float32(t) for t in operands) and len({t.device for t in operands}) == 1:
        return None
    if not any(is_tensor(t) and t.is_cuda for t in operands):
        return _NO_GRAD                                # (no ROCm tensor in the call: the refusal it has always had)
    return ("gradients are built for float32 ROCm tensors on one device, I and joint_image alike (got I: %s%s)"
            % (_describe(I), "" if joint_image is None else ", joint_image: %s" % _describe(joint_image)))


def recursive_filter(I, sigma_s=60, sigma_r=0.4, num_iterations=3, joint_image=None):
    """domain_transform.recursive_filter (domain_transform.py:6-85): the domain-transform recursive filter, guided by
    ``joint_image`` (an image of ``I``'s shape, read in ``I``'s dtype) or by ``I`` itself.  Differentiable with respect to ``I``
    and ``joint_image`` when they are float32 ROCm tensors on one device and either requires grad (the module docstring)."""
    shape, dt = check_image(I, allow_half=True)
    ss, sr, n = _positive("sigma_s", sigma_s), _positive("sigma_r", sigma_r), _iterations(num_iterations)
    if joint_image is not None:
        try:
            jshape, _ = check_image(joint_image, allow_half=True)
        except TypeError as e:
            raise TypeError("joint_image: %s" % e) from None
        except ValueError:
            jshape = None
        if jshape != shape:
            raise ValueError("joint_image must have the image's shape %r, got %r" % (shape, tuple(joint_image.shape)))
    if wants_grad(I, joint_image):
        reason = _recursive_grad_refusal(I, joint_image)
        if reason is not None:
            refuse_under_grad("recursive_filter", reason)
        from ._autograd import RecursiveFilterFunction
        return RecursiveFilterFunction.apply(I, joint_image, ss, sr, n, _recursive)
    return _recursive(I, joint_image, ss, sr, n, dt)


def normalized_convolution(I, sigma_s=60, sigma_r=0.4, num_iterations=3):
    """The domain transform's normalized convolution (NC.cpp:143-204), per image; H and W up to 8190."""
    shape, dt = check_image(I, allow_half=True)
    ss, sr, n = _positive("sigma_s", sigma_s), _positive("sigma_r", sigma_r), _iterations(num_iterations)
    if shape[2] > _NC_MAX_SIDE or shape[3] > _NC_MAX_SIDE:
        raise NotImplementedError("normalized_convolution is built for H and W up to %d, got %d x %d" % (_NC_MAX_SIDE, shape[2], shape[3]))
    if wants_grad(I):
        refuse_under_grad("normalized_convolution", _NO_GRAD)
    return staged(I, dt, lambda eng, i, o, ex: eng.dt_normalized_convolution_ptr(i, o[0], DTYPES[dt], shape, ss, sr, n))[0][0]


def edge_aware_filtering(img, sigma_s, sigma_r, *, prefilter='bilateral'):
    """deblurring.edge_aware_filtering (deblurring.py:99-110) -> (img_smoothed, img_noise = img - img_smoothed).
    ``prefilter``: 'bilateral' -- the reference's live path, ``bilateral_filter(img)`` with its defaults, ``sigma_s`` and
    ``sigma_r`` unused (:107-108) --, 'domain_transform' (``recursive_filter`` with one iteration) or 'normalized_convolution'
    (``normalized_convolution`` with one iteration).  Under grad (a float32 ROCm ``img`` that requires grad, 'bilateral'): both
    results are in the graph."""
    check_image(img, allow_half=True)
    if prefilter not in _PREFILTER:
        raise ValueError("prefilter must be 'bilateral', 'domain_transform' or 'normalized_convolution'")
    under_grad = wants_grad(img)
    if under_grad and not (prefilter == "bilateral" and is_rocm_float32(img)):
        refuse_under_grad("edge_aware_filtering", _NO_GRAD)
    if prefilter == "bilateral":
        smooth = bilateral_filter(img)
    elif prefilter == "domain_transform":
        smooth = recursive_filter(img, sigma_s=sigma_s, sigma_r=sigma_r, num_iterations=1)
    else:
        smooth = normalized_convolution(img, sigma_s=sigma_s, sigma_r=sigma_r, num_iterations=1)
    if isinstance(img, np.ndarray):
        return smooth, (img.astype(smooth.dtype, copy=False) - smooth)
    return smooth, (img if under_grad else img.detach()) - smooth
