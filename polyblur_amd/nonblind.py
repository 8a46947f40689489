"""The reference's non-blind functions with a kernel of the caller's (deblurring.py:211-239, filters.py:14-37,
edgetaper.py:26-33):

    from polyblur_amd import inverse_filtering_rank3, convolve2d, edgetaper

Same names, arguments and defaults.  ``img`` is a (B,C,H,W) ``torch.Tensor`` -- on a ROCm device (used in place, on torch's
current stream) or on the CPU (staged through the GPU) -- or an ``np.ndarray`` of that shape; float32, or float16 for the
inverse filter.  The result has the type and device of ``img``.  ``kernel`` is a (B,1,h,w) tensor or array -- one kernel per
image --, (B,C,h,w) -- one per plane --, or either with a batch of 1, which broadcasts; 1 <= h <= 49, 2 <= w <= 49, even, odd,
square or rectangular, taps used as given.

``method`` is the boundary model, as in the blind driver: 'direct' = F.conv2d(padding='same'), zero outside the padded
domain; 'fft' = circular convolution over it with the PSF rolled by -(h//2), -(w//2).  Under 'direct' the reference itself
fails for per-plane kernels and for B > 1 (filters.py:45-49); here every plane gets its own correlation.

Refused before any device work: a kernel one tap wide (the reference's crop [0:-0] is empty) and one that does not fit the
domain (ValueError); sides above 49, tuple kernels / method='direct_separable', and -- in convolve2d, edgetaper and
do_edgetaper=True under 'fft' -- a kernel taller than wide, for which the reference's circular pad by the half-width is no
circular convolution over the domain (NotImplementedError).

``compute_polynomial`` and ``inverse_filtering_nonsymmetric`` bring the reference's cure for kernels that are not
point-symmetric (deblurring.py:141-169, ``not_symmetric=True``): the image spectrum times the pure-phase filter
conj(K) / (|K| + 1e-8) before the polynomial.  That is one transform over the whole (padded) domain; both of its sides must
be line lengths the engine holds in LDS (up to 20480 samples when every prime factor is <= 7, up to 8192 otherwise):
NotImplementedError before any device work otherwise.  Where |K| falls to fp32 roundoff (about 1e-7 -- a wide Gaussian has
such bins near Nyquist) the phase of that filter is noise, in the reference as much as here: a property of the method.

Gradients (the reference's README: "fully differentiable"): ``convolve2d``, ``compute_polynomial`` and
``inverse_filtering_rank3`` return a tensor with a ``grad_fn`` when autograd is enabled and ``img`` or ``kernel`` is a tensor
that requires grad -- with respect to the image and to the taps, and to ``alpha`` and ``b`` where they are tensors (below; no
double backward).  The backward passes
are the engine's too (pb_convolve2d_taps_backward, pb_compute_polynomial_taps_backward); the pad, crop and clamp of
``inverse_filtering_rank3`` are then torch's own ops -- the replicate pad composed of slices, expand and cat, whose backward is
an ordered sum where F.pad's adds with float atomics.  ``remove_halo=True`` under grad is ``halo_masking`` (halo.py; DESIGN.md
4.9) between the crop and the clamp, differentiable with respect to ``grad_img`` too.  ``edgetaper()`` and ``do_edgetaper=True`` are
differentiable as well: the backward of the blends is the engine's pb_edgetaper_taps_backward, with respect to the
image and to the kernel -- through the taper weights too, which are autocorrelations of the kernel's projections; under grad
``inverse_filtering_rank3(do_edgetaper=True)`` is replicate pad -> three blends -> polynomial -> crop -> [halo masking of the
tapered, cropped image] -> clamp.  Under grad: float32 ROCm tensors and odd kernel sides only (NotImplementedError before any
device work).  Without grad nothing changes: the calls below run as before.

``compute_polynomial(..., not_symmetric=True)`` and ``inverse_filtering_nonsymmetric`` are differentiable in the same way (DESIGN.md
4.14): the backward of the pure-phase polynomial is the engine's pb_compute_polynomial_phase_taps_backward -- the image gradient
is the forward's transform with the conjugate multiplier, the tap gradient a gather from one more transform, through the phase
factor conj(K) / |K| as well --, and ``inverse_filtering_nonsymmetric`` is composed as ``inverse_filtering_rank3`` is.  Kernel
sides even or odd: nothing in that adjoint is centred.  Under grad: float32 ROCm tensors, no ``do_edgetaper`` (the edgetaper's
backward takes odd sides and is not wired in front of the pure-phase filter), padded sides the engine holds in LDS.  With no ROCm tensor among the operands the refusal is the one it has always been ("the pure-phase filter is
not differentiated").

Learnable parameters: ``alpha`` and ``b`` of ``compute_polynomial`` and ``inverse_filtering_rank3`` are Python
numbers or one-element tensors (0-dim or of shape (1,), float32 or float64, on the CPU or on the image's device; more elements:
ValueError).  A tensor's value is read once per call with ``float(t)`` -- the launch plan sizes window halos from the coefficients
on the host, so a parameter that lives on a device costs one synchronisation -- and the forward is the forward with that float,
bit for bit.  Where autograd is on and a parameter requires grad the result has a ``grad_fn`` -- a parameter alone is enough, and
then no image or kernel gradient is computed -- and its ``.grad`` is the engine's (pb_compute_polynomial_taps_params_backward:
d/d alpha = 1/2 <G, K (1 - K)^2 x>, d/d b = <G, (1 - K)^3 x> from the detail images, per image), summed over the images in index
order in float64, in the parameter's shape, dtype and device.  Refused before any device work: such a parameter beside an image
that is not a float32 ROCm tensor, and on the pure-phase path (``not_symmetric=True``, ``inverse_filtering_nonsymmetric``), where
these gradients are not built.

The arithmetic is the HIP engine's (include/polyblur_hip.h: pb_taps_create and the *_taps calls); nothing runs on the CPU.
"""
from __future__ import annotations

import numpy as np

from . import _capi as capi
from ._frontend import (CPU_WITH_GRAD, DTYPES, FLOAT32_ONLY, HALO_ONLY, NO_EDGETAPER, NO_PHASE_PARAMS, check_grad_img, check_image,
                        check_image_size, check_param, check_phase_sides, host_array, is_rocm_float32, is_tensor, param_value,
                        refuse_params, refuse_under_grad, staged, wants_grad)
from .halo import halo_masking

_BOUNDARY = {"fft": capi.PB_WRAP, "direct": capi.PB_ZERO}
_NO_PHASE = "the pure-phase filter is not differentiated"


def _check_kernel(kernel, method, img_shape, pad_domain, circular_only, correlate=False):
    """Every refusal, then the taps as (B', kh, kw) float32 with B' = B (one kernel per image) or B*C (one per plane; the
    image is then passed as B*C one-channel images) -> (taps, the image's shape as the engine takes it)."""
    if isinstance(kernel, (tuple, list)):
        raise NotImplementedError("tuple kernels (the separable 1-D form, filters.py:29-30) are not built: pass a (B,C,h,w) kernel")
    if method == "direct_separable":
        raise NotImplementedError("method='direct_separable' takes tuple kernels, which are not built here")
    if method not in _BOUNDARY:
        raise ValueError("%s not implemented" % method)
    if not (is_tensor(kernel) or isinstance(kernel, np.ndarray)):
        raise TypeError("kernel must be a numpy.ndarray or a torch.Tensor")
    if len(kernel.shape) != 4:
        raise ValueError("expected a (B,C,h,w) kernel, got shape %r" % (tuple(kernel.shape),))
    B, C, H, W = img_shape
    kb, kc, kh, kw = kernel.shape
    if kb not in (1, B) or kc not in (1, C):
        raise ValueError("kernel shape %r does not match the image's (%d,%d,...): batch 1 or %d, channels 1 or %d"
                         % (tuple(kernel.shape), B, C, B, C))
    if kh < 1 or kw < 1:
        raise ValueError("empty kernel")
    if kw == 1:
        raise ValueError("a kernel one tap wide pads by 0 samples and the reference's crop [0:-0] is then empty")
    if kh > capi.PB_KSIZE_MAX or kw > capi.PB_KSIZE_MAX:
        raise NotImplementedError("a %d x %d kernel: sides up to %d are built" % (kh, kw, capi.PB_KSIZE_MAX))
    pad = kw // 2 if pad_domain else 0
    if kh > H + 2 * pad - 1 or kw > W + 2 * pad - 1:
        raise ValueError("a %d x %d kernel does not fit the %d x %d domain (at most rows - 1, columns - 1)"
                         % (kh, kw, H + 2 * pad, W + 2 * pad))
    if circular_only and method == "fft" and kh // 2 > kw // 2:
        raise NotImplementedError("a kernel taller than wide under method='fft': the reference pads circularly by the "
                                  "half-width only, which is no circular convolution over the domain -- not built")
    k = np.asarray(host_array(kernel), np.float32)
    if correlate:
        k = k[..., ::-1, ::-1]                              # torch.rot90(kernel, 2, (-2, -1)), deblurring.py:225-226
    k = np.broadcast_to(k, (B, kc, kh, kw))
    return np.ascontiguousarray(k).reshape(B * kc, kh, kw), ((B * C, 1, H, W) if kc > 1 else img_shape)


def _run(img, dt, taps, call, extra=()):
    """call(engine, in_ptr, [out_ptr], extra pointers, kernel set) on operands of any kind (staged); `extra`: the halo mask's two
    gradient planes of the original image, or none"""
    return staged(img, dt, call, (("np.g0x", extra[0]), ("np.g0y", extra[1])) if extra else (), taps=taps)[0][0]


def _check_grad(img, kernel, what, even_ok=False):
    """what the backward passes are built for -- raised before any device work.  even_ok: the pure-phase filter's adjoint is a
    gather at p2o's positions, nothing in it is centred"""
    if is_tensor(img):
        import torch
        if img.dtype == torch.float16:
            refuse_under_grad(what + " of a float16 image", FLOAT32_ONLY)
    kh, kw = (int(v) for v in kernel.shape[-2:])
    if not even_ok and (kh % 2 == 0 or kw % 2 == 0):
        refuse_under_grad(what + " with a %d x %d kernel" % (kh, kw), "the adjoint of an even kernel side sits one sample off centre -- odd sides only")
    for name, t in (("img", img), ("kernel", kernel)):
        if is_tensor(t) and t.requires_grad and not t.is_cuda:
            refuse_under_grad(what, CPU_WITH_GRAD % name)
    if not (is_tensor(img) and img.is_cuda):
        refuse_under_grad(what, "img is a CPU tensor or a NumPy array -- gradients are built for ROCm tensors only")


def _apply_taps_function(img, kernel, taps, eshape, bnd, poly, call, correlate=False, params=(None, None)):
    """params: the tensors of (alpha, b) that ask for a gradient (check_param), None for the others"""
    if params[0] is not None or params[1] is not None:
        from ._autograd import TapsParamsFunction
        return TapsParamsFunction.apply(img, kernel if is_tensor(kernel) else None, params[0], params[1], taps, eshape, bnd, poly, correlate, call)
    from ._autograd import TapsFunction
    return TapsFunction.apply(img, kernel if is_tensor(kernel) else None, taps, eshape, bnd, poly, correlate, call)


def _any_rocm(*operands):
    return any(is_tensor(t) and t.is_cuda for t in operands)


def _apply_phase_function(img, kernel, taps, eshape, alpha, b, correlate=False):
    """compute_polynomial(method='fft', not_symmetric=True) of ``img``, the whole domain, inside the graph"""
    from ._autograd import PhaseFunction
    call = lambda eng, i, o, ex, ks: eng.compute_polynomial_taps_ptr(i, o[0], eshape, ks, alpha, b, capi.PB_WRAP, True)
    return PhaseFunction.apply(img, kernel if is_tensor(kernel) else None, taps, eshape, (alpha, b), correlate, call)


def _taper_operands(img, kernel):
    """what the edgetaper's backward is built for: a float32 ROCm image, and no CPU kernel that requires grad (anything else under
    grad keeps the refusal it has always had)"""
    return is_rocm_float32(img) and not (is_tensor(kernel) and kernel.requires_grad and not kernel.is_cuda)


def _apply_edgetaper_function(img, kernel, taps, eshape, bnd, n_tapers, correlate=False):
    """edgetaper of ``img``, the whole domain, inside the graph"""
    from ._autograd import EdgetaperFunction
    call = lambda eng, i, o, ex, ks: eng.edgetaper_taps_ptr(i, o[0], eshape, ks, bnd, n_tapers)
    return EdgetaperFunction.apply(img, kernel if is_tensor(kernel) else None, taps, eshape, bnd, n_tapers, correlate, call)


def convolve2d(img, kernel, method='direct'):
    """filters.convolve2d (filters.py:14-37) with a 2-D kernel: ``img`` is the whole domain."""
    shape, dt = check_image(img, allow_half=False)
    taps, eshape = _check_kernel(kernel, method, shape, pad_domain=False, circular_only=True)
    bnd = _BOUNDARY[method]
    call = lambda eng, i, o, ex, ks: eng.convolve2d_taps_ptr(i, o[0], eshape, ks, bnd)
    if wants_grad(img, kernel):
        _check_grad(img, kernel, "convolve2d")
        return _apply_taps_function(img, kernel, taps, eshape, bnd, None, call)
    return _run(img, dt, taps, call)


def edgetaper(img, kernel, n_tapers=3, method='fft'):
    """edgetaper.edgetaper (edgetaper.py:26-33): ``n_tapers`` blends of ``img`` with its blurred self, weighted by the
    autocorrelations of the kernel's projections.  Differentiable with respect to ``img`` and ``kernel`` (float32 ROCm tensors,
    odd kernel sides)."""
    shape, dt = check_image(img, allow_half=False)
    if not isinstance(n_tapers, (int, np.integer)) or n_tapers < 0:
        raise ValueError("n_tapers must be an integer >= 0")
    taps, eshape = _check_kernel(kernel, method, shape, pad_domain=False, circular_only=True)
    bnd = _BOUNDARY[method]
    if wants_grad(img, kernel):
        if not _taper_operands(img, kernel):
            refuse_under_grad("edgetaper", "the blends are not differentiated (call it under torch.no_grad() or on detached tensors)")
        _check_grad(img, kernel, "edgetaper")
        return _apply_edgetaper_function(img, kernel, taps, eshape, bnd, int(n_tapers))
    return _run(img, dt, taps, lambda eng, i, o, ex, ks: eng.edgetaper_taps_ptr(i, o[0], eshape, ks, bnd, int(n_tapers)))


_OWN = (None, None)         # no gradient planes of the original image: the mask takes those of the (tapered) image itself


def _chain(img, dt, shape, taps, remove_halo, grad_img, call):
    """the no-grad tail of both chains: the halo mask's checks, then the call with the gradient planes of the original image as
    its extra pointers (none: _OWN)"""
    extra = ()
    if remove_halo:
        check_image_size(*shape[-2:])
        if grad_img is not None:
            check_grad_img(grad_img, shape)
            extra = tuple(grad_img)
    return _run(img, dt, taps, call, extra)


def inverse_filtering_rank3(img, kernel, alpha=2, b=4, correlate=False, remove_halo=False, do_edgetaper=False,
                            grad_img=None, method='direct'):
    """deblurring.inverse_filtering_rank3 (deblurring.py:211-239): replicate pad by w // 2 -> [edgetaper] -> polynomial ->
    crop -> [halo masking] -> clamp.  ``grad_img``: (grad_x, grad_y) of the original image, or None for the gradients of
    the (tapered) image itself."""
    shape, dt = check_image(img, allow_half=True)
    params = (check_param(alpha, "alpha", img), check_param(b, "b", img))
    refuse_params("inverse_filtering_rank3", img, alpha=params[0], b=params[1])
    taps, eshape = _check_kernel(kernel, method, shape, pad_domain=True, circular_only=bool(do_edgetaper),
                                    correlate=bool(correlate))
    halo_planes = tuple(grad_img) if remove_halo and isinstance(grad_img, (tuple, list)) and len(grad_img) == 2 else ()
    bnd = _BOUNDARY[method]
    if wants_grad(img, kernel, *halo_planes, *params):
        # (the stage's device check first: its reason names the stage; the kernel's own checks follow: _check_grad)
        if remove_halo and not all(is_rocm_float32(t) for t in (img,) + halo_planes):
            refuse_under_grad("inverse_filtering_rank3(remove_halo=True)", HALO_ONLY)
        if do_edgetaper and not _taper_operands(img, kernel):
            refuse_under_grad("inverse_filtering_rank3(do_edgetaper=True)", NO_EDGETAPER)
        _check_grad(img, kernel, "inverse_filtering_rank3")
        # pad, crop and clamp are torch's own ops with torch's own backward; the polynomial and the mask are the engine's
        if remove_halo:
            check_image_size(*shape[-2:])
            if grad_img is not None:
                check_grad_img(grad_img, shape)
        from ._autograd import replicate_pad
        alpha, b = param_value(alpha), param_value(b)         # (every refusal has passed: a device parameter is read now)
        pad = taps.shape[-1] // 2
        xp = replicate_pad(img, pad)                          # (the polynomial's domain: the engine's shape with the padded sides)
        pshape = eshape[:2] + tuple(xp.shape[-2:])
        if do_edgetaper:                                      # (three blends of the padded plane: deblurring.py:229-230)
            xp = _apply_edgetaper_function(xp, kernel, taps, pshape, bnd, 3, bool(correlate))
            if remove_halo:
                img = xp[..., pad:-pad, pad:-pad]             # (the mask's image is the tapered one: deblurring.py:236-238)
        y = _apply_taps_function(xp, kernel, taps, pshape, bnd, (alpha, b),
                                 lambda eng, i, o, ex, ks: eng.compute_polynomial_taps_ptr(i, o[0], pshape, ks, alpha, b, bnd, False), bool(correlate),
                                 params)
        y = y[..., pad:-pad, pad:-pad]
        if remove_halo:
            y = halo_masking(img, y, grad_img)                # (grad_img None: fourier_gradients(img), inside the graph)
        return y.clamp(0.0, 1.0)
    dtype = DTYPES[dt]
    alpha, b = param_value(alpha), param_value(b)
    return _chain(img, dt, shape, taps, remove_halo, grad_img,
                  lambda eng, i, o, ex, ks: eng.inverse_filter_taps_ptr(i, o[0], dtype, eshape, ks, alpha, b, bnd, bool(do_edgetaper),
                                                                        bool(remove_halo), *(ex or _OWN)))


def compute_polynomial(img, kernel, alpha, b, method='fft', not_symmetric=False):
    """deblurring.compute_polynomial (deblurring.py:113-169): a3 K^3 x + a2 K^2 x + a1 K x + b x on ``img``, which is the whole
    domain (float32; treated as convolve2d treats it); unclamped.  ``not_symmetric=True`` ('fft' only): the pure-phase filter
    conj(K) / (|K| + 1e-8) first -- for a kernel that is not point-symmetric.  Under 'direct' the reference takes the flag and
    ignores it; here that is a ValueError.  Where |K| falls to fp32 roundoff the filter's phase is noise (see the module).
    Differentiable with respect to ``img`` and ``kernel``, with the flag too (float32 ROCm tensors)."""
    shape, dt = check_image(img, allow_half=False)
    params = (check_param(alpha, "alpha", img), check_param(b, "b", img))
    if not_symmetric and (params[0] is not None or params[1] is not None):
        refuse_under_grad("compute_polynomial(not_symmetric=True)", NO_PHASE_PARAMS)
    refuse_params("compute_polynomial", img, alpha=params[0], b=params[1])
    taps, eshape = _check_kernel(kernel, method, shape, pad_domain=False, circular_only=False)
    if not_symmetric and method != "fft":
        raise ValueError("not_symmetric=True is the pure-phase filter of method='fft' (the reference's direct form ignores the flag)")
    bnd = _BOUNDARY[method]
    # (alpha and b are read by the call when it runs: by then they are the numbers param_value gives, after every refusal)
    call = lambda eng, i, o, ex, ks: eng.compute_polynomial_taps_ptr(i, o[0], eshape, ks, alpha, b, bnd, bool(not_symmetric))
    if wants_grad(img, kernel, *params):
        if not_symmetric:
            if not _any_rocm(img, kernel):
                refuse_under_grad("compute_polynomial(not_symmetric=True)", _NO_PHASE)
            _check_grad(img, kernel, "compute_polynomial(not_symmetric=True)", even_ok=True)
            check_phase_sides(shape[2], shape[3])
            alpha, b = param_value(alpha), param_value(b)
            return _apply_phase_function(img, kernel, taps, eshape, alpha, b)
        _check_grad(img, kernel, "compute_polynomial")
        alpha, b = param_value(alpha), param_value(b)
        return _apply_taps_function(img, kernel, taps, eshape, bnd, (alpha, b), call, params=params)
    if not_symmetric:
        check_phase_sides(shape[2], shape[3])
    alpha, b = param_value(alpha), param_value(b)
    return _run(img, dt, taps, call)


def inverse_filtering_nonsymmetric(img, kernel, alpha=2, b=4, correlate=False, remove_halo=False, do_edgetaper=False,
                                   grad_img=None):
    """inverse_filtering_rank3's chain (deblurring.py:211-239) with compute_polynomial(method='fft', not_symmetric=True) in the
    polynomial's place: replicate pad by w // 2 -> [edgetaper, 'fft'] -> phase-corrected polynomial -> crop -> [halo masking]
    -> clamp.  float32 or float16 images.  Where |K| falls to fp32 roundoff the filter's phase is noise (see the module).
    Differentiable with respect to ``img``, ``kernel`` and ``grad_img`` (float32 ROCm tensors, no ``do_edgetaper``)."""
    shape, dt = check_image(img, allow_half=True)
    if check_param(alpha, "alpha", img) is not None or check_param(b, "b", img) is not None:
        refuse_under_grad("inverse_filtering_nonsymmetric", NO_PHASE_PARAMS)
    taps, eshape = _check_kernel(kernel, "fft", shape, pad_domain=True, circular_only=bool(do_edgetaper),
                                    correlate=bool(correlate))
    halo_planes = tuple(grad_img) if remove_halo and isinstance(grad_img, (tuple, list)) and len(grad_img) == 2 else ()
    pad = taps.shape[-1] // 2
    if not _any_rocm(img, kernel, *halo_planes):
        if wants_grad(img, kernel):
            refuse_under_grad("inverse_filtering_nonsymmetric", _NO_PHASE)
    elif wants_grad(img, kernel, *halo_planes):
        # inverse_filtering_rank3's composition with the phase-corrected polynomial in the polynomial's place
        if remove_halo and not all(is_rocm_float32(t) for t in (img,) + halo_planes):
            refuse_under_grad("inverse_filtering_nonsymmetric(remove_halo=True)", HALO_ONLY)
        if do_edgetaper:
            refuse_under_grad("inverse_filtering_nonsymmetric(do_edgetaper=True)", NO_EDGETAPER)
        _check_grad(img, kernel, "inverse_filtering_nonsymmetric", even_ok=True)
        check_phase_sides(shape[2] + 2 * pad, shape[3] + 2 * pad)
        if remove_halo:
            check_image_size(*shape[-2:])
            if grad_img is not None:
                check_grad_img(grad_img, shape)
        from ._autograd import replicate_pad
        alpha, b = param_value(alpha), param_value(b)
        xp = replicate_pad(img, pad)
        y = _apply_phase_function(xp, kernel, taps, eshape[:2] + tuple(xp.shape[-2:]), alpha, b, bool(correlate))
        y = y[..., pad:-pad, pad:-pad]
        if remove_halo:
            y = halo_masking(img, y, grad_img)                # (grad_img None: fourier_gradients(img), inside the graph)
        return y.clamp(0.0, 1.0)
    check_phase_sides(shape[2] + 2 * pad, shape[3] + 2 * pad)
    dtype = DTYPES[dt]
    alpha, b = param_value(alpha), param_value(b)
    return _chain(img, dt, shape, taps, remove_halo, grad_img,
                  lambda eng, i, o, ex, ks: eng.inverse_filter_phase_taps_ptr(i, o[0], dtype, eshape, ks, alpha, b, bool(do_edgetaper),
                                                                              bool(remove_halo), *(ex or _OWN)))
