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
that requires grad -- with respect to the image and to the taps (not to alpha and b; no double backward).  The backward passes
are the engine's too (pb_convolve2d_taps_backward, pb_compute_polynomial_taps_backward); the pad, crop and clamp of
``inverse_filtering_rank3`` are then torch's own ops -- the replicate pad composed of slices, expand and cat, whose backward is
an ordered sum where F.pad's adds with float atomics.  ``remove_halo=True`` under grad is ``halo_masking`` (halo.py; DESIGN.md
4.9) between the crop and the clamp, differentiable with respect to ``grad_img`` too.  Under grad: float32 ROCm tensors and odd
kernel sides only, and no ``do_edgetaper``, ``edgetaper()``, ``not_symmetric`` or ``inverse_filtering_nonsymmetric``
(NotImplementedError before any device work).  Without grad nothing changes: the calls below run as before.

The arithmetic is the HIP engine's (include/polyblur_hip.h: pb_taps_create and the *_taps calls); nothing runs on the CPU.
"""
from __future__ import annotations

import numpy as np

from . import _capi as capi
from .deblurring import _check_image_size, _is_torch_tensor
from .engine import get_engine

_BOUNDARY = {"fft": capi.PB_WRAP, "direct": capi.PB_ZERO}


def _host_array(a):
    return a.detach().cpu().numpy() if _is_torch_tensor(a) else np.asarray(a)


def _check_image(img, allow_half):
    """-> (is_tensor, shape, numpy dtype) of a (B,C,H,W) image."""
    if _is_torch_tensor(img):
        import torch
        if img.dim() != 4:
            raise ValueError("expected a (B,C,H,W) tensor, got shape %r" % (tuple(img.shape),))
        if img.dtype == torch.float32:
            dt = np.dtype(np.float32)
        elif img.dtype == torch.float16 and allow_half:
            dt = np.dtype(np.float16)
        else:
            raise TypeError("tensor dtype must be float32%s" % (" or float16" if allow_half else ""))
        shape = tuple(int(v) for v in img.shape)
        tensor = True
    elif isinstance(img, np.ndarray):
        if img.ndim != 4:
            raise ValueError("expected a (B,C,H,W) array, got shape %r" % (img.shape,))
        dt = np.dtype(np.float16) if (img.dtype == np.float16 and allow_half) else np.dtype(np.float32)
        shape = tuple(int(v) for v in img.shape)
        tensor = False
    else:
        raise TypeError("img must be a numpy.ndarray or a torch.Tensor")
    if shape[0] < 1 or shape[1] < 1 or shape[2] < 2 or shape[3] < 2:
        raise ValueError("bad image shape %r" % (shape,))
    return tensor, shape, dt


def _check_kernel(kernel, method, img_shape, pad_domain, circular_only, correlate=False):
    """Every refusal, then the taps as (B', kh, kw) float32 with B' = B (one kernel per image) or B*C (one per plane; the
    image is then passed as B*C one-channel images) -> (taps, per_plane)."""
    if isinstance(kernel, (tuple, list)):
        raise NotImplementedError("tuple kernels (the separable 1-D form, filters.py:29-30) are not built: pass a (B,C,h,w) kernel")
    if method == "direct_separable":
        raise NotImplementedError("method='direct_separable' takes tuple kernels, which are not built here")
    if method not in _BOUNDARY:
        raise ValueError("%s not implemented" % method)
    if not (_is_torch_tensor(kernel) or isinstance(kernel, np.ndarray)):
        raise TypeError("kernel must be a numpy.ndarray or a torch.Tensor")
    if len(kernel.shape) != 4:
        raise ValueError("expected a (B,C,h,w) kernel, got shape %r" % (tuple(kernel.shape),))
    B, C, H, W = img_shape
    kb, kc, kh, kw = (int(v) for v in kernel.shape)
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
    k = np.asarray(_host_array(kernel), np.float32)
    if correlate:
        k = k[..., ::-1, ::-1]                              # torch.rot90(kernel, 2, (-2, -1)), deblurring.py:225-226
    per_plane = kc > 1
    k = np.broadcast_to(k, (B, kc, kh, kw))
    return np.ascontiguousarray(k).reshape(B * kc, kh, kw), per_plane


def _run(img, tensor, dt, shape, taps, per_plane, call, extra=()):
    """call(engine, kernel set, in_ptr, out_ptr, shape, extra_ptrs) on the right stream; `extra`: further (B,C,H,W) float32
    operands (tensors or arrays) the call reads."""
    B, C, H, W = shape
    eshape = (B * C, 1, H, W) if per_plane else shape
    if tensor and img.is_cuda:
        import torch
        dev = img.device.index if img.device.index is not None else torch.cuda.current_device()
        eng = get_engine(dev)
        xin = img.contiguous()
        out = torch.empty_like(xin)
        ex = [torch.as_tensor(e, dtype=torch.float32, device=img.device).contiguous() for e in extra]
        with torch.cuda.device(dev):
            eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
            ks = eng.set_taps(taps)
            try:
                call(eng, ks, xin.data_ptr(), out.data_ptr(), eshape, [e.data_ptr() for e in ex])
            finally:
                ks.free()                                   # (waits for the stream: the set is in use until then)
        return out
    eng = get_engine(0)
    eng.set_stream(0)
    x = np.ascontiguousarray(_host_array(img), dtype=dt)
    din = eng.to_device("np.in", x)
    dout = eng.buffer("np.out", x.nbytes)
    ex = [eng.to_device("np.g0%s" % "xy"[i], np.ascontiguousarray(_host_array(e), np.float32)).ptr for i, e in enumerate(extra)]
    ks = eng.set_taps(taps)
    try:
        call(eng, ks, din.ptr, dout.ptr, eshape, ex)
        eng.synchronize()
    finally:
        ks.free()
    out = dout.download(x.shape, x.dtype)
    if tensor:
        import torch
        return torch.from_numpy(out)
    return out


def _wants_grad(img, kernel):
    """autograd is on and the image or the kernel is a tensor that requires grad"""
    ts = [t for t in (img, kernel) if _is_torch_tensor(t)]
    if not ts:
        return False
    import torch
    return torch.is_grad_enabled() and any(t.requires_grad for t in ts)


def _refuse_under_grad(what, reason):
    raise NotImplementedError("%s has no backward pass: %s" % (what, reason))


def _check_grad(img, kernel, what):
    """what the backward passes are built for -- raised before any device work"""
    if _is_torch_tensor(img):
        import torch
        if img.dtype == torch.float16:
            _refuse_under_grad(what + " of a float16 image", "gradients are built for float32 images")
    kh, kw = (int(v) for v in kernel.shape[-2:])
    if kh % 2 == 0 or kw % 2 == 0:
        _refuse_under_grad(what + " with a %d x %d kernel" % (kh, kw), "the adjoint of an even kernel side sits one sample off centre -- odd sides only")
    for name, t in (("img", img), ("kernel", kernel)):
        if _is_torch_tensor(t) and t.requires_grad and not t.is_cuda:
            _refuse_under_grad(what, "%s requires grad and is a CPU tensor -- gradients are built for ROCm tensors only" % name)
    if not (_is_torch_tensor(img) and img.is_cuda):
        _refuse_under_grad(what, "img is a CPU tensor or a NumPy array -- gradients are built for ROCm tensors only")


def _replicate_pad(x, pad):
    """F.pad(x, (pad,) * 4, mode='replicate') -- the same values, bit for bit -- composed of slices, expand and cat: the backward
    of torch's own replicate pad adds the pad's gradients into the edge pixels with float atomics on the GPU, so two identical
    backward calls differ in the last bits; the backward of expand is an ordered sum"""
    import torch
    B, C, H, W = x.shape
    x = torch.cat([x[:, :, :1].expand(B, C, pad, W), x, x[:, :, -1:].expand(B, C, pad, W)], dim=2)
    return torch.cat([x[..., :1].expand(B, C, H + 2 * pad, pad), x, x[..., -1:].expand(B, C, H + 2 * pad, pad)], dim=3)


_TAPS_FUNCTION = None


def _taps_function():
    """the autograd.Function of both differentiable passes (made on first use: torch is imported lazily in this module)"""
    global _TAPS_FUNCTION
    if _TAPS_FUNCTION is not None:
        return _TAPS_FUNCTION
    import torch
    from torch.autograd.function import once_differentiable

    class TapsFunction(torch.autograd.Function):
        """convolve2d (poly is None) or compute_polynomial (poly = (alpha, b)) of a ROCm float32 image that is the whole
        domain.  taps: the (B', kh, kw) host array _check_kernel made of `kernel` (already rotated when `correlate`)."""

        @staticmethod
        def forward(ctx, img, kernel, taps, per_plane, bnd, poly, correlate):
            shape = tuple(int(v) for v in img.shape)
            if poly is None:
                call = lambda eng, ks, i, o, s, ex: eng.convolve2d_taps_ptr(i, o, s, ks, bnd)
            else:
                call = lambda eng, ks, i, o, s, ex: eng.compute_polynomial_taps_ptr(i, o, s, ks, poly[0], poly[1], bnd, False)
            x = img.detach()
            out = _run(x, True, np.dtype(np.float32), shape, taps, per_plane, call)
            ctx.save_for_backward(x)
            ctx.pb = (taps, per_plane, bnd, poly, bool(correlate), shape)
            ctx.kernel_like = kernel                        # (None: the kernel is an array)
            return out

        @staticmethod
        @once_differentiable
        def backward(ctx, grad_out):
            (x,) = ctx.saved_tensors
            taps, per_plane, bnd, poly, correlate, shape = ctx.pb
            want_x, want_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            B, C, H, W = shape
            eshape = (B * C, 1, H, W) if per_plane else shape
            dev = x.device.index if x.device.index is not None else torch.cuda.current_device()
            eng = get_engine(dev)
            xin = x.contiguous()
            g = grad_out.detach().to(torch.float32).contiguous()
            gx = torch.empty_like(xin) if want_x else None
            gk = torch.empty(taps.shape, dtype=torch.float32, device=x.device) if want_k else None
            with torch.cuda.device(dev):
                eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
                ks = eng.set_taps(taps)
                try:
                    args = (xin.data_ptr(), g.data_ptr(), gx.data_ptr() if want_x else None, gk.data_ptr() if want_k else None, eshape, ks)
                    if poly is None:
                        eng.convolve2d_taps_backward_ptr(*args, bnd)
                    else:
                        eng.compute_polynomial_taps_backward_ptr(*args, poly[0], poly[1], bnd)
                finally:
                    ks.free()                               # (waits for the stream)
            if want_k:
                # back to kernel.shape: the taps were broadcast over the batch (summed here; the engine has summed over the
                # planes of a one-channel kernel) and rotated for correlate=True (rotated back)
                kernel = ctx.kernel_like
                kb, kc, kh, kw = (int(v) for v in kernel.shape)
                gk = gk.view(B, kc, kh, kw)
                if kb == 1 and B > 1:
                    gk = gk.sum(0, keepdim=True)
                if correlate:
                    gk = gk.flip(-2, -1)
                gk = gk.to(device=kernel.device, dtype=kernel.dtype)
            return gx, gk, None, None, None, None, None

    _TAPS_FUNCTION = TapsFunction
    return TapsFunction


def _apply_taps_function(img, kernel, taps, per_plane, bnd, poly, correlate=False):
    return _taps_function().apply(img, kernel if _is_torch_tensor(kernel) else None, taps, per_plane, bnd, poly, correlate)


def convolve2d(img, kernel, method='direct'):
    """filters.convolve2d (filters.py:14-37) with a 2-D kernel: ``img`` is the whole domain."""
    tensor, shape, dt = _check_image(img, allow_half=False)
    taps, per_plane = _check_kernel(kernel, method, shape, pad_domain=False, circular_only=True)
    bnd = _BOUNDARY[method]
    if _wants_grad(img, kernel):
        _check_grad(img, kernel, "convolve2d")
        return _apply_taps_function(img, kernel, taps, per_plane, bnd, None)
    return _run(img, tensor, dt, shape, taps, per_plane,
                lambda eng, ks, i, o, s, ex: eng.convolve2d_taps_ptr(i, o, s, ks, bnd))


def edgetaper(img, kernel, n_tapers=3, method='fft'):
    """edgetaper.edgetaper (edgetaper.py:26-33): ``n_tapers`` blends of ``img`` with its blurred self, weighted by the
    autocorrelations of the kernel's projections."""
    tensor, shape, dt = _check_image(img, allow_half=False)
    if not isinstance(n_tapers, (int, np.integer)) or n_tapers < 0:
        raise ValueError("n_tapers must be an integer >= 0")
    taps, per_plane = _check_kernel(kernel, method, shape, pad_domain=False, circular_only=True)
    if _wants_grad(img, kernel):
        _refuse_under_grad("edgetaper", "the blends are not differentiated (call it under torch.no_grad() or on detached tensors)")
    bnd = _BOUNDARY[method]
    return _run(img, tensor, dt, shape, taps, per_plane,
                lambda eng, ks, i, o, s, ex: eng.edgetaper_taps_ptr(i, o, s, ks, bnd, int(n_tapers)))


def inverse_filtering_rank3(img, kernel, alpha=2, b=4, correlate=False, remove_halo=False, do_edgetaper=False,
                            grad_img=None, method='direct'):
    """deblurring.inverse_filtering_rank3 (deblurring.py:211-239): replicate pad by w // 2 -> [edgetaper] -> polynomial ->
    crop -> [halo masking] -> clamp.  ``grad_img``: (grad_x, grad_y) of the original image, or None for the gradients of
    the (tapered) image itself."""
    tensor, shape, dt = _check_image(img, allow_half=True)
    taps, per_plane = _check_kernel(kernel, method, shape, pad_domain=True, circular_only=bool(do_edgetaper),
                                    correlate=bool(correlate))
    halo_planes = tuple(grad_img) if remove_halo and isinstance(grad_img, (tuple, list)) and len(grad_img) == 2 else ()
    if _wants_grad(img, kernel) or (halo_planes and _wants_grad(*halo_planes)):
        if remove_halo:
            # (the stage's device check first: its reason names the stage)
            import torch
            for t in (img,) + halo_planes:                    # (the kernel's own checks follow: _check_grad)
                if not _is_torch_tensor(t) or not t.is_cuda or t.dtype != torch.float32:
                    _refuse_under_grad("inverse_filtering_rank3(remove_halo=True)", "halo masking is differentiated for float32 ROCm tensors only")
        if do_edgetaper:
            _refuse_under_grad("inverse_filtering_rank3(do_edgetaper=True)", "the edgetaper is not differentiated")
        _check_grad(img, kernel, "inverse_filtering_rank3")
        # pad, crop and clamp are torch's own ops with torch's own backward; the polynomial and the mask are the engine's
        import torch
        if remove_halo:
            from .halo import _check_grad_img
            _check_image_size(*shape[-2:])
            if grad_img is not None:
                _check_grad_img(grad_img, shape)
        pad = taps.shape[-1] // 2
        xp = _replicate_pad(img, pad)
        y = _apply_taps_function(xp, kernel, taps, per_plane, _BOUNDARY[method], (alpha, b), bool(correlate))
        y = y[..., pad:-pad, pad:-pad]
        if remove_halo:
            from .halo import halo_masking
            y = halo_masking(img, y, grad_img)                # (grad_img None: fourier_gradients(img), inside the graph)
        return torch.clamp(y, 0.0, 1.0)
    extra = ()
    if remove_halo:
        _check_image_size(*shape[-2:])
        if grad_img is not None:
            if not isinstance(grad_img, (tuple, list)) or len(grad_img) != 2:
                raise ValueError("grad_img must be (grad_x, grad_y)")
            for gpart in grad_img:
                if tuple(int(v) for v in gpart.shape) != shape:
                    raise ValueError("grad_img planes must have the image's shape %r" % (shape,))
            extra = tuple(grad_img)
    bnd = _BOUNDARY[method]
    dtype = capi.PB_F16 if dt == np.float16 else capi.PB_F32

    def call(eng, ks, i, o, s, ex):
        eng.inverse_filter_taps_ptr(i, o, dtype, s, ks, alpha, b, bnd, bool(do_edgetaper), bool(remove_halo),
                                    ex[0] if ex else None, ex[1] if ex else None)

    return _run(img, tensor, dt, shape, taps, per_plane, call, extra)


def _check_phase_sides(hp, wp):
    """the pure-phase filter transforms whole lines of the domain in LDS (pb_fft_length_supported == 1; needs no GPU)"""
    lib = capi.load_library()
    for n in (hp, wp):
        if lib.pb_fft_length_supported(int(n)) != 1:
            raise NotImplementedError("the pure-phase filter transforms the whole %d x %d domain: a side of %d samples is not held "
                                      "in LDS (up to 20480 with prime factors <= 7, up to 8192 otherwise)" % (hp, wp, n))


def compute_polynomial(img, kernel, alpha, b, method='fft', not_symmetric=False):
    """deblurring.compute_polynomial (deblurring.py:113-169): a3 K^3 x + a2 K^2 x + a1 K x + b x on ``img``, which is the whole
    domain (float32; treated as convolve2d treats it); unclamped.  ``not_symmetric=True`` ('fft' only): the pure-phase filter
    conj(K) / (|K| + 1e-8) first -- for a kernel that is not point-symmetric.  Under 'direct' the reference takes the flag and
    ignores it; here that is a ValueError.  Where |K| falls to fp32 roundoff the filter's phase is noise (see the module)."""
    tensor, shape, dt = _check_image(img, allow_half=False)
    taps, per_plane = _check_kernel(kernel, method, shape, pad_domain=False, circular_only=False)
    if not_symmetric and method != "fft":
        raise ValueError("not_symmetric=True is the pure-phase filter of method='fft' (the reference's direct form ignores the flag)")
    if _wants_grad(img, kernel):
        if not_symmetric:
            _refuse_under_grad("compute_polynomial(not_symmetric=True)", "the pure-phase filter is not differentiated")
        _check_grad(img, kernel, "compute_polynomial")
        return _apply_taps_function(img, kernel, taps, per_plane, _BOUNDARY[method], (alpha, b))
    if not_symmetric:
        _check_phase_sides(shape[2], shape[3])
    bnd = _BOUNDARY[method]
    return _run(img, tensor, dt, shape, taps, per_plane,
                lambda eng, ks, i, o, s, ex: eng.compute_polynomial_taps_ptr(i, o, s, ks, alpha, b, bnd, bool(not_symmetric)))


def inverse_filtering_nonsymmetric(img, kernel, alpha=2, b=4, correlate=False, remove_halo=False, do_edgetaper=False,
                                   grad_img=None):
    """inverse_filtering_rank3's chain (deblurring.py:211-239) with compute_polynomial(method='fft', not_symmetric=True) in the
    polynomial's place: replicate pad by w // 2 -> [edgetaper, 'fft'] -> phase-corrected polynomial -> crop -> [halo masking]
    -> clamp.  float32 or float16 images.  Where |K| falls to fp32 roundoff the filter's phase is noise (see the module)."""
    tensor, shape, dt = _check_image(img, allow_half=True)
    taps, per_plane = _check_kernel(kernel, "fft", shape, pad_domain=True, circular_only=bool(do_edgetaper),
                                    correlate=bool(correlate))
    if _wants_grad(img, kernel):
        _refuse_under_grad("inverse_filtering_nonsymmetric", "the pure-phase filter is not differentiated")
    pad = taps.shape[-1] // 2
    _check_phase_sides(shape[2] + 2 * pad, shape[3] + 2 * pad)
    extra = ()
    if remove_halo:
        _check_image_size(*shape[-2:])
        if grad_img is not None:
            if not isinstance(grad_img, (tuple, list)) or len(grad_img) != 2:
                raise ValueError("grad_img must be (grad_x, grad_y)")
            for gpart in grad_img:
                if tuple(int(v) for v in gpart.shape) != shape:
                    raise ValueError("grad_img planes must have the image's shape %r" % (shape,))
            extra = tuple(grad_img)
    dtype = capi.PB_F16 if dt == np.float16 else capi.PB_F32

    def call(eng, ks, i, o, s, ex):
        eng.inverse_filter_phase_taps_ptr(i, o, dtype, s, ks, alpha, b, bool(do_edgetaper), bool(remove_halo),
                                          ex[0] if ex else None, ex[1] if ex else None)

    return _run(img, tensor, dt, shape, taps, per_plane, call, extra)
