"""The package's autograd.Functions: the forward and backward passes are the engine's, on ROCm float32
tensors and torch's current stream; no double backward.  The public functions import this module on first use under grad --
it is the only one that needs torch at import time -- after every check and refusal of theirs has passed."""
from __future__ import annotations

import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import _capi as capi
from ._frontend import bound_engine, staged


def _upstream(g):
    return g.detach().to(torch.float32).contiguous()


def replicate_pad(x, pad):
    """F.pad(x, (pad,) * 4, mode='replicate') -- the same values, bit for bit -- composed of slices, expand and cat: the backward
    of torch's own replicate pad adds the pad's gradients into the edge pixels with float atomics on the GPU, so two identical
    backward calls differ in the last bits; the backward of expand is an ordered sum"""
    B, C, H, W = x.shape
    x = torch.cat([x[:, :, :1].expand(B, C, pad, W), x, x[:, :, -1:].expand(B, C, pad, W)], dim=2)
    return torch.cat([x[..., :1].expand(B, C, H + 2 * pad, pad), x, x[..., -1:].expand(B, C, H + 2 * pad, pad)], dim=3)


def _kernel_grad(gk, kernel_like, B, correlate):
    """the engine's (B', kh, kw) tap gradient back to kernel.shape: the taps were broadcast over the batch (summed here; the engine
    has summed over the planes of a one-channel kernel) and rotated for correlate=True (rotated back)"""
    (kb, kc, kh, kw), kdtype, kdevice = kernel_like
    gk = gk.view(B, kc, kh, kw)
    if kb == 1 and B > 1:
        gk = gk.sum(0, keepdim=True)
    if correlate:
        gk = gk.flip(-2, -1)
    return gk.to(device=kdevice, dtype=kdtype)


class TapsFunction(torch.autograd.Function):
    """convolve2d (poly is None) or compute_polynomial (poly = (alpha, b)) of a ROCm float32 image that is the whole
    domain.  taps, eshape: the (B', kh, kw) host array and the engine's view of the image's shape that nonblind._check_kernel made of
    `kernel` (already rotated when `correlate`);
    kernel: the tensor itself, for the graph, or None when it is an array; call: the forward's engine call, the caller's own
    (staged's form)."""

    @staticmethod
    def forward(ctx, img, kernel, taps, eshape, bnd, poly, correlate, call):
        x = img.detach()
        (out,), _ = staged(x, np.float32, call, taps=taps)
        ctx.save_for_backward(x)
        ctx.pb = (taps, bnd, poly, bool(correlate), int(img.shape[0]), eshape)
        # (of the kernel only what the backward needs to shape its gradient: the tensor itself is not kept alive)
        ctx.kernel_like = None if kernel is None else (tuple(int(v) for v in kernel.shape), kernel.dtype, kernel.device)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        taps, bnd, poly, correlate, B, eshape = ctx.pb
        want_x, want_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        xin = x.contiguous()
        g = _upstream(grad_out)
        gx = torch.empty_like(xin) if want_x else None
        gk = torch.empty(taps.shape, dtype=torch.float32, device=x.device) if want_k else None
        with bound_engine(x) as eng:
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
            gk = _kernel_grad(gk, ctx.kernel_like, B, correlate)
        return gx, gk, None, None, None, None, None, None


def _param_grad(rows, p):
    """the engine's per-image rows of a parameter's gradient -- a (B',) float32 device tensor -- summed in index order in float64,
    in the shape, dtype and device of the parameter tensor ``p``"""
    return rows.to(torch.float64).cumsum(0)[-1].to(device=p.device, dtype=p.dtype).reshape(p.shape)


class TapsParamsFunction(torch.autograd.Function):
    """compute_polynomial with alpha and / or b as one-element tensors that require grad: TapsFunction with the two
    parameter tensors (either may be None) behind the kernel.  The forward is TapsFunction's, with poly = the parameters' float values;
    the backward runs pb_compute_polynomial_taps_backward only where the image or the kernel asks, and
    pb_compute_polynomial_taps_params_backward only where a parameter does."""

    @staticmethod
    def forward(ctx, img, kernel, alpha_t, beta_t, taps, eshape, bnd, poly, correlate, call):
        x = img.detach()
        (out,), _ = staged(x, np.float32, call, taps=taps)
        ctx.save_for_backward(x, *(t for t in (alpha_t, beta_t) if t is not None))
        ctx.pb = (taps, bnd, poly, bool(correlate), int(img.shape[0]), eshape, alpha_t is not None, beta_t is not None)
        ctx.kernel_like = None if kernel is None else (tuple(int(v) for v in kernel.shape), kernel.dtype, kernel.device)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, params = ctx.saved_tensors[0], list(ctx.saved_tensors[1:])
        taps, bnd, poly, correlate, B, eshape, has_a, has_b = ctx.pb
        alpha_t = params.pop(0) if has_a else None
        beta_t = params.pop(0) if has_b else None
        want_x, want_k, want_a, want_b = ctx.needs_input_grad[:4]
        xin = x.contiguous()
        g = _upstream(grad_out)
        gx = torch.empty_like(xin) if want_x else None
        gk = torch.empty(taps.shape, dtype=torch.float32, device=x.device) if want_k else None
        gp = torch.empty((int(eshape[0]), 2), dtype=torch.float32, device=x.device) if want_a or want_b else None
        with bound_engine(x) as eng:
            ks = eng.set_taps(taps)
            try:
                if want_x or want_k:
                    eng.compute_polynomial_taps_backward_ptr(xin.data_ptr(), g.data_ptr(), gx.data_ptr() if want_x else None,
                                                             gk.data_ptr() if want_k else None, eshape, ks, poly[0], poly[1], bnd)
                if gp is not None:
                    eng.compute_polynomial_taps_params_backward_ptr(xin.data_ptr(), g.data_ptr(), gp.data_ptr(), eshape, ks, poly[0], poly[1], bnd)
            finally:
                ks.free()                               # (waits for the stream)
        if want_k:
            gk = _kernel_grad(gk, ctx.kernel_like, B, correlate)
        ga = _param_grad(gp[:, 0], alpha_t) if want_a else None
        gb = _param_grad(gp[:, 1], beta_t) if want_b else None
        return gx, gk, ga, gb, None, None, None, None, None, None


class EdgetaperFunction(torch.autograd.Function):
    """edgetaper of a ROCm float32 image that is the whole domain: ``n_tapers`` blends, differentiated with respect to
    the image and to the kernel -- through the taper weights too; odd kernel sides.  The arguments are TapsFunction's, with the
    blend count in poly's place; the forward is the one call of pb_edgetaper_taps, so its bits are those under torch.no_grad()."""

    @staticmethod
    def forward(ctx, img, kernel, taps, eshape, bnd, n_tapers, correlate, call):
        x = img.detach()
        (out,), _ = staged(x, np.float32, call, taps=taps)
        ctx.save_for_backward(x)
        ctx.pb = (taps, bnd, int(n_tapers), bool(correlate), int(img.shape[0]), eshape)
        ctx.kernel_like = None if kernel is None else (tuple(int(v) for v in kernel.shape), kernel.dtype, kernel.device)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        taps, bnd, n_tapers, correlate, B, eshape = ctx.pb
        want_x, want_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        xin = x.contiguous()
        g = _upstream(grad_out)
        gx = torch.empty_like(xin) if want_x else None
        gk = torch.empty(taps.shape, dtype=torch.float32, device=x.device) if want_k else None
        with bound_engine(x) as eng:
            ks = eng.set_taps(taps)
            try:
                eng.edgetaper_taps_backward_ptr(xin.data_ptr(), g.data_ptr(), gx.data_ptr() if want_x else None,
                                                gk.data_ptr() if want_k else None, eshape, ks, bnd, n_tapers)
            finally:
                ks.free()                               # (waits for the stream)
        if want_k:
            gk = _kernel_grad(gk, ctx.kernel_like, B, correlate)
        return gx, gk, None, None, None, None, None, None


class PhaseFunction(torch.autograd.Function):
    """compute_polynomial(method='fft', not_symmetric=True) of a ROCm float32 image that is the whole domain; kernel
    sides even or odd.  The arguments are TapsFunction's, with poly = (alpha, b)."""

    @staticmethod
    def forward(ctx, img, kernel, taps, eshape, poly, correlate, call):
        x = img.detach()
        (out,), _ = staged(x, np.float32, call, taps=taps)
        ctx.save_for_backward(x)
        ctx.pb = (taps, poly, bool(correlate), int(img.shape[0]), eshape)
        ctx.kernel_like = None if kernel is None else (tuple(int(v) for v in kernel.shape), kernel.dtype, kernel.device)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        taps, poly, correlate, B, eshape = ctx.pb
        want_x, want_k = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        xin = x.contiguous()
        g = _upstream(grad_out)
        gx = torch.empty_like(xin) if want_x else None
        gk = torch.empty(taps.shape, dtype=torch.float32, device=x.device) if want_k else None
        with bound_engine(x) as eng:
            ks = eng.set_taps(taps)
            try:
                eng.compute_polynomial_phase_taps_backward_ptr(xin.data_ptr(), g.data_ptr(), gx.data_ptr() if want_x else None,
                                                               gk.data_ptr() if want_k else None, eshape, ks, poly[0], poly[1])
            finally:
                ks.free()                               # (waits for the stream)
        if want_k:
            gk = _kernel_grad(gk, ctx.kernel_like, B, correlate)
        return gx, gk, None, None, None, None, None


class EstimationFunction(torch.autograd.Function):
    """gaussian_blur_estimation of a ROCm float32 image with q = 0; the records stay on the device for the backward.
    records: image -> its records; unpack: records -> the function's outputs (estimation._records, _kernel_of / _params_of)."""

    @staticmethod
    def forward(ctx, img, opts, ker_size, filters, records, unpack):
        x = img.detach().contiguous()
        rec = records(x)
        ctx.save_for_backward(x, rec)
        ctx.pb = (opts, int(ker_size), bool(filters))
        out = unpack(rec)
        if not filters:
            ctx.mark_non_differentiable(out[2])               # (theta comes from integer tensors: blur_estimation.py:160-167)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        x, rec = ctx.saved_tensors
        opts, ker_size, filters = ctx.pb
        gk = gsr = None
        if filters:
            gk = _upstream(grads[0])
        else:
            gsr = torch.cat([grads[0].detach().to(torch.float32).reshape(-1, 1), grads[1].detach().to(torch.float32).reshape(-1, 1)], dim=1).contiguous()
        gin = torch.empty_like(x)
        with bound_engine(x) as eng:
            eng.estimate_blur_backward_ptr(x.data_ptr(), x.shape, opts, rec.data_ptr(), gk.data_ptr() if filters else None,
                                           None if filters else gsr.data_ptr(), ker_size if filters else capi.PB_KSIZE, gin.data_ptr())
        return gin, None, None, None, None, None


class EstimationParamsFunction(torch.autograd.Function):
    """gaussian_blur_estimation with c and / or b of the affine model as one-element tensors that require grad:
    EstimationFunction with the two parameter tensors (either may be None) behind the image.  The backward is one call of
    pb_estimate_blur_params_backward: the image's gradient only where the image asks (no scatter otherwise), the (B,2) rows of
    d loss / d (c, b) only where a parameter does."""

    @staticmethod
    def forward(ctx, img, c_t, b_t, opts, ker_size, filters, records, unpack):
        x = img.detach().contiguous()
        rec = records(x)
        ctx.save_for_backward(x, rec, *(t for t in (c_t, b_t) if t is not None))
        ctx.pb = (opts, int(ker_size), bool(filters), c_t is not None, b_t is not None)
        out = unpack(rec)
        if not filters:
            ctx.mark_non_differentiable(out[2])               # (theta comes from integer tensors: blur_estimation.py:160-167)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        x, rec = ctx.saved_tensors[:2]
        params = list(ctx.saved_tensors[2:])
        opts, ker_size, filters, has_c, has_b = ctx.pb
        c_t = params.pop(0) if has_c else None
        b_t = params.pop(0) if has_b else None
        want_x, want_c, want_b = ctx.needs_input_grad[:3]
        gk = gsr = None
        if filters:
            gk = _upstream(grads[0])
        else:
            gsr = torch.cat([grads[0].detach().to(torch.float32).reshape(-1, 1), grads[1].detach().to(torch.float32).reshape(-1, 1)], dim=1).contiguous()
        gin = torch.empty_like(x) if want_x else None
        gcb = torch.empty((int(x.shape[0]), 2), dtype=torch.float32, device=x.device) if want_c or want_b else None
        with bound_engine(x) as eng:
            eng.estimate_blur_params_backward_ptr(x.data_ptr(), x.shape, opts, rec.data_ptr(), gk.data_ptr() if filters else None,
                                                  None if filters else gsr.data_ptr(), ker_size if filters else capi.PB_KSIZE,
                                                  None if gin is None else gin.data_ptr(), None if gcb is None else gcb.data_ptr())
        gc = _param_grad(gcb[:, 0], c_t) if want_c else None
        gb = _param_grad(gcb[:, 1], b_t) if want_b else None
        return gin, gc, gb, None, None, None, None, None


class FourierGradientsFunction(torch.autograd.Function):
    """fourier_gradients of a ROCm float32 tensor: linear, nothing is saved.  gradients: image -> (gx, gy) (halo._gradients)"""

    @staticmethod
    def forward(ctx, img, gradients):
        gx, gy = gradients(img.detach())
        ctx.set_materialize_grads(False)                  # (an output the loss does not reach: None, and no transform for it)
        return gx, gy

    @staticmethod
    @once_differentiable
    def backward(ctx, ggx, ggy):
        if ggx is None and ggy is None:
            return None, None
        ggx, ggy = (None if g is None else _upstream(g) for g in (ggx, ggy))
        like = ggx if ggx is not None else ggy
        gin = torch.empty_like(like)
        with bound_engine(like) as eng:
            eng.fourier_gradients_backward_ptr(None if ggx is None else ggx.data_ptr(), None if ggy is None else ggy.data_ptr(),
                                               like.shape, gin.data_ptr())
        return gin, None


class HaloMaskingFunction(torch.autograd.Function):
    """halo_masking of ROCm float32 tensors with given gradient planes.  mask: (img, imout, gx, gy) -> the masked image (halo._mask)"""

    @staticmethod
    def forward(ctx, img, imout, gx, gy, mask):
        x, y, a, b = (t.detach().contiguous() for t in (img, imout, gx, gy))
        out = mask(x, y, a, b)
        ctx.save_for_backward(x, y, a, b)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, y, a, b = ctx.saved_tensors
        g = _upstream(grad_out)
        outs = [torch.empty_like(x) if need else None for need in ctx.needs_input_grad[:4]]
        with bound_engine(x) as eng:
            eng.halo_mask_backward_ptr(x.data_ptr(), y.data_ptr(), a.data_ptr(), b.data_ptr(), g.data_ptr(),
                                       *[o.data_ptr() if o is not None else None for o in outs], x.shape)
        return tuple(outs) + (None,)


class RecursiveFilterFunction(torch.autograd.Function):
    """recursive_filter of ROCm float32 tensors, differentiated with respect to the image and to joint_image (None: guided by the
    image, whose gradient then holds both paths); the two sigma and the iteration count are Python numbers.
    filt: (image, joint or None, sigma_s, sigma_r, n) -> the filtered image (edge_aware._recursive)"""

    @staticmethod
    def forward(ctx, img, joint, sigma_s, sigma_r, num_iterations, filt):
        x = img.detach().contiguous()
        j = None if joint is None else joint.detach().contiguous()
        out = filt(x, j, sigma_s, sigma_r, num_iterations)
        ctx.save_for_backward(*((x,) if j is None else (x, j)))
        ctx.pb = (float(sigma_s), float(sigma_r), int(num_iterations))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        x, j = (ctx.saved_tensors + (None,))[:2]
        g = _upstream(grad_out)
        gx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        gj = torch.empty_like(j) if j is not None and ctx.needs_input_grad[1] else None
        with bound_engine(x) as eng:
            eng.dt_recursive_filter_backward_ptr(x.data_ptr(), None if j is None else j.data_ptr(), g.data_ptr(),
                                                 None if gx is None else gx.data_ptr(), None if gj is None else gj.data_ptr(),
                                                 x.shape, *ctx.pb)
        return gx, gj, None, None, None, None


class BilateralFunction(torch.autograd.Function):
    """bilateral_filter of a ROCm float32 tensor, differentiated with respect to the image (the two sigma are Python floats).
    filt: image -> the filtered image (edge_aware._bilateral)"""

    @staticmethod
    def forward(ctx, img, ksize, sigma_spatial, sigma_color, filt):
        x = img.detach().contiguous()
        out = filt(x, ksize, sigma_spatial, sigma_color)
        ctx.save_for_backward(x)
        ctx.pb = (int(ksize), float(sigma_spatial), float(sigma_color))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        g = _upstream(grad_out)
        gin = torch.empty_like(x)
        with bound_engine(x) as eng:
            eng.bilateral_backward_ptr(x.data_ptr(), g.data_ptr(), gin.data_ptr(), x.shape, *ctx.pb)
        return gin, None, None, None, None


class ExtractPatchesFunction(torch.autograd.Function):
    """image_to_patches of an even-sized ROCm float32 image: all n_i * n_j patches of the lattice ``grid``
    (patches.patch_grid) in one call of pb_extract_patches, [n*B + b]; the backward is pb_extract_patches_backward."""

    @staticmethod
    def forward(ctx, img, grid):
        x = img.detach().contiguous()
        B, Cc = x.shape[:2]
        n_p = grid["n_i"] * grid["n_j"]
        patches = torch.empty((n_p * B, Cc, grid["ph"], grid["pw"]), dtype=x.dtype, device=x.device)
        with bound_engine(x) as eng:
            eng.extract_patches_ptr(x.data_ptr(), patches.data_ptr(), capi.PB_F32, x.shape, grid, 0, n_p)
        ctx.pb = (tuple(int(v) for v in x.shape), dict(grid))
        return patches

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_patches):
        shape, grid = ctx.pb
        g = _upstream(grad_patches)
        gin = torch.empty(shape, dtype=torch.float32, device=g.device)
        with bound_engine(g) as eng:
            eng.extract_patches_backward_ptr(g.data_ptr(), gin.data_ptr(), shape, grid)
        return gin, None


class OverlapAddFunction(torch.autograd.Function):
    """patches_to_image of ROCm float32 patches: the one call of pb_overlap_add into an image of ``shape``, with the
    window tensors wy, wx (patches.windows); the backward is pb_overlap_add_backward, which forms the clamp mask from the patches
    again with the forward's own cover sum."""

    @staticmethod
    def forward(ctx, patches, shape, grid, wy, wx):
        p = patches.detach().contiguous()
        out = torch.empty(shape, dtype=p.dtype, device=p.device)
        with bound_engine(p) as eng:
            eng.overlap_add_ptr(p.data_ptr(), out.data_ptr(), capi.PB_F32, shape, grid, wy.data_ptr(), wx.data_ptr())
        ctx.save_for_backward(p, wy, wx)
        ctx.pb = (shape, dict(grid))
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_out):
        p, wy, wx = ctx.saved_tensors
        shape, grid = ctx.pb
        g = _upstream(grad_out)
        gp = torch.empty_like(p)
        with bound_engine(p) as eng:
            eng.overlap_add_backward_ptr(p.data_ptr(), g.data_ptr(), gp.data_ptr(), shape, grid, wy.data_ptr(), wx.data_ptr())
        return gp, None, None, None, None
