"""Drop-in for the reference's public API (polyblur/deblurring.py:23-25 and :250-347).

    from polyblur_amd import polyblur_deblurring, PolyblurDeblurring

Same names, keyword arguments, defaults (including the functional/module defaults that
differ in the reference), and the same in/out type rule:

* ``np.ndarray`` (H,W) or (H,W,C)  ->  ``np.ndarray`` of the same shape, float32
  (deblurring.py:46-48,93-94);
* ``torch.Tensor`` (B,C,H,W)       ->  ``torch.Tensor`` on the same device, same dtype.
  ROCm tensors are used in place (zero copy, on torch's current stream); CPU tensors
  are staged through the GPU.

The work is done by the HIP engine behind include/polyblur_hip.h; there is no CPU
implementation here.  ``method`` keeps the reference's meaning as a *boundary model*:
'fft' = circular reblurring on the replicate-padded domain (the reference default),
'direct' = zero-padded reblurring -- both evaluated by the same reblurring pass (separable or 2-D
stencil, or -- dense kernels -- overlap-save on 64x64 windows inside LDS; no image-sized transform
exists on the device).

Extras that the reference does not have (all keyword-only, defaults keep reference
behaviour): ``support`` ('full' | 'adaptive'), ``prefilter`` ('bilateral' |
'domain_transform' -- which edge-aware filter ``prefiltering=True`` uses; the reference's
live code path is the bilateral one, deblurring.py:107-108), ``return_info``, ``temporaries``
('fp32' | 'fp16': float16 tensors only -- store the two Horner temporaries as fp16).

A float32 ROCm tensor that requires grad takes the differentiable composition (``_blind_under_grad``): estimation, non-blind
step, ``remove_halo=True``, ``edgetaping=True`` and ``prefiltering=True`` with the bilateral prefilter have the engine's own
backward passes; the other two prefilters and ``q > 0`` are refused before any device work.  ``PolyblurDeblurring(patch_decomposition=
True)`` of such a tensor -- or of a float32 ROCm image beside a learnable parameter -- cuts every patch once, runs this composition
on groups of ``batch_size`` patches and blends them (patches.py, DESIGN.md 4.17: the extraction and the overlap-add have the engine's
own backward passes); any other image under grad is refused there.

Learnable parameters: ``c``, ``b``, ``alpha`` and ``beta`` are Python numbers or one-element tensors (0-dim or of
shape (1,), float32 or float64, on the CPU or on the image's device).  One that requires grad, with autograd on, takes the same
composition -- beside a float32 ROCm image, which need not require grad itself -- and its ``.grad`` accumulates over the ``n_iter``
iterations through autograd (estimation.py, nonblind.py: a tensor's value is read with ``float(t)`` in every stage call, one
synchronisation each where it lives on a device).  Any other tensor parameter is read once and the call runs as with the number.
"""
from __future__ import annotations

from time import time

import numpy as np

from . import _capi as capi
from ._frontend import (_PREFILTER, CPU_WITH_GRAD, DTYPES, FLOAT32_ONLY, HALO_ONLY, NO_EDGETAPER, NO_QUANTILE, bound_engine,
                        build_options, check_image_size, check_param, is_rocm_float32, is_tensor, param_value, refuse_params, refuse_under_grad, staged,
                        wants_grad)
from .edge_aware import edge_aware_filtering
from .estimation import gaussian_blur_estimation
from .halo import fourier_gradients
from .nonblind import inverse_filtering_rank3
from .patches import blend, check_lattice, even_part, extract, kaiser_window_periodic, patch_grid  # noqa: F401  (the lattice lives there)


def _info_to_dicts(info, n_angles, n_interp):
    if info is None:
        return None
    out = []
    for it in range(info.shape[0]):
        rec = info[it]
        out.append(dict(mags=rec["mags"][:, :n_angles + 1].copy(), interp=rec["interp"][:, :n_interp].copy(),
                        i_min=rec["i_min"].copy(), theta=rec["theta"].copy(), sigma=rec["sigma"].copy(),
                        rho=rec["rho"].copy(), kernel=rec["kernel"].copy(), separable=rec["separable"].copy(),
                        radius=rec["radius"].copy(), nphase=rec["nphase"].copy(), lo=rec["gray_min"].copy(),
                        hi=rec["gray_max"].copy()))
    return out


def _print_stage_times(prof, wall):
    """verbose=True: device time per stage from hipEvents around every launch (the reference prints host
    wall-clock per stage without synchronising, deblurring.py:59-90)."""
    ms = {k: v[0] for k, v in prof.items()}
    est = ms["gray"] + ms["grad_rows"] + ms["grad_cols"] + ms["params"]
    print('-- blur estimation:   %1.5f  (gray/min-max %1.5f, row derivative %1.5f, column derivative + maxima %1.5f, '
          'parameters %1.5f)' % (est / 1e3, ms["gray"] / 1e3, ms["grad_rows"] / 1e3, ms["grad_cols"] / 1e3, ms["params"] / 1e3))
    deb = ms["conv"] + ms["halo"] + ms["prefilter"] + ms["other"]
    print('-- deblurring:        %1.5f  (%d stencil passes %1.5f, halo masking %1.5f, prefilter %1.5f, other %1.5f)'
          % (deb / 1e3, prof["conv"][1], ms["conv"] / 1e3, ms["halo"] / 1e3, ms["prefilter"] / 1e3, ms["other"] / 1e3))
    print('-- polyblur (hip):    %1.5f s wall' % wall)


def _run(x, dt, opts, return_info, device, verbose=False):
    """the blind call on a (B,C,H,W) image of any kind (staged), of NumPy dtype dt -> (output, records or None, stage times or None)"""
    def call(eng, i, o, ex):
        if not verbose:
            return eng.polyblur_ptr(i, o[0], DTYPES[np.dtype(dt)], x.shape, opts, want_info=return_info), None
        eng.profile_begin()
        try:
            info = eng.polyblur_ptr(i, o[0], DTYPES[np.dtype(dt)], x.shape, opts, want_info=return_info)
        finally:                                            # (a failed call must not leave the thread's context profiling)
            prof = eng.profile_end()
        return info, prof
    (out,), (info, prof) = staged(x, dt, call, device=device)
    return out, info, prof


def polyblur_deblurring(img, n_iter=1, c=0.352, b=0.768, alpha=2, beta=3, sigma_r=0.8, sigma_s=2.0, ker_size=25, q=0.0,
                        n_angles=6, n_interpolated_angles=30, remove_halo=False, edgetaping=False, prefiltering=False,
                        discard_saturation=False, multichannel_kernel=False, method='fft', verbose=False, *,
                        support='full', prefilter='bilateral', return_info=False, device=None, temporaries='fp32'):
    """Blind deblurring of ``img`` -- see the module docstring; reference deblurring.py:23-96."""
    start = time()
    array = isinstance(img, np.ndarray)
    # (learnable parameters, DESIGN.md 4.16: the tensors of c, b, alpha, beta that ask for a gradient -- none: the floats go on)
    params = dict(c=check_param(c, "c", img), b=check_param(b, "b", img), alpha=check_param(alpha, "alpha", img),
                  beta=check_param(beta, "beta", img))
    refuse_params("polyblur_deblurring", img, **params)
    if all(t is None for t in params.values()):
        params = None
    if array:
        # utils.to_tensor + unsqueeze (deblurring.py:46-48): HWC -> (1,C,H,W) float32 copy
        if img.ndim == 2:
            x = img[None, None]
        elif img.ndim == 3:
            x = np.moveaxis(img, 2, 0)[None]
        else:
            raise ValueError("expected an (H,W) or (H,W,C) array, got shape %r" % (img.shape,))
        x = np.ascontiguousarray(x, dtype=np.float32)
        dt, temporaries = np.float32, "fp32"                  # (`temporaries` is about float16 tensors: arrays never read it)
    else:
        if not is_tensor(img):
            raise TypeError("img must be a numpy.ndarray or a torch.Tensor")
        import torch
        if img.dim() != 4:
            raise ValueError("expected a (B,C,H,W) tensor, got shape %r" % (tuple(img.shape),))
        if img.dtype not in (torch.float32, torch.float16):
            raise TypeError("tensor dtype must be float32 or float16 (the reference is float32-only)")
        if wants_grad(img) or params:
            return _blind_under_grad(img, n_iter, c, b, alpha, beta, ker_size, q, n_angles, n_interpolated_angles, remove_halo, edgetaping,
                                     prefiltering, discard_saturation, multichannel_kernel, method, support, return_info, temporaries,
                                     prefilter, sigma_s, sigma_r)
        x, dt = img, (np.float32 if img.dtype == torch.float32 else np.float16)
    check_image_size(*x.shape[-2:])
    if temporaries == "fp16" and dt != np.float16:
        raise ValueError("temporaries='fp16' applies to float16 images only")
    c, b, alpha, beta = param_value(c), param_value(b), param_value(alpha), param_value(beta)     # (tensors that ask for nothing: numbers)
    opts = build_options(x.shape[1], n_iter, c, b, alpha, beta, sigma_r, sigma_s, ker_size, q, n_angles,
                         n_interpolated_angles, remove_halo, edgetaping, prefiltering, discard_saturation,
                         multichannel_kernel, method, support, prefilter, temporaries=temporaries)
    out, info, prof = _run(x, dt, opts, return_info, device, verbose)
    if verbose:
        _print_stage_times(prof, time() - start)
    if array:
        # utils.to_array (utils.py:24-31): squeeze, CHW -> HWC
        out = np.squeeze(out)
        if out.ndim == 3:
            out = np.ascontiguousarray(np.moveaxis(out, 0, -1))
    return (out, _info_to_dicts(info, n_angles, n_interpolated_angles)) if return_info else out


def _refusals_under_grad(img, n_iter, ker_size, q, remove_halo, edgetaping, prefiltering, method, support, return_info, temporaries,
                         prefilter):
    """what polyblur_deblurring refuses of a tensor ``img`` under grad, before any device work (the patch branch asks for the whole
    image, before it extracts a patch)"""
    import torch
    what = "polyblur_deblurring"
    if remove_halo and not (img.is_cuda and img.dtype == torch.float32):     # (the stage's device check first: its reason names the stage)
        refuse_under_grad(what + "(remove_halo=True)", HALO_ONLY)
    if edgetaping and not (img.is_cuda and img.dtype == torch.float32):      # (the edgetaper's backward is the engine's: 4.15)
        refuse_under_grad(what + "(edgetaping=True)", NO_EDGETAPER)
    if prefiltering:
        rocm_float32 = img.is_cuda and img.dtype == torch.float32
        if rocm_float32 and prefilter not in _PREFILTER:
            raise ValueError("prefilter must be 'bilateral', 'domain_transform' or 'normalized_convolution'")     # (build_options')
        if not (rocm_float32 and prefilter == "bilateral"):                  # (the bilateral filter's backward alone is built: 4.12)
            refuse_under_grad(what + "(prefiltering=True)", "the edge-aware prefilters are not differentiated")
    if q > 0:
        refuse_under_grad("%s(q=%g)" % (what, q), NO_QUANTILE)
    if method == "direct_separable":
        refuse_under_grad(what + "(method='direct_separable')", "the x-t separable approximation is not differentiated")
    if method not in ("fft", "direct"):
        raise ValueError("%s not implemented" % method)
    if not (isinstance(ker_size, (int, np.integer)) and 3 <= ker_size <= capi.PB_KSIZE and ker_size % 2 == 1):
        refuse_under_grad("%s(ker_size=%r)" % (what, ker_size), "gradients are built for odd kernel sizes from 3 to 25")
    if support != "full":
        refuse_under_grad("%s(support=%r)" % (what, support), "gradients are built for support='full'")
    if temporaries != "fp32":
        refuse_under_grad("%s(temporaries=%r)" % (what, temporaries), "gradients are built for float32 images and temporaries")
    if return_info:
        refuse_under_grad(what + "(return_info=True)", "the records are not part of the graph -- call gaussian_blur_estimation for the kernels")
    if img.dtype == torch.float16:
        refuse_under_grad(what + " of a float16 image", FLOAT32_ONLY)
    if not img.is_cuda:
        refuse_under_grad(what, CPU_WITH_GRAD % "img")
    if not (isinstance(n_iter, (int, np.integer)) and n_iter >= 0):
        raise ValueError("n_iter must be an integer >= 0")


def _blind_under_grad(img, n_iter, c, b, alpha, beta, ker_size, q, n_angles, n_interpolated_angles, remove_halo, edgetaping,
                      prefiltering, discard_saturation, multichannel_kernel, method, support, return_info, temporaries, prefilter,
                      sigma_s, sigma_r):
    """polyblur_deblurring of a tensor that requires grad (the reference's README: "fully differentiable"): the blind call as a
    composition of the package's own differentiable functions -- estimate (estimation.py), with ``prefiltering``
    the bilateral split (edge_aware.py; 4.12: the step runs on the smooth part and the noise is added back, deblurring.py:80-84),
    non-blind step (nonblind.py; 4.7) with the halo mask where asked (halo.py; 4.9), clip, n_iter times (deblurring.py:54-90).
    Every refusal comes before any device work."""
    _refusals_under_grad(img, n_iter, ker_size, q, remove_halo, edgetaping, prefiltering, method, support, return_info, temporaries, prefilter)
    x = img
    # (the halo mask's gradient planes are those of the original input, for every iteration: deblurring.py:61,83)
    grad_img = fourier_gradients(img) if remove_halo and n_iter > 0 else None
    for _ in range(int(n_iter)):
        kernel = gaussian_blur_estimation(x, q=0, n_angles=n_angles, n_interpolated_angles=n_interpolated_angles, c=c, b=b,
                                          ker_size=ker_size, discard_saturation=discard_saturation, multichannel=multichannel_kernel)
        if prefiltering:                                                     # (deblurring.py:80-84; the mask's x is the smooth part)
            smooth, noise = edge_aware_filtering(x, sigma_s, sigma_r, prefilter=prefilter)
            x = (inverse_filtering_rank3(smooth, kernel, alpha, beta, remove_halo=bool(remove_halo), do_edgetaper=bool(edgetaping),
                                         grad_img=grad_img, method=method) + noise).clip(0, 1)
        else:
            x = inverse_filtering_rank3(x, kernel, alpha, beta, remove_halo=bool(remove_halo), do_edgetaper=bool(edgetaping),
                                        grad_img=grad_img, method=method).clip(0, 1)
    return x if n_iter > 0 else img.clone()


def polyblur_deblurring_uint8(img, n_iter=1, c=0.352, b=0.768, alpha=2, beta=3, sigma_r=0.8, sigma_s=2.0, ker_size=25,
                              q=0.0, n_angles=6, n_interpolated_angles=30, remove_halo=False, edgetaping=False,
                              prefiltering=False, discard_saturation=False, multichannel_kernel=False, method='fft',
                              verbose=False, *, support='full', prefilter='bilateral', return_info=False, device=None):
    """8-bit images in, 8-bit images out: the reference CLI's
    ``img_as_ubyte(polyblur_deblurring(img_as_float32(imread(...)), ...))`` (main.py:80-82,146) with both
    conversions done inside the first / last device kernels (scikit-image 0.19.2 semantics:
    ``v * float32(1/255)`` on load, ``clip(rint(v * 255), 0, 255)`` on store; fp32 in between).

    ``numpy.ndarray`` uint8 (H,W) / (H,W,C) -> same shape uint8;  ``torch.Tensor`` uint8 (B,C,H,W) -> same."""
    start = time()
    array = isinstance(img, np.ndarray)
    if array:
        if img.dtype != np.uint8:
            raise TypeError("expected a uint8 image, got %s" % img.dtype)
        if img.ndim == 2:
            x = img[None, :, :, None]
        elif img.ndim == 3:
            x = img[None]
        else:
            raise ValueError("expected an (H,W) or (H,W,C) array, got shape %r" % (img.shape,))
        C = x.shape[3]
    else:
        if not is_tensor(img):
            raise TypeError("img must be a numpy.ndarray or a torch.Tensor")
        import torch
        if img.dim() != 4 or img.dtype != torch.uint8:
            raise TypeError("expected a (B,C,H,W) uint8 tensor")
        C = img.shape[1]
    opts = build_options(C, n_iter, c, b, alpha, beta, sigma_r, sigma_s, ker_size, q, n_angles,
                         n_interpolated_angles, remove_halo, edgetaping, prefiltering, discard_saturation,
                         multichannel_kernel, method, support, prefilter)
    if array:                                               # (interleaved bytes: planarised and re-interleaved on the device)
        with bound_engine(None, device) as eng:
            res = eng.polyblur_u8_hwc(x, opts, want_info=return_info)
        out, info = res if return_info else (res, None)
        out = out.reshape(img.shape)
    else:
        out, info, _ = _run(img, np.uint8, opts, return_info, device)
    if verbose:
        print('-- polyblur (hip, uint8): %1.5f s' % (time() - start))
    return (out, _info_to_dicts(info, n_angles, n_interpolated_angles)) if return_info else out


def _device_index(device):
    """`device` of PolyblurDeblurring.forward (deblurring.py:322-330: where the patches are deblurred) -> GPU index."""
    if device is None:
        return None
    if isinstance(device, int):
        return device
    import torch
    d = torch.device(device)
    if d.type != "cuda":
        raise ValueError("device=%r: the engine runs on a GPU only (there is no CPU implementation)" % (device,))
    return d.index if d.index is not None else torch.cuda.current_device()


def _patchwise_deblurring(images, patch_size, overlap, batch_size, kwargs, device=None, under_grad=False):
    """PolyblurDeblurring.forward, patch branch (deblurring.py:269-340, fix-forward).  ``under_grad``: a float32 ROCm image with autograd
    on and the image or one of c, b, alpha, beta asking for a gradient."""
    import torch
    if not is_tensor(images) or images.dim() != 4:
        raise ValueError("patch decomposition expects a (B,C,H,W) tensor")
    if images.dtype not in (torch.float32, torch.float16):
        raise TypeError("tensor dtype must be float32 or float16")
    if kwargs.pop("return_info", False):
        raise TypeError("return_info is not available with patch_decomposition=True (one record set per patch group)")
    check_lattice(images.shape[-2], images.shape[-1], patch_size, overlap)        # (the lattice first)
    if under_grad:                                          # (what the blind call refuses under grad, before a patch is cut)
        _refusals_under_grad(images, kwargs.get("n_iter", 1), kwargs.get("ker_size", 25), kwargs.get("q", 0.0), kwargs.get("remove_halo", False),
                             kwargs.get("edgetaping", False), kwargs.get("prefiltering", False), kwargs.get("method", "fft"),
                             kwargs.get("support", "full"), False, kwargs.get("temporaries", "fp32"), kwargs.get("prefilter", "bilateral"))
    was_cuda = images.is_cuda
    want = _device_index(device)
    if was_cuda:
        dev = images.device.index if images.device.index is not None else torch.cuda.current_device()
        if want is not None and want != dev:
            raise ValueError("images live on cuda:%d but device=cuda:%d was requested" % (dev, want))
    else:
        dev = 0 if want is None else want                   # reference: patches.to(device) ... .cpu() (deblurring.py:322-330)
    x = even_part(images if was_cuda else images.to("cuda:%d" % dev))       # :273-279 make the size even
    h, w = x.shape[-2:]
    B, Cc = x.shape[:2]
    g = patch_grid(h, w, patch_size, overlap)
    if g["ph"] < 2 or g["pw"] < 2 or g["step_h"] < 1 or g["step_w"] < 1:
        raise ValueError("patch size / overlap incompatible: patches of at least 2x2 with a positive step are needed")
    n_p = g["n_i"] * g["n_j"]
    group = max(1, int(batch_size))
    if under_grad:
        # every patch once -- through ExtractPatchesFunction where the image asks for a gradient, the plain call where it is data --,
        # the blind call on groups of `batch_size` patches with the caller's c, b, alpha, beta as they are, one overlap-add through
        # OverlapAddFunction: patches are independent images, so the grouping changes no bit of the output or of the image's gradient
        # A learnable parameter goes to the groups as its float64 copy: a group's gradient is the float64 sum of its images' float32
        # rows (_autograd._param_grad), autograd adds the groups and the iterations in float64 -- sums of a few hundred float32
        # values, which float64 holds exactly -- and the one rounding to the parameter's dtype comes last: the grouping does not
        # reach the parameter's gradient either.
        for name in ("c", "b", "alpha", "beta"):
            if check_param(kwargs.get(name), name, images) is not None:
                kwargs[name] = kwargs[name].double()
        patches = extract(x, g)
        restored = [polyblur_deblurring(patches[first * B:min(first + group, n_p) * B], **kwargs) for first in range(0, n_p, group)]
        return blend(torch.cat(restored) if len(restored) > 1 else restored[0].contiguous(), x.shape, g)
    dtype = capi.PB_F32 if x.dtype == torch.float32 else capi.PB_F16
    wy = torch.from_numpy(kaiser_window_periodic(g["ph"])).to(x.device)
    wx = torch.from_numpy(kaiser_window_periodic(g["pw"])).to(x.device)
    restored = torch.empty((n_p * B, Cc, g["ph"], g["pw"]), dtype=x.dtype, device=x.device)
    with bound_engine(x) as eng:
        for first in range(0, n_p, group):                       # :310 groups of `batch_size` patches
            count = min(group, n_p - first)
            patches = torch.empty((count * B, Cc, g["ph"], g["pw"]), dtype=x.dtype, device=x.device)
            eng.extract_patches_ptr(x.data_ptr(), patches.data_ptr(), dtype, x.shape, g, first, count)
            restored[first * B:(first + count) * B] = polyblur_deblurring(patches, **kwargs)
        out = torch.empty_like(x)
        eng.overlap_add_ptr(restored.data_ptr(), out.data_ptr(), dtype, x.shape, g, wy.data_ptr(), wx.data_ptr())
        eng.synchronize()                                        # wy / wx / restored must outlive the kernels
    return out if was_cuda else out.cpu()


class _ModuleBase:
    pass


try:                                      # be an nn.Module when torch is importable, like the reference
    import torch.nn as _nn
    _Base = _nn.Module
except Exception:                         # pragma: no cover
    _Base = _ModuleBase


class PolyblurDeblurring(_Base):
    """Stateless module wrapper, reference deblurring.py:250-347.

    ``patch_decomposition=True`` raises ``NameError`` in the reference (undefined
    ``handling_saturation``, deblurring.py:289).  Here it is built "fix-forward" (SURVEY 8f row 1):
    the saturation branch is dropped and the restored patches of a batch are indexed per image;
    everything else -- even-size crop, replicate padding to the patch grid, periodic Kaiser(beta=5)
    window, overlap-add normalised by the summed window + 1e-8, clamp, crop -- follows :269-340.
    Note the defaults of ``forward`` differ from the functional API's (deblurring.py:266-268).
    """

    def __init__(self, patch_decomposition=False, patch_size=400, patch_overlap=0.25, batch_size=1):
        super().__init__()
        self.batch_size = batch_size
        self.patch_decomposition = patch_decomposition
        self.patch_size = (patch_size, patch_size)
        self.patch_overlap = patch_overlap

    def forward(self, images, n_iter=1, c=0.352, b=0.468, alpha=2, beta=4, sigma_s=2, ker_size=25, sigma_r=0.4,
                q=0.0, n_angles=6, n_interpolated_angles=30, remove_halo=False, edgetaping=False, prefiltering=False,
                discard_saturation=False, multichannel_kernel=False, method='fft', device=None, **extras):
        if self.patch_decomposition:
            under_grad = wants_grad(images) or any(check_param(t, n, images) is not None for n, t in (("c", c), ("b", b), ("alpha", alpha), ("beta", beta)))
            if under_grad and not is_rocm_float32(images):    # (float32 ROCm images take the differentiable branch: DESIGN.md 4.17)
                refuse_under_grad("PolyblurDeblurring(patch_decomposition=True)", "the patch extraction and the windowed overlap-add "
                                  "(pb_extract_patches, pb_overlap_add) are not differentiated")
            return _patchwise_deblurring(images, self.patch_size, self.patch_overlap, self.batch_size,
                                         dict(n_iter=n_iter, c=c, b=b, alpha=alpha, beta=beta, ker_size=ker_size,
                                              sigma_s=sigma_s, sigma_r=sigma_r, remove_halo=remove_halo,
                                              edgetaping=edgetaping, prefiltering=prefiltering,
                                              discard_saturation=discard_saturation,
                                              multichannel_kernel=multichannel_kernel, method=method, q=q,
                                              n_angles=n_angles, n_interpolated_angles=n_interpolated_angles, **extras),
                                         device=device, under_grad=under_grad)
        return polyblur_deblurring(images, n_iter=n_iter, c=c, b=b, alpha=alpha, beta=beta, ker_size=ker_size,
                                   sigma_s=sigma_s, sigma_r=sigma_r, remove_halo=remove_halo, edgetaping=edgetaping,
                                   prefiltering=prefiltering, discard_saturation=discard_saturation,
                                   multichannel_kernel=multichannel_kernel, method=method, q=q, n_angles=n_angles,
                                   n_interpolated_angles=n_interpolated_angles, device=_device_index(device), **extras)

    if _Base is _ModuleBase:              # pragma: no cover
        __call__ = forward
