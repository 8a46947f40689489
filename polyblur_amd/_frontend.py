"""What every public function of the package shares on the host: the checks and refusals that come before any
device work, the marshalling of the blind driver's options, the one place that binds the calling thread's engine to a device and
a stream, and the one staging of the three kinds of operand -- a ROCm tensor is used in place on torch's current stream, a CPU
tensor and an ``np.ndarray`` go through the GPU, and the result comes back in the kind of ``img``.

torch is not imported here at import time: the package imports without it, and NumPy callers never load it.  The public modules
(deblurring, nonblind, halo, estimation, edge_aware) import this one and the engine; nothing here imports them back.  The autograd.Functions
live in _autograd.py, which the public functions import on first use under grad.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from . import _capi as capi
from .engine import _DT as DTYPES, Engine, get_engine          # (DTYPES: NumPy dtype -> the C ABI's PB_F32 / PB_F16 / PB_U8)

# 'direct_separable': the reference's own separable path raises NameError (blur_estimation.py:77, filters.py:71,78); its
# intent -- a 1-D pass followed by an oblique 1-D pass with linear interpolation, separable_gaussian2d.cpp:91-183 -- is an
# opt-in APPROXIMATION of the 25x25 kernel here (zero boundary like 'direct'); rank-1 kernels are exact either way
_METHODS = {"fft": capi.PB_WRAP, "direct": capi.PB_ZERO, "direct_separable": capi.PB_ZERO}
_SUPPORT = {"full": capi.PB_SUPPORT_FULL, "adaptive": capi.PB_SUPPORT_ADAPTIVE}
_PREFILTER = {"bilateral": capi.PB_PREFILTER_BILATERAL, "domain_transform": capi.PB_PREFILTER_DOMAIN_TRANSFORM,
              "normalized_convolution": capi.PB_PREFILTER_NORMALIZED_CONVOLUTION}

# the reasons of refuse_under_grad that more than one caller gives
HALO_ONLY = "halo masking is differentiated for float32 ROCm tensors only"
FLOAT32_ONLY = "gradients are built for float32 images"
NO_QUANTILE = "the backward of torch.quantile is not built -- pass q=0, which is what the blind driver defaults to"
NO_EDGETAPER = "the edgetaper is not differentiated"
CPU_WITH_GRAD = "%s requires grad and is a CPU tensor -- gradients are built for ROCm tensors only"
PARAM_NOT_ROCM = "%s requires grad and the image is not a float32 ROCm tensor -- parameter gradients are built for float32 ROCm images only"
NO_PHASE_PARAMS = "the gradients with respect to alpha and b are not built for the pure-phase filter"


# ---- predicates and checks ------------------------------------------------------------------------------------------------
def is_tensor(x) -> bool:
    mod = type(x).__module__
    return (mod == "torch" or mod.startswith("torch.")) and hasattr(x, "data_ptr")


def is_rocm_float32(t) -> bool:
    if not is_tensor(t):
        return False
    import torch
    return t.is_cuda and t.dtype == torch.float32


def host_array(a):
    return a.detach().cpu().numpy() if is_tensor(a) else np.asarray(a)


def check_image(img, allow_half):
    """-> (shape, numpy dtype) of a (B,C,H,W) image."""
    if is_tensor(img):
        import torch
        if img.dim() != 4:
            raise ValueError("expected a (B,C,H,W) tensor, got shape %r" % (tuple(img.shape),))
        if img.dtype == torch.float32:
            dt = np.dtype(np.float32)
        elif img.dtype == torch.float16 and allow_half:
            dt = np.dtype(np.float16)
        else:
            raise TypeError("tensor dtype must be float32%s" % (" or float16" if allow_half else ""))
        shape = tuple(img.shape)
    elif isinstance(img, np.ndarray):
        if img.ndim != 4:
            raise ValueError("expected a (B,C,H,W) array, got shape %r" % (img.shape,))
        dt = np.dtype(np.float16) if (img.dtype == np.float16 and allow_half) else np.dtype(np.float32)
        shape = tuple(img.shape)
    else:
        raise TypeError("img must be a numpy.ndarray or a torch.Tensor")
    if shape[0] < 1 or shape[1] < 1 or shape[2] < 2 or shape[3] < 2:
        raise ValueError("bad image shape %r" % (shape,))
    return shape, dt


@lru_cache(maxsize=1024)
def _line_class(n):
    """pb_fft_length_supported(n): 1 = a whole line in LDS, 2 = through a line buffer, 0 = not taken (a pure function of n,
    asked on every call: remembered)"""
    return capi.load_library().pb_fft_length_supported(n)


def check_image_size(h, w):
    """Line lengths the spectral derivative takes (include/polyblur_hip.h: pb_fft_length_supported): whole lines in LDS up
    to 20480 samples (8192 when a prime factor exceeds 7), through a line buffer in device memory up to 65536."""
    for n, what in ((int(h), "height"), (int(w), "width")):
        if n >= 2 and not _line_class(n):
            raise ValueError("image %s %d is beyond the engine's spectral derivative: sides up to 65536 are supported" % (what, n))


def check_phase_sides(hp, wp):
    """the pure-phase filter transforms whole lines of the domain in LDS (pb_fft_length_supported == 1; needs no GPU)"""
    for n in (hp, wp):
        if _line_class(int(n)) != 1:
            raise NotImplementedError("the pure-phase filter transforms the whole %d x %d domain: a side of %d samples is not held "
                                      "in LDS (up to 20480 with prime factors <= 7, up to 8192 otherwise)" % (hp, wp, n))


def check_grad_img(grad_img, shape):
    if not isinstance(grad_img, (tuple, list)) or len(grad_img) != 2:
        raise ValueError("grad_img must be (grad_x, grad_y)")
    for gpart in grad_img:
        if not (is_tensor(gpart) or isinstance(gpart, np.ndarray)):
            raise TypeError("grad_img planes must be numpy.ndarrays or torch.Tensors")
        if tuple(gpart.shape) != shape:
            raise ValueError("grad_img planes must have the image's shape %r" % (shape,))


def wants_grad(*operands) -> bool:
    """autograd is on and one of the operands is a tensor that requires grad"""
    for t in operands:
        if is_tensor(t) and t.requires_grad:
            import torch
            return torch.is_grad_enabled()
    return False


def refuse_under_grad(what, reason):
    raise NotImplementedError("%s has no backward pass: %s" % (what, reason))


# ---- learnable parameters ------------------------------------------------------------------------------------
def check_param(p, name, img=None):
    """A scalar parameter (alpha, beta, c, b) is a Python number or a one-element tensor -- 0-dim or (1,), float32 or float64, on the
    CPU or on the device of the image ``img`` (ValueError otherwise).  -> the tensor where autograd is on and it requires grad, else
    None.  Reads nothing from a device: the value is read later, once, by ``param_value``."""
    if not is_tensor(p):
        return None
    import torch
    if p.numel() != 1 or p.dim() > 1:
        raise ValueError("%s must be a number or a one-element tensor (0-dim or of shape (1,)), got shape %r" % (name, tuple(p.shape)))
    if p.dtype not in (torch.float32, torch.float64):
        raise TypeError("%s: a tensor parameter must be float32 or float64" % name)
    if p.device.type != "cpu" and not (is_tensor(img) and img.device == p.device):
        raise ValueError("%s lives on %s and the image on %s: a tensor parameter lives on the CPU or on the image's device"
                         % (name, p.device, img.device if is_tensor(img) else "the host"))
    return p if p.requires_grad and torch.is_grad_enabled() else None


def param_value(p):
    """the number the engine runs with: ``float(t)`` of a tensor parameter -- one synchronisation when it lives on a device (the
    launch plan sizes window halos from the coefficients on the host) --, a Python number as it is"""
    return float(p.detach()) if is_tensor(p) else p


def refuse_params(what, img, **params):
    """a parameter that requires grad beside an image that is not a float32 ROCm tensor; params: name -> check_param's result"""
    for name, t in params.items():
        if t is not None and not is_rocm_float32(img):
            refuse_under_grad(what, PARAM_NOT_ROCM % name)


def build_options(C, n_iter, c, b, alpha, beta, sigma_r, sigma_s, ker_size, q, n_angles, n_interpolated_angles,
                  remove_halo, edgetaping, prefiltering, discard_saturation, multichannel_kernel, method, support,
                  prefilter, force_theta_deg=-1.0, temporaries="fp32"):
    if method == "direct_separable" and edgetaping:
        raise NotImplementedError("edgetaping is not defined for method='direct_separable'")
    if method not in _METHODS:
        raise ValueError("%s not implemented" % method)          # reference: deblurring.py:119 (never raised there)
    if temporaries not in ("fp32", "fp16"):
        raise ValueError("temporaries must be 'fp32' or 'fp16'")
    if support not in _SUPPORT:
        raise ValueError("support must be 'full' or 'adaptive'")
    if prefilter not in _PREFILTER:
        raise ValueError("prefilter must be 'bilateral', 'domain_transform' or 'normalized_convolution'")
    if not (isinstance(ker_size, (int, np.integer)) and 2 <= ker_size <= capi.PB_KSIZE_MAX):
        # up to 25 the kernel lives in a 25 x 25 record; 26 .. 49 take the large-kernel pass (csrc/conv_big.hip); the replicate
        # pad is ker_size // 2 (even sizes: off-centre, as the reference's grid arange(k) - (k - 1) // 2 and its two convolution
        # paths place them).  sigma is clamped to 4, so 49 holds +-6 sigma: nothing beyond it is built
        raise NotImplementedError("ker_size must be between 2 and 49")
    if ker_size % 2 == 0 and method == "direct_separable":
        raise NotImplementedError("an even ker_size is built for the 'fft' / 'direct' methods only (not with 'direct_separable')")
    if ker_size > capi.PB_KSIZE and method == "direct_separable":
        raise NotImplementedError("a ker_size above 25 is built for the 'fft' / 'direct' methods only (not with 'direct_separable')")
    if not (0 <= q < 0.5):
        raise ValueError("q must be in [0, 0.5)")
    if multichannel_kernel and C not in (1, 3):
        raise NotImplementedError("per-channel kernels crash in the reference for C not in {1,3}")
    if not (1 <= n_angles <= capi.PB_MAX_ANGLES - 1 and 1 <= n_interpolated_angles <= capi.PB_MAX_INTERP):
        raise ValueError("n_angles / n_interpolated_angles out of range")
    return Engine.make_options(n_iter=n_iter, c=c, b=b, alpha=alpha, beta=beta, sigma_r=sigma_r, sigma_s=sigma_s, q=q,
                               n_angles=n_angles, n_interpolated_angles=n_interpolated_angles, remove_halo=remove_halo,
                               edgetaping=edgetaping,
                               prefilter=_PREFILTER[prefilter] if prefiltering else capi.PB_PREFILTER_NONE,
                               discard_saturation=discard_saturation, boundary=_METHODS[method],
                               support=_SUPPORT[support], force_theta_deg=force_theta_deg, ker_size=ker_size,
                               separable_approx=(method == "direct_separable"), half_temporaries=(temporaries == "fp16"))


# ---- the engine of a call, and the staging of its operands --------------------------------------------------------------------
class bound_engine:
    """``with bound_engine(t, device) as eng``: the calling thread's engine for the length of a call -- of the device of the ROCm
    tensor ``t``, under torch's device guard and on torch's current stream there; for host data (``t`` None) of GPU ``device``
    (None: 0) on its default stream.  The only place that hands a stream to an engine.  (A class with slots, not a generator:
    this is inside every timed call.)"""
    __slots__ = ("t", "device", "guard")

    def __init__(self, t=None, device=None):
        self.t, self.device, self.guard = t, device, None

    def __enter__(self):
        t = self.t
        if t is None:
            eng = get_engine(0 if self.device is None else int(self.device))
            eng.set_stream(0)
            return eng
        import torch
        dev = t.device.index
        if dev is None:
            dev = torch.cuda.current_device()
        eng = get_engine(dev)
        guard = self.guard = torch.cuda.device(dev)
        guard.__enter__()
        try:
            eng.set_stream(torch.cuda.current_stream(dev).cuda_stream)
        except BaseException:
            guard.__exit__(None, None, None)
            raise
        return eng

    def __exit__(self, *exc):
        if self.guard is not None:
            self.guard.__exit__(*exc)


def _invoke(eng, call, taps, in_ptr, out_ptrs, extra_ptrs):
    """call, with a KernelSet of `taps` as its last argument where there are taps -- freed when the call is over, which waits
    for the stream: the set is in use until then"""
    if taps is None:
        return call(eng, in_ptr, out_ptrs, extra_ptrs)
    ks = eng.set_taps(taps)
    try:
        return call(eng, in_ptr, out_ptrs, extra_ptrs, ks)
    finally:
        ks.free()


_ONE = ("np.out",)


def staged(img, dt, call, extra=(), outputs=_ONE, taps=None, device=None):
    """One engine call on operands of any of the three kinds: ``call(eng, in_ptr, out_ptrs, extra_ptrs[, ks])`` with device
    pointers -> (the outputs, in the kind of ``img``; what ``call`` returned).

    ``img`` -- a tensor or an array: the caller has checked it -- goes in with NumPy dtype ``dt``; ``extra`` are (pool name,
    operand) pairs the call reads as float32, or (pool name, operand, np.float16) triples it reads as float16; each of ``outputs`` is the pool name of an output like ``img`` or a (pool name,
    shape) pair of float32 words; ``taps``, a (B', kh, kw) host array, becomes the call's KernelSet ``ks``.

    A ROCm ``img``: everything stays on its device and on torch's current stream, asynchronously; every temporary is a torch
    tensor, so torch's allocator keeps it until the stream has passed it.  This is the timed path: the common shape of a call,
    one output and no extras, builds no lists.  Otherwise: through the engine's named pool buffers on GPU ``device``
    (Engine.host_call), synchronously."""
    array = isinstance(img, np.ndarray)
    if not array and img.is_cuda:
        import torch
        xin = img.contiguous()
        if outputs is _ONE:
            out = torch.empty_like(xin)
            outs, out_ptrs = (out,), (out.data_ptr(),)
        else:
            outs = [torch.empty_like(xin) if isinstance(o, str) else torch.empty(o[1], dtype=torch.float32, device=img.device) for o in outputs]
            out_ptrs = [o.data_ptr() for o in outs]
        if extra:
            ex = [torch.as_tensor(e[1], dtype=torch.float16 if e[2:] == (np.float16,) else torch.float32, device=img.device).contiguous()
                  for e in extra]                                                                                  # (kept alive to the end)
            extra_ptrs = [e.data_ptr() for e in ex]
        else:
            extra_ptrs = ()
        with bound_engine(img) as eng:
            return outs, _invoke(eng, call, taps, xin.data_ptr(), out_ptrs, extra_ptrs)
    with bound_engine(None, device) as eng:
        x = np.ascontiguousarray(host_array(img), dtype=dt)
        spec = [(o, x.shape, x.dtype) if isinstance(o, str) else (o[0], o[1], np.float32) for o in outputs]
        outs, ret = eng.host_call(x, lambda i, o, ex: _invoke(eng, call, taps, i, o, ex), [(e[0], host_array(e[1])) + tuple(e[2:]) for e in extra], spec)
    if not array:
        import torch
        outs = [torch.from_numpy(o) for o in outs]
    return outs, ret
