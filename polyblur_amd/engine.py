"""Host-side driver of the C ABI: one `Engine` (= one pb_ctx) per GPU.

Everything here is plumbing: device buffers, option marshalling, numpy <-> device copies.
The arithmetic all happens in libpolyblur_hip.so.
"""
from __future__ import annotations

import ctypes as C
import threading
import weakref

import numpy as np

from . import _capi as capi
from ._capi import PolyblurHipError

_DT = {np.dtype(np.float32): capi.PB_F32, np.dtype(np.float16): capi.PB_F16, np.dtype(np.uint8): capi.PB_U8}


class DeviceBuffer:
    """A hipMalloc'ed buffer owned by an Engine (used when the caller hands us host data)."""

    def __init__(self, engine: "Engine", nbytes: int):
        self.engine = engine
        self.nbytes = int(nbytes)
        p = C.c_void_p()
        engine._check(engine.lib.pb_malloc(engine.ctx, C.byref(p), C.c_size_t(max(self.nbytes, 1))))
        self.ptr = p.value

    def upload(self, arr: np.ndarray):
        arr = np.ascontiguousarray(arr)
        assert arr.nbytes <= self.nbytes
        self.engine._check(self.engine.lib.pb_memcpy_h2d(self.engine.ctx, self.ptr, arr.ctypes.data, arr.nbytes))
        return self

    def download(self, shape, dtype) -> np.ndarray:
        out = np.empty(shape, dtype=dtype)
        assert out.nbytes <= self.nbytes
        self.engine._check(self.engine.lib.pb_memcpy_d2h(self.engine.ctx, out.ctypes.data, self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            self.engine.lib.pb_free(self.engine.ctx, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class KernelSet:
    """A caller's kernels on the device (pb_taps): B kernels of kh x kw taps, owned by this object and not by the engine's
    scratch -- it survives any other call on the engine and is released by free() (or with the object)."""

    def __init__(self, engine: "Engine", taps: np.ndarray, support: int = capi.PB_SUPPORT_FULL):
        k = np.ascontiguousarray(taps, np.float32)
        if k.ndim != 3:
            raise ValueError("expected (B, kh, kw) taps, got shape %r" % (k.shape,))
        self.engine = engine
        self.B, self.kh, self.kw = (int(v) for v in k.shape)
        h = C.c_void_p()
        engine._check(engine.lib.pb_taps_create(engine.ctx, self.B, self.kh, self.kw, k.ctypes.data_as(C.POINTER(C.c_float)),
                                                int(support), C.byref(h)))
        self.handle = h
        engine._sets.add(self)

    def free(self):
        if self.handle and self.engine.ctx:                  # (a closed engine has taken the device memory with it)
            self.engine.lib.pb_taps_free(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class Engine:
    def __init__(self, device: int = 0, stream: int | None = None):
        self.lib = capi.load_library()
        ctx = C.c_void_p()
        rc = self.lib.pb_create(C.byref(ctx), int(device), C.c_void_p(stream or 0))
        if rc != 0:
            raise PolyblurHipError("pb_create(device=%d) failed with %s: no usable MI355X/HIP device "
                                   "(the engine has no CPU fallback)" % (device, capi.STATUS.get(rc, rc)))
        self.ctx = ctx
        self.device = device
        self._pool = {}
        self._sets = weakref.WeakSet()       # live KernelSets: their device memory goes before the context does

    # ---- infrastructure ------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != 0:
            msg = self.lib.pb_last_error_string(self.ctx)
            raise PolyblurHipError("%s: %s" % (capi.STATUS.get(rc, rc), msg.decode() if msg else ""))

    def close(self):
        if self.ctx:
            for b in self._pool.values():
                b.free()
            self._pool.clear()
            for ks in list(self._sets):
                ks.free()
            self.lib.pb_destroy(self.ctx)
            self.ctx = None

    def set_stream(self, stream: int):
        self._check(self.lib.pb_set_stream(self.ctx, C.c_void_p(stream or 0)))

    def synchronize(self):
        self._check(self.lib.pb_synchronize(self.ctx))

    def set_dense_eval(self, mode: str = "auto", min_phases: int = 16):
        """How dense (non rank-1) kernels are evaluated: 'stencil' = always the 2-D stencil body; 'auto' = kernels with
        at least `min_phases` live stencil phases take the tile-spectrum body (pb_set_dense_eval)."""
        m = {"stencil": capi.PB_DENSE_STENCIL, "auto": capi.PB_DENSE_AUTO}[mode]
        self._check(self.lib.pb_set_dense_eval(self.ctx, m, int(min_phases)))

    def set_phase_budget(self, nbytes: int = 0):
        """Bytes of complex scratch one group of plane pairs of the pure-phase polynomial may take (0: the default, 256 MiB;
        one pair is always allowed).  Results do not depend on it (pb_set_phase_budget)."""
        self._check(self.lib.pb_set_phase_budget(self.ctx, C.c_size_t(int(nbytes))))

    def body_selection(self, B: int, iteration: int = -1) -> np.ndarray:
        """(B, 6) int32: per image {tile-spectrum body, halo class, strip, one-pass polynomial, halo x, halo y} of iteration
        `iteration` of the most recent polyblur call (-1: of the most recent estimation / reblurring pass; pb_body_selection)."""
        out = np.zeros((B, 6), np.int32)
        self._check(self.lib.pb_body_selection(self.ctx, int(iteration), out.ctypes.data_as(capi.C.POINTER(capi.C.c_int)), int(B)))
        return out

    def workspace_bytes(self) -> int:
        return int(self.lib.pb_workspace_bytes(self.ctx))

    def buffer(self, name: str, nbytes: int) -> DeviceBuffer:
        """A named, reusable device buffer (grows on demand)."""
        b = self._pool.get(name)
        if b is None or b.nbytes < nbytes:
            if b is not None:
                b.free()
            b = DeviceBuffer(self, nbytes)
            self._pool[name] = b
        return b

    def to_device(self, name: str, arr: np.ndarray) -> DeviceBuffer:
        return self.buffer(name, arr.nbytes).upload(arr)

    @staticmethod
    def make_options(n_iter=1, c=0.352, b=0.768, alpha=2, beta=3, sigma_r=0.8, sigma_s=2.0, q=0.0, n_angles=6,
                     n_interpolated_angles=30, remove_halo=False, edgetaping=False, prefilter=capi.PB_PREFILTER_NONE,
                     discard_saturation=False, boundary=capi.PB_WRAP, support=capi.PB_SUPPORT_FULL,
                     force_theta_deg=-1.0, ker_size=capi.PB_KSIZE, separable_approx=False, half_temporaries=False) -> capi.pb_options:
        o = capi.pb_options()
        o.n_iter = int(n_iter); o.c = float(c); o.b = float(b); o.alpha = float(alpha); o.beta = float(beta)
        o.sigma_s = float(sigma_s); o.sigma_r = float(sigma_r); o.q = float(q); o.n_angles = int(n_angles)
        o.n_interpolated_angles = int(n_interpolated_angles); o.remove_halo = int(bool(remove_halo))
        o.edgetaping = int(bool(edgetaping)); o.prefilter = int(prefilter)
        o.discard_saturation = int(bool(discard_saturation)); o.boundary = int(boundary); o.support = int(support)
        o.force_theta_deg = float(force_theta_deg)
        o.ker_size = int(ker_size)
        o.separable_approx = int(bool(separable_approx))
        o.half_temporaries = int(bool(half_temporaries))
        return o

    # ---- raw-pointer entry points (device pointers as ints) --------------------------------
    def polyblur_ptr(self, in_ptr: int, out_ptr: int, dtype: int, shape, opts: capi.pb_options, want_info=False):
        B, Cc, H, W = (int(v) for v in shape)
        info = None
        ip = None
        if want_info and opts.n_iter > 0:
            info = np.zeros((opts.n_iter, B), dtype=capi.INFO_DTYPE)
            ip = info.ctypes.data
        self._check(self.lib.pb_polyblur_batch(self.ctx, in_ptr, out_ptr, dtype, B, Cc, H, W, C.byref(opts), ip))
        return info

    # ---- numpy conveniences (host arrays in, host arrays out) -------------------------------
    def host_call(self, x: np.ndarray, call, extra=(), outputs=None, sync=True):
        """The one upload / call / download of host data: x goes to "np.in", each (pool name, array) of `extra` to its buffer as
        float32 (a third element: as that dtype); call(in_ptr, out_ptrs, extra_ptrs) runs on the context's stream; `outputs` -- (pool name, shape, dtype) each,
        by default one like x in "np.out" -- come back as arrays.  -> (outputs, what call returned).  `sync`: wait for the
        stream before the download (which waits for it as well: whether a method says so is kept as it was written)."""
        din = self.to_device("np.in", x)
        spec = [("np.out", x.shape, x.dtype)] if outputs is None else outputs
        bufs = [self.buffer(name, int(np.prod(shape)) * np.dtype(dt).itemsize) for name, shape, dt in spec]
        ex = [self.to_device(name, np.ascontiguousarray(a, dt[0] if dt else np.float32)).ptr for name, a, *dt in extra]
        ret = call(din.ptr, [b.ptr for b in bufs], ex)
        if sync:
            self.synchronize()
        return [b.download(shape, dt) for b, (_, shape, dt) in zip(bufs, spec)], ret

    def _one(self, x, call, extra=()):
        """host_call with one output like x, which is all that most conveniences need"""
        return self.host_call(x, lambda i, o, ex: call(i, o[0], *ex), extra)[0][0]

    @staticmethod
    def _grad0(grad0):
        """the halo mask's gradient planes of the original image as `extra` of host_call"""
        return (("np.g0x", grad0[0]), ("np.g0y", grad0[1]))

    def polyblur(self, x: np.ndarray, opts: capi.pb_options, want_info=False):
        x = np.ascontiguousarray(x)
        if x.dtype not in _DT:
            x = x.astype(np.float32)
        (out,), info = self.host_call(x, lambda i, o, ex: self.polyblur_ptr(i, o[0], _DT[x.dtype], x.shape, opts, want_info), sync=False)
        return (out, info) if want_info else out

    def polyblur_u8_hwc(self, imgs: np.ndarray, opts: capi.pb_options, want_info=False):
        """(B,H,W,C) uint8 host images -> deblurred (B,H,W,C) uint8: the bytes go up as they are, are planarised,
        deblurred (8-bit load / store fused into the first / last kernels) and re-interleaved on the device."""
        imgs = np.ascontiguousarray(imgs, dtype=np.uint8)
        B, H, W, Cc = imgs.shape
        hwc = self.to_device("np.u8.hwc", imgs)
        chw = self.buffer("np.u8.chw", imgs.nbytes)
        res = self.buffer("np.u8.out", imgs.nbytes)
        self._check(self.lib.pb_u8_deinterleave(self.ctx, hwc.ptr, chw.ptr, B, Cc, H, W))
        info = self.polyblur_ptr(chw.ptr, res.ptr, capi.PB_U8, (B, Cc, H, W), opts, want_info)
        self._check(self.lib.pb_u8_interleave(self.ctx, res.ptr, hwc.ptr, B, Cc, H, W))
        out = hwc.download(imgs.shape, np.uint8)
        return (out, info) if want_info else out

    def info_buffer(self, name: str, B: int) -> DeviceBuffer:
        return self.buffer(name, B * capi.INFO_DTYPE.itemsize)

    def make_kernels(self, sigma, rho, theta_rad, support=capi.PB_SUPPORT_FULL, name="np.info") -> DeviceBuffer:
        s = np.ascontiguousarray(sigma, np.float32).reshape(-1)
        r = np.ascontiguousarray(rho, np.float32).reshape(-1)
        t = np.ascontiguousarray(theta_rad, np.float32).reshape(-1)
        B = s.size
        buf = self.info_buffer(name, B)
        fp = C.POINTER(C.c_float)
        self._check(self.lib.pb_make_kernels(self.ctx, B, s.ctypes.data_as(fp), r.ctypes.data_as(fp),
                                             t.ctypes.data_as(fp), int(support), buf.ptr))
        return buf

    def set_kernels(self, taps, support=capi.PB_SUPPORT_FULL, name="np.info") -> DeviceBuffer:
        k = np.ascontiguousarray(taps, np.float32).reshape(-1, capi.PB_KSIZE, capi.PB_KSIZE)
        buf = self.info_buffer(name, k.shape[0])
        self._check(self.lib.pb_set_kernels(self.ctx, k.shape[0], k.ctypes.data_as(C.POINTER(C.c_float)),
                                            int(support), buf.ptr))
        return buf

    def read_info(self, buf: DeviceBuffer, B: int) -> np.ndarray:
        self.synchronize()
        return buf.download((B,), capi.INFO_DTYPE)

    def estimate_blur(self, x: np.ndarray, opts: capi.pb_options) -> np.ndarray:
        x = np.ascontiguousarray(x)
        return self.host_call(x, lambda i, o, ex: self.estimate_blur_ptr(i, _DT[x.dtype], x.shape, opts, o[0]),
                              outputs=[("np.info", (x.shape[0],), capi.INFO_DTYPE)])[0][0]

    def fourier_gradients(self, x: np.ndarray):
        x = np.ascontiguousarray(x, np.float32)
        return tuple(self.host_call(x, lambda i, o, ex: self.fourier_gradients_ptr(i, x.shape, o[0], o[1]),
                                    outputs=[("np.gx", x.shape, np.float32), ("np.gy", x.shape, np.float32)])[0])

    def inverse_filter(self, x: np.ndarray, info: DeviceBuffer, alpha, beta, boundary=capi.PB_WRAP, edgetaping=False,
                       remove_halo=False, grad0=None) -> np.ndarray:
        x = np.ascontiguousarray(x)
        B, Cc, H, W = x.shape
        extra = self._grad0(grad0) if remove_halo else ()     # (here the planes are the caller's to give: none is an error)
        return self._one(x, lambda i, o, g0x=None, g0y=None: self._check(self.lib.pb_inverse_filter(
            self.ctx, i, o, _DT[x.dtype], B, Cc, H, W, info.ptr, float(alpha), float(beta), int(boundary), int(bool(edgetaping)),
            int(bool(remove_halo)), g0x, g0y)), extra)

    def convolve2d(self, xp: np.ndarray, info: DeviceBuffer, boundary=capi.PB_WRAP) -> np.ndarray:
        xp = np.ascontiguousarray(xp, np.float32)
        B, Cc, Hp, Wp = xp.shape
        return self._one(xp, lambda i, o: self._check(self.lib.pb_convolve2d(self.ctx, i, o, B, Cc, Hp, Wp, info.ptr, int(boundary))))

    def edgetaper(self, xp: np.ndarray, info: DeviceBuffer, boundary=capi.PB_WRAP) -> np.ndarray:
        xp = np.ascontiguousarray(xp, np.float32)
        B, Cc, Hp, Wp = xp.shape
        return self._one(xp, lambda i, o: self._check(self.lib.pb_edgetaper(self.ctx, i, o, B, Cc, Hp, Wp, info.ptr, int(boundary))))

    # ---- caller-owned kernel sets (pb_taps): any kh x kw up to 49 x 49 ---------------------
    def set_taps(self, taps, support=capi.PB_SUPPORT_FULL) -> KernelSet:
        """(B, kh, kw) taps -> a KernelSet; the caller frees it (KernelSet.free) before the engine is closed."""
        return KernelSet(self, taps, support)

    def convolve2d_taps_ptr(self, in_ptr: int, out_ptr: int, shape, ks: KernelSet, boundary=capi.PB_ZERO):
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_convolve2d_taps(self.ctx, in_ptr, out_ptr, B, Cc, H, W, ks.handle, int(boundary)))

    def edgetaper_taps_ptr(self, in_ptr: int, out_ptr: int, shape, ks: KernelSet, boundary=capi.PB_WRAP, n_tapers=3):
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_edgetaper_taps(self.ctx, in_ptr, out_ptr, B, Cc, H, W, ks.handle, int(boundary), int(n_tapers)))

    def inverse_filter_taps_ptr(self, in_ptr: int, out_ptr: int, dtype: int, shape, ks: KernelSet, alpha, beta,
                                boundary=capi.PB_ZERO, edgetaping=False, remove_halo=False, g0x_ptr=None, g0y_ptr=None):
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_inverse_filter_taps(self.ctx, in_ptr, out_ptr, dtype, B, Cc, H, W, ks.handle, float(alpha),
                                                    float(beta), int(boundary), int(bool(edgetaping)), int(bool(remove_halo)),
                                                    g0x_ptr, g0y_ptr))

    def compute_polynomial_taps_ptr(self, in_ptr: int, out_ptr: int, shape, ks: KernelSet, alpha, beta, boundary=capi.PB_WRAP,
                                    not_symmetric=False):
        """compute_polynomial on float32 planes that are the whole domain (pb_compute_polynomial_taps); unclamped"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_compute_polynomial_taps(self.ctx, in_ptr, out_ptr, B, Cc, H, W, ks.handle, float(alpha), float(beta),
                                                        int(boundary), int(bool(not_symmetric))))

    def inverse_filter_phase_taps_ptr(self, in_ptr: int, out_ptr: int, dtype: int, shape, ks: KernelSet, alpha, beta,
                                      edgetaping=False, remove_halo=False, g0x_ptr=None, g0y_ptr=None):
        """the non-blind chain with the pure-phase filter in the polynomial (pb_inverse_filter_phase_taps)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_inverse_filter_phase_taps(self.ctx, in_ptr, out_ptr, dtype, B, Cc, H, W, ks.handle, float(alpha),
                                                          float(beta), int(bool(edgetaping)), int(bool(remove_halo)), g0x_ptr, g0y_ptr))

    # ---- backward passes of the two above (README: "fully differentiable"); odd kernel sides only -----------------------
    def tap_gradient_ptr(self, u_ptr: int, v_ptr: int, shape, kh: int, kw: int, boundary, grad_ptr: int, scale=1.0, accumulate=False):
        """grad (B,kh,kw; device) = or += scale * the lag correlation of u with v over each image's planes (pb_tap_gradient)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_tap_gradient(self.ctx, u_ptr, v_ptr, B, Cc, H, W, int(kh), int(kw), int(boundary), float(scale),
                                             int(bool(accumulate)), grad_ptr))

    def convolve2d_taps_backward_ptr(self, x_ptr, grad_out_ptr: int, grad_x_ptr, grad_taps_ptr, shape, ks: KernelSet,
                                     boundary=capi.PB_ZERO):
        """grad_x_ptr or grad_taps_ptr may be None, not both; x_ptr may be None without grad_taps_ptr (pb_convolve2d_taps_backward)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_convolve2d_taps_backward(self.ctx, x_ptr, grad_out_ptr, grad_x_ptr, grad_taps_ptr, B, Cc, H, W,
                                                         ks.handle, int(boundary)))

    def compute_polynomial_taps_backward_ptr(self, x_ptr, grad_out_ptr: int, grad_x_ptr, grad_taps_ptr, shape, ks: KernelSet, alpha,
                                             beta, boundary=capi.PB_WRAP):
        """the same for compute_polynomial(not_symmetric=False) (pb_compute_polynomial_taps_backward)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_compute_polynomial_taps_backward(self.ctx, x_ptr, grad_out_ptr, grad_x_ptr, grad_taps_ptr, B, Cc, H, W,
                                                                 ks.handle, float(alpha), float(beta), int(boundary)))

    def compute_polynomial_taps_params_backward_ptr(self, x_ptr: int, grad_out_ptr: int, grad_params_ptr: int, shape, ks: KernelSet, alpha,
                                                    beta, boundary=capi.PB_WRAP):
        """(d / d alpha, d / d beta) of compute_polynomial(not_symmetric=False) per image into the (B,2) float32 device array at
        grad_params_ptr (pb_compute_polynomial_taps_params_backward)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_compute_polynomial_taps_params_backward(self.ctx, x_ptr, grad_out_ptr, grad_params_ptr, B, Cc, H, W,
                                                                        ks.handle, float(alpha), float(beta), int(boundary)))

    def compute_polynomial_phase_taps_backward_ptr(self, x_ptr, grad_out_ptr: int, grad_x_ptr, grad_taps_ptr, shape, ks: KernelSet, alpha,
                                                   beta):
        """the same for compute_polynomial(method='fft', not_symmetric=True); kernel sides even or odd
        (pb_compute_polynomial_phase_taps_backward)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_compute_polynomial_phase_taps_backward(self.ctx, x_ptr, grad_out_ptr, grad_x_ptr, grad_taps_ptr, B, Cc, H,
                                                                       W, ks.handle, float(alpha), float(beta)))

    def edgetaper_taps_backward_ptr(self, x_ptr, grad_out_ptr: int, grad_x_ptr, grad_taps_ptr, shape, ks: KernelSet,
                                    boundary=capi.PB_WRAP, n_tapers=3):
        """the same for edgetaper, through the taper weights as well (pb_edgetaper_taps_backward)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_edgetaper_taps_backward(self.ctx, x_ptr, grad_out_ptr, grad_x_ptr, grad_taps_ptr, B, Cc, H, W,
                                                        ks.handle, int(boundary), int(n_tapers)))

    # ---- the blind estimation on device pointers, and its backward pass --------------------------------------------------
    def estimate_blur_ptr(self, in_ptr: int, dtype: int, shape, opts: capi.pb_options, info_ptr: int):
        """B records into device memory at info_ptr (pb_estimate_blur); asynchronous on the context's stream"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_estimate_blur(self.ctx, in_ptr, int(dtype), B, Cc, H, W, C.byref(opts), info_ptr))

    def estimate_blur_backward_ptr(self, in_ptr: int, shape, opts: capi.pb_options, info_ptr: int, grad_kernel_ptr, grad_sigma_rho_ptr,
                                   ker_size: int, grad_in_ptr: int):
        """d loss / d image for upstream gradients of the (B,k,k) kernels and / or of (sigma, rho) (B,2); either may be None
        (pb_estimate_blur_backward: float32 images, q = 0, odd ker_size up to 25)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_estimate_blur_backward(self.ctx, in_ptr, B, Cc, H, W, C.byref(opts), info_ptr, grad_kernel_ptr,
                                                       grad_sigma_rho_ptr, int(ker_size), grad_in_ptr))

    def estimate_blur_params_backward_ptr(self, in_ptr: int, shape, opts: capi.pb_options, info_ptr: int, grad_kernel_ptr,
                                          grad_sigma_rho_ptr, ker_size: int, grad_in_ptr, grad_cb_ptr):
        """estimate_blur_backward_ptr with one more output: d loss / d (c, b) per image into the (B,2) float32 device array at
        grad_cb_ptr; grad_in_ptr or grad_cb_ptr may be None, not both (pb_estimate_blur_params_backward)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_estimate_blur_params_backward(self.ctx, in_ptr, B, Cc, H, W, C.byref(opts), info_ptr, grad_kernel_ptr,
                                                              grad_sigma_rho_ptr, int(ker_size), grad_in_ptr, grad_cb_ptr))

    def convolve2d_taps(self, x: np.ndarray, ks: KernelSet, boundary=capi.PB_ZERO) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        return self._one(x, lambda i, o: self.convolve2d_taps_ptr(i, o, x.shape, ks, boundary))

    def edgetaper_taps(self, x: np.ndarray, ks: KernelSet, boundary=capi.PB_WRAP, n_tapers=3) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        return self._one(x, lambda i, o: self.edgetaper_taps_ptr(i, o, x.shape, ks, boundary, n_tapers))

    def inverse_filter_taps(self, x: np.ndarray, ks: KernelSet, alpha, beta, boundary=capi.PB_ZERO, edgetaping=False,
                            remove_halo=False, grad0=None) -> np.ndarray:
        x = np.ascontiguousarray(x)
        return self._one(x, lambda i, o, g0x=None, g0y=None: self.inverse_filter_taps_ptr(
            i, o, _DT[x.dtype], x.shape, ks, alpha, beta, boundary, edgetaping, remove_halo, g0x, g0y), self._grad0(grad0) if remove_halo and grad0 is not None else ())

    def compute_polynomial_taps(self, x: np.ndarray, ks: KernelSet, alpha, beta, boundary=capi.PB_WRAP, not_symmetric=False) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        return self._one(x, lambda i, o: self.compute_polynomial_taps_ptr(i, o, x.shape, ks, alpha, beta, boundary, not_symmetric))

    def inverse_filter_phase_taps(self, x: np.ndarray, ks: KernelSet, alpha, beta, edgetaping=False, remove_halo=False,
                                  grad0=None) -> np.ndarray:
        x = np.ascontiguousarray(x)
        return self._one(x, lambda i, o, g0x=None, g0y=None: self.inverse_filter_phase_taps_ptr(
            i, o, _DT[x.dtype], x.shape, ks, alpha, beta, edgetaping, remove_halo, g0x, g0y), self._grad0(grad0) if remove_halo and grad0 is not None else ())

    def halo_mask(self, x, y, g0x, g0y) -> np.ndarray:
        x = np.ascontiguousarray(x, np.float32)
        return self._one(x, lambda i, o, y_ptr, gx_ptr, gy_ptr: self.halo_mask_ptr(i, y_ptr, gx_ptr, gy_ptr, o, x.shape),
                         (("np.y", y),) + self._grad0((g0x, g0y)))

    # ---- halo masking and the spectral derivative on device pointers, and their backward passes ----------
    def fourier_gradients_ptr(self, in_ptr: int, shape, gx_ptr, gy_ptr):
        """gx / gy (either may be None) of the float32 planes at in_ptr (pb_fourier_gradients); asynchronous"""
        H, W = (int(v) for v in shape[-2:])
        self._check(self.lib.pb_fourier_gradients(self.ctx, in_ptr, int(np.prod(shape[:-2], dtype=np.int64)), H, W, gx_ptr, gy_ptr))

    def fourier_gradients_backward_ptr(self, grad_gx_ptr, grad_gy_ptr, shape, grad_in_ptr: int):
        """grad_in = -(Dx grad_gx + Dy grad_gy); either upstream may be None, not both (pb_fourier_gradients_backward)"""
        H, W = (int(v) for v in shape[-2:])
        self._check(self.lib.pb_fourier_gradients_backward(self.ctx, grad_gx_ptr, grad_gy_ptr, int(np.prod(shape[:-2], dtype=np.int64)),
                                                           H, W, grad_in_ptr))

    def halo_mask_ptr(self, x_ptr: int, y_ptr: int, g0x_ptr: int, g0y_ptr: int, out_ptr: int, shape):
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_halo_mask(self.ctx, x_ptr, y_ptr, g0x_ptr, g0y_ptr, out_ptr, B, Cc, H, W))

    def halo_mask_backward_ptr(self, x_ptr: int, y_ptr: int, g0x_ptr: int, g0y_ptr: int, grad_out_ptr: int, grad_x_ptr, grad_y_ptr,
                               grad_g0x_ptr, grad_g0y_ptr, shape):
        """any of the four outputs may be None, not all (pb_halo_mask_backward)"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_halo_mask_backward(self.ctx, x_ptr, y_ptr, g0x_ptr, g0y_ptr, grad_out_ptr, grad_x_ptr, grad_y_ptr,
                                                   grad_g0x_ptr, grad_g0y_ptr, B, Cc, H, W))

    def dt_recursive_filter(self, x: np.ndarray, sigma_s=60.0, sigma_r=0.4, num_iterations=3, joint=None) -> np.ndarray:
        x = np.ascontiguousarray(x)
        B, Cc, H, W = x.shape
        dj = self.to_device("np.joint", np.ascontiguousarray(joint, x.dtype)).ptr if joint is not None else None
        return self._one(x, lambda i, o: self._check(self.lib.pb_dt_recursive_filter(
            self.ctx, i, dj, o, _DT[x.dtype], B, Cc, H, W, float(sigma_s), float(sigma_r), int(num_iterations))))

    def dt_normalized_convolution(self, x: np.ndarray, sigma_s=60.0, sigma_r=0.4, num_iterations=3) -> np.ndarray:
        x = np.ascontiguousarray(x)
        B, Cc, H, W = x.shape
        return self._one(x, lambda i, o: self._check(self.lib.pb_dt_normalized_convolution(
            self.ctx, i, o, _DT[x.dtype], B, Cc, H, W, float(sigma_s), float(sigma_r), int(num_iterations))))

    def bilateral5(self, x: np.ndarray) -> np.ndarray:
        x = np.ascontiguousarray(x)
        B, Cc, H, W = x.shape
        return self._one(x, lambda i, o: self._check(self.lib.pb_bilateral5(self.ctx, i, o, _DT[x.dtype], B, Cc, H, W)))

    # ---- the edge-aware filters on device pointers (polyblur_amd/edge_aware.py) ------------------------------------------
    def bilateral_ptr(self, in_ptr: int, out_ptr: int, dtype: int, shape, ksize, sigma_spatial, sigma_color):
        """the bilateral filter with an odd window of up to 25 x 25 (pb_bilateral; 5: pb_bilateral5's kernel); asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_bilateral(self.ctx, in_ptr, out_ptr, int(dtype), B, Cc, H, W, int(ksize), float(sigma_spatial),
                                          float(sigma_color)))

    def bilateral_backward_ptr(self, in_ptr: int, grad_out_ptr: int, grad_in_ptr: int, shape, ksize, sigma_spatial, sigma_color):
        """d loss / d image of bilateral_ptr's filter, float32 (pb_bilateral_backward); grad_in may alias neither input; asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_bilateral_backward(self.ctx, in_ptr, grad_out_ptr, grad_in_ptr, B, Cc, H, W, int(ksize),
                                                   float(sigma_spatial), float(sigma_color)))

    def dt_recursive_filter_ptr(self, in_ptr: int, joint_ptr, out_ptr: int, dtype: int, shape, sigma_s, sigma_r, num_iterations):
        """joint_ptr: an image like the input's, of its dtype, or None for the input itself (pb_dt_recursive_filter); asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_dt_recursive_filter(self.ctx, in_ptr, joint_ptr, out_ptr, int(dtype), B, Cc, H, W, float(sigma_s),
                                                    float(sigma_r), int(num_iterations)))

    def dt_recursive_filter_backward_ptr(self, in_ptr: int, joint_ptr, grad_out_ptr: int, grad_in_ptr, grad_joint_ptr, shape,
                                         sigma_s, sigma_r, num_iterations):
        """d loss / d image and d loss / d guide of dt_recursive_filter_ptr's filter, float32 (pb_dt_recursive_filter_backward).
        joint_ptr None: guided by the input -- grad_joint_ptr must be None, grad_in receives both paths; either output may be None
        (not both) and is then not computed; the outputs alias no input and not each other; asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_dt_recursive_filter_backward(self.ctx, in_ptr, joint_ptr, grad_out_ptr, grad_in_ptr, grad_joint_ptr,
                                                             B, Cc, H, W, float(sigma_s), float(sigma_r), int(num_iterations)))

    def dt_normalized_convolution_ptr(self, in_ptr: int, out_ptr: int, dtype: int, shape, sigma_s, sigma_r, num_iterations):
        """pb_dt_normalized_convolution (H, W <= 8190); asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        self._check(self.lib.pb_dt_normalized_convolution(self.ctx, in_ptr, out_ptr, int(dtype), B, Cc, H, W, float(sigma_s),
                                                          float(sigma_r), int(num_iterations)))

    # ---- the patch lattice of PolyblurDeblurring(patch_decomposition=True) on device pointers -----------------------------
    def extract_patches_ptr(self, in_ptr: int, patches_ptr: int, dtype: int, shape, grid: dict, first: int, count: int):
        """patches first .. first + count - 1 of every image, replicate-padded to the lattice `grid` (deblurring.patch_grid;
        pb_extract_patches); asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        g = grid
        self._check(self.lib.pb_extract_patches(self.ctx, in_ptr, patches_ptr, dtype, B, Cc, H, W, g["ph"], g["pw"], g["step_h"], g["step_w"],
                                                g["n_i"], g["n_j"], g["pad_top"], g["pad_left"], int(first), int(count)))

    def overlap_add_ptr(self, patches_ptr: int, out_ptr: int, dtype: int, shape, grid: dict, wy_ptr: int, wx_ptr: int):
        """the windowed, normalised overlap-add of all patches, clamped and cropped (pb_overlap_add); asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        g = grid
        self._check(self.lib.pb_overlap_add(self.ctx, patches_ptr, out_ptr, dtype, B, Cc, H, W, g["ph"], g["pw"], g["step_h"], g["step_w"],
                                            g["n_i"], g["n_j"], g["pad_top"], g["pad_left"], C.c_void_p(wy_ptr), C.c_void_p(wx_ptr)))

    def extract_patches_backward_ptr(self, grad_patches_ptr: int, grad_img_ptr: int, shape, grid: dict):
        """d loss / d image of extract_patches_ptr over all n_i * n_j patches ([n*B + b] layout), float32
        (pb_extract_patches_backward); grad_img is written, not accumulated; asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        g = grid
        self._check(self.lib.pb_extract_patches_backward(self.ctx, grad_patches_ptr, grad_img_ptr, B, Cc, H, W, g["ph"], g["pw"],
                                                         g["step_h"], g["step_w"], g["n_i"], g["n_j"], g["pad_top"], g["pad_left"]))

    def overlap_add_backward_ptr(self, patches_ptr: int, grad_out_ptr: int, grad_patches_ptr: int, shape, grid: dict, wy_ptr: int,
                                 wx_ptr: int):
        """d loss / d patches of overlap_add_ptr, float32 (pb_overlap_add_backward): the clamp passes the gradient where the
        forward's value lies in [0, 1], both ends included; grad_patches is written everywhere and aliases no input; asynchronous"""
        B, Cc, H, W = (int(v) for v in shape)
        g = grid
        self._check(self.lib.pb_overlap_add_backward(self.ctx, patches_ptr, grad_out_ptr, grad_patches_ptr, B, Cc, H, W, g["ph"], g["pw"],
                                                     g["step_h"], g["step_w"], g["n_i"], g["n_j"], g["pad_top"], g["pad_left"],
                                                     C.c_void_p(wy_ptr), C.c_void_p(wx_ptr)))

    def profile_begin(self):
        self._check(self.lib.pb_profile_begin(self.ctx))

    def profile_end(self):
        """-> {tag: (total_ms, launches)} for the launches issued since profile_begin()."""
        ms = (C.c_float * len(capi.PROF_TAGS))()
        cnt = (C.c_int * len(capi.PROF_TAGS))()
        self._check(self.lib.pb_profile_end(self.ctx, ms, cnt))
        return {t: (float(ms[i]), int(cnt[i])) for i, t in enumerate(capi.PROF_TAGS)}

    def time_inner_loop(self, in_ptr: int, out_ptr: int, dtype: int, shape, info_ptr: int, alpha, beta,
                        boundary=capi.PB_WRAP, reps=10) -> float:
        B, Cc, H, W = (int(v) for v in shape)
        ms = C.c_float(0)
        self._check(self.lib.pb_time_inner_loop(self.ctx, in_ptr, out_ptr, dtype, B, Cc, H, W, info_ptr, float(alpha),
                                                float(beta), int(boundary), int(reps), C.byref(ms)))
        return float(ms.value)


_tls = threading.local()


class _ThreadEngines:
    """The engines of one host thread; closed (contexts destroyed, scratch freed) when the thread ends."""

    def __init__(self):
        self.by_device = {}

    def __del__(self):
        for e in self.by_device.values():
            try:
                e.close()
            except Exception:
                pass


def get_engine(device: int = 0) -> Engine:
    """The calling thread's Engine for a GPU (created on first use).  A pb_ctx is not thread-safe and owns its
    scratch buffers, so every host thread gets its own -- kept in thread-local storage, so that a thread that ends takes
    its contexts (and their HBM) with it and a recycled thread id never inherits another thread's engine; within a
    thread, calls on different streams are ordered by pb_set_stream (the new stream waits for the work queued on the
    previous one)."""
    box = getattr(_tls, "engines", None)
    if box is None:
        box = _tls.engines = _ThreadEngines()
    e = box.by_device.get(int(device))
    if e is None or e.ctx is None:
        e = Engine(device)
        box.by_device[int(device)] = e
    return e
