#!/usr/bin/env python3
"""Times the differentiable blind path on one fp32 3-channel image: polyblur_amd.gaussian_blur_estimation forward
alone, its backward alone (pb_estimate_blur_backward on resident records, and split by kernel class with the engine's profiler),
and polyblur_deblurring(n_iter=3) forward + backward under grad, beside the same call under torch.no_grad().

    python tools/time_blind_autograd.py [--reps 25] [--height 1080 --width 1920]

Device tensors in and out: events around each call on torch's current stream, a warm-up (scratch, plans, kernel attributes), the
median of --reps calls (at least 20).  The image is synthetic blurred noise in [0.05, 0.95].  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_ms(fn, reps):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return round(float(np.median(ms)), 4)


def blurred_noise(rng, shape):
    B, C, H, W = shape
    fy, fx = np.meshgrid(np.fft.fftfreq(H), np.fft.fftfreq(W), indexing="ij")
    u, v = 0.8 * fx + 0.6 * fy, -0.6 * fx + 0.8 * fy
    y = np.real(np.fft.ifft2(np.fft.fft2(rng.random(shape)) * np.exp(-2 * np.pi ** 2 * ((2.2 * u) ** 2 + (1.1 * v) ** 2))))
    return (0.05 + 0.9 * (y - y.min()) / (y.max() - y.min())).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import _capi as capi, gaussian_blur_estimation, polyblur_deblurring
    from polyblur_amd.engine import Engine, get_engine
    rng = np.random.default_rng(1)
    shape = (1, 3, a.height, a.width)
    x = torch.tensor(blurred_noise(rng, shape), device="cuda")
    w = torch.tensor(rng.uniform(-1, 1, shape).astype(np.float32), device="cuda")
    wk = torch.tensor(rng.uniform(-1, 1, (1, 25, 25)).astype(np.float32), device="cuda")
    eng = get_engine(0)
    opts = Engine.make_options(c=0.352, b=0.768, q=0.0)
    rec = torch.empty((1, capi.INFO_DTYPE.itemsize // 4), device="cuda")
    gin = torch.empty_like(x)

    def est_forward():
        with torch.no_grad():
            gaussian_blur_estimation(x, q=0.0, c=0.352, b=0.768)

    def est_backward():
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.estimate_blur_backward_ptr(x.data_ptr(), shape, opts, rec.data_ptr(), wk.data_ptr(), None, 25, gin.data_ptr())

    def blind_plain():
        with torch.no_grad():
            polyblur_deblurring(x, n_iter=3)

    def blind_grad():
        xt = x.clone().requires_grad_(True)
        polyblur_deblurring(xt, n_iter=3).backward(w)

    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    eng.estimate_blur_ptr(x.data_ptr(), capi.PB_F32, shape, opts, rec.data_ptr())
    out = {"image": list(shape), "reps": reps, "estimation_forward_ms": median_ms(est_forward, reps),
           "estimation_backward_ms": median_ms(est_backward, reps)}
    # where the backward's time goes: the engine's event pairs around every launch, by kernel class
    eng.profile_begin()
    est_backward()
    prof = eng.profile_end()
    out["estimation_backward_by_class_ms"] = {k: round(v[0], 4) for k, v in prof.items() if v[1]}
    out["blind3_no_grad_ms"] = median_ms(blind_plain, reps)
    out["blind3_forward_backward_ms"] = median_ms(blind_grad, reps)
    out["workspace_mib"] = round(eng.workspace_bytes() / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
