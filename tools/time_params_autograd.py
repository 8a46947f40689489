#!/usr/bin/env python3
"""Times the parameter gradients on one fp32 3-channel image at 1080p and at 4K:

  * the polynomial's backward (25 x 25 oblique Gaussian, method 'fft'): pb_compute_polynomial_taps_backward for grad_x alone and
    for grad_x and grad_taps, and pb_compute_polynomial_taps_params_backward (three passes and one read of three plane sets);
  * the estimation's backward on resident records: pb_estimate_blur_backward (grad_in) against pb_estimate_blur_params_backward
    with grad_cb alone (no scatter) and with both.

    python tools/time_params_autograd.py [--reps 25] [--sizes 1080x1920,2160x3840]

Device tensors in and out: events around each call on torch's current stream, three warm-up calls (scratch, plans, kernel
attributes), then --reps calls (at least 20): median, minimum and maximum.  Prints one JSON line per size."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed_ms(fn, reps):
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
    return dict(median=round(float(np.median(ms)), 4), min=round(float(min(ms)), 4), max=round(float(max(ms)), 4))


def smooth_noise(rng, shape):
    x = rng.random(shape, dtype=np.float32)
    for _ in range(3):
        for ax in (-2, -1):
            x = 0.25 * np.roll(x, 1, ax) + 0.5 * x + 0.25 * np.roll(x, -1, ax)
    return (0.05 + 0.9 * (x - x.min()) / (x.max() - x.min())).astype(np.float32)


def gaussian_taps(k=25, s1=2.2, s2=1.1, t=0.6):
    yy, xx = np.meshgrid(np.arange(k) - k // 2, np.arange(k) - k // 2, indexing="ij")
    u, v = np.cos(t) * xx + np.sin(t) * yy, -np.sin(t) * xx + np.cos(t) * yy
    e = np.exp(-0.5 * ((u / s1) ** 2 + (v / s2) ** 2))
    return (e / e.sum()).astype(np.float32)[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import _capi as capi
    from polyblur_amd.engine import Engine, get_engine
    eng = get_engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    rng = np.random.default_rng(1)
    for size in a.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        shape = (1, 3, H, W)
        x = torch.tensor(smooth_noise(rng, shape), device="cuda")
        g = torch.tensor(rng.uniform(-1, 1, shape).astype(np.float32), device="cuda")
        gx, gk, gp = torch.empty_like(x), torch.empty((1, 25, 25), device="cuda"), torch.empty((1, 2), device="cuda")
        ks = eng.set_taps(gaussian_taps())
        out = dict(size=size, reps=reps)
        try:
            poly = lambda a_, b_: eng.compute_polynomial_taps_backward_ptr(x.data_ptr(), g.data_ptr(), a_, b_, shape, ks, 6, 1, capi.PB_WRAP)
            out["poly_grad_x"] = timed_ms(lambda: poly(gx.data_ptr(), None), reps)
            out["poly_grad_x_taps"] = timed_ms(lambda: poly(gx.data_ptr(), gk.data_ptr()), reps)
            out["poly_grad_params"] = timed_ms(lambda: eng.compute_polynomial_taps_params_backward_ptr(
                x.data_ptr(), g.data_ptr(), gp.data_ptr(), shape, ks, 6, 1, capi.PB_WRAP), reps)
        finally:
            ks.free()
        opts = Engine.make_options(c=0.352, b=0.768, q=0.0)
        rec = torch.empty((1, capi.INFO_DTYPE.itemsize // 4), device="cuda")
        wk = torch.tensor(rng.uniform(-1, 1, (1, 25, 25)).astype(np.float32), device="cuda")
        eng.estimate_blur_ptr(x.data_ptr(), capi.PB_F32, shape, opts, rec.data_ptr())
        est = lambda gi, gc: eng.estimate_blur_params_backward_ptr(x.data_ptr(), shape, opts, rec.data_ptr(), wk.data_ptr(), None, 25, gi, gc)
        out["est_grad_in_old"] = timed_ms(lambda: eng.estimate_blur_backward_ptr(x.data_ptr(), shape, opts, rec.data_ptr(), wk.data_ptr(), None, 25,
                                                                                gx.data_ptr()), reps)
        out["est_grad_cb"] = timed_ms(lambda: est(None, gp.data_ptr()), reps)
        out["est_grad_in_cb"] = timed_ms(lambda: est(gx.data_ptr(), gp.data_ptr()), reps)
        print(json.dumps(out), flush=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    main()
