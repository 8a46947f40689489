#!/usr/bin/env python3
"""Times the backward pass of polyblur_amd.compute_polynomial (method='fft') on one fp32 3-channel image with 5 x 5, 25 x 25
and 49 x 49 kernels: forward alone, forward + backward with respect to the image, forward + backward with respect to image and
kernel, and the tap gradient (pb_tap_gradient, conv_grad.hip) alone.

    python tools/time_autograd.py [--reps 25] [--height 1080 --width 1920]

Device tensors in and out: events around each call on torch's current stream, a warm-up (scratch, kernel attributes), the median
of --reps calls (at least 20).  Every call builds its kernel set (pb_taps_create copies the taps and synchronises), the backward
builds it again: that is inside the figures.  "tap_gradient_ms" is one pb_tap_gradient call on resident planes, nothing else
between its events.  Prints one JSON line per kernel size."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import _capi as capi, compute_polynomial
    from polyblur_amd.engine import get_engine
    rng = np.random.default_rng(1)
    shape = (1, 3, a.height, a.width)
    x = torch.tensor(rng.random(shape, dtype=np.float32), device="cuda")
    w = torch.tensor(rng.uniform(-1, 1, shape).astype(np.float32), device="cuda")
    eng = get_engine(0)
    for size in (5, 25, 49):
        k = rng.random((1, 1, size, size)) ** 3
        k = torch.tensor((k / k.sum()).astype(np.float32), device="cuda")

        def forward():
            with torch.no_grad():
                compute_polynomial(x, k, 6, 1, method="fft")

        def backward(image, kernel):
            xt, kt = x.clone().requires_grad_(image), k.clone().requires_grad_(kernel)
            compute_polynomial(xt, kt, 6, 1, method="fft").backward(w)

        g = torch.empty((1, size, size), device="cuda")

        def taps():
            eng.set_stream(torch.cuda.current_stream().cuda_stream)
            eng.tap_gradient_ptr(w.data_ptr(), x.data_ptr(), shape, size, size, capi.PB_WRAP, g.data_ptr())

        print(json.dumps({"kernel": "%dx%d" % (size, size), "image": list(shape), "reps": reps,
                          "forward_ms": median_ms(forward, reps),
                          "forward_backward_image_ms": median_ms(lambda: backward(True, False), reps),
                          "forward_backward_image_kernel_ms": median_ms(lambda: backward(True, True), reps),
                          "tap_gradient_ms": median_ms(taps, reps),
                          "workspace_mib": round(eng.workspace_bytes() / 2 ** 20, 1)}), flush=True)


if __name__ == "__main__":
    main()
