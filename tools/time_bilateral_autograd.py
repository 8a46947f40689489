#!/usr/bin/env python3
"""Times the differentiable bilateral prefilter on one fp32 3-channel image: polyblur_amd.bilateral_filter forward
alone, pb_bilateral_backward alone and forward + backward through the Function at ksize 5, 13 and 25, and
polyblur_deblurring(n_iter=3) forward + backward under grad with and without prefiltering.

    python tools/time_bilateral_autograd.py [--reps 25] [--height 1080 --width 1920]

Device tensors in and out: events around each call on torch's current stream, a warm-up (scratch, kernel attributes), then --reps
calls (at least 20): every figure is [median, smallest, largest] in ms.  The image is synthetic blurred noise in [0.05, 0.95] plus
noise of 0.01.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_blind_autograd import blurred_noise  # noqa: E402


def median_range_ms(fn, reps):
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
    return [round(float(v), 4) for v in (np.median(ms), min(ms), max(ms))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import bilateral_filter, polyblur_deblurring
    from polyblur_amd.engine import get_engine
    rng = np.random.default_rng(1)
    shape = (1, 3, a.height, a.width)
    x = torch.tensor(np.clip(blurred_noise(rng, shape) + 0.01 * rng.standard_normal(shape), 0, 1).astype(np.float32), device="cuda")
    w = torch.tensor(rng.uniform(-1, 1, shape).astype(np.float32), device="cuda")
    eng = get_engine(0)
    gin = torch.empty_like(x)
    out = {"image": list(shape), "reps": reps, "figures": "[median, min, max] ms"}
    for k in (5, 13, 25):
        def forward():
            with torch.no_grad():
                bilateral_filter(x, k)

        def backward_alone():
            eng.set_stream(torch.cuda.current_stream().cuda_stream)
            eng.bilateral_backward_ptr(x.data_ptr(), w.data_ptr(), gin.data_ptr(), shape, k, 5.0, 0.1)

        def forward_backward():
            xt = x.clone().requires_grad_(True)
            bilateral_filter(xt, k).backward(w)

        out["ksize_%d" % k] = {"forward_ms": median_range_ms(forward, reps), "backward_alone_ms": median_range_ms(backward_alone, reps),
                               "forward_backward_ms": median_range_ms(forward_backward, reps)}

    def blind(prefiltering):
        def run():
            xt = x.clone().requires_grad_(True)
            polyblur_deblurring(xt, n_iter=3, prefiltering=prefiltering).backward(w)
        return run

    def blind_plain(prefiltering):
        def run():
            with torch.no_grad():
                polyblur_deblurring(x, n_iter=3, prefiltering=prefiltering)
        return run

    out["blind3_no_grad_ms"] = median_range_ms(blind_plain(False), reps)
    out["blind3_no_grad_prefiltering_ms"] = median_range_ms(blind_plain(True), reps)
    out["blind3_forward_backward_ms"] = median_range_ms(blind(False), reps)
    out["blind3_forward_backward_prefiltering_ms"] = median_range_ms(blind(True), reps)
    out["workspace_mib"] = round(eng.workspace_bytes() / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
