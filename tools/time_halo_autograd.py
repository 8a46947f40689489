#!/usr/bin/env python3
"""Times differentiable halo masking on one fp32 3-channel image: polyblur_amd.halo_masking forward alone and
forward + backward (all four gradients), pb_halo_mask_backward alone split by kernel class with the engine's profiler, and
polyblur_deblurring(n_iter=3) forward + backward under grad with and without remove_halo.

    python tools/time_halo_autograd.py [--reps 25] [--height 1080 --width 1920]

Device tensors in and out: events around each call on torch's current stream, a warm-up (scratch, plans, kernel attributes), the
median of --reps calls (at least 20).  The image is synthetic blurred noise in [0.05, 0.95], the "deblurred" operand of the stage
alone another such image.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_blind_autograd import blurred_noise, median_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--width", type=int, default=1920)
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import fourier_gradients, halo_masking, polyblur_deblurring
    from polyblur_amd.engine import get_engine
    rng = np.random.default_rng(1)
    shape = (1, 3, a.height, a.width)
    x = torch.tensor(blurred_noise(rng, shape), device="cuda")
    y = torch.tensor(blurred_noise(rng, shape), device="cuda")
    w = torch.tensor(rng.uniform(-1, 1, shape).astype(np.float32), device="cuda")
    gx, gy = fourier_gradients(x)
    eng = get_engine(0)
    outs = [torch.empty_like(x) for _ in range(4)]

    def halo_forward():
        with torch.no_grad():
            halo_masking(x, y, (gx, gy))

    def halo_forward_backward():
        ts = [t.clone().requires_grad_(True) for t in (x, y, gx, gy)]
        halo_masking(ts[0], ts[1], (ts[2], ts[3])).backward(w)

    def halo_backward_alone():
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.halo_mask_backward_ptr(x.data_ptr(), y.data_ptr(), gx.data_ptr(), gy.data_ptr(), w.data_ptr(), *[o.data_ptr() for o in outs], shape)

    def halo_backward_image_only():
        eng.set_stream(torch.cuda.current_stream().cuda_stream)
        eng.halo_mask_backward_ptr(x.data_ptr(), y.data_ptr(), gx.data_ptr(), gy.data_ptr(), w.data_ptr(), outs[0].data_ptr(), outs[1].data_ptr(),
                                   None, None, shape)

    def blind(remove_halo):
        def run():
            xt = x.clone().requires_grad_(True)
            polyblur_deblurring(xt, n_iter=3, remove_halo=remove_halo).backward(w)
        return run

    def blind_plain(remove_halo):
        def run():
            with torch.no_grad():
                polyblur_deblurring(x, n_iter=3, remove_halo=remove_halo)
        return run

    out = {"image": list(shape), "reps": reps, "halo_forward_ms": median_ms(halo_forward, reps),
           "halo_forward_backward_ms": median_ms(halo_forward_backward, reps),
           "halo_backward_alone_ms": median_ms(halo_backward_alone, reps),
           "halo_backward_alone_x_y_only_ms": median_ms(halo_backward_image_only, reps)}
    eng.profile_begin()
    halo_backward_alone()
    prof = eng.profile_end()
    out["halo_backward_by_class_ms"] = {k: round(v[0], 4) for k, v in prof.items() if v[1]}
    out["blind3_no_grad_ms"] = median_ms(blind_plain(False), reps)
    out["blind3_no_grad_remove_halo_ms"] = median_ms(blind_plain(True), reps)
    out["blind3_forward_backward_ms"] = median_ms(blind(False), reps)
    out["blind3_forward_backward_remove_halo_ms"] = median_ms(blind(True), reps)
    out["workspace_mib"] = round(eng.workspace_bytes() / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
