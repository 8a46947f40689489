#!/usr/bin/env python3
"""Times the differentiable recursive filter on one fp32 3-channel image at 1080p and at 4K, one and three
iterations: polyblur_amd.recursive_filter forward alone (self-guided, torch.no_grad()), pb_dt_recursive_filter_backward alone with
a joint image -- the image's gradient only (no guide gradient: no Dbar planes, no guide kernel) and both gradients -- and
self-guided.

    python tools/time_dt_autograd.py [--reps 25]

Device tensors in and out: events around each call on torch's current stream, a warm-up (scratch), then --reps calls (at least
20): every figure is [median, smallest, largest] in ms.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from time_bilateral_autograd import median_range_ms  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import recursive_filter
    from polyblur_amd.engine import get_engine
    eng = get_engine(0)
    out = {"reps": reps, "figures": "[median, min, max] ms", "sigma_s": 60.0, "sigma_r": 0.4}
    for name, (H, W) in (("1080p", (1080, 1920)), ("4k", (2160, 3840))):
        shape = (1, 3, H, W)
        x, j, w = (torch.rand(shape, device="cuda") for _ in range(3))
        gx, gj = torch.empty_like(x), torch.empty_like(x)
        for n in (1, 3):
            def forward():
                with torch.no_grad():
                    recursive_filter(x, 60.0, 0.4, n)

            def backward(joint, want_j):
                def run():
                    eng.set_stream(torch.cuda.current_stream().cuda_stream)
                    eng.dt_recursive_filter_backward_ptr(x.data_ptr(), j.data_ptr() if joint else None, w.data_ptr(), gx.data_ptr(),
                                                         gj.data_ptr() if want_j else None, shape, 60.0, 0.4, n)
                return run

            out["%s_n%d" % (name, n)] = {"forward_ms": median_range_ms(forward, reps),
                                         "backward_image_only_ms": median_range_ms(backward(True, False), reps),
                                         "backward_image_and_guide_ms": median_range_ms(backward(True, True), reps),
                                         "backward_self_guided_ms": median_range_ms(backward(False, False), reps)}
    out["workspace_mib"] = round(eng.workspace_bytes() / 2 ** 20, 1)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
