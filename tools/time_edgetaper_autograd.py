#!/usr/bin/env python3
"""Times the edgetaper and its backward (api.hip: pb_edgetaper_taps, pb_edgetaper_taps_backward; edgetaper_grad.hip)
on the replicate-padded domain of a 1080p and a 4K fp32 three-channel image with a 25 x 25 kernel and three blends, PB_WRAP:

    forward          pb_edgetaper_taps
    backward image   pb_edgetaper_taps_backward(grad_x only)
    backward both    ... (grad_x and grad_taps)

    python tools/time_edgetaper_autograd.py [--reps 25] [--sizes 1080x1920,2160x3840]

Device tensors in and out and one kernel set per image made before the clock starts, so a call is its launches: events around each
call on torch's current stream, a warm-up (scratch, kernel attributes, the records' spectra), the median and the range of --reps calls
(at least 20), all on the same build in the same run.  Prints one JSON line per image."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timed(fn, reps):
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
    ms.sort()
    return {"median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--sizes", default="1080x1920,2160x3840")
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import _capi as capi
    from polyblur_amd.engine import get_engine
    from polyblur_amd.synthetic import synthetic_blurry_batch
    eng = get_engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    ksize, n, pad = 25, 3, 12
    for size in a.sizes.split(","):
        h, w = (int(v) for v in size.split("x"))
        x0, _ = synthetic_blurry_batch(1, 3, h, w, seed0=1)
        x = torch.nn.functional.pad(torch.from_numpy(x0.astype(np.float32)).cuda(), (pad,) * 4, mode="replicate").contiguous()
        g = torch.empty_like(x).uniform_(-1, 1)
        out, gx = torch.empty_like(x), torch.empty_like(x)
        gk = torch.empty((1, ksize, ksize), device="cuda")
        k = np.random.default_rng(ksize).random((1, ksize, ksize)) ** 3
        ks = eng.set_taps((k / k.sum()).astype(np.float32))
        ptr = lambda t: t.data_ptr()
        back = lambda px, pk: eng.edgetaper_taps_backward_ptr(ptr(x), ptr(g), px, pk, x.shape, ks, capi.PB_WRAP, n)
        row = {"image": [1, 3, h, w], "domain": list(x.shape[-2:]), "kernel": "%dx%d" % (ksize, ksize), "n_tapers": n, "reps": reps}
        row["forward"] = timed(lambda: eng.edgetaper_taps_ptr(ptr(x), ptr(out), x.shape, ks, capi.PB_WRAP, n), reps)
        row["backward_image"] = timed(lambda: back(ptr(gx), None), reps)
        row["backward_both"] = timed(lambda: back(ptr(gx), ptr(gk)), reps)
        row["workspace_mib"] = round(eng.workspace_bytes() / 2 ** 20, 1)          # (the context's, forward and backward scratch: grows, never shrinks)
        ks.free()
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
