#!/usr/bin/env python3
"""Times the two ends of the patch decomposition and their backward passes on one fp32 image: pb_extract_patches
of all patches plus pb_overlap_add (the forward pair), pb_extract_patches_backward plus pb_overlap_add_backward (the backward pair),
and each of the four alone.

    python tools/time_patch_autograd.py [--reps 25] [--height 2160 --width 3840] [--patch 400] [--overlap 0.25]

Device tensors in and out, events around each call on torch's current stream, a warm-up (scratch), then --reps rounds (at least
20) in which the measurements alternate, so that a drift of the clocks meets all of them alike: every figure is [median, smallest,
largest] in ms.  Prints one JSON line."""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=25)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--patch", type=int, default=400)
    ap.add_argument("--overlap", type=float, default=0.25)
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import _capi as capi
    from polyblur_amd.engine import get_engine
    from polyblur_amd.patches import check_lattice, windows
    shape = (1, 3, a.height // 2 * 2, a.width // 2 * 2)
    g = check_lattice(shape[2], shape[3], (a.patch, a.patch), a.overlap)
    n_p = g["n_i"] * g["n_j"]
    gen = torch.Generator("cuda").manual_seed(1)
    x = torch.rand(shape, device="cuda", generator=gen)
    w = torch.rand(shape, device="cuda", generator=gen) - 0.5
    patches = torch.empty((n_p * shape[0], shape[1], g["ph"], g["pw"]), device="cuda")
    gp, out, gx = torch.empty_like(patches), torch.empty_like(x), torch.empty_like(x)
    wy, wx = windows(g, x.device)
    eng = get_engine(0)
    eng.set_stream(torch.cuda.current_stream().cuda_stream)
    calls = {
        "extract": lambda: eng.extract_patches_ptr(x.data_ptr(), patches.data_ptr(), capi.PB_F32, shape, g, 0, n_p),
        "overlap_add": lambda: eng.overlap_add_ptr(patches.data_ptr(), out.data_ptr(), capi.PB_F32, shape, g, wy.data_ptr(), wx.data_ptr()),
        "overlap_add_backward": lambda: eng.overlap_add_backward_ptr(patches.data_ptr(), w.data_ptr(), gp.data_ptr(), shape, g, wy.data_ptr(), wx.data_ptr()),
        "extract_backward": lambda: eng.extract_patches_backward_ptr(gp.data_ptr(), gx.data_ptr(), shape, g),
    }
    calls["forward_pair"] = lambda: (calls["extract"](), calls["overlap_add"]())
    calls["backward_pair"] = lambda: (calls["overlap_add_backward"](), calls["extract_backward"]())
    for _ in range(3):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in calls}
    for _ in range(reps):
        for k, fn in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    res = {"image": list(shape), "patch": a.patch, "overlap": a.overlap, "patches": n_p, "pads": [g["pad_top"], g["pad_left"]], "reps": reps,
           "figures": "[median, min, max] ms"}
    for k, v in ms.items():
        res[k + "_ms"] = [round(float(t), 4) for t in (np.median(v), min(v), max(v))]
    res["patch_mib"] = round(patches.numel() * 4 / 2 ** 20, 1)
    res["workspace_mib"] = round(eng.workspace_bytes() / 2 ** 20, 1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
