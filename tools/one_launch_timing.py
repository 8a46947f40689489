#!/usr/bin/env python3
"""What four wave jobs per workgroup cost against one (csrc/conv_win.hip against csrc/conv_wfft.hip / csrc/conv_w128.hip): the
one-pass polynomial of one 3840 x 2160 x 3 fp32 image with the headline's three estimates as host-built records, through a
context that issues the merged launch with the exact grid (the lab switch PB_POLY_ONE_LAUNCH=2) and one that issues the
separate launch the records need (PB_POLY_ONE_LAUNCH=0: exact launches, exact grids), timed with pb_time_inner_loop; median
of 5 x 50 passes.  Iteration 1 runs 128 x 128 windows -- same body, same workgroups: it must not move --, iterations 2 and 3 the
wave bodies, whose slots the merged launch holds until the slowest of four neighbouring jobs ends.
GPU box only:  python tools/one_launch_timing.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from polyblur_amd import _capi as capi
from polyblur_amd.engine import Engine

H, W, C = 2160, 3840, 3
RECORDS = [("iteration 1", 66.0, 2.095, 1.314), ("iteration 2", 66.0, 1.656, 1.009), ("iteration 3", 66.0, 1.240, 0.625)]


def engine(one_launch):
    os.environ["PB_POLY_ONE_LAUNCH"] = str(one_launch)
    try:
        return Engine(0)
    finally:
        del os.environ["PB_POLY_ONE_LAUNCH"]


def main():
    x = torch.rand(1, C, H, W, device="cuda")
    engs = {"separate": engine(0), "merged": engine(2)}
    outs = {k: torch.empty_like(x) for k in engs}
    for name, deg, sg, rh in RECORDS:
        res = {}
        for kind, eng in engs.items():
            eng.set_stream(torch.cuda.current_stream(0).cuda_stream)
            buf = eng.make_kernels([sg], [rh], [np.float32(np.deg2rad(deg))], support=capi.PB_SUPPORT_FULL, name="ol.info")
            ms = [eng.time_inner_loop(x.data_ptr(), outs[kind].data_ptr(), capi.PB_F32, x.shape, buf.ptr, 6.0, 1.0, capi.PB_WRAP, 50) for _ in range(5)]
            sel = eng.body_selection(1)[0]
            res[kind] = float(np.median(ms))
            print("%s  %-8s  form %d halos (%d, %d)  %.2f us per pass (median of 5 x 50; %s)"
                  % (name, kind, sel[3], sel[4], sel[5], 1e3 * np.median(ms), " ".join("%.2f" % (1e3 * m) for m in ms)), flush=True)
        torch.cuda.synchronize()
        print("%s  merged - separate: %+.2f us (%.3f x)   same bits: %s"
              % (name, 1e3 * (res["merged"] - res["separate"]), res["merged"] / res["separate"], bool(torch.equal(outs["merged"], outs["separate"]))),
              flush=True)


if __name__ == "__main__":
    main()
