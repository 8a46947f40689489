#!/usr/bin/env python3
"""What a window 64 wide and 128 tall costs in pairs of 64 x 64 windows (PB_POLY_COST_TALL, csrc/common.h): the one-pass
polynomial of one 3840 x 2160 x 3 fp32 image with the headline's three estimates as host-built records (the constant is the
second's figure; the first shows what the 128 x 128 form the model keeps there is worth), through a
context that always takes the tall form (PB_POLY_TALL=2) and one that never does (PB_POLY_TALL=0), timed with
pb_time_inner_loop; time per job = time per pass / jobs per pass.  GPU box only:  python tools/tall_timing.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from polyblur_amd import _capi as capi
from polyblur_amd.engine import Engine

H, W, C = 2160, 3840, 3
RECORDS = [("iteration 1", 66.0, 2.095, 1.314), ("iteration 2", 66.0, 1.656, 1.009), ("iteration 3", 66.0, 1.240, 0.625)]


def engine(tall):
    os.environ["PB_POLY_TALL"] = str(tall)
    try:
        return Engine(0)
    finally:
        del os.environ["PB_POLY_TALL"]


def jobs(hx, hy, tall, form):
    """jobs of a pass: single tall windows, pairs of 64 x 64 windows (form 1) or pairs of 128 x 128 windows (form 2)"""
    n = 128 if form == 2 else 64
    tx, ty = n - 2 * hx, (128 if tall else n) - 2 * hy
    nx = -(-W // tx)
    return (nx if tall else (nx + 1) // 2) * -(-H // ty) * C


def main():
    x = torch.rand(1, C, H, W, device="cuda")
    o = torch.empty_like(x)
    engs = {0: engine(0), 2: engine(2)}
    for name, deg, sg, rh in RECORDS:
        res = {}
        for tall, eng in engs.items():
            eng.set_stream(torch.cuda.current_stream(0).cuda_stream)
            buf = eng.make_kernels([sg], [rh], [np.float32(np.deg2rad(deg))], support=capi.PB_SUPPORT_FULL, name="tt.info")
            ms = [eng.time_inner_loop(x.data_ptr(), o.data_ptr(), capi.PB_F32, x.shape, buf.ptr, 6.0, 1.0, capi.PB_WRAP, 50) for _ in range(5)]
            sel = eng.body_selection(1)[0]
            n = jobs(int(sel[4]), int(sel[5]), tall == 2, int(sel[3]))
            res[tall] = (float(np.median(ms)), n)
            print("%s  PB_POLY_TALL=%d  form %d halos (%d, %d)  %d jobs  %.2f us per pass (median of 5 x 50; %s)  %.3f ns per job"
                  % (name, tall, sel[3], sel[4], sel[5], n, 1e3 * np.median(ms), " ".join("%.2f" % (1e3 * m) for m in ms),
                     1e6 * np.median(ms) / n), flush=True)
        (t0, n0), (t2, n2) = res[0], res[2]
        print("%s  a tall job in 64 x 64 pair jobs: %.3f   pass time tall / pairs: %.3f" % (name, (t2 / n2) / (t0 / n0), t2 / t0), flush=True)


if __name__ == "__main__":
    main()
