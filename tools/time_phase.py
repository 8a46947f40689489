#!/usr/bin/env python3
"""Times one 4K fp32 3-channel call of polyblur_amd.inverse_filtering_nonsymmetric (the pure-phase filter: one transform over
the whole padded domain, conv_phase.hip) with a 25 x 25 and a 49 x 49 kernel, and the same calls of
inverse_filtering_rank3(method='fft') on the same build.

    python tools/time_phase.py [--reps 25] [--height 2160 --width 3840]

Device tensors in and out, so a call is its launches: events around each call on torch's current stream, a warm-up (plans,
scratch, kernel attributes), the median of --reps calls (at least 20); "launches_ms" is the device time of one more call's
launches alone (the engine's own event pairs).  Both functions build their kernel set per call
(pb_taps_create copies the taps and synchronises): that is inside the figure, for both alike.  Prints one JSON line per
(function, kernel)."""
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
    a = ap.parse_args()
    reps = max(20, a.reps)
    import torch
    from polyblur_amd import inverse_filtering_nonsymmetric, inverse_filtering_rank3
    from polyblur_amd.engine import get_engine
    from polyblur_amd.synthetic import synthetic_blurry_batch
    x0, _ = synthetic_blurry_batch(1, 3, a.height, a.width, seed0=1)
    x = torch.from_numpy((0.3 + 0.4 * x0).astype(np.float32)).cuda()
    calls = (("inverse_filtering_nonsymmetric", lambda k: inverse_filtering_nonsymmetric(x, k, 2, 3)),
             ("inverse_filtering_rank3_fft", lambda k: inverse_filtering_rank3(x, k, 2, 3, method="fft")))
    for size in (25, 49):
        k = np.random.default_rng(size).random((1, 1, size, size)) ** 3
        k = (k / k.sum()).astype(np.float32)
        for name, fn in calls:
            for _ in range(3):
                fn(k)
            torch.cuda.synchronize()
            ms = []
            for _ in range(reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(k)
                e1.record()
                e1.synchronize()
                ms.append(e0.elapsed_time(e1))
            ms.sort()
            # the launches alone (event pairs around each, pb_profile_begin / _end): what the call costs without the host's part
            eng = get_engine(0)
            eng.profile_begin()
            fn(k)
            prof = eng.profile_end()
            launches_ms = sum(v[0] for v in prof.values())
            print(json.dumps({"call": name, "kernel": "%dx%d" % (size, size), "image": [1, 3, a.height, a.width],
                              "median_ms": round(float(np.median(ms)), 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4),
                              "reps": reps, "launches_ms": round(launches_ms, 4), "workspace_mib": round(get_engine(0).workspace_bytes() / 2 ** 20, 1)}), flush=True)


if __name__ == "__main__":
    main()
