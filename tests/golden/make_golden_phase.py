#!/usr/bin/env python3
"""Golden vectors from the REFERENCE itself for the pure-phase filter of its Fourier polynomial (this container only; same
import recipe as make_golden_nonblind.py): deblurring.compute_polynomial(method='fft', not_symmetric=True)
(deblurring.py:113-169), alone on the replicate-padded image and inside inverse_filtering_rank3's chain (deblurring.py:211-239),
which the reference never calls with the flag -- the chain is composed here from the reference's own functions:

    utils.pad_with_kernel -> [edgetaper.edgetaper(method='fft')] -> compute_polynomial(method='fft', not_symmetric=True)
    -> utils.crop_with_kernel -> [halo_masking, grad_img=None] -> clamp

    python tests/golden/make_golden_phase.py

reads the image and the kernels of tests/golden/nonblind.npz and writes tests/golden/nonblind_phase.npz (outputs only), and
prints how far the plain polynomial is from the phase-corrected one, how far an fp64 evaluation is from the reference's fp32 one,
the clamped share and min |K| of every case.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sk = types.ModuleType("skimage")
sk.img_as_float32 = lambda x: np.asarray(x, np.float32) / (255.0 if np.asarray(x).dtype == np.uint8 else 1.0)
sys.modules["skimage"] = sk
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")
sys.path.insert(0, REPO)

import torch  # noqa: E402

torch.set_num_threads(8)
from polyblur import edgetaper as ref_edgetaper, filters as ref_filters, utils as ref_utils  # noqa: E402
from polyblur.deblurring import compute_polynomial, halo_masking  # noqa: E402

SHAPES = ["49x49", "26x26", "3x49", "25x24"]


def chain(x, k, alpha, b, correlate=False, full=False, halo=False, dtype=torch.float32):
    img, kernel = torch.from_numpy(x.copy()).to(dtype), torch.from_numpy(k.copy()).to(dtype)
    if correlate:
        kernel = torch.rot90(kernel, k=2, dims=(-2, -1))
    img = ref_utils.pad_with_kernel(img, kernel)
    if full:
        img = ref_edgetaper.edgetaper(img, kernel, method="fft")
    imout = compute_polynomial(img, kernel, alpha, b, method="fft", not_symmetric=True)
    imout = ref_utils.crop_with_kernel(imout, kernel)
    if full or halo:
        imout = halo_masking(ref_utils.crop_with_kernel(img, kernel), imout, None)
    return torch.clamp(imout, 0.0, 1.0).numpy()


def main():
    d = np.load(os.path.join(HERE, "nonblind.npz"))
    x = d["x"]
    out = {}
    stats = []

    def add(name, k, alpha, b, **kw):
        y = chain(x, k, alpha, b, **kw)
        out[name] = y
        y64 = chain(x, k, alpha, b, dtype=torch.float64, **kw)
        K = ref_filters.p2o(torch.from_numpy(k.copy()), (x.shape[-2] + 2 * (k.shape[-1] // 2), x.shape[-1] + 2 * (k.shape[-1] // 2)))
        stats.append((name, float(np.abs(y - y64).max()), float(np.mean((y == 0) | (y == 1))), float(torch.abs(K).min())))

    for s in SHAPES:
        k = d["k_" + s]
        add("phase_%s_plain_a2b3" % s, k, 2, 3)
        add("phase_%s_full_a2b3" % s, k, 2, 3, full=True)
    for s in ("49x49", "25x24"):
        add("phase_%s_plain_a6b1" % s, d["k_" + s], 6, 1)
    add("phase_correlate_25x24_a2b3", d["k_25x24"], 2, 3, correlate=True)
    add("phase_perchannel_15x15_halo_a2b3", d["k_perchannel_15x15"], 2, 3, halo=True)
    # compute_polynomial on the replicate-padded image, unclamped
    shift = []
    for s, flags in (("25x24", ((True, "fft"), (False, "fft"), (False, "direct"))), ("3x49", ((True, "fft"),))):
        k = d["k_" + s]
        xp = ref_utils.pad_with_kernel(torch.from_numpy(x.copy()), torch.from_numpy(k.copy()))
        for ns, method in flags:
            y = compute_polynomial(xp, torch.from_numpy(k.copy()), 2, 3, method=method, not_symmetric=ns).numpy()
            out["poly_%s_%s_%s" % (s, method, "ns" if ns else "sym")] = y
        if len(flags) > 1:
            shift.append((s, float(np.abs(out["poly_%s_fft_ns" % s] - out["poly_%s_fft_sym" % s]).max())))
    path = os.path.join(HERE, "nonblind_phase.npz")
    np.savez_compressed(path, **out)
    print("nonblind_phase.npz", os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})
    for name, e64, clamped, kmin in stats:
        print("%-36s fp32 vs fp64 %.2e  clamped %.2f %%  min|K| %.2e" % (name, e64, 100 * clamped, kmin))
    print("phase-corrected vs plain polynomial, max abs:", shift)


if __name__ == "__main__":
    main()
