#!/usr/bin/env python3
"""Golden vectors from the REFERENCE itself for its non-blind functions with a kernel of the caller's (this container only;
same import recipe as make_golden_big_taper.py): inverse_filtering_rank3 (deblurring.py:211-239), filters.convolve2d
(filters.py:14-37) and edgetaper.edgetaper (edgetaper.py:26-33) with dense kernels that are not point-symmetric -- square and
rectangular, odd and even, up to 49 x 49.

    python tests/golden/make_golden_nonblind.py

writes tests/golden/nonblind.npz (the image, the kernels, every inverse-filter output), nonblind_conv.npz and
nonblind_taper.npz (convolve2d / edgetaper on the replicate-padded image: three files so that each stays below 1 MiB), and
prints how far the oracle (oracle/polyblur_ref.py) is from the reference on each -- two independent fp32 evaluations.
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
from polyblur import edgetaper as ref_edgetaper, filters as ref_filters  # noqa: E402
from polyblur.deblurring import inverse_filtering_rank3  # noqa: E402
from polyblur_amd.synthetic import synthetic_blurry_batch  # noqa: E402
from oracle import polyblur_ref as oracle  # noqa: E402

SHAPES = [(49, 49), (26, 26), (3, 49), (25, 24)]
STAGE_SHAPES = [(49, 49), (3, 49)]
ALPHA, BETA = 2, 3


def make_kernel(shape, seed):
    k = np.random.default_rng(seed).random((1, 1) + tuple(shape)) ** 3
    return (k / k.sum()).astype(np.float32)


def ref_inverse(x, k, **kw):
    return inverse_filtering_rank3(torch.from_numpy(x.copy()), torch.from_numpy(k.copy()), alpha=ALPHA, b=BETA, **kw).numpy()


def main():
    x0, _ = synthetic_blurry_batch(1, 3, 50, 70, seed0=7100)
    x = (0.3 + 0.4 * x0).astype(np.float32)          # (keeps the final clamp out of the comparison)
    inv, conv, taper = {"x": x}, {}, {}
    worst = {"inverse": 0.0, "convolve2d": 0.0, "edgetaper": 0.0}
    clamp = 0.0

    def note(kind, got, want):
        worst[kind] = max(worst[kind], float(np.abs(got - want).max()))

    def note_clamp(o):
        nonlocal clamp
        clamp = max(clamp, float(np.mean((o == 0) | (o == 1))))

    for i, (h, w) in enumerate(SHAPES):
        k = make_kernel((h, w), 7200 + i)
        inv["k_%dx%d" % (h, w)] = k
        for method in ("fft", "direct"):
            for tag, kw in (("plain", {}), ("full", dict(do_edgetaper=True, remove_halo=True))):
                y = ref_inverse(x, k, method=method, **kw)
                inv["inv_%dx%d_%s_%s" % (h, w, method, tag)] = y
                o = oracle.inverse_filtering_rank3(x, k, ALPHA, BETA, method=method, **kw)
                note("inverse", o, y)
                note_clamp(o)
    # correlate=True: rot90(kernel, 2) first (deblurring.py:225-226)
    k = inv["k_25x24"]
    inv["inv_correlate_25x24_fft"] = ref_inverse(x, k, method="fft", correlate=True)
    o = oracle.inverse_filtering_rank3(x, np.ascontiguousarray(k[..., ::-1, ::-1]), ALPHA, BETA, method="fft")
    note("inverse", o, inv["inv_correlate_25x24_fft"])
    note_clamp(o)
    # one kernel per colour plane, 'fft' (under 'direct' the reference itself fails for these, filters.py:45-49), with halo
    # masking and without the edgetaper: edgetaper_alpha divides by torch.max(z) over ALL planes (edgetaper.py:15), the engine
    # and the oracle by each plane's own maximum
    kc = np.concatenate([make_kernel((15, 15), 7204 + c) for c in range(3)], axis=1)
    inv["k_perchannel_15x15"] = kc
    inv["inv_perchannel_15x15_fft_halo"] = ref_inverse(x, kc, method="fft", remove_halo=True)
    o = np.concatenate([oracle.inverse_filtering_rank3(x[:, c:c + 1], kc[:, c:c + 1], ALPHA, BETA, method="fft", remove_halo=True)
                        for c in range(3)], axis=1)
    note("inverse", o, inv["inv_perchannel_15x15_fft_halo"])
    note_clamp(o)
    # the two stages on the replicate-padded image
    for (h, w) in STAGE_SHAPES:
        k = inv["k_%dx%d" % (h, w)]
        xp = oracle.replicate_pad(x, w // 2)
        for method in ("fft", "direct"):
            name = "%dx%d_%s" % (h, w, method)
            conv["conv_" + name] = ref_filters.convolve2d(torch.from_numpy(xp.copy()), torch.from_numpy(k.copy()), method=method).numpy()
            taper["taper_" + name] = ref_edgetaper.edgetaper(torch.from_numpy(xp.copy()), torch.from_numpy(k.copy()), method=method).numpy()
            note("convolve2d", oracle.convolve2d(xp, k, method=method), conv["conv_" + name])
            note("edgetaper", oracle.edgetaper(xp, k, method=method), taper["taper_" + name])
    for fname, d in (("nonblind.npz", inv), ("nonblind_conv.npz", conv), ("nonblind_taper.npz", taper)):
        path = os.path.join(HERE, fname)
        np.savez_compressed(path, **d)
        print(fname, os.path.getsize(path), "bytes", {k: v.shape for k, v in d.items()})
    print("oracle vs reference, max abs difference:", worst)
    print("oracle outputs at exactly 0 or 1, worst case: %.2f %%" % (100 * clamp))


if __name__ == "__main__":
    main()
