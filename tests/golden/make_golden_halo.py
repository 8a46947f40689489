#!/usr/bin/env python3
"""Golden vectors from the REFERENCE itself for halo masking on inputs where the mask has a strong effect (this container only;
same import recipe as make_golden_nonblind.py): halo_masking (deblurring.py:193-208) and inverse_filtering_rank3(...,
remove_halo=True, grad_img=...) (deblurring.py:211-239) with the sparse, reversed gradient planes of tests/halo_ref.py.

    python tests/golden/make_golden_halo.py

writes tests/golden/halo_strong.npz and prints, for every entry, how far the fp32 oracle and the float64 restatement
(tests/halo_ref.py) are from the reference, and that the gauge (halo_ref.power) holds.  The reference's 'direct' convolution
takes one kernel for a whole batch (filters.py:45-49), so batches go through it image by image.
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

torch.set_num_threads(8)
from polyblur.deblurring import halo_masking, inverse_filtering_rank3  # noqa: E402
from oracle import polyblur_ref as oracle  # noqa: E402
import halo_ref as hr  # noqa: E402


def t(a):
    return torch.from_numpy(np.array(a, np.float32))


def main():
    out = {}
    worst = {"oracle": 0.0, "float64": 0.0}

    def note(name, want, o32, o64, s):
        why = hr.power(s["want"], s["unmasked"], s["tol"], s["z"], s["pole"])
        assert why is None, (name, why)
        worst["oracle"] = max(worst["oracle"], float(np.abs(o32 - want).max()))
        worst["float64"] = max(worst["float64"], float(np.abs(o64 - want).max()))
        print("%-28s oracle %.3g  float64 %.3g  mask's effect %.3g" % (name, np.abs(o32 - want).max(), np.abs(o64 - want).max(),
                                                                      np.abs(s["want"] - s["unmasked"]).max()))

    for shape in hr.GOLDEN_SHAPES:
        tag = "w%d" % shape[-1]
        s = hr.stage_set(shape)
        for key in ("x", "gx", "gy"):
            out["%s_%s" % (tag, key)] = s[key]
        out[tag + "_y"] = s["y32"]
        want = halo_masking(t(s["x"]), t(s["y32"]), (t(s["gx"]), t(s["gy"]))).numpy()
        out[tag + "_halo"] = want
        note(tag + "_halo", want, oracle.halo_masking(s["x"], s["y32"], (s["gx"], s["gy"])), s["want"], dict(s, tol=hr.TOL_STAGE))

        x, k, gx, gy = hr.golden_inverse_inputs(shape)
        out[tag + "_image"], out[tag + "_k"], out[tag + "_igx"], out[tag + "_igy"] = x, k, gx, gy
        for method, taper in hr.GOLDEN_VARIANTS:
            name = "%s_inv_%s_%s" % (tag, method, "taper" if taper else "plain")
            want = np.concatenate([inverse_filtering_rank3(t(x[i:i + 1]), t(k[i:i + 1]), hr.ALPHA, hr.BETA, remove_halo=True,
                                                           grad_img=(t(gx[i:i + 1]), t(gy[i:i + 1])), do_edgetaper=taper,
                                                           method=method).numpy() for i in range(shape[0])])
            out[name] = want
            _, xc, y, _ = hr.chain_f64(x, k, taper, method)
            w64, z, pole = hr.halo_f64(xc, y, gx, gy, True, parts=True)
            o32 = oracle.inverse_filtering_rank3(x, k, hr.ALPHA, hr.BETA, remove_halo=True, grad_img=(gx, gy), do_edgetaper=taper,
                                                 method=method)
            note(name, want, o32, w64, dict(want=w64, unmasked=np.clip(y, 0, 1), z=z, pole=pole, tol=hr.TOL_INV))
    path = os.path.join(HERE, "halo_strong.npz")
    np.savez_compressed(path, **out)
    print("halo_strong.npz", os.path.getsize(path), "bytes", {k: v.shape for k, v in out.items()})
    print("against the reference, max abs difference:", worst)


if __name__ == "__main__":
    main()
