#!/usr/bin/env python3
"""Golden vectors from the REFERENCE itself for the blur estimation with direction counts other than 6 x 30, quantiles and the
saturation mask, on the planted inputs of tests/estimation_ref.py (this container only; same import recipe as
make_golden_halo.py): blur_estimation.gaussian_blur_estimation (blur_estimation.py:18-79) with the grids built as the blind driver
builds them (deblurring.py:62-63: both truncated to whole degrees).

    python tests/golden/make_golden_estimation.py

writes tests/golden/estimation_planted.npz (inputs, options, kernel, sigma / rho / theta) and prints how far the fp32 oracle and
the float64 restatement are from the reference.  The reference's `return_2d_filters=False` branch raises NameError
(blur_estimation.py:77 names `theta`, which does not exist), so sigma / rho / theta are taken from the same sub-routines in the
order of the function's body (:59-70) and checked against the kernel the function itself returns.
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
from polyblur import blur_estimation as be  # noqa: E402
from oracle import polyblur_ref as oracle  # noqa: E402
import estimation_ref as er  # noqa: E402


def reference(x, o):
    """-> kernel (B,1,k,k), sigma, rho, theta (B,)"""
    img = torch.from_numpy(np.array(x, np.float32))
    thetas = torch.linspace(0, 180, o["n_angles"] + 1).unsqueeze(0).long()                      # deblurring.py:62-63
    interp = torch.arange(0, 180, 180 / o["n_interp"]).unsqueeze(0).long()
    kernel = be.gaussian_blur_estimation(img, q=o["q"], n_angles=o["n_angles"], n_interpolated_angles=o["n_interp"], c=o["c"],
                                         b=o["b"], ker_size=25, discard_saturation=o["discard_saturation"], thetas=thetas,
                                         interpolated_thetas=interp)
    gray = img.mean(dim=1, keepdims=True)
    mask = be.get_saturation_mask(gray, o["discard_saturation"])
    grads = be.compute_gradients(be.normalize(gray, q=o["q"]), mask=mask)
    mags = be.compute_gradient_magnitudes(grads, n_angles=o["n_angles"])
    m_n, m_o, th = be.find_maximal_blur_direction(mags, thetas, interp)
    sigma, rho = be.compute_gaussian_parameters(m_n, m_o, c=o["c"], b=o["b"])
    again = be.create_gaussian_filter(th, sigma, rho, ksize=25)
    assert torch.equal(again, kernel)
    return kernel.numpy(), sigma.numpy().reshape(-1), rho.numpy().reshape(-1), th.numpy().reshape(-1).astype(np.float32)


def main():
    out = {}
    worst = {"oracle": {}, "float64": {}}
    for name, case in er.golden_cases():
        x, o = er.image(case), case.opts
        x32 = x.astype(np.float32) * np.float32(1.0 / 255.0) if x.dtype == np.uint8 else x.astype(np.float32)
        kernel, sigma, rho, theta = reference(x32, o)
        out[name + "_x"] = x
        out[name + "_opts"] = np.array([o["n_angles"], o["n_interp"], o["q"], float(o["discard_saturation"]), o["c"], o["b"]], np.float64)
        out[name + "_kernel"], out[name + "_sigma"], out[name + "_rho"], out[name + "_theta"] = kernel, sigma, rho, theta
        k32, info = oracle.estimate_gaussian_blur(x32, c=o["c"], b=o["b"], q=o["q"], n_angles=o["n_angles"],
                                                  n_interpolated_angles=o["n_interp"], discard_saturation=o["discard_saturation"],
                                                  return_info=True)
        recs = er.run(case)
        for who, got in (("oracle", dict(kernel=k32, sigma=info["sigma"], rho=info["rho"], theta=info["theta"])),
                         ("float64", dict(kernel=np.stack([r["kernel"] for r in recs])[:, None], sigma=[r["sigma"] for r in recs],
                                          rho=[r["rho"] for r in recs], theta=[r["theta"] for r in recs]))):
            for f, want in (("kernel", kernel), ("sigma", sigma), ("rho", rho), ("theta", theta)):
                d = float(np.abs(np.asarray(got[f], np.float64) - want).max())
                worst[who][f] = max(worst[who].get(f, 0.0), d)
        print("%-44s sigma %s rho %s theta %s" % (name, sigma, rho, np.rad2deg(theta)))
    path = os.path.join(HERE, "estimation_planted.npz")
    np.savez_compressed(path, **out)
    print("estimation_planted.npz", os.path.getsize(path), "bytes,", len(out) // 6, "entries")
    print("against the reference, max abs difference:", worst)


if __name__ == "__main__":
    main()
