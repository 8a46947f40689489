#!/usr/bin/env python3
"""Golden gradients of the blind path with prefiltering=True from the reference's own autograd (this container only; same import
recipe as make_golden_blind_autograd.py): polyblur_deblurring (deblurring.py:23-96) with the bilateral split of every iteration
(:80-84, :99-110), with and without remove_halo, differentiated with respect to the image.

    python tests/golden/make_golden_prefilter_autograd.py

writes tests/golden/prefilter_grad.npz: per case the input x and the weights w (float32 values), the reference's x.grad, and
`cases`, the JSON list of what each case is.  Data only.

These are the reference's FLOAT32 gradients (its estimation does not run in float64); tests/test_bilateral_autograd_cpu.py measures
the float64 restatement (tests/bilateral_grad_ref.py: blind_gradient) against them.

One function of the reference is replaced while this script runs: filters.bilateral_filter itself cannot be differentiated by
torch -- it scales the result of torch.exp in place (filters.py:136-138, "F *= gw[y]..."), and the backward of exp needs that
result ("one of the variables needed for gradient computation has been modified by an inplace operation") -- so
polyblur.filters.bilateral_filter is bound to tests/bilateral_grad_ref.forward for the length of the run: the same formula with the
product written out of place, in float32.  Everything else -- the estimation, the non-blind step, the mask, the driver's order of
the steps and the noise it adds back -- is the reference's own code under its own autograd.

loss = sum(w * polyblur_deblurring(x, n_iter, c, b, alpha, beta, q = 0, remove_halo, prefiltering=True, method='fft')), the
options bilateral_grad_ref.PLAIN_KW without the mask and HALO_KW with it.  Inputs: blurred noise (without the mask) or halo_ref's
line image (with it) plus noise of 0.01.  The seed is searched, as make_golden_blind_autograd.py searches its own, until at every
iteration's input and in float64 the margins of that script hold -- arg-max runner-up, range ends, clamp states of sigma and rho,
no unclamped output within 1e-3 of 0 or 1 -- and, with the mask, the kink band of tests/halo_grad_ref.py is empty."""
import json
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
from polyblur import filters as ref_filters  # noqa: E402
from polyblur.deblurring import polyblur_deblurring  # noqa: E402
import bilateral_grad_ref as bg  # noqa: E402

ref_filters.bilateral_filter = bg.forward                    # (the module docstring: the in-place product)


def main():
    out, cases = {}, []
    for n, (shape, n_iter, halo) in enumerate(bg.GOLDEN_BLIND):
        c = bg.blind_case(shape, n_iter, halo)
        x, w = c["x"], c["w"]
        xt = torch.tensor(x, requires_grad=True)
        y = polyblur_deblurring(xt, n_iter=n_iter, q=0.0, remove_halo=halo, prefiltering=True, method="fft", **bg.blind_kw(halo))
        (y * torch.tensor(w)).sum().backward()
        name = "p%02d" % n
        cases.append(dict(name=name, kind="blind", shape=list(shape), n_iter=n_iter, remove_halo=halo, seed=c["seed"]))
        out.update({name + "_x": x, name + "_w": w, name + "_dx": xt.grad.numpy()})
        g = bg.blind_gradient(x, w, n_iter, halo, steps=c["steps"])
        plain = bg.blind_gradient(x, w, n_iter, halo, steps=c["steps"], mutant="smooth detached")
        print(name, shape, "n_iter", n_iter, "remove_halo", halo, "seed", c["seed"], "|gx| %.3g" % np.abs(g).max(),
              "restatement off by %.3g of max" % (np.abs(g - xt.grad.numpy()).max() / np.abs(g).max()),
              "| the filter taken for a constant: off by %.3g of max" % (np.abs(plain - g).max() / np.abs(g).max()))
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "prefilter_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
