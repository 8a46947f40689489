#!/usr/bin/env python3
"""Golden gradients from the REFERENCE's own autograd (this container only; same import recipe as make_golden_nonblind.py):
filters.convolve2d (filters.py:14-37), deblurring.compute_polynomial (deblurring.py:113-169) and inverse_filtering_rank3
(deblurring.py:211-239), differentiated in float64 with respect to the image and to the kernel for loss = sum(w * y).

    python tests/golden/make_golden_autograd.py

writes tests/golden/nonblind_grad.npz: per case the inputs x, k and the weight image w (float32 values), the reference's
x.grad and kernel.grad (float64), and `cases`, the JSON list of what each case is.

What is in and what is left out:
  * 'fft' cases take (B,1,h,w), (B,C,h,w) and (1,1,h,w) kernels; 'direct' cases take B = 1 with a (1,1,h,w) kernel only -- the
    reference's F.conv2d wrapper fails for per-image and per-plane kernels there (filters.py:45-49).
  * convolve2d(method='fft') with a kernel taller than wide is no circular convolution over the domain in the reference
    (filters.py:33): no such case.
  * Every case differentiated; none had to be dropped.
The images are i.i.d. uniform noise (a lag off by one sample then changes every tap gradient by far more than any tolerance),
the kernels rng.random ** 3 normalised -- dense, not point-symmetric.  For the inverse_filtering_rank3 cases the seed is searched
until no unclamped float64 output lies within 1e-3 of 0 or 1 and at least 5 % of the samples are clamped: the clamp's mask is then
the same for any evaluation within 50 x the project's forward tolerance."""
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
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

torch.set_num_threads(8)
from polyblur import filters as ref_filters  # noqa: E402
from polyblur.deblurring import compute_polynomial, inverse_filtering_rank3  # noqa: E402
import autograd_ref as ar  # noqa: E402

# (func, method, image shape, kernel shape, alpha, b, correlate)
CASES = [
    ("convolve2d", "fft", (2, 3, 24, 28), (2, 1, 5, 9), 0, 0, False),
    ("polynomial", "fft", (2, 3, 24, 28), (2, 1, 5, 9), 2, 3, False),
    ("rank3", "fft", (2, 3, 12, 14), (2, 1, 5, 9), 6, 1, False),
    ("convolve2d", "fft", (2, 3, 24, 28), (2, 3, 3, 3), 0, 0, False),
    ("polynomial", "fft", (2, 3, 24, 28), (2, 3, 3, 3), 6, 1, False),
    ("rank3", "fft", (2, 3, 12, 14), (2, 3, 3, 3), 6, 1, False),
    ("convolve2d", "fft", (2, 1, 40, 44), (1, 1, 25, 25), 0, 0, False),
    ("polynomial", "fft", (2, 1, 40, 44), (1, 1, 25, 25), 6, 1, False),
    ("rank3", "fft", (2, 1, 18, 20), (1, 1, 25, 25), 6, 1, False),
    ("rank3", "fft", (2, 1, 18, 20), (1, 1, 25, 25), 2, 3, True),
    ("convolve2d", "fft", (1, 1, 64, 72), (1, 1, 49, 49), 0, 0, False),
    ("polynomial", "fft", (1, 1, 64, 72), (1, 1, 49, 49), 2, 3, False),
    ("rank3", "fft", (1, 2, 16, 20), (1, 1, 49, 49), 6, 1, False),
    ("convolve2d", "direct", (1, 3, 24, 28), (1, 1, 5, 9), 0, 0, False),
    ("polynomial", "direct", (1, 3, 24, 28), (1, 1, 5, 9), 6, 1, False),
    ("rank3", "direct", (1, 3, 12, 14), (1, 1, 5, 9), 6, 1, False),
    ("rank3", "direct", (1, 3, 12, 14), (1, 1, 3, 3), 6, 1, True),
    ("polynomial", "direct", (1, 1, 40, 44), (1, 1, 25, 25), 2, 3, False),
    ("rank3", "direct", (1, 1, 18, 20), (1, 1, 25, 25), 6, 1, False),
    ("rank3", "direct", (1, 1, 16, 20), (1, 1, 49, 49), 6, 1, False),
]


def inputs(seed, xshape, kshape):
    rng = np.random.default_rng(seed)
    x = rng.random(xshape).astype(np.float32)
    w = rng.uniform(-1, 1, xshape).astype(np.float32)
    k = rng.random(kshape) ** 3
    return x, w, (k / k.sum(axis=(-2, -1), keepdims=True)).astype(np.float32)


def clamp_margin(y):
    """(distance of the nearest unclamped value to 0 or 1, fraction of clamped samples)"""
    return float(np.minimum(np.abs(y), np.abs(y - 1)).min()), float(np.mean((y <= 0) | (y >= 1)))


def reference(func, method, x, k, w, alpha, b, correlate):
    xt = torch.tensor(x, dtype=torch.float64, requires_grad=True)
    kt = torch.tensor(k, dtype=torch.float64, requires_grad=True)
    if func == "convolve2d":
        y = ref_filters.convolve2d(xt, kt, method=method)
    elif func == "polynomial":
        y = compute_polynomial(xt, kt, alpha, b, method=method)
    else:
        y = inverse_filtering_rank3(xt, kt, alpha=alpha, b=b, correlate=correlate, method=method)
    (y * torch.tensor(w, dtype=torch.float64)).sum().backward()
    return y.detach().numpy(), xt.grad.numpy(), kt.grad.numpy()


def main():
    out, cases, worst = {}, [], [0.0, 0.0]
    for n, (func, method, xshape, kshape, alpha, b, correlate) in enumerate(CASES):
        seed = 9000 + 100 * n
        while True:
            x, w, k = inputs(seed, xshape, kshape)
            if func != "rank3":
                break
            yu = ar.rank3_unclamped(torch.tensor(x, dtype=torch.float64), torch.tensor(k, dtype=torch.float64), alpha, b, method, correlate).numpy()
            margin, clamped = clamp_margin(yu)
            if margin > 1e-3 and clamped >= 0.05:
                break
            seed += 1
        y, gx, gk = reference(func, method, x, k, w, alpha, b, correlate)
        _, rx, rk = ar.gradients(func, x, k, w, alpha, b, method, correlate)
        worst = [max(worst[0], float(np.abs(rx - gx).max())), max(worst[1], float(np.abs(rk - gk).max()))]
        name = "c%02d" % n
        cases.append(dict(name=name, func=func, method=method, alpha=alpha, b=b, correlate=bool(correlate), seed=seed))
        out.update({name + "_x": x, name + "_w": w, name + "_k": k, name + "_gx": gx, name + "_gk": gk})
        print(name, func, method, xshape, kshape, "seed", seed, "|gx| %.3g |gk| %.3g" % (np.abs(gx).max(), np.abs(gk).max()),
              ("clamped %.1f %% margin %.2g" % (100 * clamped, margin)) if func == "rank3" else "")
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "nonblind_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")
    print("restatement (tests/autograd_ref.py) vs reference, max abs difference: grad_x %.3g, grad_k %.3g" % tuple(worst))


if __name__ == "__main__":
    main()
