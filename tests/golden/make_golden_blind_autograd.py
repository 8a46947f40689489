#!/usr/bin/env python3
"""Golden gradients of the BLIND path from the reference's own autograd (this container only; same import recipe as
make_golden_autograd.py): blur_estimation.gaussian_blur_estimation (blur_estimation.py:18-79) and polyblur_deblurring
(deblurring.py:23-96), differentiated with respect to the image.

    python tests/golden/make_golden_blind_autograd.py

writes tests/golden/blind_grad.npz: per case the input x and the weights w (float32 values), the reference's x.grad, and `cases`,
the JSON list of what each case is.

These are the reference's FLOAT32 gradients: its estimation does not run in float64 (cubic_interpolator multiplies a float32
matrix with the magnitudes: "expected scalar type Float but found Double"), so the goldens carry the reference's own float32
error; tests/test_blind_autograd_cpu.py measures the float64 restatement (tests/estimation_grad_ref.py) against them.

  * estimation-only cases: loss = sum(w * kernel), q = 0, the function's defaults (c = 0.362, b = 0.464, ker_size = 25);
  * blind cases: loss = sum(w * polyblur_deblurring(x, n_iter, alpha, beta, q = 0, method)), the driver's defaults otherwise;
    'direct' with B = 1, the only 'direct' form the reference runs (filters.py:45-49).

Inputs: uniform noise blurred by an oblique Gaussian and scaled into [0.05, 0.95] (estimation_grad_ref.blurred_noise).  The seed
is searched until, at every iteration's input and in float64 (the restatement's forward): every directional maximum lies at least
1e-3 (relative) above its runner-up, the two smallest and the two largest gray values differ by at least 1e-3 of the range, the
two smallest interpolated magnitudes differ by at least 1e-3 (relative), sigma^2 and rho^2 lie at least 1 % away from 0.09 and 16,
and no unclamped output lies within 1e-3 of 0 or 1 -- no evaluation within these margins of the float64 one then picks another
pixel, direction or clamp state.  `want` asks for a clamp state of (sigma, rho) in the first iteration of every image of a case."""
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
from polyblur import blur_estimation as ref_estimation  # noqa: E402
from polyblur.deblurring import polyblur_deblurring  # noqa: E402
import autograd_ref as ar  # noqa: E402
import estimation_grad_ref as er  # noqa: E402

FREE, UNCLAMPED, RHO_LOW = None, (False, False), (False, True)
# (shape, blur of the input (sigma along, across), clamp state asked for)
ESTIMATION = [
    ((1, 1, 16, 24), (2.2, 1.1), FREE),
    ((2, 3, 37, 45), (2.2, 1.1), UNCLAMPED),
    ((2, 3, 40, 48), (2.4, 0.25), RHO_LOW),
    ((1, 3, 64, 56), (1.8, 1.0), UNCLAMPED),
]
# (shape, blur, clamp state, n_iter, alpha, beta, method): small images -- the margin of the clamp has to hold for every sample of
# every iteration's output, which a seed meets the more rarely the more samples there are; three channels -- a clipped one-channel
# image has ties at both ends of its range from the second iteration on
BLIND = [
    ((2, 3, 20, 24), (2.2, 1.1), UNCLAMPED, 1, 6, 1, "fft"),
    ((1, 3, 18, 22), (2.2, 1.1), FREE, 2, 6, 1, "fft"),
    ((1, 3, 14, 16), (2.2, 1.1), FREE, 3, 6, 1, "fft"),
    ((2, 3, 20, 24), (2.4, 0.25), RHO_LOW, 1, 2, 3, "fft"),
    ((1, 3, 18, 22), (2.2, 1.1), FREE, 2, 2, 3, "fft"),
    ((1, 3, 14, 16), (2.2, 1.1), FREE, 3, 2, 3, "fft"),
    ((1, 3, 18, 22), (2.2, 1.1), FREE, 2, 6, 1, "direct"),
]


def state_ok(recs, want):
    return want is None or all(fl == want for fl in er.margins(recs)[4])


def main():
    out, cases = {}, []
    for n, (shape, sig, want) in enumerate(ESTIMATION):
        seed = 7000 + 100 * n
        while True:
            x = er.blurred_noise(seed, shape, sig)
            recs = er.estimate(x)
            if er.case_ok(recs) and state_ok(recs, want):
                break
            seed += 1
        w = np.random.default_rng(seed + 50).uniform(-1, 1, (shape[0], 1, 25, 25)).astype(np.float32)
        xt = torch.tensor(x, requires_grad=True)
        k = ref_estimation.gaussian_blur_estimation(xt, q=0.0)
        (k * torch.tensor(w)).sum().backward()
        name = "e%02d" % n
        cases.append(dict(name=name, kind="estimation", seed=seed, sig=list(sig), clamped=[list(f) for f in er.margins(recs)[4]]))
        out.update({name + "_x": x, name + "_w": w, name + "_gx": xt.grad.numpy()})
        print(name, shape, "seed", seed, "clamped (sigma, rho):", er.margins(recs)[4], "|gx| %.3g" % np.abs(xt.grad.numpy()).max(),
              "restatement off by %.3g" % np.abs(er.estimate_backward(recs, grad_kernel=w) - xt.grad.numpy()).max())
    for n, (shape, sig, want, n_iter, alpha, beta, method) in enumerate(BLIND):
        seed = 8000 + 1000 * n
        while True:
            x = er.blurred_noise(seed, shape, sig)
            steps, xi = [], np.asarray(x, np.float64)
            for it in range(n_iter):                         # (er.blind, leaving at the first iteration that misses a margin)
                recs = er.estimate(xi, 0.352, 0.768)
                if not er.case_ok(recs) or (it == 0 and not state_ok(recs, want)):
                    break
                yu = ar.rank3_unclamped(torch.tensor(xi), torch.tensor(er.kernels(recs)), alpha, beta, method).numpy()
                if ar.clamp_margin(yu)[0] <= 1e-3:
                    break
                steps.append((xi, recs, yu))
                xi = np.clip(yu, 0.0, 1.0)
            if len(steps) == n_iter:
                break
            seed += 1
        w = np.random.default_rng(seed + 50).uniform(-1, 1, shape).astype(np.float32)
        xt = torch.tensor(x, requires_grad=True)
        y = polyblur_deblurring(xt, n_iter=n_iter, alpha=alpha, beta=beta, q=0.0, method=method)
        (y * torch.tensor(w)).sum().backward()
        name = "b%02d" % n
        flags = [[list(f) for f in er.margins(recs)[4]] for _, recs, _ in steps]
        cases.append(dict(name=name, kind="blind", seed=seed, sig=list(sig), n_iter=n_iter, alpha=alpha, beta=beta, method=method, clamped=flags))
        out.update({name + "_x": x, name + "_w": w, name + "_gx": xt.grad.numpy()})
        g = er.blind_gradient(x, w, n_iter, alpha, beta, method, steps=steps)
        print(name, shape, method, "n_iter", n_iter, "seed", seed, "clamped:", flags, "|gx| %.3g" % np.abs(xt.grad.numpy()).max(),
              "restatement off by %.3g" % np.abs(g - xt.grad.numpy()).max())
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "blind_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
