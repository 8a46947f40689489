#!/usr/bin/env python3
"""Golden gradients with respect to the four scalars of Polyblur -- alpha, beta, c, b -- from the reference's own autograd (this
container only; the import recipe of make_golden_blind_autograd.py): every one of them given as a torch.tensor(..., requires_grad=True).

    python tests/golden/make_golden_params_autograd.py

writes tests/golden/params_grad.npz: per case what the tests cannot form again bit for bit (the kernels of the polynomial cases, the
images and weights of the others), the reference's gradients, and `cases`, the JSON list of what each case is.

  * polynomial cases (params_grad_ref.POLY): deblurring.compute_polynomial and inverse_filtering_rank3 with loss = sum(w * out), in
    float64 (`_g64`) and in float32 (`_g32`): (d alpha, d beta).  Image and weights: params_grad_ref.smooth_image(seed); the seed is
    drawn until min(|d alpha|, |d beta|) >= 0.1 max(|d alpha|, |d beta|) in float64 (no case tests a near-zero scalar) and, for
    inverse_filtering_rank3, no unclamped float64 output lies within 1e-3 of 0 or 1;
  * estimation cases (params_grad_ref.ESTIMATION): gaussian_blur_estimation(q=0) with loss = sum(w * kernel): (d c, d b), float32 --
    the reference does not run this stage in float64 --, on estimation_grad_ref.blurred_noise with its seed search and margins and
    the clamp state asked for; the last case is unblurred noise on which both variances clamp: exactly (0, 0);
  * blind cases (make_golden_blind_autograd.BLIND's list): polyblur_deblurring with all four as tensors: (d c, d b, d alpha, d beta),
    float32, under the margins of make_golden_blind_autograd; and two more on the image of b01, n_iter = 2 with remove_halo=True
    (`h00`) and with edgetaping=True (`t00`).

Prints E, the reference's float32 error against the float64 truth relative to the case's larger gradient, per kind: what the
tolerances in tests/params_grad_ref.py are held to."""
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
sys.path.insert(0, HERE)

import torch  # noqa: E402

torch.set_num_threads(8)
from polyblur import blur_estimation as ref_estimation  # noqa: E402
from polyblur import deblurring as ref_deblurring  # noqa: E402
import autograd_ref as ar  # noqa: E402
import estimation_grad_ref as er  # noqa: E402
import params_grad_ref as pr  # noqa: E402
from make_golden_blind_autograd import BLIND, state_ok  # noqa: E402


def ref_poly(func, x, k, w, alpha, beta, method, dtype):
    xt, kt, wt = (torch.tensor(np.asarray(a), dtype=dtype) for a in (x, k, w))
    at, bt = torch.tensor(float(alpha), dtype=dtype, requires_grad=True), torch.tensor(float(beta), dtype=dtype, requires_grad=True)
    if func == "polynomial":
        y = ref_deblurring.compute_polynomial(xt, kt, at, bt, method=method)
    else:
        y = ref_deblurring.inverse_filtering_rank3(xt, kt, at, bt, method=method)
    (y * wt).sum().backward()
    return np.array([float(at.grad), float(bt.grad)])


def main():
    out, cases = {}, []
    e_poly = e_est = e_blind = 0.0
    for n, (func, xshape, kshape, kind, method, (alpha, beta)) in enumerate(pr.POLY):
        seed = 3000 + 100 * n
        k = pr.make_kernel(seed, kshape, kind)
        while True:
            x, w = pr.smooth_image(seed, xshape)
            g64 = ref_poly(func, x, k, w, alpha, beta, method, torch.float64)
            ok = np.abs(g64).min() >= 0.1 * np.abs(g64).max()
            if ok and func == "rank3":
                ok = ar.clamp_margin(ar.rank3_unclamped(torch.tensor(x, dtype=torch.float64), torch.tensor(k, dtype=torch.float64), alpha, beta, method).numpy())[0] > 1e-3
            if ok:
                break
            seed += 1
        g32 = ref_poly(func, x, k, w, alpha, beta, method, torch.float32)
        rows = (pr.poly_param_rows(x, k, w, method) if func == "polynomial" else pr.rank3_param_rows(x, k, w, alpha, beta, method)).sum(axis=0)
        name = "p%02d" % n
        cases.append(dict(name=name, kind="poly", func=func, xshape=list(xshape), kshape=list(kshape), kernel=kind, method=method,
                          alpha=alpha, beta=beta, seed=seed))
        out.update({name + "_k": k, name + "_g64": g64, name + "_g32": g32})
        e = pr.rel_error(g32, g64)
        e_poly = max(e_poly, e)
        print(name, func, xshape, kshape, kind, method, "seed", seed, "g64", g64, "E %.3g" % e, "restatement off by %.3g" % pr.rel_error(rows, g64))
    for n, (shape, sig, want) in enumerate(pr.ESTIMATION):
        seed = 7000 + 100 * n
        while True:
            x = pr.noise_image(seed, shape) if sig is None else er.blurred_noise(seed, shape, sig)
            recs = er.estimate(x)
            if er.case_ok(recs) and state_ok(recs, want):
                break
            seed += 1
        w = np.random.default_rng(seed + 50).uniform(-1, 1, (shape[0], 1, 25, 25)).astype(np.float32)
        ct, bt = torch.tensor(pr.EST_C, requires_grad=True), torch.tensor(pr.EST_B, requires_grad=True)
        kk = ref_estimation.gaussian_blur_estimation(torch.tensor(x), q=0.0, c=ct, b=bt)
        (kk * torch.tensor(w)).sum().backward()
        g32 = np.array([float(ct.grad), float(bt.grad)], np.float32)
        truth = pr.estimation_param_rows(recs, w).sum(axis=0)
        name = "e%02d" % n
        flags = [list(f) for f in er.margins(recs)[4]]
        cases.append(dict(name=name, kind="estimation", seed=seed, sig=None if sig is None else list(sig), clamped=flags))
        out.update({name + "_x": x, name + "_w": w, name + "_g32": g32})
        e = pr.rel_error(g32, truth) if np.abs(truth).max() > 0 else float(np.abs(g32).max())
        e_est = max(e_est, e)
        print(name, shape, "seed", seed, "clamped (sigma, rho):", flags, "g32", g32, "truth", truth, "E %.3g" % e)
    for n, (shape, sig, want, n_iter, alpha, beta, method) in enumerate(BLIND):
        seed = 8000 + 1000 * n
        while True:
            x = er.blurred_noise(seed, shape, sig)
            steps, xi = [], np.asarray(x, np.float64)
            for it in range(n_iter):
                recs = er.estimate(xi, pr.BLIND_C, pr.BLIND_B)
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
        ps = [torch.tensor(float(v), requires_grad=True) for v in (pr.BLIND_C, pr.BLIND_B, alpha, beta)]
        y = ref_deblurring.polyblur_deblurring(torch.tensor(x), n_iter=n_iter, c=ps[0], b=ps[1], alpha=ps[2], beta=ps[3], q=0.0, method=method)
        (y * torch.tensor(w)).sum().backward()
        g32 = np.array([float(p.grad) for p in ps], np.float32)
        truth = pr.blind_param_grads(x, w, n_iter, alpha, beta, method, steps=steps)
        name = "b%02d" % n
        flags = [[list(f) for f in er.margins(recs)[4]] for _, recs, _ in steps]
        cases.append(dict(name=name, kind="blind", seed=seed, sig=list(sig), n_iter=n_iter, alpha=alpha, beta=beta, method=method, clamped=flags))
        out.update({name + "_x": x, name + "_w": w, name + "_g32": g32})
        e = pr.rel_error(g32, truth)
        e_blind = max(e_blind, e)
        print(name, shape, method, "n_iter", n_iter, "seed", seed, "g32", g32, "truth", truth, "E %.3g" % e)
    # two iterations with the halo mask and with the edgetaper, on the image of b01 (the margins hold for its plain chain; the
    # restatement has neither stage, so these are checked against the reference alone)
    x, w = out["b01_x"], out["b01_w"]
    for name, extra in (("h00", dict(remove_halo=True)), ("t00", dict(edgetaping=True))):
        ps = [torch.tensor(float(v), requires_grad=True) for v in (pr.BLIND_C, pr.BLIND_B, 6, 1)]
        y = ref_deblurring.polyblur_deblurring(torch.tensor(x), n_iter=2, c=ps[0], b=ps[1], alpha=ps[2], beta=ps[3], q=0.0, method="fft", **extra)
        (y * torch.tensor(w)).sum().backward()
        g32 = np.array([float(p.grad) for p in ps], np.float32)
        cases.append(dict(name=name, kind="blind_extra", of="b01", n_iter=2, alpha=6, beta=1, method="fft", **extra))
        out[name + "_g32"] = g32
        print(name, extra, "g32", g32)
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "params_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")
    print("E: polynomial %.3g, estimation %.3g, blind %.3g" % (e_poly, e_est, e_blind))


if __name__ == "__main__":
    main()
