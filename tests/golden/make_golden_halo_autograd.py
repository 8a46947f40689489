#!/usr/bin/env python3
"""Golden gradients of halo masking from the reference's own autograd (this container only; same import recipe as
make_golden_blind_autograd.py): deblurring.halo_masking (deblurring.py:193-208), inverse_filtering_rank3(remove_halo=True)
(:211-239) and polyblur_deblurring(remove_halo=True) (:23-96).

    python tests/golden/make_golden_halo_autograd.py

writes tests/golden/halo_grad.npz: per case the inputs (float32 values), the upstream weights and the reference's gradients, and
`cases`, the JSON list of what each case is.

  * stage cases (float64): loss = sum(g * halo_masking(x, y, (gx, gy))), gradients of all four inputs, on four small sets of
    tests/halo_grad_ref.py (halo_ref.stage_set, kink band repaired);
  * chain cases (float64): loss = sum(w * inverse_filtering_rank3(x, k, alpha, beta, remove_halo=True, grad_img, method)) -- built
    (reversed) gradients, and grad_img=None on halo_ref's line image with beta < 0, where the image's own gradients make the mask
    act; 'fft' with B = 2, 'direct' with B = 1, the only 'direct' form the reference runs (filters.py:45-49); image and kernel
    gradients, and grad_img's where given;
  * blind cases (FLOAT32: the reference's estimation does not run in float64): loss = sum(w * polyblur_deblurring(x,
    **halo_ref.PIPE_KW, n_iter)), the line image plus noise of 0.01.

The seeds of the chain and blind cases are searched until, in float64 (the restatement's forward), no unclamped output lies within
1e-3 of 0 or 1, the kink band of tests/halo_grad_ref.py is empty and -- blind cases, at every iteration -- the margins of
make_golden_blind_autograd.py hold (arg-max runner-up, range ends, clamp states of sigma and rho) and the mask moves the gradient by
50 of the GPU test's tolerances on 6 % of every plane's samples (halo_grad_ref.blind_moved)."""
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
from polyblur.deblurring import halo_masking, inverse_filtering_rank3, polyblur_deblurring  # noqa: E402
import halo_grad_ref as hg  # noqa: E402
import halo_ref as hr  # noqa: E402

F32, F64 = np.float32, np.float64


def t64(a, grad=True):
    return torch.tensor(np.asarray(a, F64), requires_grad=grad)


def main():
    out, cases = {}, []
    for n, (shape, zeros) in enumerate(hg.GOLDEN_STAGE):
        s = hg.repaired_set(shape, zeros)
        ts = [t64(s[k]) for k in hg.NAMES]
        halo_masking(ts[0], ts[1], (ts[2], ts[3])).backward(t64(s["g"], False))
        name = "s%02d" % n
        cases.append(dict(name=name, kind="stage", shape=list(shape), zeros=bool(zeros)))
        for k, t in zip(hg.NAMES, ts):
            out[name + "_" + k] = s[k]
            out[name + "_d" + k] = t.grad.numpy()
        out[name + "_g"] = s["g"]
        print(name, shape, "restatement off by", max(hg.plane_error(s["want"][k], t.grad.numpy()) for k, t in zip(hg.NAMES, ts)))
    for n, (shape, kshape, method, own) in enumerate(hg.GOLDEN_CHAIN):
        c = hg.chain_case(shape, kshape, method, own, seed=None)
        x, k, w, grad_img = c["x"], c["k"], c["w"], c["grad_img"]
        xt, kt = t64(x), t64(k)
        gs = None if own else (t64(grad_img[0]), t64(grad_img[1]))
        y = inverse_filtering_rank3(xt, kt, c["alpha"], c["beta"], remove_halo=True, grad_img=gs, method=method)
        (y * t64(w, False)).sum().backward()
        name = "c%02d" % n
        cases.append(dict(name=name, kind="chain", shape=list(shape), kshape=list(kshape), method=method, own=bool(own), seed=c["seed"],
                          alpha=c["alpha"], beta=c["beta"]))
        out.update({name + "_x": x, name + "_k": k, name + "_w": w, name + "_dx": xt.grad.numpy(), name + "_dk": kt.grad.numpy()})
        if not own:
            out.update({name + "_gx": grad_img[0], name + "_gy": grad_img[1], name + "_dgx": gs[0].grad.numpy(), name + "_dgy": gs[1].grad.numpy()})
        _, want = hg.chain_gradients(x, k, grad_img, w, c["alpha"], c["beta"], method)
        print(name, shape, method, "own" if own else "built", "seed", c["seed"], "restatement off by %.3g" % hg.plane_error(want["x"], xt.grad.numpy()))
    for n, (shape, n_iter) in enumerate(hg.GOLDEN_BLIND):
        c = hg.blind_case(shape, n_iter, seed=None)
        x, w = c["x"], c["w"]
        xt = torch.tensor(x, requires_grad=True)
        kw = dict(hr.PIPE_KW, n_iter=n_iter)
        y = polyblur_deblurring(xt, q=0.0, method="fft", **kw)
        (y * torch.tensor(w)).sum().backward()
        name = "b%02d" % n
        cases.append(dict(name=name, kind="blind", shape=list(shape), n_iter=n_iter, seed=c["seed"]))
        out.update({name + "_x": x, name + "_w": w, name + "_dx": xt.grad.numpy()})
        g = hg.blind_gradient(x, w, n_iter, hr.PIPE_KW, steps=c["steps"])
        print(name, shape, "n_iter", n_iter, "seed", c["seed"], "|gx| %.3g" % np.abs(g).max(),
              "restatement off by %.3g of max" % (np.abs(g - xt.grad.numpy()).max() / np.abs(g).max()))
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "halo_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
