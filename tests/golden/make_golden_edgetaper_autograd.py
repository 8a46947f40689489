#!/usr/bin/env python3
"""Golden gradients of the edgetaper from the reference's own autograd (this container only; same import recipe as
make_golden_autograd.py): edgetaper.edgetaper (edgetaper.py:10-33), inverse_filtering_rank3(do_edgetaper=True) (deblurring.py:211-239)
and polyblur_deblurring(edgetaping=True) (deblurring.py:23-96).

    python tests/golden/make_golden_edgetaper_autograd.py [--search]

writes tests/golden/edgetaper_grad.npz: for every case of edgetaper_grad_ref.TAPER_CASES and CHAIN_CASES the reference's x.grad and
kernel.grad in float64 (`_dx`, `_dk`) and float32 (`_fx`, `_fk`) -- the inputs are built again by tests/edgetaper_grad_ref.py from
their seeds --; `E`, a JSON table: per case the reference's float32 error against its float64 gradients relative to the largest
float64 entry, how far the restatement is from the float64 gradients, the share of the taper weights' path in the largest tap
entry, and for chain cases the clamp margins; for the blind cases (float32 only: the reference's estimation does not run in float64,
make_golden_blind_autograd.py) x, w and x.grad, and `blind`, the JSON list of what each is.

The reference takes torch.max(z) over the whole kernel tensor, the engine per kernel: every case has a kernel batch of 1 (broadcast
over the images where B = 2), and the blind cases have B = 1.  --search: look for the chain cases' seeds again."""
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
from polyblur.deblurring import inverse_filtering_rank3, polyblur_deblurring  # noqa: E402
from polyblur.edgetaper import edgetaper  # noqa: E402
import edgetaper_grad_ref as eg  # noqa: E402
import estimation_grad_ref as er  # noqa: E402


def taper_gradients(c, dtype):
    x = torch.tensor(np.asarray(c["x"]), dtype=dtype, requires_grad=True)
    k = torch.tensor(np.asarray(c["k"]), dtype=dtype, requires_grad=True)
    y = edgetaper(x, k, n_tapers=c["n"], method=c["method"])
    (y * torch.tensor(np.asarray(c["w"]), dtype=dtype)).sum().backward()
    return {"x": x.grad.numpy(), "k": k.grad.numpy()}


def chain_gradients(c, dtype):
    x = torch.tensor(np.asarray(c["x"]), dtype=dtype, requires_grad=True)
    k = torch.tensor(np.asarray(c["k"]), dtype=dtype, requires_grad=True)
    y = inverse_filtering_rank3(x, k, eg.ALPHA, eg.BETA, correlate=c["correlate"], remove_halo=c["remove_halo"], do_edgetaper=True,
                                method=c["method"])
    (y * torch.tensor(np.asarray(c["w"]), dtype=dtype)).sum().backward()
    return {"x": x.grad.numpy(), "k": k.grad.numpy()}


def main():
    out, table, blind = {}, {}, []
    for case in eg.TAPER_CASES:
        name = case[0]
        c = eg.taper_case(name)
        g64, g32 = taper_gradients(c, torch.float64), taper_gradients(c, torch.float32)
        hx, hk = eg.backward(c["x"], c["k"], c["w"], c["method"], c["n"])
        _, ck = eg.backward(c["x"], c["k"], c["w"], c["method"], c["n"], mutant="constant_weights")
        table[name] = dict(kind="taper", E_x=eg.rel_error(g32["x"], g64["x"]), E_k=eg.rel_error(g32["k"], g64["k"]),
                           restatement=max(eg.rel_error(hx, g64["x"]), eg.rel_error(hk, g64["k"])), weight_path=eg.rel_error(ck, g64["k"]))
        for n in ("x", "k"):
            out["%s_d%s" % (name, n)], out["%s_f%s" % (name, n)] = g64[n], g32[n]
        print(name, case[1:5], json.dumps(table[name]))
    for case in eg.CHAIN_CASES:
        name = case[0]
        seed = eg.CHAIN_SEEDS[name]
        if "--search" in sys.argv:
            seed = case[6]
            while not eg.chain_ok(eg.chain_case(name, seed)):
                seed += 1
        c = eg.chain_case(name, seed)
        g64, g32 = chain_gradients(c, torch.float64), chain_gradients(c, torch.float32)
        _, hx, hk = eg.chain_gradients(c)
        margin, clamped = eg.ar.clamp_margin(eg.chain_unclamped(c))
        table[name] = dict(kind="chain", seed=seed, margin=margin, clamped=clamped, E_x=eg.rel_error(g32["x"], g64["x"]),
                           E_k=eg.rel_error(g32["k"], g64["k"]), restatement=max(eg.rel_error(hx, g64["x"]), eg.rel_error(hk, g64["k"])))
        for n in ("x", "k"):
            out["%s_d%s" % (name, n)], out["%s_f%s" % (name, n)] = g64[n], g32[n]
        print(name, case[1:6], json.dumps(table[name]))
    for name, shape, sig, n_iter, alpha, beta, method, seed in eg.BLIND_CASES:
        while True:
            x = er.blurred_noise(seed, shape, sig)
            if eg.blind_steps(x, n_iter, alpha, beta, method) is not None:
                break
            seed += 1
        w = np.random.default_rng(seed + 50).uniform(-1, 1, shape).astype(np.float32)
        xt = torch.tensor(x, requires_grad=True)
        y = polyblur_deblurring(xt, n_iter=n_iter, alpha=alpha, beta=beta, q=0.0, edgetaping=True, method=method)
        (y * torch.tensor(w)).sum().backward()
        gx = xt.grad.numpy()
        off = eg.rel_error(eg.blind_gradient(x, w, n_iter, alpha, beta, method), gx)
        blind.append(dict(name=name, seed=seed, sig=list(sig), n_iter=n_iter, alpha=alpha, beta=beta, method=method, restatement=off))
        out.update({name + "_x": x, name + "_w": w, name + "_gx": gx})
        print(name, shape, method, "n_iter", n_iter, "seed", seed, "|gx| %.3g" % np.abs(gx).max(), "restatement off by %.3g of it" % off)
    for kind in ("taper", "chain"):
        rows = [t for t in table.values() if t["kind"] == kind]
        print("%s: E_x %.3g, E_k %.3g (maxima)" % (kind, max(t["E_x"] for t in rows), max(t["E_k"] for t in rows)))
    out["E"] = np.array(json.dumps(table))
    out["blind"] = np.array(json.dumps(blind))
    path = os.path.join(HERE, "edgetaper_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
