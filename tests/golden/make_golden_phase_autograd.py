#!/usr/bin/env python3
"""Golden gradients of the polynomial with the pure-phase filter from the reference's own autograd (this container only; same
import recipe as make_golden_phase.py): deblurring.compute_polynomial(method='fft', not_symmetric=True) (deblurring.py:113-169) on
the replicate-padded domain, and inside inverse_filtering_rank3's chain (deblurring.py:211-239), which the reference never calls
with the flag -- composed here from the reference's own functions:

    utils.pad_with_kernel -> compute_polynomial(method='fft', not_symmetric=True) -> utils.crop_with_kernel
    -> [halo_masking] -> clamp

    python tests/golden/make_golden_phase_autograd.py [--search]

writes tests/golden/nonblind_phase_grad.npz: for the cases of phase_grad_ref.GOLDEN_POLY and every chain case the reference's
gradients of the image and of the kernel (and of grad_img where given) in float64 (`_d*`) and in float32 (`_f*`) -- the inputs are
built again by tests/phase_grad_ref.py from their seeds --, and `E`, a JSON table: for EVERY case the GPU tests run (those without
stored gradients too) the reference's float32 error against its float64 gradients relative to the largest float64 entry, min |K|,
and for chain cases the clamp margins.  --search: look for the chain cases' seeds again (phase_grad_ref.chain_ok)."""
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
from polyblur import filters as ref_filters, utils as ref_utils  # noqa: E402
from polyblur.deblurring import compute_polynomial, halo_masking  # noqa: E402
import phase_grad_ref as pg  # noqa: E402


def poly_gradients(c, dtype):
    x = torch.tensor(np.asarray(c["x"]), dtype=dtype, requires_grad=True)
    k = torch.tensor(np.asarray(c["k"]), dtype=dtype, requires_grad=True)
    y = compute_polynomial(x, k, c["alpha"], c["b"], method="fft", not_symmetric=True)
    (y * torch.tensor(np.asarray(c["w"]), dtype=dtype)).sum().backward()
    return {"x": x.grad.numpy(), "k": k.grad.numpy()}


def chain_gradients(c, dtype):
    x = torch.tensor(np.asarray(c["x"]), dtype=dtype, requires_grad=True)
    k = torch.tensor(np.asarray(c["k"]), dtype=dtype, requires_grad=True)
    gs = None if c["grad_img"] is None else tuple(torch.tensor(np.asarray(a), dtype=dtype, requires_grad=True) for a in c["grad_img"])
    kernel = torch.rot90(k, k=2, dims=(-2, -1)) if c["correlate"] else k
    xp = ref_utils.pad_with_kernel(x, kernel)
    y = ref_utils.crop_with_kernel(compute_polynomial(xp, kernel, c["alpha"], c["b"], method="fft", not_symmetric=True), kernel)
    if c["remove_halo"]:
        y = halo_masking(x, y, gs)
    (torch.clamp(y, 0.0, 1.0) * torch.tensor(np.asarray(c["w"]), dtype=dtype)).sum().backward()
    out = {"x": x.grad.numpy(), "k": k.grad.numpy()}
    if gs is not None:
        out.update(gx=gs[0].grad.numpy(), gy=gs[1].grad.numpy())
    return out


def main():
    out, table = {}, {}
    for name in pg.POLY_NAMES + [pg.LONG]:
        c = pg.poly_case(name)
        g64, g32 = poly_gradients(c, torch.float64), poly_gradients(c, torch.float32)
        K = ref_filters.p2o(torch.tensor(np.asarray(c["k"], np.float64)), c["x"].shape[-2:])
        want = pg.poly_want(name)
        table[name] = dict(kind="poly", E_x=pg.rel_error(g32["x"], g64["x"]), E_k=pg.rel_error(g32["k"], g64["k"]), min_K=float(K.abs().min()),
                           restatement=max(pg.rel_error(want[0], g64["x"]), pg.rel_error(want[1], g64["k"])))
        if name in pg.GOLDEN_POLY:
            for n in ("x", "k"):
                out["%s_d%s" % (name, n)], out["%s_f%s" % (name, n)] = g64[n], g32[n]
        print(name, c["x"].shape, json.dumps(table[name]))
    for case in pg.CHAIN_CASES:
        name = case[0]
        c = pg.chain_case(name, None if "--search" in sys.argv else -1)
        g64, g32 = chain_gradients(c, torch.float64), chain_gradients(c, torch.float32)
        with pg.reference_frequencies():
            want = pg.chain_backward(c["x"], c["k"], c["w"], c["alpha"], c["b"], c["correlate"], c["remove_halo"], c["grad_img"])
        margin, clamped, band_empty, moved = pg.chain_margins(c)
        table[name] = dict(kind="chain", seed=c["seed"], margin=margin, clamped=clamped, band_empty=band_empty, moved=moved,
                           restatement=max(pg.rel_error(want[n], g64[n]) for n in g64), **{"E_" + n: pg.rel_error(g32[n], g64[n]) for n in g64})
        for n in g64:
            out["%s_d%s" % (name, n)], out["%s_f%s" % (name, n)] = g64[n], g32[n]
        print(name, case[1], json.dumps(table[name]))
    out["E"] = np.array(json.dumps(table))
    path = os.path.join(HERE, "nonblind_phase_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
