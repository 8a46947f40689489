#!/usr/bin/env python3
"""Golden gradients of the domain-transform recursive filter from the reference's own autograd (this container only; same import
recipe as make_golden_prefilter_autograd.py): domain_transform.recursive_filter (domain_transform.py:6-85) differentiated with
respect to the image and to joint_image, in float64 and again in float32.  Nothing of the reference is replaced: its in-place scan
(:78-83) differentiates as it is.

    python tests/golden/make_golden_dt_autograd.py

writes tests/golden/dt_grad.npz: the inputs x, the guides j and the upstream weights w (float32 values), per case the reference's
x.grad and joint_image.grad from the float64 run (_dx64, _dj64) and from the float32 run (_dx32, _dj32), and `cases`, the JSON list
of what each case is and which arrays are its inputs.  Data only.

loss = sum(w * recursive_filter(x, sigma_s, sigma_r, num_iterations, joint_image)).  Setting n of dt_grad_ref.SETTINGS runs on shape n
of SHAPES, self-guided and with a joint image (the two share x and w) -- every setting on every shape would be 1.2 MB of float64
gradients, beyond what a committed file may hold.  One more case has a guide in multiples of 1/8: about one neighbour pair in nine
is equal there (sign(0) = 0), and the others differ by an amount float32 holds exactly."""
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
from polyblur.domain_transform import recursive_filter  # noqa: E402
import dt_grad_ref as dg  # noqa: E402

SHAPES = [(2, 3, 17, 65), (1, 1, 33, 130), (2, 4, 5, 7)]
QUANTISED = ((1, 3, 9, 70), dg.SETTINGS[1])


def reference_gradients(x, j, w, setting, dtype):
    ss, sr, n = setting
    xt = torch.tensor(x, dtype=dtype, requires_grad=True)
    jt = None if j is None else torch.tensor(j, dtype=dtype, requires_grad=True)
    y = recursive_filter(xt, sigma_s=ss, sigma_r=sr, num_iterations=n, joint_image=jt)
    (y * torch.tensor(w, dtype=dtype)).sum().backward()
    return xt.grad.numpy(), None if jt is None else jt.grad.numpy()


def main():
    out, cases = {}, []
    plan = [(shape, dg.SETTINGS[n], False) for n, shape in enumerate(SHAPES)] + [QUANTISED + (True,)]
    for n, (shape, setting, quantised) in enumerate(plan):
        seed = 4130 + n
        x, j, w = dg.inputs(shape, seed, joint=True, quantised=quantised)
        pre = "s%d" % n
        out.update({pre + "_x": x, pre + "_j": j, pre + "_w": w})
        for joint in ([True] if quantised else [False, True]):
            name = "%s%s" % (pre, "j" if joint else "i")
            jj = j if joint else None
            g64 = reference_gradients(x, jj, w, setting, torch.float64)
            g32 = reference_gradients(x, jj, w, setting, torch.float32)
            mine = dg.backward(x, jj, w, *setting)
            cases.append(dict(name=name, shape=list(shape), sigma_s=setting[0], sigma_r=setting[1], num_iterations=setting[2],
                              joint=joint, quantised=quantised, seed=seed, x=pre + "_x", w=pre + "_w", j=pre + "_j" if joint else None))
            for key, a64, a32, m in (("dx", g64[0], g32[0], mine[0]), ("dj", g64[1], g32[1], mine[1])):
                if a64 is None:
                    continue
                out[name + "_" + key + "64"], out[name + "_" + key + "32"] = a64, a32
                print(name, shape, setting, key, "max |grad| %.3g" % np.abs(a64).max(), "float32 run off by %.3g of max" % dg.rel_error(a32, a64),
                      "| restatement off by %.3g of max" % dg.rel_error(m, a64))
    out["cases"] = np.array(json.dumps(cases))
    path = os.path.join(HERE, "dt_grad.npz")
    np.savez_compressed(path, **out)
    print(os.path.basename(path), os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
