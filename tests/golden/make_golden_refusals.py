#!/usr/bin/env python3
"""Writes tests/golden/frontend_refusals.json: how every call of tests/frontend_cases.py ends before any device work -- the
exception class and message, "DEVICE" (every check passed: the call asked for an engine) or "RETURNED".

    python -m polyblur_amd.build && python tests/golden/make_golden_refusals.py

Run it on the commit whose answers are to be kept (the file in the tree was recorded on the parent of the commit that gave the
front end one owner, polyblur_amd/_frontend.py); tests/test_frontend_cpu.py replays the table and demands equality.  It needs the
built library (pb_fft_length_supported, which needs no GPU) and no GPU.

EXPECTED_CHANGES are the answers that differ from the recorded commit's on purpose, written with their new value: a grad_img
plane that is neither an array nor a tensor, without grad, used to die on the plane's missing .shape (AttributeError); it gets the
one grad_img check's TypeError."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

import frontend_cases as fc  # noqa: E402

EXPECTED_CHANGES = {"%s/remove_halo/grad_img=mistyped" % f: ["TypeError", "grad_img planes must be numpy.ndarrays or torch.Tensors"]
                    for f in ("inverse_filtering_rank3", "inverse_filtering_nonsymmetric")}


def main():
    answers = {name: fc.outcome(call) for name, call in fc.table()}
    for name, new in EXPECTED_CHANGES.items():
        print("%s: recorded %r, kept as %r" % (name, answers[name], new))
        answers[name] = new
    with open(os.path.join(HERE, "frontend_refusals.json"), "w") as f:
        json.dump(answers, f, indent=0, sort_keys=True)
        f.write("\n")
    kinds = {}
    for a in answers.values():
        kinds[a if isinstance(a, str) else a[0]] = kinds.get(a if isinstance(a, str) else a[0], 0) + 1
    print(len(answers), "cases:", kinds)


if __name__ == "__main__":
    main()
