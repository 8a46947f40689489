"""The front end's checks, refusals and their order (polyblur_amd/_frontend.py): every call of
tests/frontend_cases.py ends as tests/golden/frontend_refusals.json recorded it -- the same exception class and message, or the
same arrival at the engine -- and the package keeps the structure that gives each piece of host glue one owner."""
import json
import os
import re

import pytest

import frontend_cases as fc
from polyblur_amd import _capi as capi

if not os.path.exists(capi.library_path()):                   # (the size checks ask pb_fft_length_supported: the library, no GPU)
    from polyblur_amd.build import build
    build(verbose=False)

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(REPO, "tests", "golden", "frontend_refusals.json")) as _f:
    RECORDED = json.load(_f)
TABLE = dict(fc.table())


def test_the_table_is_the_recorded_one():
    assert sorted(TABLE) == sorted(RECORDED) and len(TABLE) >= 100
    ends = {a if isinstance(a, str) else a[0] for a in RECORDED.values()}
    assert {"DEVICE", "ValueError", "TypeError", "NotImplementedError"} <= ends       # (a table of one answer would say little)


@pytest.mark.parametrize("name", sorted(RECORDED))
def test_every_call_ends_as_recorded(name):
    assert fc.outcome(TABLE[name]) == RECORDED[name]


def _sources():
    pkg = os.path.join(REPO, "polyblur_amd")
    return {n: open(os.path.join(pkg, n)).read() for n in sorted(os.listdir(pkg)) if n.endswith(".py")}


def test_each_piece_of_host_glue_has_one_owner():
    src = _sources()
    assert [n for n, s in src.items() if "current_stream(" in s] == ["_frontend.py"] and src["_frontend.py"].count("current_stream(") == 1
    assert [n for n, s in src.items() if "once_differentiable" in s] == ["_autograd.py"]
    assert sum(s.count("halo masking is differentiated for float32 ROCm tensors only") for s in src.values()) == 1
    # (the binding's own `global _lib` aside: the library handle, not a lazily built class)
    assert [n for n, s in src.items() if re.search(r"^\s*global\s", s, re.M)] == ["_capi.py"]
    assert "ctypes" not in src["deblurring.py"]
    assert not re.search(r"^import torch|^from torch", src["_frontend.py"], re.M)        # (torch stays optional at import time)
