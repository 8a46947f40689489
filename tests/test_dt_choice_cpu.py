"""What the domain-transform recursive filter runs for a call on one- or three-channel images is ONE host-side choice
(csrc/dt_choice.h: choose_dt), asked once per call by the launcher of csrc/dt.hip.  Through the host query pb_debug_dt_choice --
no GPU:

(a) the sweep equals tests/golden/dt_choices.json: both element sizes, one and three channels, guided and self-guided input,
    operands on and off 16-byte boundaries, the default knobs and the knob set of every dt_* engine of
    tests/test_gpu_round5_forms.py (tests/dt_form_cases.py), over shapes with a value on each side of every threshold: W = 256 /
    257, 1024 / 1025, 2048 / 2049, 4096 / 4097, 8192 / 8193; B H = 8192 / 8200; B W = 24576 and above; H = 63 / 64 and 127 /
    128; W = 0 and 2 mod 4, and 4 mod 8; three-channel 8192-wide planes of 21845 and 21846 rows (C H W 4 = 2 GiB).

    The file was recorded from the launcher as it decided BEFORE there was a chooser -- the if / else cascade inside the
    per-iteration loop of dt_filter_fused (csrc/filters.hip at that commit) -- and not from a restatement of it: a program
    took that function's text as it stood, with its thresholds and the DtCoop sizes beside it, replaced every
    hipLaunchKernelGGL by an append of the kernel's name and template arguments to a host list, pb_scratch and
    hipFuncSetAttribute by appends of their names and sizes, left every condition as written, and ran the shapes below
    through it with two iterations (pointers that are never dereferenced stand for the operands).  Kernel names map to the
    fields here one to one: dt_rows_fused_kernel<T, T> = MEMORY, dt_rows_reg_kernel<.., NCH> = WAVE with NCH chunks,
    dt_rows_regw_kernel<.., CPW> = WORKGROUP with CPW chunks per wave; dt_cols_fused_kernel = SWEEPS, dt_cols_down_kernel<..,
    S, false> + dt_cols_up_kernel = STRIPS of S rows, dt_cols_down_kernel<.., S, true> + dt_cols_upw_kernel = STRIPS_WEIGHTS,
    dt_cols_coop_kernel<.., R> = COOP with blocks of R rows; carry / weights = the floats of "dt.carry" / "dt.weights".  (The
    second iteration's record: dt_rows_fused_kernel<T, float> in place and the same column launches, for every case.)
    `python tests/test_dt_choice_cpu.py --record` rewrites the file from choose_dt: a changed threshold is a diff of it.
(b) the pieces agree: carry and weights are those of the chosen strip or block rows, dynamic LDS belongs to the cooperative
    form alone, a forced knob changes only the pass it names;
(c) reachability: over the shapes, dtypes and engines of the two GPU form tests (tests/dt_form_cases.py) every kernel
    instantiation the launcher can reach -- row form x chunk count x channels x dtype, column form x channels x dtype -- is
    taken by at least one case.
"""
import ctypes
import json
import os
import sys

import numpy as np
import pytest

import dt_form_cases as cases

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "dt_choices.json")
FIELDS = ("rows", "chunks", "cols", "cols_rows", "carry", "weights", "lds")
MEMORY, WAVE, WORKGROUP = 0, 1, 2                       # rows (dt_choice.h)
SWEEPS, STRIPS, STRIPS_WEIGHTS, COOP = 0, 1, 2, 3       # cols
KNOB_ENV = ("PB_DT_ROWS_REG", "PB_DT_COLS_STRIP", "PB_DT_COLS_COOP")
KNOB_SETS = ["default"] + list(cases.DT_ENGINE_KNOBS)

WIDTHS = (254, 256, 257, 260, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193)
SHAPES = [(B, H, W) for W in WIDTHS for B, H in ((1, 64), (2, 4096), (2, 4100))] + \
         [(B, H, W) for H in (63, 64, 127, 128) for B, W in ((1, 256), (1, 254), (3, 260))] + \
         [(3, 64, 8192), (4, 64, 8192), (6, 128, 4096), (7, 128, 4096), (24, 64, 1024), (25, 64, 1024), (12, 127, 2048), (13, 127, 2048)] + \
         [(1, 21845, 8192), (1, 21846, 8192), (2, 21845, 8192), (2, 21846, 8192)]
KEYS = [(elem, C, self_guided, aligned, k) for elem in (4, 2) for C in (1, 3) for self_guided in (1, 0) for aligned in (1, 0) for k in KNOB_SETS]


@pytest.fixture(scope="module")
def lib():
    from polyblur_amd import _capi as capi
    if not os.path.exists(capi.library_path()):
        from polyblur_amd.build import build
        build(verbose=False)
    return capi.load_library()


def query(lib, elem, C, B, H, W, self_guided, aligned, knobs):
    """the choice as a dict of FIELDS; knobs: (rows_reg, cols_strip, cols_coop), or None for the environment's"""
    out = (ctypes.c_longlong * 7)()
    rc = lib.pb_debug_dt_choice(elem, C, B, H, W, self_guided, aligned, (ctypes.c_int * 3)(*knobs) if knobs is not None else None, out)
    assert rc == 0, (rc, elem, C, B, H, W, self_guided, aligned, knobs)
    return dict(zip(FIELDS, out[:]))


def key_name(key):
    return "%d %d %s %s %s" % (key[0], key[1], "self" if key[2] else "joint", "aligned" if key[3] else "unaligned", key[4])


def run_sweep(lib):
    """{key name: [choice per shape]}"""
    return {key_name(k): [query(lib, k[0], k[1], B, H, W, k[2], k[3], cases.knobs_of(k[4])) for B, H, W in SHAPES] for k in KEYS}


@pytest.fixture(scope="module")
def sweep(lib):
    return run_sweep(lib)


def golden_form(res):
    """every distinct row choice and column choice once; per key the two indices of every shape, flattened"""
    rows, cols, ri, ci, table = [], [], {}, {}, {}
    for key, per_shape in res.items():
        flat = []
        for c in per_shape:
            r, k = (c["rows"], c["chunks"]), (c["cols"], c["cols_rows"], c["carry"], c["weights"], c["lds"])
            if r not in ri:
                ri[r] = len(rows); rows.append(list(r))
            if k not in ci:
                ci[k] = len(cols); cols.append(list(k))
            flat += [ri[r], ci[k]]
        table[key] = flat
    return {"fields": list(FIELDS), "knobs": {k: list(cases.knobs_of(k)) for k in KNOB_SETS}, "shapes": [list(s) for s in SHAPES],
            "rows": rows, "cols": cols, "sweep": table}


def expand(g, key):
    flat = g["sweep"][key]
    return [tuple(g["rows"][flat[i]]) + tuple(g["cols"][flat[i + 1]]) for i in range(0, len(flat), 2)]


def test_sweep_equals_the_recorded_choices(sweep):
    want = json.load(open(GOLDEN))
    got = golden_form(sweep)
    assert [got[k] for k in ("fields", "knobs", "shapes")] == [want[k] for k in ("fields", "knobs", "shapes")]
    assert sorted(got["sweep"]) == sorted(want["sweep"])
    for key in got["sweep"]:
        for shape, a, b in zip(SHAPES, expand(got, key), expand(want, key)):
            assert a == b, (key, shape, dict(zip(FIELDS, a)), dict(zip(FIELDS, b)))


def test_the_environment_is_read_where_no_knobs_are_given(lib, monkeypatch):
    """a null knob pointer: the knobs as pb_create reads them"""
    for k in KNOB_ENV:
        monkeypatch.delenv(k, raising=False)
    args = (4, 3, 1, 720, 1280, 1, 1)
    assert query(lib, *args, None) == query(lib, *args, (1, 1, 1))
    for name, env in cases.DT_ENGINE_KNOBS.items():
        for k in KNOB_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, str(v))
        assert query(lib, *args, None) == query(lib, *args, cases.knobs_of(name)), name


def test_scratch_and_lds_are_those_of_the_chosen_form(sweep):
    ceil = lambda a, b: (a + b - 1) // b
    for k in KEYS:
        C = k[1]
        for (B, H, W), c in zip(SHAPES, sweep[key_name(k)]):
            where = (key_name(k), B, H, W, c)
            assert (c["chunks"] == 0) == (c["rows"] == MEMORY), where
            if c["rows"] == WAVE:
                assert c["chunks"] in (16, 32, 64) and W <= 64 * c["chunks"], where
            if c["rows"] == WORKGROUP:
                assert c["chunks"] in (4, 8, 16, 32) and W <= 256 * c["chunks"], where
            R = c["cols_rows"]
            if c["cols"] == SWEEPS:
                assert (R, c["carry"], c["weights"], c["lds"]) == (0, 0, 0, 0), where
            elif c["cols"] in (STRIPS, STRIPS_WEIGHTS):
                assert R == (32 if c["cols"] == STRIPS_WEIGHTS else 16) and c["lds"] == 0, where
                assert c["carry"] == ceil(H, R) * C * B * W, where
                assert c["weights"] == (H * B * W if c["cols"] == STRIPS_WEIGHTS else 0), where
            else:
                CG = 64 if C == 1 else 16
                assert c["cols"] == COOP and R == (64 if C == 1 else 96) and c["weights"] == 0, where
                assert c["carry"] == B * ceil(W, CG) * ceil(H, R) * C * CG, where
                # (more than the 48 KB a kernel may take unasked: the launcher raises the kernel's limit, once per call)
                assert 48 * 1024 < c["lds"] <= 80 * 1024 + 4096 and c["lds"] % 1024 == 0, where


def test_a_forced_knob_changes_only_the_pass_it_names(sweep):
    row_fields, col_fields = FIELDS[:2], FIELDS[2:]
    for k in KEYS:
        if k[4] == "default":
            continue
        rows_knob = "PB_DT_ROWS_REG" in cases.DT_ENGINE_KNOBS[k[4]]
        for shape, c, d in zip(SHAPES, sweep[key_name(k)], sweep[key_name(k[:4] + ("default",))]):
            same = col_fields if rows_knob else row_fields
            assert [c[f] for f in same] == [d[f] for f in same], (key_name(k), shape, c, d)


def _instantiations(choice, C, elem):
    return {("rows", choice["rows"], choice["chunks"], C, elem), ("cols", choice["cols"], C, elem)}


def test_every_instantiation_is_reached_by_a_gpu_form_case(lib, sweep):
    """what the launcher can reach: every (form, chunk count, channels, dtype) the sweep above shows -- which must itself hold the
    full list -- against what tests/test_gpu_round5_forms.py runs: test_dt_rows_register_form (self-guided) and
    test_dt_columns_in_strips (self-guided and with a joint image of its own), each under its engines' knobs"""
    reachable = set()
    for k in KEYS:
        for c in sweep[key_name(k)]:
            reachable |= _instantiations(c, k[1], k[0])
    full = {("rows", f, n, C, e) for f, ns in ((MEMORY, (0,)), (WAVE, (16, 32, 64)), (WORKGROUP, (4, 8, 16, 32))) for n in ns for C in (1, 3) for e in (4, 2)} | \
           {("cols", f, C, e) for f in (SWEEPS, STRIPS, COOP) for C in (1, 3) for e in (4, 2)} | {("cols", STRIPS_WEIGHTS, 3, 4)}
    assert reachable == full, (sorted(full - reachable), sorted(reachable - full))
    reached = set()
    for shape in cases.ROW_FORM_SHAPES:
        for dtype in cases.ROW_FORM_DTYPES:
            for eng in cases.ROW_FORMS:
                B, C, H, W = shape
                reached |= _instantiations(query(lib, np.dtype(dtype).itemsize, C, B, H, W, 1, 1, cases.knobs_of(eng)), C, np.dtype(dtype).itemsize)
    for shape, dtype in cases.COLUMN_FORM_CASES:
        for eng in cases.COLUMN_FORMS:
            for self_guided in (1, 0):
                B, C, H, W = shape
                reached |= _instantiations(query(lib, np.dtype(dtype).itemsize, C, B, H, W, self_guided, 1, cases.knobs_of(eng)), C, np.dtype(dtype).itemsize)
    assert reached == full, sorted(full - reached)


def test_bad_arguments_are_refused(lib):
    out = (ctypes.c_longlong * 7)()
    for args in ((3, 3, 1, 8, 8, 1, 1), (4, 2, 1, 8, 8, 1, 1), (4, 3, 0, 8, 8, 1, 1), (4, 3, 1, 0, 8, 1, 1), (4, 3, 1, 8, 0, 1, 1)):
        assert lib.pb_debug_dt_choice(*args, None, out) != 0, args
    assert lib.pb_debug_dt_choice(4, 3, 1, 8, 8, 1, 1, None, None) != 0


def write_golden(g, path=GOLDEN):
    """one key per line: a change reads as a diff"""
    with open(path, "w") as f:
        f.write('{%s,\n"rows": %s,\n"cols": [\n%s\n],\n"sweep": {\n%s\n}}\n' % (
            ",\n".join('"%s": %s' % (k, json.dumps(g[k])) for k in ("fields", "knobs", "shapes")), json.dumps(g["rows"]),
            ",\n".join(json.dumps(c) for c in g["cols"]),
            ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v).replace(" ", "")) for k, v in g["sweep"].items())))
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, REPO)
    from polyblur_amd import _capi
    write_golden(golden_form(run_sweep(_capi.load_library())))
