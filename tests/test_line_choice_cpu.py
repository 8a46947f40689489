"""What the line transforms of the estimation run for a launch is ONE host-side choice (csrc/line_choice.h: choose_rows,
choose_cols), read by the launchers, by pb_estimate_impl and by pb_gradient_planes_half.  Through the host query
pb_debug_line_choice -- no GPU -- over every line length of the compiled tables and the shapes whose plans take the other
paths (Bluestein, radices above 16, lines through global memory), P from one image to a batch past every threshold, every use:

* the pieces agree: a shape pb_gradient_planes_half accepts gets compiled fp16-writing kernels on both axes at every P; the tiles
  per image are those of the tile width; the stage order does not depend on P;
* the compiled kernel is chosen exactly where the table holds the plan and the knob allows it, and every row of both tables is
  reached;
* the whole sweep equals tests/golden/line_choices.json, recorded from the launchers as they decided before the choice became
  one function (`python tests/test_line_choice_cpu.py --record` rewrites it: a changed threshold is a diff of that file).
"""
import ctypes
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "line_choices.json")
MEMORY, RUNTIME, COMPILED = 0, 1, 2
F32, F16, U8 = 0, 1, 2
FIELDS = ("kind", "taken", "threads", "lognb", "tiles", "lds", "max_radix", "sat", "half_ok", "ext", "first", "bluestein_m", "nstage")
PS = (1, 2, 6, 8, 13, 32, 64, 200)
KNOBS = ("PB_COLS_FIXED", "PB_ROWS_FIXED", "PB_FFT_FIRST", "PB_FFT_FIRST_ROWS", "PB_FFT_EXT_RADIX", "PB_EST_GRAY_ROWS")


def _table(name):
    """the rows of an X-macro table of csrc/line_choice.h as tuples of ints"""
    src = open(os.path.join(REPO, "polyblur_amd", "csrc", "line_choice.h")).read()
    body = re.search(r"#define %s\(X\)((?:.*\\\n)*.*)\n" % name, src).group(1)
    return [tuple(int(v) for v in m.split(",")) for m in re.findall(r"X\(([^)]*)\)", body)]


COLS_PLANS = _table("PB_COLS_PLANS")                              # (n, r0, r1, r2, lognb narrow, lognb wide or 0)
ROWS_PLANS = [r + ((256, 128),) for r in _table("PB_ROWS_PLANS")] + [r + ((512,),) for r in _table("PB_ROWS_PLAN_8K")]   # (n, r0, r1, r2, threads)

# (use name, LineUse: C, in_dtype, out_dtype, normalize, maxima, n_angles, discard_sat)
ROWS_USES = [("planes_f32", (0, F32, F32, 0, 0, 0, 0)), ("planes_f32_normalize", (0, F32, F32, 1, 0, 0, 0)), ("planes_f16", (0, F32, F16, 0, 0, 0, 0))] + \
            [("gray_c%d_%s" % (C, tn), (C, t, F32, 0, 0, 0, 0)) for C in (1, 3, 4) for t, tn in ((F32, "f32"), (F16, "f16"), (U8, "u8"))]
COLS_USES = [("maxima%d%s%s" % (na + 1, "_normalize" if nz else "", "_sat" if sat else ""), (0, F32, F32, nz, 1, na, sat))
             for na in (6, 11) for nz in (0, 1) for sat in (0, 1)] + [("gy_f32", (0, F32, F32, 0, 0, 0, 0)), ("gy_f16", (0, F32, F16, 0, 0, 0, 0))]
ESTIMATION_USE = dict(COLS_USES)["maxima7"]

# pictures (H, W): every column length of the table against a few widths, every row length against a few heights (the sizes
# the tables name, and 32), the BASELINE pictures, and the shapes of the other paths in both orientations
PICTURES = sorted({(r[0], w) for r in COLS_PLANS for w in (32, 1920)} | {(h, r[0]) for r in ROWS_PLANS for h in (32, 1080)} |
                  {(2160, 3840), (4320, 7680), (512, 640), (1200, 720), (1280, 720), (720, 1200)} |
                  {s for a, b in ((700, 500), (37, 75), (97, 101), (3240, 24), (8200, 10), (20736, 10)) for s in ((a, b), (b, a))})


@pytest.fixture(scope="module")
def lib():
    from polyblur_amd import _capi as capi
    if not os.path.exists(capi.library_path()):
        from polyblur_amd.build import build
        build(verbose=False)
    return capi.load_library()


def query(lib, axis, n, other, P, use):
    out = (ctypes.c_int * 37)()
    rc = lib.pb_debug_line_choice(axis, n, other, P, (ctypes.c_int * 7)(*use), out)
    assert rc == 0, (rc, axis, n, other, P, use)
    c = dict(zip(FIELDS, out[:13]))
    c["radix"] = tuple(out[13:13 + c["nstage"]])
    return c


def planes_half(lib, H, W):
    out = (ctypes.c_int * 37)()
    assert lib.pb_debug_line_choice(2, H, W, 1, (ctypes.c_int * 7)(), out) == 0
    return bool(out[0])


def run_sweep(lib):
    """{"rows|cols H W use": [choice per P]}"""
    assert not [k for k in KNOBS if k in os.environ], "the sweep is that of the default knobs"
    res = {}
    for H, W in PICTURES:
        for name, use in ROWS_USES:
            res["rows %d %d %s" % (H, W, name)] = [query(lib, 0, W, H, P, use) for P in PS]
        for name, use in COLS_USES:
            res["cols %d %d %s" % (H, W, name)] = [query(lib, 1, H, W, P, use) for P in PS]
    return res


@pytest.fixture(scope="module")
def sweep(lib):
    return run_sweep(lib)


RECORDED = ("kind", "taken", "threads", "lognb", "max_radix", "half_ok", "bluestein_m")   # (tiles and lds follow from these: below)


def _golden_form(res):
    """{"fields", "choices": every distinct (RECORDED..., radices) once, "sweep": {"H W": [rows uses, cols uses]}}: per use the
    index of the choice, or the eight indices where it depends on P"""
    choices, index, table = [], {}, {}
    for H, W in PICTURES:
        per_axis = []
        for axis, uses in (("rows", ROWS_USES), ("cols", COLS_USES)):
            per_use = []
            for name, _ in uses:
                ids = []
                for c in res["%s %d %d %s" % (axis, H, W, name)]:
                    t = tuple(c[f] for f in RECORDED) + c["radix"]
                    ids.append(index.setdefault(t, len(index)))
                    if len(choices) < len(index):
                        choices.append(list(t))
                per_use.append(ids[0] if len(set(ids)) == 1 else ids)
            per_axis.append(per_use)
        table["%d %d" % (H, W)] = per_axis
    return {"fields": list(RECORDED) + ["radices..."], "P": list(PS), "rows_uses": [n for n, _ in ROWS_USES],
            "cols_uses": [n for n, _ in COLS_USES], "choices": choices, "sweep": table}


def test_sweep_equals_the_recorded_choices(sweep):
    want = json.load(open(GOLDEN))
    got = _golden_form(sweep)
    assert [got[k] for k in ("fields", "P", "rows_uses", "cols_uses")] == [want[k] for k in ("fields", "P", "rows_uses", "cols_uses")]
    assert sorted(got["sweep"]) == sorted(want["sweep"])
    expand = lambda g, v: [g["choices"][i] for i in (v if isinstance(v, list) else [v] * len(PS))]
    for key in got["sweep"]:
        for axis in (0, 1):
            for u, (a, b) in enumerate(zip(got["sweep"][key][axis], want["sweep"][key][axis])):
                assert expand(got, a) == expand(want, b), (key, "rows" if axis == 0 else "cols", u)


def test_tiles_follow_the_tile_width_and_the_estimation_asks_once(lib, sweep):
    """tiles per image = ceil(W / (2 << lognb)) for every column choice (what sizes est.mags and what blur_params_kernel folds);
    rows: one workgroup per row pair.  pb_estimate_impl and launch_cols read the same object: asked twice, the same answer."""
    for key, per_p in sweep.items():
        axis, H, W = key.split()[0], int(key.split()[1]), int(key.split()[2])
        for c in per_p:
            assert c["tiles"] == ((W + (2 << c["lognb"]) - 1) // (2 << c["lognb"]) if axis == "cols" else (H + 1) // 2), (key, c)
            if c["kind"] != COMPILED:                     # (the lines of the tile; compiled: padded rows, tile + twiddle table)
                assert c["lds"] == (c["bluestein_m"] or (H if axis == "cols" else W)) * 8 << c["lognb"], (key, c)
    for H, W in PICTURES:
        for P in PS:
            assert query(lib, 1, H, W, P, ESTIMATION_USE) == sweep["cols %d %d maxima7" % (H, W)][PS.index(P)]


def test_stage_order_is_the_same_for_every_batch(sweep):
    """bits depend on the order of the stages, and an image must get the same bits alone and in a batch"""
    for key, per_p in sweep.items():
        assert len({(c["radix"], c["bluestein_m"], c["ext"], c["first"]) for c in per_p}) == 1, key


def test_fp16_planes_where_both_axes_say_so_at_every_batch(lib, sweep):
    """ADVICE's finding on estimate.hip as a test: a shape pb_gradient_planes_half accepts must get a compiled kernel that writes
    fp16 on both axes at every P -- anything else fails an fp16 call with remove_halo outright.  The other way round it may
    refuse only the widths that are no multiple of 32 (kept from the rule before the choosers)."""
    accepted = 0
    for H, W in PICTURES:
        rows, cols = sweep["rows %d %d planes_f16" % (H, W)], sweep["cols %d %d gy_f16" % (H, W)]
        both = all(c["kind"] == COMPILED and c["half_ok"] for c in rows + cols)
        assert planes_half(lib, H, W) == (both and W % 32 == 0), (H, W)
        accepted += planes_half(lib, H, W)
    assert accepted >= len(COLS_PLANS)               # (every column length of the table at W = 1920 at least)


def _cols_row(c):
    """(table row, threads) of the compiled column kernel for this plan and tile width, or None"""
    for n, r0, r1, r2, ln, lw in COLS_PLANS:
        if (c["bluestein_m"], c["radix"]) == (0, (r0, r1, r2)) and c["lognb"] in (ln, lw) and c["lognb"] != 0:
            return (n, c["lognb"]), 1024 if c["lognb"] == lw else 512
    return None


def _rows_row(c):
    for n, r0, r1, r2, threads in ROWS_PLANS:
        if (c["bluestein_m"], c["radix"]) == (0, (r0, r1, r2)) and c["threads"] in threads:
            return (n, c["threads"]), c["threads"]
    return None


def test_compiled_exactly_where_the_table_holds_the_plan(sweep):
    """... and the use has a compiled instance (the un-normalised image; the 7 directions or the y derivative; gray from one or
    three fp32 channels; whole tiles).  Every row of both tables, on each of its tile widths / thread counts, is reached."""
    reached = set()
    for key, per_p in sweep.items():
        axis, H, W, use = key.split()
        H, W = int(H), int(W)
        u = dict(ROWS_USES + COLS_USES)[use]
        for c in per_p:
            if axis == "cols":
                n = H
                row = _cols_row(c) if (not u[3] and (not u[4] or u[5] == 6) and W % (2 << c["lognb"]) == 0) else None
            else:
                n = W
                row = _rows_row(c) if (not u[3] and c["taken"] and u[0] in (0, 1, 3)) else None
            if row is not None and c["kind"] != MEMORY and row[0][0] == n:
                assert c["kind"] == COMPILED and c["threads"] == row[1], (key, c)
                reached.add((axis,) + row[0])
            else:
                assert c["kind"] != COMPILED, (key, c)
    want = {("cols", r[0], l) for r in COLS_PLANS for l in r[4:6] if l} | {("rows", r[0], t) for r in ROWS_PLANS for t in r[4]}
    assert reached == want, sorted(want - reached)


@pytest.mark.parametrize("knob", ["PB_COLS_FIXED", "PB_ROWS_FIXED"])
def test_the_knob_selects_the_run_time_plan_kernels(lib, sweep, knob, monkeypatch):
    """PB_COLS_FIXED=0 / PB_ROWS_FIXED=0 (the GPU tests' bit-identity reference): no compiled kernel on that axis, the same plan,
    and no fp16 planes for any shape"""
    monkeypatch.setenv(knob, "0")
    axis, uses = (1, COLS_USES) if knob == "PB_COLS_FIXED" else (0, ROWS_USES)
    for H, W in PICTURES[::3]:
        for name, use in uses:
            for i, P in enumerate(PS):
                c = query(lib, axis, H if axis else W, W if axis else H, P, use)
                d = sweep["%s %d %d %s" % ("cols" if axis else "rows", H, W, name)][i]
                assert c["kind"] != COMPILED and not c["half_ok"] and c["radix"] == d["radix"], (H, W, name, P, c)
                if d["kind"] != COMPILED and not (axis and H == 1080):     # (1080-point columns keep the narrow tile for lines_fixed.hip only)
                    assert c == d, (H, W, name, P)
        assert not planes_half(lib, H, W)


if __name__ == "__main__" and "--record" in sys.argv:
    sys.path.insert(0, REPO)
    from polyblur_amd import _capi
    with open(GOLDEN, "w") as f:
        g = _golden_form(run_sweep(_capi.load_library()))                # (one choice, one key per line: a change reads as a diff)
        f.write('{%s,\n"choices": [\n%s\n],\n"sweep": {\n%s\n}}\n' % (
            ",\n".join('"%s": %s' % (k, json.dumps(g[k])) for k in ("fields", "P", "rows_uses", "cols_uses")),
            ",\n".join(json.dumps(c) for c in g["choices"]),
            ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in g["sweep"].items())))
    print("wrote", GOLDEN, os.path.getsize(GOLDEN), "bytes")
