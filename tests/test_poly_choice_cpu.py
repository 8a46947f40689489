"""What a reblurring call issues -- every launch of one pass (pb_launch_conv) or of the three Horner steps of a polynomial
(pb_launch_conv_poly), in order, with its stream -- is ONE host-side plan (csrc/poly_choice.h: choose_pass / choose_poly), made from
facts the launcher gathers before its first launch and issued by one loop of csrc/conv.hip.  Through the host query
pb_debug_poly_plan -- no GPU:

(a) the sweep equals tests/golden/poly_plans.json.  The file was recorded from the two launchers as they decided BEFORE there was a
    chooser, not from a restatement of them: a program took the text of known_flags, pb_launch_conv, launch_tile_spectrum,
    composite_pass, SideStream and pb_launch_conv_poly as it stood (csrc/conv.hip at that commit), left every condition as
    written, and replaced launch_stencil, pb_launch_conv_wfft / _fft / _w128 / _win / _strip by appends of their name with the
    pass (which step, or the composite), its poly and ring, whether `known` was null, whether the context's stream was the side
    stream, and whose spectra the pass carried; pb_build_khat / _ring by appends with the `launch` argument; SpectraSet.drop by an
    append; the event calls by FORK (the side stream's wait) and JOIN (the caller's); pb_fail by an append of the message.  The
    predicates answered from the case's facts.  The wave and merged launchers kept their own "not this pass" answers of that commit
    (types not built; a three-step job list beyond the grid), the workgroup launcher its refusal of types; pb_build_khat kept its
    treatment of the first scratch set (the second set's spectra handed out untouched, a stale set launched and claimed whatever
    `launch` says).  A refusing case is recorded as the message the call returned (the choosers refuse before the first launch).
    `python tests/test_poly_choice_cpu.py --record` rewrites the file from the choosers: a changed rule is a diff of it
    (`--cases FILE` writes the cases the sweep asks, one per line: polynomial, strip outcome, the facts).

    The sweep (SLABS): every condition of the two functions has a value on each side; not the full product of the 45 facts (2.8e7
    polynomials) but
      poly:       fft off / on / each step failing fft_pass_ok  x  spec (on 0-3 x always 0 / 1, and on 0 always 2)  x  wrap / zero  x
                  fold  x  records (none; host-read with every meaningful flag pattern)  x  the first scratch set (held x by_estimate x
                  what a build will do)  x  (aux, prof_on, 12287 / 12288 tiles) in the five combinations the two stream conditions
                  tell apart -- at the default knobs, every predicate true;
      poly knobs: fft_wave 0 / 1 x poly_one_launch 0 / 1 / 2 over the same, with three scratch states and two stream combinations
                  (the knobs are read beside neither);
      poly preds: each of the 14 types / feasibility predicates false ALONE, under both fft_wave, with one scratch state (a predicate
                  decides which launcher an op names, the scratch the `launch` flag of a build; two false predicates at once are
                  not swept: the text treats each in a branch of its own, and where two refusals meet -- a ring step on the side
                  stream and the window pass -- it reported the later one, which no caller could reach);
      poly strip: the experimental strip body, taking the pass and declining it;
      pass ...:   the single pass likewise, with khat_ready, no_fft, poly 0 / 2, ring 0 / 4 / 5 and the windows-only case (on 0,
                  always 2, records not read).
    `ksel` is `have and on` throughout, as known_flags gives it.
(b) consistency: a plan with a fork has exactly one join, after its last side-stream op; nothing goes to the side stream where
    there is none or under profiling; no form is launched whose types predicate is false; a refusal ends the plan.
(c) reachability: every op kind and every refusal message is produced by some case; the longest plan fits PB_POLY_MAX_OPS.
"""
import ctypes
import itertools
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "poly_plans.json")

FACTS = ("fft_on", "fft_wave", "poly_one_launch", "strip_mode", "aux", "prof_on",
         "step_ok0", "step_ok1", "step_ok2", "wave_types0", "wave_types1", "wave_types2", "wave_fits0", "wave_fits1", "wave_fits2",
         "wg_types0", "wg_types1", "wg_types2", "strip_pass0", "strip_pass1", "strip_pass2",
         "whole_ok", "whole_wave_types", "whole_wave_fits", "whole_wg_types", "whole_win_types",
         "on", "always", "zero", "fold", "no_fft", "khat_ready", "ring", "poly", "side_tiles",
         "have", "any_fft", "any_other", "any_strip", "any_tile", "any_fft3", "ksel", "held", "by_estimate", "spectra")
OP_FIELDS = ("kind", "step", "poly", "ring", "side", "known", "set", "arg")
BUILD, BUILD_RING, DROP, STENCIL, WAVE, WG, W128, WIN, STRIP, FORK, JOIN, FAIL = range(1, 13)      # poly_choice.h: PB_OP_*
LAUNCHES = (STENCIL, WAVE, WG, W128, WIN, STRIP)
WHOLE = 3                                  # PolyOp.step of the composite pass
READY, STALE, SECOND = 0, 1, 2             # PB_SPECTRA_*
WHEN_STRIP_REFUSED = 1
MESSAGES = 5
MAX_OPS = 20
PREDICATES = FACTS[9:18] + FACTS[21:26]

BASE = dict.fromkeys(FACTS, 0)
BASE.update({k: 1 for k in FACTS[6:18] + FACTS[21:26]}, fft_on=1, fft_wave=1, poly_one_launch=1, aux=1, spectra=STALE)


def dim(**options):
    return list(options.items())


FFT = dim(off=dict(fft_on=0), on={}, fail0=dict(step_ok0=0), fail1=dict(step_ok1=0), fail2=dict(step_ok2=0))
SPEC = [("on%d_always%d" % (on, al), dict(on=on, always=al)) for on in range(4) for al in (0, 1)] + [("on0_always2", dict(on=0, always=2))]
ZERO = dim(wrap={}, zero=dict(zero=1))
FOLD = dim(nofold={}, fold=dict(fold=1))
RECORDS = dim(none={}, fft=dict(have=1, any_fft=1), fft3=dict(have=1, any_fft=1, any_fft3=1), stencil=dict(have=1, any_other=1, any_tile=1),
              both=dict(have=1, any_fft=1, any_other=1, any_tile=1), both3=dict(have=1, any_fft=1, any_fft3=1, any_other=1, any_tile=1),
              strip=dict(have=1, any_other=1, any_strip=1), strip_tile=dict(have=1, any_other=1, any_strip=1, any_tile=1),
              strip_fft=dict(have=1, any_fft=1, any_fft3=1, any_other=1, any_strip=1))
SCRATCH = [("held%d_est%d_%s" % (h, e, ("ready", "stale", "second")[s]), dict(held=h, by_estimate=e, spectra=s))
           for h, e, s in ((0, 0, STALE), (0, 0, SECOND), (1, 0, READY), (1, 1, READY), (1, 0, STALE), (1, 1, STALE), (1, 0, SECOND), (1, 1, SECOND))]
SCRATCH3 = [SCRATCH[0], SCRATCH[3], SCRATCH[2]]
SCRATCH2 = SCRATCH3[:2]
STREAMS = [("aux%d_prof%d_tiles%d" % v, dict(aux=v[0], prof_on=v[1], side_tiles=v[2])) for v in ((1, 0, 1), (1, 0, 0), (0, 0, 1), (1, 1, 1), (0, 1, 0))]
STREAMS2 = STREAMS[:2]
KNOBS = [("wave%d_one%d" % (w, o), dict(fft_wave=w, poly_one_launch=o)) for w in (1, 0) for o in (1, 0, 2)]
WAVE_KNOB = dim(wave=dict(fft_wave=1), wg=dict(fft_wave=0))
FALSE = [("no_" + p, {p: 0}) for p in PREDICATES]
STRIP_POLY = [("strip%d%d%d_%s" % (a, b, c, "taken" if t else "declined"), dict(strip_mode=1, strip_pass0=a, strip_pass1=b, strip_pass2=c, strip_takes=t))
              for a, b, c in ((1, 1, 1), (0, 1, 0), (0, 0, 0)) for t in (1, 0)]
STRIP_PASS = [("strip%d_%s" % (a, "taken" if t else "declined"), dict(strip_mode=1, strip_pass0=a, strip_takes=t)) for a in (1, 0) for t in (1, 0)]
READINESS = [("ready%d_nofft%d" % (k, n), dict(khat_ready=k, no_fft=n)) for k in (0, 1) for n in (0, 1)]
POLY02 = dim(poly0={}, poly2=dict(poly=2))
RING = dim(ring4=dict(ring=4), ring5=dict(ring=5))

# name: (polynomial, dimensions); a row of the golden file is one choice of the first two dimensions
SLABS = {
    "poly": (1, [FFT, SPEC, ZERO, FOLD, RECORDS, SCRATCH, STREAMS]),
    "poly knobs": (1, [KNOBS[1:], SPEC, FFT[1:4:2], ZERO, FOLD, RECORDS, SCRATCH3, STREAMS2]),
    "poly preds": (1, [FALSE, SPEC, WAVE_KNOB, ZERO, FOLD, RECORDS, SCRATCH[3:4], STREAMS2]),
    "poly strip": (1, [STRIP_POLY, SPEC, FFT[:2], FOLD, RECORDS[0:1] + RECORDS[3:4] + RECORDS[6:], SCRATCH2]),
    "pass": (0, [FFT[:3], SPEC, RECORDS, SCRATCH, READINESS, POLY02, WAVE_KNOB]),
    "pass ring": (0, [RING, SPEC, RECORDS, SCRATCH2, POLY02]),
    "pass preds": (0, [FALSE[0:1] + FALSE[3:4] + FALSE[6:7], SPEC, WAVE_KNOB, RECORDS, POLY02]),
    "pass strip": (0, [STRIP_PASS, SPEC, FFT[:2], RECORDS, POLY02]),
}


def slab_cases(name):
    """(row key, [(facts dict, strip outcome)]) per row, in the file's order"""
    polynomial, dims = SLABS[name]
    for head in itertools.product(*dims[:2]):
        row = []
        for tail in itertools.product(*dims[2:]):
            f = dict(BASE)
            for _, over in head + tail:
                f.update(over)
            takes = f.pop("strip_takes", 0)
            f["ksel"] = int(f["have"] and f["on"] != 0)          # (known_flags: the selections come with a one-pass spec)
            if polynomial and not f["fold"]:
                f["strip_pass2"] = 0                             # (the last step stores another type than fp32 then)
            row.append((f, takes))
        yield " ".join(label for label, _ in head), row


@pytest.fixture(scope="module")
def lib():
    from polyblur_amd import _capi as capi
    if not os.path.exists(capi.library_path()):
        from polyblur_amd.build import build
        build(verbose=False)
    return capi.load_library()


_out = (ctypes.c_int * (8 * MAX_OPS))()


def query(lib, polynomial, facts):
    """the plan as a tuple of ops, each a tuple of OP_FIELDS"""
    arr = (ctypes.c_int * len(FACTS))(*[facts[k] for k in FACTS])
    n = lib.pb_debug_poly_plan(polynomial, arr, len(FACTS), _out, MAX_OPS)
    assert n >= 0, (n, polynomial, facts)
    v = _out[:8 * n]
    return tuple(tuple(v[i:i + 8]) for i in range(0, 8 * n, 8))


def as_recorded(plan, strip_takes):
    """the plan as a recording of the launchers shows it: the stencil launch that waits for the strip body's answer issued or not; a
    refusing plan is its message (nothing of it is issued)"""
    if plan and plan[-1][0] == FAIL:
        return ((FAIL, 0, 0, 0, 0, 0, 0, plan[-1][7]),)
    out, stripped = [], set()
    for op in plan:
        op = list(op)
        if op[0] == STRIP:
            stripped.add(op[1])
        if op[0] == STENCIL:
            if op[7] == WHEN_STRIP_REFUSED and strip_takes and op[1] in stripped:
                continue
            op[7] = 0
        out.append(tuple(op))
    return tuple(out)


def run_sweep(lib):
    """{slab: {row key: [(facts, strip outcome, plan)]}}"""
    return {name: {key: [(f, t, query(lib, SLABS[name][0], f)) for f, t in row] for key, row in slab_cases(name)} for name in SLABS}


@pytest.fixture(scope="module")
def sweep(lib):
    return run_sweep(lib)


LETTERS = "ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz"
OP_LETTERS = LETTERS + "0123456789!#$%&()*+,-./:;<=>?@[]^_{|}~"


def golden_form(recorded):
    """recorded: {slab: {row key: [plan as recorded]}} -> the file's form, kept small: every distinct op once ("ops"), every distinct
    plan once as a string of one character per op ("plans"), and per row of a slab the cases in order as two letters per plan, followed
    by a count where the plan repeats; a row equal to an earlier one of its slab is "=" and that row's key"""
    ops, op_index, plans, index, slabs = [], {}, [], {}, {}
    for name, rows in recorded.items():
        slabs[name] = {"polynomial": SLABS[name][0], "dims": [[label for label, _ in d] for d in SLABS[name][1]], "rows": {}}
        seen = {}
        for key, row in rows.items():
            codes = []
            for plan in row:
                if plan not in index:
                    for op in plan:
                        if op not in op_index:
                            op_index[op] = len(ops)
                            ops.append(list(op))
                    index[plan] = len(plans)
                    plans.append("".join(OP_LETTERS[op_index[op]] for op in plan))
                i = index[plan]
                codes.append(LETTERS[i // 52] + LETTERS[i % 52])
            text = "".join(c + (str(n) if n > 1 else "") for c, n in ((c, len(list(g))) for c, g in itertools.groupby(codes)))
            slabs[name]["rows"][key] = "=" + seen[text] if text in seen else text
            seen.setdefault(text, key)
    assert len(ops) <= len(OP_LETTERS) and len(plans) <= 52 * 52
    return {"facts": list(FACTS), "op_fields": list(OP_FIELDS), "ops": ops, "plans": plans, "slabs": slabs}


def expand(g, name, key):
    rows = g["slabs"][name]["rows"]
    s = rows[key]
    if s.startswith("="):
        s = rows[s[1:]]
    out = []
    for code, count in re.findall(r"([A-Za-z]{2})(\d*)", s):
        plan = tuple(tuple(g["ops"][OP_LETTERS.index(c)]) for c in g["plans"][LETTERS.index(code[0]) * 52 + LETTERS.index(code[1])])
        out += [plan] * int(count or 1)
    return out


def recorded_form(sweep):
    return {name: {key: [as_recorded(plan, t) for _, t, plan in row] for key, row in rows.items()} for name, rows in sweep.items()}


def test_sweep_equals_the_recorded_plans(sweep):
    want = json.load(open(GOLDEN))
    assert want["facts"] == list(FACTS) and want["op_fields"] == list(OP_FIELDS)
    assert sorted(want["slabs"]) == sorted(SLABS)
    for name, rows in sweep.items():
        w = want["slabs"][name]
        assert w["dims"] == [[label for label, _ in d] for d in SLABS[name][1]], name
        assert sorted(w["rows"]) == sorted(rows), name
        for key, row in rows.items():
            rec = expand(want, name, key)
            assert len(rec) == len(row), (name, key)
            for (f, t, plan), r in zip(row, rec):
                assert as_recorded(plan, t) == r, (name, key, {k: v for k, v in f.items() if v != BASE[k]}, t, as_recorded(plan, t), r)


def test_plans_are_consistent(sweep):
    for name, rows in sweep.items():
        for key, row in rows.items():
            for f, _, plan in row:
                where = (name, key, {k: v for k, v in f.items() if v != BASE[k]}, plan)
                kinds = [op[0] for op in plan]
                assert len(plan) <= 16, where
                assert FAIL not in kinds[:-1], where
                side = [i for i, op in enumerate(plan) if op[4]]
                if FORK in kinds or side:
                    assert f["aux"] and not f["prof_on"], where
                    assert kinds.count(FORK) == 1 and (kinds.count(JOIN) == 1 or (kinds[-1] == FAIL and JOIN not in kinds)), where
                    assert kinds[-1] == FAIL or side, where
                    assert not side or kinds.index(FORK) < side[0], where
                    if JOIN in kinds:
                        assert kinds.index(JOIN) > side[-1], where
                        assert side == list(range(side[0], side[-1] + 1)), where      # (one run of side-stream ops: one record, one wait)
                else:
                    assert JOIN not in kinds, where
                for kind, step, poly, ring, on_side, known, spectra, arg in plan:
                    whole = step == WHOLE
                    if kind == WAVE:
                        assert f["whole_wave_types"] if whole else f["wave_types%d" % step], where
                    if kind == WG:
                        assert f["whole_wg_types"] if whole else f["wg_types%d" % step], where
                    if kind == WIN:
                        assert whole and f["whole_win_types"] and poly == 1, where
                    if kind == STRIP:
                        assert f["strip_mode"] and f["strip_pass%d" % step] and f["any_strip"], where
                    if kind in LAUNCHES and kind != STENCIL and kind != STRIP:
                        assert spectra != 0, where                                     # (a window launch without spectra)
                    if known:
                        assert f["ksel"], where


def test_every_op_and_every_refusal_is_reached(sweep):
    kinds, messages, longest = set(), set(), 0
    for rows in sweep.values():
        for row in rows.values():
            for _, _, plan in row:
                longest = max(longest, len(plan))
                for op in plan:
                    kinds.add(op[0])
                    if op[0] == FAIL:
                        messages.add(op[7])
    assert kinds == set(range(1, 13)), sorted(set(range(1, 13)) - kinds)
    assert messages == set(range(MESSAGES)), sorted(messages)
    assert longest <= 16, longest


def test_bad_arguments_are_refused(lib):
    arr = (ctypes.c_int * len(FACTS))(*[BASE[k] for k in FACTS])
    assert lib.pb_debug_poly_plan(1, arr, len(FACTS) - 1, _out, MAX_OPS) < 0
    assert lib.pb_debug_poly_plan(1, None, len(FACTS), _out, MAX_OPS) < 0
    assert lib.pb_debug_poly_plan(1, arr, len(FACTS), None, MAX_OPS) < 0
    assert lib.pb_debug_poly_plan(1, arr, len(FACTS), _out, 1) < 0         # (the plan is longer than one op)
    bad = dict(BASE, ring=6)
    assert lib.pb_debug_poly_plan(0, (ctypes.c_int * len(FACTS))(*[bad[k] for k in FACTS]), len(FACTS), _out, MAX_OPS) < 0


def write_golden(g, path=GOLDEN):
    """one row per line: a change reads as a diff"""
    with open(path, "w") as f:
        f.write('{"facts": %s,\n"op_fields": %s,\n"ops": %s,\n"plans": %s,\n"slabs": {\n' % (
            json.dumps(g["facts"]), json.dumps(g["op_fields"]), json.dumps(g["ops"]).replace(" ", ""), json.dumps(g["plans"])))
        blocks = []
        for name, s in g["slabs"].items():
            blocks.append('%s: {"polynomial": %d, "dims": %s, "rows": {\n%s\n}}' % (
                json.dumps(name), s["polynomial"], json.dumps(s["dims"]), ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in s["rows"].items())))
        f.write(",\n".join(blocks) + "\n}}\n")
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    sys.path.insert(0, REPO)
    if "--cases" in sys.argv:
        with open(sys.argv[sys.argv.index("--cases") + 1], "w") as out:
            for name in SLABS:
                for _, row in slab_cases(name):
                    for f, t in row:
                        out.write("%d %d %s\n" % (SLABS[name][0], t, " ".join(str(f[k]) for k in FACTS)))
    if "--record" in sys.argv:
        from polyblur_amd import _capi
        write_golden(golden_form(recorded_form(run_sweep(_capi.load_library()))))
