// The host-side plan of a reblurring call (csrc/poly_choice.h: choose_pass / choose_poly) as a program of its own, over a wider
// grid than tests/test_poly_choice_cpu.py asks through the library -- the knobs, streams, specs, boundary, fold, records and
// scratch states as a full product, with every single and every pair of the 20 predicate facts false -- for a sanitizer, which
// cannot see code loaded into python:
//   c++ -std=c++17 -O1 -g -fsanitize=address,undefined tools/poly_choice_sweep.cpp -o /tmp/poly_sweep && /tmp/poly_sweep
#include "../polyblur_amd/csrc/poly_choice.h"
#include <cstdio>
#include <cstring>

static long n_plans, kinds[PB_OP_KINDS], messages[PB_MSG_COUNT], checksum;
static int longest;

// what the issuing loop relies on
static bool consistent(const PolyFacts &f, const PolyPlan &pl) {
    if (pl.overflow || pl.n > PB_POLY_MAX_OPS) return false;      // (an empty plan: records the host has read, none of which any launch is for)
    int forks = 0, joins = 0, last_side = -1;
    bool ring_built = false, built = false;
    for (int i = 0; i < pl.n; ++i) {
        const PolyOp &o = pl.op[i];
        if (o.kind < 1 || o.kind >= PB_OP_KINDS || o.step > PB_PASS_WHOLE || o.poly > 2 || o.ring > 5 || o.set > PB_SET_RING) return false;
        if (o.kind == PB_OP_FAIL && (i != pl.n - 1 || o.arg >= PB_MSG_COUNT)) return false;
        if (o.kind == PB_OP_FORK) { if (forks++ || !f.aux || f.prof_on) return false; }
        if (o.kind == PB_OP_JOIN) { if (!forks || joins++ || last_side < 0) return false; }
        if (o.side) { if (!forks || joins) return false; last_side = i; }
        if (o.kind == PB_OP_BUILD) built = true;
        if (o.kind == PB_OP_BUILD_RING) ring_built = true;
        if (o.set == PB_SET_FIRST && !built) return false;          // a pass never gets spectra no op has built
        if (o.set == PB_SET_RING && !ring_built) return false;
        const bool whole = o.step == PB_PASS_WHOLE;
        if (o.kind == PB_OP_WAVE && !(whole ? f.whole_wave_types : f.wave_types[o.step])) return false;
        if (o.kind == PB_OP_WG && !(whole ? f.whole_wg_types : f.wg_types[o.step])) return false;
        if (o.kind == PB_OP_WIN && !(whole && f.whole_win_types)) return false;
        if (o.known && !f.ksel) return false;
        ++kinds[o.kind];
        if (o.kind == PB_OP_FAIL) ++messages[o.arg];
        checksum += (i + 1) * (o.kind + 3 * o.step + 5 * o.poly + 7 * o.ring + 11 * o.side + 13 * o.known + 17 * o.set + 19 * o.arg);
    }
    if (forks && !joins && !pl.failed()) return false;
    ++n_plans;
    if (pl.n > longest) longest = pl.n;
    return true;
}

int main() {
    const int specs[9][2] = {{0, 0}, {0, 1}, {1, 0}, {1, 1}, {2, 0}, {2, 1}, {3, 0}, {3, 1}, {0, 2}};
    const int records[9][5] = {{0, 0, 0, 0, 0}, {1, 0, 0, 0, 0}, {1, 0, 0, 0, 1}, {0, 1, 0, 1, 0}, {1, 1, 0, 1, 0}, {1, 1, 0, 1, 1}, {0, 1, 1, 0, 0}, {0, 1, 1, 1, 0}, {1, 1, 1, 0, 1}};
    const int scratch[8][3] = {{0, 0, PB_SPECTRA_STALE}, {0, 0, PB_SPECTRA_SECOND}, {1, 0, PB_SPECTRA_READY}, {1, 1, PB_SPECTRA_READY},
                               {1, 0, PB_SPECTRA_STALE}, {1, 1, PB_SPECTRA_STALE}, {1, 0, PB_SPECTRA_SECOND}, {1, 1, PB_SPECTRA_SECOND}};
    constexpr int NPRED = 20;       // step_ok .. wg_types (12), whole_ok .. whole_win_types (5), strip_pass (3)
    for (int knobs = 0; knobs < 24; ++knobs) for (int streams = 0; streams < 8; ++streams) for (const auto &sp : specs)
        for (int zf = 0; zf < 4; ++zf) for (int r = 0; r < 10; ++r) for (const auto &sc : scratch)
            for (int a = -1; a < NPRED; ++a) for (int b = a; b < NPRED; ++b) {
                if (a < 0 && b > a) continue;           // (-1, -1): every predicate true
                PolyFacts f = {};
                f.fft_on = knobs & 1; f.fft_wave = knobs >> 1 & 1; f.strip_mode = knobs >> 2 & 1; f.poly_one_launch = knobs >> 3;
                f.aux = streams & 1; f.prof_on = streams >> 1 & 1; f.side_tiles = streams >> 2;
                f.on = sp[0]; f.always = sp[1]; f.zero = zf & 1; f.fold = zf >> 1;
                if (r) { const int *k = records[r - 1]; f.have = 1; f.any_fft = k[0]; f.any_other = k[1]; f.any_strip = k[2]; f.any_tile = k[3]; f.any_fft3 = k[4]; f.ksel = f.on != 0; }
                f.held = sc[0]; f.by_estimate = sc[1]; f.spectra = sc[2];
                int v[PB_POLY_NFACTS];                  // (facts 6 - 25: step_ok, wave_types, wave_fits, wg_types, strip_pass, then the composite's five)
                std::memcpy(v, &f, sizeof f);
                for (int i = 0; i < NPRED; ++i) v[6 + i] = i != a && i != b;
                std::memcpy(&f, v, sizeof f);
                if (!consistent(f, choose_poly(f))) { std::printf("inconsistent polynomial plan: knobs %d streams %d spec %d %d zf %d records %d false %d %d\n", knobs, streams, sp[0], sp[1], zf, r, a, b); return 1; }
                if (zf || streams || (a >= 0 && a % 3) || (b >= 0 && b % 3)) continue;       // the single pass: step 0's facts, neither stream nor boundary
                for (int call = 0; call < 24; ++call) {
                    f.khat_ready = call & 1; f.no_fft = call >> 1 & 1; f.poly = (call >> 2 & 1) * 2; f.ring = call >> 3 ? 3 + (call >> 3) : 0;
                    if (!consistent(f, choose_pass(f))) { std::printf("inconsistent pass plan: knobs %d spec %d %d records %d false %d %d call %d\n", knobs, sp[0], sp[1], r, a, b, call); return 1; }
                }
            }
    std::printf("%ld plans, longest %d ops, checksum %ld\nops by kind:", n_plans, longest, checksum);
    for (int k = 1; k < PB_OP_KINDS; ++k) std::printf(" %ld", kinds[k]);
    std::printf("\nrefusals by message:");
    for (long m : messages) std::printf(" %ld", m);
    std::printf("\n");
    for (int k = 1; k < PB_OP_KINDS; ++k) if (!kinds[k]) { std::printf("op kind %d never planned\n", k); return 1; }
    for (int m = 0; m < PB_MSG_COUNT; ++m) if (!messages[m]) { std::printf("message %d never raised\n", m); return 1; }
    return 0;
}
