// The host half of the line transforms' choice (csrc/line_choice.h: plans, compiled tables, choosers) as a program of its own,
// over the lengths, batch sizes and uses of tests/test_line_choice_cpu.py -- for a sanitizer, which cannot see code loaded
// into python:  c++ -std=c++17 -g -fsanitize=address,undefined tools/line_choice_sweep.cpp -o /tmp/sweep && /tmp/sweep
#include "../polyblur_amd/csrc/line_choice.h"
#include <cstdio>

int main() {
    std::vector<int> lens = {7680, 700, 500, 37, 75, 97, 101, 3240, 24, 8200, 10, 20736, 32};
#define LEN(N_, ...) lens.push_back(N_);
    PB_COLS_PLANS(LEN) PB_ROWS_PLANS(LEN)
    long n = 0, compiled = 0, sum = 0;
    for (int env = 0; env < 4; ++env) {
        LineKnobs k;
        k.cols_fixed = k.rows_fixed = !(env & 1); k.fft_ext_radix = !(env & 2); k.fft_first = k.fft_first_rows = env == 3 ? 0 : -1;
        for (int a : lens) for (int b : lens) for (int P : {1, 2, 6, 8, 13, 32, 64, 200}) {
            HostPlans memo;                                   // (fresh: every plan is factorized in this run)
            for (int C : {0, 1, 3, 4}) for (int t = 0; t < 3; ++t) for (int nz = 0; nz < 2; ++nz) {
                LineUse u; u.C = C; u.in_dtype = t; u.out_dtype = C ? 0 : t % 2; u.normalize = nz;
                const LineChoice r = choose_rows(memo, k, a, b, P, u);
                u.C = 0; u.maxima = C != 0; u.n_angles = C == 4 ? 11 : 6; u.discard_sat = t == 2;
                const LineChoice c = choose_cols(memo, k, a, b, P, u);
                n += 2; compiled += (r.kind == PB_LINE_COMPILED) + (c.kind == PB_LINE_COMPILED);
                sum += r.threads + r.lds + r.plan.radix[r.plan.nstage - 1] + c.tiles + c.lds + c.plan.radix[c.plan.nstage - 1];
            }
        }
    }
    std::printf("%ld choices, %ld compiled, checksum %ld\n", n, compiled, sum);
    return 0;
}
