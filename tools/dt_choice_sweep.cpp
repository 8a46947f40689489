// The host-side choice of the domain-transform filter (csrc/dt_choice.h: choose_dt) as a program of its own, over the grid of
// tests/test_dt_choice_cpu.py as a full product -- every threshold's two sides, the 2 GiB edges of the size arithmetic included --
// for a sanitizer, which cannot see code loaded into python:
//   c++ -std=c++17 -g -fsanitize=address,undefined tools/dt_choice_sweep.cpp -o /tmp/dt_sweep && /tmp/dt_sweep
#include "../polyblur_amd/csrc/dt_choice.h"
#include <cstdio>
#include <initializer_list>

int main() {
    const int widths[] = {2, 254, 256, 257, 260, 1024, 1025, 2048, 2049, 4096, 4097, 8192, 8193, 65536};
    const int heights[] = {1, 63, 64, 127, 128, 4096, 4100, 21845, 21846, 65536};
    const int batches[] = {1, 2, 3, 4, 6, 7, 12, 13, 24, 25, 1024};
    const DtKnobs knobs[] = {{1, 1, 1}, {0, 1, 1}, {2, 1, 1}, {3, 1, 1}, {1, 0, 0}, {1, 2, 0}, {1, 1, 0}, {1, 1, 2}};
    long n = 0, forms[3][4] = {}, sum = 0;
    for (const DtKnobs &k : knobs) for (int elem : {4, 2}) for (int C : {1, 3}) for (int self = 0; self < 2; ++self) for (int al = 0; al < 2; ++al)
        for (int B : batches) for (int H : heights) for (int W : widths) {
            const DtChoice c = choose_dt(k, elem, C, B, H, W, self != 0, al != 0);
            const long samples = (long)B * C * H * W;
            // what the launcher relies on: scratch that holds what the kernels index, never more than the image itself plus a strip
            bool ok = c.carry >= 0 && c.weights >= 0 && c.carry <= samples + (long)B * C * 64 * ((W + 63) / 64 * 64) && c.weights <= samples;
            if (c.cols == PB_DT_COLS_COOPERATIVE) ok = ok && c.lds > 0 && c.lds <= 160 * 1024 && (long)C * H * W * 4 < (1l << 31) && c.cols_rows == dtc_rows(C);
            else ok = ok && c.lds == 0;
            if (c.rows == PB_DT_ROWS_WAVE) ok = ok && self && W <= 64 * c.chunks;
            if (c.rows == PB_DT_ROWS_WORKGROUP) ok = ok && self && W <= 256 * c.chunks;
            if (!ok) { std::printf("inconsistent choice: knobs %d %d %d elem %d C %d self %d aligned %d B %d H %d W %d\n", k.rows_reg, k.cols_strip, k.cols_coop, elem, C, self, al, B, H, W); return 1; }
            ++n; ++forms[c.rows][c.cols];
            sum += c.chunks + c.cols_rows + c.carry % 1000 + c.weights % 1000 + c.lds;
        }
    std::printf("%ld choices, checksum %ld\nrows x cols:", n, sum);
    for (auto &r : forms) for (long v : r) std::printf(" %ld", v);
    std::printf("\n");
    return 0;
}
