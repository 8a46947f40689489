// The cover sum of the windowed overlap-add (reference deblurring.py:332-340), stated once: overlap_add_kernel (filters.hip) and the
// first launch of pb_overlap_add_backward (patch_grad.hip) call it, so the backward's clamp mask comes from the very bits of the
// forward's pre-clamp value.
#pragma once

#include "common.h"

struct PatchCover { float num, den; };      // sum_n w restored_n and sum_n w over the patches n that cover one padded position

// The patches k_lo .. k_hi of one axis -- n patches of `size` samples every `step` -- that hold the padded position p (patch k covers
// k step .. k step + size - 1; a k of the range whose p - k step falls outside the patch is skipped by the caller's own test).
__device__ __forceinline__ void patch_cover_range(int p, int size, int step, int n, int &k_lo, int &k_hi) {
    k_lo = (p - size + step) / step; if (p - size + 1 <= 0) k_lo = 0;
    k_hi = min(p / step, n - 1);
}

// The patches (ki, kj) of the n_i x n_j lattice that hold the padded position (py, px), rows then columns in index order; patches
// laid out [n*B + b, c, y, x].
template <typename T>
__device__ __forceinline__ PatchCover patch_cover(const T *__restrict__ patches, int B, int C, int ph, int pw, int step_h, int step_w,
                                                  int n_i, int n_j, int b, int c, int py, int px, const float *__restrict__ win_y,
                                                  const float *__restrict__ win_x) {
    int ki_lo, ki_hi, kj_lo, kj_hi;
    patch_cover_range(py, ph, step_h, n_i, ki_lo, ki_hi);
    patch_cover_range(px, pw, step_w, n_j, kj_lo, kj_hi);
    float num = 0.f, den = 0.f;
    for (int ki = ki_lo; ki <= ki_hi; ++ki) {
        const int y = py - ki * step_h;
        if (y < 0 || y >= ph) continue;
        for (int kj = kj_lo; kj <= kj_hi; ++kj) {
            const int x = px - kj * step_w;
            if (x < 0 || x >= pw) continue;
            const float w = win_y[y] * win_x[x];
            const long n = (long)ki * n_j + kj;
            num += w * pb_ld(patches + (((n * B + b) * C + c) * ph + y) * pw + x);
            den += w;
        }
    }
    return PatchCover{num, den};
}

// the overlap-add before its clamp
__device__ __forceinline__ float patch_cover_value(const PatchCover &cv) { return cv.num / (cv.den + 1e-8f); }
