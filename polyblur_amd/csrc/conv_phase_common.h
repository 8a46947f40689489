// What the pure-phase polynomial (conv_phase.hip) and its backward (conv_phase_grad.hip) share on the host and between their
// kernels: how planes are paired into slots, how many lines a workgroup takes, which instantiation a footprint gets.  One
// statement of each, so that both directions tile a domain the same way.
#pragma once
#include "common.h"
#include "fft.h"

namespace {

constexpr size_t kPhaseMaxLds = 160 * 1024;

// slot `g` of the call: planes 2q and 2q + 1 of image g / spi, the second one missing where C is odd
__device__ __forceinline__ void phase_slot(int g, int C, long &plane, bool &two) {
    const int spi = (C + 1) >> 1;
    const int b = g / spi, q = g - b * spi;
    plane = (long)b * C + 2 * q;
    two = 2 * q + 1 < C;
}

size_t phase_lds(const FftPlan *pl, int lognb) { return ((size_t)(pl->bluestein_m ? pl->bluestein_m : pl->n) << lognb) * sizeof(float2); }

// rows: a few lines per workgroup while they fit 32 KB (short lines would leave most of a workgroup idle)
int phase_rows_lognb(const FftPlan *pl, int rows) {
    int lognb = 3;
    while (lognb > 0 && (phase_lds(pl, lognb) > 32 * 1024 || (1 << lognb) > 2 * rows)) --lognb;
    return lognb;
}
// columns: the widest tile, up to 16 columns (128 bytes of a complex row), whose lines fit 80 KB -- two workgroups per CU;
// where not even two lines do (Bluestein cores of 8192), two lines in one workgroup if LDS holds them: 16 contiguous bytes
// per row instead of 8
int phase_cols_lognb(const FftPlan *pl, int cols) {
    int lognb = 4;
    while (lognb > 0 && (phase_lds(pl, lognb) > 80 * 1024 || (1 << lognb) > 2 * cols)) --lognb;
    if (lognb == 0 && cols > 1 && phase_lds(pl, 1) <= kPhaseMaxLds) lognb = 1;
    return lognb;
}
// a workgroup's transform is a chain of dependent stages: large LDS footprints leave room for one workgroup per CU, which
// then runs 1024 threads
bool phase_wide(size_t lds) { return lds >= 128 * 1024; }

// one launch of the 256- or the 1024-thread instantiation of a kernel, by its LDS footprint
template <typename K, typename... A>
int phase_launch(pb_ctx *ctx, K k256, K k1024, dim3 grid, size_t lds, A... args) {
    const bool wide = phase_wide(lds);
    K k = wide ? k1024 : k256;
    if (lds > 48 * 1024)
        PB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(k, grid, dim3(wide ? 1024 : 256), lds, ctx->stream, args...);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace
