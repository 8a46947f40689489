// The bilateral filter with any odd window up to 25 x 25 (filters.py:107-148): per plane, replicate pad of ksize / 2, the weight
// of a tap exp(-(dx^2 + dy^2) / (2 sigma_spatial^2)) exp(-(v - centre)^2 / (2 sigma_color^2)), out = sum w v / (sum w + 1e-5).
// ksize == 5 is filters.hip's bilateral5_kernel with the caller's two sigma; every other size takes bilateral_kernel below.
#include <climits>
#include <cmath>

#include "common.h"

int pb_bilateral5_sigma_impl(pb_ctx *ctx, const void *in, int in_dtype, void *out, int out_dtype, int P, int H, int W,
                             double sigma_space, double sigma_color);

namespace {

constexpr int NT = 256;
constexpr int TWB = 64, THB = 16;                      // outputs of a workgroup
constexpr int PER = THB / (NT / TWB);                  // vertically adjacent outputs of a thread
constexpr int RMAX = PB_KSIZE / 2;
constexpr int LW_MAX = TWB + 2 * RMAX, LH_MAX = THB + 2 * RMAX;        // 88 x 40 floats: 14 KB

// One row of a thread's window: the 2 R + 1 samples at `row` go to outputs LO .. HI of the thread's PER, the ones whose windows
// hold that row -- one LDS read per sample for all of them.  ey[o] = dy^2 ks1 of this row for output o.  The weight is one
// exponential, as in bilateral5_kernel: exp2(d^2 kc + (dx^2 + dy^2) ks1).
template <int LO, int HI>
__device__ __forceinline__ void window_row(const float *__restrict__ row, int R, float kc, float ks1, const float (&ctr)[PER],
                                           const float (&ey)[PER], float (&num)[PER], float (&den)[PER]) {
    float dx = (float)-R;
    for (int j = 0; j <= 2 * R; ++j) {
        const float v = row[j];
        const float dx2 = dx * dx;
        dx += 1.f;
#pragma unroll
        for (int o = LO; o <= HI; ++o) {
            const float d = v - ctr[o];
            const float w = __builtin_amdgcn_exp2f(fmaf(d * d, kc, fmaf(dx2, ks1, ey[o])));
            num[o] = fmaf(w, v, num[o]);
            den[o] += w;
        }
    }
}

// One workgroup per 64 x 16 tile of outputs: the tile and its halo of R samples go to LDS once ((64 + 2 R) x (16 + 2 R) floats),
// a thread forms PER = 4 vertically adjacent outputs of one column and walks the 4 + 2 R rows their windows cover: rows
// 3 .. 2 R serve all four outputs, the first and last three serve the outputs that reach them (the choice is the same for every
// lane: a scalar branch per row).  A wave reads 64 consecutive floats of one LDS row: no bank conflicts for any R.
template <typename T>
__global__ __launch_bounds__(NT) void bilateral_kernel(const T *__restrict__ in, T *__restrict__ out, int P, int H, int W, int R,
                                                       float kc, float ks1) {
    __shared__ float s[LH_MAX * LW_MAX];
    const int LW = TWB + 2 * R, LH = THB + 2 * R;
    const int x0 = blockIdx.x * TWB, y0 = blockIdx.y * THB;
    const int lane = threadIdx.x % TWB, wv = threadIdx.x / TWB;
    const int ty = wv * PER;                                           // outputs: rows ty .. ty + PER - 1 of the tile, column lane
    const long HW = (long)H * W;
    for (int plane = blockIdx.z; plane < P; plane += gridDim.z) {      // (grid.z is capped at 65535)
        if (plane != (int)blockIdx.z) __syncthreads();
        const T *src = in + (long)plane * HW;
        for (int r = wv; r < LH; r += NT / TWB) {
            const int yy = min(max(y0 + r - R, 0), H - 1);             // replicate pad
            for (int c = lane; c < LW; c += TWB) {
                const int xx = min(max(x0 + c - R, 0), W - 1);
                s[r * LW + c] = pb_ld(src + (long)yy * W + xx);
            }
        }
        __syncthreads();
        float ctr[PER], num[PER], den[PER], ey[PER];
#pragma unroll
        for (int o = 0; o < PER; ++o) {
            ctr[o] = s[(ty + o + R) * LW + lane + R];
            num[o] = 0.f;
            den[o] = 0.f;
        }
        for (int r = 0; r < PER + 2 * R; ++r) {                        // output o holds window row r where 0 <= r - o <= 2 R
            const float *row = s + (ty + r) * LW + lane;
#pragma unroll
            for (int o = 0; o < PER; ++o) {
                const float dy = (float)(r - o - R);
                ey[o] = dy * dy * ks1;
            }
            const int lo = max(r - 2 * R, 0), hi = min(r, PER - 1);
            switch (lo * PER + hi) {
#define PB_ROW(LO, HI) case LO * PER + HI: window_row<LO, HI>(row, R, kc, ks1, ctr, ey, num, den); break
                PB_ROW(0, 0); PB_ROW(0, 1); PB_ROW(0, 2); PB_ROW(0, 3);
                PB_ROW(1, 1); PB_ROW(1, 2); PB_ROW(1, 3);
                PB_ROW(2, 2); PB_ROW(2, 3);
                PB_ROW(3, 3);
#undef PB_ROW
            }
        }
        const int xx = x0 + lane;
#pragma unroll
        for (int o = 0; o < PER; ++o) {
            const int yy = y0 + ty + o;
            if (yy < H && xx < W) pb_st(out + (long)plane * HW + (long)yy * W + xx, num[o] / (den[o] + 1e-5f));
        }
    }
}
static_assert(PER == 4, "window_row's cases are written for four outputs per thread");

}  // namespace

extern "C" int pb_bilateral(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W, int ksize,
                            float sigma_spatial, float sigma_color) {
    if (!ctx) return PB_ERR_BADARG;
    if (dtype != PB_F32 && dtype != PB_F16) return pb_fail(ctx, PB_ERR_BADARG, "dtype must be PB_F32 or PB_F16");
    if (B < 1 || C < 1 || H < 2 || W < 2 || (long)B * C > INT_MAX) return pb_fail(ctx, PB_ERR_BADARG, "bad shape (%d,%d,%d,%d)", B, C, H, W);
    if (!in || !out) return pb_fail(ctx, PB_ERR_BADARG, "null argument");
    if (in == out) return pb_fail(ctx, PB_ERR_BADARG, "out may not alias in");
    if (ksize < 1 || ksize > PB_KSIZE || ksize % 2 == 0) return pb_fail(ctx, PB_ERR_BADARG, "ksize must be odd, from 1 to %d (got %d)", PB_KSIZE, ksize);
    if (!(sigma_spatial > 0.f) || !(sigma_color > 0.f) || !std::isfinite(sigma_spatial) || !std::isfinite(sigma_color))
        return pb_fail(ctx, PB_ERR_BADARG, "sigma_spatial and sigma_color must be positive and finite");
    const double log2e = 1.4426950408889634;
    const float kc = (float)(-log2e / (2. * sigma_color * sigma_color)), ks1 = (float)(-log2e / (2. * sigma_spatial * sigma_spatial));   // (exp2's arguments)
    if (!std::isfinite(kc) || !std::isfinite(ks1)) return pb_fail(ctx, PB_ERR_BADARG, "sigma_spatial and sigma_color must be at least 1e-18");   // (0 x inf at the centre tap)
    PB_HIP(hipSetDevice(ctx->device));
    const int P = B * C;
    if (ksize == 5) return pb_bilateral5_sigma_impl(ctx, in, dtype, out, dtype, P, H, W, sigma_spatial, sigma_color);
    const dim3 grid((W + TWB - 1) / TWB, (H + THB - 1) / THB, P < 65535 ? P : 65535);
    ProfScope prof(ctx, PB_PROF_PREFILTER);
    if (dtype == PB_F32)
        hipLaunchKernelGGL((bilateral_kernel<float>), grid, dim3(NT), 0, ctx->stream, static_cast<const float *>(in),
                           static_cast<float *>(out), P, H, W, ksize / 2, kc, ks1);
    else
        hipLaunchKernelGGL((bilateral_kernel<__half>), grid, dim3(NT), 0, ctx->stream, static_cast<const __half *>(in),
                           static_cast<__half *>(out), P, H, W, ksize / 2, kc, ks1);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
