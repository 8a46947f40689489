// The gradient of a reblurring pass with respect to its taps: the lag correlation
//
//     D[dy][dx] = sum over the C planes of an image, over every sample p of the domain, of  u[p] * v[p + (dy, dx)],
//     |dy| <= kh / 2, |dx| <= kw / 2 (kh, kw odd, up to 49 x 49 = 2401 lags),
//
// v zero outside the H x W domain (PB_ZERO) or read at indices taken modulo it (PB_WRAP).  With u the upstream gradient and v
// the operand of the pass this is d loss / d taps of filters.convolve2d (filters.py:14-37) -- tap (i, j) of the zero form sits
// at lag (i - kh / 2, j - kw / 2), of the wrap form at lag (kh / 2 - i, kw / 2 - j), api.hip: pb_taps_create -- and three of
// them make the tap gradient of deblurring.compute_polynomial (deblurring.py:113-169).  The reference gets both from ATen's
// autograd (README, "Import into your projects": "fully differentiable").
//
// Deterministic: no float atomics (their sums depend on arrival order).  Image b gets G workgroups; workgroup g walks the tiles
// g, g + G, g + 2 G ... of the image's C planes in that order and keeps every lag it owns -- lags tid, tid + 256, ... -- in a
// register; one partial table per workgroup goes to context scratch (B * G * kh * kw floats) and tap_grad_reduce sums the G
// partials of a lag in index order, scales, and stores or accumulates.  Same inputs, same bits.
//
// A tile is 32 x 32 samples of u and the (32 + kh - 1) x (32 + kw - 1) samples of v around it, both in LDS (at most 30016
// bytes); halo samples are zeros or wrapped reads at load time, so domains smaller than a tile or than the halo need nothing
// special.  The v tile's pitch is kw + 32 words: the lane that owns lag l = i * kw + j reads word i * (kw + 32) + j = l + 32 i
// past the sample, i.e. bank l mod 32 -- the 32 lanes of a ds_read_b32 group hit 32 different banks whatever kw is.  The u
// sample is one address for the whole wave (a broadcast), read four at a time.  fp32 accumulation in three levels -- a tile row,
// a tile, the workgroup's tiles -- so that no chain of additions is longer than 32 rows or the workgroup's tile count.
#include <algorithm>

#include "common.h"

namespace {

constexpr int TG_NT = 256, TG_T = 32, TG_R = 24;

template <int NL>
__global__ __launch_bounds__(TG_NT) void tap_grad_kernel(const float *__restrict__ u, const float *__restrict__ v, float *__restrict__ partial,
                                                        int C, int H, int W, int kh, int kw, int wrap, int G, int tiles_x, int tiles_y) {
    extern __shared__ __attribute__((aligned(16))) float tg_lds[];
    float *ut = tg_lds, *vt = tg_lds + TG_T * TG_T;
    const int ry = kh / 2, rx = kw / 2, nlags = kh * kw;
    const int pitch = kw + TG_T, vrows = TG_T + 2 * ry, vcols = TG_T + 2 * rx;
    const int img = blockIdx.x / G, g = blockIdx.x - img * G;
    const int tid = threadIdx.x;
    int off[NL];
    float tot[NL];
#pragma unroll
    for (int n = 0; n < NL; ++n) {
        const int lag = tid + TG_NT * n, l = lag < nlags ? lag : 0;      // (a lag beyond the table: reads lag 0's samples, stores nothing)
        off[n] = (l / kw) * pitch + l % kw;
        tot[n] = 0.f;
    }
    const int tpp = tiles_x * tiles_y, tiles = C * tpp;
    for (int t = g; t < tiles; t += G) {
        const int c = t / tpp, r = t - c * tpp, ty = r / tiles_x, tx = r - ty * tiles_x;
        const int y0 = ty * TG_T, x0 = tx * TG_T;
        const long plane = ((long)img * C + c) * (long)H * W;
        const float *up = u + plane, *vp = v + plane;
        __syncthreads();                                                  // (the previous tile has been read)
        for (int i = tid; i < TG_T * TG_T; i += TG_NT) {
            const int gy = y0 + (i >> 5), gx = x0 + (i & 31);
            ut[i] = (gy < H && gx < W) ? up[(long)gy * W + gx] : 0.f;
        }
        for (int rr = tid >> 6; rr < vrows; rr += TG_NT / 64) {
            int gy = y0 - ry + rr;
            if (wrap) { gy %= H; if (gy < 0) gy += H; }
            const bool yin = gy >= 0 && gy < H;
            for (int cc = tid & 63; cc < vcols; cc += 64) {
                int gx = x0 - rx + cc;
                if (wrap) { gx %= W; if (gx < 0) gx += W; }
                vt[rr * pitch + cc] = (yin && gx >= 0 && gx < W) ? vp[(long)gy * W + gx] : 0.f;
            }
        }
        __syncthreads();
        const int th = min(TG_T, H - y0), tw4 = (min(TG_T, W - x0) + 3) >> 2;     // (the tile's live rows and groups of four columns)
        float acc[NL];
#pragma unroll
        for (int n = 0; n < NL; ++n) acc[n] = 0.f;
        for (int y = 0; y < th; ++y) {
            float row[NL];
#pragma unroll
            for (int n = 0; n < NL; ++n) row[n] = 0.f;
            const float *ur = ut + y * TG_T, *vr = vt + y * pitch;
            for (int xg = 0; xg < tw4; ++xg) {
                const float4 u4 = *reinterpret_cast<const float4 *>(ur + 4 * xg);
#pragma unroll
                for (int n = 0; n < NL; ++n) {
                    const float *q = vr + 4 * xg + off[n];
                    row[n] = fmaf(u4.x, q[0], row[n]);
                    row[n] = fmaf(u4.y, q[1], row[n]);
                    row[n] = fmaf(u4.z, q[2], row[n]);
                    row[n] = fmaf(u4.w, q[3], row[n]);
                }
            }
#pragma unroll
            for (int n = 0; n < NL; ++n) acc[n] += row[n];
        }
#pragma unroll
        for (int n = 0; n < NL; ++n) tot[n] += acc[n];
    }
    float *out = partial + (long)blockIdx.x * nlags;
#pragma unroll
    for (int n = 0; n < NL; ++n) {
        const int lag = tid + TG_NT * n;
        if (lag < nlags) out[lag] = tot[n];
    }
}

// grad[b][i][j] (= or +=) scale * sum over g, in index order, of partial[b][g][lag]; flip: tap (i, j) sits at lag
// (kh / 2 - i, kw / 2 - j) -- the wrap form -- instead of (i - kh / 2, j - kw / 2)
__global__ __launch_bounds__(TG_NT) void tap_grad_reduce(const float *__restrict__ partial, float *__restrict__ grad, int G, int nlags, int flip,
                                                        float scale, int accumulate, int total) {
    const int idx = blockIdx.x * TG_NT + threadIdx.x;
    if (idx >= total) return;
    const int b = idx / nlags, lag = idx - b * nlags;
    const float *p = partial + (long)b * G * nlags + lag;
    float s = 0.f;
    for (int g = 0; g < G; ++g) s += p[(long)g * nlags];
    float *o = grad + (long)b * nlags + (flip ? nlags - 1 - lag : lag);
    const float val = scale * s;
    *o = accumulate ? *o + val : val;
}

}  // namespace

// how many workgroups an image's tiles are dealt to: all of them, or about four per compute unit over the batch
int pb_tap_gradient_groups(int B, int C, int H, int W) {
    const long tiles = (long)C * ((H + TG_T - 1) / TG_T) * ((W + TG_T - 1) / TG_T);
    const long cap = std::max(1, 1024 / std::max(B, 1));
    return (int)std::min(tiles, cap);
}

int pb_launch_tap_gradient(pb_ctx *ctx, const float *u, const float *v, int B, int C, int H, int W, int kh, int kw, int boundary,
                           float scale, int accumulate, float *grad) {
    if (kh < 1 || kw < 1 || !(kh & 1) || !(kw & 1) || kh / 2 > TG_R || kw / 2 > TG_R)
        return pb_fail(ctx, PB_ERR_BADARG, "tap gradient: bad size %d x %d", kh, kw);
    const int nlags = kh * kw, G = pb_tap_gradient_groups(B, C, H, W);
    const long blocks = (long)B * G;
    if (blocks > 0x7fffffffL || (long)B * nlags > 0x7fffffffL) return pb_fail(ctx, PB_ERR_BADARG, "tap gradient: bad grid");
    float *partial = static_cast<float *>(pb_scratch(ctx, "grad.partial", sizeof(float) * (size_t)blocks * nlags));
    if (!partial) return PB_ERR_NOMEM;
    ProfScope prof(ctx, PB_PROF_OTHER);
    const int tiles_x = (W + TG_T - 1) / TG_T, tiles_y = (H + TG_T - 1) / TG_T;
    const size_t lds = sizeof(float) * (size_t)(TG_T * TG_T + (TG_T + 2 * (kh / 2)) * (kw + TG_T));
    const int wrap = boundary == PB_WRAP ? 1 : 0;
    const dim3 grid((unsigned)blocks), block(TG_NT);
    if (nlags <= TG_NT)
        hipLaunchKernelGGL(tap_grad_kernel<1>, grid, block, lds, ctx->stream, u, v, partial, C, H, W, kh, kw, wrap, G, tiles_x, tiles_y);
    else if (nlags <= 3 * TG_NT)
        hipLaunchKernelGGL(tap_grad_kernel<3>, grid, block, lds, ctx->stream, u, v, partial, C, H, W, kh, kw, wrap, G, tiles_x, tiles_y);
    else
        hipLaunchKernelGGL(tap_grad_kernel<10>, grid, block, lds, ctx->stream, u, v, partial, C, H, W, kh, kw, wrap, G, tiles_x, tiles_y);
    PB_LAUNCH_CHECK();
    const int total = B * nlags;
    hipLaunchKernelGGL(tap_grad_reduce, dim3((unsigned)((total + TG_NT - 1) / TG_NT)), block, 0, ctx->stream, partial, grad, G, nlags, wrap, scale,
                       accumulate, total);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
