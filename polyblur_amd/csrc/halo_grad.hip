// The backward pass of halo masking: deblurring.halo_masking (deblurring.py:173-208, bug-compatible: M uses
// gy * gy, :174) and filters.fourier_gradients (filters.py:159-186) under autograd.  Per plane of H x W, with upstream g:
//
//   ox = Dx y        nM = sum gx^2 + gy^2        M = -gx ox - gy^2        r = M / (nM + M)        z = max(r, 0)
//   out = y + z (x - y)
//
//   dz = g (x - y)   q = r >= 0 ? dz / (nM + M)^2 : 0      dM = q nM      S = sum_plane -q M  (= d loss / d nM)
//   grad_x  = g z
//   grad_y  = g (1 - z) - Dx(-gx dM)                (the circulant of the spectral derivative is odd: its transpose is -Dx)
//   grad_gx = -ox dM + 2 gx S
//   grad_gy = -2 gy dM + 2 gy S
//
// (torch.clamp(min=0) passes the gradient on the closed side, r >= 0.)  Launches:
//
//   (the forward's own launchers: nM and ox again, the forward's bits)
//   halo_grad_pass1    streams the planes once: grad_x, g (1 - z) into grad_y, -ox dM and -2 gy dM into the two grad0 outputs,
//                      -gx dM into a scratch plane, per workgroup the partial sum of -q M
//   pb_fold_partials_kernel   one wave per plane folds its partials in index order: S
//   (the forward's row transform on the scratch plane, into the plane that held ox)
//   halo_grad_finish   grad_y -= T, grad_gx += 2 gx S, grad_gy += 2 gy S
//
// Whatever the NULL outputs make unnecessary is skipped.  Sums per thread in index order, then xor shuffles over the wave, the
// waves in index order through LDS, the fold in index order: no float atomics, the same call gives the same bits.
#include <algorithm>
#include <cstdint>
#include <initializer_list>

#include "stage_math.h"

int pb_grad_energy(pb_ctx *ctx, const void *gx, const void *gy, float *nM, int P, long HW, int g_dtype = PB_F32);

namespace {

constexpr int HG_NT = 256;

struct HgSample {
    float gradx, grady0, ggx0, ggy0, t, s;       // s: -q M
};

// One sample of pass one.  M, r and z are halo_kernel's own (pb_halo_ratio, stage_math.h): a sample on the kink is classified
// as the forward classified it; every rounding written out, so that both forms of the kernel give the same bits.
__device__ __forceinline__ HgSample hg_sample(float x, float y, float gx, float gy, float ox, float g, float nm) {
    const PbHalo h = pb_halo_ratio(gx, gy, ox, nm);
    const float dz = __fmul_rn(g, x - y);
    const float q = h.r >= 0.f ? dz / __fmul_rn(h.den, h.den) : 0.f;
    const float dM = __fmul_rn(q, nm);
    HgSample o;
    o.gradx = __fmul_rn(g, h.z);
    o.grady0 = g - o.gradx;
    o.ggx0 = __fmul_rn(-ox, dM);
    o.ggy0 = __fmul_rn(-2.f * gy, dM);
    o.t = __fmul_rn(-gx, dM);
    o.s = __fmul_rn(-q, h.M);
    return o;
}

// VEC: planes of whole groups of four samples on 16-byte boundaries.  One workgroup = block `blk` of `bpp` of one plane
// (blockIdx.x = plane * bpp + blk: the grid's x dimension takes any number of planes).  Outputs that are nullptr are not stored.
template <bool VEC>
__global__ __launch_bounds__(HG_NT) void halo_grad_pass1(const float *__restrict__ x, const float *__restrict__ y,
                                                         const float *__restrict__ gx, const float *__restrict__ gy,
                                                         const float *__restrict__ ox, const float *__restrict__ g,
                                                         const float *__restrict__ nM, float *__restrict__ grad_x,
                                                         float *__restrict__ grad_y, float *__restrict__ ggx, float *__restrict__ ggy,
                                                         float *__restrict__ t, float *__restrict__ partial, long HW, int bpp) {
    const int plane = blockIdx.x / bpp;
    const int blk = blockIdx.x - plane * bpp;
    const long base = (long)plane * HW;
    const float nm = nM[plane];
    float s = 0.f;
    if constexpr (VEC) {
        for (long i = 4 * ((long)blk * HG_NT + threadIdx.x); i < HW; i += 4l * bpp * HG_NT) {
            const long k = base + i;
            const float4 xv = pb_ld4(x + k), yv = pb_ld4(y + k), av = pb_ld4(gx + k), bv = pb_ld4(gy + k), ov = pb_ld4(ox + k), gv = pb_ld4(g + k);
            const HgSample e0 = hg_sample(xv.x, yv.x, av.x, bv.x, ov.x, gv.x, nm);
            const HgSample e1 = hg_sample(xv.y, yv.y, av.y, bv.y, ov.y, gv.y, nm);
            const HgSample e2 = hg_sample(xv.z, yv.z, av.z, bv.z, ov.z, gv.z, nm);
            const HgSample e3 = hg_sample(xv.w, yv.w, av.w, bv.w, ov.w, gv.w, nm);
            if (grad_x) pb_st4(grad_x + k, make_float4(e0.gradx, e1.gradx, e2.gradx, e3.gradx));
            if (grad_y) {
                pb_st4(grad_y + k, make_float4(e0.grady0, e1.grady0, e2.grady0, e3.grady0));
                pb_st4(t + k, make_float4(e0.t, e1.t, e2.t, e3.t));
            }
            if (ggx) pb_st4(ggx + k, make_float4(e0.ggx0, e1.ggx0, e2.ggx0, e3.ggx0));
            if (ggy) pb_st4(ggy + k, make_float4(e0.ggy0, e1.ggy0, e2.ggy0, e3.ggy0));
            s += e0.s; s += e1.s; s += e2.s; s += e3.s;
        }
    } else {
        for (long i = (long)blk * HG_NT + threadIdx.x; i < HW; i += (long)bpp * HG_NT) {
            const long k = base + i;
            const HgSample e = hg_sample(x[k], y[k], gx[k], gy[k], ox[k], g[k], nm);
            if (grad_x) grad_x[k] = e.gradx;
            if (grad_y) { grad_y[k] = e.grady0; t[k] = e.t; }
            if (ggx) ggx[k] = e.ggx0;
            if (ggy) ggy[k] = e.ggy0;
            s += e.s;
        }
    }
    if (!partial) return;                                        // (uniform: no grad0 output, no S)
    __shared__ float red[HG_NT / 64];
    const float v = pb_block_sum_to_first<HG_NT>(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = v;
}

// grad_y -= T;  grad_gx += 2 gx S;  grad_gy += 2 gy S          (nullptr: not asked for)
template <bool VEC>
__global__ __launch_bounds__(HG_NT) void halo_grad_finish(const float *__restrict__ gx, const float *__restrict__ gy,
                                                          const float *__restrict__ T, const float *__restrict__ S,
                                                          float *__restrict__ grad_y, float *__restrict__ ggx, float *__restrict__ ggy,
                                                          long HW, int bpp) {
    const int plane = blockIdx.x / bpp;
    const int blk = blockIdx.x - plane * bpp;
    const long base = (long)plane * HW;
    const float s2 = (ggx || ggy) ? 2.f * S[plane] : 0.f;
    if constexpr (VEC) {
        for (long i = 4 * ((long)blk * HG_NT + threadIdx.x); i < HW; i += 4l * bpp * HG_NT) {
            const long k = base + i;
            if (grad_y) {
                const float4 a = pb_ld4(grad_y + k), b = pb_ld4(T + k);
                pb_st4(grad_y + k, make_float4(a.x - b.x, a.y - b.y, a.z - b.z, a.w - b.w));
            }
            if (ggx) {
                const float4 a = pb_ld4(ggx + k), b = pb_ld4(gx + k);
                pb_st4(ggx + k, make_float4(fmaf(b.x, s2, a.x), fmaf(b.y, s2, a.y), fmaf(b.z, s2, a.z), fmaf(b.w, s2, a.w)));
            }
            if (ggy) {
                const float4 a = pb_ld4(ggy + k), b = pb_ld4(gy + k);
                pb_st4(ggy + k, make_float4(fmaf(b.x, s2, a.x), fmaf(b.y, s2, a.y), fmaf(b.z, s2, a.z), fmaf(b.w, s2, a.w)));
            }
        }
    } else {
        for (long i = (long)blk * HG_NT + threadIdx.x; i < HW; i += (long)bpp * HG_NT) {
            const long k = base + i;
            if (grad_y) grad_y[k] = grad_y[k] - T[k];
            if (ggx) ggx[k] = fmaf(gx[k], s2, ggx[k]);
            if (ggy) ggy[k] = fmaf(gy[k], s2, ggy[k]);
        }
    }
}

// out = -(out + other)  (other == nullptr: out = -out)
template <bool VEC>
__global__ __launch_bounds__(HG_NT) void neg_sum_kernel(float *__restrict__ out, const float *__restrict__ other, long n) {
    if constexpr (VEC) {
        for (long i = 4 * ((long)blockIdx.x * HG_NT + threadIdx.x); i < n; i += 4l * gridDim.x * HG_NT) {
            float4 a = pb_ld4(out + i);
            if (other) {
                const float4 b = pb_ld4(other + i);
                a = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
            }
            pb_st4(out + i, make_float4(-a.x, -a.y, -a.z, -a.w));
        }
    } else {
        for (long i = (long)blockIdx.x * HG_NT + threadIdx.x; i < n; i += (long)gridDim.x * HG_NT)
            out[i] = other ? -(out[i] + other[i]) : -out[i];
    }
}

bool hg_aligned16(std::initializer_list<const void *> ps) {
    uintptr_t u = 0;
    for (const void *p : ps) u |= reinterpret_cast<uintptr_t>(p);
    return u % 16 == 0;
}

bool hg_same(const void *a, const void *b) { return a && b && a == b; }

}  // namespace

int pb_fourier_gradients_backward_impl(pb_ctx *ctx, const float *grad_gx, const float *grad_gy, int P, int H, int W,
                                             float *grad_planes) {
    if (!grad_planes || (!grad_gx && !grad_gy)) return pb_fail(ctx, PB_ERR_BADARG, "pb_fourier_gradients_backward: null argument");
    if (hg_same(grad_planes, grad_gx) || hg_same(grad_planes, grad_gy))
        return pb_fail(ctx, PB_ERR_BADARG, "pb_fourier_gradients_backward: grad_planes may not alias an upstream gradient");
    if (P < 1 || H < 2 || W < 2) return pb_fail(ctx, PB_ERR_BADARG, "bad shape (%d,%d,%d)", P, H, W);
    if ((grad_gx && !pb_fft_length_supported(W)) || (grad_gy && !pb_fft_length_supported(H)))
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "planes of %d x %d: lines of up to %d samples are supported", H, W, kMaxLineLength);
    const long n = (long)P * H * W;
    float *other = nullptr;
    if (grad_gx && grad_gy) {
        other = static_cast<float *>(pb_scratch(ctx, "halog.fy", sizeof(float) * (size_t)n));
        if (!other) return PB_ERR_NOMEM;
    }
    // the transposes of the two circulants are their negatives: the forward's own transforms, then one pass that adds and negates
    int rc = grad_gx ? pb_fourier_gradients_impl(ctx, grad_gx, P, H, W, grad_planes, nullptr)
                     : pb_fourier_gradients_impl(ctx, grad_gy, P, H, W, nullptr, grad_planes);
    if (rc) return rc;
    if (other) {
        rc = pb_fourier_gradients_impl(ctx, grad_gy, P, H, W, nullptr, other);
        if (rc) return rc;
    }
    ProfScope prof(ctx, PB_PROF_OTHER);
    const bool vec = n % 4 == 0 && hg_aligned16({grad_planes, other});
    const long units = vec ? n / 4 : n;
    const unsigned grid = (unsigned)std::max(1L, std::min((units + HG_NT - 1) / HG_NT, 8192L));
    if (vec) hipLaunchKernelGGL(neg_sum_kernel<true>, dim3(grid), dim3(HG_NT), 0, ctx->stream, grad_planes, other, n);
    else hipLaunchKernelGGL(neg_sum_kernel<false>, dim3(grid), dim3(HG_NT), 0, ctx->stream, grad_planes, other, n);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_halo_mask_backward_impl(pb_ctx *ctx, const float *x, const float *y, const float *grad0_x, const float *grad0_y,
                                     const float *grad_out, float *grad_x, float *grad_y, float *grad_grad0_x, float *grad_grad0_y,
                                     int B, int C, int H, int W) {
    if (!x || !y || !grad0_x || !grad0_y || !grad_out || (!grad_x && !grad_y && !grad_grad0_x && !grad_grad0_y))
        return pb_fail(ctx, PB_ERR_BADARG, "pb_halo_mask_backward: null argument");
    float *outs[4] = {grad_x, grad_y, grad_grad0_x, grad_grad0_y};
    const float *ins[5] = {x, y, grad0_x, grad0_y, grad_out};
    for (int i = 0; i < 4; ++i) {
        for (int j = 0; j < 5; ++j)
            if (hg_same(outs[i], ins[j])) return pb_fail(ctx, PB_ERR_BADARG, "pb_halo_mask_backward: an output may not alias an input");
        for (int j = i + 1; j < 4; ++j)
            if (hg_same(outs[i], outs[j])) return pb_fail(ctx, PB_ERR_BADARG, "pb_halo_mask_backward: two outputs may not alias");
    }
    if (B < 1 || C < 1 || H < 2 || W < 2) return pb_fail(ctx, PB_ERR_BADARG, "bad shape (%d,%d,%d,%d)", B, C, H, W);
    if (!pb_fft_length_supported(W))
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "image width %d: lines of up to %d samples are supported", W, kMaxLineLength);
    const long HW = (long)H * W;
    const long P = (long)B * C;
    int bpp = (int)((HW + HG_NT * 16 - 1) / (HG_NT * 16));
    if (bpp > 256) bpp = 256;
    if (bpp < 1) bpp = 1;
    if (P * bpp > 0xffffffL)                                  // (one workgroup per plane and block: 2^32 threads per grid dimension)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "pb_halo_mask_backward: %ld planes of %d blocks -- up to 2^24 workgroups", P, bpp);
    const bool want_g0 = grad_grad0_x || grad_grad0_y;
    const size_t plane_bytes = sizeof(float) * (size_t)P * HW;
    float *nM = static_cast<float *>(pb_scratch(ctx, "halog.nM", sizeof(float) * (size_t)P));
    float *ox = static_cast<float *>(pb_scratch(ctx, "halog.ox", plane_bytes));
    if (!nM || !ox) return PB_ERR_NOMEM;
    float *t = nullptr, *partial = nullptr, *S = nullptr;
    if (grad_y) {
        t = static_cast<float *>(pb_scratch(ctx, "halog.t", plane_bytes));
        if (!t) return PB_ERR_NOMEM;
    }
    if (want_g0) {
        partial = static_cast<float *>(pb_scratch(ctx, "halog.part", sizeof(float) * (size_t)P * bpp));
        S = static_cast<float *>(pb_scratch(ctx, "halog.S", sizeof(float) * (size_t)P));
        if (!partial || !S) return PB_ERR_NOMEM;
    }
    // nM and ox by the forward's own launchers: the forward's bits
    int rc = pb_grad_energy(ctx, grad0_x, grad0_y, nM, (int)P, HW);
    if (rc) return rc;
    rc = pb_fourier_gradients_impl(ctx, y, (int)P, H, W, ox, nullptr);
    if (rc) return rc;
    const bool vec = HW % 4 == 0 && hg_aligned16({x, y, grad0_x, grad0_y, grad_out, grad_x, grad_y, grad_grad0_x, grad_grad0_y, ox, t});
    const dim3 grid((unsigned)(P * bpp));
    {
        ProfScope prof(ctx, PB_PROF_HALO);
        if (vec)
            hipLaunchKernelGGL(halo_grad_pass1<true>, grid, dim3(HG_NT), 0, ctx->stream, x, y, grad0_x, grad0_y, ox, grad_out, nM, grad_x,
                               grad_y, grad_grad0_x, grad_grad0_y, t, partial, HW, bpp);
        else
            hipLaunchKernelGGL(halo_grad_pass1<false>, grid, dim3(HG_NT), 0, ctx->stream, x, y, grad0_x, grad0_y, ox, grad_out, nM, grad_x,
                               grad_y, grad_grad0_x, grad_grad0_y, t, partial, HW, bpp);
        PB_LAUNCH_CHECK();
        if (want_g0) {
            hipLaunchKernelGGL(pb_fold_partials_kernel, dim3((unsigned)P), dim3(64), 0, ctx->stream, partial, S, bpp);
            PB_LAUNCH_CHECK();
        }
    }
    if (!grad_y && !want_g0) return PB_OK;
    if (grad_y) {
        rc = pb_fourier_gradients_impl(ctx, t, (int)P, H, W, ox, nullptr);      // (ox has been consumed by pass one)
        if (rc) return rc;
    }
    ProfScope prof(ctx, PB_PROF_HALO);
    if (vec)
        hipLaunchKernelGGL(halo_grad_finish<true>, grid, dim3(HG_NT), 0, ctx->stream, grad0_x, grad0_y, ox, S, grad_y, grad_grad0_x,
                           grad_grad0_y, HW, bpp);
    else
        hipLaunchKernelGGL(halo_grad_finish<false>, grid, dim3(HG_NT), 0, ctx->stream, grad0_x, grad0_y, ox, S, grad_y, grad_grad0_x,
                           grad_grad0_y, HW, bpp);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
