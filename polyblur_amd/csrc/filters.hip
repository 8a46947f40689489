// Optional stages of the hot path:
//   halo masking                     deblurring.py:172-208   (bug-compatible, see halo_kernel)
//   5x5 bilateral filter             filters.py:107-148
//   prefilter recombination          deblurring.py:84,88
#include "stage_math.h"
#include "patch_cover.h"

int pb_fourier_gradients_impl(pb_ctx *ctx, const float *planes, int P, int H, int W, float *gx, float *gy);
int pb_bilateral5_sigma_impl(pb_ctx *ctx, const void *in, int in_dtype, void *out, int out_dtype, int P, int H, int W,
                             double sigma_space, double sigma_color);

namespace {

constexpr int NT = 256;

// ------------------------------------------------------------------------------------
// halo masking
// ------------------------------------------------------------------------------------
// nM[plane] = sum_{H,W} gx^2 + gy^2          (deblurring.py:178-179,206)
// VEC: planes of whole groups of four samples on 16-byte (fp16: 8-byte) boundaries -- four samples per lane and trip (round 6:
// 78 -> 45 us on a 4K image's three planes); which samples a lane sums, and in which order, depends on the plane's size alone.
template <typename TG, bool VEC>
__global__ __launch_bounds__(NT) void grad_energy_kernel(const TG *__restrict__ gx, const TG *__restrict__ gy,
                                                         float *__restrict__ partial, long HW, int blocks_per_plane) {
    const int plane = blockIdx.x / blocks_per_plane;
    const int blk = blockIdx.x - plane * blocks_per_plane;
    const TG *a = gx + (long)plane * HW, *b = gy + (long)plane * HW;
    float s = 0.f;
    if constexpr (VEC) {
        for (long i = 4 * ((long)blk * NT + threadIdx.x); i < HW; i += 4l * blocks_per_plane * NT) {
            const float4 u = pb_ld4(a + i), v = pb_ld4(b + i);
            s += u.x * u.x + v.x * v.x;
            s += u.y * u.y + v.y * v.y;
            s += u.z * u.z + v.z * v.z;
            s += u.w * u.w + v.w * v.w;
        }
    } else {
        for (long i = (long)blk * NT + threadIdx.x; i < HW; i += (long)blocks_per_plane * NT) {
            const float u = pb_ld(a + i), v = pb_ld(b + i);
            s += u * u + v * v;
        }
    }
    __shared__ float red[NT / 64];
    const float t = pb_block_sum_to_first<NT>(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = t;       // (folded per plane by pb_fold_partials_kernel: nM is bit-reproducible)
}

// z = max(M / (nM + M), 0), M = -gx*ox - gy*gy (sic) -- pb_halo_ratio, stage_math.h;  out = y + z (x - y)   [+ clamp to [0,1], deblurring.py:239]
// With a prefilter the masked result is recombined on the spot (cur != nullptr; recombine_kernel's arithmetic):
// out = clip(clip(out, 0, 1) + (cur - smooth), 0, 1) -- one pass over the batch instead of a store, a load and a pass.
// TG: the type the three gradient planes are kept in -- fp32, or fp16 where the call's images are fp16 (z = M / (nM + M) is a
// ratio of one sample's products to the whole plane's energy, ~1e-5 on an image: an fp16 rounding of its factors moves the
// output by ~1e-9, and the three planes are 12 of the 28 bytes this kernel moves per sample)
// VEC: every plane's rows start on a boundary of four samples (W, the x operand's pitch and plane stride multiples of 4): four
// samples per thread and trip -- the same operations per sample, 16-byte (fp16: 8-byte) accesses, no 64-bit division per sample
template <typename TX, typename TOut, typename TG, bool VEC>
__global__ __launch_bounds__(NT) void halo_kernel(const TX *__restrict__ x, int x_pitch, long x_plane,
                                                  const float *__restrict__ y, const TG *__restrict__ gx,
                                                  const TG *__restrict__ gy, const TG *__restrict__ ox,
                                                  const float *__restrict__ nM, TOut *__restrict__ out, int P, int H, int W,
                                                  int clamp01, const void *__restrict__ cur, int cur_is_half,
                                                  const float *smooth) {
    const long HW = (long)H * W;
    if constexpr (VEC) {
        const int W4 = W >> 2;
        const long n4 = HW >> 2;
        for (int plane = blockIdx.y; plane < P; plane += gridDim.y) {
            const float nm = nM[plane];
            for (long i4 = (long)blockIdx.x * NT + threadIdx.x; i4 < n4; i4 += (long)gridDim.x * NT) {
                const int r = (int)((unsigned)i4 / (unsigned)W4), c = 4 * ((int)i4 - r * W4);       // (H W / 4 < 2^32: sides up to 65536)
                const long k = (long)plane * HW + 4 * i4;
                const float4 gxx = pb_ld4(gx + k), gyy = pb_ld4(gy + k), oxx = pb_ld4(ox + k), yv = pb_ld4(y + k);
                const float4 xv = pb_ld4(x + (long)plane * x_plane + (long)r * x_pitch + c);
                float4 cv = make_float4(0.f, 0.f, 0.f, 0.f), sm = cv;
                if (cur) {
                    cv = cur_is_half ? pb_ld4(static_cast<const __half *>(cur) + k) : pb_ld4(static_cast<const float *>(cur) + k);
                    sm = pb_ld4(smooth + k);
                }
                const float g1[4] = {gxx.x, gxx.y, gxx.z, gxx.w}, g2[4] = {gyy.x, gyy.y, gyy.z, gyy.w}, o1[4] = {oxx.x, oxx.y, oxx.z, oxx.w};
                const float xs[4] = {xv.x, xv.y, xv.z, xv.w}, ys[4] = {yv.x, yv.y, yv.z, yv.w};
                const float cs[4] = {cv.x, cv.y, cv.z, cv.w}, ss[4] = {sm.x, sm.y, sm.z, sm.w};
                float o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float z = pb_halo_ratio(g1[e], g2[e], o1[e], nm).z;
                    float v = fmaf(z, xs[e] - ys[e], ys[e]);
                    if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
                    if (cur) {
                        const float d = cs[e] - ss[e];
                        v = fminf(fmaxf(v, 0.f), 1.f) + d;
                        v = fminf(fmaxf(v, 0.f), 1.f);
                    }
                    o[e] = v;
                }
                pb_st4(out + k, make_float4(o[0], o[1], o[2], o[3]));
            }
        }
        return;
    }
    for (int plane = blockIdx.y; plane < P; plane += gridDim.y) {      // (grid.y is capped at 65535)
    const float nm = nM[plane];
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < HW; i += (long)gridDim.x * NT) {
        const int r = (int)(i / W), c = (int)(i - (long)r * W);
        const long k = (long)plane * HW + i;
        const float gxx = pb_ld(gx + k), gyy = pb_ld(gy + k);
        const float z = pb_halo_ratio(gxx, gyy, pb_ld(ox + k), nm).z;
        const float xv = pb_ld(x + (long)plane * x_plane + (long)r * x_pitch + c);
        const float yv = y[k];
        float v = fmaf(z, xv - yv, yv);
        if (clamp01) v = fminf(fmaxf(v, 0.f), 1.f);
        if (cur) {
            const float cv = cur_is_half ? pb_ld(static_cast<const __half *>(cur) + k) : static_cast<const float *>(cur)[k];
            const float d = cv - smooth[k];
            v = fminf(fmaxf(v, 0.f), 1.f) + d;
            v = fminf(fmaxf(v, 0.f), 1.f);
        }
        pb_st(out + k, v);
    }
    }
}

// out = clip(clip(y,0,1) + (cur - smooth), 0, 1)          (deblurring.py:84,88,239)
template <typename TC, typename TO>
__global__ __launch_bounds__(NT) void recombine_kernel(const float *__restrict__ y, const TC *__restrict__ cur,
                                                       const float *__restrict__ smooth, TO *__restrict__ out, long n) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const float d = pb_ld(cur + i) - smooth[i];
        const float v = fminf(fmaxf(y[i], 0.f), 1.f) + d;
        pb_st(out + i, fminf(fmaxf(v, 0.f), 1.f));
    }
}

// ------------------------------------------------------------------------------------
// bilateral 5x5
// ------------------------------------------------------------------------------------
// Round 6: the weight of a tap is ONE exponential, exp2(d^2 kc + r^2 ks) with kc = -log2(e) / (2 sigma_color^2) and ks likewise
// for the spatial term (filters.py:111,134-136: exp(-d^2 / var2) * gw -- the same number; the library expf spent ~14
// instructions per tap on an accuracy a weight does not need: v_exp_f32 is within 1 ulp, and an error of the exponent's
// rounding, ~|x| 2^-24, weighs on taps whose weight is ~e^x), and a thread forms four vertically adjacent outputs from an
// 8 x 5 window held in registers: 10 LDS reads per output instead of 25.  370 -> ~150 us per 4K image.
template <typename TIn, typename TOut>
__global__ __launch_bounds__(NT) void bilateral5_kernel(const TIn *__restrict__ in, TOut *__restrict__ out, int P, int H, int W,
                                                        float kc, float ks1) {
    constexpr int TWB = 64, THB = 16, R = 2, LW = TWB + 2 * R, LH = THB + 2 * R, PER = THB / (NT / TWB);
    __shared__ float s[LH * LW];
    const int x0 = blockIdx.x * TWB, y0 = blockIdx.y * THB;
    float ks[9];                                                     // by squared distance 0 .. 8
#pragma unroll
    for (int d = 0; d < 9; ++d) ks[d] = (float)d * ks1;
    for (int plane = blockIdx.z; plane < P; plane += gridDim.z) {      // (grid.z is capped at 65535)
    if (plane != (int)blockIdx.z) __syncthreads();
    const TIn *src = in + (long)plane * H * W;
    for (int e = threadIdx.x; e < LH * LW; e += NT) {
        const int r = e / LW, c = e - r * LW;
        const int yy = min(max(y0 + r - R, 0), H - 1), xx = min(max(x0 + c - R, 0), W - 1);   // replicate pad
        s[e] = pb_ld(src + (long)yy * W + xx);
    }
    __syncthreads();
    const int tx = threadIdx.x % TWB, ty = (threadIdx.x / TWB) * PER;     // outputs: rows ty .. ty + PER - 1 of the tile, column tx
    float win[PER + 2 * R][5];
#pragma unroll
    for (int r = 0; r < PER + 2 * R; ++r)
#pragma unroll
        for (int j = 0; j < 5; ++j) win[r][j] = s[(ty + r) * LW + tx + j];
#pragma unroll
    for (int o = 0; o < PER; ++o) {
        const int yy = y0 + ty + o, xx = x0 + tx;
        if (yy >= H || xx >= W) continue;
        const float ctr = win[o + R][R];
        float num = 0.f, den = 0.f;
#pragma unroll
        for (int i = 0; i < 5; ++i)
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const float v = win[o + i][j];
                const float d = v - ctr;
                const float w = __builtin_amdgcn_exp2f(fmaf(d * d, kc, ks[(i - 2) * (i - 2) + (j - 2) * (j - 2)]));
                num = fmaf(w, v, num);
                den += w;
            }
        pb_st(out + (long)plane * H * W + (long)yy * W + xx, num / (den + 1e-5f));
    }
    }
}

template <typename T> __global__ void to_float_kernel(const T *__restrict__ in, float *__restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = pb_ld(in + i);
}
template <typename T> __global__ void from_float_kernel(const float *__restrict__ in, T *__restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) pb_st(out + i, in[i]);
}

unsigned grid_for(long n, int per_block = NT, int cap = 8192) {
    long g = (n + per_block - 1) / per_block;
    if (g > cap) g = cap;
    if (g < 1) g = 1;
    return (unsigned)g;
}

}  // namespace

// (common.h) one wave per output folds that output's per-workgroup partial sums in a fixed order
__global__ __launch_bounds__(64) void pb_fold_partials_kernel(const float *__restrict__ partial, float *__restrict__ out, int per_out) {
    const float *p = partial + (long)blockIdx.x * per_out;
    float s = 0.f;
    for (int i = threadIdx.x; i < per_out; i += 64) s += p[i];
    s = pb_wave_sum(s);
    if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// ---- internal entry points used by api.hip --------------------------------------------------
int pb_grad_energy(pb_ctx *ctx, const void *gx, const void *gy, float *nM, int P, long HW, int g_dtype) {
    ProfScope prof(ctx, PB_PROF_HALO);
    int bpp = (int)((HW + NT * 16 - 1) / (NT * 16));
    if (bpp > 256) bpp = 256;
    if (bpp < 1) bpp = 1;
    float *partial = static_cast<float *>(pb_scratch(ctx, "halo.partial", sizeof(float) * (size_t)P * bpp));
    if (!partial) return PB_ERR_NOMEM;
    const bool vec = HW % 4 == 0 && (reinterpret_cast<uintptr_t>(gx) | reinterpret_cast<uintptr_t>(gy)) % 16 == 0;
#define PB_GE(TG, VEC)                                                                                                             \
    hipLaunchKernelGGL((grad_energy_kernel<TG, VEC>), dim3(P * bpp), dim3(NT), 0, ctx->stream, static_cast<const TG *>(gx),       \
                       static_cast<const TG *>(gy), partial, HW, bpp)
    if (g_dtype == PB_F16) { if (vec) PB_GE(__half, true); else PB_GE(__half, false); }
    else { if (vec) PB_GE(float, true); else PB_GE(float, false); }
#undef PB_GE
    hipLaunchKernelGGL(pb_fold_partials_kernel, dim3(P), dim3(64), 0, ctx->stream, partial, nM, bpp);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_halo_apply(pb_ctx *ctx, const void *x, int x_dtype, int x_pitch, long x_plane, const float *y, const void *gx,
                  const void *gy, const void *ox, const float *nM, void *out, int out_dtype, int P, int H, int W,
                  int clamp01, const void *recomb_cur, int recomb_cur_dtype, const float *recomb_smooth, int g_dtype) {
    // four samples per thread where every row of every plane starts on a boundary of four samples (and x's first sample does:
    // the interior of a padded plane starts pad (pp + 1) samples in)
    const size_t xb = x_dtype == PB_F16 ? 2 : 4;
    const bool vec = (W & 3) == 0 && (x_pitch & 3) == 0 && (x_plane & 3) == 0 && (reinterpret_cast<size_t>(x) % (4 * xb)) == 0 &&
                     (long)H * W / 4 < 0xffffffffL;
    dim3 grid(grid_for((long)H * W / (vec ? 4 : 1), NT, 2048), P < 65535 ? P : 65535);
    ProfScope prof(ctx, PB_PROF_HALO);
    if (recomb_cur && recomb_cur_dtype != PB_F32 && recomb_cur_dtype != PB_F16)
        return pb_fail(ctx, PB_ERR_BADARG, "halo: the recombined image must be fp32 or fp16");
    const int cur_is_half = recomb_cur_dtype == PB_F16;
#define PB_HALO_V(TX, TO, TG, VEC)                                                                                 \
    hipLaunchKernelGGL((halo_kernel<TX, TO, TG, VEC>), grid, dim3(NT), 0, ctx->stream, static_cast<const TX *>(x), x_pitch, \
                       x_plane, y, static_cast<const TG *>(gx), static_cast<const TG *>(gy), static_cast<const TG *>(ox), nM, \
                       static_cast<TO *>(out), P, H, W, clamp01, recomb_cur, cur_is_half, recomb_smooth)
#define PB_HALO(TX, TO, TG) do { if (vec) PB_HALO_V(TX, TO, TG, true); else PB_HALO_V(TX, TO, TG, false); } while (0)
#define PB_HALO_G(TX, TO) do { if (g_dtype == PB_F16) PB_HALO(TX, TO, __half); else PB_HALO(TX, TO, float); } while (0)
    if (x_dtype == PB_F32 && out_dtype == PB_F32) PB_HALO_G(float, float);
    else if (x_dtype == PB_F32 && out_dtype == PB_F16) PB_HALO_G(float, __half);
    else if (x_dtype == PB_F16 && out_dtype == PB_F32) PB_HALO_G(__half, float);
    else PB_HALO_G(__half, __half);
#undef PB_HALO_G
#undef PB_HALO
#undef PB_HALO_V
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_recombine(pb_ctx *ctx, const float *y, const void *cur, int cur_dtype, const float *smooth, void *out, int out_dtype,
                 long n) {
    ProfScope prof(ctx, PB_PROF_PREFILTER);
#define PB_REC(TC, TO)                                                                                           \
    hipLaunchKernelGGL((recombine_kernel<TC, TO>), dim3(grid_for(n)), dim3(NT), 0, ctx->stream, y,                \
                       static_cast<const TC *>(cur), smooth, static_cast<TO *>(out), n)
    if (cur_dtype == PB_F32 && out_dtype == PB_F32) PB_REC(float, float);
    else if (cur_dtype == PB_F32) PB_REC(float, __half);
    else if (out_dtype == PB_F32) PB_REC(__half, float);
    else PB_REC(__half, __half);
#undef PB_REC
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_bilateral5_impl(pb_ctx *ctx, const void *in, int in_dtype, void *out, int out_dtype, int P, int H, int W) {
    return pb_bilateral5_sigma_impl(ctx, in, in_dtype, out, out_dtype, P, H, W, 5.0, 0.1);
}

// the same launch with the caller's two sigma (pb_bilateral at ksize == 5, bilateral.hip); 5.0f and 0.1f give the floats 5.0 and 0.1 give
int pb_bilateral5_sigma_impl(pb_ctx *ctx, const void *in, int in_dtype, void *out, int out_dtype, int P, int H, int W,
                             double sigma_space, double sigma_color) {
    const double log2e = 1.4426950408889634;
    const float ivc = (float)(-log2e / (2. * sigma_color * sigma_color)), ivs = (float)(-log2e / (2. * sigma_space * sigma_space));   // (exp2's arguments)
    dim3 grid((W + 63) / 64, (H + 15) / 16, P < 65535 ? P : 65535);
    ProfScope prof(ctx, PB_PROF_PREFILTER);
#define PB_BIL(TI, TO)                                                                                           \
    hipLaunchKernelGGL((bilateral5_kernel<TI, TO>), grid, dim3(NT), 0, ctx->stream, static_cast<const TI *>(in),  \
                       static_cast<TO *>(out), P, H, W, ivc, ivs)
    if (in_dtype == PB_F32 && out_dtype == PB_F32) PB_BIL(float, float);
    else if (in_dtype == PB_F16 && out_dtype == PB_F32) PB_BIL(__half, float);
    else if (in_dtype == PB_F16 && out_dtype == PB_F16) PB_BIL(__half, __half);
    else PB_BIL(float, __half);
#undef PB_BIL
    PB_LAUNCH_CHECK();
    return PB_OK;
}

// (H,W,C) interleaved bytes <-> (C,H,W) planar bytes.  One thread per pixel: the interleaved side is touched
// as C consecutive bytes per lane (a wavefront covers one contiguous 64*C-byte span), the planar side as
// one byte per lane per plane.
template <bool TO_PLANAR>
__global__ void u8_layout_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out, int C, long HW, long total) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long b = i / HW, p = i - b * HW;
        const long inter = (b * HW + p) * C, planar = b * C * HW + p;
        for (int c = 0; c < C; ++c) {
            if (TO_PLANAR) out[planar + c * HW] = in[inter + c];
            else out[inter + c] = in[planar + c * HW];
        }
    }
}

int pb_u8_layout(pb_ctx *ctx, const unsigned char *in, unsigned char *out, int B, int C, int H, int W, int to_planar) {
    const long HW = (long)H * W, total = (long)B * HW;
    if (to_planar) hipLaunchKernelGGL(u8_layout_kernel<true>, dim3(grid_for(total)), dim3(NT), 0, ctx->stream, in, out, C, HW, total);
    else hipLaunchKernelGGL(u8_layout_kernel<false>, dim3(grid_for(total)), dim3(NT), 0, ctx->stream, in, out, C, HW, total);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_convert_to_float(pb_ctx *ctx, const void *in, int dtype, float *out, long n) {
    if (dtype == PB_F32) PB_HIP(hipMemcpyAsync(out, in, sizeof(float) * n, hipMemcpyDeviceToDevice, ctx->stream));
    else if (dtype == PB_U8) {
        hipLaunchKernelGGL(to_float_kernel<unsigned char>, dim3(grid_for(n)), dim3(NT), 0, ctx->stream, static_cast<const unsigned char *>(in), out, n);
        PB_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(to_float_kernel<__half>, dim3(grid_for(n)), dim3(NT), 0, ctx->stream, static_cast<const __half *>(in), out, n);
        PB_LAUNCH_CHECK();
    }
    return PB_OK;
}

int pb_convert_from_float(pb_ctx *ctx, const float *in, void *out, int dtype, long n) {
    if (dtype == PB_F32) PB_HIP(hipMemcpyAsync(out, in, sizeof(float) * n, hipMemcpyDeviceToDevice, ctx->stream));
    else if (dtype == PB_U8) {
        hipLaunchKernelGGL(from_float_kernel<unsigned char>, dim3(grid_for(n)), dim3(NT), 0, ctx->stream, in, static_cast<unsigned char *>(out), n);
        PB_LAUNCH_CHECK();
    } else {
        hipLaunchKernelGGL(from_float_kernel<__half>, dim3(grid_for(n)), dim3(NT), 0, ctx->stream, in, static_cast<__half *>(out), n);
        PB_LAUNCH_CHECK();
    }
    return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// patch decomposition with windowed overlap-add (reference deblurring.py:269-340, fix-forward:
// the undefined `handling_saturation` branch is dropped and patches of a batch are indexed
// [n*B, (n+1)*B) instead of the reference's [n::batch_size], which is only right for B == 1)
// ---------------------------------------------------------------------------------------------
namespace {

// patches[(n*B + b), c, y, x] = img[b, c, clamp(i0 + y - pad_top), clamp(j0 + x - pad_left)],
// n = first + local patch index, (i0, j0) = (n / n_j * step_h, n % n_j * step_w): pad_with_new_size
// (replicate, deblurring.py:368-377) and the slicing (:312-313) in one pass.
template <typename T>
__global__ __launch_bounds__(NT) void extract_patches_kernel(const T *__restrict__ img, T *__restrict__ patches, int B, int C,
                                                             int H, int W, int ph, int pw, int step_h, int step_w, int n_j,
                                                             int pad_top, int pad_left, int first, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int x = (int)(i % pw);
        long r = i / pw;
        const int y = (int)(r % ph); r /= ph;
        const int c = (int)(r % C); r /= C;
        const int b = (int)(r % B);
        const int n = first + (int)(r / B);
        const int i0 = (n / n_j) * step_h, j0 = (n % n_j) * step_w;
        const int sy = min(max(i0 + y - pad_top, 0), H - 1), sx = min(max(j0 + x - pad_left, 0), W - 1);
        patches[i] = img[(((long)b * C + c) * H + sy) * W + sx];
    }
}

// out[b, c, Y, X] = clamp( sum_n restored_n * w / (sum_n w + 1e-8), 0, 1 ) over the patches that cover the
// (padded) pixel, written straight into the cropped H x W result (deblurring.py:332-340): a gather, so
// no atomics and no window_sum buffer.  The cover sum is patch_cover.h's, shared with pb_overlap_add_backward.
template <typename T>
__global__ __launch_bounds__(NT) void overlap_add_kernel(const T *__restrict__ patches, T *__restrict__ out, int B, int C, int H,
                                                         int W, int ph, int pw, int step_h, int step_w, int n_i, int n_j,
                                                         int pad_top, int pad_left, const float *__restrict__ win_y,
                                                         const float *__restrict__ win_x, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int X = (int)(i % W);
        long r = i / W;
        const int Y = (int)(r % H); r /= H;
        const int c = (int)(r % C);
        const int b = (int)(r / C);
        const PatchCover cv = patch_cover(patches, B, C, ph, pw, step_h, step_w, n_i, n_j, b, c, Y + pad_top, X + pad_left, win_y, win_x);
        pb_st(out + i, fminf(fmaxf(patch_cover_value(cv), 0.f), 1.f));
    }
}

}  // namespace

int pb_extract_patches_impl(pb_ctx *ctx, const void *img, void *patches, int dtype, int B, int C, int H, int W, int ph, int pw,
                            int step_h, int step_w, int n_j, int pad_top, int pad_left, int first, int count) {
    const long total = (long)count * B * C * ph * pw;
    ProfScope prof(ctx, PB_PROF_OTHER);
    if (dtype == PB_F32)
        hipLaunchKernelGGL(extract_patches_kernel<float>, dim3(grid_for(total)), dim3(NT), 0, ctx->stream,
                           static_cast<const float *>(img), static_cast<float *>(patches), B, C, H, W, ph, pw, step_h, step_w, n_j,
                           pad_top, pad_left, first, total);
    else
        hipLaunchKernelGGL(extract_patches_kernel<__half>, dim3(grid_for(total)), dim3(NT), 0, ctx->stream,
                           static_cast<const __half *>(img), static_cast<__half *>(patches), B, C, H, W, ph, pw, step_h, step_w,
                           n_j, pad_top, pad_left, first, total);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_overlap_add_impl(pb_ctx *ctx, const void *patches, void *out, int dtype, int B, int C, int H, int W, int ph, int pw,
                        int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left, const float *win_y,
                        const float *win_x) {
    const long total = (long)B * C * H * W;
    ProfScope prof(ctx, PB_PROF_OTHER);
    if (dtype == PB_F32)
        hipLaunchKernelGGL(overlap_add_kernel<float>, dim3(grid_for(total)), dim3(NT), 0, ctx->stream,
                           static_cast<const float *>(patches), static_cast<float *>(out), B, C, H, W, ph, pw, step_h, step_w, n_i,
                           n_j, pad_top, pad_left, win_y, win_x, total);
    else
        hipLaunchKernelGGL(overlap_add_kernel<__half>, dim3(grid_for(total)), dim3(NT), 0, ctx->stream,
                           static_cast<const __half *>(patches), static_cast<__half *>(out), B, C, H, W, ph, pw, step_h, step_w,
                           n_i, n_j, pad_top, pad_left, win_y, win_x, total);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
