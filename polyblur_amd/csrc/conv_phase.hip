// The polynomial with the pure-phase filter (reference deblurring.py:141-169, not_symmetric=True): the one transform over the
// whole padded domain in the engine.  No other path uses it.
//
//   X = ifft2( M . fft2(x) ),   M = C (((a3 K + a2) K + a1) K + b) / (Hp Wp),   K = fft2(p2o(kernel)),  C = conj(K) / (|K| + 1e-8)
//
// 1 / |K| has no finite support, so no window or stencil body can evaluate it.  Per image:
//   phase_krows_kernel   the kh rows of p2o(kernel) that hold taps (filters.py:255-273: tap (i, j) at ((i - kh/2) mod Hp,
//                        (j - kw/2) mod Wp)), transformed along x into a zeroed complex plane
//   phase_cols_kernel<1> that plane transformed along y, and M formed from K in place
//   phase_rows_fwd       the image's rows (replicate pad as an index clamp, or a padded plane), two real planes packed as one
//                        complex plane, transformed along x into complex scratch
//   phase_cols_kernel<0> columns forward, times M, columns back -- the 2-D spectrum exists in LDS only
//   phase_rows_inv       the interior rows back along x, cropped, [clamped,] stored as fp32 or fp16
// A direct plan leaves its spectrum digit-reversed, a Bluestein plan in natural order: the image and the kernel go through the
// same two plans, so their spectra agree position by position and the order never matters.  The inverse is the forward
// transform of the conjugate (fft.h: line_inverse).
// Two planes per transform: M is Hermitian-symmetric for real taps, so ifft2(M fft2(x1 + i x2)) = X1 + i X2.  Only planes of one
// image are paired (C = 3: planes 0 + 1, plane 2 alone), so an image's bits do not depend on the rest of the batch.
#include <algorithm>

#include "common.h"
#include "conv_phase_common.h"
#include "fft.h"

namespace {

// where the planes of a call live.  virt: an un-padded H x W plane addressed in padded coordinates (replicate pad by index clamp)
struct PhaseSrc { const void *p; int virt; int pitch; long plane; };

template <typename T>
__device__ __forceinline__ float phase_ld(const PhaseSrc &src, long plane, int r, int c, int pad, int H, int W) {
    if (src.virt) {
        r = min(max(r - pad, 0), H - 1);
        c = min(max(c - pad, 0), W - 1);
    }
    return pb_ld<T>(static_cast<const T *>(src.p) + plane * src.plane + (long)r * src.pitch + c);
}

// grid (ceil(Hp / nb), slots): nb rows of one slot, element (c, j) at s[c * nb + j]
template <typename T, int NTH>
__global__ __launch_bounds__(NTH) void phase_rows_fwd(PhaseSrc src, float2 *__restrict__ G, int slot0, int C, int H, int W,
                                                      int pad, int lognb, pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int r0 = blockIdx.x << lognb;
    long plane; bool two;
    phase_slot(slot0 + blockIdx.y, C, plane, two);
    for (int idx = threadIdx.x; idx < (Wp << lognb); idx += NTH) {
        const int j = idx / Wp, c = idx - j * Wp, r = r0 + j;
        float2 v = make_float2(0.f, 0.f);
        if (r < Hp) {
            v.x = phase_ld<T>(src, plane, r, c, pad, H, W);
            if (two) v.y = phase_ld<T>(src, plane + 1, r, c, pad, H, W);
        }
        sph[(c << lognb) + j] = v;
    }
    __syncthreads();
    pbfft::line_forward(sph, plan, lognb);
    float2 *dst = G + (long)blockIdx.y * Hp * Wp;
    for (int idx = threadIdx.x; idx < (Wp << lognb); idx += NTH) {
        const int j = idx / Wp, c = idx - j * Wp, r = r0 + j;
        if (r < Hp) dst[(long)r * Wp + c] = sph[(c << lognb) + j];
    }
}

// grid (kh): row i of the taps of one kernel at row (i - kh/2) mod Hp of the zeroed plane, transformed along x
template <int NTH>
__global__ __launch_bounds__(NTH) void phase_krows_kernel(const float *__restrict__ taps, float2 *__restrict__ K, int kh, int kw,
                                                          int Hp, int Wp, pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int i = blockIdx.x;
    for (int c = threadIdx.x; c < Wp; c += NTH) sph[c] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int j = threadIdx.x; j < kw; j += NTH) {
        int c = j - kw / 2;
        if (c < 0) c += Wp;
        sph[c] = make_float2(taps[i * kw + j], 0.f);
    }
    __syncthreads();
    pbfft::line_forward(sph, plan, 0);
    int r = i - kh / 2;
    if (r < 0) r += Hp;
    for (int c = threadIdx.x; c < Wp; c += NTH) K[(long)r * Wp + c] = sph[c];
}

// grid (ceil(Wp / nb), slots): nb adjacent columns interleaved, element (p, j) at s[p * nb + j] <-> G[p][c0 + j]
// MODE 0: forward, times M, back, in place.  MODE 1: forward, then M from K in place (one slot: the kernel's plane)
template <int MODE, int NTH>
__global__ __launch_bounds__(NTH) void phase_cols_kernel(float2 *__restrict__ G, const float2 *__restrict__ M, int Hp, int Wp,
                                                         int lognb, pbfft::DevPlan plan, float a3, float a2, float a1, float b,
                                                         float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int nb = 1 << lognb;
    const int c0 = blockIdx.x << lognb;
    float2 *g = G + (long)blockIdx.y * Hp * Wp;
    for (int e = threadIdx.x; e < (Hp << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        sph[e] = c < Wp ? g[(long)p * Wp + c] : make_float2(0.f, 0.f);
    }
    __syncthreads();
    pbfft::line_forward(sph, plan, lognb);
    if (MODE == 1) {
        for (int e = threadIdx.x; e < (Hp << lognb); e += NTH) {
            const int p = e >> lognb, c = c0 + (e & (nb - 1));
            if (c >= Wp) continue;
            const float2 k = sph[e];
            // deblurring.py:157: C = conj(K) / (|K| + 1e-8); :161-167 is linear in Y, so its four lines are one multiplier
            const float inv = 1.f / (sqrtf(k.x * k.x + k.y * k.y) + 1e-8f);
            const float2 cph = make_float2(k.x * inv, -k.y * inv);
            float2 h = make_float2(a3 * k.x + a2, a3 * k.y);
            h = pbfft::cmul(k, h); h.x += a1;
            h = pbfft::cmul(k, h); h.x += b;
            const float2 m = pbfft::cmul(cph, h);
            g[(long)p * Wp + c] = make_float2(m.x * scale, m.y * scale);
        }
        return;
    }
    for (int e = threadIdx.x; e < (Hp << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        float2 z = make_float2(0.f, 0.f);
        if (c < Wp) z = pbfft::cmul(sph[e], M[(long)p * Wp + c]);
        sph[e] = make_float2(z.x, -z.y);
    }
    __syncthreads();
    pbfft::line_inverse(sph, plan, lognb);
    for (int e = threadIdx.x; e < (Hp << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        if (c < Wp) g[(long)p * Wp + c] = make_float2(sph[e].x, -sph[e].y);
    }
}

// grid (ceil(H / nb), slots): the interior rows back along x; the crop, the clamp and the store
template <typename T, int NTH>
__global__ __launch_bounds__(NTH) void phase_rows_inv(const float2 *__restrict__ G, T *__restrict__ out, int slot0, int C, int H,
                                                      int W, int pad, int lognb, int clamp01, pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int Hp = H + 2 * pad, Wp = W + 2 * pad;
    const int r0 = blockIdx.x << lognb;
    long plane; bool two;
    phase_slot(slot0 + blockIdx.y, C, plane, two);
    const float2 *src = G + (long)blockIdx.y * Hp * Wp;
    for (int idx = threadIdx.x; idx < (Wp << lognb); idx += NTH) {
        const int j = idx / Wp, c = idx - j * Wp, r = r0 + j;
        float2 v = make_float2(0.f, 0.f);
        if (r < H) v = src[(long)(r + pad) * Wp + c];
        sph[(c << lognb) + j] = make_float2(v.x, -v.y);
    }
    __syncthreads();
    pbfft::line_inverse(sph, plan, lognb);
    for (int idx = threadIdx.x; idx < (W << lognb); idx += NTH) {
        const int j = idx / W, c = idx - j * W, r = r0 + j;
        if (r >= H) continue;
        const float2 v = sph[((c + pad) << lognb) + j];          // conj(x1 + i x2)
        float x1 = v.x, x2 = -v.y;
        if (clamp01) { x1 = fminf(fmaxf(x1, 0.f), 1.f); x2 = fminf(fmaxf(x2, 0.f), 1.f); }
        pb_st<T>(out + plane * H * W + (long)r * W + c, x1);
        if (two) pb_st<T>(out + (plane + 1) * H * W + (long)r * W + c, x2);
    }
}

template <typename T>
int launch_rows_fwd(pb_ctx *ctx, const PhaseSrc &src, float2 *G, int slot0, int slots, const PhaseCall &c, int lognb, size_t lds,
                    const pbfft::DevPlan &dp) {
    const dim3 grid((unsigned)((c.H + 2 * c.pad + (1 << lognb) - 1) >> lognb), (unsigned)slots);
    return phase_launch(ctx, phase_rows_fwd<T, 256>, phase_rows_fwd<T, 1024>, grid, lds, src, G, slot0, c.C, c.H, c.W, c.pad, lognb, dp);
}

template <typename T>
int launch_rows_inv(pb_ctx *ctx, const float2 *G, int slot0, int slots, const PhaseCall &c, int lognb, size_t lds,
                    const pbfft::DevPlan &dp) {
    const dim3 grid((unsigned)((c.H + (1 << lognb) - 1) >> lognb), (unsigned)slots);
    return phase_launch(ctx, phase_rows_inv<T, 256>, phase_rows_inv<T, 1024>, grid, lds, G, static_cast<T *>(c.dst), slot0, c.C, c.H, c.W,
                        c.pad, lognb, c.clamp01, dp);
}

template <int MODE>
int launch_cols(pb_ctx *ctx, float2 *G, const float2 *M, int slots, int Hp, int Wp, int lognb, size_t lds, const pbfft::DevPlan &dp,
                float a3, float a2, float a1, float b, float scale) {
    const dim3 grid((unsigned)((Wp + (1 << lognb) - 1) >> lognb), (unsigned)slots);
    return phase_launch(ctx, phase_cols_kernel<MODE, 256>, phase_cols_kernel<MODE, 1024>, grid, lds, G, M, Hp, Wp, lognb, dp, a3, a2, a1, b, scale);
}

}  // namespace

int pb_phase_sides_supported(pb_ctx *ctx, int Hp, int Wp) {
    if (pb_fft_length_supported(Hp) != 1 || pb_fft_length_supported(Wp) != 1)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "the pure-phase filter transforms the whole %d x %d domain with every line in LDS: sides of up to "
                       "20480 samples whose prime factors are all <= 7, up to 8192 otherwise (pb_fft_length_supported == 1)", Hp, Wp);
    return PB_OK;
}

int pb_launch_phase(pb_ctx *ctx, const PhaseCall &c) {
    const int Hp = c.H + 2 * c.pad, Wp = c.W + 2 * c.pad;
    int rc = pb_phase_sides_supported(ctx, Hp, Wp);
    if (rc) return rc;
    if (c.kh > Hp - 1 || c.kw > Wp - 1 || c.kh < 1 || c.kw < 1) return pb_fail(ctx, PB_ERR_BADARG, "a %d x %d kernel does not fit the %d x %d domain", c.kh, c.kw, Hp, Wp);
    const FftPlan *plw = pb_get_plan(ctx, Wp), *plh = pb_get_plan(ctx, Hp);       // (greedy plans: radices up to 16)
    if (!plw || !plh) return PB_ERR_NOMEM;
    const pbfft::DevPlan dpw = pbfft::dev_plan(plw), dph = pbfft::dev_plan(plh);
    const int lr_f = phase_rows_lognb(plw, Hp), lr_i = phase_rows_lognb(plw, c.H), lc = phase_cols_lognb(plh, Wp);
    const size_t lds_rf = phase_lds(plw, lr_f), lds_ri = phase_lds(plw, lr_i), lds_c = phase_lds(plh, lc), lds_k = phase_lds(plw, 0);
    // scratch of its own (none of the two spectra sets): one complex plane for M, and the slots of one group of plane pairs --
    // as many as the budget holds, at least one
    const size_t plane_bytes = sizeof(float2) * (size_t)Hp * Wp;
    const int spi = (c.C + 1) / 2;
    const size_t budget = ctx->phase_budget > 0 ? (size_t)ctx->phase_budget : (size_t)256 << 20;
    const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)spi, std::min<size_t>(budget / plane_bytes, 32768)));
    float2 *M = static_cast<float2 *>(pb_scratch(ctx, "phase.m", plane_bytes));
    float2 *G = static_cast<float2 *>(pb_scratch(ctx, "phase.g", plane_bytes * group));
    if (!M || !G) return PB_ERR_NOMEM;
    const float a3 = c.alpha / 2 - c.beta + 2, a2 = 3 * c.beta - c.alpha - 6, a1 = 5 - 3 * c.beta + c.alpha / 2;
    const float scale = (float)(1.0 / ((double)Hp * Wp));
    PhaseSrc src{c.src, c.src_virtual, c.src_pitch, c.src_plane};
    ProfScope prof(ctx, PB_PROF_CONV_FFT);
    for (int b = 0; b < c.B; ++b) {
        PB_HIP(hipMemsetAsync(M, 0, plane_bytes, ctx->stream));
        const float *taps = c.taps + (size_t)b * c.kh * c.kw;
        rc = phase_launch(ctx, phase_krows_kernel<256>, phase_krows_kernel<1024>, dim3(c.kh), lds_k, taps, M, c.kh, c.kw, Hp, Wp, dpw);
        if (rc) return rc;
        rc = launch_cols<1>(ctx, M, nullptr, 1, Hp, Wp, lc, lds_c, dph, a3, a2, a1, c.beta, scale);
        if (rc) return rc;
        for (int s0 = 0; s0 < spi; s0 += group) {
            const int n = std::min(group, spi - s0), slot0 = b * spi + s0;
            rc = c.src_dtype == PB_F16 ? launch_rows_fwd<__half>(ctx, src, G, slot0, n, c, lr_f, lds_rf, dpw)
                                       : launch_rows_fwd<float>(ctx, src, G, slot0, n, c, lr_f, lds_rf, dpw);
            if (rc) return rc;
            rc = launch_cols<0>(ctx, G, M, n, Hp, Wp, lc, lds_c, dph, 0.f, 0.f, 0.f, 0.f, 0.f);
            if (rc) return rc;
            rc = c.dst_dtype == PB_F16 ? launch_rows_inv<__half>(ctx, G, slot0, n, c, lr_i, lds_ri, dpw)
                                       : launch_rows_inv<float>(ctx, G, slot0, n, c, lr_i, lds_ri, dpw);
            if (rc) return rc;
        }
    }
    return PB_OK;
}
