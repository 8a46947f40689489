// Backward of the polynomial with the pure-phase filter (conv_phase.hip; reference deblurring.py:141-169 with
// not_symmetric=True, filters.py:255-273 for p2o): the gradients of the image and of the taps, over the whole H x W domain.
//
//   forward   y = Re ifft2( M . fft2(x) ),   M = C P,   C = conj(K) / (r + 1e-8),   r = |K|,   K = fft2(p2o(kernel)),
//             P = ((a3 K + a2) K + a1) K + b,   P' = (3 a3 K + 2 a2) K + a1
//   image     grad_x = Re ifft2( conj(M) . fft2(g) )                              g = grad_out
//   taps      A   = (1 / N) sum over the planes of the image  fft2(x) . conj(fft2(g)),   N = H W
//             C_K = -conj(K)^2 / (2 r (r + eps)^2),   C_Kbar = 1 / (r + eps) - r / (2 (r + eps)^2)      (C is not holomorphic in K)
//             S   = A (C_K P + C P') + conj(A C_Kbar P)
//             grad_taps[i][j] = Re fft2(S) at ((i - kh/2) mod H, (j - kw/2) mod W)       (the adjoint of p2o: a gather)
//
// Per image:
//   phaseg_krows       the kh rows of p2o(kernel) that hold taps, transformed along x into a zeroed complex plane ("phaseg.k")
//   phaseg_cols_k      that plane transformed along y: K itself stays (the forward keeps only M; here M, C_K and C_Kbar are
//                      formed from K where they are used)
//   phaseg_rows_fwd    the rows of g -- and, for the taps, of x -- two real planes packed as one complex plane, along x
//   phaseg_cols_a      taps: columns of x and of g forward, A += fft2(x) conj(fft2(g)) -- the pairs of the image one after the
//                      other in ONE workgroup per column tile, so the sum has one order whatever the group size
//   phaseg_cols_x      image: columns of g forward, times conj(M), columns back -- the 2-D spectrum exists in LDS only
//   phaseg_rows_inv    image: the rows back along x, stored
//   phaseg_cols_s      taps: S from A and K, columns transformed (fft(S) = line_inverse of S: fft.h), of which only the kh rows
//                      the gather reads are stored
//   phaseg_taps_rows   taps: those kh rows transformed along x, the kw real parts of each gathered
// The image, the upstream gradient and the kernel go through the same row plan and the same column plan, so their spectra
// agree position by position and the order of a spectrum never matters.
// Pairing: for two real planes packed as x1 + i x2 and g1 + i g2 the product fft2(x) conj(fft2(g)) holds the wanted
// X1 conj(G1) + X2 conj(G2) plus i (X2 conj(G1) - X1 conj(G2)); that second part is anti-Hermitian, A -> S is real-linear and
// keeps the symmetry, so it ends in the imaginary part of fft2(S), which the gather drops.  Only planes of one image are paired.
// No float atomics; every access is one element wide.
#include <algorithm>

#include "common.h"
#include "conv_phase_common.h"
#include "fft.h"

namespace {

// the parts of the multiplier at one bin
struct PhaseBin { float2 cph, P, dP; float r, inv; };

__device__ __forceinline__ PhaseBin phase_bin(float2 k, float a3, float a2, float a1, float b) {
    PhaseBin q;
    q.r = sqrtf(k.x * k.x + k.y * k.y);
    q.inv = 1.f / (q.r + 1e-8f);                                 // deblurring.py:157
    q.cph = make_float2(k.x * q.inv, -k.y * q.inv);
    float2 h = make_float2(a3 * k.x + a2, a3 * k.y);
    h = pbfft::cmul(k, h); h.x += a1;
    h = pbfft::cmul(k, h); h.x += b;
    q.P = h;
    float2 d = make_float2(3.f * a3 * k.x + 2.f * a2, 3.f * a3 * k.y);
    d = pbfft::cmul(k, d); d.x += a1;
    q.dP = d;
    return q;
}

// S = A (C_K P + C P') + conj(A C_Kbar P) at one bin.  |K| has no derivative at 0: the reference's autograd takes 0 there
__device__ __forceinline__ float2 phase_tap_bin(float2 A, float2 k, float a3, float a2, float a1, float b) {
    const PhaseBin q = phase_bin(k, a3, a2, a1, b);
    const float ir = q.r > 0.f ? 1.f / q.r : 0.f;
    const float2 kc = make_float2(k.x, -k.y);
    const float h = 0.5f * q.inv * q.inv;
    float2 ck = pbfft::cmul(kc, make_float2(kc.x * ir, kc.y * ir));
    ck = make_float2(-ck.x * h, -ck.y * h);
    const float ckb = q.inv - q.r * h;
    const float2 t1 = pbfft::cmul(ck, q.P), t2 = pbfft::cmul(q.cph, q.dP);
    const float2 s1 = pbfft::cmul(A, make_float2(t1.x + t2.x, t1.y + t2.y));
    const float2 s2 = pbfft::cmul(A, make_float2(ckb * q.P.x, ckb * q.P.y));
    return make_float2(s1.x + s2.x, s1.y - s2.y);
}

// grid (ceil(H / nb), slots): nb rows of one slot of (B,C,H,W) fp32 planes, element (c, j) at s[c * nb + j]
template <int NTH>
__global__ __launch_bounds__(NTH) void phaseg_rows_fwd(const float *__restrict__ src, float2 *__restrict__ G, int slot0, int C, int H,
                                                       int W, int lognb, pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int r0 = blockIdx.x << lognb;
    long plane; bool two;
    phase_slot(slot0 + blockIdx.y, C, plane, two);
    const float *p1 = src + plane * H * W, *p2 = p1 + (long)H * W;
    for (int idx = threadIdx.x; idx < (W << lognb); idx += NTH) {
        const int j = idx / W, c = idx - j * W, r = r0 + j;
        float2 v = make_float2(0.f, 0.f);
        if (r < H) {
            v.x = p1[(long)r * W + c];
            if (two) v.y = p2[(long)r * W + c];
        }
        sph[(c << lognb) + j] = v;
    }
    __syncthreads();
    pbfft::line_forward(sph, plan, lognb);
    float2 *dst = G + (long)blockIdx.y * H * W;
    for (int idx = threadIdx.x; idx < (W << lognb); idx += NTH) {
        const int j = idx / W, c = idx - j * W, r = r0 + j;
        if (r < H) dst[(long)r * W + c] = sph[(c << lognb) + j];
    }
}

// grid (kh): row i of the taps of one kernel at row (i - kh/2) mod H of the zeroed plane, transformed along x
template <int NTH>
__global__ __launch_bounds__(NTH) void phaseg_krows(const float *__restrict__ taps, float2 *__restrict__ K, int kh, int kw, int H, int W,
                                                    pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int i = blockIdx.x;
    for (int c = threadIdx.x; c < W; c += NTH) sph[c] = make_float2(0.f, 0.f);
    __syncthreads();
    for (int j = threadIdx.x; j < kw; j += NTH) {
        int c = j - kw / 2;
        if (c < 0) c += W;
        sph[c] = make_float2(taps[i * kw + j], 0.f);
    }
    __syncthreads();
    pbfft::line_forward(sph, plan, 0);
    int r = i - kh / 2;
    if (r < 0) r += H;
    for (int c = threadIdx.x; c < W; c += NTH) K[(long)r * W + c] = sph[c];
}

// nb adjacent columns of one plane interleaved: element (p, j) at s[p * nb + j] <-> g[p][c0 + j]; columns past W read as 0
template <int NTH>
__device__ __forceinline__ void phaseg_tile_load(float2 *s, const float2 *g, int H, int W, int c0, int lognb) {
    const int nb = 1 << lognb;
    for (int e = threadIdx.x; e < (H << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        s[e] = c < W ? g[(long)p * W + c] : make_float2(0.f, 0.f);
    }
    __syncthreads();
}

// grid (ceil(W / nb)): the kernel's plane along y, in place
template <int NTH>
__global__ __launch_bounds__(NTH) void phaseg_cols_k(float2 *K, int H, int W, int lognb, pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int nb = 1 << lognb, c0 = blockIdx.x << lognb;
    phaseg_tile_load<NTH>(sph, K, H, W, c0, lognb);
    pbfft::line_forward(sph, plan, lognb);
    for (int e = threadIdx.x; e < (H << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        if (c < W) K[(long)p * W + c] = sph[e];
    }
}

// grid (ceil(W / nb), slots): columns forward, times conj(M) / N, columns back, in place
template <int NTH>
__global__ __launch_bounds__(NTH) void phaseg_cols_x(float2 *G, const float2 *__restrict__ K, int H, int W, int lognb, pbfft::DevPlan plan,
                                                     float a3, float a2, float a1, float b, float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int nb = 1 << lognb, c0 = blockIdx.x << lognb;
    float2 *g = G + (long)blockIdx.y * H * W;
    phaseg_tile_load<NTH>(sph, g, H, W, c0, lognb);
    pbfft::line_forward(sph, plan, lognb);
    for (int e = threadIdx.x; e < (H << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        float2 z = make_float2(0.f, 0.f);
        if (c < W) {
            const PhaseBin q = phase_bin(K[(long)p * W + c], a3, a2, a1, b);
            const float2 m = pbfft::cmul(q.cph, q.P);
            z = pbfft::cmul(sph[e], make_float2(m.x * scale, -m.y * scale));
        }
        sph[e] = make_float2(z.x, -z.y);
    }
    __syncthreads();
    pbfft::line_inverse(sph, plan, lognb);
    for (int e = threadIdx.x; e < (H << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        if (c < W) g[(long)p * W + c] = make_float2(sph[e].x, -sph[e].y);
    }
}

// grid (ceil(W / nb)): the n slots of a group in index order -- columns of x forward (kept in X: a thread reads back what it
// wrote itself), columns of g forward, A = or += fft2(x) conj(fft2(g))
template <int NTH>
__global__ __launch_bounds__(NTH) void phaseg_cols_a(float2 *X, const float2 *G, float2 *A, int n, int first, int H, int W, int lognb,
                                                     pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int nb = 1 << lognb, c0 = blockIdx.x << lognb;
    for (int s = 0; s < n; ++s) {
        float2 *x = X + (long)s * H * W;
        phaseg_tile_load<NTH>(sph, x, H, W, c0, lognb);
        pbfft::line_forward(sph, plan, lognb);
        for (int e = threadIdx.x; e < (H << lognb); e += NTH) {
            const int p = e >> lognb, c = c0 + (e & (nb - 1));
            if (c < W) x[(long)p * W + c] = sph[e];
        }
        __syncthreads();
        phaseg_tile_load<NTH>(sph, G + (long)s * H * W, H, W, c0, lognb);
        pbfft::line_forward(sph, plan, lognb);
        for (int e = threadIdx.x; e < (H << lognb); e += NTH) {
            const int p = e >> lognb, c = c0 + (e & (nb - 1));
            if (c >= W) continue;
            const long at = (long)p * W + c;
            const float2 gv = sph[e];
            float2 v = pbfft::cmul(x[at], make_float2(gv.x, -gv.y));
            if (!(first && s == 0)) { const float2 a = A[at]; v = make_float2(a.x + v.x, a.y + v.y); }
            A[at] = v;
        }
        __syncthreads();
    }
}

// grid (ceil(W / nb)): S from A / N and K, transformed along y (fft(S): line_inverse takes S as it stands), in place; only
// the rows (i - kh/2) mod H, i < kh, are stored
template <int NTH>
__global__ __launch_bounds__(NTH) void phaseg_cols_s(float2 *A, const float2 *__restrict__ K, int kh, int H, int W, int lognb,
                                                     pbfft::DevPlan plan, float a3, float a2, float a1, float b, float scale) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int nb = 1 << lognb, c0 = blockIdx.x << lognb;
    for (int e = threadIdx.x; e < (H << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        float2 z = make_float2(0.f, 0.f);
        if (c < W) {
            const float2 a = A[(long)p * W + c];
            z = phase_tap_bin(make_float2(a.x * scale, a.y * scale), K[(long)p * W + c], a3, a2, a1, b);
        }
        sph[e] = z;
    }
    __syncthreads();
    pbfft::line_inverse(sph, plan, lognb);
    for (int e = threadIdx.x; e < (H << lognb); e += NTH) {
        const int p = e >> lognb, c = c0 + (e & (nb - 1));
        int i = p + kh / 2;
        if (i >= H) i -= H;
        if (c < W && i < kh) A[(long)p * W + c] = sph[e];
    }
}

// grid (kh): row (i - kh/2) mod H of that plane transformed along x; tap (i, j) is the real part at column (j - kw/2) mod W
template <int NTH>
__global__ __launch_bounds__(NTH) void phaseg_taps_rows(const float2 *__restrict__ A, float *__restrict__ grad, int kh, int kw, int H, int W,
                                                        pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int i = blockIdx.x;
    int r = i - kh / 2;
    if (r < 0) r += H;
    for (int c = threadIdx.x; c < W; c += NTH) sph[c] = A[(long)r * W + c];
    __syncthreads();
    pbfft::line_inverse(sph, plan, 0);
    for (int j = threadIdx.x; j < kw; j += NTH) {
        int c = j - kw / 2;
        if (c < 0) c += W;
        grad[i * kw + j] = sph[c].x;
    }
}

// grid (ceil(H / nb), slots): the rows back along x; plane 2q from the real part, plane 2q + 1 from the imaginary part
template <int NTH>
__global__ __launch_bounds__(NTH) void phaseg_rows_inv(const float2 *__restrict__ G, float *__restrict__ out, int slot0, int C, int H, int W,
                                                       int lognb, pbfft::DevPlan plan) {
    extern __shared__ __attribute__((aligned(16))) float2 sph[];
    const int r0 = blockIdx.x << lognb;
    long plane; bool two;
    phase_slot(slot0 + blockIdx.y, C, plane, two);
    const float2 *src = G + (long)blockIdx.y * H * W;
    for (int idx = threadIdx.x; idx < (W << lognb); idx += NTH) {
        const int j = idx / W, c = idx - j * W, r = r0 + j;
        float2 v = make_float2(0.f, 0.f);
        if (r < H) v = src[(long)r * W + c];
        sph[(c << lognb) + j] = make_float2(v.x, -v.y);
    }
    __syncthreads();
    pbfft::line_inverse(sph, plan, lognb);
    float *o1 = out + plane * H * W, *o2 = o1 + (long)H * W;
    for (int idx = threadIdx.x; idx < (W << lognb); idx += NTH) {
        const int j = idx / W, c = idx - j * W, r = r0 + j;
        if (r >= H) continue;
        const float2 v = sph[(c << lognb) + j];                  // conj(x1 + i x2)
        o1[(long)r * W + c] = v.x;
        if (two) o2[(long)r * W + c] = -v.y;
    }
}

}  // namespace

int pb_launch_phase_backward(pb_ctx *ctx, const PhaseGradCall &c) {
    const int H = c.H, W = c.W;
    int rc = pb_phase_sides_supported(ctx, H, W);
    if (rc) return rc;
    if (c.kh > H - 1 || c.kw > W - 1 || c.kh < 1 || c.kw < 1) return pb_fail(ctx, PB_ERR_BADARG, "a %d x %d kernel does not fit the %d x %d domain", c.kh, c.kw, H, W);
    const FftPlan *plw = pb_get_plan(ctx, W), *plh = pb_get_plan(ctx, H);
    if (!plw || !plh) return PB_ERR_NOMEM;
    const pbfft::DevPlan dpw = pbfft::dev_plan(plw), dph = pbfft::dev_plan(plh);
    const int lr = phase_rows_lognb(plw, H), lc = phase_cols_lognb(plh, W);
    const size_t lds_r = phase_lds(plw, lr), lds_c = phase_lds(plh, lc), lds_k = phase_lds(plw, 0);
    // scratch of its own: one complex plane for K, the slots of one group of plane pairs of g and -- for the taps -- as many of
    // x and one plane for A.  A group is as many pairs as the budget holds (two planes a pair with the taps), at least one
    const bool want_taps = c.grad_taps != nullptr;
    const size_t plane_bytes = sizeof(float2) * (size_t)H * W;
    const int spi = (c.C + 1) / 2;
    const size_t budget = ctx->phase_budget > 0 ? (size_t)ctx->phase_budget : (size_t)256 << 20;
    const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)spi, std::min<size_t>(budget / (plane_bytes * (want_taps ? 2 : 1)), 32768)));
    float2 *K = static_cast<float2 *>(pb_scratch(ctx, "phaseg.k", plane_bytes));
    float2 *G = static_cast<float2 *>(pb_scratch(ctx, "phaseg.g", plane_bytes * group));
    float2 *X = nullptr, *A = nullptr;
    if (want_taps) {
        X = static_cast<float2 *>(pb_scratch(ctx, "phaseg.x", plane_bytes * group));
        A = static_cast<float2 *>(pb_scratch(ctx, "phaseg.a", plane_bytes));
        if (!X || !A) return PB_ERR_NOMEM;
    }
    if (!K || !G) return PB_ERR_NOMEM;
    const float a3 = c.alpha / 2 - c.beta + 2, a2 = 3 * c.beta - c.alpha - 6, a1 = 5 - 3 * c.beta + c.alpha / 2;
    const float scale = (float)(1.0 / ((double)H * W));
    const dim3 grid_r((unsigned)((H + (1 << lr) - 1) >> lr)), grid_c((unsigned)((W + (1 << lc) - 1) >> lc));
    ProfScope prof(ctx, PB_PROF_CONV_FFT);
    for (int b = 0; b < c.B; ++b) {
        PB_HIP(hipMemsetAsync(K, 0, plane_bytes, ctx->stream));
        rc = phase_launch(ctx, phaseg_krows<256>, phaseg_krows<1024>, dim3(c.kh), lds_k, c.taps + (size_t)b * c.kh * c.kw, K, c.kh, c.kw, H, W, dpw);
        if (rc) return rc;
        rc = phase_launch(ctx, phaseg_cols_k<256>, phaseg_cols_k<1024>, grid_c, lds_c, K, H, W, lc, dph);
        if (rc) return rc;
        for (int s0 = 0; s0 < spi; s0 += group) {
            const int n = std::min(group, spi - s0), slot0 = b * spi + s0;
            const dim3 gr(grid_r.x, (unsigned)n), gc(grid_c.x, (unsigned)n);
            rc = phase_launch(ctx, phaseg_rows_fwd<256>, phaseg_rows_fwd<1024>, gr, lds_r, c.grad_out, G, slot0, c.C, H, W, lr, dpw);
            if (rc) return rc;
            if (want_taps) {
                rc = phase_launch(ctx, phaseg_rows_fwd<256>, phaseg_rows_fwd<1024>, gr, lds_r, c.x, X, slot0, c.C, H, W, lr, dpw);
                if (rc) return rc;
                rc = phase_launch(ctx, phaseg_cols_a<256>, phaseg_cols_a<1024>, grid_c, lds_c, X, (const float2 *)G, A, n, s0 == 0 ? 1 : 0, H, W, lc, dph);
                if (rc) return rc;
            }
            if (c.grad_x) {
                rc = phase_launch(ctx, phaseg_cols_x<256>, phaseg_cols_x<1024>, gc, lds_c, G, (const float2 *)K, H, W, lc, dph, a3, a2, a1, c.beta, scale);
                if (rc) return rc;
                rc = phase_launch(ctx, phaseg_rows_inv<256>, phaseg_rows_inv<1024>, gr, lds_r, (const float2 *)G, c.grad_x, slot0, c.C, H, W, lr, dpw);
                if (rc) return rc;
            }
        }
        if (want_taps) {
            rc = phase_launch(ctx, phaseg_cols_s<256>, phaseg_cols_s<1024>, grid_c, lds_c, A, (const float2 *)K, c.kh, H, W, lc, dph, a3, a2, a1, c.beta, scale);
            if (rc) return rc;
            rc = phase_launch(ctx, phaseg_taps_rows<256>, phaseg_taps_rows<1024>, dim3(c.kh), lds_k, (const float2 *)A, c.grad_taps + (size_t)b * c.kh * c.kw,
                              c.kh, c.kw, H, W, dpw);
            if (rc) return rc;
        }
    }
    return PB_OK;
}
