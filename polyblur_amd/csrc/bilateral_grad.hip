// The backward pass of the bilateral filter: filters.bilateral_filter (filters.py:107-148) under autograd, with
// respect to the image.  Per plane v of H x W, R = ksize / 2, q over the window of p with the replicate pad as an index clamp:
//
//   s_pq = exp(-(dx^2 + dy^2) / (2 sigma_spatial^2))     d_pq = v_q - v_p     w_pq = s_pq exp(-d_pq^2 / (2 sigma_color^2))
//   D_p = sum_q w_pq       S1_p = sum_q w_pq d_pq       S2_p = sum_q w_pq d_pq^2
//   out_p = (v_p D_p + S1_p) / (D_p + 1e-5)             G_p = g_p / (D_p + 1e-5)         (g: the upstream gradient)
//
//   cen_p = G_p / sigma_color^2 (S2_p + (v_p - out_p) S1_p)                                  the centre of every weight of p's window
//   T_r'  = sum_{p in the image, |p - r'| <= R} G_p w_pr' (1 - (v_r' - out_p)(v_r' - v_p) / sigma_color^2)
//                                                          the taps: r' over the padded (H + 2 R) x (W + 2 R) domain, v_r' clamped
//   grad_v[r] = cen_r + sum_{r' that clamps to r} T_r'   the adjoint of the replicate pad: (R + 1)^2 positions at a corner
//
// Launches:
//
//   bilg_centre   the forward's layout (64 x 16 outputs and their halo in LDS, four vertically adjacent outputs per thread): one
//                 walk of the window gives D, S1, S2; writes out and G to scratch planes and cen to grad_in
//   bilg_taps     tiles the PADDED domain: v, G and out with a halo of R in LDS (G = 0 outside the image), gathers T into a padded
//                 scratch plane -- a gather, so no float atomics
//   bilg_fold     grad_in += the padded positions that clamp to the sample, in index order
//
// D and out are formed again with this file's own arithmetic (the filter has no kink: nothing depends on the forward's bits; ksize
// == 5 takes the same kernels as every other size here).  Every sum runs in an order the shape alone fixes: the same call gives
// the same bits.  The weight is one exponential, exp2(d^2 kc + (dx^2 + dy^2) ks1), as in the forward (bilateral.hip).
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace {

constexpr int NT = 256;
constexpr int TWB = 64, THB = 16;                      // outputs of a workgroup
constexpr int PER = THB / (NT / TWB);                  // vertically adjacent outputs of a thread
constexpr int RMAX = PB_KSIZE / 2;
constexpr int LW_MAX = TWB + 2 * RMAX, LH_MAX = THB + 2 * RMAX;        // 88 x 40 floats: 14 KB a tile
constexpr float EPS = 1e-5f;

struct BilgConst { float kc, ks1, ic2; };              // exp2's two factors, 1 / sigma_color^2

// One row of a thread's window in bilg_centre: the 2 R + 1 samples at `row` go to outputs LO .. HI of the thread's PER.
template <int LO, int HI>
__device__ __forceinline__ void centre_row(const float *__restrict__ row, int R, float kc, float ks1, const float (&ctr)[PER],
                                           const float (&ey)[PER], float (&den)[PER], float (&s1)[PER], float (&s2)[PER]) {
    float dx = (float)-R;
    for (int j = 0; j <= 2 * R; ++j) {
        const float v = row[j];
        const float dx2 = dx * dx;
        dx += 1.f;
#pragma unroll
        for (int o = LO; o <= HI; ++o) {
            const float d = v - ctr[o];
            const float w = __builtin_amdgcn_exp2f(fmaf(__fmul_rn(d, d), kc, fmaf(dx2, ks1, ey[o])));
            const float wd = __fmul_rn(w, d);
            den[o] += w;
            s1[o] += wd;
            s2[o] = fmaf(wd, d, s2[o]);
        }
    }
}

// One row of a thread's window in bilg_taps: the samples p of `vrow` with their G and out, for the padded positions LO .. HI of
// the thread's PER (ctr: their clamped samples).  d = v_p - v_r', so 1 - (v_r' - out_p)(v_r' - v_p) / sc^2 = 1 + (v_r' - out_p) d / sc^2.
template <int LO, int HI>
__device__ __forceinline__ void taps_row(const float *__restrict__ vrow, const float *__restrict__ grow, const float *__restrict__ orow,
                                         int R, float kc, float ks1, float ic2, const float (&ctr)[PER], const float (&ey)[PER],
                                         float (&acc)[PER]) {
    float dx = (float)-R;
    for (int j = 0; j <= 2 * R; ++j) {
        const float v = vrow[j], G = grow[j], op = orow[j];
        const float dx2 = dx * dx;
        dx += 1.f;
#pragma unroll
        for (int o = LO; o <= HI; ++o) {
            const float d = v - ctr[o];
            const float w = __builtin_amdgcn_exp2f(fmaf(__fmul_rn(d, d), kc, fmaf(dx2, ks1, ey[o])));
            const float f = fmaf(__fmul_rn(ctr[o] - op, d), ic2, 1.f);
            acc[o] = fmaf(__fmul_rn(G, w), f, acc[o]);
        }
    }
}

#define PB_BILG_ROWS(CALL)                                                     \
    switch (lo * PER + hi) {                                                   \
        case 0 * PER + 0: CALL(0, 0); break;                                   \
        case 0 * PER + 1: CALL(0, 1); break;                                   \
        case 0 * PER + 2: CALL(0, 2); break;                                   \
        case 0 * PER + 3: CALL(0, 3); break;                                   \
        case 1 * PER + 1: CALL(1, 1); break;                                   \
        case 1 * PER + 2: CALL(1, 2); break;                                   \
        case 1 * PER + 3: CALL(1, 3); break;                                   \
        case 2 * PER + 2: CALL(2, 2); break;                                   \
        case 2 * PER + 3: CALL(2, 3); break;                                   \
        case 3 * PER + 3: CALL(3, 3); break;                                   \
    }
static_assert(PER == 4, "the row cases are written for four outputs per thread");

// One workgroup per 64 x 16 tile of the image, as bilateral_kernel: the tile and its halo of R samples in LDS with the clamp, a
// thread walks the 4 + 2 R rows that the windows of its four outputs cover.  outp = out, Gp = g / (D + 1e-5), cen (into grad_in).
__global__ __launch_bounds__(NT) void bilg_centre(const float *__restrict__ in, const float *__restrict__ g, float *__restrict__ outp,
                                                  float *__restrict__ Gp, float *__restrict__ cen, int P, int H, int W, int R,
                                                  BilgConst k) {
    __shared__ float s[LH_MAX * LW_MAX];
    const int LW = TWB + 2 * R, LH = THB + 2 * R;
    const int x0 = blockIdx.x * TWB, y0 = blockIdx.y * THB;
    const int lane = threadIdx.x % TWB, wv = threadIdx.x / TWB;
    const int ty = wv * PER;
    const long HW = (long)H * W;
    for (int plane = blockIdx.z; plane < P; plane += gridDim.z) {      // (grid.z is capped at 65535)
        if (plane != (int)blockIdx.z) __syncthreads();
        const float *src = in + (long)plane * HW;
        for (int r = wv; r < LH; r += NT / TWB) {
            const int yy = min(max(y0 + r - R, 0), H - 1);             // replicate pad
            for (int c = lane; c < LW; c += TWB) {
                const int xx = min(max(x0 + c - R, 0), W - 1);
                s[r * LW + c] = src[(long)yy * W + xx];
            }
        }
        __syncthreads();
        float ctr[PER], den[PER], s1[PER], s2[PER], ey[PER];
#pragma unroll
        for (int o = 0; o < PER; ++o) {
            ctr[o] = s[(ty + o + R) * LW + lane + R];
            den[o] = 0.f;
            s1[o] = 0.f;
            s2[o] = 0.f;
        }
        for (int r = 0; r < PER + 2 * R; ++r) {                        // output o holds window row r where 0 <= r - o <= 2 R
            const float *row = s + (ty + r) * LW + lane;
#pragma unroll
            for (int o = 0; o < PER; ++o) {
                const float dy = (float)(r - o - R);
                ey[o] = dy * dy * k.ks1;
            }
            const int lo = max(r - 2 * R, 0), hi = min(r, PER - 1);
#define PB_CALL(LO, HI) centre_row<LO, HI>(row, R, k.kc, k.ks1, ctr, ey, den, s1, s2)
            PB_BILG_ROWS(PB_CALL)
#undef PB_CALL
        }
        const int xx = x0 + lane;
#pragma unroll
        for (int o = 0; o < PER; ++o) {
            const int yy = y0 + ty + o;
            if (yy < H && xx < W) {
                const long i = (long)plane * HW + (long)yy * W + xx;
                const float Dp = den[o] + EPS;
                const float out = fmaf(ctr[o], den[o], s1[o]) / Dp;
                const float G = g[i] / Dp;
                outp[i] = out;
                Gp[i] = G;
                cen[i] = __fmul_rn(__fmul_rn(G, k.ic2), fmaf(ctr[o] - out, s1[o], s2[o]));
            }
        }
    }
}

// One workgroup per 64 x 16 tile of the padded (H + 2 R) x (W + 2 R) domain.  LDS cell (r, c) of a tile at (X0, Y0) is the padded
// position (Y0 + r - R, X0 + c - R), the image position (Y0 + r - 2 R, X0 + c - 2 R): v with the clamp, G and out where that is
// inside the image, zero elsewhere (G = 0 takes the term out; every factor stays finite).  T: P planes of Hp x Wp.
__global__ __launch_bounds__(NT) void bilg_taps(const float *__restrict__ in, const float *__restrict__ outp, const float *__restrict__ Gp,
                                                float *__restrict__ T, int P, int H, int W, int R, BilgConst k) {
    __shared__ float sv[LH_MAX * LW_MAX], sg[LH_MAX * LW_MAX], so[LH_MAX * LW_MAX];
    const int LW = TWB + 2 * R, LH = THB + 2 * R;
    const int Hp = H + 2 * R, Wp = W + 2 * R;
    const int x0 = blockIdx.x * TWB, y0 = blockIdx.y * THB;            // padded coordinates
    const int lane = threadIdx.x % TWB, wv = threadIdx.x / TWB;
    const int ty = wv * PER;
    const long HW = (long)H * W, HWp = (long)Hp * Wp;
    for (int plane = blockIdx.z; plane < P; plane += gridDim.z) {
        if (plane != (int)blockIdx.z) __syncthreads();
        const long base = (long)plane * HW;
        for (int r = wv; r < LH; r += NT / TWB) {
            const int iy = y0 + r - 2 * R;
            const int yy = min(max(iy, 0), H - 1);
            for (int c = lane; c < LW; c += TWB) {
                const int ix = x0 + c - 2 * R;
                const int xx = min(max(ix, 0), W - 1);
                const long i = base + (long)yy * W + xx;
                const bool inside = iy == yy && ix == xx;
                sv[r * LW + c] = in[i];
                sg[r * LW + c] = inside ? Gp[i] : 0.f;
                so[r * LW + c] = inside ? outp[i] : 0.f;
            }
        }
        __syncthreads();
        float ctr[PER], acc[PER], ey[PER];
#pragma unroll
        for (int o = 0; o < PER; ++o) {
            ctr[o] = sv[(ty + o + R) * LW + lane + R];
            acc[o] = 0.f;
        }
        for (int r = 0; r < PER + 2 * R; ++r) {
            const int off = (ty + r) * LW + lane;
#pragma unroll
            for (int o = 0; o < PER; ++o) {
                const float dy = (float)(r - o - R);
                ey[o] = dy * dy * k.ks1;
            }
            const int lo = max(r - 2 * R, 0), hi = min(r, PER - 1);
#define PB_CALL(LO, HI) taps_row<LO, HI>(sv + off, sg + off, so + off, R, k.kc, k.ks1, k.ic2, ctr, ey, acc)
            PB_BILG_ROWS(PB_CALL)
#undef PB_CALL
        }
        const int xx = x0 + lane;
#pragma unroll
        for (int o = 0; o < PER; ++o) {
            const int yy = y0 + ty + o;
            if (yy < Hp && xx < Wp) T[(long)plane * HWp + (long)yy * Wp + xx] = acc[o];
        }
    }
}

// grad[r] += the padded positions that clamp to r, rows then columns in index order (one position for an interior sample)
__global__ __launch_bounds__(NT) void bilg_fold(const float *__restrict__ T, float *__restrict__ grad, long n, int H, int W, int R) {
    const int Wp = W + 2 * R;
    const long HW = (long)H * W, HWp = (long)(H + 2 * R) * Wp;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < n; i += (long)gridDim.x * NT) {
        const long plane = i / HW;
        const long rem = i - plane * HW;
        const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
        const int ya = y == 0 ? 0 : y + R, yb = y == H - 1 ? H - 1 + 2 * R : y + R;
        const int xa = x == 0 ? 0 : x + R, xb = x == W - 1 ? W - 1 + 2 * R : x + R;
        const float *t = T + plane * HWp;
        float s = 0.f;
        for (int yy = ya; yy <= yb; ++yy)
            for (int xx = xa; xx <= xb; ++xx) s += t[(long)yy * Wp + xx];
        grad[i] = grad[i] + s;
    }
}

}  // namespace

extern "C" int pb_bilateral_backward(pb_ctx *ctx, const float *in, const float *grad_out, float *grad_in, int B, int C, int H, int W,
                                     int ksize, float sigma_spatial, float sigma_color) {
    if (!ctx) return PB_ERR_BADARG;
    if (B < 1 || C < 1 || H < 2 || W < 2 || (long)B * C > INT_MAX) return pb_fail(ctx, PB_ERR_BADARG, "bad shape (%d,%d,%d,%d)", B, C, H, W);
    if (!in || !grad_out || !grad_in) return pb_fail(ctx, PB_ERR_BADARG, "pb_bilateral_backward: null argument");
    if (grad_in == in || grad_in == grad_out) return pb_fail(ctx, PB_ERR_BADARG, "pb_bilateral_backward: grad_in may not alias an input");
    if (ksize < 1 || ksize > PB_KSIZE || ksize % 2 == 0) return pb_fail(ctx, PB_ERR_BADARG, "ksize must be odd, from 1 to %d (got %d)", PB_KSIZE, ksize);
    if (!(sigma_spatial > 0.f) || !(sigma_color > 0.f) || !std::isfinite(sigma_spatial) || !std::isfinite(sigma_color))
        return pb_fail(ctx, PB_ERR_BADARG, "sigma_spatial and sigma_color must be positive and finite");
    const double log2e = 1.4426950408889634;
    BilgConst k;
    k.kc = (float)(-log2e / (2. * sigma_color * sigma_color));
    k.ks1 = (float)(-log2e / (2. * sigma_spatial * sigma_spatial));
    k.ic2 = (float)(1. / ((double)sigma_color * sigma_color));
    if (!std::isfinite(k.kc) || !std::isfinite(k.ks1) || !std::isfinite(k.ic2))
        return pb_fail(ctx, PB_ERR_BADARG, "sigma_spatial and sigma_color must be at least 1e-18");
    PB_HIP(hipSetDevice(ctx->device));
    const int P = B * C, R = ksize / 2;
    const long HW = (long)H * W, HWp = (long)(H + 2 * R) * (W + 2 * R);
    const size_t plane_bytes = sizeof(float) * (size_t)P * HW;
    float *outp = static_cast<float *>(pb_scratch(ctx, "bilg.out", plane_bytes));
    float *Gp = static_cast<float *>(pb_scratch(ctx, "bilg.G", plane_bytes));
    float *T = static_cast<float *>(pb_scratch(ctx, "bilg.T", sizeof(float) * (size_t)P * HWp));
    if (!outp || !Gp || !T) return PB_ERR_NOMEM;
    const unsigned gz = P < 65535 ? P : 65535;
    ProfScope prof(ctx, PB_PROF_PREFILTER);
    hipLaunchKernelGGL(bilg_centre, dim3((W + TWB - 1) / TWB, (H + THB - 1) / THB, gz), dim3(NT), 0, ctx->stream, in, grad_out, outp, Gp,
                       grad_in, P, H, W, R, k);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(bilg_taps, dim3((W + 2 * R + TWB - 1) / TWB, (H + 2 * R + THB - 1) / THB, gz), dim3(NT), 0, ctx->stream, in, outp, Gp,
                       T, P, H, W, R, k);
    PB_LAUNCH_CHECK();
    const long n = (long)P * HW;
    const unsigned blocks = (unsigned)std::min((n + NT - 1) / NT, 1L << 20);
    hipLaunchKernelGGL(bilg_fold, dim3(blocks), dim3(NT), 0, ctx->stream, T, grad_in, n, H, W, R);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
