// The backward pass of the blur estimation: d loss / d image of gaussian_blur_estimation
// (blur_estimation.py:18-79) for an upstream gradient of the ker_size x ker_size kernel and / or of (sigma, rho).  In the
// reference ATen's autograd walks the chain taps <- (sigma, rho) <- the two interpolated magnitudes <- the n_angles + 1
// directional maxima (torch.amax: to the arg-max pixel) <- the spectral derivative <- the range normalisation <- the channel
// mean; here five launches do:
//
//   est_gray_extrema   the gray plane (pb_gray_of, the forward's own, so that == gray_min / gray_max means what it meant there)
//                      and, per workgroup, how many samples sit at either end of the range
//   (the forward's spectral-derivative launchers: gradient planes of the gray image -- the arg-max of |proj| and its sign
//    do not depend on the positive factor 1 / (hi - lo))
//   est_dir_argmax     per direction the sample of largest |cos t gx - sin t gy|: (value, linear index) per thread, wave,
//   est_argmax_reduce  workgroup, image -- larger |value| first, then the lower index, at every level; no atomics
//   est_param_grad     one workgroup per image: the scalar chain from the forward's record, the 2 (n_angles + 1) row / column
//                      coefficients, d lo and d hi; where asked, d loss / d (c, b) of the affine model as well
//   est_grad_scatter   every output sample sums its row and column terms with the impulse response of the spectral
//                      derivative in closed form, adds its share of d lo / d hi, divides by C
//
// The formulas this file shares with the forward are the forward's own definitions (stage_math.h).
// The forward's decisions (i_min, theta, gray_min, gray_max, the clamps' state) come from its record; the arg-max pixels are found
// again, and the magnitudes, sigma and rho are evaluated again at those pixels in double (est_param_grad says why).  Sums in a
// fixed order, no float atomics: the same call gives the same bits.
#include <algorithm>
#include <cmath>

#include "stage_math.h"

namespace {

constexpr int EG_NT = 256;

// what est_param_grad leaves for the scatter, per image
struct EgCoef {
    float cx[PB_MAX_ANGLES], cy[PB_MAX_ANGLES];     // row / column coefficients, already divided by (hi - lo)
    int ia[PB_MAX_ANGLES], ja[PB_MAX_ANGLES];       // arg-max pixel of every direction (-1: none)
    float lo, hi, lo_share, hi_share;               // d lo / count(lo), d hi / count(hi)
};

struct EgSel {
    float p;         // the signed projection at the arg-max
    int idx;         // its linear index in the plane; 0x7fffffff: no sample (NaN planes)
};

__device__ __forceinline__ bool eg_better(float av, int ai, float bv, int bi) {   // is (bv, bi) ahead of (av, ai)?
    const float a = fabsf(av), b = fabsf(bv);
    return b > a || (b == a && bi < ai);
}

// impulse response of the spectral derivative along an axis of N samples (filters.py:172-184): out[j] = sum_m in[m] d[(j - m) mod N]
__device__ __forceinline__ float eg_deriv(int n, int N) {
    if (n == 0) return 0.f;
    // d[N - n] = -d[n]: the upper half through the lower one, where n / N <= 1/2 and sin(pi n / N) keeps the relative accuracy of
    // its argument (near n = N the rounding of n / N alone would cost N ulps)
    const bool upper = 2 * n > N;
    const int m = upper ? N - n : n;
    const float x = (float)m / (float)N;
    const float a = (((m & 1) != 0) != upper ? -3.14159265358979323846f : 3.14159265358979323846f) / (float)N;
    const float s = sinpif(x);
    return (N & 1) ? a / s : a * cospif(x) / s;              // (N even: the Nyquist bin is dropped by real(), d[N / 2] = 0)
}

__device__ __forceinline__ double eg_deriv_d(int n, int N) {                      // the same in double (est_param_grad)
    if (n == 0) return 0.0;
    const bool upper = 2 * n > N;
    const int m = upper ? N - n : n;
    const double x = (double)m / (double)N;
    const double a = (((m & 1) != 0) != upper ? -3.14159265358979323846 : 3.14159265358979323846) / (double)N;
    const double s = sinpi(x);
    return (N & 1) ? a / s : a * cospi(x) / s;
}

__device__ __forceinline__ float eg_gray(const float *src, long HW, long i, int C, float invc) {
    float s = src[i];
    for (int c = 1; c < C; ++c) s += src[c * HW + i];
    return pb_gray_of(s, C, invc);
}

__global__ __launch_bounds__(EG_NT) void est_gray_extrema(const float *__restrict__ in, const pb_blur_info *__restrict__ infos,
                                                          float *__restrict__ gray, uint2 *__restrict__ counts, int C, long HW, int bpi) {
    const int b = blockIdx.y, blk = blockIdx.x;
    const float *src = in + (long)b * C * HW;
    float *dst = gray + (long)b * HW;
    const float lo = infos[b].gray_min, hi = infos[b].gray_max, invc = 1.f / (float)C;
    unsigned nlo = 0, nhi = 0;
    for (long i = (long)blk * EG_NT + threadIdx.x; i < HW; i += (long)bpi * EG_NT) {
        const float g = eg_gray(src, HW, i, C, invc);
        dst[i] = g;
        nlo += g == lo ? 1u : 0u;
        nhi += g == hi ? 1u : 0u;
    }
    nlo = pb_wave_sum(nlo); nhi = pb_wave_sum(nhi);
    __shared__ unsigned slo[EG_NT / 64], shi[EG_NT / 64];
    if ((threadIdx.x & 63) == 0) { slo[threadIdx.x >> 6] = nlo; shi[threadIdx.x >> 6] = nhi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < EG_NT / 64; ++w) { nlo += slo[w]; nhi += shi[w]; }
        counts[(long)b * bpi + blk] = make_uint2(nlo, nhi);
    }
}

// VEC: HW % 4 == 0 -- the planes are walked in 16-byte units
template <bool VEC>
__global__ __launch_bounds__(EG_NT) void est_dir_argmax(const float *__restrict__ gx, const float *__restrict__ gy, const float *__restrict__ gray,
                                                        EgSel *__restrict__ part, long HW, int bpi, int na, int discard_sat, float thr,
                                                        PbAngleTable ang) {
    const int b = blockIdx.y, blk = blockIdx.x;
    const float *px = gx + (long)b * HW, *py = gy + (long)b * HW, *pg = gray + (long)b * HW;
    float bv[PB_MAX_ANGLES];
    int bi[PB_MAX_ANGLES];
#pragma unroll
    for (int k = 0; k < PB_MAX_ANGLES; ++k) { bv[k] = 0.f; bi[k] = 0x7fffffff; }
    // (a thread meets its samples in rising index order: a strictly larger |value| replaces, an equal one does not)
    auto fold = [&](float dx, float dy, int idx) {
#pragma unroll
        for (int k = 0; k < PB_MAX_ANGLES; ++k) {
            if (k < na) {
                const float p = pb_dir_proj(ang.cs[k], ang.sn[k], dx, dy);
                if (fabsf(p) > fabsf(bv[k]) || (bi[k] == 0x7fffffff && p == p)) { bv[k] = p; bi[k] = idx; }
            }
        }
    };
    if (VEC) {
        const long n4 = HW >> 2;
        for (long i = (long)blk * EG_NT + threadIdx.x; i < n4; i += (long)bpi * EG_NT) {
            const float4 x4 = *reinterpret_cast<const float4 *>(px + 4 * i), y4 = *reinterpret_cast<const float4 *>(py + 4 * i);
            float4 g4 = make_float4(0.f, 0.f, 0.f, 0.f);
            if (discard_sat) g4 = *reinterpret_cast<const float4 *>(pg + 4 * i);
            const int base = (int)(4 * i);
            if (!(discard_sat && g4.x > thr)) fold(x4.x, y4.x, base);
            if (!(discard_sat && g4.y > thr)) fold(x4.y, y4.y, base + 1);
            if (!(discard_sat && g4.z > thr)) fold(x4.z, y4.z, base + 2);
            if (!(discard_sat && g4.w > thr)) fold(x4.w, y4.w, base + 3);
        }
    } else {
        for (long i = (long)blk * EG_NT + threadIdx.x; i < HW; i += (long)bpi * EG_NT)
            if (!(discard_sat && pg[i] > thr)) fold(px[i], py[i], (int)i);
    }
    __shared__ float sv[EG_NT / 64][PB_MAX_ANGLES];
    __shared__ int si[EG_NT / 64][PB_MAX_ANGLES];
#pragma unroll
    for (int k = 0; k < PB_MAX_ANGLES; ++k) {
        float v = bv[k];
        int ix = bi[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o);
            const int oi = __shfl_xor(ix, o);
            if (eg_better(v, ix, ov, oi)) { v = ov; ix = oi; }
        }
        if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6][k] = v; si[threadIdx.x >> 6][k] = ix; }
    }
    __syncthreads();
    if ((int)threadIdx.x < na) {
        const int k = threadIdx.x;
        float v = sv[0][k];
        int ix = si[0][k];
        for (int w = 1; w < EG_NT / 64; ++w)
            if (eg_better(v, ix, sv[w][k], si[w][k])) { v = sv[w][k]; ix = si[w][k]; }
        EgSel s; s.p = v; s.idx = ix;
        part[((long)b * bpi + blk) * PB_MAX_ANGLES + k] = s;
    }
}

// one workgroup per image: the workgroups' partials -> one (value, index) per direction
__global__ __launch_bounds__(EG_NT) void est_argmax_reduce(const EgSel *__restrict__ part, EgSel *__restrict__ sel, int bpi, int na) {
    const int b = blockIdx.x;
    __shared__ float sv[EG_NT / 64];
    __shared__ int si[EG_NT / 64];
    for (int k = 0; k < na; ++k) {
        float v = 0.f;
        int ix = 0x7fffffff;
        for (int i = threadIdx.x; i < bpi; i += EG_NT) {
            const EgSel s = part[((long)b * bpi + i) * PB_MAX_ANGLES + k];
            if (eg_better(v, ix, s.p, s.idx)) { v = s.p; ix = s.idx; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ov = __shfl_xor(v, o);
            const int oi = __shfl_xor(ix, o);
            if (eg_better(v, ix, ov, oi)) { v = ov; ix = oi; }
        }
        __syncthreads();
        if ((threadIdx.x & 63) == 0) { sv[threadIdx.x >> 6] = v; si[threadIdx.x >> 6] = ix; }
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < EG_NT / 64; ++w)
                if (eg_better(v, ix, sv[w], si[w])) { v = sv[w]; ix = si[w]; }
            EgSel s; s.p = v; s.idx = ix;
            sel[(long)b * PB_MAX_ANGLES + k] = s;
        }
    }
}

__global__ __launch_bounds__(EG_NT) void est_param_grad(const pb_blur_info *__restrict__ infos, const float *__restrict__ grad_kernel,
                                                        const float *__restrict__ grad_sr, const float *__restrict__ wts,
                                                        const EgSel *__restrict__ sel, const float *__restrict__ gray,
                                                        const uint2 *__restrict__ counts, EgCoef *__restrict__ coefs, int H, int W,
                                                        int bpi_counts, int n_angles, int n_interp, float c, float bq, int ksize,
                                                        PbAngleTable ang, float *__restrict__ grad_cb) {
    const int b = blockIdx.x, tid = threadIdx.x;
    const pb_blur_info *info = infos + b;
    const int na = n_angles + 1;
    __shared__ float red[EG_NT / 64];
    __shared__ double redd[EG_NT / 64];
    __shared__ EgCoef sc;
    __shared__ unsigned s_cnt[2];
    __shared__ double s_mag[PB_MAX_ANGLES], s_par[2], s_m[2];
    __shared__ float s_sign[PB_MAX_ANGLES];
    __shared__ int s_im[2], s_pass[2];
    const float *g = gray + (long)b * H * W;
    // ---- what the forward DECIDED comes from its record: the direction (i_min, theta), the range (gray_min, gray_max: exact
    // minima / maxima), the clamp's state; where it looked is found again (sel).  What it MEASURED -- the directional maxima and,
    // from them, the two magnitudes, sigma and rho -- is evaluated again here at those pixels, in double: the record's fp32 values
    // carry the line transforms' rounding (sigma to about 1e-6 relative), which the chain below -- sums of upstream gradients
    // of any sign over the taps -- was measured to amplify fifteen-fold, past what an fp32 evaluation of the chain itself costs
    const float lo = info->gray_min, hi = info->gray_max;
    const double inv_d = hi > lo ? 1.0 / ((double)hi - (double)lo) : 0.0;
    if (tid < PB_MAX_ANGLES) {
        int ia = -1, ja = -1;
        if (tid < na) {
            const EgSel q = sel[(long)b * PB_MAX_ANGLES + tid];
            if (q.idx != 0x7fffffff && q.p != 0.f) { ia = q.idx / W; ja = q.idx - ia * W; }
        }
        sc.ia[tid] = ia; sc.ja[tid] = ja;
    }
    __syncthreads();
    for (int k = 0; k < na; ++k) {
        const int ia = sc.ia[k], ja = sc.ja[k];
        double sx = 0.0, sy = 0.0;
        if (ia >= 0) {                                          // (uniform)
            for (int m = tid; m < W; m += EG_NT) { int n = ja - m; if (n < 0) n += W; sx += eg_deriv_d(n, W) * (double)g[(long)ia * W + m]; }
            for (int m = tid; m < H; m += EG_NT) { int n = ia - m; if (n < 0) n += H; sy += eg_deriv_d(n, H) * (double)g[(long)m * W + ja]; }
        }
        sx = pb_block_sum<double, EG_NT>(sx, redd);
        sy = pb_block_sum<double, EG_NT>(sy, redd);
        if (tid == 0) {
            const double t = 3.14159265358979323846 * (double)k / (double)n_angles;
            const double p = cos(t) * sx - sin(t) * sy;
            s_mag[k] = ia >= 0 ? fabs(p) * inv_d : (double)info->mags[k];
            s_sign[k] = p > 0.0 ? 1.f : (p < 0.0 ? -1.f : 0.f);
        }
    }
    if (tid == 0) {
        int theta_deg;
        pb_interp_pair(min(max(info->i_min, 0), n_interp - 1), n_interp, -1.f, &theta_deg, &s_im[0], &s_im[1]);
        const double cc = (double)c * c, bb = (double)bq * bq;
        for (int e = 0; e < 2; ++e) {
            double m = 0.0;
            for (int k = 0; k < na; ++k) m += (double)wts[s_im[e] * na + k] * s_mag[k];
            // (the clamp's state is the forward's: its own fp32 value of v)
            const float mf = info->interp[s_im[e]];
            s_pass[e] = pb_variance_passes(pb_variance_of(mf, c * c, bq * bq)) ? 1 : 0;
            s_m[e] = m;
            s_par[e] = s_pass[e] ? pb_sigma_of(pb_variance_of(m, cc, bb)) : (double)(e == 0 ? info->sigma : info->rho);
        }
    }
    __syncthreads();
    // ---- taps -> (sigma, rho): K = E / sum E, E = exp(-Q / 2); gE = (g_K - sum g_K K) K; 625-term sums of any sign, in double
    const double theta = (double)info->theta, sigma = s_par[0], rho = s_par[1];
    double d_i1 = 0.0, d_i2 = 0.0;
    if (grad_kernel) {
        const int r = ksize / 2, kk = ksize * ksize;
        const float *gk = grad_kernel + (long)b * kk;
        const double ct = cos(-theta), st = sin(-theta);
        const double i1 = 1.0 / (sigma * sigma), i2 = 1.0 / (rho * rho);
        const double a00 = ct * ct * i1 + st * st * i2, a01 = st * ct * (i1 - i2), a11 = ct * ct * i2 + st * st * i1;
        double esum = 0.0, dot = 0.0;
        for (int i = tid; i < kk; i += EG_NT) {
            const int iy = i / ksize, ix = i - iy * ksize;
            const double X = ix - r, Y = iy - r;
            const double e = exp(-0.5 * (a00 * X * X + 2.0 * a01 * X * Y + a11 * Y * Y));
            esum += e; dot += (double)gk[i] * e;
        }
        esum = pb_block_sum<double, EG_NT>(esum, redd);
        dot = pb_block_sum<double, EG_NT>(dot, redd) / esum;
        double sxx = 0.0, sxy = 0.0, syy = 0.0;
        for (int i = tid; i < kk; i += EG_NT) {
            const int iy = i / ksize, ix = i - iy * ksize;
            const double X = ix - r, Y = iy - r;
            const double K = exp(-0.5 * (a00 * X * X + 2.0 * a01 * X * Y + a11 * Y * Y)) / esum;
            const double ge = ((double)gk[i] - dot) * K;
            sxx += ge * X * X; sxy += ge * X * Y; syy += ge * Y * Y;
        }
        sxx = pb_block_sum<double, EG_NT>(sxx, redd); sxy = pb_block_sum<double, EG_NT>(sxy, redd); syy = pb_block_sum<double, EG_NT>(syy, redd);
        const double cc = ct * ct, ss = st * st, sc2 = 2.0 * st * ct;
        d_i1 = -0.5 * (cc * sxx + sc2 * sxy + ss * syy);
        d_i2 = -0.5 * (ss * sxx - sc2 * sxy + cc * syy);
    }
    if (tid == 0) {
        double dpar[2] = {d_i1 * (-2.0 / (sigma * sigma * sigma)), d_i2 * (-2.0 / (rho * rho * rho))};
        if (grad_sr) { dpar[0] += (double)grad_sr[2 * b]; dpar[1] += (double)grad_sr[2 * b + 1]; }
        // (sigma, rho) -> the two interpolated magnitudes (blur_estimation.py:171-185; torch's clamp passes the gradient on
        // the closed interval)
        const double cc = (double)c * c;
        double dm[2], d_c = 0.0, d_b = 0.0;
        for (int e = 0; e < 2; ++e) {
            const double m = s_m[e], den = m * m + PbVariance<double>::eps;
            const double dv = s_pass[e] ? dpar[e] / (2.0 * s_par[e]) : 0.0;
            dm[e] = dv * (-2.0 * cc * m) / (den * den);
            // the model's own parameters: a clamped variance passes nothing on, dv is exactly 0
            d_c += dv * pb_variance_dc(m, (double)c);
            d_b += dv * pb_variance_db((double)bq);
        }
        if (grad_cb) { grad_cb[2 * b] = (float)d_c; grad_cb[2 * b + 1] = (float)d_b; }
        // interpolation and maxima: d mags = W^T d interp; the maxima were divided by the range
        for (int k = 0; k < PB_MAX_ANGLES; ++k) {
            float cx = 0.f, cy = 0.f;
            if (k < na && sc.ia[k] >= 0) {
                const double dmag = ((double)wts[s_im[0] * na + k] * dm[0] + (double)wts[s_im[1] * na + k] * dm[1]) * (double)s_sign[k] * inv_d;
                cx = (float)(dmag * (double)ang.cs[k]);
                cy = (float)(-dmag * (double)ang.sn[k]);
            }
            sc.cx[k] = cx; sc.cy[k] = cy;
        }
        sc.lo = lo; sc.hi = hi;
    }
    // how many samples sit at either end of the range
    unsigned nlo = 0, nhi = 0;
    for (int i = tid; i < bpi_counts; i += EG_NT) { const uint2 q = counts[(long)b * bpi_counts + i]; nlo += q.x; nhi += q.y; }
    nlo = pb_wave_sum(nlo); nhi = pb_wave_sum(nhi);
    if (tid == 0) { s_cnt[0] = 0u; s_cnt[1] = 0u; }
    __syncthreads();
    if ((tid & 63) == 0) { atomicAdd(&s_cnt[0], nlo); atomicAdd(&s_cnt[1], nhi); }       // (integers: any order, one sum)
    __syncthreads();
    // d lo, d hi: with d n the sparse gradient of the normalised plane (cx, cy carry 1 / (hi - lo) already),
    //   d lo = sum d n (g - hi) / (hi - lo),  d hi = -sum d n (g - lo) / (hi - lo)
    float t_lo = 0.f, t_hi = 0.f;
    for (int k = 0; k < na; ++k) {
        const int ia = sc.ia[k], ja = sc.ja[k];
        if (ia < 0) continue;                                  // (uniform)
        const float cx = sc.cx[k], cy = sc.cy[k];
        float a_lo = 0.f, a_hi = 0.f;
        for (int m = tid; m < W; m += EG_NT) {
            int n = ja - m; if (n < 0) n += W;
            const float d = eg_deriv(n, W), gv = g[(long)ia * W + m];
            a_lo = fmaf(d, gv - hi, a_lo); a_hi = fmaf(d, gv - lo, a_hi);
        }
        t_lo = fmaf(cx, a_lo, t_lo); t_hi = fmaf(cx, a_hi, t_hi);
        a_lo = 0.f; a_hi = 0.f;
        for (int m = tid; m < H; m += EG_NT) {
            int n = ia - m; if (n < 0) n += H;
            const float d = eg_deriv(n, H), gv = g[(long)m * W + ja];
            a_lo = fmaf(d, gv - hi, a_lo); a_hi = fmaf(d, gv - lo, a_hi);
        }
        t_lo = fmaf(cy, a_lo, t_lo); t_hi = fmaf(cy, a_hi, t_hi);
    }
    t_lo = pb_block_sum<float, EG_NT>(t_lo, red);
    t_hi = pb_block_sum<float, EG_NT>(t_hi, red);
    if (tid == 0) {
        const float inv = hi > lo ? 1.f / (hi - lo) : 0.f;
        sc.lo_share = s_cnt[0] ? t_lo * inv / (float)s_cnt[0] : 0.f;
        sc.hi_share = s_cnt[1] ? -t_hi * inv / (float)s_cnt[1] : 0.f;
        coefs[b] = sc;
    }
}

__global__ __launch_bounds__(EG_NT) void est_grad_scatter(const float *__restrict__ gray, const EgCoef *__restrict__ coefs,
                                                          float *__restrict__ grad_in, int C, int H, int W, int na) {
    const int b = blockIdx.y;
    __shared__ EgCoef sc;
    if (threadIdx.x == 0) sc = coefs[b];
    __syncthreads();
    const long HW = (long)H * W;
    const float *g = gray + (long)b * HW;
    float *out = grad_in + (long)b * C * HW;
    const float invc = 1.f / (float)C;
    for (long idx = (long)blockIdx.x * EG_NT + threadIdx.x; idx < HW; idx += (long)gridDim.x * EG_NT) {
        const int i = (int)(idx / W), j = (int)(idx - (long)i * W);
        float v = 0.f;
        for (int k = 0; k < na; ++k) {
            const int ia = sc.ia[k], ja = sc.ja[k];
            if (i == ia) { int n = ja - j; if (n < 0) n += W; v = fmaf(sc.cx[k], eg_deriv(n, W), v); }
            if (j == ja) { int n = ia - i; if (n < 0) n += H; v = fmaf(sc.cy[k], eg_deriv(n, H), v); }
        }
        const float gv = g[idx];
        if (gv == sc.lo) v += sc.lo_share;
        if (gv == sc.hi) v += sc.hi_share;
        v *= invc;
        for (int c = 0; c < C; ++c) out[c * HW + idx] = v;
    }
}

static int eg_blocks(long work, int B) {
    long n = (work + EG_NT * 8 - 1) / (EG_NT * 8);
    const long cap = std::max(1, 2048 / std::max(B, 1));
    return (int)std::max(1L, std::min(n, cap));
}

}  // namespace

// both entry points: grad_in (the image's gradient) and grad_cb (the model parameters') -- either may be null, not both
static int estimate_backward(pb_ctx *ctx, const char *who, const float *in, int B, int C, int H, int W, const pb_options *opt,
                             const pb_blur_info *dev_info, const float *grad_kernel, const float *grad_sigma_rho, int ker_size,
                             float *grad_in, float *grad_cb) {
    if (!in || !opt || !dev_info || (!grad_in && !grad_cb) || (!grad_kernel && !grad_sigma_rho))
        return pb_fail(ctx, PB_ERR_BADARG, "%s: null argument", who);
    if (grad_in == in) return pb_fail(ctx, PB_ERR_BADARG, "%s: grad_in may not alias in", who);
    if (grad_cb && (static_cast<const void *>(grad_cb) == in || grad_cb == grad_in || grad_cb == grad_kernel || grad_cb == grad_sigma_rho))
        return pb_fail(ctx, PB_ERR_BADARG, "%s: grad_cb aliases another argument", who);
    if (B < 1 || C < 1 || H < 2 || W < 2) return pb_fail(ctx, PB_ERR_BADARG, "bad shape (%d,%d,%d,%d)", B, C, H, W);
    if (opt->q != 0.f)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "%s: q = %g -- the backward of the quantile normalisation is not built (q = 0 only)", who, (double)opt->q);
    const int ksize = ker_size == 0 ? PB_KSIZE : ker_size;
    if (ksize < 1 || ksize > PB_KSIZE || !(ksize & 1))
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "%s: ker_size %d -- odd sizes up to %d only", who, ker_size, PB_KSIZE);
    if (opt->force_theta_deg >= 0.f) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "%s: not with a forced direction", who);
    if (opt->n_angles < 1 || opt->n_angles + 1 > PB_MAX_ANGLES || opt->n_interpolated_angles < 1 || opt->n_interpolated_angles > PB_MAX_INTERP)
        return pb_fail(ctx, PB_ERR_BADARG, "n_angles / n_interpolated_angles out of range");
    const long HW = (long)H * W;
    if (HW > 0x7fffffffL - 4) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "%s: planes of up to 2^31 samples", who);
    if (!pb_fft_length_supported(H) || !pb_fft_length_supported(W))
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "image %d x %d: lines of up to %d samples are supported", H, W, kMaxLineLength);
    PB_HIP(hipSetDevice(ctx->device));
    const int na = opt->n_angles + 1;
    const int bpi = eg_blocks(HW, B);
    const size_t plane = sizeof(float) * (size_t)B * HW;
    float *gray = static_cast<float *>(pb_scratch(ctx, "estg.gray", plane));
    float *gx = static_cast<float *>(pb_scratch(ctx, "estg.gx", plane));
    float *gy = static_cast<float *>(pb_scratch(ctx, "estg.gy", plane));
    // partials: per workgroup the end-of-range counts and the directions' (value, index); per image the directions' winners and
    // the coefficients
    const size_t part_bytes = (size_t)B * bpi * (sizeof(uint2) + sizeof(EgSel) * PB_MAX_ANGLES) + (size_t)B * (sizeof(EgSel) * PB_MAX_ANGLES + sizeof(EgCoef));
    char *part = static_cast<char *>(pb_scratch(ctx, "estg.part", part_bytes));
    if (!gray || !gx || !gy || !part) return PB_ERR_NOMEM;
    EgSel *apart = reinterpret_cast<EgSel *>(part);
    EgSel *sel = apart + (size_t)B * bpi * PB_MAX_ANGLES;
    EgCoef *coefs = reinterpret_cast<EgCoef *>(sel + (size_t)B * PB_MAX_ANGLES);
    uint2 *counts = reinterpret_cast<uint2 *>(coefs + B);
    const float *wts = pb_get_interp_weights(ctx, opt->n_angles, opt->n_interpolated_angles);
    if (!wts) return PB_ERR_NOMEM;
    PbAngleTable ang;
    pb_angle_table(opt->n_angles, ang.cs, ang.sn, PB_MAX_ANGLES);
    {
        ProfScope prof(ctx, PB_PROF_OTHER);
        hipLaunchKernelGGL(est_gray_extrema, dim3(bpi, B), dim3(EG_NT), 0, ctx->stream, in, dev_info, gray, counts, C, HW, bpi);
        PB_LAUNCH_CHECK();
    }
    int rc = pb_fourier_gradients_impl(ctx, gray, B, H, W, gx, gy);
    if (rc) return rc;
    ProfScope prof(ctx, PB_PROF_OTHER);
    const int sat = opt->discard_saturation ? 1 : 0;
    if ((HW & 3) == 0)
        hipLaunchKernelGGL(est_dir_argmax<true>, dim3(bpi, B), dim3(EG_NT), 0, ctx->stream, gx, gy, gray, apart, HW, bpi, na, sat, 0.99f, ang);
    else
        hipLaunchKernelGGL(est_dir_argmax<false>, dim3(bpi, B), dim3(EG_NT), 0, ctx->stream, gx, gy, gray, apart, HW, bpi, na, sat, 0.99f, ang);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(est_argmax_reduce, dim3(B), dim3(EG_NT), 0, ctx->stream, apart, sel, bpi, na);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(est_param_grad, dim3(B), dim3(EG_NT), 0, ctx->stream, dev_info, grad_kernel, grad_sigma_rho, wts, sel, gray, counts,
                       coefs, H, W, bpi, opt->n_angles, opt->n_interpolated_angles, opt->c, opt->b, ksize, ang, grad_cb);
    PB_LAUNCH_CHECK();
    if (!grad_in) return PB_OK;                              // (the parameters alone: nothing to scatter)
    hipLaunchKernelGGL(est_grad_scatter, dim3(bpi, B), dim3(EG_NT), 0, ctx->stream, gray, coefs, grad_in, C, H, W, na);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

extern "C" int pb_estimate_blur_backward(pb_ctx *ctx, const float *in, int B, int C, int H, int W, const pb_options *opt,
                                         const pb_blur_info *dev_info, const float *grad_kernel, const float *grad_sigma_rho,
                                         int ker_size, float *grad_in) {
    if (!ctx) return PB_ERR_BADARG;
    if (!grad_in) return pb_fail(ctx, PB_ERR_BADARG, "pb_estimate_blur_backward: null argument");
    return estimate_backward(ctx, "pb_estimate_blur_backward", in, B, C, H, W, opt, dev_info, grad_kernel, grad_sigma_rho, ker_size, grad_in, nullptr);
}

extern "C" int pb_estimate_blur_params_backward(pb_ctx *ctx, const float *in, int B, int C, int H, int W, const pb_options *opt,
                                                const pb_blur_info *dev_info, const float *grad_kernel, const float *grad_sigma_rho,
                                                int ker_size, float *grad_in, float *grad_cb) {
    if (!ctx) return PB_ERR_BADARG;
    return estimate_backward(ctx, "pb_estimate_blur_params_backward", in, B, C, H, W, opt, dev_info, grad_kernel, grad_sigma_rho, ker_size, grad_in, grad_cb);
}
