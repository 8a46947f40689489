// The formulas a forward kernel and its backward have to agree on bit for bit, each stated once: the
// backward of a stage classifies a sample on a kink, finds an arg-max or compares with == exactly as the forward did
// because both call the definition below.  Also the fixed-order sums the project uses instead of float atomics.
// A change to a formula here changes every kernel that uses it together.
#pragma once
#include <cmath>

#include "common.h"

// ------------------------------------------------------------------------------------
// estimation
// ------------------------------------------------------------------------------------
// The gray sample of a pixel from the sum s of its C channels, summed in index order by the caller (blur_estimation.py:36:
// the mean over the channel axis; invc = 1 / C).  CC: the channel count where the kernel has it at compile time (1 or 3),
// 0 = any other
template <int CC> __device__ __forceinline__ float pb_gray_of(float s, float invc) { return CC == 1 ? s : (CC == 3 ? s / 3.0f : s * invc); }
__device__ __forceinline__ float pb_gray_of(float s, int C, float invc) {
    return (C == 1) ? s : ((C == 3) ? pb_gray_of<3>(s, invc) : pb_gray_of<0>(s, invc));
}
// ... of two and of four samples: one decision for the group
__device__ __forceinline__ void pb_gray_of(float &a, float &b, int C, float invc) {
    if (C == 3) { a = pb_gray_of<3>(a, invc); b = pb_gray_of<3>(b, invc); }
    else if (C != 1) { a = pb_gray_of<0>(a, invc); b = pb_gray_of<0>(b, invc); }
}
__device__ __forceinline__ float4 pb_gray_of(float4 s, int C, float invc) {
    if (C == 1) return s;
    if (C == 3) return make_float4(pb_gray_of<3>(s.x, invc), pb_gray_of<3>(s.y, invc), pb_gray_of<3>(s.z, invc), pb_gray_of<3>(s.w, invc));
    return make_float4(pb_gray_of<0>(s.x, invc), pb_gray_of<0>(s.y, invc), pb_gray_of<0>(s.z, invc), pb_gray_of<0>(s.w, invc));
}

// cos(t) gx - sin(t) gy of the directional maxima (blur_estimation.py:129-133) with its roundings written out (the second
// product rounded, the first fused into the difference), so that every kernel that folds a sample gets the same bits
__device__ __forceinline__ float pb_dir_proj(float cs, float sn, float dx, float dy) { return fmaf(cs, dx, -__fmul_rn(sn, dy)); }

// cos / sin of the directions t_k = k pi / n_angles, k < count (blur_estimation.py:129-131), evaluated once on the host in
// float: what every kernel that projects a gradient is handed
struct PbAngleTable {
    float cs[PB_MAX_ANGLES], sn[PB_MAX_ANGLES];
};
inline void pb_angle_table(int n_angles, float *cs, float *sn, int count) {
    for (int k = 0; k < count; ++k) {
        const float t = n_angles > 0 ? 3.14159265358979323846f * (float)k / (float)n_angles : 0.f;
        cs[k] = std::cos(t);
        sn[k] = std::sin(t);
    }
}

// The interpolated angle the estimation settles on, and the pair of indices whose magnitudes give sigma and rho
// (blur_estimation.py:160-169): i0 = the arg-min, or the index of a forced direction (force_theta_deg >= 0); i1 = the index
// of the direction 90 degrees on
__device__ __forceinline__ void pb_interp_pair(int i_min, int n_interp, float force_theta_deg, int *theta_deg, int *i0, int *i1) {
    const float step = 180.0f / (float)n_interp;
    int deg = (int)((float)i_min * step);                     // interpolated_thetas.long()
    if (force_theta_deg >= 0.f) {
        deg = (int)force_theta_deg;
        i_min = (int)((float)deg / step);
    }
    *theta_deg = deg;
    *i0 = i_min;
    *i1 = (int)((float)((deg + 90) % 180) / step);
}

// Magnitude to variance (blur_estimation.py:171-185): v = c^2 / (m^2 + eps) - b^2, clamped to [lo, hi] before the square
// root.  The float literals are the forward's; the double ones serve the re-evaluation of est_param_grad (estimate_grad.hip)
template <typename T> struct PbVariance;
template <> struct PbVariance<float> { static constexpr float eps = 1e-8f, lo = 0.09f, hi = 16.0f; };
template <> struct PbVariance<double> { static constexpr double eps = 1e-8, lo = 0.09, hi = 16.0; };
template <typename T> __device__ __forceinline__ T pb_variance_of(T m, T cc, T bb) { return cc / (m * m + PbVariance<T>::eps) - bb; }
// ... and its derivatives with respect to the model's own parameters (est_param_grad): d v / d c = 2 c / (m^2 + eps),
// d v / d b = -2 b
template <typename T> __device__ __forceinline__ T pb_variance_dc(T m, T c) { return T(2) * c / (m * m + PbVariance<T>::eps); }
template <typename T> __device__ __forceinline__ T pb_variance_db(T b) { return T(-2) * b; }
// whether the clamp passes v on (torch's clamp passes the gradient on the closed interval)
template <typename T> __device__ __forceinline__ bool pb_variance_passes(T v) { return v >= PbVariance<T>::lo && v <= PbVariance<T>::hi; }
__device__ __forceinline__ float pb_sigma_of(float v) { return sqrtf(fminf(fmaxf(v, PbVariance<float>::lo), PbVariance<float>::hi)); }
__device__ __forceinline__ double pb_sigma_of(double v) { return sqrt(fmin(fmax(v, PbVariance<double>::lo), PbVariance<double>::hi)); }

// ------------------------------------------------------------------------------------
// halo masking
// ------------------------------------------------------------------------------------
// M = -gx ox - gy gy (sic: deblurring.py:174 multiplies grad_y by itself), r = M / (nM + M), z = max(r, 0) of one sample;
// every rounding written out, so that the vector and the scalar form of a kernel, and the forward and the backward, give
// the same bits -- a sample on the kink r >= 0 is classified once
struct PbHalo { float M, den, r, z; };
__device__ __forceinline__ PbHalo pb_halo_ratio(float gx, float gy, float ox, float nM) {
    PbHalo h;
    h.M = fmaf(-gx, ox, -__fmul_rn(gy, gy));
    h.den = nM + h.M;
    h.r = h.M / h.den;
    h.z = fmaxf(h.r, 0.f);
    return h;
}

// ------------------------------------------------------------------------------------
// domain transform: the recursive filter and its backward (dt.hip, dt_grad.hip)
// ------------------------------------------------------------------------------------
// A call is 2 N one-dimensional passes, rows then columns for iteration k = 0 .. N - 1 (domain_transform.py:48-61), with
// a_k = exp(log_a_k), log_a_k = dt_log_a(sigma_s, k, N).  One pass along a line of n samples: input x (C channels), weights
// v_i = exp(d_i log_a_k) shared by the channels, d_i = 1 + ratio sum_c |J_c,i - J_c,i-1| for i >= 1, ratio = sigma_s / sigma_r.
//
//   forward   f_0 = x_0;            f_i = x_i + v_i (f_{i-1} - x_i)          i = 1 .. n-1
//             g_{n-1} = f_{n-1};    g_i = f_i + v_{i+1} (g_{i+1} - f_i)      i = n-2 .. 0
//   backward, given G (the adjoint of the pass's output g)
//             P_0 = G_0;            P_i = G_i + v_i P_{i-1}                  left -> right
//             fbar_i = (1 - v_{i+1}) P_i  (i < n-1);   fbar_{n-1} = P_{n-1}
//             Q_{n-1} = fbar_{n-1}; Q_i = fbar_i + v_{i+1} Q_{i+1}           right -> left
//             xbar_i = (1 - v_i) Q_i  (i >= 1);        xbar_0 = Q_0
//             vbar_i = sum_c P_{i-1} (g_i - f_{i-1}) + Q_i (f_{i-1} - x_i)   i >= 1
//   weights   Dbar_i = sum_k log_a_k v_{k,i} vbar_{k,i}      one plane for the rows (Dbar_x), one for the columns (Dbar_y)
//   guide     Jbar_c,i = ratio (s_c,i Dbar_i - s_c,i+1 Dbar_{i+1}),  s_c,i = sign(J_c,i - J_c,i-1),  sign(0) = 0; the terms
//             with i = 0 and with i + 1 = n are absent; the row term and the column term add
//
// xbar of a pass is G of the pass before it; xbar of the first pass is the gradient of the image (plus Jbar when the filter is
// guided by its own input).  The only kink, |J_i - J_{i-1}|, is a function of the inputs: the backward forms f, g and v again
// with its own arithmetic and owes nothing to the forward's bits.

// the filter's coefficient of iteration i of N (domain_transform.py:50,53), as the logarithm the kernels take
inline float dt_log_a(float sigma_s, int i, int N) {
    const double sigma_i = (double)sigma_s * std::sqrt(3.0) * std::pow(2.0, N - (i + 1)) / std::sqrt(std::pow(4.0, N) - 1.0);
    const float a = (float)std::exp(-std::sqrt(2.0) / sigma_i);
    return std::log(a);
}
// v = a^d from l1 = sum_c |J_c,i - J_c,i-1|, and the factor of that sum's derivative with respect to J_c,i
__device__ __forceinline__ float pb_dt_weight(float l1, float ratio, float log_a) { return expf((1.f + ratio * l1) * log_a); }
__device__ __forceinline__ float pb_dt_sign(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// ------------------------------------------------------------------------------------
// sums and extrema in a fixed order (no float atomics: the same call gives the same bits)
// ------------------------------------------------------------------------------------
// over the 64 lanes of a wave by xor shuffles: every lane gets the result
template <typename T> __device__ __forceinline__ T pb_wave_sum(T v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// (min, max) of a pair of running extrema, the two shuffles of a step side by side
__device__ __forceinline__ void pb_wave_minmax(float &lo, float &hi) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o));
        hi = fmaxf(hi, __shfl_xor(hi, o));
    }
}

// over a workgroup of NT threads: the waves in index order through red (NT / 64 entries of LDS).  Every thread gets the
// sum; a barrier stands before the write, so red may be used again at once
template <typename T, int NT> __device__ __forceinline__ T pb_block_sum(T v, T *red) {
    v = pb_wave_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    T s = 0;
    for (int w = 0; w < NT / 64; ++w) s += red[w];
    return s;
}
// ... thread 0 alone gets the sum (the others 0), and no barrier stands before the write: one use of red.  The workgroups'
// sums are then folded by pb_fold_partials_kernel (common.h)
template <int NT> __device__ __forceinline__ float pb_block_sum_to_first(float v, float *red) {
    v = pb_wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x != 0) return 0.f;
    float t = 0.f;
    for (int w = 0; w < NT / 64; ++w) t += red[w];
    return t;
}
