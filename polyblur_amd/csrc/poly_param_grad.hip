// The gradient of the deconvolution polynomial with respect to its two parameters.  For
//
//     out = a3 K^3 x + a2 K^2 x + a1 K x + beta x,   a3 = alpha / 2 - beta + 2,  a2 = 3 beta - alpha - 6,  a1 = 5 - 3 beta + alpha / 2
//
// (deblurring.py:122-138) and an upstream gradient G
//
//     d loss / d alpha = 1/2 <G, K (1 - K)^2 x>,      d loss / d beta = <G, (1 - K)^3 x>.
//
// Expanded into the dot products <G, K^i x> these cancel a hundredfold on a blurred image (four sums near 20 for a result near
// 0.25), so the detail images are formed instead -- u1 = x - K x, u2 = u1 - K u1, u3 = u2 - K u2, three plain Horner steps of the
// forward's own pass (api.hip: pb_compute_polynomial_taps_params_backward) -- and one streaming kernel here reads G, u2 and u3
// once:  d beta = sum G u3,  d alpha = 1/2 sum G (u2 - u3)  (K u2 = u2 - u3), per image over its C planes.
//
// Deterministic: no float atomics.  Image b gets `groups` workgroups; workgroup g of it takes the samples g * 256 + tid +
// k * groups * 256, k = 0, 1, ... in that order -- one sample per load, so that the order owes nothing to where the operands
// start: any element offset gives the aligned call's bits.  The product of two fp32 samples is exact in double, and the sums are
// double at every level (thread, wave, workgroup, image): an image's sum is rounded to fp32 once, at the store.
#include <algorithm>

#include "stage_math.h"

namespace {

constexpr int PG_NT = 256;

__global__ __launch_bounds__(PG_NT) void poly_param_partials(const float *__restrict__ grad_out, const float *__restrict__ u2,
                                                             const float *__restrict__ u3, double *__restrict__ partial, long n, int groups) {
    const int b = blockIdx.y, g = blockIdx.x;
    const long base = (long)b * n;
    const float *pg = grad_out + base, *p2 = u2 + base, *p3 = u3 + base;
    const long stride = (long)groups * PG_NT;
    double sa = 0.0, sb = 0.0;
    long i = (long)g * PG_NT + threadIdx.x;
    // (four samples in flight per thread; the sums take them in index order either way)
    for (; i + 3 * stride < n; i += 4 * stride) {
        const float g0 = pg[i], g1 = pg[i + stride], g2 = pg[i + 2 * stride], g3 = pg[i + 3 * stride];
        const float a0 = p2[i], a1 = p2[i + stride], a2 = p2[i + 2 * stride], a3 = p2[i + 3 * stride];
        const float b0 = p3[i], b1 = p3[i + stride], b2 = p3[i + 2 * stride], b3 = p3[i + 3 * stride];
        sb = fma((double)g0, (double)b0, sb); sa = fma((double)g0, (double)a0 - (double)b0, sa);
        sb = fma((double)g1, (double)b1, sb); sa = fma((double)g1, (double)a1 - (double)b1, sa);
        sb = fma((double)g2, (double)b2, sb); sa = fma((double)g2, (double)a2 - (double)b2, sa);
        sb = fma((double)g3, (double)b3, sb); sa = fma((double)g3, (double)a3 - (double)b3, sa);
    }
    for (; i < n; i += stride) {
        const float gv = pg[i], av = p2[i], bv = p3[i];
        sb = fma((double)gv, (double)bv, sb); sa = fma((double)gv, (double)av - (double)bv, sa);
    }
    __shared__ double red[PG_NT / 64];
    sa = pb_block_sum<double, PG_NT>(sa, red);
    sb = pb_block_sum<double, PG_NT>(sb, red);
    if (threadIdx.x == 0) {
        double *o = partial + 2 * ((long)b * groups + g);
        o[0] = sa; o[1] = sb;
    }
}

// one wave per image: lane l sums the partials l, l + 64, ... in index order, the lanes by xor shuffles;
// grad_params[b] = (1/2 sum_a, sum_b)
__global__ __launch_bounds__(64) void poly_param_fold(const double *__restrict__ partial, float *__restrict__ grad_params, int groups) {
    const int b = blockIdx.x;
    const double *p = partial + 2 * (long)b * groups;
    double sa = 0.0, sb = 0.0;
    for (int g = threadIdx.x; g < groups; g += 64) { sa += p[2 * g]; sb += p[2 * g + 1]; }
    sa = pb_wave_sum(sa); sb = pb_wave_sum(sb);
    if (threadIdx.x == 0) {
        grad_params[2 * b] = (float)(0.5 * sa);
        grad_params[2 * b + 1] = (float)sb;
    }
}

}  // namespace

// how many workgroups an image's n samples are dealt to: a function of the shape alone (eight samples a thread, about 2048
// workgroups over the batch)
int pb_poly_param_groups(int B, long n) {
    const long want = (n + PG_NT * 8 - 1) / (PG_NT * 8);
    const long cap = std::max(1, 2048 / std::max(B, 1));
    return (int)std::max(1L, std::min(want, cap));
}

// grad_params (B,2) = per image (1/2 sum G (u2 - u3), sum G u3) over its n = C * H * W samples.  Partials in the scratch
// "ppg.partial": 2 * B * pb_poly_param_groups doubles
int pb_launch_poly_param_reduce(pb_ctx *ctx, const float *grad_out, const float *u2, const float *u3, float *grad_params, int B, long n) {
    if (B < 1 || B > 65535) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "polynomial parameter gradient: %d images (the grid takes up to 65535)", B);
    const int groups = pb_poly_param_groups(B, n);
    double *partial = static_cast<double *>(pb_scratch(ctx, "ppg.partial", sizeof(double) * 2 * (size_t)B * groups));
    if (!partial) return PB_ERR_NOMEM;
    ProfScope prof(ctx, PB_PROF_OTHER);
    hipLaunchKernelGGL(poly_param_partials, dim3((unsigned)groups, (unsigned)B), dim3(PG_NT), 0, ctx->stream, grad_out, u2, u3, partial, n, groups);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(poly_param_fold, dim3((unsigned)B), dim3(64), 0, ctx->stream, partial, grad_params, groups);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
