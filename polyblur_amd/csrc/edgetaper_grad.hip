// The backward of the edgetaper's blends (reference edgetaper.py:10-33, differentiated there by ATen's autograd).
//
// One blend is  x' = A x + (1 - A) (K x),  A[py][px] = v1[py] v2[px],  v[p] = 1 - z[p] / ac[0],  z[p] = ac[p] + ac[n - 1 - p],
// ac the autocorrelation of the kernel's projection onto that axis.  With g the gradient that arrives at x':
//
//     u = (1 - A) g            the upstream of K x: K^T u is the adjoint pass, L(u, x) the lag correlation (conv_grad.hip)
//     g_x = A g + K^T u        (the pass adds ag = A g as its x operand)
//     Abar += sum over the image's planes of g (x - K x)
//
// etg_blend_kernel forms u, ag and Abar in one sweep -- one thread per sample of the domain, the image's C planes in index
// order, Abar read and written by the thread that owns the sample: an order the shape alone fixes, no atomics.  After the last
// blend the chain runs once per kernel: etg_reduce_kernel folds Abar to vbar1[py] = sum_px Abar v2[px] and
// vbar2[px] = sum_py Abar v1[py] -- one workgroup per row or column of the RING, the lines within kh - 1 (kw - 1) samples of an
// end: z is zero on every other line, so their vbar is never read and stored as 0 --, and etg_chain_kernel takes
//
//     zbar[p] = -vbar[p] / ac[0];  acbar[l] = zbar[l] + zbar[n - 1 - l];  acbar[0] += sum_p vbar[p] z[p] / ac[0]^2
//     kbar[m] = sum_l acbar[l] (k[m + l] + k[m - l])                  (k: the projection, zero outside 0 .. side - 1)
//
// per axis and adds kbar_y[i] + kbar_x[j] into tap (i, j) of the caller's orientation (a projection reflected has the same
// autocorrelation, and the sum above is symmetric in l, so the boundary's orientation plays no part).
//
// The weight is the forward's statement, restated: taper_weight (conv_common.h:38) and big_taper_weight (conv_big.hip:106) are
// one formula with 25 and 49 stored lags -- etg_weight takes the count --, reciprocal by __frcp_rn, read from the same
// autocorrelations the forward reads (the set's records or tables).
#include "common.h"
#include "stage_math.h"

namespace {

constexpr int EG_NT = 256;

__device__ __forceinline__ float etg_z(const float *ac, int p, int n, int nlag) {
    const int q = n - 1 - p;
    return ((p < nlag) ? ac[p] : 0.f) + ((q < nlag) ? ac[q] : 0.f);
}
__device__ __forceinline__ float etg_weight(const float *ac, int p, int n, int nlag) { return 1.f - etg_z(ac, p, n, nlag) * __frcp_rn(ac[0]); }

template <int V> struct EtgVec { float v[V]; };
template <int V> __device__ __forceinline__ EtgVec<V> etg_ld(const float *p) {
    EtgVec<V> r;
    if constexpr (V == 4) { const float4 t = *reinterpret_cast<const float4 *>(p); r.v[0] = t.x; r.v[1] = t.y; r.v[2] = t.z; r.v[3] = t.w; }
    else r.v[0] = *p;
    return r;
}
template <int V> __device__ __forceinline__ void etg_st(float *p, const EtgVec<V> &r) {
    if constexpr (V == 4) *reinterpret_cast<float4 *>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
    else *p = r.v[0];
}

// V samples of a row per thread: 4 -- 16-byte loads and stores -- where W is a multiple of 4 and every plane is 16-byte aligned,
// else 1; a sample's arithmetic is the same either way (the same bits)
template <int V>
__global__ __launch_bounds__(EG_NT) void etg_blend_kernel(const TaperAcorr ac, const float *__restrict__ x, const float *__restrict__ kx,
                                                         const float *__restrict__ g, float *__restrict__ u, float *__restrict__ ag,
                                                         float *__restrict__ abar, int first, int C, int H, int W) {
    const long HW = (long)H * W, p = ((long)blockIdx.x * EG_NT + threadIdx.x) * V;
    if (p >= HW) return;
    const int b = blockIdx.y, py = (int)(p / W), px = (int)(p - (long)py * W);
    const float wy = etg_weight(ac.acy + b * ac.stride, py, H, ac.nlag);
    float al[V], om[V];
    EtgVec<V> d;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        al[j] = wy * etg_weight(ac.acx + b * ac.stride, px + j, W, ac.nlag);
        om[j] = 1.f - al[j];
        d.v[j] = 0.f;
    }
    for (int c = 0; c < C; ++c) {
        const long o = ((long)b * C + c) * HW + p;
        const EtgVec<V> gv = etg_ld<V>(g + o);
        EtgVec<V> uv, av;
#pragma unroll
        for (int j = 0; j < V; ++j) { uv.v[j] = om[j] * gv.v[j]; av.v[j] = al[j] * gv.v[j]; }
        etg_st<V>(u + o, uv);
        etg_st<V>(ag + o, av);
        if (abar) {
            const EtgVec<V> xv = etg_ld<V>(x + o), kv = etg_ld<V>(kx + o);
#pragma unroll
            for (int j = 0; j < V; ++j) d.v[j] = fmaf(gv.v[j], xv.v[j] - kv.v[j], d.v[j]);
        }
    }
    if (abar) {
        float *a = abar + (long)b * HW + p;
        if (!first) {
            const EtgVec<V> old = etg_ld<V>(a);
#pragma unroll
            for (int j = 0; j < V; ++j) d.v[j] = old.v[j] + d.v[j];
        }
        etg_st<V>(a, d);
    }
}

// line < H: row `line`, weighted by v2; else column line - H, weighted by v1
__global__ __launch_bounds__(EG_NT) void etg_reduce_kernel(const TaperAcorr ac, const float *__restrict__ abar, float *__restrict__ vbar, int H,
                                                          int W, int kh, int kw) {
    __shared__ float red[EG_NT / 64];
    const int b = blockIdx.y, line = blockIdx.x;
    const bool row = line < H;
    const int p = row ? line : line - H, n = row ? H : W, k = row ? kh : kw;
    float *out = vbar + (long)b * (H + W) + line;
    if (!(p < k || n - 1 - p < k)) {                            // (the whole workgroup: not a line of the ring)
        if (threadIdx.x == 0) *out = 0.f;
        return;
    }
    const float *A = abar + (long)b * H * W;
    const float *aco = (row ? ac.acx : ac.acy) + b * ac.stride;
    const int m = row ? W : H;
    float s = 0.f;
    for (int t = threadIdx.x; t < m; t += EG_NT) {
        const float a = row ? A[(long)p * W + t] : A[(long)t * W + p];
        s = fmaf(a, etg_weight(aco, t, m, ac.nlag), s);
    }
    s = pb_block_sum<float, EG_NT>(s, red);
    if (threadIdx.x == 0) *out = s;
}

__global__ __launch_bounds__(64) void etg_chain_kernel(const TaperAcorr ac, const float *__restrict__ vbar, const float *__restrict__ raw,
                                                      float *__restrict__ grad, int H, int W, int kh, int kw) {
    __shared__ float proj[PB_KSIZE_MAX], acb[PB_KSIZE_MAX], kb[2][PB_KSIZE_MAX];
    const int b = blockIdx.x, t = threadIdx.x;
    const float *k = raw + (long)b * kh * kw;
    for (int ax = 0; ax < 2; ++ax) {
        const int kn = ax ? kw : kh, n = ax ? W : H;
        const float *a = (ax ? ac.acx : ac.acy) + b * ac.stride;
        const float *vb = vbar + (long)b * (H + W) + (ax ? H : 0);
        const float ac0 = a[0];
        __syncthreads();                                        // (the other axis has read proj and acb)
        if (t < kn) {
            float s = 0.f;
            if (ax) for (int i = 0; i < kh; ++i) s += k[i * kw + t];
            else for (int j = 0; j < kw; ++j) s += k[t * kw + j];
            proj[t] = s;
            float v = -(vb[t] + vb[n - 1 - t]) / ac0;           // lag t is read at p = t and at p = n - 1 - t (both, where they meet)
            if (t == 0) {
                float nrm = 0.f;                                // ac[0] also divides every z: the ring's lines, each once
                for (int p = 0; p < kn; ++p) nrm = fmaf(vb[p], etg_z(a, p, n, ac.nlag), nrm);
                for (int p = max(kn, n - kn); p < n; ++p) nrm = fmaf(vb[p], etg_z(a, p, n, ac.nlag), nrm);
                v += nrm / (ac0 * ac0);
            }
            acb[t] = v;
        }
        __syncthreads();
        if (t < kn) {
            float s = 0.f;
            for (int l = 0; l < kn; ++l) {
                const float pk = (t + l < kn ? proj[t + l] : 0.f) + (t - l >= 0 ? proj[t - l] : 0.f);
                s = fmaf(acb[l], pk, s);
            }
            kb[ax][t] = s;
        }
    }
    __syncthreads();
    float *o = grad + (long)b * kh * kw;
    for (int idx = t; idx < kh * kw; idx += 64) o[idx] += kb[0][idx / kw] + kb[1][idx % kw];
}

}  // namespace

int pb_launch_taper_blend_adjoint(pb_ctx *ctx, const TaperAcorr &ac, const float *x, const float *kx, const float *g, float *u, float *ag,
                                  float *abar, int first, int B, int C, int H, int W) {
    if (abar && (!x || !kx)) return pb_fail(ctx, PB_ERR_BADARG, "edgetaper backward: the weight gradient needs x and K x");
    uintptr_t bits = reinterpret_cast<uintptr_t>(g) | reinterpret_cast<uintptr_t>(u) | reinterpret_cast<uintptr_t>(ag);
    if (abar) bits |= reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(kx) | reinterpret_cast<uintptr_t>(abar);
    const int V = (W % 4 == 0 && bits % 16 == 0) ? 4 : 1;
    const long blocks = ((long)H * W / V + EG_NT - 1) / EG_NT;
    if (B > 65535 || blocks > 0x7fffffffL) return pb_fail(ctx, PB_ERR_BADARG, "edgetaper backward: bad grid");
    ProfScope prof(ctx, PB_PROF_OTHER);
    const dim3 grid((unsigned)blocks, (unsigned)B), block(EG_NT);
    if (V == 4) hipLaunchKernelGGL(etg_blend_kernel<4>, grid, block, 0, ctx->stream, ac, x, kx, g, u, ag, abar, first, C, H, W);
    else hipLaunchKernelGGL(etg_blend_kernel<1>, grid, block, 0, ctx->stream, ac, x, kx, g, u, ag, abar, first, C, H, W);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

int pb_launch_taper_weight_chain(pb_ctx *ctx, const TaperAcorr &ac, const float *abar, const float *raw, int kh, int kw, int B, int H, int W,
                                 float *grad_taps) {
    if (B > 65535 || kh < 1 || kw < 1 || kh > PB_KSIZE_MAX || kw > PB_KSIZE_MAX || kh > ac.nlag || kw > ac.nlag || kh > H - 1 || kw > W - 1)
        return pb_fail(ctx, PB_ERR_BADARG, "edgetaper backward: bad size %d x %d", kh, kw);
    float *vbar = static_cast<float *>(pb_scratch(ctx, "etg.vbar", sizeof(float) * (size_t)B * (H + W)));
    if (!vbar) return PB_ERR_NOMEM;
    ProfScope prof(ctx, PB_PROF_OTHER);
    hipLaunchKernelGGL(etg_reduce_kernel, dim3((unsigned)(H + W), (unsigned)B), dim3(EG_NT), 0, ctx->stream, ac, abar, vbar, H, W, kh, kw);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(etg_chain_kernel, dim3((unsigned)B), dim3(64), 0, ctx->stream, ac, vbar, raw, grad_taps, H, W, kh, kw);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
