// The backward pass of the domain-transform recursive filter: domain_transform.recursive_filter
// (domain_transform.py:6-85) under autograd, with respect to the image and to the guide.  The formulas -- the two sweeps of a
// pass, their adjoints P and Q, the weights' adjoint vbar, Dbar and the guide's gradient -- are stated once in stage_math.h.
//
// Launches of pb_dt_recursive_filter_backward, N iterations = 2 N passes (rows, columns, rows, ...):
//
//   the forward again   passes 0 .. 2 N - 2 with GRAD = false, each into its own plane set: the backward needs the INPUT of every
//                       pass (the output of the last one is never formed).  The filter's only kink, |J_i - J_{i-1}|, is decided by
//                       the inputs, so these are this file's own kernels and arithmetic, not the forward's forms.
//   the passes backward 2 N - 1 .. 0 with GRAD = true.  The first sweep (left to right, top to bottom) forms f and P together --
//                       both are the affine recurrence t_i = v_i t_{i-1} + b_i, with one slope -- and leaves them in two scratch
//                       plane sets; the second sweep (right to left, bottom to top) forms g and Q together -- again one slope,
//                       v_{i+1} -- and from them xbar and, where a guide gradient is asked for, log_a v_i vbar_i into Dbar_x
//                       (rows) or Dbar_y (columns): written by the last iteration's pass, added to by the earlier ones, each
//                       sample by the one lane that owns it.  xbar overwrites the pass's own upstream gradient, which the first
//                       sweep has consumed.
//   the guide           dtg_guide_kernel gathers Jbar from Dbar_x and Dbar_y: every sample reads its own two row terms and two
//                       column terms.  Not launched without a guide gradient; neither are the Dbar planes formed then.
//
// Rows: one wave per (image, row) over chunks of 64 samples, the maps composed by a wave scan (as dt.hip's row kernels); columns:
// one thread per (image, column), adjacent lanes = adjacent columns, the operands of DTG_U rows requested together before the
// dependent steps run (as dt.hip's column kernels).  One and three channels share the slope of the map among their channels
// (G = C); any other channel count runs the channels one after the other (G = 1), the weight formed from all C channels of J each
// time and Dbar added to channel by channel -- in index order by the same lane, so every sum is in an order the shape alone
// fixes: no float atomics, the same call gives the same bits.  No access is wider than one float: any element offset of the
// operands is as good as another.
//
// Scratch: "dtg.x" (2 N - 1 plane sets of (B,C,H,W) floats: the inputs of passes 1 .. 2 N - 1), "dtg.f", "dtg.p", "dtg.g" (one plane
// set each: f, P, and the gradient between passes) -- 2 N + 2 plane sets -- and, with a guide gradient, "dtg.dx" and "dtg.dy"
// ((B,H,W) floats each).
#include <algorithm>
#include <climits>
#include <cmath>

#include "stage_math.h"

namespace {

constexpr int NT = 256;
constexpr int DTG_U = 4;                               // rows whose operands a column thread requests together

// sum_c |J_c[i] - J_c[i - stride]| of the C channels at p = &J_0[i]
__device__ __forceinline__ float dtg_l1(const float *p, long HW, int C, long stride) {
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += fabsf(p[c * HW] - p[c * HW - stride]);
    return s;
}

// Wave-level inclusive scan of affine maps t -> ma t + mb[m] (one slope, M intercepts): after it lane l holds the composition
// of the maps of lanes 0 .. l, lane 0's applied first (dt.hip: compose)
template <int M> __device__ __forceinline__ void dtg_scan(float &ma, float (&mb)[M]) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float pa = __shfl_up(ma, o);
        float pb[M];
#pragma unroll
        for (int m = 0; m < M; ++m) pb[m] = __shfl_up(mb[m], o);
        if (lane >= o) {
#pragma unroll
            for (int m = 0; m < M; ++m) mb[m] = fmaf(ma, pb[m], mb[m]);
            ma *= pa;
        }
    }
}

// One horizontal pass over every row of every image.  GRAD = false: the forward, X -> Fb (f, then g in place).  GRAD = true: its
// backward -- X the pass's input, GB the gradient of its output, Fb / Pb scratch for f / P, XB the gradient of its input (may be
// GB), D the (B,H,W) plane Dbar_x or nullptr; acc: D is added to, not written.
template <int G, bool GRAD>
__global__ __launch_bounds__(NT) void dtg_rows_kernel(const float *J, const float *X, float *Fb, float *Pb, const float *GB, float *XB,
                                                      float *D, int acc, int C, int H, int W, float ratio, float log_a, long rows_total) {
    constexpr int M = GRAD ? 2 * G : G;
    const int lane = threadIdx.x & 63;
    const long row_id = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);   // over B*H: one wave = one row, every channel
    if (row_id >= rows_total) return;
    const long b = row_id / H;
    const int r = (int)(row_id - b * H);
    const long HW = (long)H * W, off = (b * C * H + r) * (long)W;
    const float *j = J + off;
    float *d = D ? D + (b * H + r) * (long)W : nullptr;
    const int last_base = ((W - 1) / 64) * 64;
    for (int c0 = 0; c0 < C; c0 += G) {
        const long o = off + c0 * HW;
        // ---- left -> right: f_i = v_i f_{i-1} + (1 - v_i) x_i and P_i = v_i P_{i-1} + G_i, f_0 = x_0, P_0 = G_0
        float carry[M];
#pragma unroll
        for (int m = 0; m < M; ++m) carry[m] = 0.f;
        for (int base = 0; base < W; base += 64) {
            const int i = base + lane;
            const bool in = i < W, first = i == 0;
            float v = 1.f;
            if (in && !first) v = pb_dt_weight(dtg_l1(j + i, HW, C, 1), ratio, log_a);
            float ma = in ? (first ? 0.f : v) : 1.f, mb[M];       // (lanes past the row: the identity)
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float x = in ? X[o + g * HW + i] : 0.f;
                mb[g] = first ? x : (1.f - v) * x;
                if constexpr (GRAD) mb[G + g] = in ? GB[o + g * HW + i] : 0.f;
            }
            dtg_scan<M>(ma, mb);
            const int src = base + 63 >= W ? (W - 1) - base : 63;   // the row's last sample, or the chunk's
#pragma unroll
            for (int m = 0; m < M; ++m) {
                const float y = fmaf(ma, carry[m], mb[m]);
                if (in) (m < G ? Fb : Pb)[o + (m % G) * HW + i] = y;
                carry[m] = __shfl(y, src);
            }
        }
        __threadfence_block();                               // the right-to-left sweep reads what other lanes have just written
        // ---- right -> left, lane l <-> sample base + 63 - l: g_i = v_{i+1} g_{i+1} + (1 - v_{i+1}) f_i and
        //      Q_i = v_{i+1} Q_{i+1} + (1 - v_{i+1}) P_i, g_{n-1} = f_{n-1}, Q_{n-1} = P_{n-1}
#pragma unroll
        for (int m = 0; m < M; ++m) carry[m] = 0.f;
        float vnext0 = 1.f;                                  // v of the first sample of the chunk to the right
        for (int base = last_base; base >= 0; base -= 64) {
            const int i = base + (63 - lane);
            const bool in = i < W, last = i >= W - 1;
            float v = 1.f;                                   // v_i: this sample's own, the slope of the sample to its left
            if (in && i > 0) v = pb_dt_weight(dtg_l1(j + i, HW, C, 1), ratio, log_a);
            float vr = __shfl_up(v, 1);                      // v_{i+1}
            if (lane == 0) vr = vnext0;
            vnext0 = __shfl(v, 63);
            float ma = in ? (last ? 0.f : vr) : 1.f, mb[M];
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float f = in ? Fb[o + g * HW + i] : 0.f;
                mb[g] = last ? f : (1.f - vr) * f;
                if constexpr (GRAD) {
                    const float p = in ? Pb[o + g * HW + i] : 0.f;
                    mb[G + g] = last ? p : (1.f - vr) * p;
                }
            }
            dtg_scan<M>(ma, mb);
            float vbar = 0.f;
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const float gi = fmaf(ma, carry[g], mb[g]);
                carry[g] = __shfl(gi, 63);                   // sample `base`, the left-most of this chunk
                if constexpr (!GRAD) {
                    if (in) Fb[o + g * HW + i] = gi;
                } else {
                    const float qi = fmaf(ma, carry[G + g], mb[G + g]);
                    carry[G + g] = __shfl(qi, 63);
                    if (in) {
                        XB[o + g * HW + i] = i > 0 ? (1.f - v) * qi : qi;
                        if (d && i > 0) {
                            const float fl = Fb[o + g * HW + i - 1], pl = Pb[o + g * HW + i - 1];
                            vbar += pl * (gi - fl) + qi * (fl - X[o + g * HW + i]);
                        }
                    }
                }
            }
            if constexpr (GRAD) {
                if (d && in) {
                    const float t = i > 0 ? log_a * v * vbar : 0.f;
                    d[i] = (acc || c0 > 0) ? d[i] + t : t;
                }
            }
        }
    }
}

// One vertical pass; thread = (image, column), the operands as dtg_rows_kernel's.  D: the plane Dbar_y.
template <int G, bool GRAD>
__global__ __launch_bounds__(NT) void dtg_cols_kernel(const float *J, const float *X, float *Fb, float *Pb, const float *GB, float *XB,
                                                      float *D, int acc, int C, int H, int W, float ratio, float log_a, long cols_total) {
    const long id = (long)blockIdx.x * NT + threadIdx.x;     // over B*W
    if (id >= cols_total) return;
    const long b = id / W;
    const int col = (int)(id - b * W);
    const long HW = (long)H * W, off = b * C * HW + col;
    const float *j = J + off;
    float *d = D ? D + b * HW + col : nullptr;
    for (int c0 = 0; c0 < C; c0 += G) {
        const long o = off + c0 * HW;
        // ---- top -> bottom: f and P
        float fp[G], pp[G];
#pragma unroll
        for (int g = 0; g < G; ++g) {
            fp[g] = X[o + g * HW];
            Fb[o + g * HW] = fp[g];
            if constexpr (GRAD) {
                pp[g] = GB[o + g * HW];
                Pb[o + g * HW] = pp[g];
            }
        }
        for (int r0 = 1; r0 < H; r0 += DTG_U) {
            float xs[DTG_U][G], gs[DTG_U][G], l1[DTG_U];
#pragma unroll
            for (int u = 0; u < DTG_U; ++u) {
                const long rw = (long)min(r0 + u, H - 1) * W;     // (rows past the end: the last row again -- loaded, never used)
                l1[u] = dtg_l1(j + rw, HW, C, W);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    xs[u][g] = X[o + g * HW + rw];
                    if constexpr (GRAD) gs[u][g] = GB[o + g * HW + rw];
                }
            }
#pragma unroll
            for (int u = 0; u < DTG_U; ++u) {
                if (r0 + u < H) {
                    const long rw = (long)(r0 + u) * W;
                    const float v = pb_dt_weight(l1[u], ratio, log_a);
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        fp[g] = xs[u][g] + v * (fp[g] - xs[u][g]);
                        Fb[o + g * HW + rw] = fp[g];
                        if constexpr (GRAD) {
                            pp[g] = fmaf(v, pp[g], gs[u][g]);
                            Pb[o + g * HW + rw] = pp[g];
                        }
                    }
                }
            }
        }
        // ---- bottom -> top: g and Q, xbar and vbar
        float gn[G], qn[G], vn = 0.f;                         // g, Q and v of the row below
#pragma unroll
        for (int g = 0; g < G; ++g) { gn[g] = 0.f; qn[g] = 0.f; }
        for (int r0 = H - 1; r0 >= 0; r0 -= DTG_U) {
            float fs[DTG_U + 1][G], ps[DTG_U + 1][G], xs[DTG_U][G], l1[DTG_U];   // f and P of rows r0 .. r0 - DTG_U
#pragma unroll
            for (int u = 0; u <= DTG_U; ++u) {
                const long rw = (long)max(r0 - u, 0) * W;         // (rows above the plane: row 0 again -- loaded, never used)
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    fs[u][g] = Fb[o + g * HW + rw];
                    if constexpr (GRAD) ps[u][g] = Pb[o + g * HW + rw];
                }
            }
#pragma unroll
            for (int u = 0; u < DTG_U; ++u) {
                const int r = max(r0 - u, 0);
                l1[u] = r > 0 ? dtg_l1(j + (long)r * W, HW, C, W) : 0.f;
                if constexpr (GRAD) {
#pragma unroll
                    for (int g = 0; g < G; ++g) xs[u][g] = X[o + g * HW + (long)r * W];
                }
            }
#pragma unroll
            for (int u = 0; u < DTG_U; ++u) {
                const int r = r0 - u;
                if (r >= 0) {
                    const long rw = (long)r * W;
                    const float v = r > 0 ? pb_dt_weight(l1[u], ratio, log_a) : 0.f;
                    float vbar = 0.f;
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const float f = fs[u][g];
                        const float gi = r == H - 1 ? f : f + vn * (gn[g] - f);
                        gn[g] = gi;
                        if constexpr (!GRAD) {
                            Fb[o + g * HW + rw] = gi;
                        } else {
                            const float p = ps[u][g];
                            const float qi = r == H - 1 ? p : fmaf(vn, qn[g], (1.f - vn) * p);
                            qn[g] = qi;
                            XB[o + g * HW + rw] = r > 0 ? (1.f - v) * qi : qi;
                            if (d && r > 0) vbar += ps[u + 1][g] * (gi - fs[u + 1][g]) + qi * (fs[u + 1][g] - xs[u][g]);
                        }
                    }
                    if constexpr (GRAD) {
                        if (d) {
                            const float t = r > 0 ? log_a * v * vbar : 0.f;
                            d[rw] = (acc || c0 > 0) ? d[rw] + t : t;
                        }
                    }
                    vn = v;
                }
            }
        }
    }
}

// out_c[y][x] = (add ? add_c[y][x] : 0) + ratio (s_x Dx[y][x] - s_{x+1} Dx[y][x+1] + s_y Dy[y][x] - s_{y+1} Dy[y+1][x]), s the sign
// of J_c's difference over that step; add may be out
__global__ __launch_bounds__(NT) void dtg_guide_kernel(const float *J, const float *Dx, const float *Dy, const float *add, float *out,
                                                       int B, int C, int H, int W, float ratio) {
    const long HW = (long)H * W;
    for (int b = blockIdx.y; b < B; b += gridDim.y)              // (grid.y is capped at 65535)
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < HW; i += (long)gridDim.x * NT) {
        const float *jb = J + (long)b * C * HW, *dx = Dx + (long)b * HW, *dy = Dy + (long)b * HW;
        const int y = (int)(i / W), x = (int)(i - (long)y * W);
        const bool xm = x > 0, xp = x + 1 < W, ym = y > 0, yp = y + 1 < H;
        const float dxm = xm ? dx[i] : 0.f, dxp = xp ? dx[i + 1] : 0.f, dym = ym ? dy[i] : 0.f, dyp = yp ? dy[i + W] : 0.f;
        for (int c = 0; c < C; ++c) {
            const float *p = jb + c * HW + i;
            const float v = *p;
            float t = 0.f;
            if (xm) t += pb_dt_sign(v - p[-1]) * dxm;
            if (xp) t -= pb_dt_sign(p[1] - v) * dxp;
            if (ym) t += pb_dt_sign(v - p[-W]) * dym;
            if (yp) t -= pb_dt_sign(p[W] - v) * dyp;
            const long k = ((long)b * C + c) * HW + i;
            out[k] = add ? add[k] + ratio * t : ratio * t;
        }
    }
}

struct DtgPass {
    const float *J, *X;
    float *Fb, *Pb;
    const float *GB;
    float *XB, *D;
    int acc;
    float log_a;
};

template <int G, bool GRAD>
void dtg_launch(pb_ctx *ctx, bool rows, const DtgPass &p, int B, int C, int H, int W, float ratio) {
    if (rows) {
        const long rows_total = (long)B * H;
        hipLaunchKernelGGL((dtg_rows_kernel<G, GRAD>), dim3((unsigned)((rows_total + NT / 64 - 1) / (NT / 64))), dim3(NT), 0, ctx->stream,
                           p.J, p.X, p.Fb, p.Pb, p.GB, p.XB, p.D, p.acc, C, H, W, ratio, p.log_a, rows_total);
    } else {
        const long cols_total = (long)B * W;
        hipLaunchKernelGGL((dtg_cols_kernel<G, GRAD>), dim3((unsigned)((cols_total + NT - 1) / NT)), dim3(NT), 0, ctx->stream,
                           p.J, p.X, p.Fb, p.Pb, p.GB, p.XB, p.D, p.acc, C, H, W, ratio, p.log_a, cols_total);
    }
}

template <int G>
int dtg_run(pb_ctx *ctx, const float *in, const float *J, const float *grad_out, float *grad_x, float *grad_guide, const float *guide_add,
            int B, int C, int H, int W, float sigma_s, float ratio, int N) {
    const long HW = (long)H * W;
    const size_t n = (size_t)B * C * HW, set = sizeof(float) * n;
    float *xs = static_cast<float *>(pb_scratch(ctx, "dtg.x", set * (size_t)(2 * N - 1)));
    float *fb = static_cast<float *>(pb_scratch(ctx, "dtg.f", set));
    float *pb = static_cast<float *>(pb_scratch(ctx, "dtg.p", set));
    float *gb = static_cast<float *>(pb_scratch(ctx, "dtg.g", set));
    if (!xs || !fb || !pb || !gb) return PB_ERR_NOMEM;
    float *dx = nullptr, *dy = nullptr;
    if (grad_guide) {
        dx = static_cast<float *>(pb_scratch(ctx, "dtg.dx", sizeof(float) * (size_t)B * HW));
        dy = static_cast<float *>(pb_scratch(ctx, "dtg.dy", sizeof(float) * (size_t)B * HW));
        if (!dx || !dy) return PB_ERR_NOMEM;
    }
    ProfScope prof(ctx, PB_PROF_PREFILTER);
    const int passes = 2 * N;
    auto input_of = [&](int p) { return p == 0 ? in : xs + (size_t)(p - 1) * n; };
    // the forward again: the input of every pass
    for (int p = 0; p + 1 < passes; ++p) {
        const DtgPass a{J, input_of(p), xs + (size_t)p * n, nullptr, nullptr, nullptr, nullptr, 0, dt_log_a(sigma_s, p / 2, N)};
        dtg_launch<G, false>(ctx, p % 2 == 0, a, B, C, H, W, ratio);
        PB_LAUNCH_CHECK();
    }
    // the passes backward
    for (int p = passes - 1; p >= 0; --p) {
        const bool rows = p % 2 == 0;
        const DtgPass a{J, input_of(p), fb, pb, p == passes - 1 ? grad_out : gb, p == 0 && grad_x ? grad_x : gb,
                        rows ? dx : dy, p / 2 < N - 1, dt_log_a(sigma_s, p / 2, N)};
        dtg_launch<G, true>(ctx, rows, a, B, C, H, W, ratio);
        PB_LAUNCH_CHECK();
    }
    if (grad_guide) {
        const dim3 grid((unsigned)std::min((HW + NT - 1) / NT, 2048l), (unsigned)std::min(B, 65535));
        hipLaunchKernelGGL(dtg_guide_kernel, grid, dim3(NT), 0, ctx->stream, J, dx, dy, guide_add, grad_guide, B, C, H, W, ratio);
        PB_LAUNCH_CHECK();
    }
    return PB_OK;
}

}  // namespace

extern "C" int pb_dt_recursive_filter_backward(pb_ctx *ctx, const float *in, const float *joint, const float *grad_out, float *grad_in,
                                               float *grad_joint, int B, int C, int H, int W, float sigma_s, float sigma_r,
                                               int num_iterations) {
    if (!ctx) return PB_ERR_BADARG;
    if (B < 1 || C < 1 || H < 1 || W < 1) return pb_fail(ctx, PB_ERR_BADARG, "bad shape (%d,%d,%d,%d)", B, C, H, W);
    if (!in || !grad_out) return pb_fail(ctx, PB_ERR_BADARG, "pb_dt_recursive_filter_backward: null argument");
    if (!grad_in && !grad_joint) return pb_fail(ctx, PB_ERR_BADARG, "pb_dt_recursive_filter_backward: no output asked for");
    if (!joint && grad_joint) return pb_fail(ctx, PB_ERR_BADARG, "pb_dt_recursive_filter_backward: grad_joint without joint (grad_in receives both paths)");
    for (const float *o : {static_cast<const float *>(grad_in), static_cast<const float *>(grad_joint)})
        if (o && (o == in || o == joint || o == grad_out)) return pb_fail(ctx, PB_ERR_BADARG, "pb_dt_recursive_filter_backward: an output may not alias an input");
    if (grad_in && grad_in == grad_joint) return pb_fail(ctx, PB_ERR_BADARG, "pb_dt_recursive_filter_backward: the outputs may not alias each other");
    if (!(sigma_s > 0.f) || !(sigma_r > 0.f) || !std::isfinite(sigma_s) || !std::isfinite(sigma_r))
        return pb_fail(ctx, PB_ERR_BADARG, "sigma_s and sigma_r must be positive and finite");
    if (num_iterations < 1) return pb_fail(ctx, PB_ERR_BADARG, "num_iterations must be at least 1 (got %d)", num_iterations);
    PB_HIP(hipSetDevice(ctx->device));
    const float ratio = sigma_s / sigma_r;
    // guided by its own input: the guide's gradient is added to the image's, in place on grad_in
    const float *J = joint ? joint : in;
    float *grad_guide = joint ? grad_joint : grad_in;
    const float *guide_add = joint ? nullptr : grad_in;
    return C == 3 ? dtg_run<3>(ctx, in, J, grad_out, grad_in, grad_guide, guide_add, B, C, H, W, sigma_s, ratio, num_iterations)
                  : dtg_run<1>(ctx, in, J, grad_out, grad_in, grad_guide, guide_add, B, C, H, W, sigma_s, ratio, num_iterations);
}
