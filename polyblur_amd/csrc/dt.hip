// The domain-transform recursive filter (domain_transform.py:6-85, native twin RF.cpp:14-92): the prefilter of the pipeline
// (deblurring.py:80-88) and pb_dt_filter.  One- and three-channel images take the kernels without domain planes, in the forms
// choose_dt (dt_choice.h: every threshold and block size, with its measurement) picks once per call; other channel counts take
// dt_domain_kernel, dt_rows_kernel and dt_cols_kernel.
#include <algorithm>

#include "stage_math.h"

int pb_convert_to_float(pb_ctx *ctx, const void *in, int dtype, float *out, long n);      // filters.hip

namespace {

constexpr int NT = 256;

// The recurrence F[i] <- F[i] + V[i] (F[i-1] - F[i]) is the affine map F[i] = V[i] F[i-1] + (1-V[i]) x[i].
// Rows: one wave per (image, row); lanes own 64 consecutive columns and combine their maps with a
// wave-level inclusive scan (composition of affine maps), carrying the last value between chunks, so
// every global access is a coalesced 256-B row segment.  Columns: one thread per column walks down
// and up (adjacent lanes = adjacent columns, already coalesced).
//
// dom[i] = 1 + sigma_s/sigma_r * sum_c |J[c][i] - J[c][i-1]| (0 difference at i = 0);  V = a^dom.

template <typename T>
__global__ __launch_bounds__(NT) void dt_domain_kernel(const T *__restrict__ J, float *__restrict__ domx,
                                                       float *__restrict__ domy, int C, int H, int W, float ratio) {
    const int b = blockIdx.y;
    const long HW = (long)H * W;
    const T *src = J + (long)b * C * HW;
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < HW; i += (long)gridDim.x * NT) {
        const int r = (int)(i / W), c = (int)(i - (long)r * W);
        float dx = 0.f, dy = 0.f;
        for (int ch = 0; ch < C; ++ch) {
            const float v = pb_ld(src + ch * HW + i);
            if (c > 0) dx += fabsf(v - pb_ld(src + ch * HW + i - 1));
            if (r > 0) dy += fabsf(v - pb_ld(src + ch * HW + i - W));
        }
        domx[(long)b * HW + i] = 1.f + ratio * dx;
        domy[(long)b * HW + i] = 1.f + ratio * dy;
    }
}

struct Affine { float a, b; };   // f(t) = a t + b
__device__ __forceinline__ Affine compose(Affine second, Affine first) {   // second(first(t))
    return Affine{second.a * first.a, fmaf(second.a, first.b, second.b)};
}

// One horizontal pass (left->right then right->left) over every row of every plane, in place on F.
__global__ __launch_bounds__(NT) void dt_rows_kernel(float *__restrict__ F, const float *__restrict__ domx, int C, int H,
                                                     int W, float log_a, long rows_total) {
    const int lane = threadIdx.x & 63;
    const long row_id = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);   // over B*C*H
    if (row_id >= rows_total) return;
    const long plane = row_id / H;
    const int r = (int)(row_id - plane * H);
    const long b = plane / C;
    float *f = F + row_id * W;
    const float *d = domx + (b * H + r) * (long)W;
    // ---- left -> right:  F[i] = V[i] F[i-1] + (1 - V[i]) F[i],  i >= 1
    float carry = 0.f;
    for (int base = 0; base < W; base += 64) {
        const int i = base + lane;
        float x = 0.f, v = 1.f;
        if (i < W) { x = f[i]; v = expf(d[i] * log_a); }
        Affine m = (i == 0 || i >= W) ? Affine{0.f, x} : Affine{v, (1.f - v) * x};
        if (i >= W) m = Affine{1.f, 0.f};
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            Affine prev{__shfl_up(m.a, o), __shfl_up(m.b, o)};
            if (lane >= o) m = compose(m, prev);
        }
        const float y = fmaf(m.a, carry, m.b);
        if (i < W) f[i] = y;
        carry = __shfl(y, 63);
        if (base + 63 >= W) carry = __shfl(y, (W - 1) - base);
    }
    // ---- right -> left:  F[i] = V[i+1] F[i+1] + (1 - V[i+1]) F[i],  i <= W-2
    const int last_base = ((W - 1) / 64) * 64;
    carry = 0.f;
    for (int base = last_base; base >= 0; base -= 64) {
        const int i = base + (63 - lane);            // lane 0 handles the right-most element of the chunk
        float x = 0.f, v = 1.f;
        if (i < W) x = f[i];
        if (i + 1 < W) v = expf(d[i + 1] * log_a);
        Affine m = (i >= W - 1) ? Affine{0.f, x} : Affine{v, (1.f - v) * x};
        if (i >= W) m = Affine{1.f, 0.f};
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            Affine prev{__shfl_up(m.a, o), __shfl_up(m.b, o)};
            if (lane >= o) m = compose(m, prev);
        }
        const float y = fmaf(m.a, carry, m.b);
        if (i < W) f[i] = y;
        carry = __shfl(y, 63);                        // element `base`, the left-most of this chunk
    }
}

// One vertical pass (top->bottom then bottom->top) in place on F; thread = (plane, column).  The recurrence is
// sequential down a column, but its operands are not: the samples and domain weights of the next DT_U rows are
// fetched together before the U dependent steps run, so a column waits for memory once per U rows, not every row.
__global__ __launch_bounds__(NT) void dt_cols_kernel(float *__restrict__ F, const float *__restrict__ domy, int C, int H,
                                                     int W, float log_a, long cols_total) {
    const long id = (long)blockIdx.x * NT + threadIdx.x;   // over B*C*W
    if (id >= cols_total) return;
    const long plane = id / W;
    const int c = (int)(id - plane * W);
    const long b = plane / C;
    float *f = F + plane * (long)H * W + c;
    const float *d = domy + b * (long)H * W + c;
    float prev = f[0];
    for (int r0 = 1; r0 < H; r0 += DT_U) {
        float xs[DT_U], vs[DT_U];
#pragma unroll
        for (int u = 0; u < DT_U; ++u) {
            const int r = min(r0 + u, H - 1);
            xs[u] = f[(long)r * W];
            vs[u] = d[(long)r * W];
        }
#pragma unroll
        for (int u = 0; u < DT_U; ++u) {
            if (r0 + u < H) {
                const float v = expf(vs[u] * log_a);
                prev = xs[u] + v * (prev - xs[u]);
                f[(long)(r0 + u) * W] = prev;
            }
        }
    }
    for (int r0 = H - 2; r0 >= 0; r0 -= DT_U) {
        float xs[DT_U], vs[DT_U];
#pragma unroll
        for (int u = 0; u < DT_U; ++u) {
            const int r = max(r0 - u, 0);
            xs[u] = f[(long)r * W];
            vs[u] = d[(long)(r + 1) * W];
        }
#pragma unroll
        for (int u = 0; u < DT_U; ++u) {
            if (r0 - u >= 0) {
                const float v = expf(vs[u] * log_a);
                prev = xs[u] + v * (prev - xs[u]);
                f[(long)(r0 - u) * W] = prev;
            }
        }
    }
}

// ---- the same filter without the domain planes (C == 1 or 3) -----------------------------------------------------------
// dom is a function of two neighbouring samples of the joint image, which both passes have in hand or one cache line
// away: recomputing it where it is used removes dt_domain_kernel, its two fp32 planes per image (written once, read
// twice per pass) and the fp32 copy of the input -- 53 B per sample become 32 for fp32 images (44 -> 28 for fp16).
// Same expressions as the kernels above (the wave scan associates its products differently: last-bit differences).
// Wave-level inclusive scan of affine maps (shared slope ma, one intercept per channel) with DPP moves instead of LDS
// permutes: four row_shr steps inside each row of 16 lanes, then row_bcast:15 into rows 1 and 3 and row_bcast:31 into
// rows 2 and 3.  Lanes without a source take the identity map (1, 0), under which compose() returns its argument exactly.
// Round 6: a step is the instructions themselves -- v_fmac_f32_dpp mb, mb(lane - k), ma and v_mul_f32_dpp ma, ma(lane - k), ma, in
// place: a lane without a source, or in a masked row, is not written and keeps its map, which is what composing with the identity
// gave it (the builtin form spent a move of the identity and a move_dpp per operand on top of the arithmetic: 72 instructions
// per scan of three channels against 24; the row kernels are bound by instruction issue once the chip is full).  The products
// and sums are those of compose().  s_nop 1: a DPP operand wants two wait states behind the VALU write of its register, and the
// compiler's hazard pass does not look inside asm.
#define PB_DPP_SHR1 "row_shr:1 row_mask:0xf bank_mask:0xf"
#define PB_DPP_SHR2 "row_shr:2 row_mask:0xf bank_mask:0xf"
#define PB_DPP_SHR4 "row_shr:4 row_mask:0xf bank_mask:0xf"
#define PB_DPP_SHR8 "row_shr:8 row_mask:0xf bank_mask:0xf"
#define PB_DPP_BC15 "row_bcast:15 row_mask:0xa bank_mask:0xf"
#define PB_DPP_BC31 "row_bcast:31 row_mask:0xc bank_mask:0xf"
#define PB_SCAN_STEP1(CTRL)                                                                                          \
    asm("s_nop 1\n\tv_fmac_f32_dpp %0, %0, %1 " CTRL "\n\tv_mul_f32_dpp %1, %1, %1 " CTRL "\n\ts_nop 1"            \
        : "+v"(mb[0]), "+v"(ma))
#define PB_SCAN_STEP3(CTRL)                                                                                          \
    asm("s_nop 1\n\tv_fmac_f32_dpp %0, %0, %3 " CTRL "\n\tv_fmac_f32_dpp %1, %1, %3 " CTRL                          \
        "\n\tv_fmac_f32_dpp %2, %2, %3 " CTRL "\n\tv_mul_f32_dpp %3, %3, %3 " CTRL                                  \
        : "+v"(mb[0]), "+v"(mb[1]), "+v"(mb[2]), "+v"(ma))
template <int C> __device__ __forceinline__ void scan_affine(float &ma, float (&mb)[C]);
template <> __device__ __forceinline__ void scan_affine<1>(float &ma, float (&mb)[1]) {
    PB_SCAN_STEP1(PB_DPP_SHR1); PB_SCAN_STEP1(PB_DPP_SHR2); PB_SCAN_STEP1(PB_DPP_SHR4); PB_SCAN_STEP1(PB_DPP_SHR8);
    PB_SCAN_STEP1(PB_DPP_BC15); PB_SCAN_STEP1(PB_DPP_BC31);
}
template <> __device__ __forceinline__ void scan_affine<3>(float &ma, float (&mb)[3]) {
    PB_SCAN_STEP3(PB_DPP_SHR1); PB_SCAN_STEP3(PB_DPP_SHR2); PB_SCAN_STEP3(PB_DPP_SHR4); PB_SCAN_STEP3(PB_DPP_SHR8);
    PB_SCAN_STEP3(PB_DPP_BC15); PB_SCAN_STEP3(PB_DPP_BC31);
    asm("s_nop 1" : "+v"(mb[0]), "+v"(mb[1]), "+v"(mb[2]), "+v"(ma));
}

template <typename TJ, typename TIN, int C>
__global__ __launch_bounds__(NT) void dt_rows_fused_kernel(const TJ *J, const TIN *in, float *F, int H, int W, float ratio,
                                                           float log_a, long rows_total) {
    const int lane = threadIdx.x & 63;
    const long row_id = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);   // over B*H: one wave = one row, all channels
    if (row_id >= rows_total) return;
    const long b = row_id / H;
    const int r = (int)(row_id - b * H);
    const long HW = (long)H * W, off = (b * C * H + r) * (long)W;
    const TJ *j = J + off;
    const TIN *x0 = in + off;
    float *f = F + off;
    // ---- left -> right
    float carry[C];
#pragma unroll
    for (int c = 0; c < C; ++c) carry[c] = 0.f;
    for (int base = 0; base < W; base += 64) {
        const int i = base + lane;
        float dx = 0.f, x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            x[c] = 0.f;
            if (i < W) {
                x[c] = pb_ld(x0 + c * HW + i);
                if (i > 0) dx += fabsf(pb_ld(j + c * HW + i) - pb_ld(j + c * HW + i - 1));
            }
        }
        float v = 1.f;
        if (i < W) v = expf((1.f + ratio * dx) * log_a);
        float ma = (i == 0 || i >= W) ? 0.f : v, mb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) mb[c] = (i == 0 || i >= W) ? x[c] : (1.f - v) * x[c];
        if (i >= W) {
            ma = 1.f;
#pragma unroll
            for (int c = 0; c < C; ++c) mb[c] = 0.f;
        }
        scan_affine<C>(ma, mb);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float y = fmaf(ma, carry[c], mb[c]);
            if (i < W) f[c * HW + i] = y;
            carry[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), base + 63 >= W ? (W - 1) - base : 63));
        }
    }
    __threadfence_block();                               // the right-to-left pass reads what other lanes have just written
    // ---- right -> left
    const int last_base = ((W - 1) / 64) * 64;
#pragma unroll
    for (int c = 0; c < C; ++c) carry[c] = 0.f;
    for (int base = last_base; base >= 0; base -= 64) {
        const int i = base + (63 - lane);                // lane 0 handles the right-most element of the chunk
        float dx = 0.f, x[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            x[c] = 0.f;
            if (i < W) x[c] = f[c * HW + i];
            if (i + 1 < W) dx += fabsf(pb_ld(j + c * HW + i + 1) - pb_ld(j + c * HW + i));
        }
        float v = 1.f;
        if (i + 1 < W) v = expf((1.f + ratio * dx) * log_a);
        float ma = (i >= W - 1) ? 0.f : v, mb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) mb[c] = (i >= W - 1) ? x[c] : (1.f - v) * x[c];
        if (i >= W) {
            ma = 1.f;
#pragma unroll
            for (int c = 0; c < C; ++c) mb[c] = 0.f;
        }
        scan_affine<C>(ma, mb);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float y = fmaf(ma, carry[c], mb[c]);
            if (i < W) f[c * HW + i] = y;
            carry[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), 63));  // element `base`, the left-most of this chunk
        }
    }
}

// ---- the row pass with the row in registers (round 5) -------------------------------------------------------------------
// A row of W <= 64 NCH samples of C channels is NCH x C values per lane: the wave reads its row ONCE (every load of the row in
// flight together), runs the left-to-right recurrence chunk by chunk, then the right-to-left one on the registers, and
// writes the row once -- where dt_rows_fused_kernel writes the intermediate row, reads it back and reads the joint image a
// second time (4.9 words per sample through HBM on 64 x 1080p against the 2 of one read and one write:
// profiles/r04_bench_cfg3_traffic.json).  Only for J == in (the pipeline's call, domain_transform.py:45-47 with joint=None):
// the neighbour differences |J[i] - J[i-1]| then come from the registers too (lane - 1, or lane 63 of the previous chunk).
// The recurrences, their operands and the order in which scan_affine composes them are those of dt_rows_fused_kernel: the
// right-to-left pass runs on lane-reversed values (lane l <-> sample base + 63 - l), exactly as that kernel lays them out --
// bit-identical results (tests/test_gpu_round5_forms.py::test_dt_rows_register_form).
template <typename TIN, int C, int NCH>
__global__ __launch_bounds__(NT, NCH == 32 ? 3 : 1) void dt_rows_reg_kernel(const TIN *in, float *F, int H, int W, float ratio, float log_a, long rows_total) {   // (32 chunks: three waves per SIMD -- 168 registers)
    const int lane = threadIdx.x & 63;
    const long row_id = (long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);   // over B*H: one wave = one row, all channels
    if (row_id >= rows_total) return;
    const long b = row_id / H;
    const int r = (int)(row_id - b * H);
    const long HW = (long)H * W, off = (b * C * H + r) * (long)W;
    const TIN *x0 = in + off;
    float *f = F + off;
    const int nch = (W + 63) >> 6;
    float x[NCH][C], v[NCH];
    // (addresses clamped into the row, not loads under a lane mask: a masked fp16 load is followed by its conversion inside
    //  the masked block and by a wait for it, which put the 96 loads of a 1080p row one after the other -- 1.55 ms on
    //  64 x 1080p fp16 against 0.77 ms for the same row in fp32.
    //  Only the row's last chunk is ragged: every other chunk's address is a uniform base plus the lane -- one offset
    //  register for all of them; a clamp per chunk cost 35 registers and the third wave per SIMD.)
    TIN raw[NCH][C];
    const int klast = nch - 1, lane_last = min(lane, W - 1 - 64 * klast);
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const TIN *xk = x0 + 64 * min(k, klast) + (k < klast ? lane : lane_last);      // (chunks past the row: the last chunk again)
#pragma unroll
        for (int c = 0; c < C; ++c) raw[k][c] = xk[c * HW];
    }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        const int i = 64 * k + lane;
#pragma unroll
        for (int c = 0; c < C; ++c) x[k][c] = (i < W) ? pb_ld(&raw[k][c]) : 0.f;
    }
    // ---- left -> right
    float carry[C], last[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { carry[c] = 0.f; last[c] = 0.f; }
#pragma unroll
    for (int k = 0; k < NCH; ++k) {
        if (k < nch) {
            const int base = 64 * k, i = base + lane;
            float dx = 0.f;
#pragma unroll
            for (int c = 0; c < C; ++c) {
                // sample i - 1: the lane before (wave_shr:1), lane 0 keeps the operand's old value -- lane 63 of the previous chunk
                const float left = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(last[c]), __float_as_int(x[k][c]), 0x138, 0xf, 0xf, false));
                last[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[k][c]), 63));
                if (i < W && i > 0) dx += fabsf(x[k][c] - left);
            }
            float vv = 1.f;
            if (i < W) vv = expf((1.f + ratio * dx) * log_a);
            v[k] = vv;
            float ma = (i == 0 || i >= W) ? 0.f : vv, mb[C];
#pragma unroll
            for (int c = 0; c < C; ++c) mb[c] = (i == 0 || i >= W) ? x[k][c] : (1.f - vv) * x[k][c];
            if (i >= W) {
                ma = 1.f;
#pragma unroll
                for (int c = 0; c < C; ++c) mb[c] = 0.f;
            }
            scan_affine<C>(ma, mb);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float y = fmaf(ma, carry[c], mb[c]);
                x[k][c] = y;
                carry[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), base + 63 >= W ? (W - 1) - base : 63));
            }
        } else {
            v[k] = 1.f;
        }
    }
    // ---- right -> left, on lane-reversed values: lane l <-> sample i = base + 63 - l; its weight is V[i + 1]
#pragma unroll
    for (int c = 0; c < C; ++c) carry[c] = 0.f;
    float vnext0 = 1.f;                                                  // V[first sample of the chunk to the right]
#pragma unroll
    for (int k = NCH - 1; k >= 0; --k) {
        if (k < nch) {
            const int base = 64 * k, i = base + (63 - lane);
            float xr[C];
#pragma unroll
            for (int c = 0; c < C; ++c) xr[c] = __shfl(x[k][c], 63 - lane);
            float vr = __shfl(v[k], (64 - lane) & 63);                       // V[base + 64 - l], l >= 1
            if (lane == 0) vr = vnext0;
            vnext0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[k]), 0));
            const float vv = (i + 1 < W) ? vr : 1.f;
            float ma = (i >= W - 1) ? 0.f : vv, mb[C];
#pragma unroll
            for (int c = 0; c < C; ++c) mb[c] = (i >= W - 1) ? xr[c] : (1.f - vv) * xr[c];
            if (i >= W) {
                ma = 1.f;
#pragma unroll
                for (int c = 0; c < C; ++c) mb[c] = 0.f;
            }
            scan_affine<C>(ma, mb);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float y = fmaf(ma, carry[c], mb[c]);
                if (i < W) f[c * HW + i] = y;
                carry[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), 63));  // sample `base`, the left-most of this chunk
            }
        }
    }
}

// ---- the register row pass, a row over the four waves of a workgroup (round 6) ---------------------------------------------------
// One wave per row spends ~0.5 us per 64-sample chunk in the two scans whatever feeds it: a lone 4K image's 2160 rows are 2160
// waves of 60 chunks each -- 162 us for 200 MB.  The scans of a row's chunks do not depend on one another; only the carry does,
// and that is one multiply-add per chunk and channel.  Here wave w of the workgroup holds chunks w CPW .. w CPW + CPW - 1 of the
// row, scans them, leaves the map of each chunk's last sample in LDS, and every wave then walks the carries of the chunks before
// its own: fmaf(a, carry, b) on the last sample's map is what lane 63's y = fmaf(ma, carry, mb) was in dt_rows_reg_kernel, so
// the carries, and with them every sample, are the same bits.  The right-to-left pass likewise (chunk k's first weight comes from
// chunk k + 1: through LDS at the waves' seams).  Rows of up to 256 CPW samples: CPW = 32 takes an 8K row.
template <typename TIN, int C, int CPW>
__global__ __launch_bounds__(NT) void dt_rows_regw_kernel(const TIN *in, float *F, int H, int W, float ratio, float log_a) {
    constexpr int WPR = NT / 64, NCH = WPR * CPW;
    __shared__ float tail[2][NCH][C + 1];              // [pass][chunk]: the map (a, b[c]) of the chunk's last sample
    __shared__ float vfirst[NCH + 1];                  // the weight of each chunk's first sample
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, k0 = wv * CPW;
    const long row_id = blockIdx.x;                    // over B*H: one workgroup = one row, all channels
    const long b = row_id / H;
    const int r = (int)(row_id - b * H);
    const long HW = (long)H * W, off = (b * C * H + r) * (long)W;
    const TIN *x0 = in + off;
    float *f = F + off;
    const int nch = (W + 63) >> 6;
    float x[CPW][C], v[CPW], ma[CPW];
    TIN raw[CPW][C], rawl[C];
    const int klast = nch - 1, lane_last = min(lane, W - 1 - 64 * klast);
#pragma unroll
    for (int q = 0; q < CPW; ++q) {
        const int k = k0 + q;
        const TIN *xk = x0 + 64 * min(k, klast) + (k < klast ? lane : lane_last);      // (chunks past the row: the last chunk again)
#pragma unroll
        for (int c = 0; c < C; ++c) raw[q][c] = xk[c * HW];
    }
#pragma unroll
    for (int c = 0; c < C; ++c) rawl[c] = x0[c * HW + min(max(64 * k0 - 1, 0), W - 1)];   // the sample left of this wave's first
#pragma unroll
    for (int q = 0; q < CPW; ++q) {
        const int i = 64 * (k0 + q) + lane;
#pragma unroll
        for (int c = 0; c < C; ++c) x[q][c] = (i < W) ? pb_ld(&raw[q][c]) : 0.f;
    }
    // ---- left -> right: the scans
    float last[C];
#pragma unroll
    for (int c = 0; c < C; ++c) last[c] = k0 > 0 ? pb_ld(&rawl[c]) : 0.f;
#pragma unroll
    for (int q = 0; q < CPW; ++q) {
        const int k = k0 + q, base = 64 * k, i = base + lane;
        float dx = 0.f;
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float left = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(last[c]), __float_as_int(x[q][c]), 0x138, 0xf, 0xf, false));
            last[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[q][c]), 63));
            if (i < W && i > 0) dx += fabsf(x[q][c] - left);
        }
        float vv = 1.f;
        if (i < W) vv = expf((1.f + ratio * dx) * log_a);
        v[q] = vv;
        float a = (i == 0 || i >= W) ? 0.f : vv, mb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) mb[c] = (i == 0 || i >= W) ? x[q][c] : (1.f - vv) * x[q][c];
        if (i >= W) {
            a = 1.f;
#pragma unroll
            for (int c = 0; c < C; ++c) mb[c] = 0.f;
        }
        scan_affine<C>(a, mb);
        ma[q] = a;
#pragma unroll
        for (int c = 0; c < C; ++c) x[q][c] = mb[c];
        if (lane == (base + 63 >= W ? max((W - 1) - base, 0) : 63)) {
            tail[0][k][0] = a;
#pragma unroll
            for (int c = 0; c < C; ++c) tail[0][k][1 + c] = mb[c];
        }
        if (lane == 0) vfirst[k] = vv;
    }
    if (threadIdx.x == 0) vfirst[NCH] = 1.f;
    __syncthreads();
    // ... the carries of the chunks before this wave's, then its own samples
    float carry[C];
#pragma unroll
    for (int c = 0; c < C; ++c) carry[c] = 0.f;
    for (int k = 0; k < min(k0, nch); ++k) {
#pragma unroll
        for (int c = 0; c < C; ++c) carry[c] = fmaf(tail[0][k][0], carry[c], tail[0][k][1 + c]);
    }
#pragma unroll
    for (int q = 0; q < CPW; ++q) {
        const int base = 64 * (k0 + q);
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const float y = fmaf(ma[q], carry[c], x[q][c]);
            x[q][c] = y;
            carry[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), base + 63 >= W ? max((W - 1) - base, 0) : 63));
        }
    }
    // ---- right -> left, on lane-reversed values: lane l <-> sample i = base + 63 - l; its weight is V[i + 1]
#pragma unroll
    for (int q = CPW - 1; q >= 0; --q) {
        const int k = k0 + q, base = 64 * k, i = base + (63 - lane);
        float xr[C];
#pragma unroll
        for (int c = 0; c < C; ++c) xr[c] = __shfl(x[q][c], 63 - lane);
        float vr = __shfl(v[q], (64 - lane) & 63);                           // V[base + 64 - l], l >= 1
        const float vnext0 = q + 1 < CPW ? __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v[q + 1 < CPW ? q + 1 : q]), 0)) : vfirst[k + 1];
        if (lane == 0) vr = k + 1 < nch ? vnext0 : 1.f;
        const float vv = (i + 1 < W) ? vr : 1.f;
        float a = (i >= W - 1) ? 0.f : vv, mb[C];
#pragma unroll
        for (int c = 0; c < C; ++c) mb[c] = (i >= W - 1) ? xr[c] : (1.f - vv) * xr[c];
        if (i >= W) {
            a = 1.f;
#pragma unroll
            for (int c = 0; c < C; ++c) mb[c] = 0.f;
        }
        scan_affine<C>(a, mb);
        ma[q] = a;
#pragma unroll
        for (int c = 0; c < C; ++c) x[q][c] = mb[c];
        if (lane == 63) {
            tail[1][k][0] = a;
#pragma unroll
            for (int c = 0; c < C; ++c) tail[1][k][1 + c] = mb[c];
        }
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < C; ++c) carry[c] = 0.f;
    for (int k = nch - 1; k >= k0 + CPW; --k) {
#pragma unroll
        for (int c = 0; c < C; ++c) carry[c] = fmaf(tail[1][k][0], carry[c], tail[1][k][1 + c]);
    }
#pragma unroll
    for (int q = CPW - 1; q >= 0; --q) {
        const int k = k0 + q, i = 64 * k + (63 - lane);
        if (k < nch) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float y = fmaf(ma[q], carry[c], x[q][c]);
                if (i < W) f[c * HW + i] = y;
                carry[c] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(y), 63));  // sample `base`, the left-most of this chunk
            }
        }
    }
}

template <typename TJ, int C>
__global__ __launch_bounds__(NT) void dt_cols_fused_kernel(const TJ *__restrict__ J, float *__restrict__ F, int H, int W,
                                                           float ratio, float log_a, long cols_total) {
    const long id = (long)blockIdx.x * NT + threadIdx.x;   // over B*W: one thread = one column, all channels
    if (id >= cols_total) return;
    const long b = id / W;
    const int col = (int)(id - b * W);
    const long HW = (long)H * W;
    float *f = F + b * C * HW + col;
    const TJ *j = J + b * C * HW + col;
    float prev[C], pj[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { prev[c] = f[c * HW]; pj[c] = pb_ld(j + c * HW); }
    for (int r0 = 1; r0 < H; r0 += DT_UF) {
        float xs[DT_UF][C], js[DT_UF][C];
#pragma unroll
        for (int u = 0; u < DT_UF; ++u) {
            const int r = min(r0 + u, H - 1);
#pragma unroll
            for (int c = 0; c < C; ++c) { xs[u][c] = f[c * HW + (long)r * W]; js[u][c] = pb_ld(j + c * HW + (long)r * W); }
        }
#pragma unroll
        for (int u = 0; u < DT_UF; ++u) {
            if (r0 + u < H) {
                float dy = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) { dy += fabsf(js[u][c] - pj[c]); pj[c] = js[u][c]; }
                const float v = expf((1.f + ratio * dy) * log_a);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    prev[c] = xs[u][c] + v * (prev[c] - xs[u][c]);
                    f[c * HW + (long)(r0 + u) * W] = prev[c];
                }
            }
        }
    }
    // pj = J[H-1], prev = F[H-1]
    for (int r0 = H - 2; r0 >= 0; r0 -= DT_UF) {
        float xs[DT_UF][C], js[DT_UF][C];
#pragma unroll
        for (int u = 0; u < DT_UF; ++u) {
            const int r = max(r0 - u, 0);
#pragma unroll
            for (int c = 0; c < C; ++c) { xs[u][c] = f[c * HW + (long)r * W]; js[u][c] = pb_ld(j + c * HW + (long)r * W); }
        }
#pragma unroll
        for (int u = 0; u < DT_UF; ++u) {
            if (r0 - u >= 0) {
                float dy = 0.f;                                      // dom of row r+1: |J[r+1] - J[r]|
#pragma unroll
                for (int c = 0; c < C; ++c) { dy += fabsf(pj[c] - js[u][c]); pj[c] = js[u][c]; }
                const float v = expf((1.f + ratio * dy) * log_a);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    prev[c] = xs[u][c] + v * (prev[c] - xs[u][c]);
                    f[c * HW + (long)(r0 - u) * W] = prev[c];
                }
            }
        }
    }
}

// ---- the column pass in strips (round 5) -----------------------------------------------------------------------------------
// dt_cols_fused_kernel moves 6 words per sample: the down sweep reads F and J and writes F, the up sweep reads both again
// and writes F again.  The up sweep at row r needs the down sweep's value of row r and the up sweep's of row r + 1, so the
// down sweep has to reach the bottom first -- but not to WRITE anything on the way except what lets its values be formed
// again: one carry per strip of S rows (dt_cols_down_kernel: 2 words per sample read, 1 / S written).  dt_cols_up_kernel
// then takes the strips bottom-up: the strip's rows of F and J into registers, the down sweep's values of the strip formed
// again from the carry above it -- the same operations on the same operands in the same order: the same bits --, the up
// sweep over them, one store per sample: 3 words.  5 words instead of 6, and one exponential per sample and column instead
// of two (the up sweep's weight of row r + 1 is the down sweep's, domain_transform.py:62-85: |J[r+1] - J[r]| either way).
// Bit-identical to dt_cols_fused_kernel (tests/test_gpu_round5_forms.py).
// Round 6: where J is C fp32 channels the up sweep reads C words per pixel only to form one weight again, so the down sweep
// stores the weight it has (WV: one word per pixel, 1 / C per sample) and dt_cols_upw_kernel reads that instead of J: 2 / C words
// against 1, 4.67 + 2 / S per sample at C = 3 -- and, no J in its registers, strips of 32 rows.  The weight is the value the
// down sweep used, the operations on it are the same: the same bits again.  (fp16 J, or one channel: J costs no more than the
// weight would -- those keep dt_cols_up_kernel.)
template <int C> __device__ __forceinline__ float dt_weight(const float (&jr)[C], const float (&jp)[C], float ratio, float log_a) {
    float dy = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) dy += fabsf(jr[c] - jp[c]);
    return expf((1.f + ratio * dy) * log_a);
}
template <typename TJ, int C, int S, bool WV>
__global__ __launch_bounds__(NT) void dt_cols_down_kernel(const TJ *__restrict__ J, const float *__restrict__ F, float *__restrict__ carry,
                                                          float *__restrict__ wts, int H, int W, float ratio, float log_a, long cols_total) {
    const long id = (long)blockIdx.x * NT + threadIdx.x;   // over B*W: one thread = one column, all channels
    if (id >= cols_total) return;
    const long b = id / W;
    const int col = (int)(id - b * W);
    const long HW = (long)H * W;
    const float *f = F + b * C * HW + col;
    const TJ *j = J + b * C * HW + col;
    float *wt = WV ? wts + b * HW + col : nullptr;         // wts[b][r][col] = the weight of row r (rows 1 .. H - 1)
    float prev[C], pj[C];
#pragma unroll
    for (int c = 0; c < C; ++c) { prev[c] = f[c * HW]; pj[c] = pb_ld(j + c * HW); }
    // carry[s][c][id] = the down sweep's value of the last row of strip s (rows S s .. S s + S - 1), for every strip but the last
    for (int r0 = 1; r0 < H; r0 += DT_UF) {
        float xs[DT_UF][C], js[DT_UF][C];
#pragma unroll
        for (int u = 0; u < DT_UF; ++u) {
            const int r = min(r0 + u, H - 1);
#pragma unroll
            for (int c = 0; c < C; ++c) { xs[u][c] = f[c * HW + (long)r * W]; js[u][c] = pb_ld(j + c * HW + (long)r * W); }
        }
#pragma unroll
        for (int u = 0; u < DT_UF; ++u) {
            const int r = r0 + u;
            if (r < H) {
                const float v = dt_weight<C>(js[u], pj, ratio, log_a);
                if constexpr (WV) wt[(long)r * W] = v;
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    pj[c] = js[u][c];
                    prev[c] = xs[u][c] + v * (prev[c] - xs[u][c]);
                }
                if ((r & (S - 1)) == S - 1 && r + 1 < H) {
#pragma unroll
                    for (int c = 0; c < C; ++c) carry[((long)(r / S) * C + c) * cols_total + id] = prev[c];
                }
            }
        }
    }
}
// the up sweep over strips of S rows with the down sweep's weights read back (see above); F only, no J
template <int C, int S>
__global__ __launch_bounds__(NT) void dt_cols_upw_kernel(float *__restrict__ F, const float *__restrict__ carry, const float *__restrict__ wts,
                                                         int H, int W, long cols_total) {
    const long id = (long)blockIdx.x * NT + threadIdx.x;
    if (id >= cols_total) return;
    const long b = id / W;
    const int col = (int)(id - b * W);
    const long HW = (long)H * W;
    float *f = F + b * C * HW + col;
    const float *wt = wts + b * HW + col;
    const int nstrips = (H + S - 1) / S;
    float fnext[C], vnext = 0.f;
#pragma unroll
    for (int c = 0; c < C; ++c) fnext[c] = 0.f;
    for (int s = nstrips - 1; s >= 0; --s) {
        const int a = s * S;
        float xs[S][C], prev[C], v[S];
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int r = min(a + u, H - 1);
#pragma unroll
            for (int c = 0; c < C; ++c) xs[u][c] = f[c * HW + (long)r * W];
            v[u] = wt[(long)max(r, 1) * W];                  // (row 0 has no weight: its slot is never written, never used)
        }
        if (s > 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) prev[c] = carry[((long)(s - 1) * C + c) * cols_total + id];
        }
#pragma unroll
        for (int u = 0; u < S; ++u) {
            const int r = a + u;
            if (r == 0) {
#pragma unroll
                for (int c = 0; c < C; ++c) prev[c] = xs[u][c];
            } else if (r < H) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    prev[c] = xs[u][c] + v[u] * (prev[c] - xs[u][c]);
                    xs[u][c] = prev[c];
                }
            }
        }
#pragma unroll
        for (int u = S - 1; u >= 0; --u) {
            const int r = a + u;
            if (r < H) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if (r < H - 1) fnext[c] = xs[u][c] + vnext * (fnext[c] - xs[u][c]);
                    else fnext[c] = xs[u][c];
                    f[c * HW + (long)r * W] = fnext[c];
                }
                vnext = v[u];
            }
        }
    }
}
template <typename TJ, int C>
__global__ __launch_bounds__(NT) void dt_cols_up_kernel(const TJ *__restrict__ J, float *__restrict__ F, const float *__restrict__ carry,
                                                        int H, int W, float ratio, float log_a, long cols_total) {
    const long id = (long)blockIdx.x * NT + threadIdx.x;
    if (id >= cols_total) return;
    const long b = id / W;
    const int col = (int)(id - b * W);
    const long HW = (long)H * W;
    float *f = F + b * C * HW + col;
    const TJ *j = J + b * C * HW + col;
    const int nstrips = (H + DT_STRIP - 1) / DT_STRIP;
    float fnext[C], vnext = 0.f;                            // the up sweep's value of the row below the strip, and that row's weight
#pragma unroll
    for (int c = 0; c < C; ++c) fnext[c] = 0.f;
    for (int s = nstrips - 1; s >= 0; --s) {
        const int a = s * DT_STRIP;
        float xs[DT_STRIP][C], js[DT_STRIP][C], pj[C], prev[C], v[DT_STRIP];
        // (rows past the plane's end: the last row again -- loaded, never used)
#pragma unroll
        for (int u = 0; u < DT_STRIP; ++u) {
            const int r = min(a + u, H - 1);
#pragma unroll
            for (int c = 0; c < C; ++c) { xs[u][c] = f[c * HW + (long)r * W]; js[u][c] = pb_ld(j + c * HW + (long)r * W); }
        }
        if (s > 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) { prev[c] = carry[((long)(s - 1) * C + c) * cols_total + id]; pj[c] = pb_ld(j + c * HW + (long)(a - 1) * W); }
        }
        // the down sweep's values of the strip, formed again (row 0 keeps its value: domain_transform.py:62-72)
#pragma unroll
        for (int u = 0; u < DT_STRIP; ++u) {
            const int r = a + u;
            if (r == 0) {
                v[u] = 0.f;
#pragma unroll
                for (int c = 0; c < C; ++c) { prev[c] = xs[u][c]; pj[c] = js[u][c]; }
            } else if (r < H) {
                v[u] = dt_weight<C>(js[u], pj, ratio, log_a);
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    pj[c] = js[u][c];
                    prev[c] = xs[u][c] + v[u] * (prev[c] - xs[u][c]);
                    xs[u][c] = prev[c];
                }
            } else {
                v[u] = 0.f;
            }
        }
        // the up sweep over the strip (the last row of the plane keeps the down sweep's value)
#pragma unroll
        for (int u = DT_STRIP - 1; u >= 0; --u) {
            const int r = a + u;
            if (r < H) {
#pragma unroll
                for (int c = 0; c < C; ++c) {
                    if (r < H - 1) fnext[c] = xs[u][c] + vnext * (fnext[c] - xs[u][c]);
                    else fnext[c] = xs[u][c];
                    f[c * HW + (long)r * W] = fnext[c];
                }
                vnext = v[u];
            }
        }
    }
}

// ---- the column pass of few columns (round 6) -------------------------------------------------------------------------------
// One thread per column is B W threads: a single 1080p image is 30 waves, each allowed 63 requests in flight -- 16 KB -- against
// a latency of ~1.3 us: 0.37 TB/s however the loop is written (measured: down + up sweep 176 + 206 us at B = 1 and at B = 4
// alike, where the planes' 250 MB would take 50 us).  Here a workgroup owns CG adjacent columns (16 of three channels, 64 of one:
// 64 bytes per row and channel) and ALL its lanes fetch: blocks of DTC_R3 (one channel: DTC_R1) rows of F and J straight into LDS (16 bytes
// per lane, waves 1 - 3; the next block in flight under the present one's recurrence), all lanes form the block's weights, and wave 0
// -- lane = (channel, column) -- runs the recurrence down the block out of LDS; carries per block; then the blocks bottom-up: the
// down sweep's values of the block formed again from the carry above it, the up sweep over them, the rows stored 16 bytes per lane
// one block late, under the next block's recurrence.  Rows 0 and H - 1 need no case of their own: their weights are 0 and
// x + 0 (p - x) = x (a sample that is -0 comes out as +0: the only difference in bits there can be).  The same operations on the same operands in the same order as dt_cols_fused_kernel: the same bits
// (tests/test_gpu_round5_forms.py::test_dt_columns_in_strips).  5 words per sample like the strips; the launch is taken where the
// per-column form cannot fill the chip (dt_choice.h, choose_dt: cols_total up to DTC_MAX_COLS).
typedef __amdgpu_buffer_rsrc_t dt_rsrc;
typedef __attribute__((address_space(3))) void dt_lds_void;
__device__ __forceinline__ void dtc_dma16(dt_rsrc r, void *dst, unsigned voffset) {
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Wold-style-cast"
    __builtin_amdgcn_raw_ptr_buffer_load_lds(r, (dt_lds_void *)dst, 16, (int)voffset, 0, 0, 0);
#pragma clang diagnostic pop
}
template <typename TJ, int C, int R> struct DtCoop {
    static constexpr int CG = dtc_cg(C), L = C * CG;
    static constexpr int FB = dtc_f_bytes(C, R);                                             // bytes of a block of F: whole KB
    static constexpr int JB = dtc_j_bytes((int)sizeof(TJ), C, R);                            // of J: the row above the block too
    static_assert(FB % 1024 == 0 && R % DTC_CH == 0, "a block of F is whole wave requests and whole chunks of the chain");
};
template <typename TJ, int C, int R>
__global__ __launch_bounds__(NT) void dt_cols_coop_kernel(const TJ *__restrict__ J, float *__restrict__ F, float *__restrict__ carry,
                                                          int H, int W, float ratio, float log_a, int groups) {
    using G = DtCoop<TJ, C, R>;
    constexpr int CG = G::CG, L = G::L, FB = G::FB, JB = G::JB, CH = DTC_CH;
    extern __shared__ __attribute__((aligned(16))) unsigned char dtc_smem[];
    unsigned char *smem = dtc_smem;
    float *vb = reinterpret_cast<float *>(smem + 2 * FB + 2 * JB);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x / groups, col0 = (blockIdx.x - b * groups) * CG;
    const long HW = (long)H * W;
    const int nb = (H + R - 1) / R;
    float *Fi = F + (long)b * C * HW;
    const dt_rsrc rF = __builtin_amdgcn_make_buffer_rsrc(Fi, 0, (int)(C * HW * 4), 0x00020000);
    const dt_rsrc rJ = __builtin_amdgcn_make_buffer_rsrc(const_cast<TJ *>(J + (long)b * C * HW), 0, (int)(C * HW * (long)sizeof(TJ)), 0x00020000);
    float *cw = carry + (long)blockIdx.x * nb * L;
    auto fbuf = [&](int k) { return reinterpret_cast<float *>(smem + (k & 1) * FB); };
    auto jbuf = [&](int k) { return reinterpret_cast<TJ *>(smem + 2 * FB + (k & 1) * JB); };
    // (waves 1 .. 3 fetch; wave 0 runs the recurrence and has no request of its own to wait for in the middle of it)
    auto request = [&](int k) {
        if (wave == 0) return;
        const int r0 = k * R;
        for (int i = wave - 1; i < FB / 1024; i += NT / 64 - 1) {
            const int e = (i * 1024 + lane * 16) / 4;
            const int u = e / L, idx = e - u * L, c = idx / CG, col = idx - c * CG;
            const bool ok = r0 + u < H && col0 + col < W;
            dtc_dma16(rF, reinterpret_cast<unsigned char *>(fbuf(k)) + i * 1024, ok ? (unsigned)((c * HW + (long)(r0 + u) * W + col0 + col) * 4) : DTC_NO_ACCESS);
        }
        for (int i = wave - 1; i < JB / 1024; i += NT / 64 - 1) {
            const int e = (i * 1024 + lane * 16) / (int)sizeof(TJ);
            const int u = e / L, idx = e - u * L, c = idx / CG, col = idx - c * CG, row = r0 - 1 + u;
            const bool ok = u <= R && row >= 0 && row < H && col0 + col < W;
            dtc_dma16(rJ, reinterpret_cast<unsigned char *>(jbuf(k)) + i * 1024, ok ? (unsigned)((c * HW + (long)row * W + col0 + col) * (long)sizeof(TJ)) : DTC_NO_ACCESS);
        }
    };
    // the weights of the block's rows (row 0 of the plane has none)
    auto weights = [&](int k) {
        const TJ *jb = jbuf(k);
        for (int p = tid; p < R * CG; p += NT) {
            const int u = p / CG, col = p - u * CG, r = k * R + u;
            float jr[C], jp[C];
#pragma unroll
            for (int c = 0; c < C; ++c) { jr[c] = pb_ld(jb + (u + 1) * L + c * CG + col); jp[c] = pb_ld(jb + u * L + c * CG + col); }
            vb[p] = r >= 1 && r < H ? dt_weight<C>(jr, jp, ratio, log_a) : 0.f;
        }
    };
    // Order of a block's steps: the requests go out AFTER the weights (the compiler waits for every outstanding request before an
    // LDS read that follows one: behind the weights a request flies under the recurrence instead of being waited for), and the
    // up sweep's rows are stored one step late, by the fetching waves, while wave 0 is in the next block's recurrence.
    // Rows 0 and H - 1 need no case of their own: the weight of row 0, and of rows past the end, is 0 (weights()) and
    // x + 0 (p - x) = x -- the row keeps its value --; rows past the end hold the zeros the requests returned.
    const int ccol = lane % CG;
    auto store_rows = [&](int k) {
        const float *fb = fbuf(k);
        for (int i = wave - 1; i < FB / 1024; i += NT / 64 - 1) {    // (a wave stores the KB it fetches: its next request into them follows its own reads)
            const int e = i * 256 + lane * 4, u = e / L, idx = e - u * L, c = idx / CG, col = idx - c * CG, r = k * R + u;
            if (r < H && col0 + col < W) *reinterpret_cast<float4 *>(Fi + c * HW + (long)r * W + col0 + col) = *reinterpret_cast<const float4 *>(fb + e);
        }
    };
    float prev = 0.f;
    request(0);
    for (int k = 0; k < nb; ++k) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        weights(k);
        __syncthreads();
        if (k + 1 < nb) {                                        // (the last block's down values are formed by the up sweep below)
            if (wave > 0) {
                request(k + 1);
            } else if (lane < L) {
                const float *fb = fbuf(k);
                for (int q = 0; q < R; q += CH) {
                    float x[CH], v[CH];
#pragma unroll
                    for (int u = 0; u < CH; ++u) { x[u] = fb[(q + u) * L + lane]; v[u] = vb[(q + u) * CG + ccol]; }
#pragma unroll
                    for (int u = 0; u < CH; ++u) prev = x[u] + v[u] * (prev - x[u]);
                }
                cw[k * L + lane] = prev;
            }
        }
    }
    float fnext = 0.f, vnext = 0.f;
    for (int k = nb - 1; k >= 0; --k) {
        if (k != nb - 1) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            weights(k);
            __syncthreads();
        }
        if (wave > 0) {
            if (k + 1 < nb) store_rows(k + 1);
            if (k > 0) request(k - 1);                           // (into the buffer of block k + 1, read out just above)
        } else if (lane < L) {
            float *fb = fbuf(k);
            // the down sweep's values of the block, into LDS in place, ...
            prev = k > 0 ? cw[(k - 1) * L + lane] : 0.f;
            for (int q = 0; q < R; q += CH) {
                float x[CH], v[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) { x[u] = fb[(q + u) * L + lane]; v[u] = vb[(q + u) * CG + ccol]; }
#pragma unroll
                for (int u = 0; u < CH; ++u) {
                    prev = x[u] + v[u] * (prev - x[u]);
                    fb[(q + u) * L + lane] = prev;
                }
            }
            // ... and the up sweep over them
            for (int q = R - CH; q >= 0; q -= CH) {
                float x[CH], v[CH];
#pragma unroll
                for (int u = 0; u < CH; ++u) { x[u] = fb[(q + u) * L + lane]; v[u] = vb[(q + u) * CG + ccol]; }
#pragma unroll
                for (int u = CH - 1; u >= 0; --u) {
                    fnext = x[u] + vnext * (fnext - x[u]);
                    fb[(q + u) * L + lane] = fnext;
                    vnext = v[u];
                }
            }
        }
    }
    __syncthreads();
    if (wave > 0) store_rows(0);
}

// One or three channels: what choose_dt chose for the call -- asked once, its scratch requested once, the cooperative kernel's
// LDS limit raised once -- then per iteration a row pass (the chosen form in the first, in place through global memory
// afterwards) and a column pass.
template <typename T, int C>
int dt_filter_fused(pb_ctx *ctx, const T *in, const T *J, float *out, int B, int H, int W, float ratio, int N, float sigma_s) {
    const long rows_total = (long)B * H, cols_total = (long)B * W;
    const bool aligned16 = (reinterpret_cast<uintptr_t>(J) | reinterpret_cast<uintptr_t>(out)) % 16 == 0;
    const DtChoice ch = choose_dt(ctx->dt, (int)sizeof(T), C, B, H, W, J == in, aligned16);
    float *carry = nullptr, *wts = nullptr;
    if (ch.carry && !(carry = static_cast<float *>(pb_scratch(ctx, "dt.carry", sizeof(float) * (size_t)ch.carry)))) return PB_ERR_NOMEM;
    if (ch.weights && !(wts = static_cast<float *>(pb_scratch(ctx, "dt.weights", sizeof(float) * (size_t)ch.weights)))) return PB_ERR_NOMEM;
    constexpr int R = dtc_rows(C), CG = dtc_cg(C);
    const auto coop = dt_cols_coop_kernel<T, C, R>;
    if (ch.lds > 48 * 1024) PB_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(coop), hipFuncAttributeMaxDynamicSharedMemorySize, ch.lds));
    const dim3 rgrid((unsigned)((rows_total + 3) / 4)), wgrid((unsigned)rows_total), cgrid((unsigned)((cols_total + NT - 1) / NT));
    for (int i = 0; i < N; ++i) {
        const float log_a = dt_log_a(sigma_s, i, N);
#define PB_DT_WAVE(NCH) hipLaunchKernelGGL((dt_rows_reg_kernel<T, C, NCH>), rgrid, dim3(NT), 0, ctx->stream, in, out, H, W, ratio, log_a, rows_total)
#define PB_DT_WG(CPW) hipLaunchKernelGGL((dt_rows_regw_kernel<T, C, CPW>), wgrid, dim3(NT), 0, ctx->stream, in, out, H, W, ratio, log_a)
        if (i > 0)
            hipLaunchKernelGGL((dt_rows_fused_kernel<T, float, C>), rgrid, dim3(NT), 0, ctx->stream, J, out, out, H, W, ratio, log_a, rows_total);
        else switch (ch.rows * 100 + ch.chunks) {
            case PB_DT_ROWS_WAVE * 100 + 16: PB_DT_WAVE(16); break;
            case PB_DT_ROWS_WAVE * 100 + 32: PB_DT_WAVE(32); break;
            case PB_DT_ROWS_WAVE * 100 + 64: PB_DT_WAVE(64); break;              // (a 4K row: one wave per SIMD, ~300 registers)
            case PB_DT_ROWS_WORKGROUP * 100 + 4: PB_DT_WG(4); break;
            case PB_DT_ROWS_WORKGROUP * 100 + 8: PB_DT_WG(8); break;
            case PB_DT_ROWS_WORKGROUP * 100 + 16: PB_DT_WG(16); break;
            case PB_DT_ROWS_WORKGROUP * 100 + 32: PB_DT_WG(32); break;
            case PB_DT_ROWS_MEMORY * 100:
                hipLaunchKernelGGL((dt_rows_fused_kernel<T, T, C>), rgrid, dim3(NT), 0, ctx->stream, J, in, out, H, W, ratio, log_a, rows_total);
                break;
            default: return pb_fail(ctx, PB_ERR_UNSUPPORTED, "dt: no row kernel of form %d with %d chunks", ch.rows, ch.chunks);
        }
#undef PB_DT_WAVE
#undef PB_DT_WG
        switch (ch.cols) {
            case PB_DT_COLS_COOPERATIVE: {
                const int groups = (W + CG - 1) / CG;
                hipLaunchKernelGGL(coop, dim3((unsigned)(B * groups)), dim3(NT), ch.lds, ctx->stream, J, out, carry, H, W, ratio, log_a, groups);
                break;
            }
            case PB_DT_COLS_STRIPS_WEIGHTS:
                if constexpr (C * sizeof(T) > 2 * sizeof(float)) {                   // (where the weights pay: dt_choice.h)
                    hipLaunchKernelGGL((dt_cols_down_kernel<T, C, DT_STRIP_W, true>), cgrid, dim3(NT), 0, ctx->stream, J, out, carry, wts, H, W, ratio, log_a, cols_total);
                    hipLaunchKernelGGL((dt_cols_upw_kernel<C, DT_STRIP_W>), cgrid, dim3(NT), 0, ctx->stream, out, carry, wts, H, W, cols_total);
                    break;
                }
                return pb_fail(ctx, PB_ERR_UNSUPPORTED, "dt: stored weights are built for three fp32 channels");
            case PB_DT_COLS_STRIPS:
                hipLaunchKernelGGL((dt_cols_down_kernel<T, C, DT_STRIP, false>), cgrid, dim3(NT), 0, ctx->stream, J, out, carry, wts, H, W, ratio, log_a, cols_total);
                hipLaunchKernelGGL((dt_cols_up_kernel<T, C>), cgrid, dim3(NT), 0, ctx->stream, J, out, carry, H, W, ratio, log_a, cols_total);
                break;
            default:
                hipLaunchKernelGGL((dt_cols_fused_kernel<T, C>), cgrid, dim3(NT), 0, ctx->stream, J, out, H, W, ratio, log_a, cols_total);
        }
        PB_LAUNCH_CHECK();
    }
    return PB_OK;
}

}  // namespace

// out (float32, B*C*H*W) = recursive_filter(in, joint)
int pb_dt_filter_impl(pb_ctx *ctx, const void *in, const void *joint, int dtype, float *out, int B, int C, int H, int W,
                      float sigma_s, float sigma_r, int num_iterations) {
    const long HW = (long)H * W, n = (long)B * C * HW;
    ProfScope prof(ctx, PB_PROF_PREFILTER);
    const void *J = joint ? joint : in;
    const float ratio = sigma_s / sigma_r;
    const int N = num_iterations;
    if (C == 1 || C == 3) {                       // gray and colour images: no domain planes (see dt_rows_fused_kernel)
        if (dtype == PB_F32) {
            const float *i32 = static_cast<const float *>(in), *j32 = static_cast<const float *>(J);
            return C == 3 ? dt_filter_fused<float, 3>(ctx, i32, j32, out, B, H, W, ratio, N, sigma_s)
                          : dt_filter_fused<float, 1>(ctx, i32, j32, out, B, H, W, ratio, N, sigma_s);
        }
        const __half *i16 = static_cast<const __half *>(in), *j16 = static_cast<const __half *>(J);
        return C == 3 ? dt_filter_fused<__half, 3>(ctx, i16, j16, out, B, H, W, ratio, N, sigma_s)
                      : dt_filter_fused<__half, 1>(ctx, i16, j16, out, B, H, W, ratio, N, sigma_s);
    }
    float *domx = static_cast<float *>(pb_scratch(ctx, "dt.domx", sizeof(float) * B * HW));
    float *domy = static_cast<float *>(pb_scratch(ctx, "dt.domy", sizeof(float) * B * HW));
    if (!domx || !domy) return PB_ERR_NOMEM;
    const dim3 dgrid((unsigned)std::min(std::max((HW + NT - 1) / NT, 1l), 2048l), B);
    if (dtype == PB_F32)
        hipLaunchKernelGGL(dt_domain_kernel<float>, dgrid, dim3(NT), 0, ctx->stream, static_cast<const float *>(J), domx, domy, C, H, W, ratio);
    else
        hipLaunchKernelGGL(dt_domain_kernel<__half>, dgrid, dim3(NT), 0, ctx->stream, static_cast<const __half *>(J), domx, domy, C, H, W, ratio);
    PB_LAUNCH_CHECK();
    if (const int rc = pb_convert_to_float(ctx, in, dtype, out, n)) return rc;
    const long rows_total = (long)B * C * H, cols_total = (long)B * C * W;
    for (int i = 0; i < N; ++i) {
        const float log_a = dt_log_a(sigma_s, i, N);
        hipLaunchKernelGGL(dt_rows_kernel, dim3((unsigned)((rows_total + 3) / 4)), dim3(NT), 0, ctx->stream, out, domx, C, H, W, log_a, rows_total);
        hipLaunchKernelGGL(dt_cols_kernel, dim3((unsigned)((cols_total + NT - 1) / NT)), dim3(NT), 0, ctx->stream, out, domy, C, H, W, log_a, cols_total);
        PB_LAUNCH_CHECK();
    }
    return PB_OK;
}

