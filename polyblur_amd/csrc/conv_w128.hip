// Tile-spectrum body of the one-pass polynomial on 128 x 128 windows: FOUR waves per window pair.
//
// Same pass, same operands, same result as the one-pass form of conv_wfft.hip (the whole polynomial a3 K^3 + a2 K^2 + a1 K + b
// of the deconvolution as ONE circular correlation per window -- the reference's own 'fft' form, deblurring.py:139-169 -- with
// the boundary models of filters.py:14-49 applied when the window is loaded): forward 2-D DFT, product with the polynomial's
// real spectrum (khat128_body, khat.h), inverse DFT, of which the samples at least (hx, hy) from the window's edge are
// kept (overlap-save); two horizontally adjacent real windows ride one complex transform, z = A + iB.
//
// Why a second window size.  The composite filter's halo is sqrt(3) times the kernel's: 20 x 24 samples for the headline's
// first estimate (sigma 2.1 / rho 1.3 at 66 degrees).  A 64 x 64 window keeps 24 x 16 of its 4096 samples then -- three
// Horner passes with the kernel's own 12-sample halo are cheaper --, a 128 x 128 window keeps 88 x 80 of 16384: 43 % in ONE
// pass against 39 % in each of three.
//
// Who does it.  A lane still holds 64 complex values, so a 128-point line is shared by the two halves of a wave: lanes l and
// l + 32 hold its two halves, exchange them with v_permlane32_swap for ONE radix-2 step (decimation in frequency forward,
// in time backward; twiddles are compile-time constants: the step's index is the register number) and run the 64-point
// transform of conv_wave_common.h on what they then hold.  A wave therefore owns 32 lines, a workgroup of four waves the 128:
//
//   load      wave w, lane (c, h): window column 32 w + c, rows 64 h .. 64 h + 63 in the registers
//   columns   radix-2 across the wave's halves, fft64 in registers: the lower lanes hold the even, the upper the odd frequencies
//   transpose through the workgroup's LDS matrix: lane (row slot, x half) holds 64 consecutive columns of one transformed row
//   rows      radix-2, fft64, x real spectrum, inverse fft64, inverse radix-2
//   transpose back, inverse column transform, epilogue (clamp, store)
//
// The transposes move 128 KB through 66 KB of LDS (two workgroups per CU: eight waves, two per SIMD, as in conv_wfft.hip) in
// two rounds: every lane sends half its registers, the waves whose rows those are receive theirs -- 64 values per lane, 32
// into the registers just freed and 32 into a spare set, which is why the window pair's 128 registers leave room for
// this at all --, then the other half.  Four workgroup barriers per transpose.
// No MFMA, no library FFT.

#include "conv_w128_body.h"

namespace {

#if defined(PB_EXPERIMENTAL) && defined(PB_W128_TRACE)
constexpr int kTraceGroups = 8192, kTraceStamps = 12;
__device__ unsigned long long g_w128_trace[kTraceGroups * kTraceStamps];
#endif

// One workgroup of four waves per window pair; the GRID is the job list, as in conv_wfft.hip: workgroup b belongs to list
// b % 8 (the XCD it is observed to run on) at position b / 8, every list owns the same contiguous eighth of every plane's
// pairs, images in order; the jobs are the window pairs of the images whose record says "one pass on 128 x 128 windows"
// (pb_fft_sel.poly == 2), each with its own halos.
template <typename TIn, typename TOut, bool ZERO>
__global__ __launch_bounds__(256, 2) void conv_w128_kernel(const ConvPass a, const W128Geom g) {
    extern __shared__ __attribute__((aligned(16))) float2 Zw[];
    const int lane = threadIdx.x & 63;
#if defined(PB_EXPERIMENTAL) && defined(PB_W128_TRACE)
    unsigned long long *tr = (blockIdx.x < kTraceGroups && threadIdx.x < 64) ? g_w128_trace + (long)blockIdx.x * kTraceStamps : nullptr;
    PB_WT(0);
    PB_WRT(9);
#endif
    const int C = a.C, B = a.P / C;
    const int q = (int)(blockIdx.x & 7u);
    int rem = (int)(blockIdx.x >> 3);
    int img = 0, hx = 0, hy = 0;
    if (B == 1) {
        const PB_CONSTANT pb_fft_sel *s0 = as_constant(a.fsel);
        if (!s0->use_fft || s0->poly != 2) return;
        hx = s0->hx; hy = s0->hy;
    } else {
        auto share_of = [&](int i) -> int {
            if (i >= B) return 0;
            const pb_fft_sel s = a.fsel[i];
            if (!s.use_fft || s.poly != 2) return 0;
            return jobs128_of(g, s.hx, s.hy).per * C;
        };
        bool work = false;
        int base = 0;
        for (int c0 = 0; c0 < B; c0 += 64) {
            const int n = share_of(c0 + lane), incl = wave_scan(n, lane);
            const unsigned long long m = __ballot(base + incl > rem);
            if (m) {
                const int l = __builtin_ctzll(m);
                img = c0 + l;
                rem -= base + (__builtin_amdgcn_readlane(incl, l) - __builtin_amdgcn_readlane(n, l));
                work = true;
                break;
            }
            base += __builtin_amdgcn_readlane(incl, 63);
        }
        if (!work) return;
        img = __builtin_amdgcn_readfirstlane(img); rem = __builtin_amdgcn_readfirstlane(rem);
        hx = as_constant(a.fsel + img)->hx; hy = as_constant(a.fsel + img)->hy;
    }
    const W128Jobs j = jobs128_of(g, hx, hy);
    const int pl = __builtin_amdgcn_readfirstlane(div_rcp128(rem, __builtin_amdgcn_rcpf((float)j.per)));
    if (pl >= C) return;
    const int pair = q * j.per + (rem - pl * j.per);
    if (pair >= j.njobs) return;
    const int ty = __builtin_amdgcn_readfirstlane(div_rcp128(pair, j.inv_pairs_x)), pxi = pair - ty * j.pairs_x;
    w128_pair<TIn, TOut, ZERO>(a, img * C + pl, ty, pxi, hx, hy, Zw, a.khat + (long)img * PB_KHAT_STRIDE PB_WT_PASS);
}

template <typename TIn, typename TOut>
int launch_w128_typed(pb_ctx *ctx, const ConvPass &p, const W128Geom &g, long groups) {
    if (p.boundary == PB_ZERO)
        hipLaunchKernelGGL((conv_w128_kernel<TIn, TOut, true>), dim3((unsigned)groups), dim3(256), kW128Lds, ctx->stream, p, g);
    else
        hipLaunchKernelGGL((conv_w128_kernel<TIn, TOut, false>), dim3((unsigned)groups), dim3(256), kW128Lds, ctx->stream, p, g);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace

#if defined(PB_EXPERIMENTAL) && defined(PB_W128_TRACE)
extern "C" int pb_debug_w128_trace(unsigned long long *host) {
    int rc = (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_w128_trace), sizeof(g_w128_trace));
    static unsigned long long zeros[kTraceGroups * kTraceStamps];
    if (!rc) rc = (int)hipMemcpyToSymbol(HIP_SYMBOL(g_w128_trace), zeros, sizeof(zeros));
    return rc;
}
#endif

bool pb_conv_w128_types(int in_dtype, int out_dtype) { return in_dtype >= 0 && in_dtype <= 2 && out_dtype >= 0 && out_dtype <= 2; }

// Whether the job list of a launch sized for the smallest tiles (records the host has not read) stays within the grid
// (pb_poly_spec_mode asks before it admits 128 x 128 windows: an oversized batch keeps the other forms instead of failing).
bool pb_conv_w128_feasible(const ConvPass &p) {
    const int oh = (p.out_kind == OUT_INTERIOR) ? p.H : p.H + 2 * p.pad, ow = (p.out_kind == OUT_INTERIOR) ? p.W : p.W + 2 * p.pad;
    const int t = PB_POLY128_MIN_T;
    const long nj = (long)(((ow + t - 1) / t + 1) / 2) * ((oh + t - 1) / t);
    const long groups = 8L * ((nj + 7) / 8) * p.P;
    return groups > 0 && groups <= (1L << 23);
}

// The one-pass polynomial of the images whose record selects 128 x 128 windows (pb_fft_sel.poly == 2): from the first step's
// input to the last step's output (p: the composite pass -- scale 1, no x operand, the last step's clamp).
int pb_launch_conv_w128(pb_ctx *ctx, const ConvPass &p, const std::vector<pb_fft_sel> *known) {
    W128Geom g;
    g.oh = (p.out_kind == OUT_INTERIOR) ? p.H : p.H + 2 * p.pad;
    g.ow = (p.out_kind == OUT_INTERIOR) ? p.W : p.W + 2 * p.pad;
    // the job list: exactly the images' where the host has their records, else the largest their halos may ask for
    // (tiles of at least PB_POLY128_MIN_T samples per side)
    long groups = 0;
    const int B = p.P / p.C;
    auto per_of = [&](int hx, int hy) -> long {
        const int tx = W_N - 2 * hx, ty = W_N - 2 * hy;
        const long nj = (long)(((g.ow + tx - 1) / tx + 1) / 2) * ((g.oh + ty - 1) / ty);
        return (nj + 7) / 8;
    };
    if (known) {
        long per_sum = 0;
        for (int b = 0; b < B && b < (int)known->size(); ++b) {
            const pb_fft_sel &e = (*known)[(size_t)b];
            if (e.use_fft && e.poly == 2) per_sum += per_of(e.hx, e.hy);
        }
        if (!per_sum) return PB_OK;
        groups = 8L * per_sum * p.C;
    } else {
        const int hmax = (W_N - PB_POLY128_MIN_T) / 2;
        groups = 8L * per_of(hmax, hmax) * p.P;
    }
    if (groups <= 0 || groups > (1L << 23)) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "conv pass: too many 128 x 128 windows");
    ProfScope prof(ctx, PB_PROF_CONV_FFT);
    switch (p.in_dtype * 3 + p.out_dtype) {
        case 0: return launch_w128_typed<float, float>(ctx, p, g, groups);
        case 1: return launch_w128_typed<float, __half>(ctx, p, g, groups);
        case 3: return launch_w128_typed<__half, float>(ctx, p, g, groups);
        case 4: return launch_w128_typed<__half, __half>(ctx, p, g, groups);
        case 2: return launch_w128_typed<float, unsigned char>(ctx, p, g, groups);
        case 5: return launch_w128_typed<__half, unsigned char>(ctx, p, g, groups);
        case 6: return launch_w128_typed<unsigned char, float>(ctx, p, g, groups);
        case 7: return launch_w128_typed<unsigned char, __half>(ctx, p, g, groups);
        case 8: return launch_w128_typed<unsigned char, unsigned char>(ctx, p, g, groups);
        default: return pb_fail(ctx, PB_ERR_UNSUPPORTED, "128 x 128 window pass: unsupported dtype combination %d -> %d", p.in_dtype, p.out_dtype);
    }
}
