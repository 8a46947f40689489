// Tile-spectrum body of the reblurring pass, one WAVE per window pair.
//
// Same pass, same operands, same result as conv_fft.hip (one Horner step  t <- K*t + coef*x  of the polynomial
// deconvolution, reference deblurring.py:122-138 / :141-169, or one edgetaper blend, edgetaper.py:30-32, with the
// boundary models of filters.py:14-49): the exact 2-D stencil of a 64 x 64 window is evaluated as a circular correlation
// -- forward 2-D DFT, product with the kernel's real 64 x 64 spectrum (khat_kernel, conv_fft.hip), inverse DFT, of which
// the samples at least R from the window's edge are kept (overlap-save); two horizontally adjacent real windows ride
// one complex transform, z = A + iB.
//
// What differs is who does it.  conv_fft.hip spreads a window pair over 512 threads: eight 8-point butterfly stages,
// six LDS round trips and seven workgroup barriers per pair, every stage exposing an LDS or barrier latency.  Here a
// window pair belongs to ONE wave and a whole 64-point line to one lane (64 complex values = 128 registers):
//
//   load      lane = window column x, register y = window row: 2 x 64 row-segment loads of 256 bytes per wave
//   columns   fft64 in registers (two radix-8 stages, compile-time twiddles in scalar registers), no LDS, no barrier
//   transpose through the wave's private LDS tile: lane = transformed row, register = column
//   rows      fft64, x real spectrum (64 values per lane, [x position][y position] layout: coalesced), inverse fft64
//   transpose back
//   columns   inverse fft64; lane = window column again: the epilogue (scale, + coef * x, clamp) and the stores walk
//             rows with 256-byte segments per wave instruction
//
// Two LDS round trips per pair instead of six, no workgroup barrier at all (a wave's DS operations execute in order;
// only the compiler has to be told, wave_lds_fence), rows wave-uniform -- every row offset, boundary mapping and
// validity test is scalar work -- and columns one map per lane and window.  Border windows, the taper epilogue and
// ragged ends therefore run the same code as interior ones with different offsets (an out-of-range buffer offset
// loads 0 / drops the store).
//
// The transposes keep only HALF a window pair in LDS at a time (16.6 KB per wave, eight waves per CU): a 64 x 64
// transpose is the swap of the two off-diagonal 32 x 32 quadrants -- v_permlane32_swap between the wave's halves --
// followed by a transpose inside each quadrant, and the quadrant pairs go through the same 32 x 64 LDS tile one after
// the other.
//
// Work items: window pairs of the images whose record selects this body, every image with its own tile size (prefix sum
// over the batch's pb_fft_sel records inside the kernel: no idle slots for images with larger tiles, no host read-back);
// workgroup b runs on XCD b % 8 (observed, used for speed only) and every XCD takes the same contiguous eighth of every
// plane's pairs, so neighbouring windows share their halos in that XCD's L2.
// No MFMA, no library FFT.

#include "conv_wfft_body.h"

namespace {

#ifdef PB_WF_TRACE
constexpr int kTraceWaves = 8192, kTraceStamps = 14;
__device__ unsigned long long g_wf_trace[kTraceWaves * kTraceStamps];
#endif

// One wave (= one workgroup) per window pair; the GRID is the job list.  The jobs are the window pairs of the images whose
// record selects this body, every image with its own halos and therefore its own tile size (prefix sum over the batch's
// pb_fft_sel records: no host read-back; the grid is sized for the smallest tile the records may select and the surplus
// workgroups leave at once).  Workgroup b belongs to list b % 8 (the XCD it is observed to run on -- used for speed only)
// at position b / 8; every list owns the same eighth of EVERY plane's pairs -- a contiguous run, so neighbouring windows
// share their halos in that XCD's L2 -- in the order image, plane, pair.
//
// (Measured and dropped, round 3: the three Horner steps of a polynomial in ONE launch -- step-major lists, per-plane
// completion counters, write-through stores, one agent-scope acquire per pair: with every synchronisation compiled out
// the single launch takes exactly what the three launches take; three waves per SIMD instead of two -- 168 registers, the
// spectrum streamed, a 16-row transpose tile: 119 us per 4K pass against 85, nothing can be requested far enough ahead.
// NOTEBOOK.md has the records.)
template <typename TIn, typename TX, typename TOut, bool ZERO>
__global__ __launch_bounds__(64, 2) void conv_wfft_kernel(const ConvPass a, const WGeom g) {
    extern __shared__ __attribute__((aligned(16))) char zb[];
    const int lane = threadIdx.x & 63;
    unsigned long long *tr = nullptr;
#ifdef PB_WF_TRACE
    if (blockIdx.x < kTraceWaves) tr = g_wf_trace + (long)blockIdx.x * kTraceStamps;
    PB_T(0);
    PB_TRT(12);
#endif
    const int C = a.C, B = a.P / C;
    const int q = (int)(blockIdx.x & 7u);
    int rem = (int)(blockIdx.x >> 3);                  // position in the list
    int img = 0, hx = 0, hy = 0;
    bool fold = false, tall = false;
    // (windows 64 wide and 128 tall: a one-pass record says so, and only the instantiation of the planes PolySpec.tall vouches for
    // carries the body)
    constexpr bool kTall = std::is_same<TIn, float>::value && std::is_same<TX, float>::value && std::is_same<TOut, float>::value && !ZERO;
    if (B == 1) {
        // (one image: its record is read on the scalar side -- no trip through the vector memory queue)
        const PB_CONSTANT pb_fft_sel *s0 = as_constant(a.fsel);
        if (!s0->use_fft || s0->poly == 2 || !poly_match(a.poly, s0->poly)) return;     // (poly == 2: conv_w128.hip's image)
        hx = s0->hx; hy = s0->hy;
        fold = a.poly == 2 && s0->poly != 0;
        tall = kTall && s0->poly == 1 && s0->pad_[0] != 0;
    } else {
        // list entries of image i: its share of every plane
        auto share_of = [&](int i) -> int {
            if (i >= B) return 0;
            const pb_fft_sel s = a.fsel[i];
            if (!s.use_fft || s.poly == 2 || !poly_match(a.poly, s.poly)) return 0;
            return jobs_of(g, s.hx, s.hy, kTall && s.poly == 1 && s.pad_[0] != 0).per * C;
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
        fold = a.poly == 2 && as_constant(a.fsel + img)->poly != 0;
        tall = kTall && as_constant(a.fsel + img)->poly == 1 && as_constant(a.fsel + img)->pad_[0] != 0;
    }
    const WJobs j = jobs_of(g, hx, hy, tall);
    const int pl = __builtin_amdgcn_readfirstlane(div_rcp(rem, __builtin_amdgcn_rcpf((float)j.per)));
    if (pl >= C) return;                               // (one image: positions beyond its planes)
    const int pair = q * j.per + (rem - pl * j.per);
    if (pair >= j.njobs) return;                       // (the ragged end of the last list's run)
    const int ty = __builtin_amdgcn_readfirstlane(div_rcp(pair, j.inv_pairs_x)), pxi = pair - ty * j.pairs_x;
    const int plane = img * C + pl;
    const float *kp = a.khat + (long)img * PB_KHAT_STRIDE;
    const pb_blur_info *info = a.info + img;
    if (a.ring && !ring_live(a, ty, pxi, hx, hy)) return;
    const ConvPass af = fold_pass(a, fold);
    if constexpr (kTall) {
        if (tall) { wave_tall(af, plane, ty, pxi, hx, hy, zb, kp); return; }
    }
    if (taper_is_copy(af, ty, pxi, hx, hy)) { copy_pair<TX, TOut>(af, plane, ty, pxi, hx, hy); return; }
    if (pair_is_fast<TIn, TX, TOut>(af, ty, pxi, hx, hy)) wave_pair<1, TIn, TX, TOut, ZERO>(af, info, plane, ty, pxi, hx, hy, zb, kp, tr);
    else if (pair_is_gen<TIn, TX, TOut>(af, pxi, hx)) wave_pair<2, TIn, TX, TOut, ZERO>(af, info, plane, ty, pxi, hx, hy, zb, kp, tr);
    else wave_pair<0, TIn, TX, TOut, ZERO>(af, info, plane, ty, pxi, hx, hy, zb, kp, tr);
}

template <typename TIn, typename TX, typename TOut>
int launch_wfft_typed(pb_ctx *ctx, const ConvPass &p, const WGeom &g, long groups) {
    if (p.boundary == PB_ZERO)
        hipLaunchKernelGGL((conv_wfft_kernel<TIn, TX, TOut, true>), dim3((unsigned)groups), dim3(64), kWfLdsWave, ctx->stream, p, g);
    else
        hipLaunchKernelGGL((conv_wfft_kernel<TIn, TX, TOut, false>), dim3((unsigned)groups), dim3(64), kWfLdsWave, ctx->stream, p, g);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace

#ifdef PB_WF_TRACE
extern "C" int pb_debug_wf_trace_clear(void) {
    void *p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_wf_trace)) != hipSuccess) return -1;
    return (int)hipMemset(p, 0, sizeof(unsigned long long) * kTraceStamps * kTraceWaves);
}
extern "C" int pb_debug_wf_trace(unsigned long long *host, int n_waves) {
    if (n_waves > kTraceWaves) n_waves = kTraceWaves;
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_wf_trace), sizeof(unsigned long long) * kTraceStamps * n_waves);
}
#endif

// (as pb_conv_w128_feasible: the largest job list a pass with one-pass images of the smallest tiles may need)
bool pb_conv_wfft_feasible(const ConvPass &p, bool poly2) {
    WGeom g; long per_max = 0;
    return wfft_geometry(p, poly2, poly2 && p.boundary == PB_WRAP, (float)PB_POLY_MIN_AREA, g, per_max);
}

bool pb_conv_wfft_types(const ConvPass &p) {
    switch (p.in_dtype * 9 + p.x_dtype * 3 + p.out_dtype) {
        case 0: case 1: case 3: case 4: case 12: case 13: case 24: case 26: case 6: case 8: case 2: return true;
        default: return false;
    }
}

// A pass it is not built for -- a dtype combination without a kernel, a three-step job list beyond the grid -- is refused: the
// chooser (poly_choice.h) asks pb_conv_wfft_types / pb_conv_wfft_feasible first and plans the workgroup form there.  Every pass whose
// types are built comes here whatever its size, so that what an image gets does not depend on the batch it travels in (the two
// forms round differently: this one rotates the window rows and has per-axis halos).  A wave takes ~19 us for its pair
// whatever the size of the launch, a 512-thread workgroup ~8 us, so a three-step pass of a few hundred pairs is a race of
// single pairs that the workgroup form used to win (700 x 500: 0.31 against 0.38 ms per call); with small images' polynomials
// mostly one window pass now, the call is faster through this form alone (0.29 ms; 1080p 0.45 against 0.53).
int pb_launch_conv_wfft(pb_ctx *ctx, const ConvPass &p, const PolySpec &spec, const std::vector<pb_fft_sel> *known) {
    const int key = p.in_dtype * 9 + p.x_dtype * 3 + p.out_dtype;
    if (!pb_conv_wfft_types(p)) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "wave-form pass: unsupported dtype combination %d", key);
    const bool poly2 = p.poly != 0 && spec.on >= 2;
    const float min_area = (float)PB_POLY_MIN_AREA;        // (the smallest one-pass tile the cost model of khat.h admits)
    WGeom g;
    long per_max = 0;
    const bool tall = poly2 && spec.tall != 0;
    if (!wfft_geometry(p, poly2, tall, min_area, g, per_max))
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "conv pass: too many windows for the tile-spectrum body");
    long groups = 8L * per_max * p.P;                       // list entries if every image had the smallest tiles its records may select
    if (known) {
        // the host has the records' choices (it built them): the grid is exactly the list of this launch's jobs
        const int B = p.P / p.C;
        long per_sum = 0, jobs = 0;
        for (int b = 0; b < B && b < (int)known->size(); ++b) {
            const pb_fft_sel &e = (*known)[(size_t)b];
            const bool takes = e.use_fft && e.poly != 2 && (p.poly == 2 || (e.poly != 0) == (p.poly != 0));      // (poly_match, conv_fft_common.h)
            if (!takes) continue;
            const long nj = wfft_jobs_of(g, e, tall);
            per_sum += (nj + 7) / 8; jobs += nj * p.C;
        }
        if (!jobs) return PB_OK;                            // nothing in this launch for any image
        groups = 8L * per_sum * p.C;                        // (the kernel's list: the images' shares of every plane, back to back)
    }
    ProfScope prof(ctx, PB_PROF_CONV_FFT);
    // fp32 planes; the second and third Horner step of fp16 images (fp32 temporaries in, fp16 x operand, fp32 or fp16 out);
    // the first step and the one-pass polynomial of fp16 images (fp16 window)
    switch (key) {
        case 0: return launch_wfft_typed<float, float, float>(ctx, p, g, groups);
        case 1: return launch_wfft_typed<float, float, __half>(ctx, p, g, groups);          // (the last store of an fp16 image after fp32 iterations)
        case 3: return launch_wfft_typed<float, __half, float>(ctx, p, g, groups);
        case 4: return launch_wfft_typed<float, __half, __half>(ctx, p, g, groups);
        case 12: return launch_wfft_typed<__half, __half, float>(ctx, p, g, groups);
        case 13: return launch_wfft_typed<__half, __half, __half>(ctx, p, g, groups);
        // 8-bit images: the first step (fp32 out) or the one-pass polynomial (fp32 or 8-bit out) from the 8-bit window, the
        // later steps with the 8-bit x operand, the last store
        case 24: return launch_wfft_typed<unsigned char, unsigned char, float>(ctx, p, g, groups);
        case 26: return launch_wfft_typed<unsigned char, unsigned char, unsigned char>(ctx, p, g, groups);
        case 6: return launch_wfft_typed<float, unsigned char, float>(ctx, p, g, groups);
        case 8: return launch_wfft_typed<float, unsigned char, unsigned char>(ctx, p, g, groups);
        case 2: return launch_wfft_typed<float, float, unsigned char>(ctx, p, g, groups);
        default: return pb_fail(ctx, PB_ERR_UNSUPPORTED, "wave-form pass: unsupported dtype combination %d", key);
    }
}
