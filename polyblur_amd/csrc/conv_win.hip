// The one window pass of a polynomial whose records the host has not read (PolySpec.always == 1): ONE launch for both window
// forms.
//
// Every image of such a polynomial takes one window pass, on 128 x 128 windows (conv_w128.hip: four waves per window pair) or
// on 64-wide ones (conv_wfft.hip: one wave per pair of 64 x 64 windows or per window 64 wide and 128 tall); which, its
// device-built record says.  Two launches, each skipping the other's images, leave one launch of a single image's call without
// work -- 3.5 - 5.8 us on the critical path of every iteration for a grid that starts and retires at once.  Here a workgroup of
// four waves looks its image's record up and runs EITHER body:
//
//   128 x 128 windows (pb_fft_sel.poly == 2)   one window pair by the four waves: w128_pair, as conv_w128_kernel runs it
//   64-wide windows   (pb_fft_sel.poly == 1)   four one-wave jobs, wave w the job 4 pos + w of the image's share of its list,
//                                              in LDS slice w: wave_pair / wave_tall with the branch order of conv_wfft_kernel
//                                              for a composite pass (no ring, no taper, no fold)
//
// The form is a fact of the image, hence of the workgroup: a workgroup that runs wave jobs never meets the barriers of
// w128_pair.  The bodies are the other two kernels' (conv_w128_body.h, conv_wfft_body.h): same jobs, same arithmetic, the same
// bits.
//
// Job lists: workgroup b belongs to list b % 8 at position b / 8, images in order, as in both other kernels; an image's share
// of a list is per * C workgroups (128 x 128: per = an eighth of a plane's window pairs) or ceil(per * C / 4) workgroups
// (64-wide: per = an eighth of a plane's jobs).  The four waves of a workgroup take consecutive jobs of the same list -- the
// same image, usually the same plane and row of tiles, neighbouring halos -- and each decodes its own plane, row and pair, so
// the waves of the workgroup that straddles two planes land in different planes; a wave past the share's end leaves.
// No MFMA, no library FFT.

#include "conv_wave_common.h"

// The bodies' lane and wave index WITHOUT the thread index: with it the kernel keeps that register alive through every body --
// the fp32 instantiation, whose 64 x 128 body needs 253 registers beside the two that hold spilled scalars, then spills it to
// scratch (8 bytes per lane, the only scratch of the kernel).  The lane from the wave's own count needs no input at all; the
// wave index is wave-uniform.
namespace {
__device__ __forceinline__ int win_lane() { return (int)__builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }
__device__ __forceinline__ int win_wave() { return __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)); }
}  // namespace
#define PB_LANE_ID() win_lane()
#define PB_WAVE_ID() win_wave()

#include "conv_w128_body.h"
#include "conv_wfft_body.h"

namespace {

constexpr size_t kWinLds = kW128Lds > 4 * kWfLdsWave ? kW128Lds : 4 * kWfLdsWave;

// which body an image's record asks of this launch: 2 = 128 x 128 windows, 1 = 64-wide windows, 0 = none (another launch's image)
__device__ __forceinline__ int win_form(const ConvPass &a, int use_fft, int poly) {
    if (!use_fft) return 0;
    if (poly == 2) return 2;
    return poly_match(a.poly, poly) ? 1 : 0;
}

template <typename TIn, typename TOut, bool ZERO>
__global__ __launch_bounds__(256, 2) void conv_win_kernel(const ConvPass a, const WGeom g) {
    extern __shared__ __attribute__((aligned(16))) char zs[];
    const int lane = win_lane();
    const int w = win_wave();
#if defined(PB_EXPERIMENTAL) && defined(PB_W128_TRACE)
    unsigned long long *tr = nullptr;
#endif
    // (windows 64 wide and 128 tall: as in conv_wfft_kernel, only the instantiation of the planes PolySpec.tall vouches for)
    constexpr bool kTall = std::is_same<TIn, float>::value && std::is_same<TOut, float>::value && !ZERO;
    const W128Geom g128 = {g.ow, g.oh};
    const int C = a.C, B = a.P / C;
    const int q = (int)(blockIdx.x & 7u);
    int rem = (int)(blockIdx.x >> 3);                  // position in the list, in workgroups
    int img = 0, hx = 0, hy = 0, form = 0;
    bool tall = false;
    if (B == 1) {
        const PB_CONSTANT pb_fft_sel *s0 = as_constant(a.fsel);
        form = win_form(a, s0->use_fft, s0->poly);
        if (!form) return;
        hx = s0->hx; hy = s0->hy;
        tall = kTall && s0->poly == 1 && s0->pad_[0] != 0;
    } else {
        // list entries of image i, in workgroups (every wave forms the same sums: nothing to share, no barrier)
        auto share_of = [&](int i) -> int {
            if (i >= B) return 0;
            const pb_fft_sel s = a.fsel[i];
            const int f = win_form(a, s.use_fft, s.poly);
            if (f == 2) return jobs128_of(g128, s.hx, s.hy).per * C;
            if (f == 1) return (jobs_of(g, s.hx, s.hy, kTall && s.poly == 1 && s.pad_[0] != 0).per * C + 3) >> 2;
            return 0;
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
        const PB_CONSTANT pb_fft_sel *si = as_constant(a.fsel + img);
        form = win_form(a, si->use_fft, si->poly);
        hx = si->hx; hy = si->hy;
        tall = kTall && si->poly == 1 && si->pad_[0] != 0;
    }
    const float *kp = a.khat + (long)img * PB_KHAT_STRIDE;
    if (form == 2) {
        // one window pair by the whole workgroup: conv_w128_kernel's decode
        const W128Jobs j = jobs128_of(g128, hx, hy);
        const int pl = __builtin_amdgcn_readfirstlane(div_rcp128(rem, __builtin_amdgcn_rcpf((float)j.per)));
        if (pl >= C) return;
        const int pair = q * j.per + (rem - pl * j.per);
        if (pair >= j.njobs) return;
        const int ty = __builtin_amdgcn_readfirstlane(div_rcp128(pair, j.inv_pairs_x)), pxi = pair - ty * j.pairs_x;
        w128_pair<TIn, TOut, ZERO>(a, img * C + pl, ty, pxi, hx, hy, reinterpret_cast<float2 *>(zs), kp PB_WT_PASS);
        return;
    }
    // four wave jobs: this wave's is the job 4 rem + w of the image's per * C (conv_wfft_kernel's decode from there on; the
    // reciprocal divisions are exact below 2^21 and job < per * C <= 2^20: pb_poly_spec_mode bounds the list)
    const WJobs j = jobs_of(g, hx, hy, tall);
    const int job = 4 * rem + w;
    if (job >= j.per * C) return;                      // (the ragged end of the share; one image: positions beyond its planes)
    const int pl = __builtin_amdgcn_readfirstlane(div_rcp(job, __builtin_amdgcn_rcpf((float)j.per)));
    const int pair = q * j.per + (job - pl * j.per);
    if (pair >= j.njobs) return;                       // (the ragged end of the last list's run)
    const int ty = __builtin_amdgcn_readfirstlane(div_rcp(pair, j.inv_pairs_x)), pxi = pair - ty * j.pairs_x;
    const int plane = img * C + pl;
    const pb_blur_info *info = a.info + img;
    char *zb = zs + w * (int)kWfLdsWave;
    if constexpr (kTall) {
        if (tall) { wave_tall(a, plane, ty, pxi, hx, hy, zb, kp); return; }
    }
    if (pair_is_fast<TIn, TIn, TOut>(a, ty, pxi, hx, hy)) wave_pair<1, TIn, TIn, TOut, ZERO>(a, info, plane, ty, pxi, hx, hy, zb, kp, nullptr);
    else if (pair_is_gen<TIn, TIn, TOut>(a, pxi, hx)) wave_pair<2, TIn, TIn, TOut, ZERO>(a, info, plane, ty, pxi, hx, hy, zb, kp, nullptr);
    else wave_pair<0, TIn, TIn, TOut, ZERO>(a, info, plane, ty, pxi, hx, hy, zb, kp, nullptr);
}

template <typename TIn, typename TOut>
int launch_win_typed(pb_ctx *ctx, const ConvPass &p, const WGeom &g, long groups) {
    if (p.boundary == PB_ZERO)
        hipLaunchKernelGGL((conv_win_kernel<TIn, TOut, true>), dim3((unsigned)groups), dim3(256), kWinLds, ctx->stream, p, g);
    else
        hipLaunchKernelGGL((conv_win_kernel<TIn, TOut, false>), dim3((unsigned)groups), dim3(256), kWinLds, ctx->stream, p, g);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

}  // namespace

// The composite passes the merged launch is built for: those both other launches serve -- a plain Horner pass without ring or
// taper, the x operand of the window's own type (it is never read: the polynomial carries its b x in the spectrum).
bool pb_conv_win_types(const ConvPass &p) {
    if (p.poly != 1 || p.ring || p.epilogue != EPI_HORNER || p.x_dtype != p.in_dtype) return false;
    return pb_conv_wfft_types(p) && pb_conv_w128_types(p.in_dtype, p.out_dtype);
}

// The one window pass of every image of the batch, whichever form its record selects (p: the composite pass).  The grid is the
// longer of the two forms' worst-case job lists where the host has not read the records, else (`known`: the timing tool's
// lab switch) exactly the images' lists.  spec: what p.khat was built under (behind an edgetaper: the second set's).
// A pass pb_conv_win_types does not admit is refused: the chooser (poly_choice.h) asks first and plans the two launches there.
int pb_launch_conv_win(pb_ctx *ctx, const ConvPass &p, const PolySpec &spec, const std::vector<pb_fft_sel> *known) {
    if (!pb_conv_win_types(p)) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "one-launch window pass: not built for this pass (types %d -> %d)", p.in_dtype, p.out_dtype);
    const bool poly2 = spec.on >= 2, tall = poly2 && spec.tall != 0;
    WGeom g;
    long per_max = 0;
    if (!wfft_geometry(p, poly2, tall, (float)PB_POLY_MIN_AREA, g, per_max))
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "conv pass: too many windows for the one-launch window pass");
    const int B = p.P / p.C;
    const int hmax = (W_N - PB_POLY128_MIN_T) / 2;
    long groups = 8L * B * std::max(w128_per_of(g.ow, g.oh, hmax, hmax) * p.C, (per_max * p.C + 3) / 4);
    if (known) {
        long share_sum = 0;
        for (int b = 0; b < B && b < (int)known->size(); ++b) {
            const pb_fft_sel &e = (*known)[(size_t)b];
            if (!e.use_fft || e.poly == 0) continue;
            if (e.poly == 2) { share_sum += w128_per_of(g.ow, g.oh, e.hx, e.hy) * p.C; continue; }
            share_sum += ((wfft_jobs_of(g, e, tall) + 7) / 8 * p.C + 3) / 4;
        }
        if (!share_sum) return PB_OK;
        groups = 8L * share_sum;
    }
    if (groups <= 0 || groups > (1L << 23)) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "conv pass: too many windows for the one-launch window pass");
    ProfScope prof(ctx, PB_PROF_CONV_FFT);
    switch (p.in_dtype * 3 + p.out_dtype) {
        case 0: return launch_win_typed<float, float>(ctx, p, g, groups);
        case 1: return launch_win_typed<float, __half>(ctx, p, g, groups);
        case 2: return launch_win_typed<float, unsigned char>(ctx, p, g, groups);
        case 3: return launch_win_typed<__half, float>(ctx, p, g, groups);
        case 4: return launch_win_typed<__half, __half>(ctx, p, g, groups);
        case 6: return launch_win_typed<unsigned char, float>(ctx, p, g, groups);
        case 8: return launch_win_typed<unsigned char, unsigned char>(ctx, p, g, groups);
        default: return pb_fail(ctx, PB_ERR_UNSUPPORTED, "one-launch window pass: not built for this pass (types %d -> %d)", p.in_dtype, p.out_dtype);
    }
}
