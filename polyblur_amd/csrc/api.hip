// C ABI of libpolyblur_hip.so (include/polyblur_hip.h): context, scratch memory, and the
// drivers that chain the kernels of conv.hip / estimate.hip / filters.hip on one stream.
// Mirrors polyblur_deblurring's main loop (reference deblurring.py:58-96) and
// inverse_filtering_rank3 (deblurring.py:211-239).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "common.h"
#include "poly_choice.h"

// (g_dtype: the type of the gradient planes gx, gy, ox -- PB_F32, or PB_F16 inside an fp16 call of the pipeline)
int pb_grad_energy(pb_ctx *ctx, const void *gx, const void *gy, float *nM, int P, long HW, int g_dtype = PB_F32);
int pb_fourier_gradients_backward_impl(pb_ctx *ctx, const float *grad_gx, const float *grad_gy, int P, int H, int W, float *grad_planes);   // halo_grad.hip
int pb_halo_mask_backward_impl(pb_ctx *ctx, const float *x, const float *y, const float *grad0_x, const float *grad0_y, const float *grad_out,
                               float *grad_x, float *grad_y, float *grad_grad0_x, float *grad_grad0_y, int B, int C, int H, int W);
int pb_halo_apply(pb_ctx *ctx, const void *x, int x_dtype, int x_pitch, long x_plane, const float *y, const void *gx,
                  const void *gy, const void *ox, const float *nM, void *out, int out_dtype, int P, int H, int W,
                  int clamp01, const void *recomb_cur = nullptr, int recomb_cur_dtype = 0, const float *recomb_smooth = nullptr,
                  int g_dtype = PB_F32);
int pb_recombine(pb_ctx *ctx, const float *y, const void *cur, int cur_dtype, const float *smooth, void *out, int out_dtype,
                 long n);
int pb_bilateral5_impl(pb_ctx *ctx, const void *in, int in_dtype, void *out, int out_dtype, int P, int H, int W);
int pb_dt_filter_impl(pb_ctx *ctx, const void *in, const void *joint, int dtype, float *out, int B, int C, int H, int W,
                      float sigma_s, float sigma_r, int num_iterations);
int pb_nc_filter_impl(pb_ctx *ctx, const void *in, int dtype, float *out, int B, int C, int H, int W, float sigma_s,
                      float sigma_r, int num_iterations);
int pb_convert_from_float(pb_ctx *ctx, const float *in, void *out, int dtype, long n);
int pb_u8_layout(pb_ctx *ctx, const unsigned char *in, unsigned char *out, int B, int C, int H, int W, int to_planar);
int pb_convert_to_float(pb_ctx *ctx, const void *in, int dtype, float *out, long n);
int pb_extract_patches_impl(pb_ctx *ctx, const void *img, void *patches, int dtype, int B, int C, int H, int W, int ph, int pw,
                            int step_h, int step_w, int n_j, int pad_top, int pad_left, int first, int count);
int pb_overlap_add_impl(pb_ctx *ctx, const void *patches, void *out, int dtype, int B, int C, int H, int W, int ph, int pw,
                        int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left, const float *win_y,
                        const float *win_x);

#ifndef PB_EXPERIMENTAL
// (conv_xt.hip -- both 1-D passes of the x-t approximation in one launch -- is a measured experiment of the --experimental
// build: slower than the exact path it approximates.  The default build runs method='direct_separable' as two launches
// of the general body over the two sparse records.)
int pb_launch_conv_xt(pb_ctx *, const ConvPass &) { return PB_ERR_UNSUPPORTED; }
#endif

int pb_fail(pb_ctx *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

void *pb_scratch(pb_ctx *ctx, const char *name, size_t bytes) {
    ScratchBuf &b = ctx->scratch[name];
    if (b.bytes >= bytes && b.p) return b.p;
    if (b.p) {
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(b.p);
        b.p = nullptr;
        b.bytes = 0;
    }
    const size_t want = (bytes + 255) & ~(size_t)255;
    if (hipMalloc(&b.p, want) != hipSuccess) {
        b.p = nullptr;
        pb_fail(ctx, PB_ERR_NOMEM, "scratch '%s': hipMalloc(%zu) failed", name, want);
        return nullptr;
    }
    b.bytes = want;
    return b.p;
}

static size_t dsize(int dtype) { return dtype == PB_F16 ? 2 : (dtype == PB_U8 ? 1 : 4); }
static int pitch4(int w) { return (w + 3) & ~3; }

// Every environment knob of the library, read ONCE per context (pb_create) into pb_ctx -- no kernel launcher looks at the
// environment.  They exist to compare forms on the same box (bench.py's context entries, tools/), not to configure a
// deployment: the defaults are the product.
//   PB_FFT_BODY=wg|wave         which form of the tile-spectrum body runs three-step passes (wave; fp16 temporaries --
//                               pb_options.half_temporaries -- always take the workgroup form, the only one built for them)
//   PB_POLY1=0..3               one-pass polynomial: 0 never, 1 4-sample halo class only, 2 + 64 x 64 windows with the
//                               composite's halos, 3 (default) + 128 x 128 windows
//   PB_ZERO_RING=0              method='direct' keeps three Horner steps over the whole image
//   PB_ZERO_RING_MIN_PAIRS=<n>  ... its window pass + border ring form only for images of at least n three-step window pairs (4096)
//   PB_TAPER_RING=0             the second and third blend of an edgetaper over the whole plane, not over the border ring
//   PB_POLY_PADDED=0            the polynomial after an edgetaper keeps three Horner steps
//   PB_POLY_ALWAYS=0            never PolySpec.always (issue every launch the records might need)
//   PB_EST_GRAY_ROWS=0|1|2      gray + range + row transform in one launch: never | fp32 lines up to 4096 | any line in LDS
//   PB_EST_LEAN=0               the parameter kernel forms the whole record before the spectra (no short chain)
//   PB_DT_ROWS_REG=0|1|2|3      the domain transform's first row pass (dt_choice.h): through global memory | the row in registers, on one wave
//                               or -- up to 8192 rows in the batch -- over the four waves of a workgroup | one wave always | four waves always
//   PB_DT_COLS_STRIP=0|1|2      its column pass by one thread per column: two sweeps through global memory | strips, the weights stored
//                               where that pays (three fp32 channels, 128 rows and up) | strips, the weights always formed from J again
//   PB_DT_COLS_COOP=0|1|2       its column pass by workgroups of 16 (one channel: 64) columns through LDS: never | up to 24576 columns
//                               in the batch | always where rows and operands lie on 16-byte boundaries
//   PB_FFT_EXT_RADIX=0          greedy transform plans only (radices up to 16)
//   PB_FFT_FIRST / _ROWS=0|r    the column / row transform's first and last stage: the greedy plan's order, or radix r (default: by line length)
//   PB_COLS_FIXED=0, PB_ROWS_FIXED=0   the line transforms always by the run-time-plan kernels (estimate.hip), also where
//                               lines_fixed.hip holds the plan (the tests' bit-identity reference)
//   PB_POLY_ONE_LAUNCH=0|2      the window pass of a polynomial on device-built records as two launches, one per window form (default 1:
//                               one launch, conv_win.hip); 2 = host-built records take the one launch too (tools/one_launch_timing.py)
//   PB_POLY_TALL=0|2            one-pass images never / wherever admitted on windows 64 wide and 128 tall (default 1: by the cost model)
//   PB_STRIP=1                  a measured experiment (conv_strip.hip): read in --experimental builds only
// A knob stays while a test, bench.py or a script under tools/ names it.  Retired, their alternatives measured and dropped in
// NOTEBOOK.md -- round 6: PB_ROWS_NT, PB_COLS_WIDE, PB_MAIN_STREAM_BODY, PB_SIDE_STREAM, PB_SIDE_MIN_TILES; after it, with their
// fields and branches: PB_POLY_GAIN, PB_POLY_MIN_AREA, PB_POLY_COST128 (constants of common.h), PB_POLY_MIN_PAIRS128,
// PB_ZERO_RING_ASIDE, PB_WAVE_MIN_JOBS, PB_FFT_LOGNB, PB_XT, PB_STRIP_SEG, PB_EST_OVERLAP, PB_DENSE_EVAL (pb_set_dense_eval is
// the interface)
static void pb_read_knobs(pb_ctx *ctx) {
    auto geti = [](const char *n, int &v) { if (const char *e = getenv(n)) v = atoi(e); };
    auto getl = [](const char *n, long &v) { if (const char *e = getenv(n)) v = atol(e); };
    if (const char *e = getenv("PB_FFT_BODY")) ctx->fft_wave = (e[0] == 'w' && e[1] == 'g') ? 0 : 1;
#ifdef PB_EXPERIMENTAL
    geti("PB_STRIP", ctx->strip_mode);
#endif
    geti("PB_EST_GRAY_ROWS", ctx->line.est_gray_rows); geti("PB_EST_LEAN", ctx->est_lean); geti("PB_DT_ROWS_REG", ctx->dt.rows_reg); geti("PB_DT_COLS_STRIP", ctx->dt.cols_strip); geti("PB_DT_COLS_COOP", ctx->dt.cols_coop);
    geti("PB_FFT_EXT_RADIX", ctx->line.fft_ext_radix); geti("PB_FFT_FIRST", ctx->line.fft_first); geti("PB_FFT_FIRST_ROWS", ctx->line.fft_first_rows); geti("PB_COLS_FIXED", ctx->line.cols_fixed); geti("PB_ROWS_FIXED", ctx->line.rows_fixed);
    geti("PB_POLY1", ctx->poly_mode); geti("PB_POLY_TALL", ctx->poly_tall); geti("PB_POLY_ONE_LAUNCH", ctx->poly_one_launch);
    geti("PB_POLY_ALWAYS", ctx->poly_always); geti("PB_POLY_PADDED", ctx->poly_padded); geti("PB_TAPER_RING", ctx->taper_ring); geti("PB_ZERO_RING", ctx->zero_ring); getl("PB_ZERO_RING_MIN_PAIRS", ctx->zero_ring_min_pairs);
}

// What the line transforms of the estimation would run for one launch (line_choice.h), under the knobs of the environment as
// pb_create reads them; host only, no device needed.  axis 0: rows of n samples, `other` of them per plane; 1: columns of n
// samples, `other` of them; use = LineUse's seven fields in order.  out (37 ints): kind, taken, threads, lognb, tiles, lds,
// max_radix, sat, half_ok, ext, first, bluestein_m, nstage, the radices.  axis 2: out[0] = pb_gradient_planes_half for n x other.
extern "C" int pb_debug_line_choice(int axis, int n, int other, int P, const int *use, int *out) {
    if (axis < 0 || axis > 2 || n < 2 || other < 2 || P < 1 || !use || !out) return PB_ERR_BADARG;
    pb_ctx ctx;
    pb_read_knobs(&ctx);
    if (axis == 2) { out[0] = pb_gradient_planes_half(&ctx, n, other) ? 1 : 0; return PB_OK; }
    const LineUse u{use[0], use[1], use[2], use[3], use[4], use[5], use[6]};
    const LineChoice c = axis == 0 ? choose_rows(ctx.host_plans, ctx.line, n, other, P, u) : choose_cols(ctx.host_plans, ctx.line, n, other, P, u);
    const int head[13] = {c.kind, c.taken, c.threads, c.lognb, c.tiles, c.lds, c.max_radix, c.sat, c.half_ok, c.ext, c.first, c.plan.bluestein_m, c.plan.nstage};
    std::copy(head, head + 13, out);
    std::copy(c.plan.radix, c.plan.radix + 24, out + 13);
    return PB_OK;
}

// What the domain-transform filter would run for one call on B images of C (1 or 3) channels, H x W samples of elem (4 or 2)
// bytes (dt_choice.h: choose_dt); host only, no device needed.  self_guided: the joint image is the input itself; aligned16: the
// joint image and the output lie on 16-byte boundaries.  knobs: PB_DT_ROWS_REG, PB_DT_COLS_STRIP, PB_DT_COLS_COOP as three ints
// -- the choice of an engine built under those --, or null: as pb_create reads the environment.  out (7): the row form of the
// first iteration, its chunks, the column form, its strip / block rows, the floats of "dt.carry" and "dt.weights", dynamic LDS.
extern "C" int pb_debug_dt_choice(int elem, int C, int B, int H, int W, int self_guided, int aligned16, const int *knobs, long long *out) {
    if ((elem != 4 && elem != 2) || (C != 1 && C != 3) || B < 1 || H < 1 || W < 1 || !out) return PB_ERR_BADARG;
    pb_ctx ctx;
    pb_read_knobs(&ctx);
    const DtKnobs k = knobs ? DtKnobs{knobs[0], knobs[1], knobs[2]} : ctx.dt;
    const DtChoice c = choose_dt(k, elem, C, B, H, W, self_guided != 0, aligned16 != 0);
    const long long v[7] = {c.rows, c.chunks, c.cols, c.cols_rows, c.carry, c.weights, c.lds};
    std::copy(v, v + 7, out);
    return PB_OK;
}

// What a reblurring call would issue (poly_choice.h); host only, no device and no context needed.  polynomial: 1 = choose_poly (the
// three Horner steps), 0 = choose_pass (one pass, step 0 of the per-step facts).  facts: PolyFacts as PB_POLY_NFACTS ints, in the
// order of the struct.  out: up to max_ops ops of 8 ints each -- kind, step, poly, ring, side stream, known selections, spectra
// set, arg (PolyOp).  Returns the number of ops, or PB_ERR_BADARG (a plan longer than max_ops or than PB_POLY_MAX_OPS included).
extern "C" int pb_debug_poly_plan(int polynomial, const int *facts, int n_facts, int *out, int max_ops) {
    if (!facts || n_facts != PB_POLY_NFACTS || !out || max_ops < 0) return PB_ERR_BADARG;
    PolyFacts f;
    memcpy(&f, facts, sizeof(f));
    if (f.ring < 0 || f.ring > 5 || f.poly < 0 || f.poly > 2) return PB_ERR_BADARG;
    const PolyPlan pl = polynomial ? choose_poly(f) : choose_pass(f);
    if (pl.overflow || pl.n > max_ops) return PB_ERR_BADARG;
    for (int i = 0; i < pl.n; ++i) {
        const PolyOp &o = pl.op[i];
        const int v[PB_POLY_OP_INTS] = {o.kind, o.step, o.poly, o.ring, o.side, o.known, o.set, o.arg};
        std::copy(v, v + PB_POLY_OP_INTS, out + i * PB_POLY_OP_INTS);
    }
    return pl.n;
}

extern "C" {

int pb_version(void) { return PB_VERSION; }

void pb_default_options(pb_options *o) {
    // deblurring.py:23-25
    memset(o, 0, sizeof(*o));
    o->n_iter = 1; o->c = 0.352f; o->b = 0.768f; o->alpha = 2.f; o->beta = 3.f;
    o->sigma_r = 0.8f; o->sigma_s = 2.0f; o->q = 0.f; o->n_angles = 6; o->n_interpolated_angles = 30;
    o->remove_halo = 0; o->edgetaping = 0; o->prefilter = PB_PREFILTER_NONE; o->discard_saturation = 0;
    o->boundary = PB_WRAP; o->support = PB_SUPPORT_FULL; o->force_theta_deg = -1.f; o->ker_size = PB_KSIZE;
}

int pb_create(pb_ctx **out, int device, void *stream) {
    if (!out) return PB_ERR_BADARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0 || device < 0 || device >= n) return PB_ERR_HIP;
    if (hipSetDevice(device) != hipSuccess) return PB_ERR_HIP;
    pb_ctx *ctx = new pb_ctx();
    ctx->device = device;
    ctx->stream = static_cast<hipStream_t>(stream);
    pb_read_knobs(ctx);
    if (hipEventCreate(&ctx->ev0) != hipSuccess || hipEventCreate(&ctx->ev1) != hipSuccess ||
        hipEventCreateWithFlags(&ctx->ev_switch, hipEventDisableTiming) != hipSuccess) { delete ctx; return PB_ERR_HIP; }
    {
        if (hipStreamCreateWithFlags(&ctx->aux, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&ctx->ev_join, hipEventDisableTiming) != hipSuccess) {
            (void)hipGetLastError();
            if (ctx->aux) (void)hipStreamDestroy(ctx->aux);
            ctx->aux = nullptr;                                  // (the engine works without it)
        }
    }
    *out = ctx;
    return PB_OK;
}

int pb_set_dense_eval(pb_ctx *ctx, int mode, int min_phases) {
    if (!ctx || (mode != PB_DENSE_STENCIL && mode != PB_DENSE_AUTO) || min_phases < 0 || min_phases > PB_MAX_PHASES + 1)
        return PB_ERR_BADARG;
    ctx->fft_min_phases = mode == PB_DENSE_STENCIL ? -1 : min_phases;
    pb_forget_hints(ctx);                                 // (which bodies the cached records take has changed; flip_sets have not)
    return PB_OK;
}

int pb_set_phase_budget(pb_ctx *ctx, size_t bytes) {
    if (!ctx) return PB_ERR_BADARG;
    ctx->phase_budget = bytes;
    return PB_OK;
}

int pb_destroy(pb_ctx *ctx) {
    if (!ctx) return PB_OK;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &kv : ctx->scratch) if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto &kv : ctx->plans) {
        FftPlan &p = kv.second;
        if (p.tw) (void)hipFree(p.tw);
        if (p.drev) (void)hipFree(p.drev);
        if (p.chirp) (void)hipFree(p.chirp);
        if (p.bfilt_rev) (void)hipFree(p.bfilt_rev);
        if (p.dnat) (void)hipFree(p.dnat);
    }
    if (ctx->interp_w) (void)hipFree(ctx->interp_w);
    for (auto &r : ctx->prof) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto e : ctx->evpool) (void)hipEventDestroy(e);
    if (ctx->ev0) (void)hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void)hipEventDestroy(ctx->ev1);
    if (ctx->ev_switch) (void)hipEventDestroy(ctx->ev_switch);
    if (ctx->aux) { (void)hipStreamSynchronize(ctx->aux); (void)hipStreamDestroy(ctx->aux); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_join) (void)hipEventDestroy(ctx->ev_join);
    delete ctx;
    return PB_OK;
}

int pb_set_stream(pb_ctx *ctx, void *stream) {
    if (!ctx) return PB_ERR_BADARG;
    hipStream_t next = static_cast<hipStream_t>(stream);
    if (next != ctx->stream) {
        // the context's scratch buffers may still be in use by work queued on the old stream: order the new
        // stream behind it (device-side dependency, no host wait)
        PB_HIP(hipSetDevice(ctx->device));
        if (hipEventRecord(ctx->ev_switch, ctx->stream) != hipSuccess || hipStreamWaitEvent(next, ctx->ev_switch, 0) != hipSuccess) {
            // (the old stream may have been destroyed by its owner: nothing can be ordered behind it any more -- wait
            // for the device instead and adopt the new stream all the same)
            (void)hipGetLastError();
            PB_HIP(hipDeviceSynchronize());
        }
        ctx->stream = next;
    }
    return PB_OK;
}

int pb_synchronize(pb_ctx *ctx) {
    if (!ctx) return PB_ERR_BADARG;
    PB_HIP(hipStreamSynchronize(ctx->stream));
    return PB_OK;
}

const char *pb_last_error_string(pb_ctx *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

size_t pb_workspace_bytes(pb_ctx *ctx) {
    size_t t = 0;
    if (ctx) for (auto &kv : ctx->scratch) t += kv.second.bytes;
    return t;
}

int pb_malloc(pb_ctx *ctx, void **dptr, size_t bytes) {
    if (!ctx || !dptr) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    if (hipMalloc(dptr, bytes ? bytes : 1) != hipSuccess) return pb_fail(ctx, PB_ERR_NOMEM, "pb_malloc(%zu) failed", bytes);
    return PB_OK;
}
int pb_free(pb_ctx *ctx, void *dptr) {
    if (!ctx) return PB_ERR_BADARG;
    // what the context has cached about records is a hint and goes wholesale; which caller-supplied record sets hold taps that
    // are not point-symmetric is not (common.h: FlipSet): only the sets inside the allocation being freed are dropped
    pb_forget_hints(ctx);
    hipDeviceptr_t base = nullptr; size_t size = 0;
    if (dptr && hipMemGetAddressRange(&base, &size, dptr) == hipSuccess) pb_forget_range(ctx, base, size);
    else {
        (void)hipGetLastError();
        ctx->flip_sets.erase(dptr);
    }
    PB_HIP(hipStreamSynchronize(ctx->stream));
    PB_HIP(hipFree(dptr));
    return PB_OK;
}
int pb_memcpy_h2d(pb_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return PB_ERR_BADARG;
    pb_forget_range(ctx, dst, bytes);                     // (the copy may overwrite records the context has cached facts about)
    PB_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    PB_HIP(hipStreamSynchronize(ctx->stream));
    return PB_OK;
}
int pb_memcpy_d2h(pb_ctx *ctx, void *dst, const void *src, size_t bytes) {
    if (!ctx) return PB_ERR_BADARG;
    PB_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    PB_HIP(hipStreamSynchronize(ctx->stream));
    return PB_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// inverse filtering (deblurring.py:211-239)
// ---------------------------------------------------------------------------------------------
namespace {

struct Geometry {
    int B, C, H, W, P, pad, Hp, Wp, pp;     // pad = ker_size / 2; pp = pitch of padded fp32 planes
    long pplane;                        // elements per padded plane
    long HW;
    // method='direct_separable': records of the two 1-D passes that stand in for every reblurring, and the plane between them
    const pb_blur_info *sep1 = nullptr, *sep2 = nullptr;
    float *sep_u = nullptr;
    // pb_options.half_temporaries: the two Horner temporaries are stored as fp16 (fp32 accumulation, fp32 x operand)
    void *t1h = nullptr, *t2h = nullptr;
    // ker_size above 25: the taps on the ker_size grid (conv_big.hip), rebuilt after every estimation; a caller's kernel set
    // beyond the 25 x 25 record (pb_taps): its table for the call's boundary
    BigTaps big;
    // the polynomial is the one with the pure-phase filter (conv_phase.hip): the caller's raw kh x kw taps, one kernel per image
    const float *phase_taps = nullptr;
    int phase_kh = 0, phase_kw = 0;
};

Geometry geometry(int B, int C, int H, int W, int pad = PB_KRAD) {
    Geometry g;
    g.B = B; g.C = C; g.H = H; g.W = W; g.P = B * C; g.pad = pad;
    g.Hp = H + 2 * pad; g.Wp = W + 2 * pad; g.pp = pitch4(g.Wp);
    g.pplane = (long)g.Hp * g.pp;
    g.HW = (long)H * W;
    return g;
}

ConvPass base_pass(const Geometry &g, const pb_blur_info *info, int boundary) {
    ConvPass p;
    memset(&p, 0, sizeof(p));
    p.H = g.H; p.W = g.W; p.pad = g.pad; p.C = g.C; p.P = g.P; p.info = info; p.boundary = boundary;
    p.scale = 1.f; p.coef = 0.f; p.epilogue = EPI_HORNER; p.clamp01 = 0;
    return p;
}
void set_in_virtual(ConvPass &p, const Geometry &g, const void *ptr, int dtype) {
    p.in = ptr; p.in_kind = SRC_VIRTUAL; p.in_dtype = dtype; p.in_pitch = g.W; p.in_plane = g.HW;
}
void set_in_padded(ConvPass &p, const Geometry &g, const void *ptr, int dtype = PB_F32) {
    p.in = ptr; p.in_kind = SRC_PADDED; p.in_dtype = dtype; p.in_pitch = g.pp; p.in_plane = g.pplane;
}
void set_x_virtual(ConvPass &p, const Geometry &g, const void *ptr, int dtype) {
    p.x = ptr; p.x_kind = SRC_VIRTUAL; p.x_dtype = dtype; p.x_pitch = g.W; p.x_plane = g.HW;
}
void set_x_padded(ConvPass &p, const Geometry &g, const float *ptr) {
    p.x = ptr; p.x_kind = SRC_PADDED; p.x_dtype = PB_F32; p.x_pitch = g.pp; p.x_plane = g.pplane;
}
void set_out_padded(ConvPass &p, const Geometry &g, void *ptr, int dtype = PB_F32) {
    p.out = ptr; p.out_kind = OUT_PADDED; p.out_dtype = dtype; p.out_pitch = g.pp; p.out_plane = g.pplane;
}
void set_out_interior(ConvPass &p, const Geometry &g, void *ptr, int dtype) {
    p.out = ptr; p.out_kind = OUT_INTERIOR; p.out_dtype = dtype; p.out_pitch = g.W; p.out_plane = g.HW;
}

// the kernels' own spectra, every kernel on the window form of a single pass (PolySpec.always == 2)
PolySpec window_form_spec() {
    PolySpec ps = no_poly();
    ps.always = 2;
    return ps;
}

// What one iteration of the pipeline asks of the spectra it builds and meets: worked out ONCE, in front of the estimation
// (pb_polyblur_batch), and handed to the estimation, the edgetaper's blends and the polynomial alike -- the estimation ends with
// exactly the spectra the passes behind it ask for.  A stage entry point has no plan: its blends are plain passes, its
// polynomial works its spec out itself (poly_spec), and every selection goes to slot 0.
struct IterPlan {
    int slot = 0;                                    // this iteration's slot of the selection scratch (pb_body_selection)
    PolySpec blends = no_poly();                     // the edgetaper's three blends
    PolySpec poly = no_poly();                       // the polynomial
    PolySpec est1 = no_poly(), est2 = no_poly();     // what the estimation builds into the first / the second set (est2 all zero: no second set)
};

// Three edgetaper blends on the padded domain (edgetaper.py:26-33).  src is an un-padded image
// (virtual replicate pad).  Returns the padded fp32 result in *result (one of the two scratch planes).
// want.spec: no_poly(), or window_form_spec() where the estimation built these records' spectra under it (one launch per blend)
int run_edgetaper(pb_ctx *ctx, const Geometry &g, const void *src, int src_dtype, const pb_blur_info *info, int boundary,
                  float *pa, float *pb, float **result, const PassWant &want) {
    ConvPass p = base_pass(g, info, boundary);
    p.epilogue = EPI_TAPER;
    set_in_virtual(p, g, src, src_dtype);
    set_x_virtual(p, g, src, src_dtype);
    set_out_padded(p, g, pa);
    if (g.big.taps) {
        // (a kernel beyond the 25 x 25 record: the three blends through conv_big.hip's pass, weights from its own autocorrelations)
        int rcb = pb_launch_conv_big(ctx, p, g.big);
        if (rcb) return rcb;
        set_in_padded(p, g, pa); set_x_padded(p, g, pa); set_out_padded(p, g, pb);
        rcb = pb_launch_conv_big(ctx, p, g.big);
        if (rcb) return rcb;
        set_in_padded(p, g, pb); set_x_padded(p, g, pb); set_out_padded(p, g, pa);
        rcb = pb_launch_conv_big(ctx, p, g.big);
        *result = pa;
        return rcb;
    }
    int rc = pb_launch_conv(ctx, p, want);
    if (rc) return rc;
    // (window form for every image: the second and the third blend only touch the ring of window pairs on which alpha < 1
    // can reach them -- the rest of `pa` keeps the first blend's copy of the image, which is what three blends with alpha = 1
    // leave there; `pb` is only ever read inside the second blend's ring)
    const bool rings = want.spec.always == 2 && ctx->taper_ring;
    set_in_padded(p, g, pa); set_x_padded(p, g, pa); set_out_padded(p, g, pb);
    p.ring = rings ? 5 : 0;
    rc = pb_launch_conv(ctx, p, want);
    if (rc) return rc;
    set_in_padded(p, g, pb); set_x_padded(p, g, pb); set_out_padded(p, g, pa);
    p.ring = rings ? 4 : 0;
    rc = pb_launch_conv(ctx, p, want);
    *result = pa;
    return rc;
}

// The three Horner steps of y = a3 K^3 x + a2 K^2 x + a1 K x + beta x (deblurring.py:122-138).
// x: the un-padded image of x_dtype (virtual pad), or -- x_padded -- a padded fp32 plane (after an edgetaper)
void make_steps(const Geometry &g, const void *x, int x_dtype, bool x_padded, const pb_blur_info *info, float alpha,
                float beta, int boundary, float *t1, float *t2, void *dst, int dst_dtype, int clamp01, ConvPass *steps) {
    const float a3 = alpha / 2 - beta + 2, a2 = 3 * beta - alpha - 6, a1 = 5 - 3 * beta + alpha / 2;
    ConvPass p = base_pass(g, info, boundary);
    auto set_x = [&](ConvPass &q) { if (x_padded) set_x_padded(q, g, static_cast<const float *>(x)); else set_x_virtual(q, g, x, x_dtype); };
    const int tdt = g.t1h ? PB_F16 : PB_F32;
    void *T1 = g.t1h ? g.t1h : static_cast<void *>(t1), *T2 = g.t2h ? g.t2h : static_cast<void *>(t2);
    // t1 = K * (a3 x) + a2 x
    if (x_padded) set_in_padded(p, g, x); else set_in_virtual(p, g, x, x_dtype);
    set_x(p); set_out_padded(p, g, T1, tdt);
    p.scale = a3; p.coef = a2;
    steps[0] = p;
    // t2 = K * t1 + a1 x
    set_in_padded(p, g, T1, tdt); set_out_padded(p, g, T2, tdt);
    p.scale = 1.f; p.coef = a1;
    steps[1] = p;
    // y = K * t2 + beta x   (only the crop is needed)
    set_in_padded(p, g, T2, tdt); set_out_interior(p, g, dst, dst_dtype);
    p.coef = beta; p.clamp01 = clamp01;
    steps[2] = p;
}

// What the spectra of a polynomial should be those of (PolySpec; conv.hip: pb_poly_spec_mode).  A function of the context's
// knobs and of the sizes, kinds and types of the three steps -- never of their planes or records, so the steps are laid out over
// none: the pipeline asks in front of the estimation, a stage entry point in front of its polynomial, and both get one answer.
// x_dtype, x_padded, dst_dtype: as make_steps.
// gaussians: the records are (or will be) point-symmetric Gaussians the estimation itself builds on an odd ker_size grid
PolySpec poly_spec(pb_ctx *ctx, const Geometry &g, int x_dtype, bool x_padded, int boundary, int dst_dtype, float alpha, float beta,
                   bool gaussians) {
    ConvPass steps[3];
    make_steps(g, nullptr, x_dtype, x_padded, nullptr, alpha, beta, boundary, nullptr, nullptr, nullptr, dst_dtype, 0, steps);
    const int mode = pb_poly_spec_mode(ctx, steps);
    if (!mode) {
        // (the zero boundary on an image too small for the ring form, the estimation's own Gaussians: every kernel on three
        // window steps -- a fact of the call again, so the polynomial issues the wave body's three launches and nothing else)
        if (boundary == PB_ZERO && gaussians && ctx->poly_always && pb_poly_three_steps_ok(ctx, steps)) return window_form_spec();
        return no_poly();
    }
    // (every composite of a 25-tap kernel fits a 128 x 128 window -- halo <= 36, tile >= 56 -- so where those windows are admitted
    // and every kernel is the estimation's own Gaussian, "every image takes one window pass" is a fact of the call's options and
    // sizes: PolySpec.always, and pb_launch_conv_poly issues the two window launches only)
    const int always = (mode == 3 && gaussians && ctx->poly_always) ? 1 : 0;
    // (under the zero boundary only that class takes one pass: interior by the window pass, frame by three ring steps)
    if (steps[0].boundary != PB_WRAP && !always) return no_poly();
    // (windows 64 wide and 128 tall, conv_wfft.hip: the composite pass from an un-tapered fp32 image to an fp32 plane under the
    // wrap boundary, an image at least one such window tall -- facts of the call, PolySpec.tall; that the taps are point-symmetric
    // -- an odd ker_size grid -- is what every one-pass form asks of a record, khat.h)
    const ConvPass &f = steps[0], &l = steps[2];
    const bool tall_ok = mode >= 2 && f.boundary == PB_WRAP && f.in_dtype == PB_F32 && f.x_dtype == PB_F32 && l.out_dtype == PB_F32 &&
                         f.in_kind == SRC_VIRTUAL && f.epilogue == EPI_HORNER && f.H >= 128;
    const int tall = tall_ok ? std::min(std::max(ctx->poly_tall, 0), 2) : 0;
    return PolySpec{mode, alpha / 2 - beta + 2, 3 * beta - alpha - 6, 5 - 3 * beta + alpha / 2, beta, PB_POLY_GAIN, PB_POLY_MIN_AREA, PB_POLY_COST128, always,
                    tall, PB_POLY_COST_TALL};
}

// y = a3 K^3 x + a2 K^2 x + a1 K x + beta x by Horner, three stencil passes (deblurring.py:122-138).
// X is either the un-padded image (virtual pad) or a padded fp32 image (after edgetaper).
// plan: the pipeline's plan of this iteration; nullptr (a stage entry point): slot 0, and the polynomial's spec from poly_spec
// here -- for records the call did not estimate itself, so nothing vouches for Gaussians
int run_polynomial(pb_ctx *ctx, const Geometry &g, const void *xsrc, int x_dtype, const float *xpadded,
                   const pb_blur_info *info, float alpha, float beta, int boundary, float *t1, float *t2, void *dst,
                   int dst_dtype, int clamp01, const IterPlan *plan = nullptr) {
    const float a3 = alpha / 2 - beta + 2, a2 = 3 * beta - alpha - 6, a1 = 5 - 3 * beta + alpha / 2;
    const PassWant plain{no_poly(), plan ? plan->slot : 0};
    if (g.sep1) {
        // K ~= K2 after K1 (estimate.hip: sep_records_kernel).  One launch per step keeps u = K1 * t in LDS (conv_xt.hip, the
        // --experimental build); where it is not built -- the default build, 8-bit images -- two launches through the sparse
        // phase lists of the general body: u = K1 * t, then t' = scale (K2 * u) + coef x
        const float scale[3] = {a3, 1.f, 1.f}, coef[3] = {a2, a1, beta};
        float *tmp[2] = {t1, t2};
        ConvPass p1 = base_pass(g, g.sep1, boundary), p2 = base_pass(g, g.sep2, boundary);
        set_x_virtual(p1, g, xsrc, x_dtype); set_out_padded(p1, g, g.sep_u);          // coef = 0: x is not used
        set_x_virtual(p2, g, xsrc, x_dtype);
        for (int step = 0; step < 3; ++step) {
            if (step < 2) set_out_padded(p2, g, tmp[step]); else set_out_interior(p2, g, dst, dst_dtype);
            p2.scale = scale[step]; p2.coef = coef[step]; p2.clamp01 = step == 2 ? clamp01 : 0;
            if (step == 0) set_in_virtual(p2, g, xsrc, x_dtype); else set_in_padded(p2, g, tmp[step - 1]);
            int rc = pb_launch_conv_xt(ctx, p2);
            if (rc != PB_OK && rc != PB_ERR_UNSUPPORTED) return rc;
            if (rc == PB_OK) {
                // images whose exact kernel is rank-1 were skipped there: the exact separable body does them
                ConvPass pe = p2;
                pe.info = info; pe.skip_general = 1;
                rc = pb_launch_conv(ctx, pe, plain);
                if (rc) return rc;
            }
            if (rc == PB_ERR_UNSUPPORTED) {
                if (step == 0) set_in_virtual(p1, g, xsrc, x_dtype); else set_in_padded(p1, g, tmp[step - 1]);
                rc = pb_launch_conv(ctx, p1, plain);
                if (rc) return rc;
                set_in_padded(p2, g, g.sep_u);
                rc = pb_launch_conv(ctx, p2, plain);
                if (rc) return rc;
            }
        }
        return PB_OK;
    }
    ConvPass steps[3];
    make_steps(g, xpadded ? xpadded : xsrc, x_dtype, xpadded != nullptr, info, alpha, beta, boundary, t1, t2, dst, dst_dtype, clamp01, steps);
    if (g.big.taps) {
        for (int s = 0; s < 3; ++s) {
            const int rc = pb_launch_conv_big(ctx, steps[s], g.big);
            if (rc) return rc;
        }
        return PB_OK;
    }
    // (under the wrap boundary the three steps are one filter, deblurring.py:139-169: images for which one window pass
    // with that filter's spectrum is the cheaper form take it, pb_fft_sel.poly; the spectra are then the polynomial's)
    const PolySpec spec = plan ? plan->poly : poly_spec(ctx, g, x_dtype, xpadded != nullptr, boundary, dst_dtype, alpha, beta, false);
    return pb_launch_conv_poly(ctx, steps, PassWant{spec, plain.slot});
}

// The same polynomial with the pure-phase filter in front (deblurring.py:141-169 with not_symmetric=True): one transform over
// the padded domain (conv_phase.hip) in the place of the three reblurring passes.
int run_phase_polynomial(pb_ctx *ctx, const Geometry &g, const void *xsrc, int x_dtype, const float *xpadded, float alpha,
                         float beta, void *dst, int dst_dtype, int clamp01) {
    PhaseCall c;
    if (xpadded) { c.src = xpadded; c.src_dtype = PB_F32; c.src_virtual = 0; c.src_pitch = g.pp; c.src_plane = g.pplane; }
    else { c.src = xsrc; c.src_dtype = x_dtype; c.src_virtual = 1; c.src_pitch = g.W; c.src_plane = g.HW; }
    c.dst = dst; c.dst_dtype = dst_dtype; c.clamp01 = clamp01;
    c.B = g.B; c.C = g.C; c.H = g.H; c.W = g.W; c.pad = g.pad;
    c.taps = g.phase_taps; c.kh = g.phase_kh; c.kw = g.phase_kw;
    c.alpha = alpha; c.beta = beta;
    return pb_launch_phase(ctx, c);
}

struct InverseScratch {
    float *t1, *t2, *y, *ox, *nM;
};

// src: what gets deconvolved (cur, or the smooth component).  dst: (B,C,H,W) of dst_dtype.
int inverse_filter(pb_ctx *ctx, const Geometry &g, const void *src, int src_dtype, void *dst, int dst_dtype,
                   const pb_blur_info *info, float alpha, float beta, int boundary, int edgetaping, int remove_halo,
                   const void *g0x, const void *g0y, const float *nM, int final_clamp,
                   const void *recomb_cur = nullptr, int recomb_cur_dtype = 0, const float *recomb_smooth = nullptr,
                   int g_dtype = PB_F32, const IterPlan *plan = nullptr) {
    // recomb_cur (only with remove_halo): the halo kernel also adds back the detail layer cur - recomb_smooth
    // plan: the pipeline's plan of this iteration (nullptr: a stage entry point -- see run_polynomial)
    float *t1 = nullptr, *t2 = nullptr;
    if (!g.t1h && !(g.phase_taps && !edgetaping)) {     // (the phase polynomial has scratch of its own; the edgetaper in front of it borrows t1)
        t1 = static_cast<float *>(pb_scratch(ctx, "inv.t1", sizeof(float) * g.P * g.pplane));
        t2 = static_cast<float *>(pb_scratch(ctx, "inv.t2", sizeof(float) * g.P * g.pplane));
        if (!t1 || !t2) return PB_ERR_NOMEM;
    }
    const float *xpadded = nullptr;
    if (edgetaping) {
        float *pa = static_cast<float *>(pb_scratch(ctx, "inv.pa", sizeof(float) * g.P * g.pplane));
        if (!pa) return PB_ERR_NOMEM;
        float *res = nullptr;
        const PassWant blends = plan ? PassWant{plan->blends, plan->slot} : PassWant();
        int rc = run_edgetaper(ctx, g, src, src_dtype, info, boundary, pa, t1, &res, blends);   // t1 is free until the polynomial
        if (rc) return rc;
        xpadded = res;
    }
    if (!remove_halo)
        return g.phase_taps ? run_phase_polynomial(ctx, g, src, src_dtype, xpadded, alpha, beta, dst, dst_dtype, final_clamp)
                            : run_polynomial(ctx, g, src, src_dtype, xpadded, info, alpha, beta, boundary, t1, t2, dst, dst_dtype,
                                             final_clamp, plan);
    float *y = static_cast<float *>(pb_scratch(ctx, "inv.y", sizeof(float) * g.P * g.HW));
    if (!y) return PB_ERR_NOMEM;
    int rc = g.phase_taps ? run_phase_polynomial(ctx, g, src, src_dtype, xpadded, alpha, beta, y, PB_F32, 0)
                          : run_polynomial(ctx, g, src, src_dtype, xpadded, info, alpha, beta, boundary, t1, t2, y, PB_F32, 0, plan);
    if (rc) return rc;
    if (!g0x) {
        // grad_img=None (deblurring.py:200-201): the gradients of the image the halo mask blends with -- the crop of the
        // padded plane, AFTER the edgetaper where there is one (:237)
        float *x32 = static_cast<float *>(pb_scratch(ctx, "inv.x32", sizeof(float) * g.P * g.HW));
        float *gx = static_cast<float *>(pb_scratch(ctx, "inv.g0x", sizeof(float) * g.P * g.HW));
        float *gy = static_cast<float *>(pb_scratch(ctx, "inv.g0y", sizeof(float) * g.P * g.HW));
        float *e = static_cast<float *>(pb_scratch(ctx, "inv.nM", sizeof(float) * g.P));
        if (!x32 || !gx || !gy || !e) return PB_ERR_NOMEM;
        if (xpadded) {
            for (int pl = 0; pl < g.P; ++pl)
                PB_HIP(hipMemcpy2DAsync(x32 + pl * g.HW, sizeof(float) * g.W, xpadded + pl * g.pplane + (long)g.pad * g.pp + g.pad,
                                        sizeof(float) * g.pp, sizeof(float) * g.W, g.H, hipMemcpyDeviceToDevice, ctx->stream));
        } else if (src_dtype != PB_F32) {
            rc = pb_convert_to_float(ctx, src, src_dtype, x32, g.P * g.HW);
            if (rc) return rc;
        }
        rc = pb_fourier_gradients_impl(ctx, (xpadded || src_dtype != PB_F32) ? x32 : static_cast<const float *>(src), g.P, g.H, g.W, gx, gy);
        if (rc) return rc;
        rc = pb_grad_energy(ctx, gx, gy, e, g.P, g.HW);
        if (rc) return rc;
        g0x = gx; g0y = gy; nM = e; g_dtype = PB_F32;
    }
    void *ox = pb_scratch(ctx, "inv.ox", dsize(g_dtype) * g.P * g.HW);    // (in the type of grad_img's planes)
    if (!ox) return PB_ERR_NOMEM;
    rc = pb_fourier_gradients_typed(ctx, y, g.P, g.H, g.W, ox, nullptr, g_dtype);     // only gout_x is used (deblurring.py:174)
    if (rc) return rc;
    if (xpadded)
        return pb_halo_apply(ctx, xpadded + (long)g.pad * g.pp + g.pad, PB_F32, g.pp, g.pplane, y, g0x, g0y, ox, nM, dst,
                             dst_dtype, g.P, g.H, g.W, final_clamp, recomb_cur, recomb_cur_dtype, recomb_smooth, g_dtype);
    return pb_halo_apply(ctx, src, src_dtype, g.W, g.HW, y, g0x, g0y, ox, nM, dst, dst_dtype, g.P, g.H, g.W, final_clamp,
                         recomb_cur, recomb_cur_dtype, recomb_smooth, g_dtype);
}

int check_shape(pb_ctx *ctx, int dtype, int B, int C, int H, int W, int allow_u8 = 0) {
    if (!ctx) return PB_ERR_BADARG;
    if (dtype != PB_F32 && dtype != PB_F16 && !(allow_u8 && dtype == PB_U8))
        return pb_fail(ctx, PB_ERR_BADARG, allow_u8 ? "dtype must be PB_F32, PB_F16 or PB_U8" : "dtype must be PB_F32 or PB_F16");
    if (B < 1 || C < 1 || H < 2 || W < 2) return pb_fail(ctx, PB_ERR_BADARG, "bad shape (%d,%d,%d,%d)", B, C, H, W);
    return PB_OK;
}

}  // namespace

extern "C" {

int pb_estimate_blur(pb_ctx *ctx, const void *in, int dtype, int B, int C, int H, int W, const pb_options *opt,
                     pb_blur_info *dev_info) {
    int rc = check_shape(ctx, dtype, B, C, H, W, 1);
    if (rc) return rc;
    if (!in || !opt || !dev_info) return pb_fail(ctx, PB_ERR_BADARG, "null argument");
    PB_HIP(hipSetDevice(ctx->device));
    pb_forget_records(ctx, dev_info, B);
    return pb_estimate_impl(ctx, in, dtype, B, C, H, W, opt, dev_info, no_poly(), no_poly(), 0);
}

int pb_make_kernels(pb_ctx *ctx, int B, const float *host_sigma, const float *host_rho, const float *host_theta_rad,
                    int support, pb_blur_info *dev_info) {
    if (!ctx || B < 1 || !host_sigma || !host_rho || !host_theta_rad || !dev_info) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    std::vector<pb_blur_info> h(B);
    memset(h.data(), 0, sizeof(pb_blur_info) * B);
    for (int i = 0; i < B; ++i) { h[i].sigma = host_sigma[i]; h[i].rho = host_rho[i]; h[i].theta = host_theta_rad[i]; }
    PB_HIP(hipMemcpyAsync(dev_info, h.data(), sizeof(pb_blur_info) * B, hipMemcpyHostToDevice, ctx->stream));
    PB_HIP(hipStreamSynchronize(ctx->stream));
    const int rc = pb_make_kernels_dev(ctx, B, dev_info, support, 0);
    return rc ? rc : pb_cache_records(ctx, dev_info, B);
}

int pb_make_separable_kernels(pb_ctx *ctx, int B, const pb_blur_info *dev_info, pb_blur_info *dev_sep, int support,
                              int ker_size) {
    if (!ctx || B < 1 || !dev_info || !dev_sep) return PB_ERR_BADARG;
    pb_options o;
    pb_default_options(&o);
    o.ker_size = ker_size;
    const int ksize = pb_kernel_size(&o);
    if (!ksize || ksize > PB_KSIZE || !(ksize & 1))
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "ker_size %d: the separable approximation is built for odd sizes from 3 to %d (an even size is the reference's off-centre grid, filters.py:78: not built)", ker_size, PB_KSIZE);
    PB_HIP(hipSetDevice(ctx->device));
    pb_forget_records(ctx, dev_sep, 2 * B);
    return pb_make_sep_records(ctx, B, dev_info, dev_sep, support, ksize);
}

int pb_set_kernels(pb_ctx *ctx, int B, const float *host_taps, int support, pb_blur_info *dev_info) {
    if (!ctx || B < 1 || !host_taps || !dev_info) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    std::vector<pb_blur_info> h(B);
    memset(h.data(), 0, sizeof(pb_blur_info) * B);
    for (int i = 0; i < B; ++i) memcpy(h[i].kernel, host_taps + (size_t)i * PB_KSIZE * PB_KSIZE, sizeof(float) * PB_KSIZE * PB_KSIZE);
    PB_HIP(hipMemcpyAsync(dev_info, h.data(), sizeof(pb_blur_info) * B, hipMemcpyHostToDevice, ctx->stream));
    PB_HIP(hipStreamSynchronize(ctx->stream));
    int rc = pb_make_kernels_dev(ctx, B, dev_info, support, 1);
    if (!rc) rc = pb_cache_records(ctx, dev_info, B);             // (forgets what was known about these records, flip set included)
    if (rc) return rc;
    // taps that are not point-symmetric: keep their reflection for the wrap boundary's passes (common.h: FlipSet)
    bool asym = false;
    for (int i = 0; i < B && !asym; ++i) {
        const float *k = host_taps + (size_t)i * PB_KSIZE * PB_KSIZE;
        for (int e = 0; e < PB_KSIZE * PB_KSIZE / 2 && !asym; ++e) asym = k[e] != k[PB_KSIZE * PB_KSIZE - 1 - e];
    }
    if (asym) {
        pb_ctx::FlipSet f;
        f.B = B; f.support = support;
        f.taps.resize((size_t)B * PB_KSIZE * PB_KSIZE);
        for (int i = 0; i < B; ++i)
            for (int e = 0; e < PB_KSIZE * PB_KSIZE; ++e)
                f.taps[(size_t)i * PB_KSIZE * PB_KSIZE + e] = host_taps[(size_t)i * PB_KSIZE * PB_KSIZE + (PB_KSIZE * PB_KSIZE - 1 - e)];
        ctx->flip_sets[dev_info] = std::move(f);
    }
    return PB_OK;
}

// The records a wrap-boundary pass runs with: the caller's, or -- caller-supplied taps that are not point-symmetric -- a copy built
// from the reflected taps (the reference's method='fft' convolves, filters.py:33-36; the records hold correlation taps).
static int wrap_records(pb_ctx *ctx, const pb_blur_info *dev_info, int B, int boundary, const pb_blur_info **use) {
    *use = dev_info;
    if (boundary != PB_WRAP) return PB_OK;
    const auto it = ctx->flip_sets.find(dev_info);
    if (it == ctx->flip_sets.end() || it->second.B < B) return PB_OK;
    pb_blur_info *flipped = static_cast<pb_blur_info *>(pb_scratch(ctx, "conv.flipinfo", sizeof(pb_blur_info) * (size_t)B));
    if (!flipped) return PB_ERR_NOMEM;
    std::vector<pb_blur_info> h(B);
    memset(h.data(), 0, sizeof(pb_blur_info) * B);
    for (int i = 0; i < B; ++i) memcpy(h[i].kernel, it->second.taps.data() + (size_t)i * PB_KSIZE * PB_KSIZE, sizeof(float) * PB_KSIZE * PB_KSIZE);
    const int support = it->second.support;
    pb_forget_records(ctx, flipped, B);
    PB_HIP(hipMemcpyAsync(flipped, h.data(), sizeof(pb_blur_info) * B, hipMemcpyHostToDevice, ctx->stream));
    PB_HIP(hipStreamSynchronize(ctx->stream));
    int rc = pb_make_kernels_dev(ctx, B, flipped, support, 1);
    if (!rc) rc = pb_cache_records(ctx, flipped, B);
    if (rc) return rc;
    *use = flipped;
    return PB_OK;
}

int pb_fourier_gradients(pb_ctx *ctx, const float *planes, int P, int H, int W, float *gx, float *gy) {
    if (!ctx || !planes) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    return pb_fourier_gradients_impl(ctx, planes, P, H, W, gx, gy);
}

int pb_inverse_filter(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                      const pb_blur_info *dev_info, float alpha, float beta, int boundary, int edgetaping,
                      int remove_halo, const float *grad0_x, const float *grad0_y) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || !dev_info) return pb_fail(ctx, PB_ERR_BADARG, "null argument");
    if (remove_halo && (!grad0_x || !grad0_y)) return pb_fail(ctx, PB_ERR_BADARG, "remove_halo needs grad0_x / grad0_y");
    PB_HIP(hipSetDevice(ctx->device));
    const Geometry g = geometry(B, C, H, W);
    float *nM = nullptr;
    if (remove_halo) {
        nM = static_cast<float *>(pb_scratch(ctx, "inv.nM", sizeof(float) * g.P));
        if (!nM) return PB_ERR_NOMEM;
        rc = pb_grad_energy(ctx, grad0_x, grad0_y, nM, g.P, g.HW);
        if (rc) return rc;
    }
    const pb_blur_info *recs = nullptr;
    rc = wrap_records(ctx, dev_info, B, boundary, &recs);
    if (rc) return rc;
    return inverse_filter(ctx, g, in, dtype, out, dtype, recs, alpha, beta, boundary, edgetaping, remove_halo, grad0_x,
                          grad0_y, nM, 1);
}

int pb_convolve2d(pb_ctx *ctx, const float *in, float *out, int B, int C, int Hp, int Wp, const pb_blur_info *dev_info,
                  int boundary) {
    if (!ctx || !in || !out || !dev_info || Hp <= 2 * PB_KRAD || Wp <= 2 * PB_KRAD) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    // The given image IS the padded domain: address it as a padded source with pitch Wp.
    Geometry g = geometry(B, C, Hp - 2 * PB_KRAD, Wp - 2 * PB_KRAD);
    g.pp = Wp; g.pplane = (long)Hp * Wp;
    const pb_blur_info *recs = nullptr;
    const int rcw = wrap_records(ctx, dev_info, B, boundary, &recs);
    if (rcw) return rcw;
    ConvPass p = base_pass(g, recs, boundary);
    set_in_padded(p, g, in); set_x_padded(p, g, in); set_out_padded(p, g, out);
    p.scale = 1.f; p.coef = 0.f;
    return pb_launch_conv(ctx, p, PassWant());
}

int pb_edgetaper(pb_ctx *ctx, const float *in, float *out, int B, int C, int Hp, int Wp, const pb_blur_info *dev_info,
                 int boundary) {
    if (!ctx || !in || !out || !dev_info || Hp <= 2 * PB_KRAD || Wp <= 2 * PB_KRAD) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    Geometry g = geometry(B, C, Hp - 2 * PB_KRAD, Wp - 2 * PB_KRAD);
    g.pp = Wp; g.pplane = (long)Hp * Wp;
    float *tmp = static_cast<float *>(pb_scratch(ctx, "taper.tmp", sizeof(float) * g.P * g.pplane));
    if (!tmp) return PB_ERR_NOMEM;
    const pb_blur_info *recs = nullptr;
    const int rcw = wrap_records(ctx, dev_info, B, boundary, &recs);
    if (rcw) return rcw;
    ConvPass p = base_pass(g, recs, boundary);
    p.epilogue = EPI_TAPER;
    set_in_padded(p, g, in); set_x_padded(p, g, in); set_out_padded(p, g, out);
    int rc = pb_launch_conv(ctx, p, PassWant());
    if (rc) return rc;
    set_in_padded(p, g, out); set_x_padded(p, g, out); set_out_padded(p, g, tmp);
    rc = pb_launch_conv(ctx, p, PassWant());
    if (rc) return rc;
    set_in_padded(p, g, tmp); set_x_padded(p, g, tmp); set_out_padded(p, g, out);
    return pb_launch_conv(ctx, p, PassWant());
}

int pb_halo_mask(pb_ctx *ctx, const float *x, const float *y, const float *grad0_x, const float *grad0_y, float *out,
                 int B, int C, int H, int W) {
    if (!ctx || !x || !y || !grad0_x || !grad0_y || !out) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    const Geometry g = geometry(B, C, H, W);
    float *nM = static_cast<float *>(pb_scratch(ctx, "inv.nM", sizeof(float) * g.P));
    float *ox = static_cast<float *>(pb_scratch(ctx, "inv.ox", sizeof(float) * g.P * g.HW));
    if (!nM || !ox) return PB_ERR_NOMEM;
    int rc = pb_grad_energy(ctx, grad0_x, grad0_y, nM, g.P, g.HW);
    if (rc) return rc;
    rc = pb_fourier_gradients_impl(ctx, y, g.P, H, W, ox, nullptr);
    if (rc) return rc;
    return pb_halo_apply(ctx, x, PB_F32, W, g.HW, y, grad0_x, grad0_y, ox, nM, out, PB_F32, g.P, H, W, 0);
}

int pb_fourier_gradients_backward(pb_ctx *ctx, const float *grad_gx, const float *grad_gy, int P, int H, int W,
                                  float *grad_planes) {
    if (!ctx) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    return pb_fourier_gradients_backward_impl(ctx, grad_gx, grad_gy, P, H, W, grad_planes);
}

int pb_halo_mask_backward(pb_ctx *ctx, const float *x, const float *y, const float *grad0_x, const float *grad0_y,
                          const float *grad_out, float *grad_x, float *grad_y, float *grad_grad0_x, float *grad_grad0_y,
                          int B, int C, int H, int W) {
    if (!ctx) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    return pb_halo_mask_backward_impl(ctx, x, y, grad0_x, grad0_y, grad_out, grad_x, grad_y, grad_grad0_x, grad_grad0_y, B, C, H, W);
}

int pb_dt_recursive_filter(pb_ctx *ctx, const void *in, const void *joint, void *out, int dtype, int B, int C, int H,
                           int W, float sigma_s, float sigma_r, int num_iterations) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || num_iterations < 1) return pb_fail(ctx, PB_ERR_BADARG, "bad argument");
    PB_HIP(hipSetDevice(ctx->device));
    const long n = (long)B * C * H * W;
    if (dtype == PB_F32) return pb_dt_filter_impl(ctx, in, joint, dtype, static_cast<float *>(out), B, C, H, W, sigma_s, sigma_r, num_iterations);
    float *tmp = static_cast<float *>(pb_scratch(ctx, "dt.out", sizeof(float) * n));
    if (!tmp) return PB_ERR_NOMEM;
    rc = pb_dt_filter_impl(ctx, in, joint, dtype, tmp, B, C, H, W, sigma_s, sigma_r, num_iterations);
    if (rc) return rc;
    return pb_convert_from_float(ctx, tmp, out, dtype, n);
}

int pb_dt_normalized_convolution(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                                 float sigma_s, float sigma_r, int num_iterations) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || num_iterations < 1 || !(sigma_r > 0.f)) return pb_fail(ctx, PB_ERR_BADARG, "bad argument");
    PB_HIP(hipSetDevice(ctx->device));
    const long n = (long)B * C * H * W;
    if (dtype == PB_F32) return pb_nc_filter_impl(ctx, in, dtype, static_cast<float *>(out), B, C, H, W, sigma_s, sigma_r, num_iterations);
    float *tmp = static_cast<float *>(pb_scratch(ctx, "dt.out", sizeof(float) * n));
    if (!tmp) return PB_ERR_NOMEM;
    rc = pb_nc_filter_impl(ctx, in, dtype, tmp, B, C, H, W, sigma_s, sigma_r, num_iterations);
    if (rc) return rc;
    return pb_convert_from_float(ctx, tmp, out, dtype, n);
}

int pb_bilateral5(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!in || !out) return pb_fail(ctx, PB_ERR_BADARG, "null argument");
    PB_HIP(hipSetDevice(ctx->device));
    return pb_bilateral5_impl(ctx, in, dtype, out, dtype, B * C, H, W);
}

// ---------------------------------------------------------------------------------------------
// polyblur_deblurring (deblurring.py:23-96)
// ---------------------------------------------------------------------------------------------
int pb_polyblur_batch(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                      const pb_options *opt, pb_blur_info *host_info) {
    int rc = check_shape(ctx, dtype, B, C, H, W, 1);
    if (rc) return rc;
    if (!in || !out || !opt) return pb_fail(ctx, PB_ERR_BADARG, "null argument");
    if (in == out) return pb_fail(ctx, PB_ERR_BADARG, "out may not alias in");
    if (opt->n_iter < 0) return pb_fail(ctx, PB_ERR_BADARG, "n_iter < 0");
    if (opt->boundary != PB_WRAP && opt->boundary != PB_ZERO) return pb_fail(ctx, PB_ERR_BADARG, "bad boundary");
    const int ksize = pb_kernel_size(opt);
    if (!ksize) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "ker_size %d: sizes from 2 to %d are built", opt->ker_size, PB_KSIZE_MAX);
    if (opt->separable_approx && opt->edgetaping)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "edgetaping is not defined for the separable approximation");
    // (an even ker_size is the reference's off-centre tap grid, blur_estimation.py:222 / filters.py:78: the 1-D kernels of the
    // separable approximation are built on the centred grid only; the edgetaper takes it since round 6 -- its weights are
    // autocorrelations of the projections, which do not care where the taps sit)
    if (!(ksize & 1) && opt->separable_approx)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "ker_size %d: the separable approximation is built for odd sizes only", ksize);
    // (kernels beyond the 25 x 25 record take conv_big.hip's pass: no separable approximation there; the edgetaper since round 6)
    if (ksize > PB_KSIZE && opt->separable_approx)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "ker_size %d: the separable approximation is built for sizes up to %d", ksize, PB_KSIZE);
    PB_HIP(hipSetDevice(ctx->device));
    ctx->sel2_mask = 0;
    Geometry g = geometry(B, C, H, W, ksize / 2);
    // the polynomial goes through pb_launch_conv_poly (a PolySpec means something to it) ...
    const bool poly_steps = !opt->separable_approx && ksize <= PB_KSIZE;
    // ... and the estimation builds its spectra, not the kernels' own
    const bool poly_eligible = (opt->boundary == PB_WRAP || ctx->zero_ring) && !opt->edgetaping && poly_steps;
    // the records are point-symmetric Gaussians the estimation of THIS call builds on an odd ker_size grid (PolySpec.always)
    const bool est_gaussians = (ksize & 1) && poly_steps;
    // ... and every one of them takes the window form of a single pass (PolySpec.always == 2): the edgetaper's three blends
    // issue the wave body's launch and nothing else
    const bool taper_windows = opt->edgetaping && est_gaussians && ctx->poly_always && ctx->poly_mode != 0 && ctx->fft_min_phases >= 0 && ctx->fft_wave;
    const long n = (long)g.P * g.HW;
    const int n_iter = opt->n_iter;
    if (n_iter == 0) {
        PB_HIP(hipMemcpyAsync(out, in, dsize(dtype) * n, hipMemcpyDeviceToDevice, ctx->stream));
        return PB_OK;
    }
    if (dtype == PB_U8 && (opt->remove_halo || opt->prefilter != PB_PREFILTER_NONE)) {
        // halo masking and the prefilters read the current image from several more kernels: those options run on
        // an fp32 copy, the conversions at either end being the same img_as_float32 / img_as_ubyte
        float *in32 = static_cast<float *>(pb_scratch(ctx, "pipe.u8in", sizeof(float) * n));
        float *out32 = static_cast<float *>(pb_scratch(ctx, "pipe.u8out", sizeof(float) * n));
        if (!in32 || !out32) return PB_ERR_NOMEM;
        rc = pb_convert_to_float(ctx, in, PB_U8, in32, n);
        if (rc) return rc;
        rc = pb_polyblur_batch(ctx, in32, out32, PB_F32, B, C, H, W, opt, host_info);
        if (rc) return rc;
        return pb_convert_from_float(ctx, out32, out, PB_U8, n);
    }
    pb_blur_info *infos = static_cast<pb_blur_info *>(pb_scratch(ctx, "pipe.info", sizeof(pb_blur_info) * (size_t)n_iter * B));
    if (!infos) return PB_ERR_NOMEM;
    // images between iterations are fp32 whatever the I/O type: fp16 / 8-bit I/O rounds once, in the last store
    // (fp32 I/O alternates between `out` and one scratch image; narrower I/O needs two fp32 scratch images)
    const int work = PB_F32;
    void *tmpimg = nullptr, *tmpimg2 = nullptr;
    if (n_iter > 1) {
        tmpimg = pb_scratch(ctx, "pipe.img", dsize(work) * n);
        if (!tmpimg) return PB_ERR_NOMEM;
    }
    if (n_iter > 2 && dtype != PB_F32) {
        tmpimg2 = pb_scratch(ctx, "pipe.img2", dsize(work) * n);
        if (!tmpimg2) return PB_ERR_NOMEM;
    }
    // gradients of the ORIGINAL image, used by halo masking in every iteration (deblurring.py:61,83)
    // (an fp16 call keeps them -- and every iteration's d/dx of the deblurred image -- as fp16 planes where the line transforms
    // can write such planes: halo_kernel's TG)
    void *g0x = nullptr, *g0y = nullptr;
    float *nM = nullptr;
    const int g_dtype = (dtype == PB_F16 && pb_gradient_planes_half(ctx, H, W)) ? PB_F16 : PB_F32;
    if (opt->remove_halo) {
        g0x = pb_scratch(ctx, "pipe.g0x", dsize(g_dtype) * n);
        g0y = pb_scratch(ctx, "pipe.g0y", dsize(g_dtype) * n);
        nM = static_cast<float *>(pb_scratch(ctx, "inv.nM", sizeof(float) * g.P));
        if (!g0x || !g0y || !nM) return PB_ERR_NOMEM;
        const float *in32 = static_cast<const float *>(in);
        if (dtype != PB_F32) {
            float *conv = static_cast<float *>(pb_scratch(ctx, "pipe.in32", sizeof(float) * n));
            if (!conv) return PB_ERR_NOMEM;
            rc = pb_convert_to_float(ctx, in, dtype, conv, n);
            if (rc) return rc;
            in32 = conv;
        }
        rc = pb_fourier_gradients_typed(ctx, in32, g.P, H, W, g0x, g0y, g_dtype);
        if (rc) return rc;
        rc = pb_grad_energy(ctx, g0x, g0y, nM, g.P, g.HW, g_dtype);
        if (rc) return rc;
    }
    float *smooth = nullptr, *ybuf = nullptr;
    if (opt->prefilter != PB_PREFILTER_NONE) {
        smooth = static_cast<float *>(pb_scratch(ctx, "pipe.smooth", sizeof(float) * n));
        ybuf = static_cast<float *>(pb_scratch(ctx, "pipe.y", sizeof(float) * n));
        if (!smooth || !ybuf) return PB_ERR_NOMEM;
    }
    if (opt->half_temporaries) {
        if (dtype != PB_F16 || opt->edgetaping || opt->separable_approx)
            return pb_fail(ctx, PB_ERR_UNSUPPORTED, "half_temporaries: fp16 images only, not with edgetaping / separable_approx");
        g.t1h = pb_scratch(ctx, "inv.t1h", sizeof(__half) * g.P * g.pplane);
        g.t2h = pb_scratch(ctx, "inv.t2h", sizeof(__half) * g.P * g.pplane);
        if (!g.t1h || !g.t2h) return PB_ERR_NOMEM;
    }
    pb_blur_info *sep = nullptr;
    if (opt->separable_approx && n_iter > 0) {
        sep = static_cast<pb_blur_info *>(pb_scratch(ctx, "pipe.sepinfo", sizeof(pb_blur_info) * 2 * (size_t)B));
        g.sep_u = static_cast<float *>(pb_scratch(ctx, "inv.u", sizeof(float) * g.P * g.pplane));
        if (!sep || !g.sep_u) return PB_ERR_NOMEM;
        g.sep1 = sep; g.sep2 = sep + B;
    }
    const void *cur = in;
    for (int it = 0; it < n_iter; ++it) {
        // the last iteration must land in `out`; alternate between out and tmpimg before that
        void *dst = ((n_iter - 1 - it) % 2 == 0) ? out : tmpimg;
        if (dtype != PB_F32 && it != n_iter - 1) dst = (it % 2 == 0) ? tmpimg : tmpimg2;
        const int cur_dtype = it == 0 ? dtype : work, dst_dtype = it == n_iter - 1 ? dtype : work;
        pb_blur_info *info = infos + (size_t)it * B;
        // The plan of the iteration.  The estimation ends with the kernels' spectra and the images' choice of body, so it has to
        // know what the passes behind it will ask for: they are handed the same plan.
        IterPlan plan;
        plan.slot = it;                           // (this iteration's choices of body keep a slot of their own: pb_body_selection)
        if (poly_steps) {
            // (the polynomial's operand: the image or its smooth component, behind an edgetaper the padded, tapered plane; its
            // result: fp32 wherever another kernel reads it before the iteration's last store)
            const int src_dtype = opt->prefilter != PB_PREFILTER_NONE ? PB_F32 : cur_dtype;
            const int last_out = (opt->remove_halo || opt->prefilter != PB_PREFILTER_NONE) ? PB_F32 : dst_dtype;
            plan.poly = poly_spec(ctx, g, src_dtype, opt->edgetaping != 0, opt->boundary, last_out, opt->alpha, opt->beta, est_gaussians);
        }
        if (poly_eligible) {
            plan.est1 = plan.poly;
            // (the zero boundary in its window-pass + ring form: the ring steps run with the kernels' OWN spectra -- the estimation
            // builds them as its second set instead of a khat_kernel launch in front of the ring)
            if (opt->boundary == PB_ZERO && plan.poly.always == 1) plan.est2 = window_form_spec();
        } else if (taper_windows) {
            plan.blends = plan.est1 = window_form_spec();      // (the blends come first: the kernels' own spectra, window form for all)
            // (... and the polynomial behind them wants ITS spectra: the second set.  The zero boundary's ring there would want a
            // third set: left to its own launch)
            if (ctx->poly_padded && opt->boundary != PB_ZERO) plan.est2 = plan.poly;
        }
        rc = pb_estimate_impl(ctx, cur, cur_dtype, B, C, H, W, opt, info, plan.est1, plan.est2, plan.slot);
        if (rc) return rc;
        if (ksize > PB_KSIZE) {
            rc = pb_build_big_taps(ctx, info, B, ksize, (!(ksize & 1) && opt->boundary == PB_WRAP) ? 1 : 0, &g.big);
            if (rc) return rc;
        }
        if (sep) {
            rc = pb_make_sep_records(ctx, B, info, sep, opt->support, ksize);
            if (rc) return rc;
        }
        if (opt->prefilter == PB_PREFILTER_NONE) {
            rc = inverse_filter(ctx, g, cur, cur_dtype, dst, dst_dtype, info, opt->alpha, opt->beta, opt->boundary,
                                opt->edgetaping, opt->remove_halo, g0x, g0y, nM, 1, nullptr, 0, nullptr, g_dtype, &plan);
            if (rc) return rc;
        } else {
            if (opt->prefilter == PB_PREFILTER_BILATERAL)
                rc = pb_bilateral5_impl(ctx, cur, cur_dtype, smooth, PB_F32, g.P, H, W);
            else if (opt->prefilter == PB_PREFILTER_NORMALIZED_CONVOLUTION)
                rc = pb_nc_filter_impl(ctx, cur, cur_dtype, smooth, B, C, H, W, opt->sigma_s, opt->sigma_r, 1);
            else
                rc = pb_dt_filter_impl(ctx, cur, nullptr, cur_dtype, smooth, B, C, H, W, opt->sigma_s, opt->sigma_r, 1);
            if (rc) return rc;
            if (opt->remove_halo) {                 // the halo kernel recombines as it stores: no ybuf round trip
                rc = inverse_filter(ctx, g, smooth, PB_F32, dst, dst_dtype, info, opt->alpha, opt->beta, opt->boundary,
                                    opt->edgetaping, 1, g0x, g0y, nM, 1, cur, cur_dtype, smooth, g_dtype, &plan);
                if (rc) return rc;
            } else {
                rc = inverse_filter(ctx, g, smooth, PB_F32, ybuf, PB_F32, info, opt->alpha, opt->beta, opt->boundary,
                                    opt->edgetaping, 0, g0x, g0y, nM, 1, nullptr, 0, nullptr, g_dtype, &plan);
                if (rc) return rc;
                rc = pb_recombine(ctx, ybuf, cur, cur_dtype, smooth, dst, dst_dtype, n);
                if (rc) return rc;
            }
        }
        cur = dst;
    }
    if (host_info) {
        PB_HIP(hipMemcpyAsync(host_info, infos, sizeof(pb_blur_info) * (size_t)n_iter * B, hipMemcpyDeviceToHost, ctx->stream));
        PB_HIP(hipStreamSynchronize(ctx->stream));
    }
    return PB_OK;
}

int pb_u8_deinterleave(pb_ctx *ctx, const unsigned char *hwc, unsigned char *chw, int B, int C, int H, int W) {
    if (!ctx || !hwc || !chw || hwc == chw || B < 1 || C < 1 || H < 1 || W < 1) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    return pb_u8_layout(ctx, hwc, chw, B, C, H, W, 1);
}

int pb_u8_interleave(pb_ctx *ctx, const unsigned char *chw, unsigned char *hwc, int B, int C, int H, int W) {
    if (!ctx || !hwc || !chw || hwc == chw || B < 1 || C < 1 || H < 1 || W < 1) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    return pb_u8_layout(ctx, chw, hwc, B, C, H, W, 0);
}

int pb_extract_patches(pb_ctx *ctx, const void *img, void *patches, int dtype, int B, int C, int H, int W, int ph, int pw,
                       int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left, int first, int count) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!img || !patches || ph < 1 || pw < 1 || step_h < 1 || step_w < 1 || n_i < 1 || n_j < 1 || first < 0 || count < 1 ||
        first + count > n_i * n_j)
        return pb_fail(ctx, PB_ERR_BADARG, "extract_patches: bad argument");
    PB_HIP(hipSetDevice(ctx->device));
    return pb_extract_patches_impl(ctx, img, patches, dtype, B, C, H, W, ph, pw, step_h, step_w, n_j, pad_top, pad_left, first, count);
}

int pb_overlap_add(pb_ctx *ctx, const void *patches, void *out, int dtype, int B, int C, int H, int W, int ph, int pw,
                   int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left, const float *dev_win_y,
                   const float *dev_win_x) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!patches || !out || !dev_win_y || !dev_win_x || ph < 1 || pw < 1 || step_h < 1 || step_w < 1 || n_i < 1 || n_j < 1)
        return pb_fail(ctx, PB_ERR_BADARG, "overlap_add: bad argument");
    PB_HIP(hipSetDevice(ctx->device));
    return pb_overlap_add_impl(ctx, patches, out, dtype, B, C, H, W, ph, pw, step_h, step_w, n_i, n_j, pad_top, pad_left,
                               dev_win_y, dev_win_x);
}

int pb_body_selection(pb_ctx *ctx, int iteration, int *host, int B) {
    if (!ctx || !host || B < 1 || iteration < -1) return PB_ERR_BADARG;
    PB_HIP(hipSetDevice(ctx->device));
    const auto it = ctx->scratch.find("conv.fftsel");
    if (it == ctx->scratch.end() || ctx->sel_B != B || it->second.bytes < sizeof(pb_fft_sel) * (size_t)B * PB_SEL_SLOTS)
        return pb_fail(ctx, PB_ERR_BADARG, "pb_body_selection: no selection for %d images on this context", B);
    const int slot = (iteration < 0 ? ctx->sel_last : iteration) % PB_SEL_SLOTS;
    std::vector<pb_fft_sel> h((size_t)B);
    // (an iteration whose polynomial read the second set's selections -- behind an edgetaper -- is reported from there)
    const pb_fft_sel *src = static_cast<const pb_fft_sel *>(it->second.p);
    const auto it2 = ctx->scratch.find("conv.fftsel2");
    if ((ctx->sel2_mask >> slot) & 1u && it2 != ctx->scratch.end() && it2->second.bytes >= sizeof(pb_fft_sel) * (size_t)B * PB_SEL_SLOTS)
        src = static_cast<const pb_fft_sel *>(it2->second.p);
    PB_HIP(hipMemcpyAsync(h.data(), src + (size_t)slot * B, sizeof(pb_fft_sel) * (size_t)B,
                          hipMemcpyDeviceToHost, ctx->stream));
    PB_HIP(hipStreamSynchronize(ctx->stream));
    for (int b = 0; b < B; ++b) {
        host[6 * b] = h[b].use_fft; host[6 * b + 1] = h[b].pad_[1] == 1 ? -1 : h[b].rf; host[6 * b + 2] = h[b].strip;      // (pad_[1]: the short chain's record workgroup found asymmetric taps)
        host[6 * b + 3] = h[b].poly; host[6 * b + 4] = h[b].hx; host[6 * b + 5] = h[b].hy;
    }
    return PB_OK;
}

int pb_profile_begin(pb_ctx *ctx) {
    if (!ctx) return PB_ERR_BADARG;
    PB_HIP(hipStreamSynchronize(ctx->stream));
    for (auto &r : ctx->prof) { ctx->evpool.push_back(r.a); ctx->evpool.push_back(r.b); }
    ctx->prof.clear();
    ctx->prof_on = true;
    return PB_OK;
}

int pb_profile_end(pb_ctx *ctx, float *host_ms, int *host_count) {
    if (!ctx || !host_ms || !host_count) return PB_ERR_BADARG;
    ctx->prof_on = false;
    PB_HIP(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < PB_PROF_NTAGS; ++t) { host_ms[t] = 0.f; host_count[t] = 0; }
    for (auto &r : ctx->prof) {
        float ms = 0.f;
        PB_HIP(hipEventElapsedTime(&ms, r.a, r.b));
        host_ms[r.tag] += ms;
        host_count[r.tag] += 1;
        ctx->evpool.push_back(r.a);
        ctx->evpool.push_back(r.b);
    }
    ctx->prof.clear();
    return PB_OK;
}

int pb_time_inner_loop(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W,
                       const pb_blur_info *dev_info, float alpha, float beta, int boundary, int reps, float *host_ms) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || !dev_info || reps < 1 || !host_ms) return pb_fail(ctx, PB_ERR_BADARG, "bad argument");
    PB_HIP(hipSetDevice(ctx->device));
    const Geometry g = geometry(B, C, H, W);
    float *t1 = static_cast<float *>(pb_scratch(ctx, "inv.t1", sizeof(float) * g.P * g.pplane));
    float *t2 = static_cast<float *>(pb_scratch(ctx, "inv.t2", sizeof(float) * g.P * g.pplane));
    if (!t1 || !t2) return PB_ERR_NOMEM;
    rc = run_polynomial(ctx, g, in, dtype, nullptr, dev_info, alpha, beta, boundary, t1, t2, out, dtype, 1);   // warm
    if (rc) return rc;
    PB_HIP(hipEventRecord(ctx->ev0, ctx->stream));
    for (int r = 0; r < reps; ++r) {
        rc = run_polynomial(ctx, g, in, dtype, nullptr, dev_info, alpha, beta, boundary, t1, t2, out, dtype, 1);
        if (rc) return rc;
    }
    PB_HIP(hipEventRecord(ctx->ev1, ctx->stream));
    PB_HIP(hipEventSynchronize(ctx->ev1));
    float ms = 0.f;
    PB_HIP(hipEventElapsedTime(&ms, ctx->ev0, ctx->ev1));
    *host_ms = ms / reps;
    return PB_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// caller-owned kernel sets: the non-blind entry points for any kh x kw taps up to 49 x 49
// (deblurring.py:211-239, filters.py:14-37, edgetaper.py:26-33 with a kernel tensor of the caller's)
// ---------------------------------------------------------------------------------------------
// Either 25 x 25 records every body of the reblurring pass serves (kh, kw <= 25, not taller than wide) or conv_big.hip's tap
// tables; either way one form for the zero boundary (correlation placed by the 'same' rule) and one for the wrap boundary (the
// taps reflected inside their own kh x kw array, THEN placed -- reflecting an embedded even-sized array is off by one
// sample).  All of it is device memory of the set's own: no other call on the context touches it.
struct pb_taps {
    pb_ctx *ctx = nullptr;
    int B = 0, kh = 0, kw = 0;
    pb_blur_info *rec_zero = nullptr, *rec_wrap = nullptr;      // records (rec_wrap == rec_zero: point-symmetric as embedded)
    float *tables = nullptr;                                    // tables: B zero-boundary ones, B wrap-boundary ones, B autocorrelations
    float *raw = nullptr;                                       // the B kh x kw kernels as given (the pure-phase polynomial places them itself: conv_phase.hip)
    BigTaps big_zero, big_wrap;
};

namespace {

bool taps_in_records(int kh, int kw) { return kh <= PB_KSIZE && kw <= PB_KSIZE && kh / 2 <= kw / 2; }

// kh x kw taps into a zeroed 25 x 25 array: tap (i, j) at row 12 - (kh - 1) / 2 + i, column 12 - (kw - 1) / 2 + j
void embed_taps(const float *k, int kh, int kw, bool reflect, float *rec) {
    const int r0 = PB_KRAD - (kh - 1) / 2, c0 = PB_KRAD - (kw - 1) / 2;
    for (int i = 0; i < kh; ++i)
        for (int j = 0; j < kw; ++j)
            rec[(r0 + i) * PB_KSIZE + c0 + j] = reflect ? k[(kh - 1 - i) * kw + (kw - 1 - j)] : k[i * kw + j];
}

int taps_records(pb_ctx *ctx, const float *host_taps, int B, int kh, int kw, bool reflect, int support, pb_blur_info *rec) {
    std::vector<pb_blur_info> h(B);
    memset(h.data(), 0, sizeof(pb_blur_info) * B);
    for (int i = 0; i < B; ++i) embed_taps(host_taps + (size_t)i * kh * kw, kh, kw, reflect, h[i].kernel);
    PB_HIP(hipMemcpyAsync(rec, h.data(), sizeof(pb_blur_info) * B, hipMemcpyHostToDevice, ctx->stream));
    PB_HIP(hipStreamSynchronize(ctx->stream));
    const int rc = pb_make_kernels_dev(ctx, B, rec, support, 1);
    return rc ? rc : pb_cache_records(ctx, rec, B);
}

// what every call with a set checks, and the geometry + records it then runs with.  domain: the given image is the whole
// domain (pb_convolve2d_taps, pb_edgetaper_taps) -- no pad; else the image is replicate-padded by kw / 2 (utils.py:48-61: the
// height of the kernel plays no part)
int taps_geometry(pb_ctx *ctx, const pb_taps *t, int B, int C, int H, int W, int boundary, bool domain, bool circular_only,
                  Geometry *g, const pb_blur_info **recs) {
    if (!t || t->ctx != ctx) return pb_fail(ctx, PB_ERR_BADARG, "the kernel set is not one of this context's");
    if (boundary != PB_WRAP && boundary != PB_ZERO) return pb_fail(ctx, PB_ERR_BADARG, "bad boundary");
    if (t->B != B) return pb_fail(ctx, PB_ERR_BADARG, "the set holds %d kernels, the batch %d images (one kernel per image)", t->B, B);
    const int pad = domain ? 0 : t->kw / 2;
    if (t->kh > H + 2 * pad - 1)
        return pb_fail(ctx, PB_ERR_BADARG, "a kernel of %d rows does not fit the %d rows of the %sdomain (at most rows - 1: filters.py:255-273, edgetaper.py:11)",
                       t->kh, H + 2 * pad, domain ? "" : "padded ");
    if (t->kw > W + 2 * pad - 1)
        return pb_fail(ctx, PB_ERR_BADARG, "a kernel of %d columns does not fit the %d columns of the domain (at most columns - 1)", t->kw, W + 2 * pad);
    if (circular_only && boundary == PB_WRAP && t->kh / 2 > t->kw / 2)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "a %d x %d kernel is taller than wide: convolve2d(method='fft') pads circularly by the half-WIDTH only "
                       "(filters.py:33, utils.py:48-61), which is no circular convolution over the domain -- not built", t->kh, t->kw);
    *g = geometry(B, C, H, W, pad);
    if (t->tables) { g->big = boundary == PB_WRAP ? t->big_wrap : t->big_zero; *recs = nullptr; }      // (conv_big.hip reads no record)
    else *recs = boundary == PB_WRAP ? t->rec_wrap : t->rec_zero;
    return PB_OK;
}

int taps_pass(pb_ctx *ctx, const Geometry &g, const ConvPass &p) { return g.big.taps ? pb_launch_conv_big(ctx, p, g.big) : pb_launch_conv(ctx, p, PassWant()); }

// The adjoint of a pass with an ODD-sized kernel is the same form under the same boundary with the taps reflected inside their
// kh x kw array -- and the set already holds that orientation as the OTHER boundary's form (records: embed_taps(reflect); tables:
// caller_taps_kernel's wrap[iy][ix] = raw[kh/2 - iy][kw/2 - ix] = zero[-iy][-ix] when (kh - 1) / 2 == kh / 2).  An even side moves the
// centre by one sample in the adjoint: refused by the callers.
void taps_adjoint(const pb_taps *t, int boundary, Geometry *g, const pb_blur_info **recs) {
    if (t->tables) { g->big = boundary == PB_WRAP ? t->big_zero : t->big_wrap; *recs = nullptr; }
    else *recs = boundary == PB_WRAP ? t->rec_zero : t->rec_wrap;
}

// The adjoint of an even kernel side sits one sample off the forms a set holds: every backward call that runs a pass with the set's
// other orientation, or the forward's own pass on the way to a gradient, takes odd sides only.  taps may be null (no rule)
int odd_sides_only(pb_ctx *ctx, const char *who, const pb_taps *taps) {
    if (taps && (!(taps->kh & 1) || !(taps->kw & 1)))
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "%s: a %d x %d kernel -- the adjoint of an even side sits one sample off the forms the set holds: "
                       "odd sides only", who, taps->kh, taps->kw);
    return PB_OK;
}

// what both backward calls check before any device work
int backward_args(pb_ctx *ctx, const char *who, const float *x, const float *grad_out, const float *grad_x, const float *grad_taps,
                  const pb_taps *taps) {
    if (!grad_out) return pb_fail(ctx, PB_ERR_BADARG, "%s: grad_out is null", who);
    if (!grad_x && !grad_taps) return pb_fail(ctx, PB_ERR_BADARG, "%s: grad_x and grad_taps are both null", who);
    if (grad_taps && !x) return pb_fail(ctx, PB_ERR_BADARG, "%s: the tap gradient needs x", who);
    if ((grad_x && (grad_x == grad_out || grad_x == x)) || (grad_taps && (grad_taps == grad_out || grad_taps == x || grad_taps == grad_x)))
        return pb_fail(ctx, PB_ERR_BADARG, "%s: an output aliases an input", who);
    return odd_sides_only(ctx, who, taps);
}

}  // namespace

extern "C" {

int pb_taps_create(pb_ctx *ctx, int B, int kh, int kw, const float *host_taps, int support, pb_taps **taps) {
    if (!ctx || !taps) return PB_ERR_BADARG;
    *taps = nullptr;
    if (B < 1 || !host_taps) return pb_fail(ctx, PB_ERR_BADARG, "pb_taps_create: bad argument");
    if (kh < 1 || kw < 1) return pb_fail(ctx, PB_ERR_BADARG, "a %d x %d kernel: sizes start at 1 x 2", kh, kw);
    if (kw == 1) return pb_fail(ctx, PB_ERR_BADARG, "a kernel one tap wide pads by 0 samples, and the reference's crop [0:-0] is then empty (utils.py:63-67)");
    if (kh > PB_KSIZE_MAX || kw > PB_KSIZE_MAX)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "a %d x %d kernel: sizes up to %d x %d are built", kh, kw, PB_KSIZE_MAX, PB_KSIZE_MAX);
    PB_HIP(hipSetDevice(ctx->device));
    pb_taps *t = new pb_taps();
    t->ctx = ctx; t->B = B; t->kh = kh; t->kw = kw;
    int rc = PB_OK;
    {
        void *m = nullptr;
        const size_t bytes = sizeof(float) * (size_t)B * kh * kw;
        if (hipMalloc(&m, bytes) != hipSuccess) {
            delete t;
            return pb_fail(ctx, PB_ERR_NOMEM, "pb_taps_create: hipMalloc of %d kernels failed", B);
        }
        t->raw = static_cast<float *>(m);
        // (no wait of its own: both forms below end in a stream synchronise before the call returns)
        if (hipMemcpyAsync(t->raw, host_taps, bytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess) {
            (void)pb_taps_free(t);
            return pb_fail(ctx, PB_ERR_HIP, "pb_taps_create: copy of the taps failed");
        }
    }
    if (taps_in_records(kh, kw)) {
        bool sym = true;                                     // (as embedded: an even size never is)
        std::vector<float> e(PB_KSIZE * PB_KSIZE);
        for (int i = 0; i < B && sym; ++i) {
            std::fill(e.begin(), e.end(), 0.f);
            embed_taps(host_taps + (size_t)i * kh * kw, kh, kw, false, e.data());
            for (int n = 0; n < PB_KSIZE * PB_KSIZE / 2 && sym; ++n) sym = e[n] == e[PB_KSIZE * PB_KSIZE - 1 - n];
        }
        void *m = nullptr;
        if (hipMalloc(&m, sizeof(pb_blur_info) * (size_t)B * (sym ? 1 : 2)) != hipSuccess) {
            (void)pb_taps_free(t);
            return pb_fail(ctx, PB_ERR_NOMEM, "pb_taps_create: hipMalloc of %d records failed", B * (sym ? 1 : 2));
        }
        t->rec_zero = static_cast<pb_blur_info *>(m);
        t->rec_wrap = sym ? t->rec_zero : t->rec_zero + B;
        rc = taps_records(ctx, host_taps, B, kh, kw, false, support, t->rec_zero);
        if (!rc && !sym) rc = taps_records(ctx, host_taps, B, kh, kw, true, support, t->rec_wrap);
    } else {
        const size_t nt = (size_t)PB_BIG_TABLE * B;
        void *m = nullptr;
        if (hipMalloc(&m, sizeof(float) * (2 * nt + (size_t)PB_BIG_ACORR * B)) != hipSuccess) {
            (void)pb_taps_free(t);
            return pb_fail(ctx, PB_ERR_NOMEM, "pb_taps_create: hipMalloc of %d tap tables failed", 2 * B);
        }
        t->tables = static_cast<float *>(m);
        rc = pb_build_caller_taps(ctx, t->raw, B, kh, kw, t->tables, t->tables + nt, t->tables + 2 * nt);
        if (!rc && hipStreamSynchronize(ctx->stream) != hipSuccess) rc = pb_fail(ctx, PB_ERR_HIP, "pb_taps_create: building the tap tables failed");
        t->big_zero.taps = t->tables; t->big_wrap.taps = t->tables + nt;
        t->big_zero.acorr = t->big_wrap.acorr = t->tables + 2 * nt;
        t->big_zero.ry = t->big_wrap.ry = kh / 2;
        t->big_zero.rx = t->big_wrap.rx = kw / 2;
    }
    if (rc) { (void)pb_taps_free(t); return rc; }
    *taps = t;
    return PB_OK;
}

int pb_taps_free(pb_taps *t) {
    if (!t) return PB_OK;
    pb_ctx *ctx = t->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    if (t->rec_zero) {
        pb_forget_records(ctx, t->rec_zero, t->rec_wrap == t->rec_zero ? t->B : 2 * t->B);      // (the address may come back with other taps)
        (void)hipFree(t->rec_zero);
    }
    if (t->tables) (void)hipFree(t->tables);
    if (t->raw) (void)hipFree(t->raw);
    delete t;
    return PB_OK;
}

int pb_convolve2d_taps(pb_ctx *ctx, const float *in, float *out, int B, int C, int H, int W, const pb_taps *taps, int boundary) {
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || in == out) return pb_fail(ctx, PB_ERR_BADARG, "null or aliased image");
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, boundary, true, true, &g, &recs);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    g.pp = W; g.pplane = g.HW;                              // (the caller's planes are not pitched)
    ConvPass p = base_pass(g, recs, boundary);
    set_in_padded(p, g, in); set_x_padded(p, g, in); set_out_padded(p, g, out);
    return taps_pass(ctx, g, p);
}

int pb_edgetaper_taps(pb_ctx *ctx, const float *in, float *out, int B, int C, int H, int W, const pb_taps *taps, int boundary,
                      int n_tapers) {
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || in == out) return pb_fail(ctx, PB_ERR_BADARG, "null or aliased image");
    if (n_tapers < 0) return pb_fail(ctx, PB_ERR_BADARG, "n_tapers < 0");
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, boundary, true, true, &g, &recs);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    g.pp = W; g.pplane = g.HW;
    if (n_tapers == 0) {
        PB_HIP(hipMemcpyAsync(out, in, sizeof(float) * g.P * g.HW, hipMemcpyDeviceToDevice, ctx->stream));
        return PB_OK;
    }
    float *tmp = nullptr;
    if (n_tapers > 1) {
        tmp = static_cast<float *>(pb_scratch(ctx, "taper.tmp", sizeof(float) * g.P * g.HW));
        if (!tmp) return PB_ERR_NOMEM;
    }
    ConvPass p = base_pass(g, recs, boundary);
    p.epilogue = EPI_TAPER;
    // (the blends alternate between `out` and the scratch plane so that the last one lands in `out`)
    const float *src = in;
    for (int i = 0; i < n_tapers; ++i) {
        float *dst = ((n_tapers - 1 - i) & 1) ? tmp : out;
        set_in_padded(p, g, src); set_x_padded(p, g, src); set_out_padded(p, g, dst);
        rc = taps_pass(ctx, g, p);
        if (rc) return rc;
        src = dst;
    }
    return PB_OK;
}

int pb_inverse_filter_taps(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W, const pb_taps *taps,
                           float alpha, float beta, int boundary, int edgetaping, int remove_halo, const float *grad0_x,
                           const float *grad0_y) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || in == out) return pb_fail(ctx, PB_ERR_BADARG, "null or aliased image");
    if ((grad0_x == nullptr) != (grad0_y == nullptr)) return pb_fail(ctx, PB_ERR_BADARG, "grad0_x and grad0_y: both or neither");
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, boundary, false, edgetaping != 0, &g, &recs);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    float *nM = nullptr;
    if (remove_halo && grad0_x) {
        nM = static_cast<float *>(pb_scratch(ctx, "inv.nM", sizeof(float) * g.P));
        if (!nM) return PB_ERR_NOMEM;
        rc = pb_grad_energy(ctx, grad0_x, grad0_y, nM, g.P, g.HW);
        if (rc) return rc;
    }
    return inverse_filter(ctx, g, in, dtype, out, dtype, recs, alpha, beta, boundary, edgetaping, remove_halo, grad0_x, grad0_y, nM, 1);
}

int pb_inverse_filter_phase_taps(pb_ctx *ctx, const void *in, void *out, int dtype, int B, int C, int H, int W, const pb_taps *taps,
                                 float alpha, float beta, int edgetaping, int remove_halo, const float *grad0_x,
                                 const float *grad0_y) {
    int rc = check_shape(ctx, dtype, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || in == out) return pb_fail(ctx, PB_ERR_BADARG, "null or aliased image");
    if ((grad0_x == nullptr) != (grad0_y == nullptr)) return pb_fail(ctx, PB_ERR_BADARG, "grad0_x and grad0_y: both or neither");
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, PB_WRAP, false, edgetaping != 0, &g, &recs);
    if (rc) return rc;
    rc = pb_phase_sides_supported(ctx, g.Hp, g.Wp);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    g.phase_taps = taps->raw; g.phase_kh = taps->kh; g.phase_kw = taps->kw;
    float *nM = nullptr;
    if (remove_halo && grad0_x) {
        nM = static_cast<float *>(pb_scratch(ctx, "inv.nM", sizeof(float) * g.P));
        if (!nM) return PB_ERR_NOMEM;
        rc = pb_grad_energy(ctx, grad0_x, grad0_y, nM, g.P, g.HW);
        if (rc) return rc;
    }
    return inverse_filter(ctx, g, in, dtype, out, dtype, recs, alpha, beta, PB_WRAP, edgetaping, remove_halo, grad0_x, grad0_y, nM, 1);
}

int pb_compute_polynomial_taps(pb_ctx *ctx, const float *in, float *out, int B, int C, int H, int W, const pb_taps *taps,
                               float alpha, float beta, int boundary, int not_symmetric) {
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    if (!in || !out || in == out) return pb_fail(ctx, PB_ERR_BADARG, "null or aliased image");
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, boundary, true, false, &g, &recs);
    if (rc) return rc;
    if (not_symmetric && boundary != PB_WRAP)
        return pb_fail(ctx, PB_ERR_BADARG, "not_symmetric with PB_ZERO: the reference's direct form takes the flag and ignores it (deblurring.py:122-138) -- "
                       "a silent no-op is refused; the pure-phase filter is PB_WRAP's");
    PB_HIP(hipSetDevice(ctx->device));
    g.pp = W; g.pplane = g.HW;                              // (the caller's planes are the whole domain, not pitched)
    if (not_symmetric) {
        g.phase_taps = taps->raw; g.phase_kh = taps->kh; g.phase_kw = taps->kw;
        return run_phase_polynomial(ctx, g, in, PB_F32, in, alpha, beta, out, PB_F32, 0);
    }
    float *t1 = static_cast<float *>(pb_scratch(ctx, "inv.t1", sizeof(float) * g.P * g.pplane));
    float *t2 = static_cast<float *>(pb_scratch(ctx, "inv.t2", sizeof(float) * g.P * g.pplane));
    if (!t1 || !t2) return PB_ERR_NOMEM;
    return run_polynomial(ctx, g, in, PB_F32, in, recs, alpha, beta, boundary, t1, t2, out, PB_F32, 0);
}

int pb_tap_gradient(pb_ctx *ctx, const float *u, const float *v, int B, int C, int H, int W, int kh, int kw, int boundary, float scale,
                    int accumulate, float *dev_grad) {
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    if (!u || !v || !dev_grad || dev_grad == u || dev_grad == v) return pb_fail(ctx, PB_ERR_BADARG, "pb_tap_gradient: null or aliased argument");
    if (boundary != PB_WRAP && boundary != PB_ZERO) return pb_fail(ctx, PB_ERR_BADARG, "bad boundary");
    if (kh < 1 || kw < 1) return pb_fail(ctx, PB_ERR_BADARG, "pb_tap_gradient: a %d x %d kernel", kh, kw);
    if (kh > PB_KSIZE_MAX || kw > PB_KSIZE_MAX)
        return pb_fail(ctx, PB_ERR_UNSUPPORTED, "a %d x %d kernel: sizes up to %d x %d are built", kh, kw, PB_KSIZE_MAX, PB_KSIZE_MAX);
    if (!(kh & 1) || !(kw & 1)) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "pb_tap_gradient: a %d x %d kernel -- odd sides only", kh, kw);
    PB_HIP(hipSetDevice(ctx->device));
    return pb_launch_tap_gradient(ctx, u, v, B, C, H, W, kh, kw, boundary, scale, accumulate, dev_grad);
}

int pb_convolve2d_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps, int B, int C, int H,
                                int W, const pb_taps *taps, int boundary) {
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    rc = backward_args(ctx, "pb_convolve2d_taps_backward", x, grad_out, grad_x, grad_taps, taps);
    if (rc) return rc;
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, boundary, true, true, &g, &recs);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    g.pp = W; g.pplane = g.HW;
    if (grad_x) {
        // grad_x = K^T grad_out: the same pass with the set's other orientation
        taps_adjoint(taps, boundary, &g, &recs);
        ConvPass p = base_pass(g, recs, boundary);
        set_in_padded(p, g, grad_out); set_x_padded(p, g, grad_out); set_out_padded(p, g, grad_x);
        rc = taps_pass(ctx, g, p);
        if (rc) return rc;
    }
    if (grad_taps) return pb_launch_tap_gradient(ctx, grad_out, x, B, C, H, W, taps->kh, taps->kw, boundary, 1.f, 0, grad_taps);
    return PB_OK;
}

int pb_compute_polynomial_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps, int B, int C,
                                        int H, int W, const pb_taps *taps, float alpha, float beta, int boundary) {
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    rc = backward_args(ctx, "pb_compute_polynomial_taps_backward", x, grad_out, grad_x, grad_taps, taps);
    if (rc) return rc;
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, boundary, true, false, &g, &recs);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    g.pp = W; g.pplane = g.HW;
    Geometry ga = g; const pb_blur_info *arecs = nullptr;
    taps_adjoint(taps, boundary, &ga, &arecs);
    if (grad_taps) {
        // grad_k = L(g, t2) + L(g2, t1) + L(g1, t0), t0 = a3 x, g2 = K^T g, g1 = K^T g2: the forward's two temporaries are formed
        // again, step by step (pb_launch_conv_poly would fold the three steps into one window pass and never write them)
        const size_t bytes = sizeof(float) * g.P * g.HW;
        float *t1 = static_cast<float *>(pb_scratch(ctx, "grad.t1", bytes)), *t2 = static_cast<float *>(pb_scratch(ctx, "grad.t2", bytes));
        float *g2 = static_cast<float *>(pb_scratch(ctx, "grad.g2", bytes)), *g1 = static_cast<float *>(pb_scratch(ctx, "grad.g1", bytes));
        if (!t1 || !t2 || !g2 || !g1) return PB_ERR_NOMEM;
        ConvPass steps[3];
        make_steps(g, x, PB_F32, true, recs, alpha, beta, boundary, t1, t2, g1, PB_F32, 0, steps);      // (steps[2], y itself, is not run)
        for (int s = 0; s < 2; ++s) {
            rc = taps_pass(ctx, g, steps[s]);
            if (rc) return rc;
        }
        ConvPass p = base_pass(ga, arecs, boundary);
        set_in_padded(p, ga, grad_out); set_x_padded(p, ga, grad_out); set_out_padded(p, ga, g2);
        rc = taps_pass(ctx, ga, p);
        if (rc) return rc;
        set_in_padded(p, ga, g2); set_x_padded(p, ga, g2); set_out_padded(p, ga, g1);
        rc = taps_pass(ctx, ga, p);
        if (rc) return rc;
        const float a3 = alpha / 2 - beta + 2;
        rc = pb_launch_tap_gradient(ctx, grad_out, t2, B, C, H, W, taps->kh, taps->kw, boundary, 1.f, 0, grad_taps);
        if (!rc) rc = pb_launch_tap_gradient(ctx, g2, t1, B, C, H, W, taps->kh, taps->kw, boundary, 1.f, 1, grad_taps);
        if (!rc) rc = pb_launch_tap_gradient(ctx, g1, x, B, C, H, W, taps->kh, taps->kw, boundary, a3, 1, grad_taps);
        if (rc) return rc;
    }
    if (grad_x) {
        // grad_x = b g + a1 K^T g + a2 K^T^2 g + a3 K^T^3 g: the same polynomial of the adjoint, in whichever form run_polynomial picks
        const size_t pbytes = sizeof(float) * ga.P * ga.pplane;
        float *t1 = static_cast<float *>(pb_scratch(ctx, "inv.t1", pbytes)), *t2 = static_cast<float *>(pb_scratch(ctx, "inv.t2", pbytes));
        if (!t1 || !t2) return PB_ERR_NOMEM;
        return run_polynomial(ctx, ga, grad_out, PB_F32, grad_out, arecs, alpha, beta, boundary, t1, t2, grad_x, PB_F32, 0);
    }
    return PB_OK;
}

int pb_compute_polynomial_taps_params_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_params, int B, int C, int H,
                                               int W, const pb_taps *taps, float alpha, float beta, int boundary) {
    static const char *who = "pb_compute_polynomial_taps_params_backward";
    (void)alpha; (void)beta;                                // (the polynomial is linear in both: neither gradient depends on them)
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    if (!x || !grad_out || !grad_params) return pb_fail(ctx, PB_ERR_BADARG, "%s: x, grad_out or grad_params is null", who);
    if (static_cast<const void *>(grad_params) == x || static_cast<const void *>(grad_params) == grad_out)
        return pb_fail(ctx, PB_ERR_BADARG, "%s: an output aliases an input", who);
    rc = odd_sides_only(ctx, who, taps);
    if (rc) return rc;
    if (B > 65535) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "%s: %d images (the kernels' grids take up to 65535)", who, B);
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, boundary, true, false, &g, &recs);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    g.pp = W; g.pplane = g.HW;
    // the detail images u1 = x - K x, u2 = u1 - K u1, u3 = u2 - K u2: three explicit Horner steps with scale -1, coef 1 and the
    // step's own input as its x operand, under the call's boundary -- K is the forward's own operator.  u3 overwrites u1
    const size_t bytes = sizeof(float) * g.P * g.HW;
    float *ua = static_cast<float *>(pb_scratch(ctx, "ppg.u1", bytes)), *ub = static_cast<float *>(pb_scratch(ctx, "ppg.u2", bytes));
    if (!ua || !ub) return PB_ERR_NOMEM;
    ConvPass p = base_pass(g, recs, boundary);
    p.scale = -1.f; p.coef = 1.f;
    const float *src[3] = {x, ua, ub};
    float *dst[3] = {ua, ub, ua};
    for (int s = 0; s < 3; ++s) {
        set_in_padded(p, g, src[s]); set_x_padded(p, g, src[s]); set_out_padded(p, g, dst[s]);
        rc = taps_pass(ctx, g, p);
        if (rc) return rc;
    }
    return pb_launch_poly_param_reduce(ctx, grad_out, ub, ua, grad_params, B, (long)C * g.HW);
}

int pb_edgetaper_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps, int B, int C, int H,
                               int W, const pb_taps *taps, int boundary, int n_tapers) {
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    rc = backward_args(ctx, "pb_edgetaper_taps_backward", x, grad_out, grad_x, grad_taps, taps);
    if (rc) return rc;
    if (n_tapers < 0) return pb_fail(ctx, PB_ERR_BADARG, "n_tapers < 0");
    if (B > 65535) return pb_fail(ctx, PB_ERR_UNSUPPORTED, "pb_edgetaper_taps_backward: %d images (the kernels' grids take up to 65535)", B);
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, boundary, true, true, &g, &recs);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    g.pp = W; g.pplane = g.HW;
    const size_t bytes = sizeof(float) * g.P * g.HW;
    const size_t tap_bytes = sizeof(float) * (size_t)B * taps->kh * taps->kw;
    if (n_tapers == 0) {
        if (grad_x) PB_HIP(hipMemcpyAsync(grad_x, grad_out, bytes, hipMemcpyDeviceToDevice, ctx->stream));
        if (grad_taps) PB_HIP(hipMemsetAsync(grad_taps, 0, tap_bytes, ctx->stream));
        return PB_OK;
    }
    // the autocorrelations the forward's blends read: the boundary's records, or the set's table
    TaperAcorr ac;
    if (taps->tables) { ac.acy = g.big.acorr; ac.acx = g.big.acorr + PB_BIG_ACORR / 2; ac.stride = PB_BIG_ACORR; ac.nlag = PB_KSIZE_MAX; }
    else { ac.acy = recs->acorr_y; ac.acx = recs->acorr_x; ac.stride = (long)(sizeof(pb_blur_info) / sizeof(float)); ac.nlag = PB_KSIZE; }
    Geometry ga = g; const pb_blur_info *arecs = nullptr;
    taps_adjoint(taps, boundary, &ga, &arecs);
    float *u = static_cast<float *>(pb_scratch(ctx, "etg.u", bytes)), *ag = static_cast<float *>(pb_scratch(ctx, "etg.ag", bytes));
    float *gb = n_tapers > 1 ? static_cast<float *>(pb_scratch(ctx, "etg.g", bytes)) : nullptr;
    if (!u || !ag || (n_tapers > 1 && !gb)) return PB_ERR_NOMEM;
    float *xs = nullptr, *kx = nullptr, *abar = nullptr;
    if (grad_taps) {
        // x_1 .. x_{n-1}: the forward's blends again, pass for pass (the forward keeps nothing), each into a plane set of its own
        kx = static_cast<float *>(pb_scratch(ctx, "etg.kx", bytes));
        abar = static_cast<float *>(pb_scratch(ctx, "etg.abar", sizeof(float) * (size_t)B * g.HW));
        if (!kx || !abar) return PB_ERR_NOMEM;
        if (n_tapers > 1) {
            xs = static_cast<float *>(pb_scratch(ctx, "etg.x", bytes * (size_t)(n_tapers - 1)));
            if (!xs) return PB_ERR_NOMEM;
        }
        ConvPass p = base_pass(g, recs, boundary);
        p.epilogue = EPI_TAPER;
        const float *src = x;
        for (int i = 0; i + 1 < n_tapers; ++i) {
            float *dst = xs + (size_t)i * g.P * g.HW;
            set_in_padded(p, g, src); set_x_padded(p, g, src); set_out_padded(p, g, dst);
            rc = taps_pass(ctx, g, p);
            if (rc) return rc;
            src = dst;
        }
    }
    const float *gn = grad_out;
    for (int i = n_tapers - 1; i >= 0; --i) {
        const float *xi = !grad_taps ? nullptr : i == 0 ? x : xs + (size_t)(i - 1) * g.P * g.HW;
        if (grad_taps) {
            ConvPass p = base_pass(g, recs, boundary);          // K x_i, for Abar
            set_in_padded(p, g, xi); set_x_padded(p, g, xi); set_out_padded(p, g, kx);
            rc = taps_pass(ctx, g, p);
            if (rc) return rc;
        }
        rc = pb_launch_taper_blend_adjoint(ctx, ac, xi, kx, gn, u, ag, abar, i == n_tapers - 1, B, C, H, W);
        if (rc) return rc;
        if (grad_taps) {
            rc = pb_launch_tap_gradient(ctx, u, xi, B, C, H, W, taps->kh, taps->kw, boundary, 1.f, i != n_tapers - 1, grad_taps);
            if (rc) return rc;
        }
        if (i == 0 && !grad_x) break;                           // (g_0 is the image gradient: nobody asked)
        // g_i = K^T u + A g: the pass with the set's other orientation, ag as its x operand
        float *dst = i == 0 ? grad_x : gb;
        ConvPass p = base_pass(ga, arecs, boundary);
        p.scale = 1.f; p.coef = 1.f;
        set_in_padded(p, ga, u); set_x_padded(p, ga, ag); set_out_padded(p, ga, dst);
        rc = taps_pass(ctx, ga, p);
        if (rc) return rc;
        gn = dst;
    }
    if (grad_taps) return pb_launch_taper_weight_chain(ctx, ac, abar, taps->raw, taps->kh, taps->kw, B, H, W, grad_taps);
    return PB_OK;
}

int pb_compute_polynomial_phase_taps_backward(pb_ctx *ctx, const float *x, const float *grad_out, float *grad_x, float *grad_taps, int B,
                                              int C, int H, int W, const pb_taps *taps, float alpha, float beta) {
    static const char *who = "pb_compute_polynomial_phase_taps_backward";
    int rc = check_shape(ctx, PB_F32, B, C, H, W);
    if (rc) return rc;
    // (backward_args with no set: even sides are taken -- nothing in this adjoint is centred, it is a gather at p2o's positions)
    rc = backward_args(ctx, who, x, grad_out, grad_x, grad_taps, nullptr);
    if (rc) return rc;
    Geometry g; const pb_blur_info *recs = nullptr;
    rc = taps_geometry(ctx, taps, B, C, H, W, PB_WRAP, true, false, &g, &recs);
    if (rc) return rc;
    rc = pb_phase_sides_supported(ctx, H, W);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    PhaseGradCall c;
    c.x = x; c.grad_out = grad_out; c.grad_x = grad_x; c.grad_taps = grad_taps;
    c.B = B; c.C = C; c.H = H; c.W = W;
    c.taps = taps->raw; c.kh = taps->kh; c.kw = taps->kw;
    c.alpha = alpha; c.beta = beta;
    return pb_launch_phase_backward(ctx, c);
}

}  // extern "C"
