// Internal declarations shared by the HIP translation units of libpolyblur_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include <cstdarg>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/polyblur_hip.h"
#include "dt_choice.h"
#include "line_choice.h"


// ------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------
struct FftPlan : HostPlan {      // (line_choice.h has the host half: n, the radices, the Bluestein core)
    float2 *tw = nullptr;         // W_n^m (or W_m^m for bluestein), m = 0..n-1
    float *drev = nullptr;        // derivative multiplier in digit-reversed order, / n
    // bluestein extras
    float2 *chirp = nullptr;      // w[n] = exp(+i pi n^2 / N), n = 0..N-1
    float2 *bfilt_rev = nullptr;  // FFT_M(b) in digit-reversed order, / M
    float *dnat = nullptr;        // derivative multiplier in natural order, / N
};

struct ScratchBuf {
    void *p = nullptr;
    size_t bytes = 0;
};

struct ProfRec {
    hipEvent_t a, b;
    int tag;
};

// One-pass polynomial: which filter the spectra in the context's scratch are those of (see pb_fft_sel.poly).
// on: 0 = the kernel's own spectrum (three Horner steps); 1 = the polynomial's for kernels within the 4-sample halo class
// (composite halo class 12: either tile-spectrum body can run it); 2 = the polynomial's wherever one window pass with
// the composite filter's own per-axis halos is cheaper than the three steps (wave body only: conv_wfft.hip); 3 = as 2, and
// on 128 x 128 windows (conv_w128.hip, pb_fft_sel.poly == 2) where THAT is cheapest -- cost128 = what a 128 x 128 window pair
// costs in units of a 64 x 64 one (four waves, longer transforms).
// gain, min_area: the cost model of mode 2 (khat.h).
// always == 2 (with on == 0): the kernel's own spectrum, and EVERY kernel takes the three-step window form whatever its phase
// count or rank -- the ring steps of a zero-boundary polynomial (pb_build_khat_ring), and the whole polynomial of a
// zero-boundary image too small for the ring form (api.hip: poly_spec): three launches of the wave body and nothing else.
// always: EVERY image of the record set takes a one-pass form (64 x 64 or 128 x 128 windows, whichever the cost model prices
// lower) -- the three-step and stencil forms are out of the model.  Asked for where the host can tell from (boundary,
// options, image size, ker_size) alone that every composite fits a 128 x 128 window and every kernel is a point-symmetric
// Gaussian the estimation itself builds: the polynomial then issues the two window launches and nothing else (no launch
// that finds no work, no side stream), without the host ever reading a record back.
// tall (with on >= 2): the host vouches that the composite pass reads and writes fp32 planes of at least 128 rows under the
// wrap boundary, un-tapered (that the taps are point-symmetric, an odd ker_size grid, is looked at on the device or vouched for
// by `always`, as for every one-pass form: khat.h) -- an image may then take its one pass on windows 64 wide and
// 128 tall (conv_wfft.hip: wave_tall, pb_fft_sel.pad_[0] = 1): 1 = where the cost model prices that form lowest (cost_tall = a
// tall window in 64 x 64 window pairs), 2 = every image it admits (env PB_POLY_TALL).
struct PolySpec { int on; float a3, a2, a1, b; float gain; int min_area; float cost128; int always; int tall; float cost_tall; };
inline PolySpec no_poly() { return PolySpec{0, 0.f, 0.f, 0.f, 0.f, 0.f, 0, 0.f, 0, 0, 0.f}; }
inline bool same_spec(const PolySpec &x, const PolySpec &y) {
    return x.on == y.on && x.always == y.always &&
           (!x.on || (x.a3 == y.a3 && x.a2 == y.a2 && x.a1 == y.a1 && x.b == y.b && (x.cost128 > 0.f) == (y.cost128 > 0.f) && x.tall == y.tall));
}

// rf = window halo class of the workgroup form (conv_fft.hip): 4, 8 or 12 -- 0 when only the wave form can run the image
// (a composite halo beyond 12); hx, hy = the wave form's window halo per axis (conv_wfft.hip): hx a multiple of 4 (windows stay
// on 16-byte boundaries), hy even; strip: rank-1 kernel of full support (conv_strip.hip may take it).
// poly: the image's spectrum is that of the WHOLE polynomial a3 K^3 + a2 K^2 + a1 K + b (the reference's own 'fft' form,
// deblurring.py:139-169) and the halos those of that composite filter: one window pass (ConvPass.poly = 1 or 2) replaces
// the image's three Horner steps, whose launches skip it.
struct pb_fft_sel { int use_fft; int rf; int strip; int poly; int hx; int hy; int pad_[2]; };

// What one scratch set of spectra + selections holds: the records they were built from (`n` of them at `owner`), the PolySpec
// they were built under, the slot of the selection scratch they were written to, whether the estimation built them (beside
// the records, on the stream: nothing to read back) and the buffer they were built into.  A hint: dropping it costs one
// khat_kernel launch.  The questions and updates the launchers need are the members; nothing else reads the fields.
struct SpectraSet {
    bool holds(const void *info, int B) const { return owner && owner == info && n == B; }
    // (same_spec compares `always` too: the kernels' own spectra under always == 2 are not those under always == 0)
    bool holds(const void *info, int B, const PolySpec &s) const { return holds(info, B) && same_spec(built, s); }
    void claim(const void *info, int B, const PolySpec &s, int slot, bool by_estimate) {
        owner = info; n = B; built = s; slot_ = slot; est = by_estimate;
    }
    void drop() { owner = nullptr; n = 0; est = false; }
    // a write into [lo, hi): a run of records that overlaps it anywhere, not only at its first record
    void drop_if_overlaps(const void *lo, const void *hi) {
        const char *o = static_cast<const char *>(owner);
        if (o && o < static_cast<const char *>(hi) && static_cast<const char *>(lo) < o + sizeof(pb_blur_info) * (size_t)n) drop();
    }
    void rebind(const void *b) { if (b != buf) { buf = b; drop(); } }      // (the scratch buffer was reallocated)
    bool by_estimate() const { return est; }
    int slot() const { return slot_; }
    const PolySpec &spec() const { return built; }
private:
    const void *owner = nullptr;         // nullptr: unknown
    int n = 0;                           // (a longer run at the same address has stale tails)
    PolySpec built = no_poly();
    int slot_ = 0;
    bool est = false;
    const void *buf = nullptr;
};

// What the pass being launched wants of the spectra it meets -- an argument of the call, never state of the context: the PolySpec
// they should be those of (no_poly(): a plain pass, the kernels' own spectra) and the slot of the selection scratch it writes to /
// reads from (one per iteration of a pipeline call, pb_body_selection; 0 for every other call).  Host only: no kernel sees it.
struct PassWant { PolySpec spec = no_poly(); int slot = 0; };
// What pb_build_khat / pb_build_khat_ring hand out: the spectra, the selections, and the PolySpec they were built under
struct Spectra { float *khat = nullptr; pb_fft_sel *sel = nullptr; PolySpec spec = no_poly(); };

struct pb_ctx {
    bool prof_on = false;
    std::vector<ProfRec> prof;
    std::vector<hipEvent_t> evpool;
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
    std::map<std::string, ScratchBuf> scratch;
    std::map<int, FftPlan> plans;   // the plans whose tables are on the device (pb_get_plan), by plan_key
    HostPlans host_plans;           // ... and the host halves the line transforms' choice has looked at (line_choice.h)
    float *interp_w = nullptr;     // (n_interp x (n_angles+1)) Keys weights
    int interp_na = 0, interp_ni = 0;
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_switch = nullptr;
    // A second stream for the launches of a polynomial that device-built records may leave without work (pb_launch_conv_poly):
    // forked from and joined back into `stream` inside the call, idle between calls.  nullptr: its creation failed (the engine works without it).
    hipStream_t aux = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    size_t est_done_bytes = 0;     // size of the zero-initialised arrival counters
    // dense (non rank-1) kernels with at least this many live stencil phases are evaluated per tile in the frequency
    // domain (conv_fft.hip) instead of by the stencil body; < 0: never (pb_set_dense_eval)
    int fft_min_phases = 16;
    // which tile-spectrum body evaluates them: 1 = one wave per window pair (conv_wfft.hip), 0 = one workgroup per
    // window pair (conv_fft.hip); env PB_FFT_BODY=wg|wave
    int fft_wave = 1;
    // What the host knows about record sets it built itself and read back (pb_make_kernels / pb_set_kernels synchronise
    // anyway): whether any image takes the tile-spectrum body, whether any takes a stencil body -- a reblurring pass then
    // skips the launch nobody needs -- and whose spectra the context's scratch currently holds.  Records estimated on the
    // device (the pipeline) are never in here: their passes issue both launches.
    // any_other = any_strip || any_tile (by body of the fp32 pass); any_fft3 = some image takes the tile-spectrum body step by step.
    // The first set is the choice of body without the one-pass polynomial (every single pass); `poly` = the choice under the
    // PolySpec `spec` (read back the first time a polynomial with that spec meets these records; sel = the device's records)
    struct BodyFlags { bool any_fft = false, any_other = false, any_strip = false, any_tile = false, any_fft3 = false; };
    struct RecFlags { int B; BodyFlags plain; bool poly_valid; PolySpec spec; BodyFlags poly; std::vector<pb_fft_sel> sel; };
    std::map<const void *, RecFlags> rec_cache;
    // Caller-supplied taps that are not point-symmetric (pb_set_kernels): the records hold them as CORRELATION taps -- what
    // F.conv2d applies, filters.py:40-49, method='direct' --, while the reference's method='fft' is a true circular convolution
    // (filters.py:33-36: K = p2o(kernel)), i.e. the point-reflected taps.  The wrap-boundary stage entry points run such records
    // through a reflected copy (api.hip: wrap_records); the host keeps the reflected taps for that.  (The pipeline's own kernels
    // are point-symmetric, or -- even ker_size -- placed per method by the parameter kernel: nothing to reflect there.)
    struct FlipSet { int B; int support; std::vector<float> taps; };
    std::map<const void *, FlipSet> flip_sets;
    int sel_last = 0, sel_B = 0;                         // "conv.fftsel" holds PB_SEL_SLOTS runs of sel_B records: the slot the last pass wrote to / read from (PassWant.slot)
    SpectraSet spectra;                  // what "conv.khat" / "conv.fftsel" hold
    // one-pass polynomial (env PB_POLY1; what a call then wants the spectra to be those of travels with it: PassWant.spec)
    // 0 never; 1 every eligible polynomial, host-built records included (those are then not cached); 2 (default) the
    // pipeline's: mildly blurred images -- the method's own use case -- estimate kernels like sigma 0.6 / rho 0.3 at an
    // oblique angle or the clamped isotropic 0.3 / 0.3, within the 4-sample halo (under the adaptive policy; the latter
    // under full support too, its other taps underflow), and their polynomial is then 1.7 x faster.  Where the first step's
    // launch can take such images along (same output type as the last step's) that costs nothing when no image
    // qualifies; otherwise a composite launch is needed, which finds no work then and costs 1 % of a 4K call even on the
    // side stream (1.182 -> 1.195 ms): issued under the adaptive policy only.
    int poly_mode = 3;
    // A SECOND set of spectra + selections ("conv.khat2" / "conv.fftsel2"), built by the estimation beside the first where the
    // call will need both -- the zero boundary's ring steps want the kernels' own spectra next to the polynomial's, the
    // polynomial behind an edgetaper wants its own next to the kernels' -- instead of by a khat_kernel launch of its own
    // between the estimation and the pass (measured: 23 us per iteration of a 4K method='direct' call, 9 us with edgetaping).
    // What the estimation is asked to build there is an argument of pb_estimate_impl (on == 0 && always == 0: nothing).
    SpectraSet spectra2;
    unsigned sel2_mask = 0;              // iterations (slots of "conv.fftsel2", as of "conv.fftsel") whose polynomial read the SECOND set's selections: pb_body_selection reports those
    long zero_ring_min_pairs = 4096;     // env PB_ZERO_RING_MIN_PAIRS: the window pass + border ring form of a zero-boundary polynomial only for images of at least this many three-step window pairs (40 x 40 tiles, all channels: two rounds of the chip)
    int zero_ring = 1;                   // env PB_ZERO_RING: 0 = a polynomial under the zero boundary (method='direct') keeps three Horner steps over the whole image
    int taper_ring = 1;                  // env PB_TAPER_RING: 0 = every blend of an edgetaper covers the whole padded plane
    int poly_padded = 1;                 // env PB_POLY_PADDED: 0 = a polynomial whose operand is a padded plane (after an edgetaper) keeps three Horner steps
    int est_lean = 1;                    // env PB_EST_LEAN: 0 = the parameter kernel always forms the whole record before the spectra
    DtKnobs dt;                          // env PB_DT_ROWS_REG, PB_DT_COLS_STRIP, PB_DT_COLS_COOP: what the domain transform's choice reads (dt_choice.h)
    int poly_always = 1;                 // env PB_POLY_ALWAYS: 0 = never PolySpec.always (every polynomial issues all the launches its records might need)
    LineKnobs line;                      // env PB_EST_GRAY_ROWS, PB_FFT_EXT_RADIX, PB_FFT_FIRST, PB_FFT_FIRST_ROWS, PB_COLS_FIXED, PB_ROWS_FIXED: what the line transforms' choice reads (line_choice.h)
    // tuning / comparison knobs of single kernels, read once in pb_create (the table of every knob: api.hip, pb_read_knobs)
    size_t phase_budget = 0;             // pb_set_phase_budget: bytes of complex scratch one group of plane pairs of the pure-phase polynomial may take (conv_phase.hip); 0 = 256 MiB.  One pair is always allowed
    int poly_one_launch = 1;             // env PB_POLY_ONE_LAUNCH: 0 = the window pass of a PolySpec.always polynomial as two launches (conv_w128.hip, conv_wfft.hip) instead of one (conv_win.hip); 2 = host-built records take the one launch too (tools/one_launch_timing.py)
    int poly_tall = 1;                   // env PB_POLY_TALL: one-pass images on windows 64 wide and 128 tall -- 0 = never, 1 = where the cost model of khat.h prices them lowest, 2 = every image the form admits
    int strip_mode = 0;                  // env PB_STRIP: 1 = rank-1 kernels of full support take the streaming strip body (fp32 planes; --experimental builds only)
};

int pb_fail(pb_ctx *ctx, int code, const char *fmt, ...);

// RAII bracket: records an event pair around the launches issued in its scope when profiling is on
struct ProfScope {
    pb_ctx *ctx;
    int idx = -1;
    ProfScope(pb_ctx *c, int tag) : ctx(c) {
        if (!c->prof_on) return;
        ProfRec r;
        r.tag = tag;
        hipEvent_t *ev[2] = {&r.a, &r.b};
        for (auto e : ev) {
            if (!c->evpool.empty()) { *e = c->evpool.back(); c->evpool.pop_back(); }
            else if (hipEventCreate(e) != hipSuccess) return;
        }
        (void)hipEventRecord(r.a, c->stream);
        c->prof.push_back(r);
        idx = (int)c->prof.size() - 1;
    }
    ~ProfScope() {
        if (idx >= 0) (void)hipEventRecord(ctx->prof[idx].b, ctx->stream);
    }
};
void *pb_scratch(pb_ctx *ctx, const char *name, size_t bytes);   // nullptr on failure (error set)
const FftPlan *pb_get_plan(pb_ctx *ctx, int n, bool ext_radices = false, int first = 0);   // host_plan(n, ext_radices, first) with its tables on the device
const float *pb_get_interp_weights(pb_ctx *ctx, int n_angles, int n_interp);

#define PB_HIP(call)                                                                          \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return pb_fail(ctx, PB_ERR_HIP, "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                               \
    } while (0)

#define PB_LAUNCH_CHECK()                                                                     \
    do {                                                                                      \
        hipError_t e_ = hipGetLastError();                                                    \
        if (e_ != hipSuccess)                                                                 \
            return pb_fail(ctx, PB_ERR_HIP, "kernel launch failed: %s (%s:%d)",               \
                           hipGetErrorString(e_), __FILE__, __LINE__);                        \
    } while (0)

// ------------------------------------------------------------------------------------
// stencil pass (conv.hip)
// ------------------------------------------------------------------------------------
enum { SRC_VIRTUAL = 0,   // an un-padded H x W plane addressed in padded coordinates (replicate pad by index clamp)
       SRC_PADDED = 1 };  // a materialised Hp x Wp plane
enum { OUT_INTERIOR = 0,  // write the H x W crop into an un-padded plane
       OUT_PADDED = 1 };  // write the whole Hp x Wp domain
enum { EPI_HORNER = 0,    // out = scale * (K*in) + coef * x   [+ clamp]
       EPI_TAPER = 1 };   // out = a * x + (1-a) * (K*in),  a = v1[py] * v2[px]

// per image: which body evaluates a dense kernel (written on the device by khat_kernel, conv_fft.hip)
constexpr int PB_SEL_SLOTS = 16;
constexpr int PB_KHAT_STRIDE = 128 * 128;                  // floats of spectrum per image in "conv.khat": 64 x 64 of them, or 128 x 128 (one pass on 128 x 128 windows)
constexpr int PB_POLY128_MIN_T = 56;                       // smallest tile side of a one-pass 128 x 128 window (bounds the job grid): composite halos up to 36 = 3 x 12, every composite there is
constexpr int PB_POLY_MIN_TX = 24, PB_POLY_MIN_TY = 16;     // smallest tile of a one-pass window (bounds the job grid)
// cost model of the one-pass forms (khat.h; the sweeps: NOTEBOOK.md), what PolySpec.gain / min_area / cost128 are filled from
constexpr float PB_POLY_GAIN = 0.7f;                       // a Horner step costs more than a one-pass window of the same tile (x operand, two launches more)
constexpr int PB_POLY_MIN_AREA = 768;                      // one pass over 768-sample tiles takes what three rank-1 stencil passes take
constexpr int PB_TALL_MIN_AREA = 2 * PB_POLY_MIN_AREA;         // ... and its smallest tile: what the smallest pair of 64 x 64 tiles keeps (the job grid grows no longer than theirs)
constexpr int PB_TALL_MAX_HY = 36;                         // largest row halo of a 64 x 128 window (every composite there is; tiles of at least 56 rows), columns as PB_POLY_MIN_TX
// a window 64 wide and 128 tall in pairs of 64 x 64 ones: measured 1.22 on the headline's second estimate (sigma 1.66 / rho 1.01 at
// 66 degrees, halos 12 / 16; one 4K polynomial, tools/tall_timing.py: 84.4 us for 6624 tall jobs = 12.74 ns a job against 102.1 us
// for 9792 pair jobs = 10.42 ns; a second visit: 77.1 against 95.0 us, 1.20; 1.11 on the third estimate)
constexpr float PB_POLY_COST_TALL = 1.22f;
// what a 128 x 128 window pair costs WITHOUT the launch PB_POLY_COST128 charges it with (measured 6 - 6.5): what the tall form is
// compared with -- it takes no launch off an image's polynomial, the 128 x 128 launch is issued either way.  Measured on the
// headline's first estimate (halos 16 / 20, tools/tall_timing.py): 1500 pairs of 128 x 128 windows 95.8 us, 9000 tall windows 103.7 us
// -- the model keeps the 128 x 128 form there at 6.5 (7.4e-4 against the tall form's 8.7e-4) and would leave it at 8 (9.5e-4)
constexpr float PB_POLY_COST128_BARE = 6.5f;
constexpr float PB_POLY_COST128 = 8.0f;                    // a 128 x 128 window pair in pairs of 64 x 64 (measured 6 - 6.5 at 4K, plus a launch of its own in the pipeline)


struct ConvPass {
    const void *in;  int in_kind;  int in_dtype;  int in_pitch;  long in_plane;
    const void *x;   int x_kind;   int x_dtype;   int x_pitch;   long x_plane;
    void *out;       int out_kind; int out_dtype; int out_pitch; long out_plane;
    int H, W;            // un-padded size; Hp = H + 2*pad, Wp = W + 2*pad
    int pad;             // replicate pad = ker_size / 2 (utils.py:48-53): 12 for the reference's default 25x25 kernel
    int C;               // planes per image
    int P;               // number of planes (B*C)
    const pb_blur_info *info;
    float scale, coef;
    int boundary;
    int epilogue;
    int clamp01;
    int skip_sep;        // rank-1 images are handled by another launch of this step: their tiles exit at once
    int skip_general;    // non-rank-1 images are handled by another launch of this step (conv_xt.hip)
    // tile-spectrum body (conv_fft.hip): per-image selection and kernel spectra (context scratch), filled in by
    // pb_launch_conv; the caller sets khat_ready when an earlier pass on the same stream built them from the same records
    const pb_fft_sel *fsel;
    const float *khat;
    int khat_ready;
    int strip;           // rank-1 images of full support are done by conv_strip.hip's launch of this step: their tiles exit at once
    int poly;            // one-pass polynomial (pb_fft_sel.poly): 0 = those images are skipped (another launch does them); 1 = the
                         // composite pass: only those images; 2 = the first step's launch takes them along -- for them it IS the
                         // composite pass, written to out2 with scale 1, coef 0 and clamp2 (same output type as `out`)
    void *out2;  int out2_kind;  int out2_pitch;  long out2_plane;  int clamp2;
    int no_fft;          // this pass keeps the stencil bodies (pb_launch_conv_poly: some step of the polynomial does not suit the other)
    int ring;            // 0: every tile.  4 / 5: the third / second blend of an edgetaper over the ring its weights differ from 1 on (api.hip:
                         // run_edgetaper).  1 / 2 / 3: Horner step 1 / 2 / 3 of the BORDER RING of a zero-boundary polynomial whose interior
                         // one window pass has done (pb_launch_conv_poly): only the window pairs the frame of outputs within 24 samples of
                         // the padded border depends on (conv_wfft.hip: ring_live)
};

int pb_launch_conv(pb_ctx *ctx, const ConvPass &p, const PassWant &want);
// the three Horner steps of one polynomial (same planes, records and x operand; step s reads what step s - 1 wrote)
int pb_launch_conv_poly(pb_ctx *ctx, const ConvPass *steps, const PassWant &want);
int pb_launch_conv_xt(pb_ctx *ctx, const ConvPass &p);                       // conv_xt.hip
// conv_fft.hip: the spectra want.spec asks for, from either scratch set (out->spec: the spec of the set handed out)
int pb_build_khat(pb_ctx *ctx, const pb_blur_info *info, int B, const PassWant &want, bool launch, Spectra *out);
int pb_build_khat_ring(pb_ctx *ctx, const pb_blur_info *info, int B, const PassWant &want, Spectra *out);   // the kernels' OWN spectra, every symmetric kernel on three-step windows, in the second scratch set (want.slot alone is read)
int pb_khat_buffers(pb_ctx *ctx, int B, const PassWant &want, float **khat, pb_fft_sel **sel);   // the scratch alone (the estimation fills it itself)
int pb_khat2_buffers(pb_ctx *ctx, int B, const PassWant &want, float **khat, pb_fft_sel **sel);  // ... of the second set
int pb_cache_records(pb_ctx *ctx, const pb_blur_info *info, int B);        // conv.hip: after the host (re)built these records
void pb_forget_range(pb_ctx *ctx, const void *dst, size_t bytes);            // a write into device memory: every fact and hint about records it overlaps
inline void pb_forget_records(pb_ctx *ctx, const void *info, int B) { pb_forget_range(ctx, info, sizeof(pb_blur_info) * (size_t)B); }   // B records at info are about to be rewritten
void pb_forget_hints(pb_ctx *ctx);                                           // the record cache and both spectra sets (flip_sets are facts: by range only)
int pb_launch_conv_fft(pb_ctx *ctx, const ConvPass &p);
int pb_launch_conv_strip(pb_ctx *ctx, const ConvPass &p);                    // conv_strip.hip; PB_ERR_UNSUPPORTED: not an all-fp32 plain Horner pass
// spec: the PolySpec p.khat was built under (Spectra.spec).  known: the records' selections where the host has read them -- the job
// grid is then exactly this launch's jobs --, nullptr where it has not: the grid is the longest list the spec admits
int pb_launch_conv_wfft(pb_ctx *ctx, const ConvPass &p, const PolySpec &spec, const std::vector<pb_fft_sel> *known);   // conv_wfft.hip; a pass it is not built for is refused (ask pb_conv_wfft_types / _feasible first)
bool pb_conv_fft_types(const ConvPass &p);                                   // conv_fft.hip: whether the workgroup form is built for the pass's types
bool pb_conv_wfft_types(const ConvPass &p);
int pb_launch_conv_w128(pb_ctx *ctx, const ConvPass &p, const std::vector<pb_fft_sel> *known);   // conv_w128.hip: the one-pass polynomial on 128 x 128 windows (pb_fft_sel.poly == 2)
int pb_launch_conv_win(pb_ctx *ctx, const ConvPass &p, const PolySpec &spec, const std::vector<pb_fft_sel> *known);   // conv_win.hip: the one window pass of every image, 128 x 128 or 64-wide windows by its record, in ONE launch
bool pb_conv_win_types(const ConvPass &p);                                   // ... whether it is built for this composite pass
bool pb_conv_w128_feasible(const ConvPass &p);                               // ... and whether its worst-case job list fits the grid
bool pb_conv_wfft_feasible(const ConvPass &p, bool poly2);                   // conv_wfft.hip: likewise for the wave form
bool pb_conv_w128_types(int in_dtype, int out_dtype);                                  // ... whether it is built for the pass's types
bool pb_poly_three_steps_ok(pb_ctx *ctx, const ConvPass *steps);             // conv.hip: the three steps can all take the wave form (PolySpec.always == 2)
int pb_poly_spec_mode(pb_ctx *ctx, const ConvPass *steps);                   // conv.hip: the PolySpec.on a polynomial with these steps may ask for
// kernels larger than the 25 x 25 record (conv_big.hip): their taps on the ker_size grid, and one Horner step with them
// BigTaps: one table of PB_BIG_TABLE floats per image (49 rows of 56: entry [iy + 24][ix + 24] multiplies the sample (iy, ix) away
// from the output, zero outside the support), PB_BIG_ACORR floats of autocorrelations per image (the edgetaper's weights), and
// the half-sizes the pass walks: kernel rows -ry .. ry, taps -rx .. rx of each
constexpr int PB_KSIZE_MAX = 49;
constexpr int PB_BIG_TABLE = PB_KSIZE_MAX * 56, PB_BIG_ACORR = 2 * 64;
struct BigTaps { const float *taps = nullptr, *acorr = nullptr; int ry = 0, rx = 0; };
int pb_build_big_taps(pb_ctx *ctx, const pb_blur_info *dev_info, int B, int ksize, int shift, BigTaps *big);
// the same tables from a caller's kh x kw taps (B * kh * kw floats on the device): `zero` placed by F.conv2d's 'same' rule,
// `wrap` the taps reflected inside their own array, then placed by p2o's roll; `acorr` serves both
int pb_build_caller_taps(pb_ctx *ctx, const float *dev_raw, int B, int kh, int kw, float *zero, float *wrap, float *acorr);
int pb_launch_conv_big(pb_ctx *ctx, const ConvPass &p, const BigTaps &big);
bool pb_conv_fft_feasible(const ConvPass &p);                                // window counts within the kernel's index arithmetic
// the polynomial with the pure-phase filter (conv_phase.hip; deblurring.py:141-169 with not_symmetric=True): one transform over
// the whole (H + 2 pad) x (W + 2 pad) domain.  src: (B,C) planes of src_dtype -- un-padded H x W ones addressed in padded
// coordinates (src_virtual: replicate pad by index clamp) or materialised padded ones --; dst: the (B,C,H,W) interior of dst_dtype;
// taps: B raw kh x kw kernels in device memory, placed as p2o places them
struct PhaseCall {
    const void *src; int src_dtype; int src_virtual; int src_pitch; long src_plane;
    void *dst; int dst_dtype; int clamp01;
    int B, C, H, W, pad;
    const float *taps; int kh, kw;
    float alpha, beta;
};
int pb_launch_phase(pb_ctx *ctx, const PhaseCall &c);
int pb_phase_sides_supported(pb_ctx *ctx, int Hp, int Wp);                   // PB_ERR_UNSUPPORTED (message set) unless both sides' lines fit LDS
// its backward (conv_phase_grad.hip): x, grad_out, grad_x (B,C,H,W) fp32 planes that are the whole domain, grad_taps (B,kh,kw);
// grad_x or grad_taps may be null (not computed), not both; x may be null without grad_taps
struct PhaseGradCall {
    const float *x, *grad_out; float *grad_x, *grad_taps;
    int B, C, H, W;
    const float *taps; int kh, kw;
    float alpha, beta;
};
int pb_launch_phase_backward(pb_ctx *ctx, const PhaseGradCall &c);

// the gradient of a pass with respect to its taps (conv_grad.hip): grad[b][i][j] (= or +=, `accumulate`) scale * the lag
// correlation of u with v over the C planes of image b -- (B,C,H,W) fp32 planes that are the whole domain, kh and kw odd, v zero
// outside the domain (PB_ZERO) or circular over it (PB_WRAP), taps indexed as pb_taps_create places them under that boundary.
// Partial tables in the scratch "grad.partial": B * pb_tap_gradient_groups * kh * kw floats
int pb_launch_tap_gradient(pb_ctx *ctx, const float *u, const float *v, int B, int C, int H, int W, int kh, int kw, int boundary,
                           float scale, int accumulate, float *grad);
int pb_tap_gradient_groups(int B, int C, int H, int W);

// the gradient of the polynomial with respect to alpha and beta (poly_param_grad.hip): grad_params[b] =
// (1/2 sum G (u2 - u3), sum G u3) over the n = C * H * W samples of image b, u2 and u3 the second and third detail image of x
// (api.hip forms them).  B up to 65535.  Partials in the scratch "ppg.partial": 2 * B * pb_poly_param_groups doubles
int pb_launch_poly_param_reduce(pb_ctx *ctx, const float *grad_out, const float *u2, const float *u3, float *grad_params, int B, long n);
int pb_poly_param_groups(int B, long n);

// the backward of an edgetaper blend (edgetaper_grad.hip).  TaperAcorr: where the forward reads the kernel's
// two autocorrelations -- image b's at acy + b * stride and acx + b * stride, nlag lags stored (25 in a record, 49 in a table).
struct TaperAcorr { const float *acy, *acx; long stride; int nlag; };
// one blend: u = (1 - A) g, ag = A g, and -- abar not null -- abar[b] (= when first, += otherwise) the sum over the image's C
// planes of g (x - kx), kx = K x.  (B,C,H,W) fp32 planes that are the whole domain; abar: B planes of H x W
int pb_launch_taper_blend_adjoint(pb_ctx *ctx, const TaperAcorr &ac, const float *x, const float *kx, const float *g, float *u, float *ag,
                                  float *abar, int first, int B, int C, int H, int W);
// abar -> vbar ("etg.vbar", B * (H + W) floats: the ring's rows, then its columns) -> kbar_y, kbar_x; grad_taps[b][i][j] +=
// kbar_y[i] + kbar_x[j].  raw: the B kh x kw kernels as the caller gave them (device)
int pb_launch_taper_weight_chain(pb_ctx *ctx, const TaperAcorr &ac, const float *abar, const float *raw, int kh, int kw, int B, int H, int W,
                                 float *grad_taps);

// ------------------------------------------------------------------------------------
// estimation (estimate.hip)
// ------------------------------------------------------------------------------------
constexpr int kMaxLineLength = 65536;          // longest line of the spectral derivative (pb_fft_length_supported, estimate.hip)
// spec1 / spec2: the PolySpec the spectra the estimation builds into the first / second scratch set are those of (spec2 with
// on == 0 && always == 0: no second set); slot: the slot of the selection scratch they go to (PassWant)
int pb_estimate_impl(pb_ctx *ctx, const void *in, int dtype, int B, int C, int H, int W,
                     const pb_options *opt, pb_blur_info *dev_info, const PolySpec &spec1, const PolySpec &spec2, int slot);
int pb_make_sep_records(pb_ctx *ctx, int B, const pb_blur_info *dev_info, pb_blur_info *sep, int support, int ksize);
int pb_kernel_size(const pb_options *opt);      // validated ker_size (2 .. PB_KSIZE_MAX; above PB_KSIZE: conv_big.hip's path); 0 if unsupported
int pb_fourier_gradients_impl(pb_ctx *ctx, const float *planes, int P, int H, int W, float *gx, float *gy);
int pb_fourier_gradients_typed(pb_ctx *ctx, const float *planes, int P, int H, int W, void *gx, void *gy, int out_dtype);   // PB_F16: __half planes out
bool pb_gradient_planes_half(pb_ctx *ctx, int H, int W);       // whether this context's line transforms can write __half planes for H x W
int pb_make_kernels_dev(pb_ctx *ctx, int B, pb_blur_info *dev_info, int support, int from_taps, int ksize = PB_KSIZE);

// ------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------
template <typename T> __device__ __forceinline__ float pb_ld(const T *p);
template <> __device__ __forceinline__ float pb_ld<float>(const float *p) { return *p; }
template <> __device__ __forceinline__ float pb_ld<__half>(const __half *p) { return __half2float(*p); }
// (the conversions are never contracted into a neighbouring FMA, so the fused edge computes exactly what the
// float pipeline computes between host-side conversions)
// 8-bit pixels: img_as_float32 on load, img_as_ubyte on store (skimage 0.19.2 util/dtype.py _convert)
__device__ __forceinline__ float pb_from_ubyte(unsigned u) {
    float r = (float)u * (1.0f / 255.0f);
    asm("" : "+v"(r));                   // keeps the product from being contracted into a neighbouring FMA (not volatile:
                                         // volatile statements keep their order, and with it the loads that feed them one
                                         // behind the other -- 128 byte loads of a window column, each waited for)
    return r;
}
template <> __device__ __forceinline__ float pb_ld<unsigned char>(const unsigned char *p) { return pb_from_ubyte(*p); }
template <typename T> __device__ __forceinline__ void pb_st(T *p, float v);
__device__ __forceinline__ unsigned pb_to_ubyte(float v) { return (unsigned)__float2int_rn(fminf(fmaxf(__fmul_rn(v, 255.f), 0.f), 255.f)); }
template <> __device__ __forceinline__ void pb_st<unsigned char>(unsigned char *p, float v) { *p = (unsigned char)pb_to_ubyte(v); }
template <> __device__ __forceinline__ void pb_st<float>(float *p, float v) { *p = v; }
template <> __device__ __forceinline__ void pb_st<__half>(__half *p, float v) { *p = __float2half_rn(v); }

// four consecutive samples as floats: one access of 16 bytes (fp32), 8 (fp16) or 4 (8-bit), on a boundary of that size
template <typename T> __device__ __forceinline__ float4 pb_ld4(const T *p);
template <> __device__ __forceinline__ float4 pb_ld4<float>(const float *p) { return *reinterpret_cast<const float4 *>(p); }
template <> __device__ __forceinline__ float4 pb_ld4<__half>(const __half *p) {
    const uint2 u = *reinterpret_cast<const uint2 *>(p);
    const __half2 a = *reinterpret_cast<const __half2 *>(&u.x), b = *reinterpret_cast<const __half2 *>(&u.y);
    const float2 fa = __half22float2(a), fb = __half22float2(b);
    return make_float4(fa.x, fa.y, fb.x, fb.y);
}
template <> __device__ __forceinline__ float4 pb_ld4<unsigned char>(const unsigned char *p) {
    const unsigned u = *reinterpret_cast<const unsigned *>(p);
    return make_float4(pb_from_ubyte(u & 255u), pb_from_ubyte((u >> 8) & 255u), pb_from_ubyte((u >> 16) & 255u), pb_from_ubyte(u >> 24));
}
template <typename T> __device__ __forceinline__ void pb_st4(T *p, float4 v);
template <> __device__ __forceinline__ void pb_st4<unsigned char>(unsigned char *p, float4 v) {
    *reinterpret_cast<unsigned *>(p) = pb_to_ubyte(v.x) | (pb_to_ubyte(v.y) << 8) | (pb_to_ubyte(v.z) << 16) | (pb_to_ubyte(v.w) << 24);
}
template <> __device__ __forceinline__ void pb_st4<float>(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }
template <> __device__ __forceinline__ void pb_st4<__half>(__half *p, float4 v) {
    const __half2 a = __floats2half2_rn(v.x, v.y), b = __floats2half2_rn(v.z, v.w);
    uint2 u;
    u.x = *reinterpret_cast<const unsigned *>(&a);
    u.y = *reinterpret_cast<const unsigned *>(&b);
    *reinterpret_cast<uint2 *>(p) = u;
}

// One wave per output folds that output's `per_out` partial sums (pb_block_sum_to_first's, stage_math.h) in a fixed order:
// out[blockIdx.x] = sum of partial[blockIdx.x * per_out ..], bit-reproducible.  Launched on 64 threads; defined in filters.hip
__global__ __launch_bounds__(64) void pb_fold_partials_kernel(const float *__restrict__ partial, float *__restrict__ out, int per_out);

// order-preserving float <-> uint encoding for atomicMin/atomicMax on floats
__device__ __forceinline__ unsigned pb_f2ord(float f) {
    unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float pb_ord2f(unsigned u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
