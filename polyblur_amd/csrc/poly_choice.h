// What one reblurring call issues (conv.hip): every launch of a single pass (pb_launch_conv) or of the three Horner steps of a
// polynomial (pb_launch_conv_poly), in order, with the stream each goes to -- chosen ONCE per call, from facts the launcher
// gathers before its first launch, by choose_pass / choose_poly; the launchers issue the plan in one loop and pb_debug_poly_plan
// hands it out.  Host code without a HIP call or type, a context, a pass or a device pointer.  tests/test_poly_choice_cpu.py sweeps
// it through the query and holds the plans against tests/golden/poly_plans.json; tools/poly_choice_sweep.cpp is the sweep as a
// program of its own.  DESIGN 4.1 has the table of forms.
#pragma once

// Everything the choosers read, all ints (pb_debug_poly_plan takes them as an array in this order).  Arrays are per Horner step;
// a single pass is step 0.
struct PolyFacts {
    // the context's knobs
    int fft_on;             // pb_ctx.fft_min_phases >= 0: dense kernels may take the tile-spectrum body
    int fft_wave;           // pb_ctx.fft_wave
    int poly_one_launch;    // pb_ctx.poly_one_launch: 0 / 1 / 2
    int strip_mode;         // pb_ctx.strip_mode (--experimental builds)
    int aux;                // the side stream exists
    int prof_on;            // per-launch profiling: everything stays on one stream
    // the steps
    int step_ok[3];         // fft_pass_ok: what the tile-spectrum body needs of the pass
    int wave_types[3];      // pb_conv_wfft_types
    int wave_fits[3];       // pb_conv_wfft_feasible(p, false)
    int wg_types[3];        // pb_conv_fft_types
    int strip_pass[3];      // all-fp32 plain Horner pass with the full pad, rank-1 images not skipped: what the strip body takes
    // the composite pass (first step's input to last step's output)
    int whole_ok, whole_wave_types, whole_wave_fits, whole_wg_types, whole_win_types;
    // the spec (PassWant.spec)
    int on, always;
    // the call
    int zero;               // boundary == PB_ZERO
    int fold;               // first and last step store the same type
    int no_fft, khat_ready, ring, poly;      // of the single pass (ConvPass); the steps of a polynomial come with 0
    int side_tiles;         // at least 12288 stencil tiles: the launches that may find no work are worth a side stream
    // what the host has read of the records under the spec (known_flags)
    int have, any_fft, any_other, any_strip, any_tile, any_fft3;
    int ksel;               // ... and their selections (one-pass spec): exact job grids
    // the first scratch set of spectra
    int held, by_estimate;  // SpectraSet.holds(info, B), and by the estimation
    int spectra;            // what pb_build_khat will do: PB_SPECTRA_*
};
constexpr int PB_POLY_NFACTS = sizeof(PolyFacts) / sizeof(int);
// stencil tiles (64 x 64, every plane) from which the launches that may find no work go to the side stream: two queue-to-queue waits
// per polynomial (~5 - 8 us each) against launches of 6 us at 4K (6405 tiles) and 33 us for 32 x 1080p (53568) -- measured: 4K 0.738 ->
// 0.722 ms of device time per call on one stream, 32 x 1080p 6.09 -> 6.61 ms without the side stream
constexpr long PB_POLY_MIN_SIDE_TILES = 12288;

enum { PB_SPECTRA_READY = 0,        // the first set holds the spec's spectra in the pass's slot: launched only where the op says so
       PB_SPECTRA_STALE = 1,        // it does not: every build launches
       PB_SPECTRA_SECOND = 2 };     // the second set holds them (the estimation built them there): handed out, nothing launched or claimed

enum { PB_OP_BUILD = 1,             // pb_build_khat; arg = its `launch` argument
       PB_OP_BUILD_RING = 2,        // pb_build_khat_ring
       PB_OP_DROP = 3,              // SpectraSet.drop(): device-built records took a pass without spectra
       PB_OP_STENCIL = 4,           // launch_stencil
       PB_OP_WAVE = 5,              // pb_launch_conv_wfft
       PB_OP_WG = 6,                // pb_launch_conv_fft
       PB_OP_W128 = 7,              // pb_launch_conv_w128
       PB_OP_WIN = 8,               // pb_launch_conv_win
       PB_OP_STRIP = 9,             // pb_launch_conv_strip (it may answer "not this pass")
       PB_OP_FORK = 10, PB_OP_JOIN = 11,
       PB_OP_FAIL = 12,             // arg = the message; always the last op, and then nothing of the plan is issued
       PB_OP_KINDS = 13 };
enum { PB_PASS_WHOLE = 3 };         // PolyOp.step: the composite pass
enum { PB_SET_NONE = 0, PB_SET_FIRST = 1, PB_SET_RING = 2 };       // whose khat / fsel the pass gets: the last BUILD's, the BUILD_RING's
enum { PB_WHEN_ALWAYS = 0, PB_WHEN_STRIP_REFUSED = 1 };            // a stencil launch that is needed only if the strip body declined
enum { PB_MSG_THREE_STEPS = 0, PB_MSG_RING = 1, PB_MSG_PER_AXIS = 2, PB_MSG_COMPOSITE = 3, PB_MSG_WG_TYPES = 4, PB_MSG_COUNT = 5 };
constexpr const char *PB_POLY_MSG[PB_MSG_COUNT] = {
    "three window steps: the wave form does not take this pass",
    "zero-boundary ring: the wave form does not take this pass",
    "one-pass polynomial with per-axis halos: the wave form does not take this pass",
    "one-pass polynomial: composite pass not feasible",
    "tile-spectrum pass: unsupported dtype combination %d" };

struct PolyOp {
    unsigned char kind, step, poly, ring;     // step: 0 - 2 or PB_PASS_WHOLE; poly, ring: ConvPass.poly / .ring of the launch
    unsigned char side, known, set, arg;      // side stream; the known selections or nullptr; PB_SET_*; launch flag / message / PB_WHEN_*
};
constexpr int PB_POLY_OP_INTS = 8;
constexpr int PB_POLY_MAX_OPS = 16;           // the longest plan there is (tools/poly_choice_sweep.cpp): step by step with the 128 x 128 launch, the strip body and the composite

struct PolyPlan {
    int n = 0;
    bool overflow = false;
    PolyOp op[PB_POLY_MAX_OPS];
    bool failed() const { return n && op[n - 1].kind == PB_OP_FAIL; }
    void add(int kind, int step = 0, int poly = 0, int ring = 0, int side = 0, int known = 0, int set = 0, int arg = 0) {
        if (failed()) return;
        if (n == PB_POLY_MAX_OPS) { overflow = true; return; }
        op[n++] = PolyOp{(unsigned char)kind, (unsigned char)step, (unsigned char)poly, (unsigned char)ring,
                         (unsigned char)side, (unsigned char)known, (unsigned char)set, (unsigned char)arg};
    }
    void append(const PolyPlan &o) { for (int i = 0; i < o.n; ++i) add(o.op[i].kind, o.op[i].step, o.op[i].poly, o.op[i].ring, o.op[i].side, o.op[i].known, o.op[i].set, o.op[i].arg); }
    void fail(int msg, int step = 0) { add(PB_OP_FAIL, step, 0, 0, 0, 0, 0, msg); }
};

namespace poly_choice {

// pb_build_khat, and what it leaves in the first scratch set
inline void build(PolyPlan &pl, PolyFacts &f, bool launch, int side = 0) {
    pl.add(PB_OP_BUILD, 0, 0, 0, side, 0, 0, launch);
    if (f.spectra == PB_SPECTRA_SECOND) return;
    if (launch || f.spectra == PB_SPECTRA_STALE) { f.held = 1; f.by_estimate = 0; f.spectra = PB_SPECTRA_READY; }
}

// The tile-spectrum launch of a pass: the wave form where it is built and worth it, else the workgroup form -- which cannot run
// one-pass images whose composite halo is beyond its classes (PolySpec.on == 2 is only asked for where the wave form takes
// every launch, pb_poly_spec_mode).  (A one-pass launch whose job list is too long is refused by the wave launcher itself.)
inline void tile_spectrum(PolyPlan &pl, const PolyFacts &f, int step, int poly, int ring, int side, int known, int set) {
    const bool whole = step == PB_PASS_WHOLE, per_axis = poly != 0 && f.on >= 2;
    const bool types = whole ? f.whole_wave_types : f.wave_types[step], fits = whole ? f.whole_wave_fits : f.wave_fits[step];
    if (f.fft_wave && types && (per_axis || fits)) return pl.add(PB_OP_WAVE, step, poly, ring, side, known, set);
    if (per_axis) return pl.fail(PB_MSG_PER_AXIS, step);
    if (!(whole ? f.whole_wg_types : f.wg_types[step])) return pl.fail(PB_MSG_WG_TYPES, step);
    pl.add(PB_OP_WG, step, poly, ring, side, 0, set);
}

// the composite launch of the images with a one-pass record (grid for the longest job list the spec admits)
inline void composite(PolyPlan &pl, const PolyFacts &f, int side) {
    if (!f.whole_ok) return pl.fail(PB_MSG_COMPOSITE, PB_PASS_WHOLE);
    tile_spectrum(pl, f, PB_PASS_WHOLE, 1, 0, side, 0, PB_SET_FIRST);
}

// One pass: each image's record decides on the device which body evaluates its tiles, so a pass issues the stencil launch and
// -- where dense kernels may take it -- the tile-spectrum launch; for records the host has read, only the launches some image needs.
inline void pass(PolyPlan &pl, PolyFacts &f, int s, int poly, int ring, bool khat_ready, bool no_fft) {
    bool fft = f.fft_on && !no_fft && f.step_ok[s];
    // (a step of a polynomial whose one-pass images another launch does: only the images that go step by step count)
    if (fft && f.have && !(f.on && poly == 0 ? f.any_fft3 : f.any_fft)) fft = false;
    int set = PB_SET_NONE;
    if (fft || (f.have && f.on)) {
        // (spectra an earlier pass built count only while the scratch still holds them for these records; the stencil bodies
        // read the selection too: they skip the one-pass images)
        build(pl, f, !((khat_ready || f.have || f.by_estimate) && f.held));
        set = PB_SET_FIRST;
    } else if (!khat_ready && !f.have) {
        pl.add(PB_OP_DROP);
        f.held = 0; f.by_estimate = 0; f.spectra = PB_SPECTRA_STALE;
    }
    // rank-1 kernels of full support on fp32 planes: the streaming strip body (host-built records only)
    const bool strip = f.strip_mode && f.have && f.any_strip && f.strip_pass[s];
    if (strip) pl.add(PB_OP_STRIP, s, poly, ring, 0, 0, set);
    // (PolySpec.always == 2, records of the estimation: every image takes the window form -- no stencil launch to find that out)
    const bool windows_only = !f.have && fft && !f.on && f.always == 2 && f.fft_wave && f.wave_types[s] && f.wave_fits[s];
    // (any_other = any_strip || any_tile: where the strip body takes its images, the stencil launch is for the others)
    if (!windows_only && (!f.have || f.any_other))
        pl.add(PB_OP_STENCIL, s, poly, ring, 0, 0, set, strip && !f.any_tile ? PB_WHEN_STRIP_REFUSED : PB_WHEN_ALWAYS);
    if (fft) tile_spectrum(pl, f, s, poly, ring, 0, f.ksel, set);
}

// the one window pass of every image (PolySpec.always): one launch carrying both window forms where conv_win.hip is built for the
// composite's types; else the 128 x 128 launch and the 64-wide one, each skipping the other's images
inline void window_pass(PolyPlan &pl, const PolyFacts &f, bool fold) {
    if (f.poly_one_launch && f.fft_wave && f.on == 3 && f.whole_win_types) {
        if (!f.whole_ok) return pl.fail(PB_MSG_COMPOSITE, PB_PASS_WHOLE);
        return pl.add(PB_OP_WIN, PB_PASS_WHOLE, 1, 0, 0, 0, PB_SET_FIRST);
    }
    if (f.on == 3) pl.add(PB_OP_W128, PB_PASS_WHOLE, 1, 0, 0, f.ksel, PB_SET_FIRST);
    if (f.whole_wave_types) return composite(pl, f, 0);
    tile_spectrum(pl, f, 0, fold ? 2 : 0, 0, 0, 0, PB_SET_FIRST);    // (the composite's types are not built: the first step's launch takes them along)
}

// Horner step s + 1 of the border ring of a zero-boundary polynomial
inline void ring_step(PolyPlan &pl, const PolyFacts &f, int s, int side) {
    if (!(f.wave_types[s] && f.wave_fits[s])) return pl.fail(PB_MSG_RING, s);
    pl.add(PB_OP_WAVE, s, 0, s + 1, side, 0, PB_SET_RING);
}

}  // namespace poly_choice

inline PolyPlan choose_pass(PolyFacts f) {
    PolyPlan pl;
    poly_choice::pass(pl, f, 0, f.poly, f.ring, f.khat_ready != 0, f.no_fft != 0);
    return pl;
}

// The three Horner steps of one polynomial.  Whether the tile-spectrum body may be used is decided once, from all three
// geometries.  The forms, first match:
inline PolyPlan choose_poly(PolyFacts f) {
    using namespace poly_choice;
    PolyPlan pl;
    const bool fft = f.fft_on && f.step_ok[0] && f.step_ok[1] && f.step_ok[2];
    // 1. PolySpec.always == 2 (records of the estimation): every image on three window steps, three launches of the wave body
    if (fft && !f.on && f.always == 2 && !f.have) {
        build(pl, f, !f.by_estimate);
        for (int s = 0; s < 3; ++s) {
            if (!(f.wave_types[s] && f.wave_fits[s])) pl.fail(PB_MSG_THREE_STEPS, s);
            pl.add(PB_OP_WAVE, s, 0, 0, 0, 0, PB_SET_FIRST);
        }
        return pl;
    }
    const bool poly_on = fft && f.on, fold = poly_on && f.fold;
    const int first = fold ? 2 : 0;        // ConvPass.poly of the first step's launches: it takes the one-pass images along
    // 2. PolySpec.always (records of the estimation): every image takes one window pass and nothing else.  Under the zero boundary
    // the frame within 24 samples of the padded border is recomputed by three ring steps; the first two touch neither the output
    // nor the first set of spectra and run on the side stream beside the window pass
    if (poly_on && f.always && !f.have) {
        build(pl, f, !f.by_estimate);
        PolyPlan win;
        window_pass(win, f, fold);
        if (!f.zero || win.failed()) { pl.append(win); return pl; }      // (a refused window pass is what the call reports, whatever the ring steps say)
        const int side = f.aux && !f.prof_on;
        if (side) pl.add(PB_OP_FORK); else pl.append(win);
        pl.add(PB_OP_BUILD_RING, 0, 0, 0, side);
        ring_step(pl, f, 0, side); ring_step(pl, f, 1, side);
        if (side) { pl.append(win); pl.add(PB_OP_JOIN); }
        ring_step(pl, f, 2, 0);
        return pl;
    }
    // 3. the lab switch of tools/one_launch_timing.py: host-built records whose every image takes one window pass go through the
    // merged launch too, with the exact grid
    if (poly_on && f.have && f.poly_one_launch == 2 && f.fft_wave && f.on == 3 && !f.zero && f.ksel && f.any_fft && !f.any_other &&
        !f.any_fft3 && f.whole_win_types) {
        build(pl, f, !f.held);
        if (!f.whole_ok) pl.fail(PB_MSG_COMPOSITE, PB_PASS_WHOLE);
        pl.add(PB_OP_WIN, PB_PASS_WHOLE, 1, 0, 0, 1, PB_SET_FIRST);
        return pl;
    }
    // 4. step by step on the caller's stream: no tile-spectrum body, records the host has read, few stencil tiles, or profiling
    if (!fft || f.have || !(f.aux && f.side_tiles) || f.prof_on) {
        if (fft && f.on == 3) {     // the images whose one pass runs on 128 x 128 windows: a launch of their own
            build(pl, f, !(f.held && (f.have || f.by_estimate)));
            pl.add(PB_OP_W128, PB_PASS_WHOLE, 1, 0, 0, f.ksel, PB_SET_FIRST);
        }
        for (int s = 0; s < 3; ++s) pass(pl, f, s, s == 0 ? first : 0, 0, s > 0, !fft);
        if (poly_on && !fold) {     // images with a one-pass record wait for this launch, on the spectra the steps have just used
            build(pl, f, false);
            composite(pl, f, 0);
        }
        return pl;
    }
    // 5. records the host has not read, many stencil tiles: the launches that probably find no work go to the side stream.  Where
    // the spec admits 128 x 128 windows the 128 x 128 launch stays on the caller's stream and the wave body's three launches
    // join the stencil launches; otherwise the wave body's stay
    build(pl, f, !f.by_estimate);
    const bool w128_main = poly_on && f.on == 3;
    pl.add(PB_OP_FORK);
    if (poly_on && !fold) composite(pl, f, 1);
    for (int s = 0; s < 3 && w128_main; ++s) tile_spectrum(pl, f, s, s == 0 ? first : 0, 0, 1, 0, PB_SET_FIRST);
    for (int s = 0; s < 3; ++s) pl.add(PB_OP_STENCIL, s, 0, 0, 1, 0, PB_SET_FIRST);
    if (w128_main) pl.add(PB_OP_W128, PB_PASS_WHOLE, 1, 0, 0, f.ksel, PB_SET_FIRST);
    else for (int s = 0; s < 3; ++s) tile_spectrum(pl, f, s, s == 0 ? first : 0, 0, 0, 0, PB_SET_FIRST);
    pl.add(PB_OP_JOIN);
    return pl;
}
