// What runs for one line transform of the estimation (the row and column FFT-derivative passes of estimate.hip and
// lines_fixed.hip): plan, tile, threads and kernel, chosen ONCE per launch by choose_rows / choose_cols and read by the
// launchers, by pb_estimate_impl (the partial maxima per image), by pb_gradient_planes_half and by pb_debug_line_choice.
// Host code without a HIP call or type: the table of compiled plans, the host half of a plan (factorize, the first-radix
// rotation, the Bluestein core) and the two choosers.  tests/test_line_choice_cpu.py sweeps them through the query and holds
// the answers against tests/golden/line_choices.json; tools/line_choice_sweep.cpp is the same sweep as a program of its own.
#pragma once
#include <algorithm>
#include <functional>
#include <map>
#include <vector>

// The knobs the choice reads (pb_ctx.line; api.hip: pb_read_knobs has the table of every knob)
struct LineKnobs {
    int est_gray_rows = 1;      // env PB_EST_GRAY_ROWS: 1 = gray + range + row transform in one launch where measured faster (fp32 planes, lines of up to 4096 samples), 2 = for any line held in LDS, 0 = never
    int fft_ext_radix = 1;      // env PB_FFT_EXT_RADIX: 0 = greedy plans only (radices up to 16)
    int fft_first = -1;         // env PB_FFT_FIRST: the radix of the column transform's first / last stage where the plan holds it; 0 = the plan's own order; -1 = chosen by trips (choose_cols)
    int fft_first_rows = -1;    // env PB_FFT_FIRST_ROWS: the same for the row transforms (choose_rows)
    int cols_fixed = 1;         // env PB_COLS_FIXED: 0 = the column transform always by the run-time-plan kernel (grad_cols_kernel), also where lines_fixed.hip holds the plan
    int rows_fixed = 1;         // env PB_ROWS_FIXED: the same for the row transforms (gray_rows_kernel / grad_rows_kernel)
};

// ------------------------------------------------------------------------------------
// FFT plans (host half)
// ------------------------------------------------------------------------------------
struct HostPlan {
    int n = 0;
    int nstage = 0;
    int radix[24] = {};
    int bluestein_m = 0;          // 0: direct mixed-radix; else the power-of-two length used
};
typedef std::map<int, HostPlan> HostPlans;       // one per (length, ext / greedy, first radix): host_plan's memo

inline void factorize(int n, std::vector<int> &radix, int &rest, bool ext_ok = false) {
    // greedy: the largest in-register radix that divides what is left (fewer LDS passes and barriers)
    static const int pref[] = {16, 15, 12, 10, 9, 8, 6, 5, 4, 7, 3, 2};
    radix.clear();
    const int n0 = n;
    bool found = true;
    while (n > 1 && found) {
        found = false;
        for (int r : pref)
            if (n % r == 0) { radix.push_back(r); n /= r; found = true; break; }
    }
    rest = n;
    // Lines held in LDS: where radices 18 / 20 / 24 save a stage over the greedy plan (4320 = 16 x 15 x 9 x 2 -> 18 x 16 x 15,
    // 7680 = 16 x 16 x 15 x 2 -> 24 x 20 x 16: two LDS round trips and barriers fewer per line), the plan with the fewest
    // stages and, among those, the smallest sum of radices; every other length keeps its greedy plan.
    if (!ext_ok || rest != 1 || (long)n0 * 8 > 160 * 1024 || radix.size() < 3) return;
    static const int ext[] = {24, 20, 18, 16, 15, 12, 10, 9, 8, 6, 5, 4, 7, 3, 2};
    std::vector<int> best, cur;
    int best_sum = 0;
    const size_t limit = radix.size() - 1;                // only plans with fewer stages are of interest
    std::function<void(int, int, int)> dfs = [&](int left, int max_r, int sum) {
        if (left == 1) {
            if (best.empty() || cur.size() < best.size() || (cur.size() == best.size() && sum < best_sum)) { best = cur; best_sum = sum; }
            return;
        }
        if (cur.size() >= limit || (!best.empty() && cur.size() >= best.size())) return;
        for (int r : ext) {
            if (r > max_r || left % r) continue;
            cur.push_back(r);
            dfs(left / r, r, sum + r);
            cur.pop_back();
        }
    };
    dfs(n0, 24, 0);
    if (best.empty() || best.size() >= radix.size()) return;
    // order: the first radix is the one of the stages that talk to global memory (and, in the column kernel, carry the
    // epilogue's prefetched operands): the largest one up to 16, as in the greedy plans; the rest ascending, so that the
    // widest butterfly is the innermost stage, which has no twiddles to hold
    std::sort(best.begin(), best.end());
    int first = -1;
    for (int i = (int)best.size() - 1; i >= 0; --i) if (best[i] <= 16) { first = i; break; }
    if (first > 0) std::rotate(best.begin(), best.begin() + first, best.begin() + first + 1);
    radix = best;
}

// (two plans per length: the kernel variants without the radices above 16 take the greedy one; and one per first radix asked for)
inline int plan_key(int n, bool ext_radices, int first) { return (ext_radices ? -1 : 1) * (n + (first << 17)); }

// The plan of n-sample lines.  ext_radices: the caller's kernel holds radices 18 / 20 / 24; first: the radix (one of the
// plan's) of the stages that talk to global memory, 0 = the plan's own order.  nstage == 0: more stages than a plan holds.
inline const HostPlan &host_plan(HostPlans &memo, const LineKnobs &k, int n, bool ext_radices, int first) {
    const int key = plan_key(n, ext_radices, first);
    auto it = memo.find(key);
    if (it != memo.end()) return it->second;
    HostPlan pl;
    pl.n = n;
    std::vector<int> radix;
    int rest = 1;
    factorize(n, radix, rest, ext_radices && k.fft_ext_radix != 0);
    if (rest != 1) {               // Bluestein with a power-of-two core
        int core = 1;
        while (core < 2 * n - 1) core *= 2;
        pl.bluestein_m = core;
        factorize(core, radix, rest);
    }
    if (first > 0 && !pl.bluestein_m) {
        auto f = std::find(radix.begin(), radix.end(), first);
        if (f != radix.end()) std::rotate(radix.begin(), f, f + 1);
    }
    if (radix.size() <= 24) {
        pl.nstage = (int)radix.size();
        for (int i = 0; i < pl.nstage; ++i) pl.radix[i] = radix[i];
    }
    return memo.emplace(key, pl).first->second;
}

// ------------------------------------------------------------------------------------
// The compiled plans (lines_fixed.hip instantiates exactly these rows; the _has functions below answer from the same rows)
// ------------------------------------------------------------------------------------
// Columns: line length = R0 x R1 x R2 in the order choose_cols gives it (smallest radix from 5 up -- or the one whose
// butterflies are one trip -- first), with the two tile widths (lognb) choose_cols can give that length: NARROW on 512 threads
// (two workgroups per CU) and WIDE on 1024 (one), 0 = that width does not occur.  The BASELINE lengths first; then the common
// picture sizes (720p, 1440p, 2K ...), where the same kernels run 1.3 - 2 x faster than the run-time-plan ones.
#define PB_COLS_PLANS(X)                                                                          \
    X(2160, 9, 16, 15, 2, 3) X(1080, 6, 15, 12, 3, 4) X(4320, 15, 16, 18, 1, 2)                    \
    X(512, 2, 16, 16, 3, 4) X(640, 4, 16, 10, 3, 4) X(720, 3, 16, 15, 3, 4) X(768, 3, 16, 16, 3, 4) \
    X(800, 5, 16, 10, 3, 4) X(960, 4, 16, 15, 3, 4) X(1024, 4, 16, 16, 3, 4) X(1200, 5, 16, 15, 3, 0) \
    X(1280, 5, 16, 16, 3, 0) X(1440, 6, 16, 15, 2, 3) X(1536, 6, 16, 16, 2, 3) X(1600, 10, 16, 10, 2, 3) \
    X(2048, 8, 16, 16, 2, 3) X(2560, 10, 16, 16, 2, 0) X(3072, 12, 16, 16, 1, 2) X(4096, 16, 16, 16, 1, 2)
// Rows, in the order choose_rows gives them, each on 256 and on 128 threads: the BASELINE widths, then the common picture
// widths; and 7680 = 16 x 20 x 24 on 512 threads (PB_ROWS_PLAN_8K)
#define PB_ROWS_PLANS(X)                                                                         \
    X(3840, 15, 16, 16) X(1920, 8, 16, 15)                                                       \
    X(512, 2, 16, 16) X(640, 4, 16, 10) X(720, 3, 16, 15) X(768, 3, 16, 16) X(800, 5, 16, 10) X(960, 4, 16, 15) \
    X(1024, 4, 16, 16) X(1200, 5, 16, 15) X(1280, 5, 16, 16) X(1440, 6, 16, 15) X(1536, 6, 16, 16) X(1600, 10, 16, 10) \
    X(2048, 8, 16, 16) X(2560, 10, 16, 16) X(3072, 12, 16, 16) X(4096, 16, 16, 16)
#define PB_ROWS_PLAN_8K(X) X(7680, 16, 20, 24)

inline bool plan_is(const HostPlan &pl, int n, int r0, int r1, int r2) {
    return !pl.bluestein_m && pl.nstage == 3 && pl.n == n && pl.radix[0] == r0 && pl.radix[1] == r1 && pl.radix[2] == r2;
}
// the threads of the compiled column kernel for this plan on tiles of 2 << lognb columns (1024 or 512); 0 = not compiled
inline int pb_cols_fixed_has(const HostPlan &pl, int lognb) {
#define PB_COLS_HAS(N_, R0, R1, R2, LN, LW) \
    if (plan_is(pl, N_, R0, R1, R2)) return (LW != 0 && lognb == LW) ? 1024 : (lognb == LN ? 512 : 0);
    PB_COLS_PLANS(PB_COLS_HAS)
#undef PB_COLS_HAS
    return 0;
}
// whether the row kernel for this plan on nth threads is compiled
inline bool pb_rows_fixed_has(const HostPlan &pl, int nth) {
#define PB_ROWS_HAS(N_, R0, R1, R2) if (plan_is(pl, N_, R0, R1, R2)) return nth == 256 || nth == 128;
#define PB_ROWS_HAS_8K(N_, R0, R1, R2) if (plan_is(pl, N_, R0, R1, R2)) return nth == 512;
    PB_ROWS_PLANS(PB_ROWS_HAS)
    PB_ROWS_PLAN_8K(PB_ROWS_HAS_8K)
#undef PB_ROWS_HAS
#undef PB_ROWS_HAS_8K
    return false;
}

// LDS of the compiled kernels.  Rows: the complex line with one pad element per 32.  Columns: the tile, and where both fit what
// a workgroup of that size may take -- all 160 KB on 1024 threads (one per CU), half of it on 512 (two per CU) -- the line's
// twiddle table beside it, each rounded up to whole 1-KB LDS-DMA requests.
constexpr int rows_lds_bytes(int n) { return (n + (n >> 5) + 1) * 8; }
constexpr bool cols_twlds(int n, int lognb, int nth) {
    return ((n * (1 << lognb) * 8 + 1023) / 1024 + (n * 8 + 1023) / 1024) * 1024 <= (nth == 1024 ? 160 : 80) * 1024;
}
constexpr int cols_lds_bytes(int n, int lognb, int nth) {
    return ((n * (1 << lognb) * 8 + 1023) / 1024 + (cols_twlds(n, lognb, nth) ? (n * 8 + 1023) / 1024 : 0)) * 1024;
}

// ------------------------------------------------------------------------------------
// The choice
// ------------------------------------------------------------------------------------
enum { PB_LINE_MEMORY = 0,        // the line buffer in global memory (grad_*_long_kernel): lines beyond 160 KB of LDS
       PB_LINE_RUNTIME = 1,       // the run-time-plan kernels of estimate.hip
       PB_LINE_COMPILED = 2 };    // the compiled-plan kernels of lines_fixed.hip
enum { PB_LINE_F32 = 0, PB_LINE_F16 = 1, PB_LINE_U8 = 2 };       // (= PB_F32, PB_F16, PB_U8 of the public header)

// What a launch is for.  Rows: C == 0: float planes in, out_dtype planes out; C > 0: gray + range + transform from the C
// channels of in_dtype images (the estimation's fused launch).  Columns: maxima == 0: the y derivative as out_dtype planes;
// else the directional maxima of n_angles + 1 directions, discard_sat: under the saturation mask.
struct LineUse { int C = 0, in_dtype = PB_LINE_F32, out_dtype = PB_LINE_F32, normalize = 0, maxima = 0, n_angles = 0, discard_sat = 0; };

struct LineChoice {
    HostPlan plan;            // the radices in stage order
    int ext = 0, first = 0;   // its key: the plan with radices above 16 allowed / the greedy one; the first radix asked for (0: the plan's own)
    int kind = PB_LINE_RUNTIME;
    int taken = 1;            // gray rows: whether the fused launch is taken at all (0: the gray pass, then rows from planes)
    int threads = 0, lognb = 0;
    int tiles = 0;            // workgroups' worth of work per plane: row pairs, or column tiles of 2 << lognb columns
    int lds = 0;              // dynamic LDS bytes of the launch (PB_LINE_MEMORY: bytes of a workgroup's slot in global memory)
    int max_radix = 16;       // columns: the widest radix of the run-time-plan kernel variant that holds the plan (16, 18 or 24)
    int sat = 0;              // columns, PB_LINE_COMPILED: the instance that looks at the saturation mask
    int half_ok = 0;          // fp16 planes can be written (the typed outputs exist in the compiled kernels only)
};

constexpr int kLineMaxLds = 160 * 1024;
constexpr int kLineLongThreads = 1024;          // threads of the through-memory kernels

inline long line_lds_bytes(const HostPlan &pl, int nb) { return (long)(pl.bluestein_m ? pl.bluestein_m : pl.n) * nb * 8; }
inline int plan_max_radix(const HostPlan &pl) { return pl.nstage ? *std::max_element(pl.radix, pl.radix + pl.nstage) : 0; }

// Which of a plan's radices its first and last stage should take -- the two that talk to global memory: the smallest one
// (up to 16) that is at least `always_from`, or at least `min_r` with n / r <= max_items butterflies per line; 0 = the
// plan's own first radix.  A function of the plan and the line length ALONE: the order of the stages decides the roundings,
// and an image gets the same bits alone and in a batch (tests/test_gpu_fullsize.py, test_gpu_round5_forms.py).
inline int first_radix_for(const HostPlan &pl, int n, int max_items, int always_from, int min_r) {
    if (pl.bluestein_m || pl.nstage < 2) return 0;
    int first = pl.radix[0];
    for (int i = 1; i < pl.nstage; ++i) {
        const int r = pl.radix[i];
        if (r <= 16 && r < first && (r >= always_from || (r >= min_r && n / r <= max_items))) first = r;
    }
    return first == pl.radix[0] ? 0 : first;
}

// the plan of a choice: the length's own, or the one with the first radix the knob (> 0) or the rule (< 0) names
inline void choose_plan(LineChoice &c, HostPlans &memo, const LineKnobs &k, int n, bool ext, int knob, int always_from) {
    const HostPlan *pl = &host_plan(memo, k, n, ext, 0);
    c.ext = ext ? 1 : 0;
    if (knob != 0 && line_lds_bytes(*pl, 1) <= kLineMaxLds) {
        const int first = knob > 0 ? knob : first_radix_for(*pl, n, 256, always_from, 2);
        if (first > 0 && first != pl->radix[0]) { pl = &host_plan(memo, k, n, ext, first); c.first = first; }
    }
    c.plan = *pl;
}

// Rows (one workgroup = one PAIR of rows as one complex line).
// The plan: of its radices (2 .. 16) the smallest whose n / r butterflies are one trip for 256 threads goes first.  Fewer
// loads and a smaller butterfly between a thread's loads and its LDS writes, every thread busy: 1920 = 16 x 15 x 8 is 120
// butterflies of radix 16 or 240 of radix 8.  Measured per launch (one image, 256 threads): 1080p 24.2 -> 21.0 us (8 first),
// 1280-sample rows 23.0 -> 19.5 (5), 700-sample rows 16.3 -> 15.1 (7), 1024 21.0 -> 16.0 (4), 720 22.6 -> 15.9 (3), 512 18.6
// -> 12.4 (2: 256 threads loading instead of 32); batches on 128 threads: 16 x 720-sample rows 126 -> 93 us, 8 x 1024 57 ->
// 50, 32 x 1080p -- where radix 8 is a second trip -- 304 -> 307 (15 first: 289).  choose_cols has the column transform's rule.
inline LineChoice choose_rows(HostPlans &memo, const LineKnobs &k, int W, int H, int P, const LineUse &use) {
    LineChoice c;
    choose_plan(c, memo, k, W, true, k.fft_first_rows, 17);       // (the 512-thread variant holds the radices above 16)
    const HostPlan &pl = c.plan;
    const long lds = line_lds_bytes(pl, 1), blocks = (long)P * ((H + 1) / 2);
    c.tiles = (H + 1) / 2;
    c.lds = (int)lds;
    const bool gray = use.C > 0;
    if (lds > kLineMaxLds) {                        // the line buffer in global memory, one slot per workgroup
        c.kind = PB_LINE_MEMORY; c.threads = kLineLongThreads; c.taken = gray ? 0 : 1;
        return c;
    }
    const bool fused = !pl.bluestein_m && pl.nstage >= 2;          // as pbfft::fused_plan
    // A workgroup's transform is a chain of dependent stages, so the kernel is as fast as the number of chains in flight.
    // Lines of up to 4096 samples (32 KB of LDS per two rows) fit five workgroups per CU.  A grid that fits the chip in ONE
    // round of five workgroups per CU (a single 4K image: 1080) is a race of dependent chains, and 256 threads -- one
    // butterfly per thread and stage, held to 96 registers so that five such workgroups still fit a CU -- shorten every
    // chain: 41.0 -> 33.4 us at 4K, 17.4 -> 15.8 us at 700 x 500.  Larger grids are throughput-bound and run 128 threads
    // (8 x 1080p: 63.7 us against 70.0 with 256).  Lines above 40 KB of LDS -- 8K rows -- are limited by LDS to two or three
    // workgroups per CU: 512 threads each keep the CU's SIMDs supplied (measured at 7680: 241 us per 8K image against 339
    // us with 128), and the 512-thread variant is the one that holds the radices above 16.
    const bool ext = plan_max_radix(pl) > 16;
    c.threads = (!ext && lds <= 32 * 1024 && blocks > 256L * 5) ? 128 : ((ext || lds > 40 * 1024) ? 512 : 256);
    if (gray) {
        // gray + range partials + row transform in one launch.  Measured (same box, PB_EST_GRAY_ROWS=0/1): 4K fp32 0.820 ->
        // 0.811 ms per call, 32 x 1080p fp32 7.11 -> 7.00 ms; but 8K lines (two workgroups per CU: six load streams with
        // nothing to hide them behind) 4.22 -> 4.33 ms, and fp16 / 8-bit planes (2- and 1-byte loads where the gray pass reads
        // 8 and 4 bytes per lane) 35.0 -> 35.4 ms for 64 x 1080p fp16: the fused launch is built for fp32 planes of the
        // un-normalised image and taken for lines of up to 4096 samples (PB_EST_GRAY_ROWS=2: any length).
        c.taken = k.est_gray_rows && !use.normalize && fused && use.in_dtype == PB_LINE_F32 &&
                  (k.est_gray_rows >= 2 || lds <= 32 * 1024) && blocks <= 0x7fffffffL;
        if (!c.taken) return c;
    }
    // (line lengths whose plan is compiled in: the same butterflies in a one-plan kernel on a padded LDS line;
    // PB_ROWS_FIXED=0: the run-time-plan kernel, the tests' reference)
    const bool fixed = k.rows_fixed && fused && !use.normalize && blocks <= 0x7fffffffL && pb_rows_fixed_has(pl, c.threads) &&
                       (gray ? (use.C == 3 || use.C == 1) : (use.out_dtype == PB_LINE_F32 || use.out_dtype == PB_LINE_F16));
    if (fixed) { c.kind = PB_LINE_COMPILED; c.lds = rows_lds_bytes(pl.n); c.half_ok = gray ? 0 : 1; }
    else if (!fused) c.threads = 256;
    return c;
}

// Columns (one workgroup = 2 << lognb adjacent columns of all rows of one plane, as 1 << lognb complex lines).
inline LineChoice choose_cols(HostPlans &memo, const LineKnobs &k, int H, int W, int P, const LineUse &use) {
    LineChoice c;
    const bool seven = use.maxima && use.n_angles == 6;
    // (the 1024-thread variants of the gy-writing and the 7-direction kernels exist with the radices above 16)
    const bool ext_variant = !use.maxima || seven;
    // Which of the plan's radices the first and the last stage take -- the two that talk to global memory, the last one with
    // the epilogue's operands (gx, the gray sample) prefetched for every output of its butterfly and the directional maxima
    // folded behind it.  The SMALLEST: fewer values per thread between the loads and the butterfly, fewer operands held for
    // the epilogue (the 1024-thread variants have 128 registers per thread), and trips over the workgroup's threads that
    // are full -- 2160 = 16 x 15 x 9 in tiles of 16 columns is 1080 butterflies of radix 16 for 1024 threads, a second
    // trip for 56 of them, or 1920 of radix 9.  Measured per launch, greedy order -> smallest first: 4K 48.5 -> 43.3 us
    // (9; 15 first: 45.2), 1080p 40.7 -> 32.0 (6; 12 first: 36.5), 1440p 50.5 -> 45.3 (6), 1920 x 1200 41.1 -> 35.2 (5),
    // 1920 x 1280 40.0 -> 35.9 (5), 720p 28.3 -> 26.9 (3), 500 x 700 31.1 -> 28.4 (7), 2048^2 33.7 -> 33.1 (8);
    // 32 x 1080p 394 -> 323 us.  Radices below 5 only for lines of up to 256 of their butterflies (every trip is a round
    // trip to memory): 512 x 512 24.6 -> 20.8 us with 2 first, 3000-sample columns -- twelve trips of radix 2 -- no different.
    // A function of the line length alone, as the rows'.
    choose_plan(c, memo, k, H, ext_variant, k.fft_first, 5);
    const HostPlan &pl = c.plan;
    if (line_lds_bytes(pl, 1) > kLineMaxLds) {     // lines through global memory (grad_cols_long_kernel): 8-column tiles
        c.kind = PB_LINE_MEMORY; c.threads = kLineLongThreads;
        c.lognb = 2;
        while (c.lognb > 0 && (2 << (c.lognb - 1)) >= W * 2) --c.lognb;
    } else {
        // How many complex lines a workgroup transforms together, and with how many threads.  Base rule: the widest tile whose
        // lines fit 80 KB of LDS (two workgroups per CU).  For the gy-writing and the 7-direction kernels on a fused plan one
        // workgroup with a tile twice as wide is 7 % faster when it fits: the same waves per CU, but half as many 128-byte
        // lines requested per useful byte of the column segments (measured, 4K: 73.7 -> 68.5 us; 8 x 1080p: 132 -> 122 us;
        // 512 threads on the narrow tile: 95 us; one 700x500 image, whose 44 narrow tiles already leave most CUs idle:
        // 31.7 -> 35.9 us, hence the workgroup-count condition).
        c.lognb = 3;
        while (c.lognb > 0 && line_lds_bytes(pl, 1 << c.lognb) > 80 * 1024) --c.lognb;
        while (c.lognb > 0 && (2 << (c.lognb - 1)) >= W * 2) --c.lognb;
        const bool wide = ext_variant && !pl.bluestein_m && pl.nstage >= 2 &&
            line_lds_bytes(pl, 2 << c.lognb) <= 140 * 1024 && (long)P * (W / (4 << c.lognb)) >= 200 &&   // still fills the chip
            // (the 7 directions of 1080-point lines through lines_fixed.hip: two 512-thread workgroups per CU on 16-column
            // tiles -- 69 KB each, one's requests under the other's stages -- beat one 1024-thread workgroup on a 32-column
            // tile: 32 x 1080p 174 against 198 us)
            !(seven && !use.normalize && k.cols_fixed && pl.n == 1080 && (W % 16) == 0);
        if (wide) ++c.lognb;
        // the line lengths whose plan is compiled in: the same arithmetic in a kernel that holds one plan -- bit-identical
        // maxima and planes (PB_COLS_FIXED=0: the run-time-plan kernel, the tests' reference)
        const int fixed = (k.cols_fixed && !use.normalize && (!use.maxima || seven) && c.lognb >= 1 && (W % (2 << c.lognb)) == 0)
                              ? pb_cols_fixed_has(pl, c.lognb) : 0;
        c.max_radix = plan_max_radix(pl) <= 16 ? 16 : ((use.maxima && plan_max_radix(pl) <= 18) ? 18 : 24);
        if (fixed) {
            c.kind = PB_LINE_COMPILED; c.threads = fixed;
            c.sat = (use.maxima && use.discard_sat) ? 1 : 0;
            c.half_ok = use.maxima ? 0 : 1;
        }
        // (a plan whose widest radix is 18 -- 4320 = 16 x 15 x 18, the 8K height -- runs the variant without 20 and 24: fewer
        // registers spilled around the butterflies it does take)
        else if (c.max_radix > 16) c.threads = 1024;
        // the y derivative on the wide tile (192 x 1080p planes: 2.27 -> 1.61 ms against 8-column tiles with 256 threads);
        // the 7 directions on 16-column tiles, one workgroup per CU: 1024 threads (16 waves) hide the stages' LDS latency
        // better than 512 (measured: 4K 62 -> 55 us, 8 x 1080p 113 -> 95 us, 8K 277 -> 268 us)
        else if (wide) c.threads = 1024;
        // the 7 directions on 8-column (or narrower) tiles, two workgroups per CU: 512 threads each (measured against 256:
        // 700x500 31 -> 23 us, 1080p 56 -> 40 us, 512x512 28 -> 25 us)
        else c.threads = seven ? 512 : 256;
    }
    const int tc = 2 << c.lognb;
    c.tiles = (W + tc - 1) / tc;
    c.lds = c.kind == PB_LINE_COMPILED ? cols_lds_bytes(pl.n, c.lognb, c.threads) : (int)line_lds_bytes(pl, 1 << c.lognb);
    return c;
}
