// What runs for one call of the domain-transform recursive filter on one- or three-channel images (dt.hip): the form of the
// first iteration's row pass, the form of every column pass and the scratch they want, chosen ONCE per call by choose_dt and
// read by the launcher (dt_filter_fused) and by pb_debug_dt_choice.  Host code without a HIP call or type: the knobs, every
// threshold and block size of the filter with its measurement, and the chooser.  tests/test_dt_choice_cpu.py sweeps it through
// the query and holds the answers against tests/golden/dt_choices.json; tools/dt_choice_sweep.cpp is the sweep as a program of
// its own.  (Iterations after the first always run dt_rows_fused_kernel<T, float, C> in place: a fact of the launcher.)
#pragma once

// The knobs the choice reads (pb_ctx.dt; api.hip: pb_read_knobs has the table of every knob)
struct DtKnobs {
    int rows_reg = 1;       // env PB_DT_ROWS_REG: the first row pass with the row in registers: 1 = one wave per row, a row over the four waves of a workgroup for up to DT_ROWSW_MAX rows in the batch; 0 = always through global memory (dt_rows_fused_kernel); 2 = one wave per row always (dt_rows_reg_kernel); 3 = a row over four waves always (dt_rows_regw_kernel)
    int cols_strip = 1;     // env PB_DT_COLS_STRIP: 0 = the column pass as two sweeps through global memory (dt_cols_fused_kernel), 1 = in strips, the weights stored where that pays, 2 = strips whose up sweep always forms the weights from J again
    int cols_coop = 1;      // env PB_DT_COLS_COOP: the few-columns form of the column pass (dt_cols_coop_kernel): 1 = for up to DTC_MAX_COLS columns in the batch, 0 = never, 2 = always where it applies
};

// ---- sizes the kernels are built on, thresholds the choice applies ------------------------------------------------------------
constexpr int DT_ROWS_WAVE_MAX = 4096;             // the widest row one wave holds in registers: 64 chunks of 64 samples (~300 registers, one wave per SIMD)
constexpr int DT_ROWSW_MIN = 256, DT_ROWSW_MAX_W = 8192;   // a row over four waves: rows of more than one chunk per wave, up to 32 chunks per wave
constexpr long DT_ROWSW_MAX = 8192;                // rows in the batch up to which a row is spread over four waves (tools/bench_dt.py)
constexpr int DT_UF = 8, DT_U = 16;                // rows whose operands a column thread of the sweeps requests together (DT_U: with domain planes, other channel counts)
constexpr int DT_STRIP = 16, DT_STRIP_W = 32;      // rows of a strip: J and F in registers; F and the stored weights (no J in registers)
constexpr int DTC_R3 = 96, DTC_R1 = 64;            // rows of a block: three channels (78 KB of LDS, two workgroups per CU), one channel
constexpr int DTC_CH = 32;                         // rows the recurrence's wave holds in registers at a time
constexpr long DTC_MAX_COLS = 24576;               // up to here the per-column forms leave CUs idle (tools/bench_dt.py)
constexpr unsigned DTC_NO_ACCESS = 0x80000000u;    // a buffer offset no request is served for (an image's planes are smaller than 2 GiB: choose_dt)

// the cooperative column form: columns of a workgroup, and its LDS -- two blocks of F, two of J with the row above, the weights
constexpr int dtc_cg(int C) { return C == 1 ? 64 : 16; }
constexpr int dtc_rows(int C) { return C == 1 ? DTC_R1 : DTC_R3; }
constexpr int dtc_f_bytes(int C, int R) { return R * C * dtc_cg(C) * 4; }                                            // whole KB
constexpr int dtc_j_bytes(int elem, int C, int R) { return ((R + 1) * C * dtc_cg(C) * elem + 1023) / 1024 * 1024; }
constexpr int dtc_lds_bytes(int elem, int C, int R) { return 2 * dtc_f_bytes(C, R) + 2 * dtc_j_bytes(elem, C, R) + R * dtc_cg(C) * 4; }

// ---- the choice -------------------------------------------------------------------------------------------------------------------
enum { PB_DT_ROWS_MEMORY = 0,          // dt_rows_fused_kernel<T, T, C>: the intermediate row through global memory
       PB_DT_ROWS_WAVE = 1,            // dt_rows_reg_kernel<T, C, chunks>: one wave per row, the row in its registers
       PB_DT_ROWS_WORKGROUP = 2 };     // dt_rows_regw_kernel<T, C, chunks>: a row over four waves, `chunks` per wave
enum { PB_DT_COLS_SWEEPS = 0,          // dt_cols_fused_kernel: down and up through global memory
       PB_DT_COLS_STRIPS = 1,          // dt_cols_down_kernel<.., DT_STRIP, false> + dt_cols_up_kernel: the weights formed again from J
       PB_DT_COLS_STRIPS_WEIGHTS = 2,  // dt_cols_down_kernel<.., DT_STRIP_W, true> + dt_cols_upw_kernel: the down sweep's weights stored and read back
       PB_DT_COLS_COOPERATIVE = 3 };   // dt_cols_coop_kernel: a workgroup per dtc_cg columns, blocks of rows through LDS

struct DtChoice {
    int rows = PB_DT_ROWS_MEMORY, chunks = 0;    // the row pass of iteration 0; chunks of 64 samples per wave (0: no such template argument)
    int cols = PB_DT_COLS_SWEEPS, cols_rows = 0; // every column pass; rows of a strip or block
    long carry = 0, weights = 0;                 // floats of "dt.carry" and "dt.weights"
    int lds = 0;                                 // dynamic LDS of the cooperative form
};

// elem: bytes of an image sample (4 or 2); C: 1 or 3; self_guided: the joint image is the input itself; aligned16: J and out
// both lie on 16-byte boundaries
inline DtChoice choose_dt(const DtKnobs &k, int elem, int C, int B, int H, int W, bool self_guided, bool aligned16) {
    DtChoice c;
    const long rows_total = (long)B * H, cols_total = (long)B * W;
    // (a filter guided by its own input: the neighbour differences come from the registers too)
    // few rows: a row over the four waves of a workgroup -- rows of up to 8192 samples; else one wave per row, up to 4096
    if (self_guided && W > DT_ROWSW_MIN && W <= DT_ROWSW_MAX_W && k.rows_reg && k.rows_reg != 2 && (k.rows_reg == 3 || rows_total <= DT_ROWSW_MAX)) {
        c.rows = PB_DT_ROWS_WORKGROUP;
        c.chunks = W <= 1024 ? 4 : (W <= 2048 ? 8 : (W <= 4096 ? 16 : 32));
    } else if (self_guided && W <= DT_ROWS_WAVE_MAX && k.rows_reg && k.rows_reg != 3) {
        c.rows = PB_DT_ROWS_WAVE;
        c.chunks = W <= 1024 ? 16 : (W <= 2048 ? 32 : 64);
    }
    // few columns: workgroups of CG columns whose lanes all fetch; 16-byte requests want rows, planes and operands on 16-byte
    // boundaries, and a buffer descriptor holds an image's planes of less than 2 GiB
    const bool coop_ok = W % 4 == 0 && W % (16 / elem) == 0 && aligned16 && (long)C * H * W * 4 < (1l << 31);
    if (k.cols_coop && coop_ok && (k.cols_coop == 2 || cols_total <= DTC_MAX_COLS)) {
        const int CG = dtc_cg(C), R = dtc_rows(C);
        c.cols = PB_DT_COLS_COOPERATIVE;
        c.cols_rows = R;
        c.carry = (long)B * ((W + CG - 1) / CG) * ((H + R - 1) / R) * C * CG;
        c.lds = dtc_lds_bytes(elem, C, R);
    } else if (k.cols_strip && H >= 4 * DT_STRIP) {
        // (the weights pay where J costs the up sweep more than a word to write and a word to read per pixel: fp32 J of 3 channels;
        //  PB_DT_COLS_STRIP=2: always J again)
        const bool weights = C * elem > 8 && k.cols_strip == 1 && H >= 4 * DT_STRIP_W;
        c.cols = weights ? PB_DT_COLS_STRIPS_WEIGHTS : PB_DT_COLS_STRIPS;
        c.cols_rows = weights ? DT_STRIP_W : DT_STRIP;
        c.carry = (long)((H + c.cols_rows - 1) / c.cols_rows) * C * cols_total;
        if (weights) c.weights = (long)H * cols_total;
    }
    return c;
}
