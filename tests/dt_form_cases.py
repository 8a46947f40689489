"""The shapes and knob sets of the domain-transform form tests, in one place for their two readers: tests/test_gpu_round5_forms.py
runs them on the GPU (every form against the global-memory form, bit for bit), tests/test_dt_choice_cpu.py asks the host-side
choice (csrc/dt_choice.h, through pb_debug_dt_choice) which kernel instantiation each of them takes under each engine's knobs --
and that every instantiation the launcher can reach is reached by one of them."""
import numpy as np

# test_dt_rows_register_form (fp32 and fp16 each): ragged tails, exactly-full chunks, the widest rows each form takes and one
# sample beyond, two-sample rows; (1, 1, 3, 1500): the one-channel row of 1025 .. 2048 samples -- 32 chunks on one wave, 8 per
# wave on four
ROW_FORM_SHAPES = [(2, 3, 37, 203), (1, 3, 90, 1920), (1, 1, 33, 1024), (3, 3, 5, 2048), (1, 3, 17, 64), (2, 1, 9, 2),
                   (1, 3, 21, 3840), (2, 3, 3, 4096), (1, 1, 7, 2500), (1, 3, 4, 4100), (1, 3, 3, 7680), (1, 1, 2, 8192),
                   (2, 3, 5, 257), (1, 3, 6, 1025), (1, 1, 4, 8200), (1, 1, 3, 1500)]
ROW_FORM_DTYPES = [np.float32, np.float16]

# test_dt_columns_in_strips
COLUMN_FORM_CASES = [((1, 3, 720, 1280), np.float32), ((2, 3, 203, 333), np.float16), ((1, 1, 1081, 700), np.float32),
                     ((3, 3, 64, 97), np.float32), ((1, 3, 65, 40), np.float16), ((1, 1, 1600, 2100), np.float32),
                     ((2, 3, 128, 70), np.float32), ((1, 3, 161, 300), np.float32), ((2, 3, 203, 336), np.float16),
                     ((1, 3, 31, 64), np.float32), ((2, 1, 96, 136), np.float16)]

# the engines of test_gpu_round5_forms.py that differ from the default one in a domain-transform knob
DT_ENGINE_KNOBS = {"dt_global": dict(PB_DT_ROWS_REG=0), "dt_rows_wave": dict(PB_DT_ROWS_REG=2), "dt_rows_regw": dict(PB_DT_ROWS_REG=3),
                   "dt_cols_sweeps": dict(PB_DT_COLS_STRIP=0, PB_DT_COLS_COOP=0), "dt_cols_reread": dict(PB_DT_COLS_STRIP=2, PB_DT_COLS_COOP=0),
                   "dt_cols_threads": dict(PB_DT_COLS_COOP=0), "dt_cols_coop": dict(PB_DT_COLS_COOP=2)}
# which forms each test compares with its reference engine (the first of each tuple)
ROW_FORMS = ("dt_global", "default", "dt_rows_wave", "dt_rows_regw")
COLUMN_FORMS = ("dt_cols_sweeps", "default", "dt_cols_threads", "dt_cols_reread", "dt_cols_coop")


def knobs_of(engine):
    """(rows_reg, cols_strip, cols_coop) of one of the engines above, or of "default" """
    k = DT_ENGINE_KNOBS.get(engine, {})
    return k.get("PB_DT_ROWS_REG", 1), k.get("PB_DT_COLS_STRIP", 1), k.get("PB_DT_COLS_COOP", 1)
