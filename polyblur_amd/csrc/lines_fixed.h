// Compiled-plan line transforms of the estimation (lines_fixed.hip): the line lengths whose plan is known at compile time.
// Which they are: PB_COLS_PLANS / PB_ROWS_PLANS and pb_cols_fixed_has / pb_rows_fixed_has of line_choice.h; the launchers take a
// choice of kind PB_LINE_COMPILED and fail loudly (pb_fail) on any other.
#pragma once
#include "common.h"

// column transform: the directional maxima (gy_out == nullptr: grad_cols_kernel's MODE 1), or the y derivative itself as
// float / __half planes (gy_out, gy_dtype = PB_F32 | PB_F16: MODE 0; gx, mags, n_angles unused)
int pb_launch_cols_fixed(pb_ctx *ctx, const LineChoice &c, const float *gray, const float *gx, int P, int W, unsigned *mags,
                         int n_angles, const FftPlan *pl, void *gy_out, int gy_dtype);
// row transform; C == 0: float planes as they are (gx_dtype = PB_F32 | PB_F16 planes out), else gray + range + transform
int pb_launch_rows_fixed(pb_ctx *ctx, const LineChoice &c, const float *in, int C, float *gray, void *gx, float2 *part, long images, int H,
                         const FftPlan *pl, int gx_dtype);
