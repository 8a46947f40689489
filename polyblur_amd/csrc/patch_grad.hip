// The backward passes of the patch lattice: PolyblurDeblurring(patch_decomposition=True) under autograd.  The image
// is (virtually) replicate-padded by (pad_top, pad_left) to new_h x new_w = (n_i - 1) step_h + ph by (n_j - 1) step_w + pw; patch
// n = ki n_j + kj starts at (i0, j0) = (ki step_h, kj step_w) of the padded image; patches are laid out [n*B + b, c, y, x].
//
// pb_extract_patches_backward, the adjoint of extract_patches_kernel (filters.hip) -- a gather of a clamped index:
//
//   P[b,c,py,px]    = sum over the patches (ki, kj) that hold (py, px) of grad_patches[n*B + b, c, py - i0, px - j0]
//   R[b,c,Y,px]     = sum over the padded rows py that clamp to Y of P[b,c,py,px]        one row, or pad + 1 at an edge
//   grad_img[b,c,Y,X] = sum over the padded columns px that clamp to X of R[b,c,Y,px]
//
//   patchg_cover      one thread per padded sample: at most the cover (the patches over one sample) terms
//   patchg_fold_rows  one thread per (Y, px): one term, or the pad's run at the first and last row
//   patchg_fold_cols  one thread per image sample: one term, or the pad's run at the first and last column
//
// pb_overlap_add_backward, the adjoint of overlap_add_kernel: with num, den the cover sums of patch_cover.h -- the forward's own
// function -- v = num / (den + 1e-8) and m = [0 <= v <= 1], inclusive at both ends (torch.clamp's gradient),
//
//   S[b,c,Y,X] = m grad_out[b,c,Y,X] / (den + 1e-8)
//   grad_patches[n*B + b, c, y, x] = win_y[y] win_x[x] S[b, c, i0 + y - pad_top, j0 + x - pad_left]   inside H x W, else exactly 0
//
//   patchg_scale      one thread per image sample: the forward's cover sum again, from `patches`
//   patchg_window     one thread per patch element
//
// x is the fastest index of every kernel: a wave reads and writes whole lines.  Every sum runs in index order, rows of patches then
// columns, padded rows, padded columns -- an order the shape alone fixes; no float atomics: the same call gives the same bits.
#include <algorithm>
#include <climits>

#include "common.h"
#include "patch_cover.h"

namespace {

constexpr int NT = 256;

struct Lattice { int B, C, H, W, ph, pw, step_h, step_w, n_i, n_j, pad_top, pad_left, new_h, new_w; };

unsigned blocks_for(long n) { return (unsigned)std::min((n + NT - 1) / NT, 1L << 20); }

__global__ __launch_bounds__(NT) void patchg_cover(const float *__restrict__ gp, float *__restrict__ P, Lattice l, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int px = (int)(i % l.new_w);
        long r = i / l.new_w;
        const int py = (int)(r % l.new_h);
        const long plane = r / l.new_h;                          // b * C + c
        const long b = plane / l.C, c = plane - b * l.C;
        int ki_lo, ki_hi, kj_lo, kj_hi;                          // (the forward's ranges: patch_cover.h)
        patch_cover_range(py, l.ph, l.step_h, l.n_i, ki_lo, ki_hi);
        patch_cover_range(px, l.pw, l.step_w, l.n_j, kj_lo, kj_hi);
        float s = 0.f;
        for (int ki = ki_lo; ki <= ki_hi; ++ki) {
            const int y = py - ki * l.step_h;
            if (y < 0 || y >= l.ph) continue;
            for (int kj = kj_lo; kj <= kj_hi; ++kj) {
                const int x = px - kj * l.step_w;
                if (x < 0 || x >= l.pw) continue;
                const long n = (long)ki * l.n_j + kj;
                s += gp[(((n * l.B + b) * l.C + c) * l.ph + y) * l.pw + x];
            }
        }
        P[i] = s;
    }
}

// the padded positions lo .. hi of an axis of `padded` samples that clamp to sample s of n, the image starting at `pad`
__device__ __forceinline__ void clamp_run(int s, int n, int pad, int padded, int &lo, int &hi) {
    lo = s == 0 ? 0 : max(s + pad, 0);
    hi = s == n - 1 ? padded - 1 : min(s + pad, padded - 1);
}

__global__ __launch_bounds__(NT) void patchg_fold_rows(const float *__restrict__ P, float *__restrict__ R, Lattice l, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int px = (int)(i % l.new_w);
        const long r = i / l.new_w;
        const int Y = (int)(r % l.H);
        const long plane = r / l.H;
        int lo, hi;
        clamp_run(Y, l.H, l.pad_top, l.new_h, lo, hi);
        const float *p = P + plane * l.new_h * l.new_w + px;
        float s = 0.f;
        for (int py = lo; py <= hi; ++py) s += p[(long)py * l.new_w];
        R[i] = s;
    }
}

__global__ __launch_bounds__(NT) void patchg_fold_cols(const float *__restrict__ R, float *__restrict__ grad, Lattice l, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int X = (int)(i % l.W);
        const long row = i / l.W;                                // (b * C + c) * H + Y
        int lo, hi;
        clamp_run(X, l.W, l.pad_left, l.new_w, lo, hi);
        const float *p = R + row * l.new_w;
        float s = 0.f;
        for (int px = lo; px <= hi; ++px) s += p[px];
        grad[i] = s;
    }
}

__global__ __launch_bounds__(NT) void patchg_scale(const float *__restrict__ patches, const float *__restrict__ g, float *__restrict__ S,
                                                   Lattice l, const float *__restrict__ win_y, const float *__restrict__ win_x,
                                                   long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int X = (int)(i % l.W);
        long r = i / l.W;
        const int Y = (int)(r % l.H); r /= l.H;
        const int c = (int)(r % l.C);
        const int b = (int)(r / l.C);
        const PatchCover cv = patch_cover(patches, l.B, l.C, l.ph, l.pw, l.step_h, l.step_w, l.n_i, l.n_j, b, c, Y + l.pad_top,
                                          X + l.pad_left, win_y, win_x);
        const float v = patch_cover_value(cv);
        S[i] = (v >= 0.f && v <= 1.f) ? g[i] / (cv.den + 1e-8f) : 0.f;
    }
}

__global__ __launch_bounds__(NT) void patchg_window(const float *__restrict__ S, float *__restrict__ gp, Lattice l,
                                                    const float *__restrict__ win_y, const float *__restrict__ win_x, long total) {
    for (long i = (long)blockIdx.x * NT + threadIdx.x; i < total; i += (long)gridDim.x * NT) {
        const int x = (int)(i % l.pw);
        long r = i / l.pw;
        const int y = (int)(r % l.ph); r /= l.ph;
        const int c = (int)(r % l.C); r /= l.C;
        const int b = (int)(r % l.B);
        const int n = (int)(r / l.B);
        const int Y = (n / l.n_j) * l.step_h + y - l.pad_top, X = (n % l.n_j) * l.step_w + x - l.pad_left;
        float v = 0.f;
        if (Y >= 0 && Y < l.H && X >= 0 && X < l.W) v = win_y[y] * win_x[x] * S[(((long)b * l.C + c) * l.H + Y) * l.W + X];
        gp[i] = v;
    }
}

// the checks the two entries share; PB_OK with `l` filled in
int lattice_of(pb_ctx *ctx, const char *who, int B, int C, int H, int W, int ph, int pw, int step_h, int step_w, int n_i, int n_j,
               int pad_top, int pad_left, Lattice &l) {
    if (B < 1 || C < 1 || H < 1 || W < 1 || (long)B * C > INT_MAX) return pb_fail(ctx, PB_ERR_BADARG, "%s: bad shape (%d,%d,%d,%d)", who, B, C, H, W);
    if (ph < 2 || pw < 2 || step_h < 1 || step_w < 1)
        return pb_fail(ctx, PB_ERR_BADARG, "%s: patches of at least 2x2 with a positive step are needed (got %dx%d, steps %d, %d)", who, ph, pw, step_h, step_w);
    if (n_i < 1 || n_j < 1) return pb_fail(ctx, PB_ERR_BADARG, "%s: the lattice holds no patch (%d x %d)", who, n_i, n_j);
    const long new_h = (long)(n_i - 1) * step_h + ph, new_w = (long)(n_j - 1) * step_w + pw;
    if (new_h > INT_MAX / 2 || new_w > INT_MAX / 2 || (long)n_i * n_j * B > INT_MAX || pad_top < -(INT_MAX / 2) || pad_top > INT_MAX / 2 ||
        pad_left < -(INT_MAX / 2) || pad_left > INT_MAX / 2)
        return pb_fail(ctx, PB_ERR_BADARG, "%s: lattice too large", who);
    l = Lattice{B, C, H, W, ph, pw, step_h, step_w, n_i, n_j, pad_top, pad_left, (int)new_h, (int)new_w};
    return PB_OK;
}

}  // namespace

extern "C" int pb_extract_patches_backward(pb_ctx *ctx, const float *grad_patches, float *grad_img, int B, int C, int H, int W, int ph,
                                           int pw, int step_h, int step_w, int n_i, int n_j, int pad_top, int pad_left) {
    if (!ctx) return PB_ERR_BADARG;
    if (!grad_patches || !grad_img) return pb_fail(ctx, PB_ERR_BADARG, "pb_extract_patches_backward: null argument");
    if (grad_img == grad_patches) return pb_fail(ctx, PB_ERR_BADARG, "pb_extract_patches_backward: grad_img may not alias grad_patches");
    Lattice l;
    const int rc = lattice_of(ctx, "pb_extract_patches_backward", B, C, H, W, ph, pw, step_h, step_w, n_i, n_j, pad_top, pad_left, l);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    const long P = (long)B * C;
    const long nP = P * l.new_h * l.new_w, nR = P * H * l.new_w, nG = P * H * W;
    float *Pd = static_cast<float *>(pb_scratch(ctx, "patchg.P", sizeof(float) * (size_t)nP));
    float *Rd = static_cast<float *>(pb_scratch(ctx, "patchg.R", sizeof(float) * (size_t)nR));
    if (!Pd || !Rd) return PB_ERR_NOMEM;
    ProfScope prof(ctx, PB_PROF_OTHER);
    hipLaunchKernelGGL(patchg_cover, dim3(blocks_for(nP)), dim3(NT), 0, ctx->stream, grad_patches, Pd, l, nP);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(patchg_fold_rows, dim3(blocks_for(nR)), dim3(NT), 0, ctx->stream, Pd, Rd, l, nR);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(patchg_fold_cols, dim3(blocks_for(nG)), dim3(NT), 0, ctx->stream, Rd, grad_img, l, nG);
    PB_LAUNCH_CHECK();
    return PB_OK;
}

extern "C" int pb_overlap_add_backward(pb_ctx *ctx, const float *patches, const float *grad_out, float *grad_patches, int B, int C,
                                       int H, int W, int ph, int pw, int step_h, int step_w, int n_i, int n_j, int pad_top,
                                       int pad_left, const float *dev_win_y, const float *dev_win_x) {
    if (!ctx) return PB_ERR_BADARG;
    if (!patches || !grad_out || !grad_patches || !dev_win_y || !dev_win_x)
        return pb_fail(ctx, PB_ERR_BADARG, "pb_overlap_add_backward: null argument");
    if (grad_patches == patches || grad_patches == grad_out || grad_patches == dev_win_y || grad_patches == dev_win_x)
        return pb_fail(ctx, PB_ERR_BADARG, "pb_overlap_add_backward: grad_patches may not alias an input");
    Lattice l;
    const int rc = lattice_of(ctx, "pb_overlap_add_backward", B, C, H, W, ph, pw, step_h, step_w, n_i, n_j, pad_top, pad_left, l);
    if (rc) return rc;
    PB_HIP(hipSetDevice(ctx->device));
    const long nS = (long)B * C * H * W, nG = (long)n_i * n_j * B * C * ph * pw;
    float *S = static_cast<float *>(pb_scratch(ctx, "patchg.S", sizeof(float) * (size_t)nS));
    if (!S) return PB_ERR_NOMEM;
    ProfScope prof(ctx, PB_PROF_OTHER);
    hipLaunchKernelGGL(patchg_scale, dim3(blocks_for(nS)), dim3(NT), 0, ctx->stream, patches, grad_out, S, l, dev_win_y, dev_win_x, nS);
    PB_LAUNCH_CHECK();
    hipLaunchKernelGGL(patchg_window, dim3(blocks_for(nG)), dim3(NT), 0, ctx->stream, S, grad_patches, l, dev_win_y, dev_win_x, nG);
    PB_LAUNCH_CHECK();
    return PB_OK;
}
