// The upsampling-branch backward's own part of the training host side, shared by neck_train.hip (fp32) and neck_train16.hip (its 16-bit
// operand twin): the workspace of a context and its budget, the recomputed forward Z = w^T x, the statistics and dZ kernels of every
// form (InstanceNorm, a frozen BatchNorm's affine, a train-mode BatchNorm; fp32 / fp64 in every mode), and the one check, plan and
// driver of the family.  What the three families share (workspace growth, the frame chunks and K ranges, the reduction of the dw
// partials) is train_host.h's.
#pragma once
#include <cmath>
#include "pp_common.h"
#include "train_planes.h" // k_affine_reduce, k_bn_coef
#include "train_host.h"

namespace {

constexpr size_t Z_BUDGET = (size_t)256 << 20; // bytes of Z / dZ workspace: larger batches run in frame chunks
constexpr int ST_MAX_SEG = 64;
constexpr int DX_BLOCK = 64;                   // rows of R that k_neck_dx sums in one accumulator before adding the block to the total

struct neck_ws {
    float* z = nullptr;     size_t z_elems = 0;
    double* st = nullptr;   size_t st_elems = 0;
    float* part = nullptr;  size_t part_elems = 0;
    float* coef = nullptr;  size_t coef_elems = 0; // [Cup][4]: k_bn_coef's coefficients (pp_neck_backward_bn)
    uint16_t* w16 = nullptr; size_t w16_elems = 0; // [part][Cin][R] bf16: the dx product's A operand (pp_neck_backward_mp, neck_train16.hip)
    uint64_t img_gen = 0;   // ctx->commit_gen the index maps belong to (0: none)
    pp_layer_image img[3];
    int32_t* wmap[3] = {nullptr, nullptr, nullptr};
};

struct geom {
    int Cin, Cup, s, ls, h, w, p, pld, R, coff, H, W;
};

// ---- Z = w^T x: workgroup tile 64 rows x 64 pixels, four waves 2 x 2, each 32 x 32 (2 x 2 MFMA tiles) -------------------------
__global__ void __launch_bounds__(256) k_neck_fwd(const float* __restrict__ x, const float* __restrict__ wt, float* __restrict__ Z, int Cin, int R,
                                                  int p, int pld)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int r0 = blockIdx.y * 64 + 32 * (wave >> 1), p0 = blockIdx.x * 64 + 32 * (wave & 1);
    const float* xf = x + (size_t)blockIdx.z * Cin * p;
    float* Zf = Z + (size_t)blockIdx.z * R * pld;
    f32x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int px0 = p0 + l16, px1 = p0 + 16 + l16;
    for (int k0 = 0; k0 < Cin; k0 += 4) {
        const float* wr = wt + (size_t)(k0 + q) * R + r0 + l16;
        const float* xr = xf + (size_t)(k0 + q) * p;
        const float a0 = wr[0], a1 = wr[16];
        const float b0 = px0 < p ? xr[px0] : 0.f, b1 = px1 < p ? xr[px1] : 0.f;
        acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc[1][1], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int px = p0 + 16 * b + l16;
            if (px < pld) // columns p .. pld-1 get exact zeros (their x was masked): the padding the dw product reads
#pragma unroll
                for (int i = 0; i < 4; ++i) Zf[(size_t)(r0 + 16 * a + 4 * q + i) * pld + px] = acc[a][b][i];
        }
}

// element i of channel co's [H][W] output plane -> its place in the row layout
__device__ __forceinline__ size_t z_index(int i, int co, int W, int ls, int w, int pld)
{
    const int s = 1 << ls, oy = i / W, ox = i - oy * W;
    const int row = (co << (2 * ls)) + ((oy & (s - 1)) << ls) + (ox & (s - 1));
    return (size_t)row * pld + (size_t)(oy >> ls) * w + (ox >> ls);
}

__device__ __forceinline__ double wave_sum(double v)
{
    for (int o = 32; o; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// ---- statistics: grid (S, Cup, frames); st[((frame Cup + co) S + seg) 4 + {z, z^2, Gr, Gr z}] ------------------------------------
__global__ void __launch_bounds__(256) k_neck_stats(const float* __restrict__ Z, const float* __restrict__ y, const float* __restrict__ dy,
                                                    double* __restrict__ st, int Cup, int coff, int H, int W, int ls, int w, int pld, int R,
                                                    int seg_len)
{
    __shared__ double red[4][4];
    const int tid = threadIdx.x, co = blockIdx.y, f = blockIdx.z, N = H * W;
    const float* Zf = Z + (size_t)f * R * pld;
    const size_t plane = ((size_t)f * 320 + coff + co) * N;
    const int i0 = blockIdx.x * seg_len, i1 = i0 + seg_len < N ? i0 + seg_len : N;
    double sz = 0.0, szz = 0.0, sg = 0.0, sgz = 0.0;
    for (int i = i0 + tid; i < i1; i += 256) {
        const double z = (double)Zf[z_index(i, co, W, ls, w, pld)];
        const double g = y[plane + i] > 0.f ? (double)dy[plane + i] : 0.0; // the mask is the caller's y, never a recomputed sign
        sz += z; szz += z * z; sg += g; sgz += g * z;
    }
    sz = wave_sum(sz); szz = wave_sum(szz); sg = wave_sum(sg); sgz = wave_sum(sgz);
    if ((tid & 63) == 0) { red[tid >> 6][0] = sz; red[tid >> 6][1] = szz; red[tid >> 6][2] = sg; red[tid >> 6][3] = sgz; }
    __syncthreads();
    if (tid < 4) st[(((size_t)f * Cup + co) * gridDim.x + blockIdx.x) * 4 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// ---- dZ over Z, same grid.  sum(Gr xhat) = rstd (sum(Gr z) - mean sum(Gr)): formed in double from the fp64 sums ------------------
__global__ void __launch_bounds__(256) k_neck_dz(float* __restrict__ Z, const float* __restrict__ y, const float* __restrict__ dy,
                                                 const double* __restrict__ st, int Cup, int coff, int H, int W, int ls, int w, int pld, int R,
                                                 int seg_len)
{
    const int tid = threadIdx.x, co = blockIdx.y, f = blockIdx.z, N = H * W, S = gridDim.x;
    const double* sp = st + ((size_t)f * Cup + co) * S * 4;
    double sz = 0.0, szz = 0.0, sg = 0.0, sgz = 0.0;
    for (int k = 0; k < S; ++k) { sz += sp[4 * k]; szz += sp[4 * k + 1]; sg += sp[4 * k + 2]; sgz += sp[4 * k + 3]; }
    const double inv_n = 1.0 / (double)N, mean = sz * inv_n;
    double var = szz * inv_n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double rstd = 1.0 / sqrt(var + 1e-3);
    const float meanf = (float)mean, rstdf = (float)rstd;
    const float c1 = (float)(sg * inv_n), c2 = (float)(rstd * (sgz - mean * sg) * inv_n);
    float* Zf = Z + (size_t)f * R * pld;
    const size_t plane = ((size_t)f * 320 + coff + co) * N;
    const int i0 = blockIdx.x * seg_len, i1 = i0 + seg_len < N ? i0 + seg_len : N;
    for (int i = i0 + tid; i < i1; i += 256) {
        const size_t zi = z_index(i, co, W, ls, w, pld);
        const float xhat = (Zf[zi] - meanf) * rstdf;
        const float g = y[plane + i] > 0.f ? dy[plane + i] : 0.f;
        Zf[zi] = rstdf * ((g - c1) - xhat * c2);
    }
}

// ---- the branch with a per-channel affine in place of the InstanceNorm (pp_neck_backward_affine), grid (S, Cup, frames) as k_neck_dz:
// g = dy [y > 0], the segment's sum g Z, sum g in fp64 -> st[frame][co][segment][2], and dZ = scale g over Z ------------------------------
__global__ void __launch_bounds__(256) k_affine_neck_dz(float* __restrict__ Z, const float* __restrict__ y, const float* __restrict__ dy,
                                                        const float* __restrict__ scale, double* __restrict__ st, int Cup, int coff, int H, int W,
                                                        int ls, int w, int pld, int R, int seg_len)
{
    __shared__ double red[4][2];
    const int tid = threadIdx.x, co = blockIdx.y, f = blockIdx.z, N = H * W;
    float* Zf = Z + (size_t)f * R * pld;
    const size_t plane = ((size_t)f * 320 + coff + co) * N;
    const float sc = scale[co];
    const int i0 = blockIdx.x * seg_len, i1 = i0 + seg_len < N ? i0 + seg_len : N;
    double sgz = 0.0, sg = 0.0;
    for (int i = i0 + tid; i < i1; i += 256) {
        const size_t zi = z_index(i, co, W, ls, w, pld);
        const float g = y[plane + i] > 0.f ? dy[plane + i] : 0.f; // the mask is the caller's y, never a recomputed sign
        sgz += (double)g * (double)Zf[zi]; sg += (double)g;
        Zf[zi] = sc * g;
    }
    sgz = wave_sum(sgz); sg = wave_sum(sg);
    if ((tid & 63) == 0) { red[tid >> 6][0] = sgz; red[tid >> 6][1] = sg; }
    __syncthreads();
    if (tid < 2) st[(((size_t)f * Cup + co) * gridDim.x + blockIdx.x) * 2 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// ---- the branch in front of a train-mode BatchNorm (pp_neck_backward_bn), grid (S, Cup, frames) as k_neck_dz.  k_bn_neck_sums: g = dy
// [y > 0], the segment's sum g Z, sum g in fp64 -> st[frame][co][segment][2], Z left as it is.  k_bn_neck_dz, once k_bn_coef has pooled
// the sums of all frames: dZ = scale ((g - c1) - zhat c2) over Z, zhat = (Z - mean) r ----------------------------------------------------
__global__ void __launch_bounds__(256) k_bn_neck_sums(const float* __restrict__ Z, const float* __restrict__ y, const float* __restrict__ dy,
                                                      double* __restrict__ st, int Cup, int coff, int H, int W, int ls, int w, int pld, int R,
                                                      int seg_len)
{
    __shared__ double red[4][2];
    const int tid = threadIdx.x, co = blockIdx.y, f = blockIdx.z, N = H * W;
    const float* Zf = Z + (size_t)f * R * pld;
    const size_t plane = ((size_t)f * 320 + coff + co) * N;
    const int i0 = blockIdx.x * seg_len, i1 = i0 + seg_len < N ? i0 + seg_len : N;
    double sgz = 0.0, sg = 0.0;
    for (int i = i0 + tid; i < i1; i += 256) {
        const float g = y[plane + i] > 0.f ? dy[plane + i] : 0.f; // the mask is the caller's y, never a recomputed sign
        sgz += (double)g * (double)Zf[z_index(i, co, W, ls, w, pld)]; sg += (double)g;
    }
    sgz = wave_sum(sgz); sg = wave_sum(sg);
    if ((tid & 63) == 0) { red[tid >> 6][0] = sgz; red[tid >> 6][1] = sg; }
    __syncthreads();
    if (tid < 2) st[(((size_t)f * Cup + co) * gridDim.x + blockIdx.x) * 2 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

__global__ void __launch_bounds__(256) k_bn_neck_dz(float* __restrict__ Z, const float* __restrict__ y, const float* __restrict__ dy,
                                                    const float* __restrict__ scale, const float* __restrict__ coef, int Cup, int coff, int H, int W,
                                                    int ls, int w, int pld, int R, int seg_len)
{
    const int tid = threadIdx.x, co = blockIdx.y, f = blockIdx.z, N = H * W;
    float* Zf = Z + (size_t)f * R * pld;
    const size_t plane = ((size_t)f * 320 + coff + co) * N;
    const float sc = scale[co];
    const float c1 = coef[4 * co], c2 = coef[4 * co + 1], meanf = coef[4 * co + 2], rf = coef[4 * co + 3];
    const int i0 = blockIdx.x * seg_len, i1 = i0 + seg_len < N ? i0 + seg_len : N;
    for (int i = i0 + tid; i < i1; i += 256) {
        const size_t zi = z_index(i, co, W, ls, w, pld);
        const float zhat = (Zf[zi] - meanf) * rf;
        const float g = y[plane + i] > 0.f ? dy[plane + i] : 0.f;
        Zf[zi] = sc * ((g - c1) - zhat * c2);
    }
}

inline neck_ws* workspace(pp_ctx* ctx)
{
    if (!ctx->neck) ctx->neck = new neck_ws();
    return (neck_ws*)ctx->neck;
}

// ---- one call: its arguments (the ones a form does not take stay null / 0).  shift is never read (the mask is the given y) --------------
struct neck_args {
    const float *x = nullptr, *wt = nullptr, *scale = nullptr, *shift = nullptr, *mean = nullptr, *var = nullptr, *y = nullptr, *dy = nullptr;
    int nb = 0;
    float *dw = nullptr, *dx = nullptr;
    double *dscale = nullptr, *dshift = nullptr;
    int chunk_frames = 0;
    hipStream_t stream = nullptr;
};

// The checks of every entry of the family, reported as "<entry>: ...", in the order the fp32 entries test them.  `what` selects the ones
// that read the branch and the context alone (NECK_CHK_SHAPE: pp_neck_backward_path runs just these, pp_neck_backward_mp runs them
// first) and the ones that read the tensors and nb.  Only the InstanceNorm form refuses a BatchNorm context; the affine and batch forms
// add their own pointers to the null test; the tests of dscale / dshift and chunk_frames pass where a form leaves those null / 0.
enum { NECK_CHK_SHAPE = 1, NECK_CHK_TENSORS = 2, NECK_CHK_ALL = 3 };
inline int neck_check(pp_ctx* ctx, const char* entry, int what, norm_form form, int branch, const neck_args& a)
{
    const bool shape = what & NECK_CHK_SHAPE, tensors = what & NECK_CHK_TENSORS;
    if (shape && form == NORM_INSTANCE && ctx->cfg.norm_kind != 0)
        return train_fail(ctx, entry, "the InstanceNorm backbone only (BatchNorm has no backward here)");
    if (shape && (branch < 0 || branch > 2)) return train_fail(ctx, entry, "branch must be 0, 1 or 2");
    if (tensors) {
        if (!a.x || !a.wt || !a.y || !a.dy || !a.dw || (form != NORM_INSTANCE && (!a.scale || !a.shift)) || (form == NORM_BATCH && (!a.mean || !a.var)))
            return train_fail(ctx, entry, "null pointer");
        if (!a.dscale != !a.dshift) return train_fail(ctx, entry, "dscale and dshift go together");
        if (a.nb < 1 || a.nb > ctx->max_batch) return train_fail(ctx, entry, "nb must be 1 .. max_batch");
        if (a.chunk_frames < 0) return train_fail(ctx, entry, "chunk_frames must be >= 0");
    }
    if (shape && ((ctx->H % 4) || (ctx->W % 4))) return train_fail(ctx, entry, "BEV grid must be a multiple of 8 in x and y");
    if (tensors) {
        if (!aligned16(a.wt)) return train_fail(ctx, entry, "w must be 16-byte aligned");
        if (((uintptr_t)a.x | (uintptr_t)a.scale | (uintptr_t)a.shift | (uintptr_t)a.mean | (uintptr_t)a.var | (uintptr_t)a.y | (uintptr_t)a.dy |
             (uintptr_t)a.dw | (uintptr_t)a.dx) & 3)
            return train_fail(ctx, entry, "tensors must be 4-byte aligned");
        if (((uintptr_t)a.dscale | (uintptr_t)a.dshift) & 7) return train_fail(ctx, entry, "dscale / dshift must be 8-byte aligned");
    }
    return 0;
}

// ---- everything of a call that is a function of the shapes alone: the branch's geometry, the frames of a chunk, the statistics segments
// (S of seg_len elements of a channel's N = H W), the dw tiles and K ranges over chunks of `kpix` pixels (16 in the fp32 kernels, 32 in
// the 16-bit ones) ----------------------------------------------------------------------------------------------------------------------
struct neck_plan {
    geom g;
    int N, fc, S, seg_len, NBt, cpf, Gp, nw;
    size_t zf_elems; // one frame's Z, elements
    dw_walk walk;
};
inline neck_plan neck_make_plan(const pp_ctx* ctx, int branch, int nb, int chunk_frames, int kpix)
{
    neck_plan p;
    geom& g = p.g;
    g.H = ctx->H; g.W = ctx->W; g.ls = branch; g.s = 1 << branch;
    g.Cin = 64 << branch; g.Cup = branch ? 128 : 64; g.coff = branch == 0 ? 0 : branch == 1 ? 64 : 192;
    g.h = g.H >> branch; g.w = g.W >> branch; g.p = g.h * g.w; g.pld = (g.p + 3) & ~3; g.R = g.Cup * g.s * g.s;
    p.N = g.H * g.W;
    p.zf_elems = (size_t)g.R * g.pld;
    p.fc = pp_chunk_frames(ctx, Z_BUDGET, p.zf_elems * sizeof(float), nb, chunk_frames);
    int S = p.N / 256 < 2048 / g.Cup ? p.N / 256 : 2048 / g.Cup;
    S = S < 1 ? 1 : S > ST_MAX_SEG ? ST_MAX_SEG : S;
    p.seg_len = (p.N + S - 1) / S;
    p.S = (p.N + p.seg_len - 1) / p.seg_len;
    p.NBt = g.R >= 128 ? 4 : 2;
    p.cpf = (g.p + kpix - 1) / kpix; p.nw = g.Cin * g.R;
    p.walk = dw_walk{nb, p.fc, (g.R / (32 * p.NBt)) * (g.Cin / 64), p.cpf, DW_WGS};
    p.Gp = count_partials(p.walk);
    return p;
}

// ---- the one driver of the family.  P holds what the fp32 entries and the 16-bit twin do not share: the pixels of a K chunk (KPIX), the
// dx product's weight image (grow_wt, pack_wt: none in fp32, which reads w itself) and the two product launches (dw, dx).  The forms
// differ in the passes between Z and the products: InstanceNorm runs k_neck_stats and k_neck_dz per chunk; the affine form one pass per
// chunk and k_affine_reduce behind the chunks; the batch form a first round over the chunks for the sums, k_bn_coef, and k_bn_neck_dz in
// the second round ----------------------------------------------------------------------------------------------------------------------
template <typename P>
int neck_run(pp_ctx* ctx, norm_form form, int branch, const neck_args& a)
{
    const int nb = a.nb;
    hipStream_t stream = a.stream;
    PP_HIP(hipSetDevice(ctx->device));
    neck_ws* ws = workspace(ctx);
    const neck_plan p = neck_make_plan(ctx, branch, nb, a.chunk_frames, P::KPIX);
    const geom& g = p.g;
    const int N = p.N, fc = p.fc, S = p.S, slen = p.seg_len;
    // st: InstanceNorm keeps the four sums of a chunk's segments; the other forms the two sums of every frame's, reduced or pooled once
    const size_t st_elems = form == NORM_INSTANCE ? (size_t)fc * g.Cup * S * 4 : (size_t)nb * g.Cup * S * 2;
    int rc;
    if ((rc = grow(ctx, &ws->z, &ws->z_elems, (size_t)fc * p.zf_elems)) ||
        (rc = grow(ctx, &ws->st, &ws->st_elems, st_elems)) ||
        (form == NORM_BATCH && (rc = grow(ctx, &ws->coef, &ws->coef_elems, (size_t)g.Cup * 4))) ||
        (rc = grow(ctx, &ws->part, &ws->part_elems, (size_t)p.Gp * p.nw)) ||
        (a.dx && (rc = P::grow_wt(ctx, ws, p.nw))))
        return rc;
    const int xvec = g.p % 4 == 0 && aligned16(a.x);
    if (a.dx) P::pack_wt(p, ws, a.wt, stream);
    auto fwd = [&](const dw_chunk& c) {
        hipLaunchKernelGGL(k_neck_fwd, dim3(pp_div_up(g.pld, 64), g.R / 64, c.fn), dim3(256), 0, stream, a.x + (size_t)c.f0 * g.Cin * g.p, a.wt, ws->z,
                           g.Cin, g.R, g.p, g.pld);
    };
    // Z is recomputed per chunk into the workspace.  The batch form needs the sums of all frames ahead of dZ.  One chunk: Z stays in place
    // between the sums and dZ.  Several: a first round over the chunks for the sums, a second that recomputes each chunk's Z (the same
    // bits) for dZ and the products.
    const bool z_in_place = form == NORM_BATCH && fc >= nb;
    if (form == NORM_BATCH) {
        for_chunks(p.walk, [&](const dw_chunk& c) {
            fwd(c);
            hipLaunchKernelGGL(k_bn_neck_sums, dim3(S, g.Cup, c.fn), dim3(256), 0, stream, ws->z, a.y + (size_t)c.f0 * 320 * N,
                               a.dy + (size_t)c.f0 * 320 * N, ws->st + (size_t)c.f0 * g.Cup * S * 2, g.Cup, g.coff, g.H, g.W, g.ls, g.w, g.pld, g.R, slen);
        });
        hipLaunchKernelGGL(k_bn_coef, dim3(pp_div_up(g.Cup, 64)), dim3(64), 0, stream, ws->st, nb, g.Cup, S, a.mean, a.var, (double)nb * (double)N,
                           ws->coef, a.dscale, a.dshift);
    }
    for_chunks(p.walk, [&](const dw_chunk& c) {
        const int fn = c.fn;
        const float* xc = a.x + (size_t)c.f0 * g.Cin * g.p;
        const float* yc = a.y + (size_t)c.f0 * 320 * N;
        const float* dyc = a.dy + (size_t)c.f0 * 320 * N;
        if (!z_in_place) fwd(c);
        if (form == NORM_INSTANCE) {
            hipLaunchKernelGGL(k_neck_stats, dim3(S, g.Cup, fn), dim3(256), 0, stream, ws->z, yc, dyc, ws->st, g.Cup, g.coff, g.H, g.W, g.ls, g.w,
                               g.pld, g.R, slen);
            hipLaunchKernelGGL(k_neck_dz, dim3(S, g.Cup, fn), dim3(256), 0, stream, ws->z, yc, dyc, ws->st, g.Cup, g.coff, g.H, g.W, g.ls, g.w, g.pld,
                               g.R, slen);
        } else if (form == NORM_AFFINE) {
            hipLaunchKernelGGL(k_affine_neck_dz, dim3(S, g.Cup, fn), dim3(256), 0, stream, ws->z, yc, dyc, a.scale,
                               ws->st + (size_t)c.f0 * g.Cup * S * 2, g.Cup, g.coff, g.H, g.W, g.ls, g.w, g.pld, g.R, slen);
        } else {
            hipLaunchKernelGGL(k_bn_neck_dz, dim3(S, g.Cup, fn), dim3(256), 0, stream, ws->z, yc, dyc, a.scale, ws->coef, g.Cup, g.coff, g.H, g.W, g.ls,
                               g.w, g.pld, g.R, slen);
        }
        P::dw(p, c, xc, ws->z, ws->part, xvec, stream);
        if (a.dx) P::dx(p, ws, a.wt, ws->z, a.dx + (size_t)c.f0 * g.Cin * g.p, fn, stream);
    });
    launch_dw_reduce(ws->part, p.Gp, p.nw, a.dw, stream);
    if (form == NORM_AFFINE && a.dscale)
        hipLaunchKernelGGL(k_affine_reduce, dim3(pp_div_up(g.Cup, 64)), dim3(64), 0, stream, ws->st, nb, g.Cup, S, a.dscale, a.dshift);
    PP_HIP(hipGetLastError());
    return 0;
}

} // namespace
