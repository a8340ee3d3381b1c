// The Resnet unit backward's own part of the training host side, shared by block_train.hip (fp32) and block_train16.hip (its 16-bit
// operand twins): the workspace of a context and its budget rules, the one check and plan of the family, and the passes behind the
// dgrad of the two BatchNorm forms (k_affine_unit_du, k_bn_unit_du; the batch form's sums are train_conv3.h's k_bn_plane_sums), which
// read u and du only.  The fp32 driver
// (unit_run) is block_train.hip's; the twin keeps a driver of its own (its pack, its InstanceNorm kernels and images differ) over the
// same check, plan and chunk walk.  What the three families share (workspace growth, the padded-plane geometry, the frame chunks and K ranges, the
// reduction of the dw partials) is train_host.h's.
#pragma once
#include "pp_common.h"
#include "train_planes.h"
#include "train_host.h"
#include "train_conv3.h"

namespace {

constexpr size_t WS_BUDGET = (size_t)256 << 20; // bytes of one frame's a + dz planes: a larger map is refused
constexpr size_t WS_CHUNK = (size_t)1 << 30;    // bytes of the planes of one chunk of frames: larger batches run in frame chunks

struct block_ws {
    float* planes = nullptr; size_t planes_elems = 0; // a [fc][C][PS], then dz [fc][C][PS]
    float* stm = nullptr;    size_t stm_elems = 0;    // [fc][C][2]: mean, rstd as the forward rounds them
    double* pst = nullptr;   size_t pst_elems = 0;    // [fc][C][segments][2]: a plane's segment sums (statistics, then the norm backward's)
    float* wT = nullptr;     size_t wT_elems = 0;
    float* part = nullptr;   size_t part_elems = 0;
    uint16_t* img16 = nullptr; size_t img16_elems = 0; // the 16-bit operand images of pp_unit_backward_mp (block_train16.hip)
    uint16_t* wT16 = nullptr;  size_t wT16_elems = 0;  // [part][9][ci][co] bf16
    // pp_update_conv_image: the committed images of the sixteen 3 x 3 convolutions in execution order and their position maps on
    // the device, each entry read back on its first use after a commit
    uint64_t img_gen[16] = {}; // ctx->commit_gen the entry belongs to (0: none)
    pp_block_image img[16];
    int32_t* pmap[16] = {};
};

inline block_ws* workspace(pp_ctx* ctx)
{
    if (!ctx->blk) ctx->blk = new block_ws();
    return (block_ws*)ctx->blk;
}

// ---- one call: its shape, its arguments (the ones a form does not take stay null / 0) ----------------------------------------------------
struct unit_shape { int C, h, w; };
struct unit_args {
    const float *u = nullptr, *wgt = nullptr, *scale = nullptr, *shift = nullptr, *mean = nullptr, *var = nullptr, *dy = nullptr, *dskip = nullptr;
    int nb = 0;
    float *dw = nullptr, *du = nullptr;
    double *dscale = nullptr, *dshift = nullptr;
    int chunk_frames = 0;
    hipStream_t stream = nullptr;
};

// The checks of every entry of the family, reported as "<entry>: ...", in the order the fp32 entries test them.  `what` selects the ones
// that read the shape alone (UNIT_CHK_SHAPE: pp_unit_backward_path runs just these, pp_unit_backward_mp runs them first), the ones
// that read the tensors and nb, and the budget of the fp32 planes (the 16-bit images have a budget of their own, which decides the
// path).  Only the InstanceNorm form refuses a BatchNorm context; the affine and batch forms add their own pointers to the null test;
// the tests of dscale / dshift and chunk_frames pass where a form leaves those null / 0.
enum { UNIT_CHK_SHAPE = 1, UNIT_CHK_TENSORS = 2, UNIT_CHK_BUDGET = 4, UNIT_CHK_ALL = 7 };
inline int unit_check(pp_ctx* ctx, const char* entry, int what, norm_form form, const unit_shape& s, const unit_args& a)
{
    const bool shape = what & UNIT_CHK_SHAPE, tensors = what & UNIT_CHK_TENSORS;
    if (shape && form == NORM_INSTANCE && ctx->cfg.norm_kind != 0)
        return train_fail(ctx, entry, "the InstanceNorm backbone only (BatchNorm has no backward here)");
    if (shape && s.C != 64 && s.C != 128 && s.C != 256) return train_fail(ctx, entry, "C must be 64, 128 or 256");
    if (tensors) {
        if (!a.u || !a.wgt || !a.dy || !a.dw || (form != NORM_INSTANCE && (!a.scale || !a.shift)) || (form == NORM_BATCH && (!a.mean || !a.var)))
            return train_fail(ctx, entry, "null pointer");
        if (!a.dscale != !a.dshift) return train_fail(ctx, entry, "dscale and dshift go together");
        if (!a.du && a.dscale) return train_fail(ctx, entry, "dscale and dshift need du (they are sums over the dgrad product)");
        if (a.nb < 1 || a.nb > ctx->max_batch) return train_fail(ctx, entry, "nb must be 1 .. max_batch");
        if (a.chunk_frames < 0) return train_fail(ctx, entry, "chunk_frames must be >= 0");
    }
    if (shape && (s.h < 1 || s.w < 1 || (int64_t)s.h * s.w < 2)) return train_fail(ctx, entry, "h, w >= 1 and h w >= 2");
    if (tensors) {
        if (!aligned16(a.wgt)) return train_fail(ctx, entry, "w must be 16-byte aligned");
        if (((uintptr_t)a.u | (uintptr_t)a.scale | (uintptr_t)a.shift | (uintptr_t)a.mean | (uintptr_t)a.var | (uintptr_t)a.dy | (uintptr_t)a.dskip |
             (uintptr_t)a.dw | (uintptr_t)a.du) & 3)
            return train_fail(ctx, entry, "tensors must be 4-byte aligned");
        if (((uintptr_t)a.dscale | (uintptr_t)a.dshift) & 7) return train_fail(ctx, entry, "dscale / dshift must be 8-byte aligned");
    }
    if ((what & UNIT_CHK_BUDGET) && 2 * (uint64_t)s.C * padded_plane(s.h, s.w).elems * sizeof(float) > WS_BUDGET)
        return train_fail(ctx, entry, "map too large (one frame's planes exceed the 256 MB workspace)");
    return 0;
}

// ---- the passes behind the dgrad of the two BatchNorm forms, run by the fp32 driver and by the 16-bit twin.  a = max(fma(u, scale,
// shift), 0) is the forward prologue's expression (affine_relu); fma rounds once and keeps the sign, so fma(u, scale, shift) > 0,
// re-evaluated from u, is the mask a > 0 bit for bit.
// k_affine_unit_du: grid (C, frames, S), in place over da: g = da [a > 0], du = scale g (+ dskip), and the segment's sum g u, sum g in
// fp64 -> pst[frame][c][segment][2].  FROM_U = false reads the mask from the fp32 plane of a (ap); FROM_U = true re-evaluates it from u:
// the twin keeps no fp32 image of a (ap is null there) --------------------------------------------------------------------------------------
__device__ __forceinline__ float affine_relu(float u, float sc, float sh) { return fmaxf(fmaf(u, sc, sh), 0.f); }

template <bool FROM_U>
__global__ void __launch_bounds__(256) k_affine_unit_du(const float* __restrict__ u, const float* __restrict__ ap, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, const float* __restrict__ dskip, float* __restrict__ du,
                                                        double* __restrict__ pst, int C, int w, int wp, int G, int PS, int N, int L, int S)
{
    __shared__ double red[256][2];
    const int tid = threadIdx.x;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float* up = u + pl * N;
    const float* ai = FROM_U ? nullptr : ap + pl * PS + G + wp + 1; // interior origin
    float* dp = du + pl * N;
    const float sc = scale[blockIdx.x], sh = FROM_U ? shift[blockIdx.x] : 0.f;
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    double sgu = 0.0, sg = 0.0;
    for (int i = lo + tid; i < hi; i += 256) {
        const float uu = up[i];
        bool on;
        if (FROM_U) {
            on = fmaf(uu, sc, sh) > 0.f;
        } else {
            const int y = i / w, x = i - y * w;
            on = ai[y * wp + x] > 0.f;
        }
        const float g = on ? dp[i] : 0.f;
        sgu += (double)g * (double)uu; sg += (double)g;
        float v = sc * g;
        if (dskip) v = v + dskip[pl * N + i];
        dp[i] = v;
    }
    block_sum2(sgu, sg, red);
    if (tid == 0) { pst[(pl * S + blockIdx.z) * 2] = sgu; pst[(pl * S + blockIdx.z) * 2 + 1] = sg; }
}

// ---- the unit behind a train-mode BatchNorm (pp_unit_backward_bn): k_affine_unit_pack and the two products as above, the raw da left in
// du.  The norm backward needs the sums of ALL frames, so it runs behind the frame chunks, on u and du alone: the mask is re-evaluated
// by the pack's own fma.  k_bn_plane_sums (train_conv3.h) takes each chunk's segment sums of g = da [fma(u, scale, shift) > 0].
// k_bn_unit_du: grid (C, frames, S), in place once k_bn_coef has pooled them: du = scale ((g - c1) - xhat c2) (+ dskip),
// xhat = (u - mean) r --------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bn_unit_du(const float* __restrict__ u, const float* __restrict__ scale, const float* __restrict__ shift,
                                                    const float* __restrict__ coef, const float* __restrict__ dskip, float* __restrict__ du, int C,
                                                    int N, int L)
{
    const int tid = threadIdx.x, c = blockIdx.x;
    const size_t pl = (size_t)blockIdx.y * C + c;
    const float* up = u + pl * N;
    float* dp = du + pl * N;
    const float sc = scale[c], sh = shift[c];
    const float c1 = coef[4 * c], c2 = coef[4 * c + 1], meanf = coef[4 * c + 2], rf = coef[4 * c + 3];
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    for (int i = lo + tid; i < hi; i += 256) {
        const float uu = up[i];
        const float g = fmaf(uu, sc, sh) > 0.f ? dp[i] : 0.f;
        const float xhat = (uu - meanf) * rf;
        float v = sc * ((g - c1) - xhat * c2);
        if (dskip) v = v + dskip[pl * N + i];
        dp[i] = v;
    }
}

// ---- everything of a call that is a function of the shapes (and, for the twin, the mode) alone: the planes `g` (padded_plane for fp32,
// planes16 for the 16-bit images), the frames of a chunk at frame_bytes each, the wgrad tiles (TN columns x tile_rows rows) and K ranges
// over chunks of `kpos` positions (16 in the fp32 kernels, 32 in the 16-bit ones), the segments of the streaming passes over the tight
// plane (S, L: statistics, norm backward) and the padded one (SP, LP: pack) -------------------------------------------------------------
struct unit_plan {
    unit_shape s;
    pad_geom g;
    int N, fc, TN, NC, cpf, Gp, nw, S, L, SP, LP;
    size_t pf_elems; // one frame's plane set [C][PS], elements
    dw_walk walk;
};
inline unit_plan unit_make_plan(const pp_ctx* ctx, const unit_shape& s, int nb, int chunk_frames, const pad_geom& g, size_t frame_bytes, int kpos,
                                int tile_rows)
{
    unit_plan p;
    p.s = s; p.g = g; p.N = s.h * s.w;
    p.pf_elems = (size_t)s.C * g.PS;
    p.fc = pp_chunk_frames(ctx, WS_CHUNK, frame_bytes, nb, chunk_frames);
    p.TN = s.C >= 128 ? 128 : 192; // columns of a wgrad tile
    p.NC = 9 * s.C; p.cpf = (g.PP + kpos - 1) / kpos; p.nw = s.C * p.NC;
    p.walk = dw_walk{nb, p.fc, (p.NC / p.TN) * (s.C / tile_rows), p.cpf, DW_WGS};
    p.Gp = count_partials(p.walk);
    p.S = plane_segs(p.N); p.L = seg_len(p.N, p.S); p.SP = plane_segs(g.PS); p.LP = seg_len(g.PS, p.SP);
    return p;
}

} // namespace
