// The strided-stage backward's own part of the training host side, shared by down_train.hip (fp32) and down_train16.hip (its 16-bit
// operand twin): the workspace of a context and its budget rules, the parity planes of x, the norm backward of every form (InstanceNorm,
// a frozen BatchNorm's affine, a train-mode BatchNorm) that writes dz into its padded plane, fp32 / fp64 in every mode, and the one
// check, plan and driver of the family.  What the stage shares with the Resnet unit is train_planes.h's (the walk over the padded plane,
// mean / rstd) and train_conv3.h's (the fp32 products, DA_BLOCK, k_bn_plane_sums); what the three families share (workspace growth, the
// padded-plane geometry, the frame chunks and K ranges, the reduction of the dw partials) is train_host.h's.
#pragma once
#include <cmath>
#include "pp_common.h"
#include "train_planes.h"
#include "train_host.h"
#include "train_conv3.h"

namespace {

constexpr size_t DOWN_WS_BUDGET = (size_t)256 << 20; // bytes of one frame's x parity planes + dz planes: a larger map is refused
constexpr size_t DOWN_WS_CHUNK = (size_t)1 << 30;    // bytes of the planes of one chunk of frames: larger batches run in frame chunks

struct down_ws {
    float* planes = nullptr; size_t planes_elems = 0; // xp [fc][Cin][4][PS], then dz [fc][Cout][PS]
    double* pst = nullptr;   size_t pst_elems = 0;    // [2][fc][Cout][segments][2]: a plane's segment sums of (z, z^2), then of (Gr, Gr xhat)
    float* wT = nullptr;     size_t wT_elems = 0;
    float* part = nullptr;   size_t part_elems = 0;
    float* coef = nullptr;   size_t coef_elems = 0;   // [Cout][4]: k_bn_coef's coefficients (pp_down_backward_bn)
    uint16_t* wT16 = nullptr; size_t wT16_elems = 0;  // [part][9][ci][co] bf16: the dgrad's A operand (pp_down_backward_mp, down_train16.hip)
};

// ---- the four parity planes of x: grid (Cin, frames, SP), one slice of LP positions per workgroup.  A position takes its 2 x 2 input
// pixels (x is read once, whole rows at a time) and writes one element of each plane -----------------------------------------------
__global__ void __launch_bounds__(256) k_down_xpack(const float* __restrict__ x, float* __restrict__ xp, int cin, int hin, int win, int ho, int wo,
                                                    int wp, int G, int PP, int PS, int LP)
{
    const size_t pl = (size_t)blockIdx.y * cin + blockIdx.x;
    const float* xi = x + pl * hin * win;
    float* xo = xp + pl * 4 * PS;
    const int lo = blockIdx.z * LP, hi = lo + LP < PS ? lo + LP : PS;
    padded_walk(lo, hi, ho, wo, wp, G, PP, [&](int j, const plane_pos& p) {
        float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f; // (row parity, column parity)
        if (p.inside) {
            const int iy = 2 * p.r, ix = 2 * p.c; // in the image: 2 (ho - 1) < hin, 2 (wo - 1) < win
            const float* r = xi + (size_t)iy * win + ix;
            const bool right = ix + 1 < win, below = iy + 1 < hin;
            v00 = r[0];
            if (right) v01 = r[1];
            if (below) v10 = r[win];
            if (right && below) v11 = r[win + 1];
        }
        xo[j] = v00; xo[PS + j] = v01; xo[2 * PS + j] = v10; xo[3 * PS + j] = v11;
    });
}

// ---- sums of the norm backward: grid (Cout, frames, S), sum Gr and sum Gr xhat of one segment -> pst2.  xhat is evaluated by one
// expression here and in k_down_norm, so the xhat of the mask is the xhat of the product -------------------------------------------
__global__ void __launch_bounds__(256) k_dplane_gstats(const float* __restrict__ z, const float* __restrict__ dy, const double* __restrict__ pst,
                                                       double* __restrict__ pst2, int cout, int N, int L, int S)
{
    __shared__ double red[256][2];
    const int tid = threadIdx.x;
    const size_t pl = (size_t)blockIdx.y * cout + blockIdx.x;
    const float* zi = z + pl * N;
    const float* dp = dy + pl * N;
    float meanf, rstdf;
    plane_mean_rstd(pst, pl, S, N, meanf, rstdf);
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    double sg = 0.0, sgx = 0.0;
    strided4(lo, hi, [&](int i) { return float2{zi[i], dp[i]}; },
             [&](float2 v) {
                 const float xhat = (v.x - meanf) * rstdf;
                 if (xhat > 0.f) {
                     const double g = (double)v.y;
                     sg += g; sgx += g * (double)xhat;
                 }
             });
    block_sum2(sg, sgx, red);
    if (tid == 0) { pst2[(pl * S + blockIdx.z) * 2] = sg; pst2[(pl * S + blockIdx.z) * 2 + 1] = sgx; }
}

// ---- norm backward, z, dy -> dz in the padded plane: grid (Cout, frames, SP), one slice of LP elements of the plane per workgroup -
__global__ void __launch_bounds__(256) k_down_norm(const float* __restrict__ z, const float* __restrict__ dy, float* __restrict__ dzp,
                                                   const double* __restrict__ pst, const double* __restrict__ pst2, int cout, int ho, int wo, int wp,
                                                   int G, int PP, int PS, int S, int LP)
{
    const int N = ho * wo;
    const size_t pl = (size_t)blockIdx.y * cout + blockIdx.x;
    const float* zi = z + pl * N;
    const float* dp = dy + pl * N;
    float meanf, rstdf;
    plane_mean_rstd(pst, pl, S, N, meanf, rstdf);
    double sg = 0.0, sgx = 0.0;
    for (int g = 0; g < S; ++g) { sg += pst2[(pl * S + g) * 2]; sgx += pst2[(pl * S + g) * 2 + 1]; }
    const double inv_n = 1.0 / (double)N;
    const float c1 = (float)(sg * inv_n), c2 = (float)(sgx * inv_n);
    float* zo = dzp + pl * PS;
    const int lo = blockIdx.z * LP, hi = lo + LP < PS ? lo + LP : PS;
    padded_walk(lo, hi, ho, wo, wp, G, PP, [&](int j, const plane_pos& p) {
        float v = 0.f;
        if (p.inside) {
            const int i = p.i;
            const float xhat = (zi[i] - meanf) * rstdf;
            const float g = xhat > 0.f ? dp[i] : 0.f;
            v = rstdf * ((g - c1) - xhat * c2);
        }
        zo[j] = v;
    });
}

// ---- the stage with a per-channel affine in place of the InstanceNorm (pp_down_backward_affine), z, dy -> dz in the padded plane: grid
// (Cout, frames, SP) as k_down_norm.  g = dy [fma(z, scale, shift) > 0], the forward prologue's expression; dz = scale g; and the slice's
// sum g z, sum g in fp64 -> pst[frame][co][slice][2] (every interior element lies in exactly one slice) -----------------------------------
__global__ void __launch_bounds__(256) k_affine_down_dz(const float* __restrict__ z, const float* __restrict__ dy, const float* __restrict__ scale,
                                                        const float* __restrict__ shift, float* __restrict__ dzp, double* __restrict__ pst, int cout,
                                                        int ho, int wo, int wp, int G, int PP, int PS, int LP)
{
    __shared__ double red[256][2];
    const int tid = threadIdx.x, N = ho * wo, SP = gridDim.z;
    const size_t pl = (size_t)blockIdx.y * cout + blockIdx.x;
    const float* zi = z + pl * N;
    const float* dp = dy + pl * N;
    const float sc = scale[blockIdx.x], sh = shift[blockIdx.x];
    float* zo = dzp + pl * PS;
    const int lo = blockIdx.z * LP, hi = lo + LP < PS ? lo + LP : PS;
    double sgz = 0.0, sg = 0.0;
    padded_walk(lo, hi, ho, wo, wp, G, PP, [&](int j, const plane_pos& p) {
        float v = 0.f;
        if (p.inside) {
            const int i = p.i;
            const float zz = zi[i];
            const float g = fmaf(zz, sc, sh) > 0.f ? dp[i] : 0.f;
            sgz += (double)g * (double)zz; sg += (double)g;
            v = sc * g;
        }
        zo[j] = v;
    });
    block_sum2(sgz, sg, red);
    if (tid == 0) { pst[(pl * SP + blockIdx.z) * 2] = sgz; pst[(pl * SP + blockIdx.z) * 2 + 1] = sg; }
}

// ---- the stage in front of a train-mode BatchNorm (pp_down_backward_bn).  The norm backward needs the sums of ALL frames, and they need
// only z and dy, so they come first, over every frame at once: k_bn_plane_sums (train_conv3.h), the segment sums of g = dy
// [fma(z, scale, shift) > 0].  k_bn_down_dz: grid (Cout, frames, SP) as k_down_norm once k_bn_coef has pooled them:
// dz = scale ((g - c1) - zhat c2), zhat = (z - mean) r, into the padded plane -----------------------------------------------------------------
__global__ void __launch_bounds__(256) k_bn_down_dz(const float* __restrict__ z, const float* __restrict__ dy, const float* __restrict__ scale,
                                                    const float* __restrict__ shift, const float* __restrict__ coef, float* __restrict__ dzp, int cout,
                                                    int ho, int wo, int wp, int G, int PP, int PS, int LP)
{
    const int N = ho * wo, co = blockIdx.x;
    const size_t pl = (size_t)blockIdx.y * cout + co;
    const float* zi = z + pl * N;
    const float* dp = dy + pl * N;
    const float sc = scale[co], sh = shift[co];
    const float c1 = coef[4 * co], c2 = coef[4 * co + 1], meanf = coef[4 * co + 2], rf = coef[4 * co + 3];
    float* zo = dzp + pl * PS;
    const int lo = blockIdx.z * LP, hi = lo + LP < PS ? lo + LP : PS;
    padded_walk(lo, hi, ho, wo, wp, G, PP, [&](int j, const plane_pos& p) {
        float v = 0.f;
        if (p.inside) {
            const int i = p.i;
            const float zz = zi[i];
            const float g = fmaf(zz, sc, sh) > 0.f ? dp[i] : 0.f;
            const float zhat = (zz - meanf) * rf;
            v = sc * ((g - c1) - zhat * c2);
        }
        zo[j] = v;
    });
}

inline down_ws* workspace(pp_ctx* ctx)
{
    if (!ctx->down) ctx->down = new down_ws();
    return (down_ws*)ctx->down;
}

// ---- one call: its shape, its arguments (the ones a form does not take stay null / 0) ----------------------------------------------------
struct down_shape { int cin, cout, hin, win; };
struct down_args {
    const float *x = nullptr, *wgt = nullptr, *z = nullptr, *scale = nullptr, *shift = nullptr, *mean = nullptr, *var = nullptr, *dy = nullptr;
    int nb = 0;
    float *dw = nullptr, *dx = nullptr;
    double *dscale = nullptr, *dshift = nullptr;
    int chunk_frames = 0;
    hipStream_t stream = nullptr;
};

// bytes of one frame's planes
inline uint64_t down_frame_bytes(const down_shape& s)
{
    return (uint64_t)(4 * s.cin + s.cout) * padded_plane(((int64_t)s.hin + 1) / 2, ((int64_t)s.win + 1) / 2).elems * sizeof(float);
}

// The checks of every entry of the family, reported as "<entry>: ...", in the order the fp32 entries test them.  `what` selects the ones
// that read the shape alone (DOWN_CHK_SHAPE: pp_down_backward_path runs just these, pp_down_backward_mp runs them first) and the ones
// that read the tensors and nb.  Only the InstanceNorm form refuses a BatchNorm context; the affine and batch forms add their own
// pointers to the null test; the tests of dscale / dshift and chunk_frames pass where a form leaves those null / 0.
enum { DOWN_CHK_SHAPE = 1, DOWN_CHK_TENSORS = 2, DOWN_CHK_ALL = 3 };
inline int down_check(pp_ctx* ctx, const char* entry, int what, norm_form form, const down_shape& s, const down_args& a)
{
    const bool shape = what & DOWN_CHK_SHAPE, tensors = what & DOWN_CHK_TENSORS;
    const int cin = s.cin, cout = s.cout;
    if (shape && form == NORM_INSTANCE && ctx->cfg.norm_kind != 0)
        return train_fail(ctx, entry, "the InstanceNorm backbone only (BatchNorm has no backward here)");
    if (shape && !((cin == 64 && cout == 64) || (cin == 64 && cout == 128) || (cin == 128 && cout == 256)))
        return train_fail(ctx, entry, "(cin, cout) must be (64, 64), (64, 128) or (128, 256)");
    if (tensors) {
        if (!a.x || !a.wgt || !a.z || !a.dy || !a.dw || (form != NORM_INSTANCE && (!a.scale || !a.shift)) || (form == NORM_BATCH && (!a.mean || !a.var)))
            return train_fail(ctx, entry, "null pointer");
        if (!a.dscale != !a.dshift) return train_fail(ctx, entry, "dscale and dshift go together");
        if (a.nb < 1 || a.nb > ctx->max_batch) return train_fail(ctx, entry, "nb must be 1 .. max_batch");
        if (a.chunk_frames < 0) return train_fail(ctx, entry, "chunk_frames must be >= 0");
    }
    if (shape && (s.hin < 1 || s.win < 1 || (((int64_t)s.hin + 1) / 2) * (((int64_t)s.win + 1) / 2) < 2))
        return train_fail(ctx, entry, "hin, win >= 1 and ho wo >= 2");
    if (tensors) {
        if (!aligned16(a.wgt)) return train_fail(ctx, entry, "w must be 16-byte aligned");
        if (((uintptr_t)a.x | (uintptr_t)a.z | (uintptr_t)a.scale | (uintptr_t)a.shift | (uintptr_t)a.mean | (uintptr_t)a.var | (uintptr_t)a.dy |
             (uintptr_t)a.dw | (uintptr_t)a.dx) & 3)
            return train_fail(ctx, entry, "tensors must be 4-byte aligned");
        if (((uintptr_t)a.dscale | (uintptr_t)a.dshift) & 7) return train_fail(ctx, entry, "dscale / dshift must be 8-byte aligned");
    }
    if (shape && down_frame_bytes(s) > DOWN_WS_BUDGET)
        return train_fail(ctx, entry, "map too large (one frame's planes exceed the 256 MB workspace)");
    return 0;
}

// ---- everything of a call that is a function of the shapes alone: the padded half-resolution plane, the frames of a chunk, the wgrad
// tiles and K ranges over chunks of `kpos` positions (16 in the fp32 kernels, 32 in the 16-bit ones) aiming at `wgs` workgroups, the
// segments of the streaming passes over the tight output plane (S, L: statistics) and the padded one (SP, LP: dz, the planes of x) ------
struct down_plan {
    down_shape s;
    pad_geom g;
    int ho, wo, No, fc, TN, NC, cpf, Gp, nw, S, L, SP, LP;
    size_t pf_elems; // one frame's planes, elements
    dw_walk walk;
};
inline down_plan down_make_plan(const pp_ctx* ctx, const down_shape& s, int nb, int chunk_frames, int kpos, int wgs)
{
    down_plan p;
    p.s = s;
    p.ho = (s.hin + 1) / 2; p.wo = (s.win + 1) / 2; p.No = p.ho * p.wo;
    p.g = padded_plane(p.ho, p.wo);
    p.pf_elems = (size_t)(4 * s.cin + s.cout) * p.g.PS;
    p.fc = pp_chunk_frames(ctx, DOWN_WS_CHUNK, p.pf_elems * sizeof(float), nb, chunk_frames);
    p.TN = s.cin >= 128 ? 128 : 192; // columns of a wgrad tile: k_conv3_wgrad / k_down_wgrad16 <4, 2> or <3, 4>
    p.NC = 9 * s.cin; p.cpf = (p.g.PP + kpos - 1) / kpos; p.nw = s.cout * p.NC;
    p.walk = dw_walk{nb, p.fc, (p.NC / p.TN) * (s.cout / 64), p.cpf, wgs};
    p.Gp = count_partials(p.walk);
    p.S = plane_segs(p.No); p.L = seg_len(p.No, p.S); p.SP = plane_segs(p.g.PS); p.LP = seg_len(p.g.PS, p.SP);
    return p;
}

// ---- the one driver of the family.  P holds what the fp32 entries and the 16-bit twin do not share: the positions of a K chunk and the
// workgroups a wgrad launch aims at (KPOS, WGS), the dgrad's weight image (grow_wt, pack_wt) and the two product launches (wgrad, dgrad).
// The forms differ in the passes around the products: InstanceNorm runs the statistics, their backward sums and k_down_norm per chunk;
// the affine form one pass per chunk and k_affine_reduce behind the chunks; the batch form its sums over all frames and k_bn_coef ahead
// of the chunks and k_bn_down_dz in them ----------------------------------------------------------------------------------------------
template <typename P>
int down_run(pp_ctx* ctx, norm_form form, const down_shape& s, const down_args& a)
{
    const int cin = s.cin, cout = s.cout, hin = s.hin, win = s.win, nb = a.nb;
    hipStream_t stream = a.stream;
    PP_HIP(hipSetDevice(ctx->device));
    down_ws* ws = workspace(ctx);
    const down_plan p = down_make_plan(ctx, s, nb, a.chunk_frames, P::KPOS, P::WGS);
    const int ho = p.ho, wo = p.wo, wp = p.g.wp, PP = p.g.PP, G = p.g.G, PS = p.g.PS, fc = p.fc, No = p.No, S = p.S, L = p.L, SP = p.SP, LP = p.LP;
    // pst: InstanceNorm keeps both sets of a chunk's segment sums; the other forms every frame's sums, reduced or pooled once
    const size_t pst_elems = form == NORM_INSTANCE ? 2 * (size_t)fc * cout * SEG_MAX * 2 : (size_t)nb * cout * SEG_MAX * 2;
    int rc;
    if ((rc = grow(ctx, &ws->planes, &ws->planes_elems, (size_t)fc * p.pf_elems)) ||
        (rc = grow(ctx, &ws->pst, &ws->pst_elems, pst_elems)) ||
        (form == NORM_BATCH && (rc = grow(ctx, &ws->coef, &ws->coef_elems, (size_t)cout * 4))) ||
        (rc = grow(ctx, &ws->part, &ws->part_elems, (size_t)p.Gp * p.nw)) ||
        (a.dx && (rc = P::grow_wt(ctx, ws, p.nw))))
        return rc;
    float* xp = ws->planes;
    float* dzp = ws->planes + (size_t)fc * cin * 4 * PS;
    if (a.dx) P::pack_wt(p, ws, a.wgt, stream);
    if (form == NORM_BATCH) {
        hipLaunchKernelGGL(k_bn_plane_sums, dim3(cout, nb, S), dim3(256), 0, stream, a.z, a.dy, a.scale, a.shift, ws->pst, cout, No, L, S);
        hipLaunchKernelGGL(k_bn_coef, dim3(pp_div_up(cout, 64)), dim3(64), 0, stream, ws->pst, nb, cout, S, a.mean, a.var, (double)nb * (double)No,
                           ws->coef, a.dscale, a.dshift);
    }
    const size_t nin = (size_t)hin * win, nout = (size_t)No;
    for_chunks(p.walk, [&](const dw_chunk& c) {
        const int fn = c.fn;
        const size_t oi = (size_t)c.f0 * cin * nin, oo = (size_t)c.f0 * cout * nout;
        const float* z = a.z + oo;
        const float* dy = a.dy + oo;
        hipLaunchKernelGGL(k_down_xpack, dim3(cin, fn, SP), dim3(256), 0, stream, a.x + oi, xp, cin, hin, win, ho, wo, wp, G, PP, PS, LP);
        if (form == NORM_INSTANCE) {
            double* pst2 = ws->pst + (size_t)fc * cout * SEG_MAX * 2;
            hipLaunchKernelGGL(k_plane_stats, dim3(cout, fn, S), dim3(256), 0, stream, z, ws->pst, cout, No, L, S);
            hipLaunchKernelGGL(k_dplane_gstats, dim3(cout, fn, S), dim3(256), 0, stream, z, dy, ws->pst, pst2, cout, No, L, S);
            hipLaunchKernelGGL(k_down_norm, dim3(cout, fn, SP), dim3(256), 0, stream, z, dy, dzp, ws->pst, pst2, cout, ho, wo, wp, G, PP, PS, S, LP);
        } else if (form == NORM_AFFINE) {
            hipLaunchKernelGGL(k_affine_down_dz, dim3(cout, fn, SP), dim3(256), 0, stream, z, dy, a.scale, a.shift, dzp,
                               ws->pst + (size_t)c.f0 * cout * SP * 2, cout, ho, wo, wp, G, PP, PS, LP);
        } else {
            hipLaunchKernelGGL(k_bn_down_dz, dim3(cout, fn, SP), dim3(256), 0, stream, z, dy, a.scale, a.shift, ws->coef, dzp, cout, ho, wo, wp, G, PP,
                               PS, LP);
        }
        P::wgrad(p, c, dzp, xp, ws->part, stream);
        if (a.dx) P::dgrad(p, ws, dzp, a.dx + oi, fn, stream);
    });
    launch_dw_reduce(ws->part, p.Gp, p.nw, a.dw, stream);
    if (form == NORM_AFFINE && a.dscale)
        hipLaunchKernelGGL(k_affine_reduce, dim3(pp_div_up(cout, 64)), dim3(64), 0, stream, ws->pst, nb, cout, SP, a.dscale, a.dshift);
    PP_HIP(hipGetLastError());
    return 0;
}

} // namespace
