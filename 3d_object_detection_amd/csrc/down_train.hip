// Training side of the backbone (gfx950): the backward of one strided stage, Conv2d(Cin -> Cout, 3 x 3, stride 2, pad 1, no bias) ->
// InstanceNorm2d(eps 1e-3, no affine) -> ReLU, the head of every block of RPN (pointpillars8_shared.py:143-161).  fp32 throughout,
// InstanceNorm backbone only, generic in (Cin, Cout) = (64, 64) | (64, 128) | (128, 256) and in the map size (odd sizes included).
//
// With ho = (Hin + 1) / 2, wo = (Win + 1) / 2, a stride-2 tap reads input row 2 oy + ky - 1: an even row (ky = 1) or an odd one (ky = 0
// at half-row oy - 1, ky = 2 at half-row oy), and likewise along a row.  So x is de-interleaved into its four row / column parity planes
// (py, px), plane element (r, c) = x[2 r + py][2 c + px] (zero past the input), and every plane, like dz, takes the padded layout of
// block_train.hip at half resolution: the (ho + 2) x wp zero-haloed image, wp = wo + 2, PP = (ho + 2) wp elements, between two guard
// bands of G >= wp + 17 zeros, PS elements in all (G and PS multiples of 4).  Tap t = (ky, kx) is then plane (ky != 1, kx != 1) shifted
// by the flat offset off_t = -(ky == 0) wp - (kx == 0), every shifted read stays inside the plane, and halo x anything = 0:
//   k_conv3_wt     wT[t][co][ci] = w[co][ci][t]: the dgrad's A operand, contiguous along its rows (train_conv3.h)
//   k_down_xpack   per (frame, ci, slice): the four parity planes of x (halo and guards rewritten), x read once
//   k_plane_stats  per (frame, co, segment): sum z, sum z^2 in fp64 over one segment of the plane (train_planes.h)
//   k_dplane_gstats  per (frame, co, segment): mean / rstd as the forward rounds them from the segments' sums added in index order,
//                  Gr = dy [xhat > 0], sum Gr, sum Gr xhat in fp64 over the segment
//   k_down_norm    per (frame, co, slice): both sets of segment sums added in index order, dz = rstd (Gr - mean(Gr) - xhat mean(Gr xhat))
//                  into the padded plane
// A plane is cut into plane_segs(elements) segments, a function of the plane size alone (train_planes.h, shared with block_train.hip: one segment up to 16384
// elements: block 3's 100 x 100 output planes run as one workgroup each, level 0's 400 x 400 as ten).
//   k_conv3_wgrad  dw[co][(ci, t)] = sum_{frame, P} dz[co][P] xp[ci][plane_t][P + off_t]    M = Cout, N = 9 Cin, K = frames x PP in ranges
//                  (train_conv3.h's kernel with the stride-2 taps, taps_s2)
//   k_dw_reduce    partials summed in index order (double, rounded once; train_host.h, shared by the three families)
//   k_down_dgrad   per output parity class (py, px), P the half-resolution position of x[2 r + py][2 c + px]:
//                  dx[ci][P] = sum_{t in class, co} wT[t][co][ci] dz[co][P + (py & ky == 0) wp + (px & kx == 0)]
//                  M = Cin, N = PP, K = Cout x {1, 2, 2, 4} taps (even: the centre tap; odd: taps 0 and 2), summed in blocks of DA_BLOCK
//                  (each tap by train_conv3.h's conv3_dgrad_tap)
// The two products run on v_mfma_f32_16x16x4_f32 with operands straight from global memory, as in block_train.hip.
//
// Determinism: no atomics at all.  Every reduction has a fixed shape: a workgroup's 256 strided fp64 partials are added in index
// order, a plane's segment sums likewise; segments and K ranges of the wgrad depend on the shapes only.  A frame's dz and dx do not depend on the batch it rides in; dw depends on
// nb within fp32 summation error (the K ranges do), and not on whether dx is asked for.
// pp_down_backward_affine is the same stage with a per-channel affine (a frozen BatchNorm2d) for the norm: k_affine_down_dz in place
// of the three norm passes, then the same products and k_affine_reduce; pp_down_backward itself stays the InstanceNorm backbone's.
// pp_down_backward_bn is that stage in front of a train-mode BatchNorm2d (batch statistics pooled over the frames): k_bn_plane_sums over
// all frames and k_bn_coef ahead of the chunks, k_bn_down_dz in them.
// The plane and norm kernels of every form and the family's one check, plan and driver (down_check, down_make_plan, down_run) are
// down_train.h's, shared with the 16-bit twin; the fp32 products are train_conv3.h's, shared with block_train.hip; this file holds the
// stage's dgrad (its taps and its store), the launches of the products and the entries, thin wrappers over them.
#include <cmath>
#include "pp_common.h"
#include "train_planes.h"

#include "down_train.h"

namespace {

// ---- dgrad: grid (position tiles, 4 parity classes, frames).  A workgroup covers ALL Cin channels (WM = Cin / 64 waves down, 4 / WM
// across), each wave 64 ci x 32 half-resolution positions, so dz is read once per tap.  K = (t in class, co): the class's taps in order,
// each tap's blocked sum over co by conv3_dgrad_tap.
// Positions past PP read a clamped index and are never stored; a position is stored where its input pixel (2 r + py, 2 c + px) exists,
// into the tight [Cin][Hin][Win] plane of dx.
template <int WM>
__global__ void __launch_bounds__(256) k_down_dgrad(const float* __restrict__ wT, const float* __restrict__ dzp, float* __restrict__ dx, int cin,
                                                    int cout, int hin, int win, int wp, int G, int PP, int PS)
{
    constexpr int WN = 4 / WM;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int ci0 = 64 * (wave / WN), p0 = blockIdx.x * (32 * WN) + 32 * (wave % WN);
    const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
    const float* zf = dzp + (size_t)blockIdx.z * cout * PS + G;
    float* dxf = dx + (size_t)blockIdx.z * cin * hin * win;
    f32x4 tot[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) tot[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int P0 = p0 + l16, P1 = p0 + 16 + l16;
    const int i0 = P0 < PP ? P0 : 0, i1 = P1 < PP ? P1 : 0;
    for (int ky = py ? 0 : 1; ky < 3; ky += 2)
        for (int kx = px ? 0 : 1; kx < 3; kx += 2) {
            const int t = ky * 3 + kx, off = (ky == 0 ? wp : 0) + (kx == 0 ? 1 : 0);
            conv3_dgrad_tap(tot, wT + (size_t)t * cout * cin + ci0 + l16, zf, off, i0, i1, q, cin, cout, PS);
        }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int P = p0 + 16 * b + l16;
        if (P >= PP) continue;
        const int y = P / wp, c = P - y * wp;
        if (y < 1 || c < 1) continue;
        const int iy = 2 * (y - 1) + py, ix = 2 * (c - 1) + px;
        if (iy >= hin || ix >= win) continue; // covers the lower / right halo as well: 2 ho + py >= hin, 2 wo + px >= win
        float* o = dxf + (size_t)iy * win + ix;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[(size_t)(ci0 + 16 * a + 4 * q + i) * hin * win] = tot[a][b][i];
    }
}

// the fp32 products of down_run (down_train.h)
struct down_fp32 {
    static constexpr int KPOS = 16, WGS = DW_WGS;
    static int grow_wt(pp_ctx* ctx, down_ws* ws, int nw) { return grow(ctx, &ws->wT, &ws->wT_elems, (size_t)nw); }
    static void pack_wt(const down_plan& p, down_ws* ws, const float* wgt, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_conv3_wt, dim3(pp_div_up(p.nw, 256)), dim3(256), 0, stream, wgt, ws->wT, p.s.cin, p.s.cout);
    }
    static void wgrad(const down_plan& p, const dw_chunk& c, const float* dzp, const float* xp, float* part, hipStream_t stream)
    {
        const int cin = p.s.cin, cout = p.s.cout;
        const dim3 gd(p.NC / p.TN, cout / 64, c.sp);
        if (cin >= 128)
            hipLaunchKernelGGL((k_conv3_wgrad<4, 2, taps_s2>), gd, dim3(256), 0, stream, dzp, xp, part, cin, cout, p.g.wp, p.g.G, p.g.PS, p.cpf, c.nchunks, c.cps,
                               c.gbase);
        else
            hipLaunchKernelGGL((k_conv3_wgrad<3, 4, taps_s2>), gd, dim3(256), 0, stream, dzp, xp, part, cin, cout, p.g.wp, p.g.G, p.g.PS, p.cpf, c.nchunks, c.cps,
                               c.gbase);
    }
    static void dgrad(const down_plan& p, const down_ws* ws, const float* dzp, float* dx, int fn, hipStream_t stream)
    {
        const int cin = p.s.cin, cout = p.s.cout, PP = p.g.PP;
        if (cin == 64)
            hipLaunchKernelGGL(k_down_dgrad<1>, dim3(pp_div_up(PP, 128), 4, fn), dim3(256), 0, stream, ws->wT, dzp, dx, cin, cout, p.s.hin, p.s.win,
                               p.g.wp, p.g.G, PP, p.g.PS);
        else
            hipLaunchKernelGGL(k_down_dgrad<2>, dim3(pp_div_up(PP, 64), 4, fn), dim3(256), 0, stream, ws->wT, dzp, dx, cin, cout, p.s.hin, p.s.win,
                               p.g.wp, p.g.G, PP, p.g.PS);
    }
};

int down_entry(pp_ctx* ctx, const char* entry, norm_form form, const down_shape& s, const down_args& a)
{
    if (!ctx) return PP_E_ARG;
    if (int rc = down_check(ctx, entry, DOWN_CHK_ALL, form, s, a)) return rc;
    return down_run<down_fp32>(ctx, form, s, a);
}

} // namespace

void pp_down_destroy(pp_ctx* ctx)
{
    down_ws* w = (down_ws*)ctx->down;
    if (!w) return;
    void* q[] = {w->planes, w->pst, w->wT, w->part, w->coef, w->wT16};
    for (void* x : q)
        if (x) (void)hipFree(x);
    delete w;
    ctx->down = nullptr;
}

extern "C" int pp_down_backward(pp_ctx* ctx, int cin, int cout, int hin, int win, const float* x, const float* wgt, const float* z, const float* dy,
                                int nb, float* dw, float* dx, void* stream_)
{
    down_args a;
    a.x = x; a.wgt = wgt; a.z = z; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx; a.stream = (hipStream_t)stream_;
    return down_entry(ctx, "pp_down_backward", NORM_INSTANCE, down_shape{cin, cout, hin, win}, a);
}

// pp_down_backward with a per-channel affine for the norm: one pass writes dz and the sums where the sibling runs three, and the two
// products run over the same planes, K ranges and frame chunks.
extern "C" int pp_down_backward_affine(pp_ctx* ctx, int cin, int cout, int hin, int win, const float* x, const float* wgt, const float* z,
                                       const float* scale, const float* shift, const float* dy, int nb, float* dw, float* dx, double* dscale,
                                       double* dshift, void* stream_)
{
    down_args a;
    a.x = x; a.wgt = wgt; a.z = z; a.scale = scale; a.shift = shift; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx;
    a.dscale = dscale; a.dshift = dshift; a.stream = (hipStream_t)stream_;
    return down_entry(ctx, "pp_down_backward_affine", NORM_AFFINE, down_shape{cin, cout, hin, win}, a);
}

// pp_down_backward_affine behind a train-mode BatchNorm: (scale, shift) are the fold of the batch statistics (mean, var) the forward used.
// Two phases: the sums over every frame and k_bn_coef first, then the frame chunks with k_bn_down_dz and the two products.  chunk_frames
// > 0 caps the frames of a chunk below the workspace rule (dx and the sums do not depend on it; dw does within fp32 summation error).
extern "C" int pp_down_backward_bn(pp_ctx* ctx, int cin, int cout, int hin, int win, const float* x, const float* wgt, const float* z,
                                   const float* scale, const float* shift, const float* mean, const float* var, const float* dy, int nb, float* dw,
                                   float* dx, double* dscale, double* dshift, int chunk_frames, void* stream_)
{
    down_args a;
    a.x = x; a.wgt = wgt; a.z = z; a.scale = scale; a.shift = shift; a.mean = mean; a.var = var; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx;
    a.dscale = dscale; a.dshift = dshift; a.chunk_frames = chunk_frames; a.stream = (hipStream_t)stream_;
    return down_entry(ctx, "pp_down_backward_bn", NORM_BATCH, down_shape{cin, cout, hin, win}, a);
}

extern "C" int pp_update_down_weight(pp_ctx* ctx, int level, const float* w, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_ARG, "pp_update_down_weight: no committed weights to update (pp_commit_weights first)");
    if (level != 2)
        return pp_fail(ctx, PP_E_ARG, "pp_update_down_weight: level 2 only (the strided convolution of block 3): level 0 carries the sparse "
                                      "first-conv packing, and nothing trains level 1 yet");
    if (!w || ((uintptr_t)w & 3)) return pp_fail(ctx, PP_E_ARG, "pp_update_down_weight: null or misaligned weight pointer");
    if (pp_effective_precision(ctx) != 0)
        return pp_fail(ctx, PP_E_ARG, "pp_update_down_weight: fp32 mode only (the committed plan packs the convolutions in a 16-bit format)");
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    int rc = pp_update_conv_image(ctx, 10, w, stream); // block 3's strided convolution: image 10
    if (rc) return rc;
    PP_HIP(hipGetLastError());
    return 0;
}
