// Mixed-precision training (gfx950): the 16-bit operand twin of neck_train.hip's upsampling-branch backward, pp_neck_backward_mp modes 1
// "bf16x3" and 2 "bf16".  The recomputed forward Z = w^T x, the statistics and dZ are neck_train.h's fp32 / fp64 kernels, so mean, rstd,
// the mask and dZ itself are the fp32 path's bits.  Only the two gradient products run on v_mfma_f32_16x16x32_bf16 (a lane's A / B
// fragment is 8 consecutive k of one row / column), with fp32 accumulation:
//   k_neck_w16    w16[part][ci][r] = bf16 parts of w[ci][r]: the dx product's A operand, 8 consecutive r per lane
//   k_neck_dw16   dw[ci][r] = sum_{frame, q} x[ci][q] dZ[r][q]   K = frames x p in chunks of 32 pixels; both operands are contiguous along K
//   k_neck_dx16   dx[ci][q] = sum_r w16[ci][r] dZ[r][q]          K = R in steps of 32 rows, blocks of DX_BLOCK = 64 from zero
// No 16-bit image of x or dZ is kept: both are read as fp32 from where the fp32 path keeps them and rounded (bf16) or split (bf16x3:
// hi = bf16(v), lo = bf16(fl32(v - hi)); a product is hi hi, hi lo, lo hi into one accumulator, in that order) in registers.  In the dw
// product a lane's 8 k are two 16-byte loads of a row of x and of dZ (pld is a multiple of 4 and a chunk starts at a multiple of 32);
// in the dx product they are 8 rows of dZ at one pixel, eight 4-byte loads that 16 lanes make 64 contiguous bytes each, as the fp32
// kernel's four.  So the workspace is pp_neck_backward's plus the small w16, frames per chunk are the same, and every shape the fp32
// entry takes runs in the mode asked for.
//
// Determinism as in neck_train.hip: no atomics, K ranges and chunks are functions of the shapes alone.
// pp_neck_backward_affine_mp / pp_neck_backward_bn_mp are the same products behind the dZ of the BatchNorm forms (k_affine_neck_dz,
// k_bn_neck_dz): mask, dZ and the two fp64 sums are the fp32 path's bits in every mode.
#include <cmath>
#include "pp_common.h"
#include "neck_train.h"
#include "train16.h"

namespace {

template <bool X3>
__global__ void __launch_bounds__(256) k_neck_w16(const float* __restrict__ w, uint16_t* __restrict__ w16, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = w[i];
    w16[i] = (uint16_t)pk_bf16(v, 0.f);
    if (X3) w16[(size_t)n + i] = (uint16_t)pk_bf16(bf16_rest(v), 0.f);
}

// floats i .. i + 3 and i + 16 .. i + 19 of a row whose length `len` and start `i` are multiples of 4 (two 16-byte loads), zero from
// `len` on
__device__ __forceinline__ void load8v(const float* __restrict__ row, int i, int len, float* v)
{
    const float4 a = i < len ? *reinterpret_cast<const float4*>(row + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 b = i + 16 < len ? *reinterpret_cast<const float4*>(row + i + 16) : make_float4(0.f, 0.f, 0.f, 0.f);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}

// ---- dw: workgroup tile 64 ci x 32 NB rows, four waves 2 x 2, each 32 ci x 16 NB rows (k_neck_dw's tile).  K runs over 32-pixel chunks
// of the launch's frames (chunk c: frame c / cpf, pixels 32 (c % cpf) ..); a lane's 8 k are pixels 4 q .. 4 q + 3 and 16 + 4 q .. 16 + 4 q + 3
// of the chunk (the sum over K is order-free; the four lane groups of a row then read 64 contiguous bytes per load).  blockIdx.z
// owns chunks [z cps, (z + 1) cps) and writes partial gbase + z.
template <int NB, bool X3>
__global__ void __launch_bounds__(256) k_neck_dw16(const float* __restrict__ x, const float* __restrict__ dZ, float* __restrict__ part, int Cin,
                                                   int R, int p, int pld, int cpf, int nchunks, int cps, int gbase, int xvec)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int ci0 = blockIdx.y * 64 + 32 * (wave >> 1), r0 = blockIdx.x * (32 * NB) + 16 * NB * (wave & 1);
    f32x4 acc[2][NB];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c0 = blockIdx.z * cps, c1 = c0 + cps < nchunks ? c0 + cps : nchunks;
    for (int c = c0; c < c1; ++c) {
        const int f = c / cpf, pb = (c - f * cpf) * 32 + 4 * q;
        const float* xf = x + (size_t)f * Cin * p;
        const float* zf = dZ + (size_t)f * R * pld;
        u32x4 xh[2], zh[NB], xl[X3 ? 2 : 1], zl[X3 ? NB : 1];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float* s_ = xf + (size_t)(ci0 + 16 * a + l16) * p;
            float v[8];
            if (xvec) {
                load8v(s_, pb, p, v);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int i = pb + (e & 3) + 4 * (e & 4);
                    v[e] = i < p ? s_[i] : 0.f;
                }
            }
            xh[a] = pk8(v);
            if (X3) xl[a] = pk8_rest(v);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            float v[8];
            load8v(zf + (size_t)(r0 + 16 * b + l16) * pld, pb, pld, v); // columns p .. pld - 1 are exact zeros
            zh[b] = pk8(v);
            if (X3) zl[b] = pk8_rest(v);
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                acc[a][b] = mfma16(xh[a], zh[b], acc[a][b]);
                if (X3) {
                    acc[a][b] = mfma16(xh[a], zl[b], acc[a][b]);
                    acc[a][b] = mfma16(xl[a], zh[b], acc[a][b]);
                }
            }
    }
    float* pw = part + (size_t)(gbase + blockIdx.z) * Cin * R;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) pw[(size_t)(ci0 + 16 * a + 4 * q + i) * R + r0 + 16 * b + l16] = acc[a][b][i];
}

// ---- dx: k_neck_dx's tiling: a workgroup covers ALL Cin channels (WM = Cin / 64 waves down, 4 / WM across), each wave 64 ci x 32
// pixels, so dZ is read once.  K = R in steps of 32 rows: lane group q takes rows 8 q .. 8 q + 7, one 16-byte load of w16 per ci row and
// eight loads of dZ per pixel.  A block of DX_BLOCK = 64 rows is two steps, accumulated from zero; the block sums are added in row order.
template <int WM, bool X3>
__global__ void __launch_bounds__(256) k_neck_dx16(const uint16_t* __restrict__ w16, const float* __restrict__ dZ, float* __restrict__ dx, int Cin,
                                                   int R, int p, int pld)
{
    constexpr int WN = 4 / WM;
    static_assert(DX_BLOCK % 32 == 0, "a block is whole k-steps");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int ci0 = 64 * (wave / WN), p0 = blockIdx.x * (32 * WN) + 32 * (wave % WN);
    const float* zf = dZ + (size_t)blockIdx.z * R * pld;
    float* dxf = dx + (size_t)blockIdx.z * Cin * p;
    const size_t wpart = (size_t)Cin * R;
    f32x4 tot[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) tot[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int px0 = p0 + l16, px1 = p0 + 16 + l16;
    for (int rb0 = 0; rb0 < R; rb0 += DX_BLOCK) { // R = Cup s s is a multiple of DX_BLOCK
        f32x4 acc[4][2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int rb = rb0; rb < rb0 + DX_BLOCK; rb += 32) {
            u32x4 wh[4], zh[2], wl[X3 ? 4 : 1], zl[X3 ? 2 : 1];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const uint16_t* wr = w16 + (size_t)(ci0 + 16 * a + l16) * R + rb + 8 * q;
                wh[a] = *reinterpret_cast<const u32x4*>(wr);
                if (X3) wl[a] = *reinterpret_cast<const u32x4*>(wr + wpart);
            }
            float v0[8], v1[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float* zr = zf + (size_t)(rb + 8 * q + e) * pld;
                v0[e] = px0 < p ? zr[px0] : 0.f;
                v1[e] = px1 < p ? zr[px1] : 0.f;
            }
            zh[0] = pk8(v0); zh[1] = pk8(v1);
            if (X3) { zl[0] = pk8_rest(v0); zl[1] = pk8_rest(v1); }
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 2; ++b) {
                    acc[a][b] = mfma16(wh[a], zh[b], acc[a][b]);
                    if (X3) {
                        acc[a][b] = mfma16(wh[a], zl[b], acc[a][b]);
                        acc[a][b] = mfma16(wl[a], zh[b], acc[a][b]);
                    }
                }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) tot[a][b] += acc[a][b];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const int px = p0 + 16 * b + l16;
            if (px < p)
#pragma unroll
                for (int i = 0; i < 4; ++i) dxf[(size_t)(ci0 + 16 * a + 4 * q + i) * p + px] = tot[a][b][i];
        }
}

// the 16-bit products of neck_run (neck_train.h): K over 32-pixel chunks, the bf16 image of w for the dx product
template <bool X3>
struct neck_bf16 {
    static constexpr int KPIX = 32;
    static int grow_wt(pp_ctx* ctx, neck_ws* ws, int nw) { return grow(ctx, &ws->w16, &ws->w16_elems, (size_t)(X3 ? 2 : 1) * nw); }
    static void pack_wt(const neck_plan& p, neck_ws* ws, const float* wt, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_neck_w16<X3>, dim3(pp_div_up(p.nw, 256)), dim3(256), 0, stream, wt, ws->w16, p.nw);
    }
    static void dw(const neck_plan& p, const dw_chunk& c, const float* xc, const float* dZ, float* part, int xvec, hipStream_t stream)
    {
        const geom& g = p.g;
        const dim3 gd(g.R / (32 * p.NBt), g.Cin / 64, c.sp);
        if (p.NBt == 4)
            hipLaunchKernelGGL((k_neck_dw16<4, X3>), gd, dim3(256), 0, stream, xc, dZ, part, g.Cin, g.R, g.p, g.pld, p.cpf, c.nchunks, c.cps, c.gbase, xvec);
        else
            hipLaunchKernelGGL((k_neck_dw16<2, X3>), gd, dim3(256), 0, stream, xc, dZ, part, g.Cin, g.R, g.p, g.pld, p.cpf, c.nchunks, c.cps, c.gbase, xvec);
    }
    static void dx(const neck_plan& p, const neck_ws* ws, const float*, const float* dZ, float* dxc, int fn, hipStream_t stream)
    {
        const geom& g = p.g;
        if (g.Cin == 64)
            hipLaunchKernelGGL((k_neck_dx16<1, X3>), dim3(pp_div_up(g.p, 128), 1, fn), dim3(256), 0, stream, ws->w16, dZ, dxc, g.Cin, g.R, g.p, g.pld);
        else if (g.Cin == 128)
            hipLaunchKernelGGL((k_neck_dx16<2, X3>), dim3(pp_div_up(g.p, 64), 1, fn), dim3(256), 0, stream, ws->w16, dZ, dxc, g.Cin, g.R, g.p, g.pld);
        else
            hipLaunchKernelGGL((k_neck_dx16<4, X3>), dim3(pp_div_up(g.p, 32), 1, fn), dim3(256), 0, stream, ws->w16, dZ, dxc, g.Cin, g.R, g.p, g.pld);
    }
};

} // namespace

extern "C" int pp_neck_backward_path(pp_ctx* ctx, int mode, int branch)
{
    if (!ctx) return -PP_E_ARG; // the modes are 0 .. 2, so an error is the negated code
    if (mode < 0 || mode > 2) return -pp_fail(ctx, PP_E_ARG, "pp_neck_backward_path: mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)");
    if (int rc = neck_check(ctx, "pp_neck_backward_mp", NECK_CHK_SHAPE, NORM_INSTANCE, branch, neck_args())) return -rc;
    return mode; // the 16-bit kernels keep no image of their own: every branch the fp32 entry takes runs in the mode asked for
}

extern "C" int pp_neck_backward_mp(pp_ctx* ctx, int mode, int branch, const float* x, const float* wt, const float* y, const float* dy, int nb,
                                   float* dw, float* dx, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, "pp_neck_backward_mp: mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)");
    if (mode == 0) return pp_neck_backward(ctx, branch, x, wt, y, dy, nb, dw, dx, stream_);
    neck_args a;
    a.x = x; a.wt = wt; a.y = y; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx; a.stream = (hipStream_t)stream_;
    int rc; // the branch and the context first, then the tensors
    if ((rc = neck_check(ctx, "pp_neck_backward_mp", NECK_CHK_SHAPE, NORM_INSTANCE, branch, a)) ||
        (rc = neck_check(ctx, "pp_neck_backward_mp", NECK_CHK_TENSORS, NORM_INSTANCE, branch, a)))
        return rc;
    return mode == 1 ? neck_run<neck_bf16<true>>(ctx, NORM_INSTANCE, branch, a) : neck_run<neck_bf16<false>>(ctx, NORM_INSTANCE, branch, a);
}

namespace {

// One _affine_mp / _bn_mp call in mode 1 or 2: the branch and the context first, then the tensors, under `form`'s rules;
// neck_run<neck_bf16<X3>> is the whole driver: the policies read the plan, x, w and the fp32 dZ, whichever pass of the form wrote it
int neck_entry16(pp_ctx* ctx, const char* entry, norm_form form, int mode, int branch, const neck_args& a)
{
    int rc;
    if ((rc = neck_check(ctx, entry, NECK_CHK_SHAPE, form, branch, a)) || (rc = neck_check(ctx, entry, NECK_CHK_TENSORS, form, branch, a))) return rc;
    return mode == 1 ? neck_run<neck_bf16<true>>(ctx, form, branch, a) : neck_run<neck_bf16<false>>(ctx, form, branch, a);
}

const char* const NECK_MODE_MSG = ": mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)";

} // namespace

// The mode pp_neck_backward_affine_mp and pp_neck_backward_bn_mp run for this branch: `mode`, on a context of either norm kind
extern "C" int pp_neck_backward_bn_path(pp_ctx* ctx, int mode, int branch)
{
    if (!ctx) return -PP_E_ARG;
    if (mode < 0 || mode > 2) return -pp_fail(ctx, PP_E_ARG, (std::string("pp_neck_backward_bn_path") + NECK_MODE_MSG).c_str());
    if (int rc = neck_check(ctx, "pp_neck_backward_bn_path", NECK_CHK_SHAPE, NORM_AFFINE, branch, neck_args())) return -rc;
    return mode;
}

// pp_neck_backward_affine / pp_neck_backward_bn with the dw and dx products in 16-bit operands.  Z, k_affine_neck_dz, k_bn_neck_sums,
// k_bn_coef and k_bn_neck_dz are the fp32 path's own passes, so the mask, dZ, dscale and dshift are its bits in every mode; mode 0 is the
// fp32 entry.
extern "C" int pp_neck_backward_affine_mp(pp_ctx* ctx, int mode, int branch, const float* x, const float* wt, const float* scale, const float* shift,
                                          const float* y, const float* dy, int nb, float* dw, float* dx, double* dscale, double* dshift,
                                          void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, (std::string("pp_neck_backward_affine_mp") + NECK_MODE_MSG).c_str());
    if (mode == 0) return pp_neck_backward_affine(ctx, branch, x, wt, scale, shift, y, dy, nb, dw, dx, dscale, dshift, stream_);
    neck_args a;
    a.x = x; a.wt = wt; a.scale = scale; a.shift = shift; a.y = y; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx;
    a.dscale = dscale; a.dshift = dshift; a.stream = (hipStream_t)stream_;
    return neck_entry16(ctx, "pp_neck_backward_affine_mp", NORM_AFFINE, mode, branch, a);
}

extern "C" int pp_neck_backward_bn_mp(pp_ctx* ctx, int mode, int branch, const float* x, const float* wt, const float* scale, const float* shift,
                                      const float* mean, const float* var, const float* y, const float* dy, int nb, float* dw, float* dx,
                                      double* dscale, double* dshift, int chunk_frames, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, (std::string("pp_neck_backward_bn_mp") + NECK_MODE_MSG).c_str());
    if (mode == 0) return pp_neck_backward_bn(ctx, branch, x, wt, scale, shift, mean, var, y, dy, nb, dw, dx, dscale, dshift, chunk_frames, stream_);
    neck_args a;
    a.x = x; a.wt = wt; a.scale = scale; a.shift = shift; a.mean = mean; a.var = var; a.y = y; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx;
    a.dscale = dscale; a.dshift = dshift; a.chunk_frames = chunk_frames; a.stream = (hipStream_t)stream_;
    return neck_entry16(ctx, "pp_neck_backward_bn_mp", NORM_BATCH, mode, branch, a);
}
