// Mixed-precision training (gfx950): the 16-bit operand twin of down_train.hip's strided-stage backward, pp_down_backward_mp modes 1
// "bf16x3" and 2 "bf16".  The parity planes of x, the plane statistics, the norm backward and the padded dz plane are down_train.h's
// fp32 / fp64 kernels, so mean, rstd, the mask xhat > 0 and dz itself are the fp32 path's bits.  Only the two gradient products run on
// v_mfma_f32_16x16x32_bf16 (a lane's A / B fragment is 8 consecutive k of one row / column), with fp32 accumulation:
//   k_conv3_wt16    wT16[part][t][ci][co] = bf16 parts of w[co][ci][t]: the dgrad's A operand, 8 consecutive co per lane (train16.h)
//   k_down_wgrad16  dw[co][(ci, t)] = sum_{frame, P} dz[co][P] xp[ci][plane_t][P + off_t]   K = frames x PP in chunks of 32 positions
//   k_down_dgrad16  per output parity class: dx[ci][P] = sum_{t in class, co} wT16[t][ci][co] dz[co][P + off]   K in steps of 32 co,
//                   blocks of DA_BLOCK = 64 from zero
// No 16-bit image of the planes is kept: the fp32 planes of down_train.h are read and rounded (bf16) or split (bf16x3: hi = bf16(v),
// lo = bf16(fl32(v - hi)); a product is hi hi, hi lo, lo hi into one accumulator, in that order) in registers.  In the wgrad a lane's 8
// positions of dz are two aligned 16-byte loads (G and PS are multiples of 4, a chunk starts at a multiple of 32) and its 8 positions of
// a parity plane, shifted by -1 or -wp, are two 16-byte loads at 4-byte alignment: an odd shift costs nothing on fp32 planes, so no
// funnel shift.  In the dgrad the 8 k are 8 planes of dz at one position, eight 4-byte loads that 16 lanes make 64 contiguous bytes.
// So the workspace is pp_down_backward's plus the small wT16, the budgets and frame chunks are its own, and every shape the fp32 entry
// takes runs in the mode asked for (a frame past the 256 MB budget is refused by both).
//
// pp_down_backward_affine_mp / pp_down_backward_bn_mp are the same products behind the dz plane of the BatchNorm forms (k_affine_down_dz,
// k_bn_down_dz): mask, dz and the two fp64 sums are the fp32 path's bits in every mode.
//
// Determinism as in down_train.hip: no atomics, K ranges, segments and chunks are functions of the shapes alone.
#include <cmath>
#include "pp_common.h"
#include "train_planes.h"
#include "down_train.h"
#include "train16.h"

namespace {

struct __attribute__((packed, aligned(4))) f32x4u { float v[4]; }; // four floats at 4-byte alignment: one global_load_dwordx4

constexpr int DW16_WGS = 2048; // workgroups a 16-bit wgrad launch aims at: its short K steps need more waves per SIMD than fp32's DW_WGS

// ---- wgrad: k_conv3_wgrad's tiles (MA = 2: waves 2 x 2, 64 co x 32 NB columns; MA = 4: waves 1 x 4, 64 co x 64 NB columns).  K runs over
// 32-position chunks of the launch's frames (chunk c: frame c / cpf, positions 32 (c % cpf) ..); a lane's 8 k are positions 4 q .. 4 q + 3
// and 16 + 4 q .. 16 + 4 q + 3 of the chunk (the sum over K is order-free: with this assignment the four lane groups of a row read 64
// contiguous bytes per load where 8 q .. 8 q + 7 reads 16 of every 32, twice the cache lines per instruction).  dz: two aligned 16-byte
// loads.  x, shifted by -1 or -wp: two 16-byte loads at 4-byte alignment (f32x4u; global loads need dword alignment only), a quarter of
// the load instructions of the fp32 kernel's element-wise reads.  A group of four that starts at PP or beyond is taken as zero in both
// operands (a chunk may reach past the plane's trailing guard, which is shorter than 32); one that straddles PP meets guard zeros of dz.  blockIdx.z owns chunks [z cps, (z + 1) cps) and writes partial gbase + z in the state_dict layout [co][ci][3][3].
template <int NB, int MA, bool X3>
__global__ void __launch_bounds__(256) k_down_wgrad16(const float* __restrict__ dzp, const float* __restrict__ xp, float* __restrict__ part, int cin,
                                                      int cout, int wp, int G, int PP, int PS, int cpf, int nchunks, int cps, int gbase)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    static_assert(MA == 2 || MA == 4, "waves 2 x 2 or 1 x 4");
    constexpr int WC = MA;
    const int co0 = blockIdx.y * 64 + (MA == 2 ? 32 * (wave >> 1) : 0), n0 = blockIdx.x * (16 * NB * WC) + 16 * NB * (wave & (WC - 1));
    const int NC = 9 * cin;
    int boff[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int n = n0 + 16 * b + l16, ci = n / 9, t = n - 9 * ci, ky = t / 3, kx = t - 3 * ky;
        const int par = (ky != 1 ? 2 : 0) + (kx != 1 ? 1 : 0);
        boff[b] = (ci * 4 + par) * PS + G - (ky == 0 ? wp : 0) - (kx == 0 ? 1 : 0);
    }
    f32x4 acc[MA][NB];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c0 = blockIdx.z * cps, c1 = c0 + cps < nchunks ? c0 + cps : nchunks;
    // the fp32 values of one chunk: loaded one chunk ahead, so that the loads of chunk c + 1 are in flight behind the MFMAs of chunk c
    // (the 16-bit products are too short to hide a load behind themselves, and a launch has only a few waves per SIMD)
    float zr[MA][8], xr[NB][8];
    auto load_chunk = [&](int c) {
        const int f = c / cpf, pb = (c - f * cpf) * 32 + 4 * q;
        const float* zf = dzp + (size_t)f * cout * PS + G + pb;
        const float* xf = xp + (size_t)f * cin * 4 * PS + pb;
        const bool in0 = pb < PP, in1 = pb + 16 < PP; // a group of 4 that starts inside PP ends inside the trailing guard (G >= 20)
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            const float* r = zf + (size_t)(co0 + 16 * a + l16) * PS;
            const float4 u = in0 ? *reinterpret_cast<const float4*>(r) : make_float4(0.f, 0.f, 0.f, 0.f);
            const float4 v = in1 ? *reinterpret_cast<const float4*>(r + 16) : make_float4(0.f, 0.f, 0.f, 0.f);
            zr[a][0] = u.x; zr[a][1] = u.y; zr[a][2] = u.z; zr[a][3] = u.w; zr[a][4] = v.x; zr[a][5] = v.y; zr[a][6] = v.z; zr[a][7] = v.w;
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const f32x4u u = in0 ? *reinterpret_cast<const f32x4u*>(xf + boff[b]) : f32x4u{{0.f, 0.f, 0.f, 0.f}};
            const f32x4u v = in1 ? *reinterpret_cast<const f32x4u*>(xf + boff[b] + 16) : f32x4u{{0.f, 0.f, 0.f, 0.f}};
#pragma unroll
            for (int e = 0; e < 4; ++e) { xr[b][e] = u.v[e]; xr[b][4 + e] = v.v[e]; }
        }
    };
    if (c0 < c1) load_chunk(c0);
    for (int c = c0; c < c1; ++c) {
        u32x4 zh[MA], xh[NB], zl[X3 ? MA : 1], xl[X3 ? NB : 1];
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            zh[a] = pk8(zr[a]);
            if (X3) zl[a] = pk8_rest(zr[a]);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            xh[b] = pk8(xr[b]);
            if (X3) xl[b] = pk8_rest(xr[b]);
        }
        if (c + 1 < c1) load_chunk(c + 1);
#pragma unroll
        for (int a = 0; a < MA; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                acc[a][b] = mfma16(zh[a], xh[b], acc[a][b]);
                if (X3) {
                    acc[a][b] = mfma16(zh[a], xl[b], acc[a][b]);
                    acc[a][b] = mfma16(zl[a], xh[b], acc[a][b]);
                }
            }
    }
    float* pw = part + (size_t)(gbase + blockIdx.z) * cout * NC;
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) pw[(size_t)(co0 + 16 * a + 4 * q + i) * NC + n0 + 16 * b + l16] = acc[a][b][i];
}

// ---- dgrad: k_down_dgrad's tiling: grid (position tiles, 4 parity classes, frames), a workgroup covers ALL Cin channels (WM = Cin / 64
// waves down, 4 / WM across), each wave 64 ci x 32 half-resolution positions.  K = (t in class, co) in steps of 32 output channels (lane
// group q takes co + 8 q .. + 7); a block of DA_BLOCK = 64 k-terms is two steps, accumulated from zero, and the block sums are added in
// (t, co) order.  A = wT16[t][ci][co .. + 7], B = dz[co .. + 7][P + off].  Positions past PP read a clamped index and are never stored.
template <int WM, bool X3>
__global__ void __launch_bounds__(256) k_down_dgrad16(const uint16_t* __restrict__ wT, const float* __restrict__ dzp, float* __restrict__ dx, int cin,
                                                      int cout, int hin, int win, int wp, int G, int PP, int PS)
{
    constexpr int WN = 4 / WM;
    static_assert(DA_BLOCK % 32 == 0, "a block is whole k-steps");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int ci0 = 64 * (wave / WN), p0 = blockIdx.x * (32 * WN) + 32 * (wave % WN);
    const int py = blockIdx.y >> 1, px = blockIdx.y & 1;
    const float* zf = dzp + (size_t)blockIdx.z * cout * PS + G;
    float* dxf = dx + (size_t)blockIdx.z * cin * hin * win;
    const size_t wpart = (size_t)9 * cin * cout;
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
            const uint16_t* wt_t = wT + ((size_t)t * cin + ci0 + l16) * cout + 8 * q;
            for (int cb0 = 0; cb0 < cout; cb0 += DA_BLOCK) { // cout is a multiple of DA_BLOCK
                f32x4 acc[4][2];
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int cb = cb0; cb < cb0 + DA_BLOCK; cb += 32) {
                    u32x4 wh[4], zh[2], wl[X3 ? 4 : 1], zl[X3 ? 2 : 1];
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        wh[a] = *reinterpret_cast<const u32x4*>(wt_t + (size_t)16 * a * cout + cb);
                        if (X3) wl[a] = *reinterpret_cast<const u32x4*>(wt_t + (size_t)16 * a * cout + cb + wpart);
                    }
                    float v0[8], v1[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) {
                        const float* zr = zf + (size_t)(cb + 8 * q + e) * PS + off;
                        v0[e] = zr[i0]; v1[e] = zr[i1];
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

// the 16-bit products of down_run (down_train.h): K over 32-position chunks, the bf16 weight image of the dgrad
template <bool X3>
struct down_bf16 {
    static constexpr int KPOS = 32, WGS = DW16_WGS;
    static int grow_wt(pp_ctx* ctx, down_ws* ws, int nw) { return grow(ctx, &ws->wT16, &ws->wT16_elems, (size_t)(X3 ? 2 : 1) * nw); }
    static void pack_wt(const down_plan& p, down_ws* ws, const float* wgt, hipStream_t stream)
    {
        hipLaunchKernelGGL(k_conv3_wt16<X3>, dim3(pp_div_up(p.nw, 256)), dim3(256), 0, stream, wgt, ws->wT16, p.s.cin, p.s.cout);
    }
    static void wgrad(const down_plan& p, const dw_chunk& c, const float* dzp, const float* xp, float* part, hipStream_t stream)
    {
        const int cin = p.s.cin, cout = p.s.cout;
        const dim3 gd(p.NC / p.TN, cout / 64, c.sp);
        if (cin >= 128)
            hipLaunchKernelGGL((k_down_wgrad16<4, 2, X3>), gd, dim3(256), 0, stream, dzp, xp, part, cin, cout, p.g.wp, p.g.G, p.g.PP, p.g.PS, p.cpf,
                               c.nchunks, c.cps, c.gbase);
        else
            hipLaunchKernelGGL((k_down_wgrad16<3, 4, X3>), gd, dim3(256), 0, stream, dzp, xp, part, cin, cout, p.g.wp, p.g.G, p.g.PP, p.g.PS, p.cpf,
                               c.nchunks, c.cps, c.gbase);
    }
    static void dgrad(const down_plan& p, const down_ws* ws, const float* dzp, float* dx, int fn, hipStream_t stream)
    {
        const int cin = p.s.cin, cout = p.s.cout, PP = p.g.PP;
        if (cin == 64)
            hipLaunchKernelGGL((k_down_dgrad16<1, X3>), dim3(pp_div_up(PP, 128), 4, fn), dim3(256), 0, stream, ws->wT16, dzp, dx, cin, cout, p.s.hin,
                               p.s.win, p.g.wp, p.g.G, PP, p.g.PS);
        else
            hipLaunchKernelGGL((k_down_dgrad16<2, X3>), dim3(pp_div_up(PP, 64), 4, fn), dim3(256), 0, stream, ws->wT16, dzp, dx, cin, cout, p.s.hin,
                               p.s.win, p.g.wp, p.g.G, PP, p.g.PS);
    }
};

} // namespace

extern "C" int pp_down_backward_path(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win)
{
    if (!ctx) return -PP_E_ARG; // the modes are 0 .. 2, so an error is the negated code
    if (mode < 0 || mode > 2) return -pp_fail(ctx, PP_E_ARG, "pp_down_backward_path: mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)");
    if (int rc = down_check(ctx, "pp_down_backward_mp", DOWN_CHK_SHAPE, NORM_INSTANCE, down_shape{cin, cout, hin, win}, down_args())) return -rc;
    return mode; // the 16-bit kernels read the fp32 planes: every shape the fp32 entry takes runs in the mode asked for
}

extern "C" int pp_down_backward_mp(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win, const float* x, const float* wgt, const float* z,
                                   const float* dy, int nb, float* dw, float* dx, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, "pp_down_backward_mp: mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)");
    if (mode == 0) return pp_down_backward(ctx, cin, cout, hin, win, x, wgt, z, dy, nb, dw, dx, stream_);
    const down_shape s{cin, cout, hin, win};
    down_args a;
    a.x = x; a.wgt = wgt; a.z = z; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx; a.stream = (hipStream_t)stream_;
    int rc; // the shape first, then the tensors
    if ((rc = down_check(ctx, "pp_down_backward_mp", DOWN_CHK_SHAPE, NORM_INSTANCE, s, a)) ||
        (rc = down_check(ctx, "pp_down_backward_mp", DOWN_CHK_TENSORS, NORM_INSTANCE, s, a)))
        return rc;
    return mode == 1 ? down_run<down_bf16<true>>(ctx, NORM_INSTANCE, s, a) : down_run<down_bf16<false>>(ctx, NORM_INSTANCE, s, a);
}

namespace {

// One _affine_mp / _bn_mp call in mode 1 or 2: the shape first, then the tensors, under `form`'s rules; down_run<down_bf16<X3>> is the whole
// driver: the policies read the plan, the fp32 dz plane and the parity planes of x, whichever pass of the form wrote dz
int down_entry16(pp_ctx* ctx, const char* entry, norm_form form, int mode, const down_shape& s, const down_args& a)
{
    int rc;
    if ((rc = down_check(ctx, entry, DOWN_CHK_SHAPE, form, s, a)) || (rc = down_check(ctx, entry, DOWN_CHK_TENSORS, form, s, a))) return rc;
    return mode == 1 ? down_run<down_bf16<true>>(ctx, form, s, a) : down_run<down_bf16<false>>(ctx, form, s, a);
}

const char* const DOWN_MODE_MSG = ": mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)";

} // namespace

// The mode pp_down_backward_affine_mp and pp_down_backward_bn_mp run for this shape: `mode`, on a context of either norm kind
extern "C" int pp_down_backward_bn_path(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win)
{
    if (!ctx) return -PP_E_ARG;
    if (mode < 0 || mode > 2) return -pp_fail(ctx, PP_E_ARG, (std::string("pp_down_backward_bn_path") + DOWN_MODE_MSG).c_str());
    if (int rc = down_check(ctx, "pp_down_backward_bn_path", DOWN_CHK_SHAPE, NORM_AFFINE, down_shape{cin, cout, hin, win}, down_args())) return -rc;
    return mode;
}

// pp_down_backward_affine / pp_down_backward_bn with the two products in 16-bit operands.  k_affine_down_dz, k_bn_plane_sums, k_bn_coef and
// k_bn_down_dz are the fp32 path's own passes, so the mask, dz, dscale and dshift are its bits in every mode; mode 0 is the fp32 entry.
extern "C" int pp_down_backward_affine_mp(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win, const float* x, const float* wgt,
                                          const float* z, const float* scale, const float* shift, const float* dy, int nb, float* dw, float* dx,
                                          double* dscale, double* dshift, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, (std::string("pp_down_backward_affine_mp") + DOWN_MODE_MSG).c_str());
    if (mode == 0) return pp_down_backward_affine(ctx, cin, cout, hin, win, x, wgt, z, scale, shift, dy, nb, dw, dx, dscale, dshift, stream_);
    down_args a;
    a.x = x; a.wgt = wgt; a.z = z; a.scale = scale; a.shift = shift; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx;
    a.dscale = dscale; a.dshift = dshift; a.stream = (hipStream_t)stream_;
    return down_entry16(ctx, "pp_down_backward_affine_mp", NORM_AFFINE, mode, down_shape{cin, cout, hin, win}, a);
}

extern "C" int pp_down_backward_bn_mp(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win, const float* x, const float* wgt, const float* z,
                                      const float* scale, const float* shift, const float* mean, const float* var, const float* dy, int nb,
                                      float* dw, float* dx, double* dscale, double* dshift, int chunk_frames, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, (std::string("pp_down_backward_bn_mp") + DOWN_MODE_MSG).c_str());
    if (mode == 0)
        return pp_down_backward_bn(ctx, cin, cout, hin, win, x, wgt, z, scale, shift, mean, var, dy, nb, dw, dx, dscale, dshift, chunk_frames, stream_);
    down_args a;
    a.x = x; a.wgt = wgt; a.z = z; a.scale = scale; a.shift = shift; a.mean = mean; a.var = var; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx;
    a.dscale = dscale; a.dshift = dshift; a.chunk_frames = chunk_frames; a.stream = (hipStream_t)stream_;
    return down_entry16(ctx, "pp_down_backward_bn_mp", NORM_BATCH, mode, down_shape{cin, cout, hin, win}, a);
}
