// Mixed-precision training (gfx950): the 16-bit operand twins of block_train.hip's Resnet unit backward, pp_unit_backward_mp modes 1
// "bf16x3" and 2 "bf16".  The two gradient products run on v_mfma_f32_16x16x32_bf16: a lane's A / B fragment is 8 consecutive k of one
// row / column.  Only the GEMM operand streams are bf16; statistics, mask, norm backward, the dw reduction and every input and output
// stay fp32.  bf16 (X3 = false) rounds every operand once (round to nearest even); bf16x3 (X3 = true) keeps x = hi + lo, hi = bf16(x),
// lo = bf16(fl32(x - hi)), as two images and issues hi hi, hi lo, lo hi into the same accumulator in that order.
//   k_conv3_wt16    wT16[part][t][ci][co] = bf16 parts of w[co][ci][t]: the dgrad's A operand, 8 consecutive co per lane (train16.h)
//   k_plane_stats   as in block_train.hip (train_planes.h)
//   k_unit_pack16   mean / rstd by plane_mean_rstd (train_planes.h) as in k_unit_pack; a and dz into padded bf16 planes, 8 positions per
//                   thread
//   k_affine_unit_pack16  the same planes for the BatchNorm forms: a by the affine, no statistics
//   k_unit_packT16  zT[P][co]: dz once more with the channel innermost, the dgrad's B operand
//   k_unit_wgrad16  dw[co][(ci, t)] = sum_{frame, P} dz[co][P] a[ci][P + off_t]      K = frames x PP16 in chunks of 32 positions
//   k_unit_dgrad16  da[ci][P] = sum_{t, co} wT16[t][ci][co] zT[P - off_t][co]        K = 9 C in steps of 32, blocks of DA_BLOCK = 64
//   k_plane_gstats_u, k_unit_norm_u  the norm backward with xhat re-evaluated from u (no fp32 image of a is kept)
//   k_dw_reduce     as in block_train.hip (train_host.h)
// Plane layout of the 16-bit images: as the fp32 one, with the row pitch wp16 = w + 2 rounded up to a multiple of 8 (the extra
// columns are halo zeros), G16 = wp16 + 40 and PS16 = 2 G16 + PP16 multiples of 8, so that a k-step of 8 positions starting at a
// multiple of 8 is one aligned 16-byte load in dz and stays aligned under a row shift (ky - 1) wp16 in a.  The column shift kx - 1 is
// an odd number of elements: the wgrad loads the aligned 16 bytes and the one dword before or behind them and funnel-shifts the five
// dwords by 16 bits in registers (v_alignbit_b32), so a is stored once.  The dgrad's B operand is 8 consecutive co at one position: zT,
// whose tap shift moves by whole rows of C elements.  Per frame that is 3 images of C PS16 bf16 (6 bytes per element against fp32's 8),
// twice that for bf16x3 (12), so a chunk of frames (<= 1 GB) holds fewer frames under bf16x3 than under fp32: at level 0 (64 channels,
// 400 x 400, 127 MB per frame) 8 where fp32 holds 12, so nb = 8 still runs as one chunk in every mode and a batch of 9 .. 12 frames
// splits under bf16x3 only.  That moves the K ranges of dw, not the bits of du.  A frame whose images exceed the 256 MB budget runs the
// fp32 kernels.
//
// The two BatchNorm forms (pp_unit_backward_affine_mp, pp_unit_backward_bn_mp) run the same products behind k_affine_unit_pack16, which has
// k_unit_pack16's grid and layout and no statistics: a = max(fma(u, scale, shift), 0) in fp32 by k_affine_unit_pack's expression, then
// rounded or split.  Behind the dgrad they run block_train.h's passes, which read u and du only: k_affine_unit_du<true> (the mask
// fma(u, scale, shift) > 0 re-evaluated from u: the fp32 path's mask bit for bit) and k_affine_reduce for the affine form; k_bn_plane_sums
// per chunk, then k_bn_coef and one in-place k_bn_unit_du over all frames for the batch form, whatever frames the 16-bit chunks held.
//
// Determinism as in block_train.hip: no atomics, K ranges, segments and chunks are functions of the shapes (and the mode) alone.
#include <cmath>
#include "pp_common.h"
#include "train_planes.h"
#include "block_train.h"
#include "train16.h"

namespace {

// ---- a and dz: grid (C, frames, SP), a thread takes groups of 8 positions (one row: wp and G are multiples of 8).  pack16_plane is the
// body of both pack kernels: act(u) is the form's a in fp32, rounded (bf16) or split (bf16x3) behind it, dz likewise; halo and guards are
// rewritten with zeros.  It keeps a walk of its own: a group of 8 tests its row once and its columns one by one, which padded_walk
// (train_planes.h, one element at a time) does not give without a second path.  a16, z16: [part][frame][C][PS]; pstride = the elements of
// one part ----------------------------------------------------------------------------------------------------------------------------------
template <bool X3, typename ACT>
__device__ __forceinline__ void pack16_plane(const float* __restrict__ up, const float* __restrict__ dp, uint16_t* __restrict__ a16,
                                             uint16_t* __restrict__ z16, size_t pl, int h, int w, int wp, int G, int PP, int PS, int LG, size_t pstride,
                                             ACT act)
{
    const int tid = threadIdx.x;
    const int ng = PS / 8, lo = blockIdx.z * LG, hi = lo + LG < ng ? lo + LG : ng;
    for (int g = lo + tid; g < hi; g += 256) {
        const int j = 8 * g, P = j - G;
        float av[8], dv[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) av[e] = dv[e] = 0.f;
        if (P >= 0 && P < PP) {
            const int y = P / wp, x0 = P - y * wp;
            if (y >= 1 && y <= h) {
                const int r = (y - 1) * w - 1;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int x = x0 + e;
                    if (x >= 1 && x <= w) {
                        av[e] = act(up[r + x]);
                        dv[e] = dp[r + x];
                    }
                }
            }
        }
        const size_t o = pl * PS + j;
        *reinterpret_cast<u32x4*>(a16 + o) = pk8(av);
        *reinterpret_cast<u32x4*>(z16 + o) = pk8(dv);
        if (X3) {
            *reinterpret_cast<u32x4*>(a16 + pstride + o) = pk8_rest(av);
            *reinterpret_cast<u32x4*>(z16 + pstride + o) = pk8_rest(dv);
        }
    }
}

// InstanceNorm: mean and rstd by plane_mean_rstd as in k_unit_pack, so the mask is fp32's
template <bool X3>
__global__ void __launch_bounds__(256) k_unit_pack16(const float* __restrict__ u, const float* __restrict__ dy, uint16_t* __restrict__ a16,
                                                     uint16_t* __restrict__ z16, float* __restrict__ stm, const double* __restrict__ pst, int C, int h,
                                                     int w, int wp, int G, int PP, int PS, int S, int LG, size_t pstride)
{
    const int N = h * w;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    float meanf, rstdf;
    plane_mean_rstd(pst, pl, S, N, meanf, rstdf);
    if (threadIdx.x == 0 && blockIdx.z == 0) { stm[pl * 2] = meanf; stm[pl * 2 + 1] = rstdf; }
    pack16_plane<X3>(u + pl * N, dy + pl * N, a16, z16, pl, h, w, wp, G, PP, PS, LG, pstride, [&](float v) {
        const float xhat = (v - meanf) * rstdf;
        return xhat > 0.f ? xhat : 0.f;
    });
}

// the two BatchNorm forms: a = max(fma(u, scale_c, shift_c), 0) by k_affine_unit_pack's expression, no statistics
template <bool X3>
__global__ void __launch_bounds__(256) k_affine_unit_pack16(const float* __restrict__ u, const float* __restrict__ dy, uint16_t* __restrict__ a16,
                                                            uint16_t* __restrict__ z16, const float* __restrict__ scale,
                                                            const float* __restrict__ shift, int C, int h, int w, int wp, int G, int PP, int PS,
                                                            int LG, size_t pstride)
{
    const int N = h * w;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float sc = scale[blockIdx.x], sh = shift[blockIdx.x];
    pack16_plane<X3>(u + pl * N, dy + pl * N, a16, z16, pl, h, w, wp, G, PP, PS, LG, pstride, [&](float v) { return affine_relu(v, sc, sh); });
}

// ---- zT[part][frame][PS][C]: grid (ceil(PS / 64), C / 64, frames), a 64 position x 64 channel tile through LDS ----------------------
template <bool X3>
__global__ void __launch_bounds__(256) k_unit_packT16(const float* __restrict__ dy, uint16_t* __restrict__ zT, int C, int h, int w, int wp, int G,
                                                      int PP, int PS, size_t pstride)
{
    __shared__ float tile[64][65];
    const int tid = threadIdx.x, N = h * w, c0 = blockIdx.y * 64;
    const float* df = dy + ((size_t)blockIdx.z * C + c0) * N;
    {
        const int p = tid & 63, P = blockIdx.x * 64 + p - G;
        int idx = -1;
        if (P >= 0 && P < PP) {
            const int y = P / wp, x = P - y * wp;
            if (y >= 1 && y <= h && x >= 1 && x <= w) idx = (y - 1) * w + x - 1;
        }
#pragma unroll 4
        for (int c = tid >> 6; c < 64; c += 4) tile[c][p] = idx >= 0 ? df[(size_t)c * N + idx] : 0.f;
    }
    __syncthreads();
    const int cg = tid & 7;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int p = (tid >> 3) + 32 * i, j = blockIdx.x * 64 + p;
        if (j >= PS) continue;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = tile[8 * cg + e][p];
        uint16_t* o = zT + ((size_t)blockIdx.z * PS + j) * C + c0 + 8 * cg;
        *reinterpret_cast<u32x4*>(o) = pk8(v);
        if (X3) *reinterpret_cast<u32x4*>(o + pstride) = pk8_rest(v);
    }
}

// ---- wgrad: workgroup tile (16 MA WR) co x (16 NB WC) columns n = ci 9 + t, four waves WR down x WC = 4 / WR across, a wave MA x NB
// MFMA tiles.  <4, 4, 2>: 128 x 128 (C >= 128); <3, 4, 1>: 64 x 192 (C = 64: 576 = 3 x 192 columns).  K runs over 32-position chunks of
// the launch's frames (chunk c: frame c / cpf, positions 32 (c % cpf) ..; positions past PP read guard zeros of dz); a lane takes
// positions 8 q .. 8 q + 7 of the chunk.  Column n reads a at the row shift (t / 3 - 1) wp as one aligned 16-byte load d, plus the dword
// e before (kx = 0) or behind (kx = 2) it; the fragment is the five dwords shifted by one element.  blockIdx.z owns chunks
// [z cps, (z + 1) cps) and writes partial gbase + z in the state_dict layout [co][ci][3][3] -------------------------------------------
template <int NB, int MA, int WR, bool X3>
__global__ void __launch_bounds__(256) k_unit_wgrad16(const uint16_t* __restrict__ z16, const uint16_t* __restrict__ a16, float* __restrict__ part,
                                                      int C, int wp, int G, int PS, int cpf, int nchunks, int cps, int gbase, size_t pstride)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    static_assert(WR == 1 || WR == 2, "waves 1 x 4 or 2 x 2");
    constexpr int WC = 4 / WR;
    const int co0 = blockIdx.y * (16 * MA * WR) + 16 * MA * (wave / WC), n0 = blockIdx.x * (16 * NB * WC) + 16 * NB * (wave % WC);
    const int NC = 9 * C;
    int boff[NB], eoff[NB], kxs[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int n = n0 + 16 * b + l16, ci = n / 9, t = n - 9 * ci;
        kxs[b] = t % 3;
        boff[b] = ci * PS + G + (t / 3 - 1) * wp; // < C PS <= 2^27: one frame's images fit the 256 MB budget
        eoff[b] = kxs[b] == 0 ? -2 : kxs[b] == 2 ? 8 : 0;
    }
    f32x4 acc[MA][NB];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c0 = blockIdx.z * cps, c1 = c0 + cps < nchunks ? c0 + cps : nchunks;
    for (int c = c0; c < c1; ++c) {
        const int f = c / cpf, pb = (c - f * cpf) * 32 + 8 * q;
        const uint16_t* zf = z16 + (size_t)f * C * PS + G + pb;
        const uint16_t* af = a16 + (size_t)f * C * PS + pb;
        u32x4 zh[MA], ah[NB], zl[X3 ? MA : 1], al[X3 ? NB : 1];
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            const uint16_t* r = zf + (size_t)(co0 + 16 * a + l16) * PS;
            zh[a] = *reinterpret_cast<const u32x4*>(r);
            if (X3) zl[a] = *reinterpret_cast<const u32x4*>(r + pstride);
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const uint16_t* r = af + boff[b];
            ah[b] = shift_frag(*reinterpret_cast<const u32x4*>(r), *reinterpret_cast<const unsigned*>(r + eoff[b]), kxs[b]);
            if (X3) al[b] = shift_frag(*reinterpret_cast<const u32x4*>(r + pstride), *reinterpret_cast<const unsigned*>(r + pstride + eoff[b]), kxs[b]);
        }
#pragma unroll
        for (int a = 0; a < MA; ++a)
#pragma unroll
            for (int b = 0; b < NB; ++b) {
                acc[a][b] = mfma16(zh[a], ah[b], acc[a][b]);
                if (X3) {
                    acc[a][b] = mfma16(zh[a], al[b], acc[a][b]);
                    acc[a][b] = mfma16(zl[a], ah[b], acc[a][b]);
                }
            }
    }
    float* pw = part + (size_t)(gbase + blockIdx.z) * C * NC;
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) pw[(size_t)(co0 + 16 * a + 4 * q + i) * NC + n0 + 16 * b + l16] = acc[a][b][i];
}

// ---- dgrad: a workgroup covers ALL C channels (WM = C / 64 waves down, 4 / WM across), each wave 64 ci x 64 positions (the weight is
// re-read once per 64 positions; at 32 it was most of the bytes a workgroup moves).  K = (t, co) in steps of 32 output channels (lane
// group q takes co + 8 q .. + 7); a block of DA_BLOCK = 64 k-terms is two steps, accumulated from zero, and the block sums are added in
// (t, co) order.  A = wT16[t][ci][co .. + 7], B = zT[P - off_t][co .. + 7].  Positions past PP read a clamped index and are never stored
template <int WM, bool X3>
__global__ void __launch_bounds__(256) k_unit_dgrad16(const uint16_t* __restrict__ wT, const uint16_t* __restrict__ zT, float* __restrict__ da, int C,
                                                      int h, int w, int wp, int G, int PP, int PS, size_t pstride)
{
    constexpr int WN = 4 / WM, NP = 4;
    static_assert(DA_BLOCK % 32 == 0, "a block is whole k-steps");
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int ci0 = 64 * (wave / WN), p0 = blockIdx.x * (16 * NP * WN) + 16 * NP * (wave % WN);
    const uint16_t* zf = zT + (size_t)blockIdx.z * PS * C + (size_t)G * C + 8 * q;
    const size_t wpart = (size_t)9 * C * C;
    float* daf = da + (size_t)blockIdx.z * C * h * w;
    f32x4 tot[4][NP];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < NP; ++b) tot[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    int ip[NP];
#pragma unroll
    for (int b = 0; b < NP; ++b) ip[b] = p0 + 16 * b + l16 < PP ? p0 + 16 * b + l16 : 0;
    for (int t = 0; t < 9; ++t) {
        const int off = (t / 3 - 1) * wp + (t % 3 - 1);
        const uint16_t* wt_t = wT + ((size_t)t * C + ci0 + l16) * C + 8 * q;
        const uint16_t* zp[NP];
#pragma unroll
        for (int b = 0; b < NP; ++b) zp[b] = zf + (ptrdiff_t)(ip[b] - off) * C;
        for (int cb0 = 0; cb0 < C; cb0 += DA_BLOCK) { // C is a multiple of DA_BLOCK
            f32x4 acc[4][NP];
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < NP; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int cb = cb0; cb < cb0 + DA_BLOCK; cb += 32) {
                u32x4 wh[4], zh[NP], wl[X3 ? 4 : 1], zl[X3 ? NP : 1];
#pragma unroll
                for (int b = 0; b < NP; ++b) {
                    zh[b] = *reinterpret_cast<const u32x4*>(zp[b] + cb);
                    if (X3) zl[b] = *reinterpret_cast<const u32x4*>(zp[b] + cb + pstride);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a) {
                    wh[a] = *reinterpret_cast<const u32x4*>(wt_t + (size_t)16 * a * C + cb);
                    if (X3) wl[a] = *reinterpret_cast<const u32x4*>(wt_t + (size_t)16 * a * C + cb + wpart);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < NP; ++b) {
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
                for (int b = 0; b < NP; ++b) tot[a][b] += acc[a][b];
        }
    }
#pragma unroll
    for (int b = 0; b < NP; ++b) {
        const int P = p0 + 16 * b + l16;
        if (P >= PP) continue;
        const int y = P / wp, x = P - y * wp;
        if (y < 1 || y > h || x < 1 || x > w) continue;
        float* o = daf + (size_t)(y - 1) * w + x - 1;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[(size_t)(ci0 + 16 * a + 4 * q + i) * h * w] = tot[a][b][i];
    }
}

// ---- norm backward without an fp32 image of a: xhat by k_unit_pack's expression from u and the stored mean / rstd; xhat > 0 is the
// mask a > 0 and, where it holds, xhat is a.  Same segments, same order of the sums as k_plane_gstats / k_unit_norm ---------------------
__global__ void __launch_bounds__(256) k_plane_gstats_u(const float* __restrict__ u, const float* __restrict__ stm, const float* __restrict__ du,
                                                        double* __restrict__ pst, int C, int N, int L, int S)
{
    __shared__ double red[256][2];
    const int tid = threadIdx.x;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float* up = u + pl * N;
    const float* dp = du + pl * N;
    const float meanf = stm[pl * 2], rstdf = stm[pl * 2 + 1];
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    double sg = 0.0, sgx = 0.0;
    strided4(lo, hi, [&](int i) { return float2{up[i], dp[i]}; },
             [&](float2 v) {
                 const float xhat = (v.x - meanf) * rstdf;
                 if (xhat > 0.f) {
                     const double g = (double)v.y;
                     sg += g; sgx += g * (double)xhat;
                 }
             });
    block_sum2(sg, sgx, red);
    if (tid == 0) { pst[(pl * S + blockIdx.z) * 2] = sg; pst[(pl * S + blockIdx.z) * 2 + 1] = sgx; }
}

__global__ void __launch_bounds__(256) k_unit_norm_u(const float* __restrict__ u, const float* __restrict__ stm, const double* __restrict__ pst,
                                                     const float* __restrict__ dskip, float* __restrict__ du, int C, int N, int L, int S)
{
    const int tid = threadIdx.x;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float* up = u + pl * N;
    float* dp = du + pl * N;
    const float meanf = stm[pl * 2], rstdf = stm[pl * 2 + 1];
    double sg = 0.0, sgx = 0.0;
    for (int g = 0; g < S; ++g) { sg += pst[(pl * S + g) * 2]; sgx += pst[(pl * S + g) * 2 + 1]; }
    const double inv_n = 1.0 / (double)N;
    const float c1 = (float)(sg * inv_n), c2 = (float)(sgx * inv_n);
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    for (int i = lo + tid; i < hi; i += 256) {
        const float xhat = (up[i] - meanf) * rstdf;
        const float g = xhat > 0.f ? dp[i] : 0.f;
        float v = rstdf * ((g - c1) - xhat * c2);
        if (dskip) v = v + dskip[pl * N + i];
        dp[i] = v;
    }
}


// geometry of the 16-bit planes: rows of wp (a multiple of 8) elements, guards of wp + 40
inline pad_geom planes16(int h, int w)
{
    const int64_t wp = ((int64_t)w + 2 + 7) & ~(int64_t)7, PP = ((int64_t)h + 2) * wp, G = wp + 40, PS = 2 * G + PP;
    return pad_geom{(int)wp, (int)PP, (int)G, (int)PS, (uint64_t)PS};
}
// bytes of one frame's 16-bit images: a, dz and zT, each of `parts` bf16 images
inline uint64_t frame16_bytes(int parts, int C, const pad_geom& g) { return (uint64_t)3 * parts * C * g.elems * sizeof(uint16_t); }

// The twin's driver for the three norm forms: the check, the plan, the chunk walk, the reduce and the passes behind the dgrad of the two
// BatchNorm forms are the family's; the packs, the InstanceNorm kernels and the images are its own.  The forms differ as in unit_run:
// InstanceNorm runs the statistics and k_unit_pack16 ahead of the products and its two norm passes behind the dgrad; the affine form
// k_affine_unit_pack16 and k_affine_unit_du<true> per chunk, k_affine_reduce behind the chunks; the batch form the affine pack and
// k_bn_plane_sums per chunk (raw da -> du), and behind the chunks k_bn_coef and one in-place k_bn_unit_du over all frames.  Those passes
// read u and du alone, so the batch form does not care that a 16-bit chunk holds other frames than an fp32 one.
template <bool X3>
int unit_backward16(pp_ctx* ctx, norm_form form, const unit_shape& s, const unit_args& a)
{
    const int C = s.C, h = s.h, w = s.w, nb = a.nb, parts = X3 ? 2 : 1;
    hipStream_t stream = a.stream;
    const pad_geom g = planes16(h, w);
    const int wp = g.wp, PP = g.PP, G = g.G, PS = g.PS;
    PP_HIP(hipSetDevice(ctx->device));
    block_ws* ws = workspace(ctx);
    // a wgrad tile: k_unit_wgrad16<4, 4, 2> (128 x 128) or <3, 4, 1> (64 x 192)
    const unit_plan p = unit_make_plan(ctx, s, nb, a.chunk_frames, g, frame16_bytes(parts, C, g), 32, C >= 128 ? 128 : 64);
    const int N = p.N, fc = p.fc, S = p.S, L = p.L, SP = p.SP, LG = (PS / 8 + SP - 1) / SP;
    const size_t pstride = (size_t)fc * p.pf_elems; // one part of one image over the chunk's frames
    // stm, pst: unit_run's rules for the forms
    const size_t stm_elems = form == NORM_INSTANCE ? (size_t)fc * C * 2 : (size_t)C * 4;
    const size_t pst_elems = (size_t)(form == NORM_INSTANCE ? fc : nb) * C * SEG_MAX * 2;
    int rc;
    if ((rc = grow(ctx, &ws->img16, &ws->img16_elems, 3 * parts * pstride)) ||
        (form != NORM_AFFINE && (rc = grow(ctx, &ws->stm, &ws->stm_elems, stm_elems))) ||
        (rc = grow(ctx, &ws->pst, &ws->pst_elems, pst_elems)) ||
        (rc = grow(ctx, &ws->part, &ws->part_elems, (size_t)p.Gp * p.nw)) ||
        (a.du && (rc = grow(ctx, &ws->wT16, &ws->wT16_elems, (size_t)parts * p.nw))))
        return rc;
    uint16_t* a16 = ws->img16;                       // [part][fc][C][PS]
    uint16_t* z16 = a16 + parts * pstride;           // [part][fc][C][PS]
    uint16_t* zT = z16 + parts * pstride;            // [part][fc][PS][C]
    if (a.du) hipLaunchKernelGGL(k_conv3_wt16<X3>, dim3(pp_div_up(p.nw, 256)), dim3(256), 0, stream, a.wgt, ws->wT16, C, C);
    for_chunks(p.walk, [&](const dw_chunk& c) {
        const int fn = c.fn;
        const size_t o = (size_t)c.f0 * C * N;
        if (form == NORM_INSTANCE) {
            hipLaunchKernelGGL(k_plane_stats, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, ws->pst, C, N, L, S);
            hipLaunchKernelGGL(k_unit_pack16<X3>, dim3(C, fn, SP), dim3(256), 0, stream, a.u + o, a.dy + o, a16, z16, ws->stm, ws->pst, C, h, w, wp, G,
                               PP, PS, S, LG, pstride);
        } else {
            hipLaunchKernelGGL(k_affine_unit_pack16<X3>, dim3(C, fn, SP), dim3(256), 0, stream, a.u + o, a.dy + o, a16, z16, a.scale, a.shift, C, h, w,
                               wp, G, PP, PS, LG, pstride);
        }
        const dim3 gd(p.NC / p.TN, C / (C >= 128 ? 128 : 64), c.sp);
        if (C >= 128)
            hipLaunchKernelGGL((k_unit_wgrad16<4, 4, 2, X3>), gd, dim3(256), 0, stream, z16, a16, ws->part, C, wp, G, PS, p.cpf, c.nchunks, c.cps, c.gbase,
                               pstride);
        else
            hipLaunchKernelGGL((k_unit_wgrad16<3, 4, 1, X3>), gd, dim3(256), 0, stream, z16, a16, ws->part, C, wp, G, PS, p.cpf, c.nchunks, c.cps, c.gbase,
                               pstride);
        if (!a.du) return;
        float* duc = a.du + o;
        hipLaunchKernelGGL(k_unit_packT16<X3>, dim3(pp_div_up(PS, 64), C / 64, fn), dim3(256), 0, stream, a.dy + o, zT, C, h, w, wp, G, PP, PS, pstride);
        if (C == 64)
            hipLaunchKernelGGL((k_unit_dgrad16<1, X3>), dim3(pp_div_up(PP, 256), 1, fn), dim3(256), 0, stream, ws->wT16, zT, duc, C, h, w, wp, G, PP, PS, pstride);
        else if (C == 128)
            hipLaunchKernelGGL((k_unit_dgrad16<2, X3>), dim3(pp_div_up(PP, 128), 1, fn), dim3(256), 0, stream, ws->wT16, zT, duc, C, h, w, wp, G, PP, PS, pstride);
        else
            hipLaunchKernelGGL((k_unit_dgrad16<4, X3>), dim3(pp_div_up(PP, 64), 1, fn), dim3(256), 0, stream, ws->wT16, zT, duc, C, h, w, wp, G, PP, PS, pstride);
        if (form == NORM_INSTANCE) {
            hipLaunchKernelGGL(k_plane_gstats_u, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, ws->stm, duc, ws->pst, C, N, L, S);
            hipLaunchKernelGGL(k_unit_norm_u, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, ws->stm, ws->pst, a.dskip ? a.dskip + o : nullptr, duc, C, N, L,
                               S);
        } else if (form == NORM_AFFINE) {
            hipLaunchKernelGGL(k_affine_unit_du<true>, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, (const float*)nullptr, a.scale, a.shift,
                               a.dskip ? a.dskip + o : nullptr, duc, ws->pst + (size_t)c.f0 * C * S * 2, C, w, 0, 0, 0, N, L, S);
        } else {
            hipLaunchKernelGGL(k_bn_plane_sums, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, duc, a.scale, a.shift, ws->pst + (size_t)c.f0 * C * S * 2,
                               C, N, L, S);
        }
    });
    launch_dw_reduce(ws->part, p.Gp, p.nw, a.dw, stream);
    if (form == NORM_AFFINE && a.dscale)
        hipLaunchKernelGGL(k_affine_reduce, dim3(pp_div_up(C, 64)), dim3(64), 0, stream, ws->pst, nb, C, S, a.dscale, a.dshift);
    if (form == NORM_BATCH && a.du) {
        hipLaunchKernelGGL(k_bn_coef, dim3(pp_div_up(C, 64)), dim3(64), 0, stream, ws->pst, nb, C, S, a.mean, a.var, (double)nb * (double)N, ws->stm,
                           a.dscale, a.dshift);
        hipLaunchKernelGGL(k_bn_unit_du, dim3(C, nb, S), dim3(256), 0, stream, a.u, a.scale, a.shift, ws->stm, a.dskip, a.du, C, N, L);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

// the mode pp_unit_backward_mp runs for a valid shape: the 16-bit tiling takes every C and map whose images fit the frame budget
int unit_path(int mode, int C, int h, int w)
{
    if (mode == 0) return 0;
    return frame16_bytes(mode == 1 ? 2 : 1, C, planes16(h, w)) <= WS_BUDGET ? mode : 0;
}

const char* const MODE_MSG = ": mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)";

// One _affine_mp / _bn_mp call in mode 1 or 2: the shape first (it decides the path); a shape no 16-bit tiling takes returns -1 and the
// caller runs its fp32 sibling; then the tensors, then the twin
int unit_entry16(pp_ctx* ctx, const char* entry, norm_form form, int mode, const unit_shape& s, const unit_args& a)
{
    if (int rc = unit_check(ctx, entry, UNIT_CHK_SHAPE, form, s, a)) return rc;
    const int path = unit_path(mode, s.C, s.h, s.w);
    if (path == 0) return -1;
    if (int rc = unit_check(ctx, entry, UNIT_CHK_TENSORS, form, s, a)) return rc;
    return path == 1 ? unit_backward16<true>(ctx, form, s, a) : unit_backward16<false>(ctx, form, s, a);
}

} // namespace

extern "C" int pp_unit_backward_path(pp_ctx* ctx, int mode, int C, int h, int w)
{
    if (!ctx) return -PP_E_ARG; // the modes are 0 .. 2, so an error is the negated code
    if (mode < 0 || mode > 2) return -pp_fail(ctx, PP_E_ARG, "pp_unit_backward_path: mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)");
    if (int rc = unit_check(ctx, "pp_unit_backward", UNIT_CHK_SHAPE, NORM_INSTANCE, unit_shape{C, h, w}, unit_args())) return -rc;
    return unit_path(mode, C, h, w);
}

// the same answer for pp_unit_backward_affine_mp and pp_unit_backward_bn_mp (the path depends on shape and mode, not on the form), on a
// context of either norm kind
extern "C" int pp_unit_backward_bn_path(pp_ctx* ctx, int mode, int C, int h, int w)
{
    if (!ctx) return -PP_E_ARG;
    if (mode < 0 || mode > 2) return -pp_fail(ctx, PP_E_ARG, (std::string("pp_unit_backward_bn_path") + MODE_MSG).c_str());
    if (int rc = unit_check(ctx, "pp_unit_backward_bn_path", UNIT_CHK_SHAPE, NORM_AFFINE, unit_shape{C, h, w}, unit_args())) return -rc;
    return unit_path(mode, C, h, w);
}

extern "C" int pp_unit_backward_mp(pp_ctx* ctx, int mode, int C, int h, int w, const float* u, const float* wgt, const float* dy, const float* dskip,
                                   int nb, float* dw, float* du, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, "pp_unit_backward_mp: mode must be 0 (fp32), 1 (bf16x3) or 2 (bf16)");
    const unit_shape s{C, h, w};
    unit_args a;
    a.u = u; a.wgt = wgt; a.dy = dy; a.dskip = dskip; a.nb = nb; a.dw = dw; a.du = du; a.stream = (hipStream_t)stream_;
    // the shape first, under pp_unit_backward's name: it decides the path, and the fp32 path is that entry
    if (int rc = unit_check(ctx, "pp_unit_backward", UNIT_CHK_SHAPE, NORM_INSTANCE, s, a)) return rc;
    const int path = unit_path(mode, C, h, w);
    if (path == 0) return pp_unit_backward(ctx, C, h, w, u, wgt, dy, dskip, nb, dw, du, stream_);
    if (int rc = unit_check(ctx, "pp_unit_backward", UNIT_CHK_TENSORS, NORM_INSTANCE, s, a)) return rc;
    return path == 1 ? unit_backward16<true>(ctx, NORM_INSTANCE, s, a) : unit_backward16<false>(ctx, NORM_INSTANCE, s, a);
}

// pp_unit_backward_affine with the two products in 16-bit operands: mode 0, and a shape whose images exceed the budget, is that entry
extern "C" int pp_unit_backward_affine_mp(pp_ctx* ctx, int mode, int C, int h, int w, const float* u, const float* wgt, const float* scale,
                                          const float* shift, const float* dy, const float* dskip, int nb, float* dw, float* du, double* dscale,
                                          double* dshift, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, (std::string("pp_unit_backward_affine_mp") + MODE_MSG).c_str());
    if (mode) {
        unit_args a;
        a.u = u; a.wgt = wgt; a.scale = scale; a.shift = shift; a.dy = dy; a.dskip = dskip; a.nb = nb; a.dw = dw; a.du = du;
        a.dscale = dscale; a.dshift = dshift; a.stream = (hipStream_t)stream_;
        const int rc = unit_entry16(ctx, "pp_unit_backward_affine_mp", NORM_AFFINE, mode, unit_shape{C, h, w}, a);
        if (rc >= 0) return rc;
    }
    return pp_unit_backward_affine(ctx, C, h, w, u, wgt, scale, shift, dy, dskip, nb, dw, du, dscale, dshift, stream_);
}

// pp_unit_backward_bn likewise.  The two phases are that entry's; chunk_frames caps the frames of a chunk of 16-bit images
extern "C" int pp_unit_backward_bn_mp(pp_ctx* ctx, int mode, int C, int h, int w, const float* u, const float* wgt, const float* scale,
                                      const float* shift, const float* mean, const float* var, const float* dy, const float* dskip, int nb,
                                      float* dw, float* du, double* dscale, double* dshift, int chunk_frames, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (mode < 0 || mode > 2) return pp_fail(ctx, PP_E_ARG, (std::string("pp_unit_backward_bn_mp") + MODE_MSG).c_str());
    if (mode) {
        unit_args a;
        a.u = u; a.wgt = wgt; a.scale = scale; a.shift = shift; a.mean = mean; a.var = var; a.dy = dy; a.dskip = dskip; a.nb = nb; a.dw = dw;
        a.du = du; a.dscale = dscale; a.dshift = dshift; a.chunk_frames = chunk_frames; a.stream = (hipStream_t)stream_;
        const int rc = unit_entry16(ctx, "pp_unit_backward_bn_mp", NORM_BATCH, mode, unit_shape{C, h, w}, a);
        if (rc >= 0) return rc;
    }
    return pp_unit_backward_bn(ctx, C, h, w, u, wgt, scale, shift, mean, var, dy, dskip, nb, dw, du, dscale, dshift, chunk_frames, stream_);
}
