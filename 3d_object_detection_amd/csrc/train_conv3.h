// What the backwards of the Resnet unit (block_train.hip: stride 1, C -> C) and of the strided stage (down_train.hip: stride 2, Cin ->
// Cout, x in its four parity planes) share as 3 x 3 convolutions over the zero-haloed padded plane (padded_plane, train_host.h), beside
// the streaming helpers of train_planes.h: the two fp32 gradient products (the dgrad's weight transpose, the wgrad kernel, the blocked
// K sum of one dgrad tap) and the sums of the train-mode BatchNorm backward.  What differs between the two strides is how a column
// (ci, t) of the wgrad finds its operand (taps_s1, taps_s2), which taps a dgrad position visits and where it is stored: the two dgrad
// kernels keep their own tap loops and stores.  One copy, so that a change to a product is made once and a shape keeps its bits in both
// families.  The 16-bit twins read other operands and keep products of their own (block_train16.hip, down_train16.hip); of this header
// they use DA_BLOCK and k_bn_plane_sums.
#pragma once
#include "pp_common.h"
#include "train_host.h" // f32x4
#include "train_planes.h"

namespace {

constexpr int DA_BLOCK = 64; // k-terms that a dgrad sums in one accumulator before adding the block to the total

// wT[t][co][ci] = w[co][ci][t]: the dgrad's A operand, contiguous along its rows
__global__ void __launch_bounds__(256) k_conv3_wt(const float* __restrict__ w, float* __restrict__ wT, int cin, int cout)
{
    const int i = blockIdx.x * 256 + threadIdx.x; // index into wT [9][cout][cin]
    if (i >= 9 * cin * cout) return;
    const int ci = i % cin, co = (i / cin) % cout, t = i / (cin * cout);
    wT[i] = w[((size_t)co * cin + ci) * 9 + t];
}

// ---- sums of the train-mode BatchNorm backward of the unit (v = u, g = the raw da) and the stage (v = z, g = dy): grid (C, frames, S)
// over the tight [C][N] planes, gm = g [fma(v, scale, shift) > 0], the forward prologue's mask; the segment's sum gm v, sum gm in fp64 ->
// pst[frame][c][segment][2].  A streaming pass like train_planes.h's, but kept out of that header: neck_train.hip includes it too, and a
// kernel that is no template is compiled into every translation unit that sees it ---------------------------------------------------------
__global__ void __launch_bounds__(256) k_bn_plane_sums(const float* __restrict__ v, const float* __restrict__ g, const float* __restrict__ scale,
                                                       const float* __restrict__ shift, double* __restrict__ pst, int C, int N, int L, int S)
{
    __shared__ double red[256][2];
    const int tid = threadIdx.x;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float* vp = v + pl * N;
    const float* gp = g + pl * N;
    const float sc = scale[blockIdx.x], sh = shift[blockIdx.x];
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    double sgv = 0.0, sg = 0.0;
    strided4(lo, hi, [&](int i) { return float2{vp[i], gp[i]}; },
             [&](float2 e) {
                 if (fmaf(e.x, sc, sh) > 0.f) {
                     const double gm = (double)e.y;
                     sgv += gm * (double)e.x; sg += gm;
                 }
             });
    block_sum2(sgv, sg, red);
    if (tid == 0) { pst[(pl * S + blockIdx.z) * 2] = sgv; pst[(pl * S + blockIdx.z) * 2 + 1] = sg; }
}

// ---- the wgrad's B operand: PLANES padded planes per input channel, and the offset of column (ci, t) in one frame's planes, the tap
// shift included.  Stride 1: tap t = (ky, kx) is the channel's one plane shifted by (ky - 1) wp + (kx - 1).  Stride 2: it is parity
// plane (ky != 1, kx != 1) shifted by -(ky == 0) wp - (kx == 0) ----------------------------------------------------------------------
struct taps_s1 {
    static constexpr int PLANES = 1;
    static __device__ __forceinline__ int offset(int ci, int t, int wp, int G, int PS) { return ci * PS + G + (t / 3 - 1) * wp + (t % 3 - 1); }
};
struct taps_s2 {
    static constexpr int PLANES = 4;
    static __device__ __forceinline__ int offset(int ci, int t, int wp, int G, int PS)
    {
        const int ky = t / 3, kx = t - 3 * ky;
        const int par = (ky != 1 ? 2 : 0) + (kx != 1 ? 1 : 0);
        return (ci * 4 + par) * PS + G - (ky == 0 ? wp : 0) - (kx == 0 ? 1 : 0);
    }
};

// ---- wgrad: dw[co][(ci, t)] = sum_{frame, P} dz[co][P] x[(ci, t)][P].  Workgroup tile 64 co x columns n = ci 9 + t, a wave MA 16-row
// blocks of co x 16 NB columns.  MA = 2: four waves 2 x 2, tile 64 x 32 NB (cin >= 128: 128 columns).  MA = 4: four waves side by side,
// every one all 64 co, tile 64 x 64 NB (cin = 64: 576 = 3 x 192 columns; a wave loads 4 dz rows and 12 x columns for 48 MFMAs where the
// 2 x 2 form loads 2 and 8 for 16).  K runs over 16-position chunks of the launch's frames (chunk c: frame c / cpf, positions
// 16 (c % cpf) ..; positions past PP read guard zeros of dz); a lane takes positions 4 q .. 4 q + 3 of the chunk as its four k-steps:
// one 16-byte load per dz row, four shifted loads per x column.  blockIdx.z owns chunks [z cps, (z + 1) cps) and writes partial
// gbase + z, already in the state_dict layout [co][ci][3][3].
template <int NB, int MA, typename TAPS>
__global__ void __launch_bounds__(256) k_conv3_wgrad(const float* __restrict__ dzp, const float* __restrict__ xp, float* __restrict__ part, int cin,
                                                     int cout, int wp, int G, int PS, int cpf, int nchunks, int cps, int gbase)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    static_assert(MA == 2 || MA == 4, "waves 2 x 2 or 1 x 4");
    constexpr int WC = MA;     // waves across the tile: 2 of 2 x 2, 4 of 1 x 4
    const int co0 = blockIdx.y * 64 + (MA == 2 ? 32 * (wave >> 1) : 0), n0 = blockIdx.x * (16 * NB * WC) + 16 * NB * (wave & (WC - 1));
    const int NC = 9 * cin;
    int boff[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const int n = n0 + 16 * b + l16, ci = n / 9, t = n - 9 * ci;
        boff[b] = TAPS::offset(ci, t, wp, G, PS);
    }
    f32x4 acc[MA][NB];
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int c0 = blockIdx.z * cps, c1 = c0 + cps < nchunks ? c0 + cps : nchunks;
    // one frame's planes of dz and of x, elements: at most 2^26 (a frame's planes fit the 256 MB budget of both families), so the strides
    // are formed once in 32 bits and the K loop pays one 32 x 32 -> 64 bit product each; 64-bit products of cin and cout taken apart cost
    // the stride-1 loop 7 scalar instructions and 0.6 % over the kernel that had a single C
    const int zfs = cout * PS, xfs = cin * TAPS::PLANES * PS;
    for (int c = c0; c < c1; ++c) {
        const int f = c / cpf, pb = (c - f * cpf) * 16 + 4 * q;
        const float* zf = dzp + (size_t)f * zfs + G + pb;
        const float* xf = xp + (size_t)f * xfs + pb;
        float za[MA][4], xb[NB][4];
#pragma unroll
        for (int a = 0; a < MA; ++a) {
            const float4 v = *reinterpret_cast<const float4*>(zf + (size_t)(co0 + 16 * a + l16) * PS);
            za[a][0] = v.x; za[a][1] = v.y; za[a][2] = v.z; za[a][3] = v.w;
        }
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int s = 0; s < 4; ++s) xb[b][s] = xf[boff[b] + s];
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int a = 0; a < MA; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(za[a][s], xb[b][s], acc[a][b], 0, 0, 0);
    }
    float* pw = part + (size_t)(gbase + blockIdx.z) * cout * NC;
#pragma unroll
    for (int a = 0; a < MA; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) pw[(size_t)(co0 + 16 * a + 4 * q + i) * NC + n0 + 16 * b + l16] = acc[a][b][i];
}

// ---- one tap of a dgrad: tot[a][b] += sum_co wT[t][co][ci] dz[co][position b], a wave's 64 ci (four 16-row blocks a) x 32 positions
// (b = 0, 1).  K = co in steps of 4 output channels (lane group q takes co + q).  The sum is blocked: each DA_BLOCK terms accumulate from
// zero and the block sums are then added to tot in co order, so the rounding error grows with the block length and the block count, not
// with K; this order fixes the bits of the dgrad.  wt_t: the tap's weight slice at the lane's first row (wT + t cout cin + ci0 + l16);
// zf: the frame's dz at position 0, shift: the tap's signed shift of it; i0, i1: the lane's two positions, clamped inside the plane.
__device__ __forceinline__ void conv3_dgrad_tap(f32x4 (&tot)[4][2], const float* __restrict__ wt_t, const float* __restrict__ zf, int shift, int i0,
                                                int i1, int q, int cin, int cout, int PS)
{
    for (int cb0 = 0; cb0 < cout; cb0 += DA_BLOCK) { // cout is a multiple of DA_BLOCK
        f32x4 acc[4][2];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) acc[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
        for (int cb = cb0; cb < cb0 + DA_BLOCK; cb += 4) {
            const int co = cb + q;
            const float* wr = wt_t + (size_t)co * cin;
            const float* zr = zf + (size_t)co * PS + shift;
            const float z0 = zr[i0], z1 = zr[i1];
            float wa[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) wa[a] = wr[16 * a];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                acc[a][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[a], z0, acc[a][0], 0, 0, 0);
                acc[a][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[a], z1, acc[a][1], 0, 0, 0);
            }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 2; ++b) tot[a][b] += acc[a][b];
    }
}

} // namespace
