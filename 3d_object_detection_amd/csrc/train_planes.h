// The device side that the streaming passes of block_train.hip and down_train.hip share (the host side of the training backwards is
// train_host.h's, the two MFMA products train_conv3.h's): how a plane is cut into segments, the fixed-order sums of a workgroup, the
// walk over a slice of the padded plane, the statistics kernel and the mean / rstd of a plane from its sums.  One copy, so that both
// files cut a plane the same way and a shape keeps its bits in both.
// k_affine_reduce, the last step of the three pp_*_backward_affine entries, is here for neck_train.hip as well, and so is k_bn_coef,
// which pools the sums of the three pp_*_backward_bn entries.
#pragma once
#include "pp_common.h"

namespace {

constexpr int SEG_ELEMS = 16384; // plane elements one workgroup of a streaming pass takes
constexpr int SEG_MAX = 16;

// ---- segments of a plane: plane_segs(n) workgroups share n elements, each a run of seg_len (a multiple of 256); one segment up to
// SEG_ELEMS elements -------------------------------------------------------------------------------------------------------------------
inline int plane_segs(int64_t n) { const int64_t s = (n + SEG_ELEMS - 1) / SEG_ELEMS; return s < 1 ? 1 : s > SEG_MAX ? SEG_MAX : (int)s; }
inline int seg_len(int64_t n, int S) { return (int)((((n + S - 1) / S) + 255) & ~(int64_t)255); }

// both sums over the 256 threads' partials (segment t: elements t, t + 256, ...), added in index order 0 .. 255 by every thread: the
// same bits in every thread
__device__ __forceinline__ void block_sum2(double& a, double& b, double (*red)[2])
{
    __syncthreads(); // red may still be read from an earlier call
    red[threadIdx.x][0] = a; red[threadIdx.x][1] = b;
    __syncthreads();
    double sa = 0.0, sb = 0.0;
    for (int t = 0; t < 256; ++t) { sa += red[t][0]; sb += red[t][1]; }
    a = sa; b = sb;
}

// thread t of the workgroup visits lo + t, lo + t + 256, ... below hi in that order, four loads in flight: acc sees the same sequence
// as the plain loop, so a sum built in it has the same bits
template <typename LD, typename ACC>
__device__ __forceinline__ void strided4(int lo, int hi, LD ld, ACC acc)
{
    int i = lo + (int)threadIdx.x;
    for (; i + 768 < hi; i += 1024) {
        const auto a = ld(i), b = ld(i + 256), c = ld(i + 512), d = ld(i + 768);
        acc(a); acc(b); acc(c); acc(d);
    }
    for (; i < hi; i += 256) acc(ld(i));
}

// thread t of the workgroup visits elements j = lo + t, lo + t + 256, ... below hi of the padded plane of an h x w map (padded_plane,
// train_host.h) in that order: body(j, pos), where pos tells whether element j is interior and, if so, its row r, column c and index
// i = r w + c in the tight [h][w] plane.  The one statement of which elements of a padded plane are interior: both products rely on
// the others, halo and guard bands, being zeros, which the callers store themselves
struct plane_pos { bool inside; int i, r, c; };
template <typename F>
__device__ __forceinline__ void padded_walk(int lo, int hi, int h, int w, int wp, int G, int PP, F body)
{
    for (int j = lo + (int)threadIdx.x; j < hi; j += 256) {
        const int P = j - G;
        plane_pos pos{false, 0, 0, 0};
        if (P >= 0 && P < PP) {
            const int y = P / wp, x = P - y * wp;
            if (y >= 1 && y <= h && x >= 1 && x <= w) pos = plane_pos{true, (y - 1) * w + x - 1, y - 1, x - 1};
        }
        body(j, pos);
    }
}

// ---- statistics: grid (C, frames, S), sum u and sum u^2 of one segment of a tight [C][N] plane -> pst[plane][segment][2] ------------
__global__ void __launch_bounds__(256) k_plane_stats(const float* __restrict__ u, double* __restrict__ pst, int C, int N, int L, int S)
{
    __shared__ double red[256][2];
    const int tid = threadIdx.x;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float* up = u + pl * N;
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    double s = 0.0, ss = 0.0;
    strided4(lo, hi, [&](int i) { return up[i]; }, [&](float f) { const double v = (double)f; s += v; ss += v * v; });
    block_sum2(s, ss, red);
    if (tid == 0) { pst[(pl * S + blockIdx.z) * 2] = s; pst[(pl * S + blockIdx.z) * 2 + 1] = ss; }
}

// mean and rstd of a plane as the forward rounds them, from its segment sums added in index order
__device__ __forceinline__ void plane_mean_rstd(const double* __restrict__ pst, size_t pl, int S, int N, float& meanf, float& rstdf)
{
    double s = 0.0, ss = 0.0;
    for (int g = 0; g < S; ++g) { s += pst[(pl * S + g) * 2]; ss += pst[(pl * S + g) * 2 + 1]; }
    const double inv_n = 1.0 / (double)N, mean = s * inv_n;
    double var = ss * inv_n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    meanf = (float)mean; rstdf = (float)(1.0 / sqrt(var + 1e-3));
}

// ---- per-channel affine (frozen BatchNorm) backward: the two sums of a channel from pst[frame][c][segment][2], segments added in index
// order, frames in frame order, left in fp64 (the caller's dgamma is a difference of the two that cancels) -----------------------------
__global__ void __launch_bounds__(64) k_affine_reduce(const double* __restrict__ pst, int nb, int C, int S, double* __restrict__ dscale,
                                                      double* __restrict__ dshift)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int f = 0; f < nb; ++f) {
        const double* p = pst + ((size_t)f * C + c) * S * 2;
        for (int s = 0; s < S; ++s) { a += p[2 * s]; b += p[2 * s + 1]; }
    }
    dscale[c] = a; dshift[c] = b;
}

// ---- train-mode BatchNorm backward (the three pp_*_backward_bn entries): a channel's two sums pooled as k_affine_reduce pools them,
// a = sum g v and b = sum g over all frames, and from them and the batch statistics the coefficients of the norm backward over n = frames
// x positions elements, formed in fp64 and rounded once each: coef[c] = {c1 = b / n, c2 = r (a - mean b) / n, mean, r}, r = 1 /
// sqrt(var + 1e-3).  dscale / dshift (nullable) take the sums themselves ----------------------------------------------------------------
__global__ void __launch_bounds__(64) k_bn_coef(const double* __restrict__ pst, int nb, int C, int S, const float* __restrict__ mean,
                                                const float* __restrict__ var, double n, float* __restrict__ coef, double* __restrict__ dscale,
                                                double* __restrict__ dshift)
{
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    double a = 0.0, b = 0.0;
    for (int f = 0; f < nb; ++f) {
        const double* p = pst + ((size_t)f * C + c) * S * 2;
        for (int s = 0; s < S; ++s) { a += p[2 * s]; b += p[2 * s + 1]; }
    }
    const float meanf = mean[c];
    const double r = 1.0 / sqrt((double)var[c] + 1e-3);
    coef[4 * c] = (float)(b / n);
    coef[4 * c + 1] = (float)(r * (a - (double)meanf * b) / n);
    coef[4 * c + 2] = meanf;
    coef[4 * c + 3] = (float)r;
    if (dscale) { dscale[c] = a; dshift[c] = b; }
}

} // namespace
