// What down_train.hip (the fp32 strided-stage backward) and down_train16.hip (its 16-bit operand twin) share: the workspace of a
// context and its budget rules, the parity planes of x, the norm backward that writes dz into its padded plane (fp32 / fp64 in every
// mode), the K ranges of a wgrad launch and the reduction of the dw partials.  One copy, so that both files build the planes, cut K
// and sum the partials the same way.
#pragma once
#include <cmath>
#include "pp_common.h"
#include "train_planes.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr size_t DOWN_WS_BUDGET = (size_t)256 << 20; // bytes of one frame's x parity planes + dz planes: a larger map is refused
constexpr size_t DOWN_WS_CHUNK = (size_t)1 << 30;    // bytes of the planes of one chunk of frames: larger batches run in frame chunks
constexpr int DW_WGS = 512;                          // workgroups a wgrad launch aims at (output tiles x K ranges)
constexpr int DW_MAX_SPLIT = 256;
constexpr int DA_BLOCK = 64;                         // k-terms that k_down_dgrad sums in one accumulator before adding the block to the total

struct down_ws {
    float* planes = nullptr; size_t planes_elems = 0; // xp [fc][Cin][4][PS], then dz [fc][Cout][PS]
    double* pst = nullptr;   size_t pst_elems = 0;    // [2][fc][Cout][segments][2]: a plane's segment sums of (z, z^2), then of (Gr, Gr xhat)
    float* wT = nullptr;     size_t wT_elems = 0;
    float* part = nullptr;   size_t part_elems = 0;
    float* coef = nullptr;   size_t coef_elems = 0;   // [Cout][4]: k_bn_coef's coefficients (pp_down_backward_bn)
    uint16_t* wT16 = nullptr; size_t wT16_elems = 0;  // [part][9][ci][co] bf16: the dgrad's A operand (pp_down_backward_mp, down_train16.hip)
};

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
int grow(pp_ctx* ctx, T** buf, size_t* have, size_t need)
{
    if (need <= *have) return 0;
    PP_HIP(hipDeviceSynchronize()); // a kernel of an earlier call, on this stream or another, may still read the old buffer
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *have = 0;
    PP_HIP(hipMalloc((void**)buf, need * sizeof(T)));
    *have = need;
    return 0;
}

// ---- the four parity planes of x: grid (Cin, frames, SP), one slice of LP positions per workgroup.  A position takes its 2 x 2 input
// pixels (x is read once, whole rows at a time) and writes one element of each plane -----------------------------------------------
__global__ void __launch_bounds__(256) k_down_xpack(const float* __restrict__ x, float* __restrict__ xp, int cin, int hin, int win, int ho, int wo,
                                                    int wp, int G, int PP, int PS, int LP)
{
    const size_t pl = (size_t)blockIdx.y * cin + blockIdx.x;
    const float* xi = x + pl * hin * win;
    float* xo = xp + pl * 4 * PS;
    const int lo = blockIdx.z * LP, hi = lo + LP < PS ? lo + LP : PS;
    for (int j = lo + threadIdx.x; j < hi; j += 256) {
        const int P = j - G;
        float v00 = 0.f, v01 = 0.f, v10 = 0.f, v11 = 0.f; // (row parity, column parity)
        if (P >= 0 && P < PP) {
            const int y = P / wp, c = P - y * wp;
            if (y >= 1 && y <= ho && c >= 1 && c <= wo) {
                const int iy = 2 * (y - 1), ix = 2 * (c - 1); // in the image: 2 (ho - 1) < hin, 2 (wo - 1) < win
                const float* r = xi + (size_t)iy * win + ix;
                const bool right = ix + 1 < win, below = iy + 1 < hin;
                v00 = r[0];
                if (right) v01 = r[1];
                if (below) v10 = r[win];
                if (right && below) v11 = r[win + 1];
            }
        }
        xo[j] = v00; xo[PS + j] = v01; xo[2 * PS + j] = v10; xo[3 * PS + j] = v11;
    }
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
    const int tid = threadIdx.x, N = ho * wo;
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
    for (int j = lo + tid; j < hi; j += 256) {
        const int P = j - G;
        float v = 0.f;
        if (P >= 0 && P < PP) {
            const int y = P / wp, c = P - y * wp;
            if (y >= 1 && y <= ho && c >= 1 && c <= wo) {
                const int i = (y - 1) * wo + c - 1;
                const float xhat = (zi[i] - meanf) * rstdf;
                const float g = xhat > 0.f ? dp[i] : 0.f;
                v = rstdf * ((g - c1) - xhat * c2);
            }
        }
        zo[j] = v;
    }
}

// partials added in index order, four loads in flight: 64-thread workgroups, so that a 64 x 64 weight spreads over all compute units
__global__ void __launch_bounds__(64) k_down_dw_reduce(const float* __restrict__ part, int G, int n, float* __restrict__ dw)
{
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const float* p = part + i;
    double s = 0.0;
    int g = 0;
    for (; g + 3 < G; g += 4) {
        const float a = p[(size_t)g * n], b = p[(size_t)(g + 1) * n], c = p[(size_t)(g + 2) * n], d = p[(size_t)(g + 3) * n];
        s += (double)a; s += (double)b; s += (double)c; s += (double)d;
    }
    for (; g < G; ++g) s += (double)p[(size_t)g * n];
    dw[i] = (float)s;
}

inline down_ws* workspace(pp_ctx* ctx)
{
    if (!ctx->down) ctx->down = new down_ws();
    return (down_ws*)ctx->down;
}

// K ranges of one wgrad launch over `nchunks` chunks of positions (16 per chunk in the fp32 kernels, 32 in the 16-bit ones)
inline void dw_ranges(int tiles, int nchunks, int* splits, int* cps, int wgs = DW_WGS)
{
    int sp = wgs / tiles;
    sp = sp < 1 ? 1 : sp > DW_MAX_SPLIT ? DW_MAX_SPLIT : sp;
    if (sp > nchunks) sp = nchunks;
    *cps = (nchunks + sp - 1) / sp;
    *splits = (nchunks + *cps - 1) / *cps;
}

} // namespace
