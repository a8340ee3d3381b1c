// What neck_train.hip (the fp32 upsampling-branch backward) and neck_train16.hip (its 16-bit operand twin) share: the workspace of a
// context and its budget, the recomputed forward Z = w^T x, the statistics and dZ kernels (fp32 / fp64 in every mode), the K ranges
// of a dw launch and the reduction of the dw partials.  One copy, so that both files form dZ, cut K and sum the partials the same way.
#pragma once
#include <cmath>
#include "pp_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr size_t Z_BUDGET = (size_t)256 << 20; // bytes of Z / dZ workspace: larger batches run in frame chunks
constexpr int DW_WGS = 512;                    // workgroups a dw launch aims at (output tiles x K ranges)
constexpr int DW_MAX_SPLIT = 256;
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

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <typename T>
int grow(pp_ctx* ctx, T** buf, size_t* have, size_t need, hipStream_t stream)
{
    if (need <= *have) return 0;
    PP_HIP(hipStreamSynchronize(stream)); // a running kernel may still read the old buffer
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *have = 0;
    PP_HIP(hipMalloc((void**)buf, need * sizeof(T)));
    *have = need;
    return 0;
}

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

__global__ void __launch_bounds__(256) k_neck_dw_reduce(const float* __restrict__ part, int G, int n, float* __restrict__ dw)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double s = 0.0;
    for (int g = 0; g < G; ++g) s += (double)part[(size_t)g * n + i];
    dw[i] = (float)s;
}

inline neck_ws* workspace(pp_ctx* ctx)
{
    if (!ctx->neck) ctx->neck = new neck_ws();
    return (neck_ws*)ctx->neck;
}

// K ranges of one dw launch over `nchunks` 16-pixel chunks (32-pixel chunks in the 16-bit kernels)
inline void dw_ranges(int tiles, int nchunks, int* splits, int* cps)
{
    int sp = DW_WGS / tiles;
    sp = sp < 1 ? 1 : sp > DW_MAX_SPLIT ? DW_MAX_SPLIT : sp;
    if (sp > nchunks) sp = nchunks;
    *cps = (nchunks + sp - 1) / sp;
    *splits = (nchunks + *cps - 1) / *cps;
}

} // namespace
