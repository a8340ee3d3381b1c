// Training the pillar feature net: PointNet.forward in train mode (BatchNorm1d with batch statistics), its backward with respect to
// the three learnable tensors, the scatter's backward, and the in-place update of the eval-mode PFN (include/pp_hip.h has the maths).
//
// Forward, three launches:
//   pfn_stats_kernel   one wave per pillar, lane = point slot: the nine decorated features in fp32 exactly as pfn_kernel forms them,
//                      then s[9] and the upper triangle of M[9][9] (45) accumulated per lane in fp64 (products of two fp32 values are
//                      exact there), one halving butterfly over the 64 lanes per wave, the eight waves of a block added in wave order through LDS and
//                      one partial row per block: part[54][blocks].  HBM: 16 T B read per pillar.
//   pfn_stats_finish   one block of 16 waves: wave v sums the partials of values v, v + 16, ... in block order; 64 threads then derive
//                      mean, biased variance and the folded scale / shift per channel in fp64.
//   pfn_train_kernel   pfn_kernel's layout (one wave per pillar, lane = channel, tile loaded once, readlane broadcast) with the batch
//                      scale / shift; it also records the first slot that attains the maximum.  HBM: 16 T B read, 256 + 64 B written.
// Backward, two launches:
//   pfn_bwd_kernel     one wave per pillar, lane = channel: each lane gathers the row of its own arg slot (the tile was just read for
//                      the pillar mean, so the 64 16-byte reads hit the cache), recomputes its nine features and z with pfn_kernel's FMA
//                      chain and accumulates S1, S2 and G[c][0:9] in fp64; the sixteen waves of a block are added in wave order through
//                      LDS and the block writes one partial row [11][64].  HBM: 16 T + 256 + 256 + 64 B read per pillar.
//   pfn_bwd_finish     one block of 16 waves: wave v adds the partial rows v, v + 16, ... (lane = channel), the waves are added in wave
//                      order through LDS, then 576 threads evaluate dW and 64 write dgamma / dbeta.
// The pillar loops are bound by the latency of a pillar's dependent loads, so both passes run large blocks (eight waves where a lane holds 54 fp64
// accumulators, sixteen in the backward): many waves in flight, few partial rows for the finishing block.
// Every sum has a fixed order that depends on the launch shape alone: no atomics, two runs agree bit for bit.
#include "pp_common.h"
#include <algorithm>
#include <cmath>

namespace {

constexpr int RED_THREADS = 1024, RED_WAVES = RED_THREADS / 64; // block shape of both reducing passes and of their finishing blocks
constexpr int ST_THREADS = 512, ST_WAVES = ST_THREADS / 64;      // the statistics pass keeps 54 fp64 accumulators per lane: 8 waves per block
constexpr int ST_BLOCKS = 512;  // statistics pass: at most 4096 waves; the finishing block reads at most 54 x 512 doubles
constexpr int NSTAT = 54;       // s[9] + upper triangle of M (45)
constexpr int BW_BLOCKS = 256;  // backward pass: one partial row [11][64] per block
constexpr int NACC = 11;        // S1, S2, G[0:9]
constexpr double BN_EPS = 1e-5;

struct pfnt_ws {
    double* st_part = nullptr; // [NSTAT][ST_BLOCKS]
    double* bw_part = nullptr; // [BW_BLOCKS][NACC][64]
    float* fold = nullptr;     // scale[64], shift[64] of the batch statistics
};

struct pfn_geom {
    float vx, vy, x_off, y_off;
    int T;
};

__device__ __forceinline__ double wave_sum(double a)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) a += __shfl_xor(a, m);
    return a;
}

// mean of x, y, z over ALL T slots divided by n, summed as pfn_kernel sums it (lane j owns floats j, j + 64, ...)
__device__ __forceinline__ void pillar_mean(const float* __restrict__ v, int T, int n, int lane, float& mx, float& my, float& mz)
{
    float s = 0.f;
    for (int j = lane; j < T * 4; j += 64) s += v[j];
    s += __shfl_xor(s, 4); s += __shfl_xor(s, 8); s += __shfl_xor(s, 16); s += __shfl_xor(s, 32);
    const float fn = (float)n;
    mx = __shfl(s, 0) / fn; my = __shfl(s, 1) / fn; mz = __shfl(s, 2) / fn;
}

__device__ __forceinline__ void decorate(float x, float y, float z, float r, float mx, float my, float mz, float cxf, float cyf, float* f)
{
    f[0] = x; f[1] = y; f[2] = z; f[3] = r;
    f[4] = x - mx; f[5] = y - my; f[6] = z - mz;
    f[7] = x - cxf; f[8] = y - cyf;
}

__device__ __forceinline__ float conv9(const float* w, const float* f)
{
    float a = w[0] * f[0];
#pragma unroll
    for (int k = 1; k < 9; ++k) a = fmaf(w[k], f[k], a);
    return a;
}

__global__ void __launch_bounds__(ST_THREADS) pfn_stats_kernel(const float* __restrict__ voxels, const int32_t* __restrict__ coors,
                                                        const int32_t* __restrict__ npts, const int32_t* __restrict__ num_pillars, int pmax,
                                                        pfn_geom g, double* __restrict__ part)
{
    __shared__ double red[ST_WAVES][NSTAT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, T = g.T;
    const int P = min(*num_pillars, pmax);
    const int waves = (gridDim.x * blockDim.x) >> 6, wave = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    double acc[NSTAT];
#pragma unroll
    for (int i = 0; i < NSTAT; ++i) acc[i] = 0.0;
    for (int p = wave; p < P; p += waves) {
        const float* v = voxels + (size_t)p * T * 4;
        const int n = min(npts[p], T);
        float mx, my, mz;
        pillar_mean(v, T, n, lane, mx, my, mz);
        const float cxf = __fadd_rn(__fmul_rn((float)coors[3 * p], g.vx), g.x_off);
        const float cyf = __fadd_rn(__fmul_rn((float)coors[3 * p + 1], g.vy), g.y_off);
        for (int t = lane; t < n; t += 64) {
            const float4 q = *reinterpret_cast<const float4*>(v + 4 * t);
            float f[9];
            decorate(q.x, q.y, q.z, q.w, mx, my, mz, cxf, cyf, f);
            double d[9];
#pragma unroll
            for (int k = 0; k < 9; ++k) { d[k] = (double)f[k]; acc[k] += d[k]; }
            int i = 9;
#pragma unroll
            for (int j = 0; j < 9; ++j)
#pragma unroll
                for (int k = j; k < 9; ++k) acc[i++] += d[j] * d[k];
        }
    }
    // 54 sums over the 64 lanes as one butterfly that halves the values a lane carries at every step (63 exchanges instead of
    // 54 x 6): at mask m the lane whose bit m is set keeps the upper half of its values and sends the lower half, so that lane l ends
    // with the wave's total of value l.  The order of every sum is fixed by the lane numbers.
    double v[64];
#pragma unroll
    for (int i = 0; i < 64; ++i) v[i] = i < NSTAT ? acc[i] : 0.0;
#pragma unroll
    for (int half = 32; half >= 1; half >>= 1) {
        const bool up = (lane & half) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const double keep = up ? v[i + half] : v[i], send = up ? v[i] : v[i + half];
            v[i] = keep + __shfl_xor(send, half);
        }
    }
    if (lane < NSTAT) red[wv][lane] = v[0];
    __syncthreads();
    if (threadIdx.x < NSTAT) {
        double a = red[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < ST_WAVES; ++w) a += red[w][threadIdx.x];
        part[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = a;
    }
}

__device__ __forceinline__ int tri(int j, int k) { return 9 + j * 9 - j * (j - 1) / 2 + (k - j); } // j <= k

__global__ void __launch_bounds__(RED_THREADS) pfn_stats_finish(const double* __restrict__ part, int nblk, const int32_t* __restrict__ num_pillars, int pmax,
                                                         int T, const float* __restrict__ w, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, double* __restrict__ stats, float* __restrict__ fold)
{
    __shared__ double sm[NSTAT];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = wv; i < NSTAT; i += RED_WAVES) {
        double a = 0.0;
#pragma unroll 4
        for (int j = lane; j < nblk; j += 64) a += part[(size_t)i * nblk + j];
        a = wave_sum(a);
        if (lane == 0) sm[i] = a;
    }
    __syncthreads();
    const int c = threadIdx.x;
    if (c < 64) {
        const double N = (double)min(*num_pillars, pmax) * (double)T;
        double wc[9], ws = 0.0, q = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) { wc[k] = (double)w[c * 9 + k]; ws += wc[k] * sm[k]; }
#pragma unroll
        for (int j = 0; j < 9; ++j) {
            double r = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) r += sm[j <= k ? tri(j, k) : tri(k, j)] * wc[k];
            q += wc[j] * r;
        }
        const double mean = ws / N;
        const double var = fmax(q / N - mean * mean, 0.0);
        const double s = (double)gamma[c] / sqrt(var + BN_EPS);
        stats[c] = mean;
        stats[64 + c] = var;
        fold[c] = (float)s;
        fold[64 + c] = (float)((double)beta[c] - mean * s);
    } else if (c < 64 + 9) {
        stats[128 + (c - 64)] = sm[c - 64];
    } else if (c < 64 + 9 + 81) {
        const int j = (c - 73) / 9, k = (c - 73) % 9;
        stats[137 + j * 9 + k] = sm[j <= k ? tri(j, k) : tri(k, j)];
    }
}

__global__ void __launch_bounds__(256) pfn_train_kernel(const float* __restrict__ voxels, const int32_t* __restrict__ coors, const int32_t* __restrict__ npts,
                                                        const int32_t* __restrict__ num_pillars, int pmax, const float* __restrict__ wgt /*[64][9]*/,
                                                        const float* __restrict__ fold, pfn_geom g, float* __restrict__ feat, uint8_t* __restrict__ arg)
{
    const int lane = threadIdx.x & 63, T = g.T;
    const int P = min(*num_pillars, pmax);
    float w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = wgt[lane * 9 + k];
    const float sc = fold[lane], sh = fold[64 + lane];
    const float pad = fmaxf(sh, 0.f);
    const int waves = (gridDim.x * blockDim.x) >> 6;
    for (int p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < P; p += waves) {
        const float* v = voxels + (size_t)p * T * 4;
        const int n = min(npts[p], T);
        float mx, my, mz;
        pillar_mean(v, T, n, lane, mx, my, mz);
        const float cxf = __fadd_rn(__fmul_rn((float)coors[3 * p], g.vx), g.x_off);
        const float cyf = __fadd_rn(__fmul_rn((float)coors[3 * p + 1], g.vy), g.y_off);
        float best = -INFINITY;
        int at = 0;
        for (int t0 = 0; t0 < n; t0 += 16) {
            const int j = t0 * 4 + lane;
            const float mine = (j < T * 4) ? v[j] : 0.f;
            const int tn = min(16, n - t0);
            for (int t = 0; t < tn; ++t) {
                const float x = __shfl(mine, 4 * t), y = __shfl(mine, 4 * t + 1), z = __shfl(mine, 4 * t + 2), r = __shfl(mine, 4 * t + 3);
                float f[9];
                decorate(x, y, z, r, mx, my, mz, cxf, cyf, f);
                const float a = fmaxf(fmaf(conv9(w, f), sc, sh), 0.f);
                if (a > best) { best = a; at = t0 + t; } // strict: the first slot that attains the maximum
            }
        }
        if (n < T && pad > best) { best = pad; at = n; } // the padded slots (z = 0) come after the real ones
        feat[(size_t)p * 64 + lane] = best;
        arg[(size_t)p * 64 + lane] = (uint8_t)at;
    }
}

// red[i][lane] = the waves' acc[i] added in wave order (lane = channel); every thread of the block calls it
__device__ __forceinline__ void block_sum_rows(double* red, const double* acc, int wv, int lane)
{
    for (int w = 0; w < RED_WAVES; ++w) {
        if (wv == w) {
#pragma unroll
            for (int i = 0; i < NACC; ++i) red[i * 64 + lane] = w ? red[i * 64 + lane] + acc[i] : acc[i];
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) scatter_bwd_kernel(const float* __restrict__ dcanvas, const int32_t* __restrict__ coors,
                                                          const int32_t* __restrict__ num_pillars, int pmax, int gx, int gy, size_t plane,
                                                          float* __restrict__ dfeat)
{
    const int lane = threadIdx.x & 63;
    const int P = min(*num_pillars, pmax);
    const int waves = (gridDim.x * blockDim.x) >> 6;
    for (int p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < P; p += waves) {
        const int cx = coors[3 * p], cy = coors[3 * p + 1];
        const bool in = (unsigned)cx < (unsigned)gx && (unsigned)cy < (unsigned)gy; // the forward skips a coordinate outside the grid
        dfeat[(size_t)p * 64 + lane] = in ? dcanvas[(size_t)lane * plane + (size_t)cx * gy + cy] : 0.f;
    }
}

__global__ void __launch_bounds__(RED_THREADS) pfn_bwd_kernel(const float* __restrict__ voxels, const int32_t* __restrict__ coors, const int32_t* __restrict__ npts,
                                                      const int32_t* __restrict__ num_pillars, int pmax, const float* __restrict__ wgt /*[64][9]*/,
                                                      const double* __restrict__ stats, const float* __restrict__ feat, const uint8_t* __restrict__ arg,
                                                      const float* __restrict__ dfeat, pfn_geom g, double* __restrict__ part)
{
    __shared__ double red[NACC * 64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, T = g.T;
    const int P = min(*num_pillars, pmax);
    float w[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) w[k] = wgt[lane * 9 + k];
    const double mean = stats[lane], invstd = 1.0 / sqrt(stats[64 + lane] + BN_EPS);
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    const int waves = (gridDim.x * blockDim.x) >> 6;
    for (int p = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; p < P; p += waves) {
        const float* v = voxels + (size_t)p * T * 4;
        const int n = min(npts[p], T);
        float mx, my, mz;
        pillar_mean(v, T, n, lane, mx, my, mz);
        const float cxf = __fadd_rn(__fmul_rn((float)coors[3 * p], g.vx), g.x_off);
        const float cyf = __fadd_rn(__fmul_rn((float)coors[3 * p + 1], g.vy), g.y_off);
        const size_t o = (size_t)p * 64 + lane;
        const double gd = feat[o] > 0.f ? (double)dfeat[o] : 0.0; // ReLU: no gradient where the maximum is not positive
        const int ts = arg[o];
        float f[9], z = 0.f;
#pragma unroll
        for (int k = 0; k < 9; ++k) f[k] = 0.f;
        if (ts < n) { // a padded slot (ts >= n) has f = 0 and z = 0
            const float4 q = *reinterpret_cast<const float4*>(v + 4 * ts);
            decorate(q.x, q.y, q.z, q.w, mx, my, mz, cxf, cyf, f);
            z = conv9(w, f);
        }
        acc[0] += gd;
        acc[1] += gd * (((double)z - mean) * invstd);
#pragma unroll
        for (int k = 0; k < 9; ++k) acc[2 + k] += gd * (double)f[k];
    }
    block_sum_rows(red, acc, wv, lane);
    for (int i = threadIdx.x; i < NACC * 64; i += RED_THREADS) part[(size_t)blockIdx.x * (NACC * 64) + i] = red[i];
}

__global__ void __launch_bounds__(RED_THREADS) pfn_bwd_finish(const double* __restrict__ part, int nblk, const int32_t* __restrict__ num_pillars, int pmax, int T,
                                                       const float* __restrict__ w, const float* __restrict__ gamma, const double* __restrict__ stats,
                                                       float* __restrict__ dw, float* __restrict__ dgamma, float* __restrict__ dbeta)
{
    __shared__ double tot[NACC * 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    double acc[NACC];
#pragma unroll
    for (int i = 0; i < NACC; ++i) acc[i] = 0.0;
    // rows wv, wv + 16, ...: four rows' loads are issued together, then added in row order
    for (int b0 = wv; b0 < nblk; b0 += 4 * RED_WAVES) {
        double x[4][NACC];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = b0 + r * RED_WAVES;
#pragma unroll
            for (int i = 0; i < NACC; ++i) x[r][i] = b < nblk ? part[(size_t)b * (NACC * 64) + i * 64 + lane] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int i = 0; i < NACC; ++i) acc[i] += x[r][i];
    }
    block_sum_rows(tot, acc, wv, lane);
    if (tid < 576) {
        const int c = tid / 9, k = tid % 9;
        const double N = (double)min(*num_pillars, pmax) * (double)T;
        const double S1 = tot[c], S2 = tot[64 + c], G = tot[(2 + k) * 64 + c];
        const double mean = stats[c], invstd = 1.0 / sqrt(stats[64 + c] + BN_EPS), sk = stats[128 + k];
        double wm = 0.0;
#pragma unroll
        for (int j = 0; j < 9; ++j) wm += (double)w[c * 9 + j] * stats[137 + j * 9 + k];
        dw[tid] = (float)((double)gamma[c] * invstd * (G - S1 * sk / N - S2 * invstd * (wm - mean * sk) / N));
    } else if (tid < 640) {
        const int c = tid - 576;
        dbeta[c] = (float)tot[c];
        dgamma[c] = (float)tot[64 + c];
    }
}

// the eval-mode fold of pp_commit_weights (pp_api.hip), on the device
__global__ void __launch_bounds__(576) pfn_fold_kernel(const float* __restrict__ w, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                       const float* __restrict__ rm, const float* __restrict__ rv, float* __restrict__ wT,
                                                       float* __restrict__ scale, float* __restrict__ shift)
{
    const int i = threadIdx.x;
    wT[(i % 9) * 64 + i / 9] = w[i];
    if (i < 64) {
        const double s = (double)gamma[i] / sqrt((double)rv[i] + BN_EPS);
        scale[i] = (float)s;
        shift[i] = (float)((double)beta[i] - (double)rm[i] * s);
    }
}

int ws_get(pp_ctx* ctx, pfnt_ws** out)
{
    if (!ctx->pfnt) {
        pfnt_ws* w = new pfnt_ws();
        ctx->pfnt = w; // pp_pfn_train_destroy frees what was allocated if a later allocation fails
        PP_HIP(hipMalloc((void**)&w->st_part, sizeof(double) * NSTAT * ST_BLOCKS));
        PP_HIP(hipMalloc((void**)&w->bw_part, sizeof(double) * BW_BLOCKS * NACC * 64));
        PP_HIP(hipMalloc((void**)&w->fold, sizeof(float) * 128));
    }
    *out = (pfnt_ws*)ctx->pfnt;
    if (!(*out)->st_part || !(*out)->bw_part || !(*out)->fold) return pp_fail(ctx, PP_E_STATE, "pfn training: the workspace could not be allocated");
    return 0;
}

pfn_geom geom_of(const pp_config& c)
{
    pfn_geom g;
    g.vx = c.voxel_size[0];
    g.vy = c.voxel_size[1];
    g.x_off = g.vx / 2 + c.offset[0]; // :18-19
    g.y_off = g.vy / 2 + c.offset[1];
    g.T = c.max_num_points;
    return g;
}

int64_t pillar_limit(const pp_ctx* ctx) { return (int64_t)ctx->max_batch * ctx->cfg.max_voxels; }

} // namespace

void pp_pfn_train_destroy(pp_ctx* ctx)
{
    pfnt_ws* w = (pfnt_ws*)ctx->pfnt;
    if (!w) return;
    void* q[] = {w->st_part, w->bw_part, w->fold};
    for (void* x : q)
        if (x) (void)hipFree(x);
    delete w;
    ctx->pfnt = nullptr;
}

extern "C" int pp_pfn_train_forward(pp_ctx* ctx, const float* voxels, const int32_t* coors, const int32_t* npts, const int32_t* num_pillars,
                                    const float* w, const float* gamma, const float* beta, float* feat, uint8_t* arg, double* stats, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (!voxels || !coors || !npts || !num_pillars || !w || !gamma || !beta || !feat || !arg || !stats)
        return pp_fail(ctx, PP_E_ARG, "pp_pfn_train_forward: null pointer");
    const pp_config& c = ctx->cfg;
    if (c.num_point_features != 4) return pp_fail(ctx, PP_E_ARG, "pp_pfn_train_forward: only F=4 point features supported");
    if (c.max_num_points > 255) return pp_fail(ctx, PP_E_ARG, "pp_pfn_train_forward: max_num_points must not exceed 255 (arg is a byte)");
    if ((uintptr_t)voxels & 15) return pp_fail(ctx, PP_E_ARG, "pp_pfn_train_forward: voxels must be 16-byte aligned");
    const int64_t pmax = pillar_limit(ctx);
    if (pmax > INT32_MAX) return pp_fail(ctx, PP_E_ARG, "pp_pfn_train_forward: max_batch * max_voxels out of range");
    int32_t P = 0;
    PP_HIP(hipMemcpyAsync(&P, num_pillars, sizeof(P), hipMemcpyDeviceToHost, stream));
    PP_HIP(hipStreamSynchronize(stream));
    if (P > pmax) P = (int32_t)pmax;
    if ((int64_t)P * c.max_num_points < 2)
        return pp_fail(ctx, PP_E_ARG, "pp_pfn_train_forward: batch statistics need more than one value per channel (pillars x max_num_points < 2)");
    pfnt_ws* ws = nullptr;
    if (int rc = ws_get(ctx, &ws)) return rc;
    const pfn_geom g = geom_of(c);
    const int blocks = std::min(ST_BLOCKS, pp_div_up(P, ST_WAVES));
    hipLaunchKernelGGL(pfn_stats_kernel, dim3(blocks), dim3(ST_THREADS), 0, stream, voxels, coors, npts, num_pillars, (int)pmax, g, ws->st_part);
    PP_HIP(hipGetLastError());
    hipLaunchKernelGGL(pfn_stats_finish, dim3(1), dim3(RED_THREADS), 0, stream, ws->st_part, blocks, num_pillars, (int)pmax, g.T, w, gamma, beta, stats,
                       ws->fold);
    PP_HIP(hipGetLastError());
    hipLaunchKernelGGL(pfn_train_kernel, dim3(std::min(1024, pp_div_up(P, 4))), dim3(256), 0, stream, voxels, coors, npts, num_pillars, (int)pmax, w,
                       ws->fold, g, feat, arg);
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_scatter_backward(pp_ctx* ctx, const float* dcanvas, const int32_t* coors, const int32_t* num_pillars, float* dfeat, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (!dcanvas || !coors || !num_pillars || !dfeat) return pp_fail(ctx, PP_E_ARG, "pp_scatter_backward: null pointer");
    const size_t plane = (size_t)ctx->gx * ctx->gy;
    hipLaunchKernelGGL(scatter_bwd_kernel, dim3(std::min(1024, std::max(1, pp_div_up(ctx->cfg.max_voxels, 4)))), dim3(256), 0, stream, dcanvas, coors,
                       num_pillars, ctx->cfg.max_voxels, ctx->gx, ctx->gy, plane, dfeat);
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_pfn_backward(pp_ctx* ctx, const float* voxels, const int32_t* coors, const int32_t* npts, const int32_t* num_pillars, const float* w,
                               const float* gamma, const double* stats, const float* feat, const uint8_t* arg, const float* dfeat, float* dw,
                               float* dgamma, float* dbeta, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (!voxels || !coors || !npts || !num_pillars || !w || !gamma || !stats || !feat || !arg || !dfeat || !dw || !dgamma || !dbeta)
        return pp_fail(ctx, PP_E_ARG, "pp_pfn_backward: null pointer");
    const pp_config& c = ctx->cfg;
    if (c.num_point_features != 4) return pp_fail(ctx, PP_E_ARG, "pp_pfn_backward: only F=4 point features supported");
    if (c.max_num_points > 255) return pp_fail(ctx, PP_E_ARG, "pp_pfn_backward: max_num_points must not exceed 255 (arg is a byte)");
    if ((uintptr_t)voxels & 15) return pp_fail(ctx, PP_E_ARG, "pp_pfn_backward: voxels must be 16-byte aligned");
    const int64_t pmax = pillar_limit(ctx);
    if (pmax > INT32_MAX) return pp_fail(ctx, PP_E_ARG, "pp_pfn_backward: max_batch * max_voxels out of range");
    pfnt_ws* ws = nullptr;
    if (int rc = ws_get(ctx, &ws)) return rc;
    const pfn_geom g = geom_of(c);
    const int blocks = (int)std::min<int64_t>(BW_BLOCKS, std::max<int64_t>(1, pp_div_up(pmax, RED_WAVES)));
    hipLaunchKernelGGL(pfn_bwd_kernel, dim3(blocks), dim3(RED_THREADS), 0, stream, voxels, coors, npts, num_pillars, (int)pmax, w, stats, feat, arg, dfeat, g,
                       ws->bw_part);
    PP_HIP(hipGetLastError());
    hipLaunchKernelGGL(pfn_bwd_finish, dim3(1), dim3(RED_THREADS), 0, stream, ws->bw_part, blocks, num_pillars, (int)pmax, g.T, w, gamma, stats, dw, dgamma,
                       dbeta);
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_update_pfn_weights(pp_ctx* ctx, const float* w, const float* gamma, const float* beta, const float* running_mean,
                                     const float* running_var, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_update_pfn_weights: weights not committed");
    if (!w || !gamma || !beta || !running_mean || !running_var) return pp_fail(ctx, PP_E_ARG, "pp_update_pfn_weights: null pointer");
    hipLaunchKernelGGL(pfn_fold_kernel, dim3(1), dim3(576), 0, stream, w, gamma, beta, running_mean, running_var, ctx->pfn_w, ctx->pfn_scale,
                       ctx->pfn_shift);
    PP_HIP(hipGetLastError());
    return 0;
}
