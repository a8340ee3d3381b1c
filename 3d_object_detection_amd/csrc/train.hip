// Training side of the anchor head (gfx950): the gradient of LossGenerator's `loss` with respect to the head outputs, the backward
// of SharedHead.forward (three 1x1 convolutions, 320 -> na + 7 na + 2 na channels) and the in-place rewrite of the head's packed
// weights after an optimizer step.  The backbone is frozen: nothing here reaches behind rpn_out, but pp_head_backward returns
// dL/d(rpn_out), the entry point of a later backbone backward.  Gradients are fp32 in every precision mode.
//
// Determinism: no float atomics.  The positive count is an integer atomic; dW / db are per-workgroup partials summed in a fixed
// order by a second kernel, so two runs on the same inputs are bit-identical.
#include <cmath>
#include <cstring>
#include "pp_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// weights of loss_generator.py:16-24 (the same constants framework/loss_generator.py combines the terms with)
constexpr double LOC_WEIGHT = 0.25, CLS_WEIGHT = 1.0, DIR_WEIGHT = 0.2;
constexpr double FOCAL_ALPHA = 0.25;          // gamma = 2 is written out as sig * sig
constexpr double SL1_SIGMA2 = 9.0;            // smooth-L1 sigma^2

struct trn_ws {
    int32_t* npos = nullptr;   // [max_batch] positives per frame of the running pp_target_loss_grad
    float* w_nat = nullptr;    // [rows_padded(na)][320] head weights in natural row order (cls | box | dir), rows >= 10 na zero
    float* part = nullptr;     // dW / db partials of pp_head_backward
    size_t part_elems = 0;
    bool dx_wide_lds = false;  // k_head_dx_wide has been given its dynamic LDS size on this device
    uint64_t w_gen = 0;        // ctx->commit_gen w_nat belongs to (0: none)
    // pp_update_head_weights: index maps of the committed head image (pp_net_head_image)
    uint64_t img_gen = 0;
    pp_head_image img;
    int32_t *wmap = nullptr, *bmap = nullptr, *bpmap = nullptr;
};

// Rows of the head backward's GEMMs: 96 up to 9 anchors per location (the kernels written for that count), above that 10 na rounded
// up to the 16 rows of an MFMA tile (k_head_dw_wide / k_head_dx_wide).
constexpr int HB_MAX_NA = 24; // 12 classes (PP_MAX_CLASSES) x 1 size x 2 rotations
inline int rows_padded(int na) { return 10 * na <= 96 ? 96 : (10 * na + 15) / 16 * 16; }

trn_ws* workspace(pp_ctx* ctx)
{
    if (ctx->trn) return (trn_ws*)ctx->trn;
    trn_ws* w = new trn_ws();
    ctx->trn = w;
    if (hipMalloc((void**)&w->npos, (size_t)ctx->max_batch * sizeof(int32_t)) != hipSuccess ||
        hipMalloc((void**)&w->w_nat, (size_t)rows_padded(ctx->cfg.num_anchor_per_loc) * 320 * sizeof(float)) != hipSuccess) {
        pp_train_destroy(ctx);
        return nullptr;
    }
    return w;
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------
// loss gradient
// ------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_count_pos(const int32_t* __restrict__ labels, int64_t A, int32_t* __restrict__ npos)
{
    const int32_t* lf = labels + (size_t)blockIdx.y * A;
    int n = 0;
    for (int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x; a < A; a += (int64_t)gridDim.x * 256) n += lf[a] > 0;
    for (int o = 32; o; o >>= 1) n += __shfl_xor(n, o);
    if ((threadIdx.x & 63) == 0 && n) atomicAdd(npos + blockIdx.y, n); // integer: order-independent
}

constexpr int LG_ANCH = 512; // anchors per workgroup: two per thread, [512][7] box and target rows staged through LDS

// One workgroup reads the contiguous [n][7] spans of box_preds and bbox_targets of its anchors with 16-byte loads into LDS (rows of 7
// floats are not 16-byte aligned, the span is), computes per anchor (LDS row stride 7 is odd: conflict-free) and writes dbox back
// through the same LDS rows with 16-byte stores.  cls / labels / dir_targets / dcls are 4-byte and dir / ddir 8-byte accesses of
// consecutive lanes (fully coalesced; 12 % and 14 % of the bytes).
__global__ void __launch_bounds__(256) k_loss_grad(const float* __restrict__ cls, const float* __restrict__ box, const float* __restrict__ dir,
                                                   const int32_t* __restrict__ labels, const float* __restrict__ tgt,
                                                   const int32_t* __restrict__ dirt, const int32_t* __restrict__ npos, int64_t A, double sc_cls,
                                                   double sc_box, double sc_dir, float* __restrict__ dcls, float* __restrict__ dbox,
                                                   float* __restrict__ ddir, int vec)
{
    __shared__ __attribute__((aligned(16))) float sb[LG_ANCH * 7];
    __shared__ __attribute__((aligned(16))) float st[LG_ANCH * 7];
    const int tid = threadIdx.x, f = blockIdx.y;
    const int64_t a0 = (int64_t)blockIdx.x * LG_ANCH;
    const int n = (int)(A - a0 < LG_ANCH ? A - a0 : LG_ANCH);
    const size_t fa = (size_t)f * A + a0;
    const float* pb = box + fa * 7;
    const float* pt = tgt + fa * 7;
    float* po = dbox + fa * 7;
    if (vec) { // A % 4 == 0 and 16-byte aligned bases: n * 7 is a multiple of 4 and every span starts on a 16-byte boundary
        for (int i = tid; i < n * 7 / 4; i += 256) {
            reinterpret_cast<float4*>(sb)[i] = reinterpret_cast<const float4*>(pb)[i];
            reinterpret_cast<float4*>(st)[i] = reinterpret_cast<const float4*>(pt)[i];
        }
    } else {
        for (int i = tid; i < n * 7; i += 256) { sb[i] = pb[i]; st[i] = pt[i]; }
    }
    __syncthreads();
    const int np = npos[f];
    // The weights (loss weight x grad_scale / batch / npos) multiply every gradient of the frame: rounded to float32 they would put
    // one common relative error (up to 6e-8; 0.2f alone is 1.5e-8 off) on all of them, a bias that an SGD step turns into a loss shift
    // of 2 x bias x the step's loss decrease (measured: 1e-8 on the small fixture's trajectory).  The float32 formulas of the focal
    // derivative measured the same way: +5.8e-8 relative on <g64, g - g64> / <g64, g64>, a bias, not noise.  So weights and per-anchor
    // arithmetic are double and each gradient is rounded to float32 once; the kernel stays bound by HBM (one exp and one log1p per
    // anchor, sin / cos and a second exp on the positives only).
    const double inv = 1.0 / (double)(np > 1 ? np : 1);
    const double wc = sc_cls * inv, wb = sc_box * inv, wd = sc_dir * inv;
    for (int a = tid; a < n; a += 256) {
        const int lab = labels[fa + a];
        // ---- sigmoid focal loss: with z = -x for a positive and x for a negative, 1 - p_t = sigmoid(z) and the cross entropy is
        // softplus(z); d/dz [alpha sig^2 softplus] = alpha sig^2 (2 (1 - sig) softplus + sig).  Everything is built from
        // e = exp(-|z|) <= 1: no overflow, and neither sig nor 1 - sig is formed by a subtraction.
        float gc = 0.f;
        if (lab >= 0) {
            const bool pos = lab > 0;
            const double x = (double)cls[fa + a];
            const double z = pos ? -x : x;
            const double e = exp(-fabs(z));
            const double r = 1.0 / (1.0 + e);
            const double sig = z >= 0.0 ? r : e * r, om = z >= 0.0 ? e * r : r;
            const double sp = fmax(z, 0.0) + log1p(e);
            const double g = (pos ? FOCAL_ALPHA : 1.0 - FOCAL_ALPHA) * sig * sig * (2.0 * om * sp + sig);
            gc = (float)((pos ? -g : g) * wc);
        }
        dcls[fa + a] = gc;
        float* b = sb + a * 7;
        const float* t = st + a * 7;
        float2 gd = make_float2(0.f, 0.f);
        if (lab > 0) {
            // ---- smooth L1 (sigma 3): 9 d inside |d| <= 1/9, sign(d) outside; code 6 is the sin difference, d/db = cos(b - t)
            double sb6, cb6, st6, ct6;
            sincos((double)b[6], &sb6, &cb6);
            sincos((double)t[6], &st6, &ct6);
            for (int k = 0; k < 7; ++k) {
                const double d = k < 6 ? (double)b[k] - (double)t[k] : sb6 * ct6 - cb6 * st6;
                const double inner = k < 6 ? 1.0 : cb6 * ct6 + sb6 * st6;
                const double g = fabs(d) <= 1.0 / SL1_SIGMA2 ? SL1_SIGMA2 * d : (d > 0.0 ? 1.0 : -1.0);
                b[k] = (float)(g * inner * wb);
            }
            // ---- 2-way softmax cross entropy: softmax - onehot; the probability of the OTHER class is formed directly
            const float2 l = reinterpret_cast<const float2*>(dir)[fa + a];
            const double dd = (double)l.y - (double)l.x;
            const double e = exp(-fabs(dd));
            const double r = 1.0 / (1.0 + e);
            const double p1 = dd >= 0.0 ? r : e * r, p0 = dd >= 0.0 ? e * r : r;
            const float g0 = (float)((dirt[fa + a] > 0 ? p0 : -p1) * wd);
            gd = make_float2(g0, -g0);
        } else {
            for (int k = 0; k < 7; ++k) b[k] = 0.f;
        }
        reinterpret_cast<float2*>(ddir)[fa + a] = gd;
    }
    __syncthreads();
    if (vec) {
        for (int i = tid; i < n * 7 / 4; i += 256) reinterpret_cast<float4*>(po)[i] = reinterpret_cast<const float4*>(sb)[i];
    } else {
        for (int i = tid; i < n * 7; i += 256) po[i] = sb[i];
    }
}

// ------------------------------------------------------------------------------------------
// head backward
// ------------------------------------------------------------------------------------------
// Both kernels walk a frame's pixels in tiles of 64 and bring the tile's dY from the head's output layout -- cls [na][P],
// box [na][P][7], dir [na][P][2], P = H W -- into a channel-major LDS tile dYs[row][pixel], rows in natural (state_dict) order:
// cls a | box na + 7 a + k | dir 8 na + 2 a + k.  Per anchor the box / dir codes of 64 consecutive pixels are ONE contiguous span
// (448 / 128 floats), read with 16-byte loads; the un-permutation happens in the LDS stores.  Rows 10 na .. 95 stay zero.
constexpr int HB_PX = 64;
constexpr int HB_ROWS = 96;
constexpr int HB_C = 320;

template <int LD>
__device__ __forceinline__ void load_dy_tile(float* __restrict__ dYs, const float* __restrict__ dcls, const float* __restrict__ dbox,
                                             const float* __restrict__ ddir, int na, int P, int p0, int np, bool full)
{
    const int tid = threadIdx.x;
    for (int i = tid; i < na * HB_PX; i += 256) {
        const int a = i >> 6, px = i & 63;
        dYs[a * LD + px] = px < np ? dcls[(size_t)a * P + p0 + px] : 0.f;
    }
    if (full) {
        for (int i = tid; i < na * (HB_PX * 7 / 4); i += 256) {
            const int a = i / (HB_PX * 7 / 4), q = i - a * (HB_PX * 7 / 4);
            const float4 v = reinterpret_cast<const float4*>(dbox + ((size_t)a * P + p0) * 7)[q];
            const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * q + j, px = e / 7, k = e - 7 * px;
                dYs[(na + 7 * a + k) * LD + px] = e4[j];
            }
        }
        for (int i = tid; i < na * (HB_PX * 2 / 4); i += 256) {
            const int a = i / (HB_PX * 2 / 4), q = i - a * (HB_PX * 2 / 4);
            const float4 v = reinterpret_cast<const float4*>(ddir + ((size_t)a * P + p0) * 2)[q];
            float* d0 = dYs + (8 * na + 2 * a) * LD + 2 * q;
            d0[0] = v.x; d0[LD] = v.y; d0[1] = v.z; d0[LD + 1] = v.w;
        }
    } else {
        for (int i = tid; i < na * HB_PX * 7; i += 256) {
            const int a = i / (HB_PX * 7), e = i - a * (HB_PX * 7), px = e / 7, k = e - 7 * px;
            dYs[(na + 7 * a + k) * LD + px] = px < np ? dbox[((size_t)a * P + p0) * 7 + e] : 0.f;
        }
        for (int i = tid; i < na * HB_PX * 2; i += 256) {
            const int a = i / (HB_PX * 2), e = i - a * (HB_PX * 2), px = e >> 1, k = e & 1;
            dYs[(8 * na + 2 * a + k) * LD + px] = px < np ? ddir[((size_t)a * P + p0) * 2 + e] : 0.f;
        }
    }
}

// dW[96 x 320] += dY[96 x 64] X[320 x 64]^T per tile on v_mfma_f32_16x16x4_f32.  Four waves, each owns 80 of the 320 channels and all
// 96 rows: 6 x 5 accumulator tiles (120 registers) that live across the workgroup's whole pixel range.  The sum over the pixel is
// order-free, so k-step s of pixel group g takes pixel 16 g + 4 (lane >> 4) + s: a lane's four k-steps are one 16-byte load of X
// straight from global memory (16 channels x 64 B per instruction) and one ds_read_b128 of dY.  A workgroup also sums its rows of dY
// (db).  Partials: part[workgroup][96 * 320 + 96].
constexpr int DW_LD = 68; // dYs row stride: 16 rows x 4-float columns fall into 64 different banks
constexpr size_t PART_STRIDE = (size_t)HB_ROWS * HB_C + HB_ROWS;

__global__ void __launch_bounds__(256, 2) k_head_dw(const float* __restrict__ X, const float* __restrict__ dcls, const float* __restrict__ dbox,
                                                    const float* __restrict__ ddir, int na, int P, int tiles_per_wg, int ntiles,
                                                    float* __restrict__ part, int vec)
{
    __shared__ __attribute__((aligned(16))) float dYs[HB_ROWS * DW_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y;
    const size_t A = (size_t)na * P;
    const float* Xf = X + (size_t)f * HB_C * P;
    dcls += f * A; dbox += f * A * 7; ddir += f * A * 2;
    f32x4 acc[6][5];
#pragma unroll
    for (int rb = 0; rb < 6; ++rb)
#pragma unroll
        for (int cb = 0; cb < 5; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    double dbacc = 0.0; // rows of dY are mostly of one sign: a float32 running sum of them measured +5e-8 relative off, one-sided
    for (int i = tid; i < HB_ROWS * DW_LD; i += 256) dYs[i] = 0.f;
    const int t0 = blockIdx.x * tiles_per_wg, t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
    for (int t = t0; t < t1; ++t) {
        const int p0 = t * HB_PX, np = P - p0 < HB_PX ? P - p0 : HB_PX;
        const bool full = vec && np == HB_PX;
        __syncthreads(); // the previous tile (or the zero fill) is done with
        load_dy_tile<DW_LD>(dYs, dcls, dbox, ddir, na, P, p0, np, full);
        __syncthreads();
        if (tid < HB_ROWS) {
            double s = 0.0;
            for (int px = 0; px < HB_PX; ++px) s += dYs[tid * DW_LD + px];
            dbacc += s;
        }
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {
            const int pg = 16 * g + 4 * q;
            float xb[5][4];
#pragma unroll
            for (int cb = 0; cb < 5; ++cb) {
                const float* px_ = Xf + (size_t)(80 * wave + 16 * cb + l16) * P + p0 + pg;
                if (full) {
                    const float4 v = *reinterpret_cast<const float4*>(px_);
                    xb[cb][0] = v.x; xb[cb][1] = v.y; xb[cb][2] = v.z; xb[cb][3] = v.w;
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) xb[cb][s] = pg + s < np ? px_[s] : 0.f;
                }
            }
            float ya[6][4];
#pragma unroll
            for (int rb = 0; rb < 6; ++rb) {
                const float4 v = *reinterpret_cast<const float4*>(&dYs[(16 * rb + l16) * DW_LD + pg]);
                ya[rb][0] = v.x; ya[rb][1] = v.y; ya[rb][2] = v.z; ya[rb][3] = v.w;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int rb = 0; rb < 6; ++rb)
#pragma unroll
                    for (int cb = 0; cb < 5; ++cb)
                        acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ya[rb][s], xb[cb][s], acc[rb][cb], 0, 0, 0);
        }
    }
    float* pw = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * PART_STRIDE;
#pragma unroll
    for (int rb = 0; rb < 6; ++rb)
#pragma unroll
        for (int cb = 0; cb < 5; ++cb)
#pragma unroll
            for (int i = 0; i < 4; ++i) pw[(size_t)(16 * rb + 4 * q + i) * HB_C + 80 * wave + 16 * cb + l16] = acc[rb][cb][i];
    if (tid < HB_ROWS) pw[(size_t)HB_ROWS * HB_C + tid] = (float)dbacc;
}

// partials -> dW / db in state_dict order (the natural row order IS state_dict order: cls rows, then box a * 7 + k, then dir a * 2 + k),
// summed over workgroups in index order: frame-major, pixel ranges ascending
// (rows: the padded row count the partials were written with, 96 or rows_padded(na))
__global__ void __launch_bounds__(256) k_head_dw_reduce(const float* __restrict__ part, int G, int na, int rows, float* __restrict__ dw_cls,
                                                        float* __restrict__ dw_box, float* __restrict__ dw_dir, float* __restrict__ db_cls,
                                                        float* __restrict__ db_box, float* __restrict__ db_dir)
{
    const int R = 10 * na;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= R * HB_C + R) return;
    const bool bias = i >= R * HB_C;
    const int r = bias ? i - R * HB_C : i / HB_C, c = bias ? 0 : i - r * HB_C;
    const float* p = part + (bias ? (size_t)rows * HB_C + r : (size_t)i);
    const size_t stride = (size_t)rows * (HB_C + 1);
    double s = 0.0; // up to ~512 partials, for db mostly of one sign: summed in double, rounded once
    for (int g = 0; g < G; ++g) s += (double)p[(size_t)g * stride];
    const int w = bias ? 1 : HB_C;
    float* dst = r < na ? (bias ? db_cls : dw_cls) + (size_t)r * w : r < 8 * na ? (bias ? db_box : dw_box) + (size_t)(r - na) * w
                                                                             : (bias ? db_dir : dw_dir) + (size_t)(r - 8 * na) * w;
    dst[c] = (float)s;
}

// dX[320 x 64] = W^T[320 x 96] dY[96 x 64] per tile.  Each wave keeps the W^T fragments of its 80 channels in registers (5 x 24
// k-steps, loaded once per workgroup from the natural-order copy) and streams the dY tile from LDS as the B operand.
constexpr int DX_LD = 80; // dYs row stride: 4 k rows x 16 pixels fall into 64 different banks

__global__ void __launch_bounds__(256, 2) k_head_dx(const float* __restrict__ Wn, const float* __restrict__ dcls, const float* __restrict__ dbox,
                                                    const float* __restrict__ ddir, int na, int P, int tiles_per_wg, int ntiles,
                                                    float* __restrict__ dX, int vec)
{
    __shared__ __attribute__((aligned(16))) float dYs[HB_ROWS * DX_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y;
    const size_t A = (size_t)na * P;
    float* dXf = dX + (size_t)f * HB_C * P;
    dcls += f * A; dbox += f * A * 7; ddir += f * A * 2;
    float wa[5][24];
#pragma unroll
    for (int cb = 0; cb < 5; ++cb)
#pragma unroll
        for (int s = 0; s < 24; ++s) wa[cb][s] = Wn[(size_t)(4 * s + q) * HB_C + 80 * wave + 16 * cb + l16];
    for (int i = tid; i < HB_ROWS * DX_LD; i += 256) dYs[i] = 0.f;
    const int t0 = blockIdx.x * tiles_per_wg, t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
    for (int t = t0; t < t1; ++t) {
        const int p0 = t * HB_PX, np = P - p0 < HB_PX ? P - p0 : HB_PX;
        __syncthreads();
        load_dy_tile<DX_LD>(dYs, dcls, dbox, ddir, na, P, p0, np, vec && np == HB_PX);
        __syncthreads();
#pragma unroll
        for (int cb = 0; cb < 5; ++cb) {
            f32x4 acc[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int s = 0; s < 24; ++s)
#pragma unroll
                for (int nt = 0; nt < 4; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[cb][s], dYs[(4 * s + q) * DX_LD + 16 * nt + l16], acc[nt], 0, 0, 0);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int px = 16 * nt + l16;
                    if (px < np) dXf[(size_t)(80 * wave + 16 * cb + 4 * q + i) * P + p0 + px] = acc[nt][i];
                }
        }
    }
}

// ------------------------------------------------------------------------------------------
// head backward, more than 96 rows (10 .. 24 anchors per location)
// ------------------------------------------------------------------------------------------
// The GEMM rows are 10 na rounded up to 16 (rows_padded).  Neither 96-row kernel's register plan stretches to them at two waves per
// SIMD (13 x 5 accumulator tiles, or 5 x 52 W^T fragments, are 260 registers), so each splits ONE dimension over the grid and keeps
// the plan of its 96-row form: k_head_dw_wide the rows, k_head_dx_wide the channels.  The split is the fastest-varying part of
// blockIdx.x, so the workgroups that read the same pixels are dispatched together and the re-read comes from the caches.

// load_dy_tile for a window of rows: rows [r0, r1) of the natural order go to dYs[(row - r0) * LD + pixel]; r1 <= 10 na.  The
// same two paths: 16-byte loads of an anchor's contiguous box / dir span for a full, aligned tile, single floats otherwise.  A span
// is read whole where only some of its rows fall in the window (at most two anchors of box and of dir per window).
template <int LD>
__device__ __forceinline__ void load_dy_rows(float* __restrict__ dYs, const float* __restrict__ dcls, const float* __restrict__ dbox,
                                             const float* __restrict__ ddir, int na, int P, int p0, int np, bool full, int r0, int r1)
{
    const int tid = threadIdx.x;
    const unsigned nr = (unsigned)(r1 - r0);
    // anchors whose cls / box / dir rows meet the window
    const int c0 = r0 < na ? r0 : na, c1 = r1 < na ? r1 : na;
    const int b0 = r0 > na ? ((r0 - na) / 7 < na ? (r0 - na) / 7 : na) : 0, b1 = r1 > na ? ((r1 - na + 6) / 7 < na ? (r1 - na + 6) / 7 : na) : 0;
    const int d0 = r0 > 8 * na ? (r0 - 8 * na) / 2 : 0, d1 = r1 > 8 * na ? (r1 - 8 * na + 1) / 2 : 0;
    for (int i = tid; i < (c1 - c0) * HB_PX; i += 256) {
        const int a = c0 + (i >> 6), px = i & 63;
        dYs[(a - r0) * LD + px] = px < np ? dcls[(size_t)a * P + p0 + px] : 0.f;
    }
    if (full) {
        for (int i = tid; i < (b1 - b0) * (HB_PX * 7 / 4); i += 256) {
            const int a = b0 + i / (HB_PX * 7 / 4), q = i - (a - b0) * (HB_PX * 7 / 4);
            const float4 v = reinterpret_cast<const float4*>(dbox + ((size_t)a * P + p0) * 7)[q];
            const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int e = 4 * q + j, px = e / 7, k = e - 7 * px;
                const unsigned row = (unsigned)(na + 7 * a + k - r0);
                if (row < nr) dYs[row * LD + px] = e4[j];
            }
        }
        for (int i = tid; i < (d1 - d0) * (HB_PX * 2 / 4); i += 256) {
            const int a = d0 + i / (HB_PX * 2 / 4), q = i - (a - d0) * (HB_PX * 2 / 4);
            const float4 v = reinterpret_cast<const float4*>(ddir + ((size_t)a * P + p0) * 2)[q];
            const unsigned row = (unsigned)(8 * na + 2 * a - r0);
            if (row < nr) { dYs[row * LD + 2 * q] = v.x; dYs[row * LD + 2 * q + 1] = v.z; }
            if (row + 1 < nr) { dYs[(row + 1) * LD + 2 * q] = v.y; dYs[(row + 1) * LD + 2 * q + 1] = v.w; }
        }
    } else {
        for (int i = tid; i < (b1 - b0) * HB_PX * 7; i += 256) {
            const int a = b0 + i / (HB_PX * 7), e = i - (a - b0) * (HB_PX * 7), px = e / 7, k = e - 7 * px;
            const unsigned row = (unsigned)(na + 7 * a + k - r0);
            if (row < nr) dYs[row * LD + px] = px < np ? dbox[((size_t)a * P + p0) * 7 + e] : 0.f;
        }
        for (int i = tid; i < (d1 - d0) * HB_PX * 2; i += 256) {
            const int a = d0 + i / (HB_PX * 2), e = i - (a - d0) * (HB_PX * 2), px = e >> 1, k = e & 1;
            const unsigned row = (unsigned)(8 * na + 2 * a + k - r0);
            if (row < nr) dYs[row * LD + px] = px < np ? ddir[((size_t)a * P + p0) * 2 + e] : 0.f;
        }
    }
}

// k_head_dw with the rows split into nrb = ceil(tiles / 6) blocks of row tiles, as evenly as they go (13 tiles: 5 | 4 | 4): a
// workgroup owns one block of one pixel range, brings only that block's rows of dY into LDS and reads the range's X again.  The
// accumulators are the 6 x 5 tiles of k_head_dw; a block with fewer row tiles skips the others (wave-uniform), so the MFMAs executed
// are those of the padded row count.  Partials: part[frame][pixel range][rows * 320 + rows], every block writing its own rows; rows
// 10 na .. rows - 1 are zero in LDS and k_head_dw_reduce never reads what they give.
__global__ void __launch_bounds__(256, 2) k_head_dw_wide(const float* __restrict__ X, const float* __restrict__ dcls, const float* __restrict__ dbox,
                                                         const float* __restrict__ ddir, int na, int P, int tiles_per_wg, int ntiles, int nrb,
                                                         int rows, float* __restrict__ part, int vec)
{
    __shared__ __attribute__((aligned(16))) float dYs[HB_ROWS * DW_LD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y, rbk = blockIdx.x % nrb, range = blockIdx.x / nrb, nranges = gridDim.x / nrb;
    const int base = (rows / 16) / nrb, rem = (rows / 16) % nrb;
    const int nrt = base + (rbk < rem), r0 = 16 * (rbk * base + (rbk < rem ? rbk : rem)); // nrt <= 6 row tiles from row r0
    const int r1 = r0 + 16 * nrt < 10 * na ? r0 + 16 * nrt : 10 * na;
    const size_t A = (size_t)na * P;
    const float* Xf = X + (size_t)f * HB_C * P;
    dcls += f * A; dbox += f * A * 7; ddir += f * A * 2;
    f32x4 acc[6][5];
#pragma unroll
    for (int rb = 0; rb < 6; ++rb)
#pragma unroll
        for (int cb = 0; cb < 5; ++cb) acc[rb][cb] = f32x4{0.f, 0.f, 0.f, 0.f};
    double dbacc = 0.0;
    for (int i = tid; i < HB_ROWS * DW_LD; i += 256) dYs[i] = 0.f;
    const int t0 = range * tiles_per_wg, t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
    for (int t = t0; t < t1; ++t) {
        const int p0 = t * HB_PX, np = P - p0 < HB_PX ? P - p0 : HB_PX;
        const bool full = vec && np == HB_PX;
        __syncthreads();
        load_dy_rows<DW_LD>(dYs, dcls, dbox, ddir, na, P, p0, np, full, r0, r1);
        __syncthreads();
        if (tid < 16 * nrt) {
            double s = 0.0;
            for (int px = 0; px < HB_PX; ++px) s += dYs[tid * DW_LD + px];
            dbacc += s;
        }
#pragma unroll 1
        for (int g = 0; g < 4; ++g) {
            const int pg = 16 * g + 4 * q;
            float xb[5][4];
#pragma unroll
            for (int cb = 0; cb < 5; ++cb) {
                const float* px_ = Xf + (size_t)(80 * wave + 16 * cb + l16) * P + p0 + pg;
                if (full) {
                    const float4 v = *reinterpret_cast<const float4*>(px_);
                    xb[cb][0] = v.x; xb[cb][1] = v.y; xb[cb][2] = v.z; xb[cb][3] = v.w;
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) xb[cb][s] = pg + s < np ? px_[s] : 0.f;
                }
            }
#pragma unroll
            for (int rb = 0; rb < 6; ++rb) {
                if (rb < nrt) {
                    const float4 v = *reinterpret_cast<const float4*>(&dYs[(16 * rb + l16) * DW_LD + pg]);
                    const float ya[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int cb = 0; cb < 5; ++cb)
                            acc[rb][cb] = __builtin_amdgcn_mfma_f32_16x16x4f32(ya[s], xb[cb][s], acc[rb][cb], 0, 0, 0);
                }
            }
        }
    }
    float* pw = part + ((size_t)f * nranges + range) * ((size_t)rows * (HB_C + 1));
#pragma unroll
    for (int rb = 0; rb < 6; ++rb)
        if (rb < nrt)
#pragma unroll
            for (int cb = 0; cb < 5; ++cb)
#pragma unroll
                for (int i = 0; i < 4; ++i) pw[(size_t)(r0 + 16 * rb + 4 * q + i) * HB_C + 80 * wave + 16 * cb + l16] = acc[rb][cb][i];
    if (tid < 16 * nrt) pw[(size_t)rows * HB_C + r0 + tid] = (float)dbacc;
}

// k_head_dx with the 320 channels split over DXW_GROUPS workgroups per pixel range: a wave keeps the W^T fragments of two 16-channel
// blocks for every row (2 x rows / 4 <= 120 registers, loaded once per workgroup), the whole dY tile [rows][64] sits in LDS (dynamic,
// rows * DX_LD floats: 77 KB at 24 anchors) and is brought in once per group.  Twenty channel blocks over 3 x 4 x 2 slots: the last
// group's waves 2 and 3 have none and only help to load the tile.
constexpr int DXW_CB = 2;                                          // 16-channel blocks per wave
constexpr int DXW_GROUPS = (HB_C / 16 + 4 * DXW_CB - 1) / (4 * DXW_CB);
constexpr int DXW_KB = (10 * HB_MAX_NA + 15) / 16;                 // blocks of 16 rows (four k-steps) at the cap

__global__ void __launch_bounds__(256, 2) k_head_dx_wide(const float* __restrict__ Wn, const float* __restrict__ dcls, const float* __restrict__ dbox,
                                                         const float* __restrict__ ddir, int na, int P, int tiles_per_wg, int ntiles, int rows,
                                                         float* __restrict__ dX, int vec)
{
    extern __shared__ __attribute__((aligned(16))) float dYw[]; // [rows][DX_LD]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int f = blockIdx.y, grp = blockIdx.x % DXW_GROUPS, range = blockIdx.x / DXW_GROUPS;
    const int nkb = rows / 16, cb0 = 4 * DXW_CB * grp + DXW_CB * wave; // this wave's channel blocks: cb0 + j where that is < 20
    const size_t A = (size_t)na * P;
    float* dXf = dX + (size_t)f * HB_C * P;
    dcls += f * A; dbox += f * A * 7; ddir += f * A * 2;
    float wa[DXW_CB][DXW_KB][4];
#pragma unroll
    for (int j = 0; j < DXW_CB; ++j)
#pragma unroll
        for (int kb = 0; kb < DXW_KB; ++kb)
#pragma unroll
            for (int s = 0; s < 4; ++s)
                wa[j][kb][s] = kb < nkb && cb0 + j < HB_C / 16 ? Wn[(size_t)(16 * kb + 4 * s + q) * HB_C + 16 * (cb0 + j) + l16] : 0.f;
    for (int i = tid; i < rows * DX_LD; i += 256) dYw[i] = 0.f;
    const int t0 = range * tiles_per_wg, t1 = t0 + tiles_per_wg < ntiles ? t0 + tiles_per_wg : ntiles;
    for (int t = t0; t < t1; ++t) {
        const int p0 = t * HB_PX, np = P - p0 < HB_PX ? P - p0 : HB_PX;
        __syncthreads();
        load_dy_rows<DX_LD>(dYw, dcls, dbox, ddir, na, P, p0, np, vec && np == HB_PX, 0, 10 * na);
        __syncthreads();
#pragma unroll
        for (int j = 0; j < DXW_CB; ++j) {
            if (cb0 + j >= HB_C / 16) continue;
            f32x4 acc[4];
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) acc[nt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kb = 0; kb < DXW_KB; ++kb) {
                if (kb < nkb) {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int nt = 0; nt < 4; ++nt)
                            acc[nt] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[j][kb][s], dYw[(16 * kb + 4 * s + q) * DX_LD + 16 * nt + l16], acc[nt], 0,
                                                                           0, 0);
                }
            }
#pragma unroll
            for (int nt = 0; nt < 4; ++nt)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int px = 16 * nt + l16;
                    if (px < np) dXf[(size_t)(16 * (cb0 + j) + 4 * q + i) * P + p0 + px] = acc[nt][i];
                }
        }
    }
}

// ------------------------------------------------------------------------------------------
// in-place rewrite of the head's packed image
// ------------------------------------------------------------------------------------------
// dst[i] = element map[i] of the concatenation src0 | src1 | src2 (n0, n1 elements in the first two), 0 where map[i] < 0
__global__ void __launch_bounds__(256) k_gather3(float* __restrict__ dst, const int32_t* __restrict__ map, int n, const float* __restrict__ s0,
                                                 const float* __restrict__ s1, const float* __restrict__ s2, int n0, int n1, int n2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int m = map[i];
    dst[i] = m < 0 || m >= n0 + n1 + n2 ? 0.f : m < n0 ? s0[m] : m < n0 + n1 ? s1[m - n0] : s2[m - n0 - n1];
}

int upload_map(pp_ctx* ctx, const std::vector<int32_t>& h, int32_t** d)
{
    if (*d) { (void)hipFree(*d); *d = nullptr; }
    if (h.empty()) return 0;
    PP_HIP(hipMalloc((void**)d, h.size() * sizeof(int32_t)));
    PP_HIP(hipMemcpy(*d, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    return 0;
}

// natural-order copy of the committed head weights for the dX product (synchronous, once per commit)
int refresh_w_nat(pp_ctx* ctx, trn_ws* w)
{
    if (w->w_gen == ctx->commit_gen) return 0;
    const int na = ctx->cfg.num_anchor_per_loc;
    const char* names[3] = {"heads.conv_cls.weight", "heads.conv_box.weight", "heads.conv_dir.weight"};
    const int cnt[3] = {na, 7 * na, 2 * na};
    std::vector<float> h((size_t)rows_padded(na) * HB_C, 0.f);
    size_t r0 = 0;
    for (int k = 0; k < 3; ++k) {
        auto it = ctx->host_w.find(names[k]);
        if (it == ctx->host_w.end() || it->second.data.size() != (size_t)cnt[k] * HB_C) return pp_fail(ctx, PP_E_NAME, "head weights missing or mis-shaped");
        std::memcpy(&h[r0 * HB_C], it->second.data.data(), sizeof(float) * cnt[k] * HB_C);
        r0 += cnt[k];
    }
    PP_HIP(hipMemcpy(w->w_nat, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    w->w_gen = ctx->commit_gen;
    return 0;
}

// pixel ranges of pp_head_backward: about 512 workgroups in all (two per CU), at least 16 and at most 128 per frame, so that the
// dW partials (123 KB each) stay at 4 - 30 % of the bytes of X they summarise (51 MB per frame on eight_20cm)
void pixel_ranges(int nb, int ntiles, int* wgs, int* tiles_per_wg)
{
    int per = (512 + nb - 1) / nb;
    per = per < 16 ? 16 : per > 128 ? 128 : per;
    if (per > ntiles) per = ntiles;
    *tiles_per_wg = (ntiles + per - 1) / per;
    *wgs = (ntiles + *tiles_per_wg - 1) / *tiles_per_wg;
}

} // namespace

void pp_train_destroy(pp_ctx* ctx)
{
    trn_ws* w = (trn_ws*)ctx->trn;
    if (!w) return;
    void* q[] = {w->npos, w->w_nat, w->part, w->wmap, w->bmap, w->bpmap};
    for (void* x : q)
        if (x) (void)hipFree(x);
    delete w;
    ctx->trn = nullptr;
}

extern "C" int pp_target_loss_grad(pp_ctx* ctx, const float* cls, const float* box, const float* dir, const int32_t* labels,
                                   const float* bbox_targets, const int32_t* dir_targets, int nb, int batch_div, float grad_scale,
                                   float* dcls, float* dbox, float* ddir, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!cls || !box || !dir || !labels || !bbox_targets || !dir_targets || !dcls || !dbox || !ddir)
        return pp_fail(ctx, PP_E_ARG, "pp_target_loss_grad: null pointer");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_target_loss_grad: nb must be 1 .. max_batch");
    if (batch_div < nb) return pp_fail(ctx, PP_E_ARG, "pp_target_loss_grad: batch_div must be at least nb");
    if (ctx->A <= 0) return pp_fail(ctx, PP_E_STATE, "pp_target_loss_grad: anchors not set");
    if (((uintptr_t)dir | (uintptr_t)ddir) & 7) return pp_fail(ctx, PP_E_ARG, "pp_target_loss_grad: dir and ddir must be 8-byte aligned");
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    trn_ws* w = workspace(ctx);
    if (!w) return pp_fail(ctx, PP_E_STATE, "pp_target_loss_grad: workspace allocation failed");
    const int64_t A = ctx->A;
    PP_HIP(hipMemsetAsync(w->npos, 0, (size_t)nb * sizeof(int32_t), stream));
    const int cb = pp_div_up(A, 256) < 64 ? pp_div_up(A, 256) : 64;
    hipLaunchKernelGGL(k_count_pos, dim3(cb, nb), dim3(256), 0, stream, labels, A, w->npos);
    const double s = (double)grad_scale / (double)batch_div;
    const int vec = A % 4 == 0 && aligned16(box) && aligned16(bbox_targets) && aligned16(dbox);
    hipLaunchKernelGGL(k_loss_grad, dim3(pp_div_up(A, LG_ANCH), nb), dim3(256), 0, stream, cls, box, dir, labels, bbox_targets, dir_targets,
                       w->npos, A, s * CLS_WEIGHT, s * LOC_WEIGHT, s * DIR_WEIGHT, dcls, dbox, ddir, vec);
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_head_backward(pp_ctx* ctx, const float* rpn_out, const float* dcls, const float* dbox, const float* ddir, int nb,
                                float* dw_cls, float* dw_box, float* dw_dir, float* db_cls, float* db_box, float* db_dir, float* dx,
                                void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_head_backward: weights not committed");
    if (!rpn_out || !dcls || !dbox || !ddir || !dw_cls || !dw_box || !dw_dir || !db_cls || !db_box || !db_dir)
        return pp_fail(ctx, PP_E_ARG, "pp_head_backward: null pointer");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_head_backward: nb must be 1 .. max_batch");
    const int na = ctx->cfg.num_anchor_per_loc, P = ctx->H * ctx->W;
    if (na > HB_MAX_NA) return pp_fail(ctx, PP_E_ARG, "pp_head_backward: more than 24 anchors per location");
    const bool wide = 10 * na > HB_ROWS;
    const int rows = rows_padded(na);
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    trn_ws* w = workspace(ctx);
    if (!w) return pp_fail(ctx, PP_E_STATE, "pp_head_backward: workspace allocation failed");
    const int ntiles = pp_div_up(P, HB_PX);
    int wgs = 0, tpw = 0;
    pixel_ranges(nb, ntiles, &wgs, &tpw);
    const size_t need = (size_t)nb * wgs * rows * (HB_C + 1); // PART_STRIDE of either dW kernel
    if (need > w->part_elems) {
        PP_HIP(hipStreamSynchronize(stream)); // a running reduce may still read the old buffer
        if (w->part) (void)hipFree(w->part);
        w->part = nullptr; w->part_elems = 0;
        PP_HIP(hipMalloc((void**)&w->part, need * sizeof(float)));
        w->part_elems = need;
    }
    const int vec = P % 4 == 0 && aligned16(rpn_out) && aligned16(dbox) && aligned16(ddir);
    if (wide) {
        const int nrb = pp_div_up(rows / 16, 6); // row blocks of at most six 16-row tiles
        hipLaunchKernelGGL(k_head_dw_wide, dim3(wgs * nrb, nb), dim3(256), 0, stream, rpn_out, dcls, dbox, ddir, na, P, tpw, ntiles, nrb, rows,
                           w->part, vec);
    } else {
        hipLaunchKernelGGL(k_head_dw, dim3(wgs, nb), dim3(256), 0, stream, rpn_out, dcls, dbox, ddir, na, P, tpw, ntiles, w->part, vec);
    }
    hipLaunchKernelGGL(k_head_dw_reduce, dim3(pp_div_up(10 * na * (HB_C + 1), 256)), dim3(256), 0, stream, w->part, nb * wgs, na, rows, dw_cls,
                       dw_box, dw_dir, db_cls, db_box, db_dir);
    if (dx) {
        int rc = refresh_w_nat(ctx, w);
        if (rc) return rc;
        if (wide) {
            const size_t lds = (size_t)rows * DX_LD * sizeof(float);
            if (!w->dx_wide_lds) { // the attribute belongs to the device, not to this context: the size at the cap serves every context
                PP_HIP(hipFuncSetAttribute((const void*)k_head_dx_wide, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)(16 * DXW_KB * DX_LD * sizeof(float))));
                w->dx_wide_lds = true;
            }
            hipLaunchKernelGGL(k_head_dx_wide, dim3(wgs * DXW_GROUPS, nb), dim3(256), lds, stream, w->w_nat, dcls, dbox, ddir, na, P, tpw, ntiles,
                               rows, dx, vec);
        } else {
            hipLaunchKernelGGL(k_head_dx, dim3(wgs, nb), dim3(256), 0, stream, w->w_nat, dcls, dbox, ddir, na, P, tpw, ntiles, dx, vec);
        }
    }
    PP_HIP(hipGetLastError());
    return 0;
}

namespace {
// mode 0: pp_update_head_weights (an fp32 plan); 1 | 2 | 3: the _mp entry for a plan committed in that 16-bit mode.  There the weight
// image goes through k_image16 (image16.hip) when the head runs a 16-bit tiling and through k_gather3 when it keeps an fp32 one; the
// bias stays fp32 in every mode, in natural order and, where the plan has that copy, in head_tile_row order.
int head_update(pp_ctx* ctx, const char* who_, int mode, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box,
                const float* w_dir, const float* b_dir, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    const std::string who(who_);
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_ARG, (who + ": no committed weights to update (pp_commit_weights first)").c_str());
    if (!w_cls || !b_cls || !w_box || !b_box || !w_dir || !b_dir) return pp_fail(ctx, PP_E_ARG, (who + ": null pointer").c_str());
    if (mode == 0 && pp_effective_precision(ctx) != 0) // (the map below may be the _mp entry's: its own refusal would not be reached)
        return pp_fail(ctx, PP_E_ARG, "head weights can be rewritten in place in the fp32 mode only (the committed plan packs the head in a 16-bit format)");
    if (mode != 0)
        if (int rc = pp_mp_mode_check(ctx, who_, mode)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    trn_ws* w = workspace(ctx);
    if (!w) return pp_fail(ctx, PP_E_STATE, (who + ": workspace allocation failed").c_str());
    if (int rc0 = pp_head_materialise(ctx, stream)) return rc0; // the last deferred pass gets its full tensors from the weights it ran with
    const int na = ctx->cfg.num_anchor_per_loc;
    bool is16 = false;
    if (mode != 0)
        if (int rc = pp_update_image16(ctx, pp_net_layer_index(ctx, 2, 0), w_cls, w_box, w_dir, na * HB_C, 7 * na * HB_C, 2 * na * HB_C, stream, &is16))
            return rc;
    if (w->img_gen != ctx->commit_gen) { // first update after a commit: read the committed image's layout back (synchronous)
        int rc = 0;
        if (is16) { // the biases alone: their maps do not depend on the tiling
            w->img.wmap.clear();
            w->img.w = nullptr;
            rc = pp_net_head_bias(ctx, &w->img);
        } else {
            rc = pp_net_head_image(ctx, &w->img, mode != 0);
        }
        if (rc) return rc;
        if ((rc = upload_map(ctx, w->img.wmap, &w->wmap)) || (rc = upload_map(ctx, w->img.bmap, &w->bmap)) ||
            (rc = upload_map(ctx, w->img.bpmap, &w->bpmap)))
            return rc;
        w->img_gen = ctx->commit_gen;
    }
    const int nw = (int)w->img.wmap.size(), nbm = (int)w->img.bmap.size(), nbp = (int)w->img.bpmap.size();
    if (nw)
        hipLaunchKernelGGL(k_gather3, dim3(pp_div_up(nw, 256)), dim3(256), 0, stream, w->img.w, w->wmap, nw, w_cls, w_box, w_dir, na * HB_C,
                           7 * na * HB_C, 2 * na * HB_C);
    hipLaunchKernelGGL(k_gather3, dim3(pp_div_up(nbm, 256)), dim3(256), 0, stream, w->img.bias, w->bmap, nbm, b_cls, b_box, b_dir, na, 7 * na,
                       2 * na);
    if (nbp)
        hipLaunchKernelGGL(k_gather3, dim3(pp_div_up(nbp, 256)), dim3(256), 0, stream, w->img.bias_perm, w->bpmap, nbp, b_cls, b_box, b_dir, na,
                           7 * na, 2 * na);
    // the natural-order copy pp_head_backward's dX product reads
    if (w->w_gen != ctx->commit_gen) {
        PP_HIP(hipMemsetAsync(w->w_nat, 0, (size_t)rows_padded(na) * HB_C * sizeof(float), stream));
        w->w_gen = ctx->commit_gen;
    }
    PP_HIP(hipMemcpyAsync(w->w_nat, w_cls, (size_t)na * HB_C * 4, hipMemcpyDeviceToDevice, stream));
    PP_HIP(hipMemcpyAsync(w->w_nat + (size_t)na * HB_C, w_box, (size_t)7 * na * HB_C * 4, hipMemcpyDeviceToDevice, stream));
    PP_HIP(hipMemcpyAsync(w->w_nat + (size_t)8 * na * HB_C, w_dir, (size_t)2 * na * HB_C * 4, hipMemcpyDeviceToDevice, stream));
    PP_HIP(hipGetLastError());
    return 0;
}
} // namespace

extern "C" int pp_update_head_weights(pp_ctx* ctx, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box,
                                      const float* w_dir, const float* b_dir, void* stream_)
{
    return head_update(ctx, "pp_update_head_weights", 0, w_cls, b_cls, w_box, b_box, w_dir, b_dir, stream_);
}

extern "C" int pp_update_head_weights_mp(pp_ctx* ctx, int mode, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box,
                                         const float* w_dir, const float* b_dir, void* stream_)
{
    return head_update(ctx, "pp_update_head_weights_mp", mode, w_cls, b_cls, w_box, b_box, w_dir, b_dir, stream_);
}
