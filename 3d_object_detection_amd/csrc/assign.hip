// Training-target side: anchor target assignment (framework/anchor_assigner.py:337-457 of the reference, box_np_ops.py:308-382),
// the NormByNumPositives detection loss (loss_generator.py:26-253) and the metric counts (metrics.py:14-69).
//   G1  ground-truth prep: near BEV box (rbbox2d_to_near_bbox, r' = |limit_period(r, 0.5, pi)| > pi/4 swaps l/w) + area,
//       per-box maximum reset.  One thread per box row.
//   G2  per-box maximum over the INSIDE anchors of the box's class: one thread per anchor, dense over the frame's boxes; a
//       wave max per box, then one 32-bit atomicMax of the float bits (IoU >= 0, so its bits order like unsigned integers:
//       the result is independent of the order the waves arrive in).
//   G3  per anchor: max / argmax over the class's boxes (strict >, first box wins like numpy argmax), the forced set
//       (IoU == that box's maximum, every tie; a box with maximum 0 matches nothing), the label rule, box_encode, direction
//       target.  Writes the reference's four arrays (pp_assign_targets) or feeds the loss terms straight into the reduction
//       of L1 (pp_batch_loss: no [A,7] target tensor is materialised).
//   L1  per anchor fp32 loss terms (focal / smooth-L1 with the sin difference / 2-way softmax CE) exactly as the torch
//       expressions order them, accumulated in fp64 per thread over a fixed anchor stride, reduced per block in a fixed
//       tree -> per-(frame, block) partials.  No float atomics: two runs are bit-identical.
//   L2  one block per frame sums the partials in a fixed tree and divides the four loss sums by max(npos, 1).
// Every IoU step is one float32 operation (the library builds with -ffp-contract=off), as in iou_jit with eps = 0.
#include <cstring>
#include <vector>
#include "pp_common.h"

namespace {

constexpr int ASG_GROUP = 64;       // frames per launch (kernel-argument table)
constexpr int LOSS_BLOCKS = 256;    // blocks per frame of L1 = partials per frame reduced by L2
constexpr int LOSS_THREADS = 256;
constexpr float PI_F = 3.14159265358979323846f;
constexpr float PI4_F = 0.78539816339744830962f; // np.pi / 4 compared with a float32 array: rounded to float32
constexpr float MATCHED_DEFAULT = 0.6f, UNMATCHED_DEFAULT = 0.45f;

struct asg_ws {
    float4* gbv = nullptr;     // [PP_ASSIGN_MAX_GT] near box (x0, y0, x1, y1)
    float* garea = nullptr;    // [PP_ASSIGN_MAX_GT]
    uint32_t* gmax = nullptr;  // [PP_ASSIGN_MAX_GT] float bits of the per-box maximum over inside anchors
    double* part = nullptr;    // [max_batch][LOSS_BLOCKS][PP_LOSS_TERMS]
};

struct asg_args {
    int32_t off[ASG_GROUP + 1];     // absolute ground-truth rows of the group's frames: frame z owns off[z] .. off[z+1]-1
    int32_t cb[PP_MAX_CLASSES], ce[PP_MAX_CLASSES];
    float thr_m[PP_MAX_CLASSES], thr_u[PP_MAX_CLASSES];
    int32_t nc;
    int32_t f0;                     // first frame of the group (frame-strided pointers)
};

__device__ __forceinline__ int anchor_class(const asg_args& p, int64_t a)
{
    for (int c = 0; c < p.nc; ++c)
        if (a >= p.cb[c] && a < p.ce[c]) return c;
    return -1;
}

// rbbox2d_to_near_bbox of one (x, y, l, w, r) row, float32 numpy order
__device__ __forceinline__ float4 near_box(float x, float y, float l, float w, float r)
{
    const float lp = fabsf(r - floorf(r / PI_F + 0.5f) * PI_F);
    const bool sw = lp > PI4_F;
    const float dx = sw ? w : l, dy = sw ? l : w;
    const float hx = dx / 2.f, hy = dy / 2.f;
    return make_float4(x - hx, y - hy, x + hx, y + hy);
}

__device__ __forceinline__ float box_area(float4 b) { return (b.z - b.x) * (b.w - b.y); }

// iou_jit (box_np_ops.py:335-363), eps = 0: anchor a (boxes), ground truth g (query_boxes)
__device__ __forceinline__ float iou_f32(float4 a, float aa, float4 g, float ga)
{
    const float iw = fminf(a.z, g.z) - fmaxf(a.x, g.x);
    if (iw > 0.f) {
        const float ih = fminf(a.w, g.w) - fmaxf(a.y, g.y);
        if (ih > 0.f) {
            const float inter = iw * ih;
            const float ua = (aa + ga) - inter;
            return inter / ua;
        }
    }
    return 0.f;
}

__global__ void __launch_bounds__(64) k_gt_prep(const float* __restrict__ gt, int G, float4* __restrict__ gbv, float* __restrict__ garea,
                                                uint32_t* __restrict__ gmax)
{
    const int g = blockIdx.x * 64 + threadIdx.x;
    if (g >= G) return;
    const float* b = gt + (size_t)g * 7;
    const float4 bv = near_box(b[0], b[1], b[3], b[4], b[6]);
    gbv[g] = bv;
    garea[g] = box_area(bv);
    gmax[g] = 0u;
}

__global__ void __launch_bounds__(256) k_gmax(asg_args p, const uint8_t* __restrict__ mask, int64_t A, const float* __restrict__ anchors,
                                              const int32_t* __restrict__ gt_cls, const float4* __restrict__ gbv,
                                              const float* __restrict__ garea, uint32_t* __restrict__ gmax)
{
    const int z = blockIdx.y;
    const int g0 = p.off[z], g1 = p.off[z + 1];
    if (g0 == g1) return; // uniform over the block
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int c = -1;
    float4 abv = make_float4(0.f, 0.f, 0.f, 0.f);
    float aa = 0.f;
    if (a < A && mask[(size_t)(p.f0 + z) * A + a]) {
        c = anchor_class(p, a);
        const float* an = anchors + a * 7;
        abv = near_box(an[0], an[1], an[3], an[4], an[6]);
        aa = box_area(abv);
    }
    for (int g = g0; g < g1; ++g) {
        const float v = (c >= 0 && gt_cls[g] == c + 1) ? iou_f32(abv, aa, gbv[g], garea[g]) : 0.f;
        if (__ballot(v > 0.f) == 0) continue;
        float m = v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
        if ((threadIdx.x & 63) == 0) atomicMax(&gmax[g], __float_as_uint(m));
    }
}

struct anchor_target {
    int32_t label;
    int32_t dir;
    float t[7]; // bbox target (0 unless label 1)
};

// G3 body: label, target and direction target of anchor a of frame z (a < A)
__device__ __forceinline__ anchor_target assign_one(const asg_args& p, int z, int64_t a, int64_t A, const uint8_t* __restrict__ mask,
                                                    const float* __restrict__ anchors, const float* __restrict__ gt,
                                                    const int32_t* __restrict__ gt_cls, const float4* __restrict__ gbv,
                                                    const float* __restrict__ garea, const uint32_t* __restrict__ gmax)
{
    anchor_target r;
    r.label = -1;
#pragma unroll
    for (int k = 0; k < 7; ++k) r.t[k] = 0.f;
    const float* an = anchors + a * 7;
    const int c = anchor_class(p, a);
    if (c >= 0 && mask[(size_t)(p.f0 + z) * A + a]) {
        const float4 abv = near_box(an[0], an[1], an[3], an[4], an[6]);
        const float aa = box_area(abv);
        float best = -1.f;
        int arg = -1;
        bool forced = false;
        for (int g = p.off[z]; g < p.off[z + 1]; ++g) {
            if (gt_cls[g] != c + 1) continue;
            const float v = iou_f32(abv, aa, gbv[g], garea[g]);
            if (v > best) { best = v; arg = g; }
            const uint32_t gm = gmax[g];
            if (gm != 0u && v == __uint_as_float(gm)) forced = true; // gmax == 0 -> -1: matches nothing
        }
        // the reference's order (anchor_assigner.py:381-392): pos (>= matched) is overwritten by bg (< unmatched), forced re-applied last
        if (arg < 0) r.label = 0; // no box of this class: the reference's else branch
        else if (forced) r.label = 1;
        else if (best < p.thr_u[c]) r.label = 0;
        else if (best >= p.thr_m[c]) r.label = 1;
        if (r.label == 1) {
            // box_encode (box_np_ops.py:366-382), float32 numpy order
            const float* b = gt + (size_t)arg * 7;
            const float diag = sqrtf(an[3] * an[3] + an[4] * an[4]);
            r.t[0] = (b[0] - an[0]) / diag;
            r.t[1] = (b[1] - an[1]) / diag;
            r.t[2] = (b[2] - an[2]) / an[5];
            r.t[3] = logf(b[3] / an[3]);
            r.t[4] = logf(b[4] / an[4]);
            r.t[5] = logf(b[5] / an[5]);
            r.t[6] = b[6] - an[6];
        }
    }
    r.dir = (r.t[6] + an[6]) > 0.f ? 1 : 0; // get_direction_target over every anchor of the range
    return r;
}

__global__ void __launch_bounds__(256) k_assign(asg_args p, const uint8_t* __restrict__ mask, int64_t A, const float* __restrict__ anchors,
                                                const float* __restrict__ gt, const int32_t* __restrict__ gt_cls,
                                                const float4* __restrict__ gbv, const float* __restrict__ garea,
                                                const uint32_t* __restrict__ gmax, int32_t* __restrict__ labels, float* __restrict__ tgt,
                                                float* __restrict__ outside_w, int32_t* __restrict__ dirt)
{
    const int z = blockIdx.y;
    const int64_t a = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (a >= A) return;
    const anchor_target r = assign_one(p, z, a, A, mask, anchors, gt, gt_cls, gbv, garea, gmax);
    const size_t i = (size_t)(p.f0 + z) * A + a;
    labels[i] = r.label;
    outside_w[i] = r.label > 0 ? 1.f : 0.f;
    dirt[i] = r.dir;
    float* t = tgt + i * 7;
#pragma unroll
    for (int k = 0; k < 7; ++k) t[k] = r.t[k];
}

// ---- loss -------------------------------------------------------------------------------------------------------------------
struct loss_acc {
    double loc = 0.0, cpos = 0.0, cneg = 0.0, dir = 0.0;
    int npos = 0;
    int cnt[16] = {};
};

__device__ __forceinline__ float sigmoid_f32(float x) { return 1.f / (1.f + expf(-x)); }

// one anchor's fp32 terms, in the order of the torch expressions of loss_generator.py / metrics.py
__device__ __forceinline__ void loss_one(loss_acc& s, int32_t lab, const float* __restrict__ t, int32_t dt, float x,
                                         const float* __restrict__ bp, const float* __restrict__ dp)
{
    if (lab < 0) return; // cls weight, reg weight, dir weight and metric weight are all 0
    const float tt = lab > 0 ? 1.f : 0.f;
    const float ce = (fmaxf(x, 0.f) - x * tt) + log1pf(expf(-fabsf(x)));
    const float pr = sigmoid_f32(x);
    const float pt = tt * pr + (1.f - tt) * (1.f - pr);
    const float om = 1.f - pt;
    const float alpha = tt * 0.25f + (1.f - tt) * 0.75f;
    const float focal = om * om * alpha * ce;
    const float th[4] = {0.1f, 0.3f, 0.5f, 0.7f};
    if (lab > 0) {
        s.cpos += (double)focal;
        ++s.npos;
    }
    if (lab > 0 && bp) {
        float l = 0.f;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const float d = k < 6 ? bp[k] - t[k] : sinf(bp[6]) * cosf(t[6]) - cosf(bp[6]) * sinf(t[6]);
            const float ad = fabsf(d);
            const float e = ad <= (1.f / 9.f) ? 0.5f * ((ad * 3.f) * (ad * 3.f)) : ad - 0.5f / 9.f;
            l += e;
        }
        s.loc += (double)l;
        const float m = fmaxf(dp[0], dp[1]);
        const float lse = m + logf(expf(dp[0] - m) + expf(dp[1] - m));
        s.dir += (double)(lse - dp[dt ? 1 : 0]);
    }
    if (lab > 0) {
#pragma unroll
        for (int i = 0; i < 4; ++i) ++s.cnt[4 * i + (pr > th[i] ? 0 : 3)]; // tp | fn
    } else {
        s.cneg += (double)focal;
#pragma unroll
        for (int i = 0; i < 4; ++i) ++s.cnt[4 * i + (pr > th[i] ? 2 : 1)]; // fp | tn
    }
}

// fixed-shape block reduction of one double (wave butterfly, then the 4 waves in order); result valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__device__ __forceinline__ void store_terms(const loss_acc& s, double* __restrict__ out)
{
    __shared__ double sh[4];
    double v[PP_LOSS_TERMS];
    v[0] = (double)s.npos; v[1] = s.loc; v[2] = s.cpos; v[3] = s.cneg; v[4] = s.dir;
#pragma unroll
    for (int k = 0; k < 16; ++k) v[5 + k] = (double)s.cnt[k];
#pragma unroll
    for (int k = 0; k < PP_LOSS_TERMS; ++k) {
        const double r = block_sum(v[k], sh);
        if (threadIdx.x == 0) out[k] = r;
    }
}

// L1 over stored targets (pp_target_loss)
__global__ void __launch_bounds__(LOSS_THREADS) k_loss_mem(int64_t A, int f0, const float* __restrict__ cls, const float* __restrict__ box,
                                                           const float* __restrict__ dir, const int32_t* __restrict__ labels,
                                                           const float* __restrict__ tgt, const int32_t* __restrict__ dirt, double* __restrict__ part)
{
    const size_t f = (size_t)(f0 + blockIdx.y);
    loss_acc s;
    for (int64_t a = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x; a < A; a += (int64_t)LOSS_BLOCKS * LOSS_THREADS) {
        const size_t i = f * A + a;
        if (box) loss_one(s, labels[i], tgt + i * 7, dirt[i], cls[i], box + i * 7, dir + i * 2);
        else loss_one(s, labels[i], nullptr, 0, cls[i], nullptr, nullptr); // counts only
    }
    store_terms(s, part + (f * LOSS_BLOCKS + blockIdx.x) * PP_LOSS_TERMS);
}

// L1 fused with G3 (pp_batch_loss): the same per-anchor terms in the same thread / block shape as k_loss_mem
__global__ void __launch_bounds__(LOSS_THREADS) k_loss_fused(asg_args p, const uint8_t* __restrict__ mask, int64_t A,
                                                             const float* __restrict__ anchors, const float* __restrict__ gt,
                                                             const int32_t* __restrict__ gt_cls, const float4* __restrict__ gbv,
                                                             const float* __restrict__ garea, const uint32_t* __restrict__ gmax,
                                                             const float* __restrict__ cls, const float* __restrict__ box,
                                                             const float* __restrict__ dir, double* __restrict__ part)
{
    const int z = blockIdx.y;
    const size_t f = (size_t)(p.f0 + z);
    loss_acc s;
    for (int64_t a = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x; a < A; a += (int64_t)LOSS_BLOCKS * LOSS_THREADS) {
        const anchor_target r = assign_one(p, z, a, A, mask, anchors, gt, gt_cls, gbv, garea, gmax);
        const size_t i = f * A + a;
        loss_one(s, r.label, r.t, r.dir, cls[i], box + i * 7, dir + i * 2);
    }
    store_terms(s, part + (f * LOSS_BLOCKS + blockIdx.x) * PP_LOSS_TERMS);
}

// L2: frame = blockIdx.x
__global__ void __launch_bounds__(LOSS_BLOCKS) k_loss_final(const double* __restrict__ part, double* __restrict__ terms)
{
    __shared__ double sh[4];
    const double* pf = part + (size_t)blockIdx.x * LOSS_BLOCKS * PP_LOSS_TERMS;
    double* out = terms + (size_t)blockIdx.x * PP_LOSS_TERMS;
    double npos = 0.0;
    for (int k = 0; k < PP_LOSS_TERMS; ++k) {
        double r = block_sum(pf[(size_t)threadIdx.x * PP_LOSS_TERMS + k], sh);
        if (k == 0) npos = r;
        if (threadIdx.x == 0) {
            if (k >= 1 && k <= 4) r /= (npos > 1.0 ? npos : 1.0);
            out[k] = r;
        }
    }
}

asg_ws* workspace(pp_ctx* ctx)
{
    if (ctx->asg) return (asg_ws*)ctx->asg;
    asg_ws* w = new asg_ws();
    const size_t G = PP_ASSIGN_MAX_GT;
    bool ok = hipMalloc((void**)&w->gbv, G * sizeof(float4)) == hipSuccess && hipMalloc((void**)&w->garea, G * 4) == hipSuccess &&
              hipMalloc((void**)&w->gmax, G * 4) == hipSuccess &&
              hipMalloc((void**)&w->part, (size_t)ctx->max_batch * LOSS_BLOCKS * PP_LOSS_TERMS * sizeof(double)) == hipSuccess;
    ctx->asg = w;
    if (!ok) {
        pp_assign_destroy(ctx);
        return nullptr;
    }
    return w;
}

asg_args make_args(const pp_ctx* ctx)
{
    asg_args p;
    std::memset(&p, 0, sizeof(p));
    p.nc = ctx->cfg.num_classes;
    for (int c = 0; c < p.nc; ++c) {
        p.cb[c] = ctx->cfg.class_begin[c];
        p.ce[c] = ctx->cfg.class_end[c];
        p.thr_m[c] = ctx->asg_thr_set ? ctx->asg_thr_m[c] : MATCHED_DEFAULT;
        p.thr_u[c] = ctx->asg_thr_set ? ctx->asg_thr_u[c] : UNMATCHED_DEFAULT;
    }
    return p;
}

// shared host checks of the ground-truth arguments
int check_gt(pp_ctx* ctx, const float* gt, const int32_t* gt_cls, const int32_t* gt_off_h, int nb, const char* who)
{
    if (!ctx) return PP_E_ARG;
    if (!gt_off_h) return pp_fail(ctx, PP_E_ARG, who);
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "assign: nb must be 1 .. max_batch");
    if (gt_off_h[0] < 0) return pp_fail(ctx, PP_E_ARG, "assign: negative gt_off_h[0]");
    for (int f = 0; f < nb; ++f)
        if (gt_off_h[f + 1] < gt_off_h[f]) return pp_fail(ctx, PP_E_ARG, "assign: gt_off_h is not monotone");
    if (gt_off_h[nb] > PP_ASSIGN_MAX_GT) return pp_fail(ctx, PP_E_ARG, "assign: more ground-truth rows than PP_ASSIGN_MAX_GT");
    if (gt_off_h[nb] > 0 && (!gt || !gt_cls)) return pp_fail(ctx, PP_E_ARG, "assign: null ground-truth pointer");
    if (ctx->A <= 0 || !ctx->anchors) return pp_fail(ctx, PP_E_STATE, "assign: anchors not set");
    return 0;
}

// G1 + G2 for frames [0, nb)
int launch_gmax(pp_ctx* ctx, asg_ws* w, const uint8_t* mask, const float* gt, const int32_t* gt_cls, const int32_t* gt_off_h, int nb,
                hipStream_t stream)
{
    const int G = gt_off_h[nb];
    if (G > 0) hipLaunchKernelGGL(k_gt_prep, dim3(pp_div_up(G, 64)), dim3(64), 0, stream, gt, G, w->gbv, w->garea, w->gmax);
    asg_args p = make_args(ctx);
    for (int f0 = 0; f0 < nb; f0 += ASG_GROUP) {
        const int g = nb - f0 < ASG_GROUP ? nb - f0 : ASG_GROUP;
        p.f0 = f0;
        for (int z = 0; z <= g; ++z) p.off[z] = gt_off_h[f0 + z];
        if (p.off[g] == p.off[0]) continue;
        hipLaunchKernelGGL(k_gmax, dim3(pp_div_up(ctx->A, 256), g), dim3(256), 0, stream, p, mask, ctx->A, ctx->anchors, gt_cls, w->gbv,
                           w->garea, w->gmax);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

} // namespace

void pp_assign_destroy(pp_ctx* ctx)
{
    asg_ws* w = (asg_ws*)ctx->asg;
    if (!w) return;
    void* q[] = {w->gbv, w->garea, w->gmax, w->part};
    for (void* x : q)
        if (x) (void)hipFree(x);
    delete w;
    ctx->asg = nullptr;
}

extern "C" int pp_set_assign_thresholds(pp_ctx* ctx, const float* matched_h, const float* unmatched_h)
{
    if (!ctx || !matched_h || !unmatched_h) return pp_fail(ctx, PP_E_ARG, "pp_set_assign_thresholds: null pointer");
    for (int c = 0; c < ctx->cfg.num_classes; ++c) {
        ctx->asg_thr_m[c] = matched_h[c];
        ctx->asg_thr_u[c] = unmatched_h[c];
    }
    ctx->asg_thr_set = true;
    return 0;
}

extern "C" int pp_assign_targets(pp_ctx* ctx, const uint8_t* mask, const float* gt, const int32_t* gt_cls, const int32_t* gt_off_h, int nb,
                                 int32_t* labels, float* bbox_targets, float* outside_w, int32_t* dir_targets, void* stream_)
{
    if (int rc = check_gt(ctx, gt, gt_cls, gt_off_h, nb, "pp_assign_targets: null gt_off_h")) return rc;
    if (!mask || !labels || !bbox_targets || !outside_w || !dir_targets) return pp_fail(ctx, PP_E_ARG, "pp_assign_targets: null pointer");
    asg_ws* w = workspace(ctx);
    if (!w) return pp_fail(ctx, -(int)hipErrorOutOfMemory, "pp_assign_targets: workspace allocation failed");
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = launch_gmax(ctx, w, mask, gt, gt_cls, gt_off_h, nb, stream)) return rc;
    asg_args p = make_args(ctx);
    for (int f0 = 0; f0 < nb; f0 += ASG_GROUP) {
        const int g = nb - f0 < ASG_GROUP ? nb - f0 : ASG_GROUP;
        p.f0 = f0;
        for (int z = 0; z <= g; ++z) p.off[z] = gt_off_h[f0 + z];
        hipLaunchKernelGGL(k_assign, dim3(pp_div_up(ctx->A, 256), g), dim3(256), 0, stream, p, mask, ctx->A, ctx->anchors, gt, gt_cls,
                           w->gbv, w->garea, w->gmax, labels, bbox_targets, outside_w, dir_targets);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_target_loss(pp_ctx* ctx, const float* cls, const float* box, const float* dir, const int32_t* labels,
                              const float* bbox_targets, const int32_t* dir_targets, int nb, double* terms, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!cls || !labels || !terms) return pp_fail(ctx, PP_E_ARG, "pp_target_loss: null pointer");
    const bool counts_only = !box && !dir && !bbox_targets && !dir_targets;
    if (!counts_only && (!box || !dir || !bbox_targets || !dir_targets))
        return pp_fail(ctx, PP_E_ARG, "pp_target_loss: box, dir, bbox_targets and dir_targets are all set or all null");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_target_loss: nb must be 1 .. max_batch");
    if (ctx->A <= 0) return pp_fail(ctx, PP_E_STATE, "pp_target_loss: anchors not set");
    asg_ws* w = workspace(ctx);
    if (!w) return pp_fail(ctx, -(int)hipErrorOutOfMemory, "pp_target_loss: workspace allocation failed");
    hipStream_t stream = (hipStream_t)stream_;
    hipLaunchKernelGGL(k_loss_mem, dim3(LOSS_BLOCKS, nb), dim3(LOSS_THREADS), 0, stream, ctx->A, 0, cls, box, dir, labels, bbox_targets,
                       dir_targets, w->part);
    hipLaunchKernelGGL(k_loss_final, dim3(nb), dim3(LOSS_BLOCKS), 0, stream, w->part, terms);
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_batch_loss(pp_ctx* ctx, const float* gt, const int32_t* gt_cls, const int32_t* gt_off_h, int nb, double* terms, void* stream_)
{
    if (int rc = check_gt(ctx, gt, gt_cls, gt_off_h, nb, "pp_batch_loss: null gt_off_h")) return rc;
    if (!terms) return pp_fail(ctx, PP_E_ARG, "pp_batch_loss: null pointer");
    if (!ctx->f_cls || !ctx->f_mask || ctx->last_nb < 1) return pp_fail(ctx, PP_E_STATE, "pp_batch_loss: no inference pass yet");
    if (nb > ctx->last_nb) return pp_fail(ctx, PP_E_ARG, "pp_batch_loss: nb exceeds the frames of the last inference pass");
    asg_ws* w = workspace(ctx);
    if (!w) return pp_fail(ctx, -(int)hipErrorOutOfMemory, "pp_batch_loss: workspace allocation failed");
    hipStream_t stream = (hipStream_t)stream_;
    if (int rc = pp_head_materialise(ctx, stream)) return rc; // a deferred pass left f_box / f_dir stale
    if (int rc = launch_gmax(ctx, w, ctx->f_mask, gt, gt_cls, gt_off_h, nb, stream)) return rc;
    asg_args p = make_args(ctx);
    for (int f0 = 0; f0 < nb; f0 += ASG_GROUP) {
        const int g = nb - f0 < ASG_GROUP ? nb - f0 : ASG_GROUP;
        p.f0 = f0;
        for (int z = 0; z <= g; ++z) p.off[z] = gt_off_h[f0 + z];
        hipLaunchKernelGGL(k_loss_fused, dim3(LOSS_BLOCKS, g), dim3(LOSS_THREADS), 0, stream, p, ctx->f_mask, ctx->A, ctx->anchors, gt, gt_cls,
                           w->gbv, w->garea, w->gmax, ctx->f_cls, ctx->f_box, ctx->f_dir, w->part);
    }
    hipLaunchKernelGGL(k_loss_final, dim3(nb), dim3(LOSS_BLOCKS), 0, stream, w->part, terms);
    PP_HIP(hipGetLastError());
    return 0;
}
