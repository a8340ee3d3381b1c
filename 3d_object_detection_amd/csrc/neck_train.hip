// Training side of the neck (gfx950): the backward of one RPN upsampling branch, ConvTranspose2d(k = s) -> InstanceNorm2d(eps 1e-3,
// no affine) -> ReLU (pointpillars8_shared.py:139-171), and the in-place rewrite of the three upsamplers' packed weights after an
// optimizer step.  fp32 throughout, InstanceNorm backbone only.
//
// A ConvTranspose with kernel = stride is a GEMM on the INPUT grid: with R = Cup s s rows r = co s s + ky s + kx and p = h w input
// pixels, Z[r][q] = sum_ci w[ci][r] x[ci][q] is output element (co, s qy + ky, s qx + kx), and w [Cin][Cup][s][s] IS [Cin][R].
// pp_neck_backward keeps Z -- and then dZ, in place -- in that row layout in a workspace ([frame][R][pld], pld = p rounded up to 4,
// padding columns zero), so both gradient products are plain GEMMs with contiguous operands:
//   k_neck_fwd    Z = w^T x                                     M = R,   N = p, K = Cin
//   k_neck_stats  per (frame, co): sum z, sum z^2, sum Gr, sum Gr z in fp64 over S segments of the channel's N = H W elements
//   k_neck_dz     mean / rstd / the two backward means from the S partials, dZ = rstd (Gr - mean(Gr) - xhat mean(Gr xhat)) over Z
//   k_neck_dw     dw[ci][r] = sum_{frame, q} x[ci][q] dZ[r][q]  M = Cin, N = R, K = frames x p, split into pixel / frame ranges
//   k_dw_reduce   partials summed in index order (double, rounded once; train_host.h, shared by the three families)
//   k_neck_dx     dx[ci][q] = sum_r w[ci][r] dZ[r][q]           M = Cin, N = p, K = R, summed in blocks of DX_BLOCK rows
// The three products run on v_mfma_f32_16x16x4_f32 with operands straight from global memory (every operand row is contiguous along
// the lane's load direction; the sum over K is order-free, so where K is the contiguous direction a lane's four k-steps are one
// 16-byte load, as in k_head_dw).
//
// Determinism: no atomics at all.  Segment and range counts depend on the shapes only; a frame's Z, statistics, dZ and dx do not depend
// on the batch it rides in, dw depends on nb within fp32 summation error (the K ranges do).
// pp_neck_backward_affine is the same branch with a per-channel affine (a frozen BatchNorm2d) for the norm: k_affine_neck_dz in place
// of k_neck_stats and k_neck_dz, then the same products and k_affine_reduce; pp_neck_backward itself stays the InstanceNorm backbone's.
// pp_neck_backward_bn is that branch in front of a train-mode BatchNorm2d (batch statistics pooled over the frames): k_bn_neck_sums
// per chunk, k_bn_coef, then k_bn_neck_dz and the products per chunk (Z recomputed when there are several).
// The Z, statistics and dZ kernels of every form and the family's one check, plan and driver (neck_check, neck_make_plan, neck_run) are
// neck_train.h's, shared with the 16-bit twin; this file holds the fp32 products and the entries, thin wrappers over them.
#include <cmath>
#include "pp_common.h"
#include "neck_train.h"

namespace {

// ---- dw: workgroup tile 64 ci x 32 NB rows, four waves 2 x 2, each 32 ci x 16 NB rows.  K runs over 16-pixel chunks of the launch's
// frames (chunk c: frame c / cpf, pixels 16 (c % cpf) ..); a lane takes pixels 4 q .. 4 q + 3 of the chunk as its four k-steps, one
// 16-byte load per operand row.  blockIdx.z owns chunks [z cps, (z + 1) cps) and writes partial gbase + z.
template <int NB>
__global__ void __launch_bounds__(256) k_neck_dw(const float* __restrict__ x, const float* __restrict__ dZ, float* __restrict__ part, int Cin, int R,
                                                 int p, int pld, int cpf, int nchunks, int cps, int gbase, int xvec)
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
        const int f = c / cpf, pb = (c - f * cpf) * 16 + 4 * q;
        const float* xf = x + (size_t)f * Cin * p + pb;
        const float* zf = dZ + (size_t)f * R * pld + pb;
        float xa[2][4], zb[NB][4];
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const float* s_ = xf + (size_t)(ci0 + 16 * a + l16) * p;
            if (xvec) {
                const float4 v = pb < p ? *reinterpret_cast<const float4*>(s_) : make_float4(0.f, 0.f, 0.f, 0.f);
                xa[a][0] = v.x; xa[a][1] = v.y; xa[a][2] = v.z; xa[a][3] = v.w;
            } else {
#pragma unroll
                for (int s = 0; s < 4; ++s) xa[a][s] = pb + s < p ? s_[s] : 0.f;
            }
        }
#pragma unroll
        for (int b = 0; b < NB; ++b) {
            const float4 v = pb < pld ? *reinterpret_cast<const float4*>(zf + (size_t)(r0 + 16 * b + l16) * pld) : make_float4(0.f, 0.f, 0.f, 0.f);
            zb[b][0] = v.x; zb[b][1] = v.y; zb[b][2] = v.z; zb[b][3] = v.w;
        }
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int b = 0; b < NB; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(xa[a][s], zb[b][s], acc[a][b], 0, 0, 0);
    }
    float* pw = part + (size_t)(gbase + blockIdx.z) * Cin * R;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < NB; ++b)
#pragma unroll
            for (int i = 0; i < 4; ++i) pw[(size_t)(ci0 + 16 * a + 4 * q + i) * R + r0 + 16 * b + l16] = acc[a][b][i];
}


// ---- dx: a workgroup covers ALL Cin channels (WM = Cin / 64 waves down, 4 / WM across), each wave 64 ci x 32 pixels, so dZ is read
// once.  K = R in steps of 16 rows: a lane's four k-steps are rows 4 q .. 4 q + 3, one 16-byte load of w per ci row.  The sum over R
// (up to 2048 terms) is blocked: each DX_BLOCK rows accumulate from zero and the block sums are then added in row order, so the
// rounding error grows with the block length and the block count, not with R (one running accumulator over R = 2048 deviates from
// float64 about eight times as much).
template <int WM>
__global__ void __launch_bounds__(256) k_neck_dx(const float* __restrict__ wt, const float* __restrict__ dZ, float* __restrict__ dx, int Cin, int R,
                                                 int p, int pld)
{
    constexpr int WN = 4 / WM;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int ci0 = 64 * (wave / WN), p0 = blockIdx.x * (32 * WN) + 32 * (wave % WN);
    const float* zf = dZ + (size_t)blockIdx.z * R * pld;
    float* dxf = dx + (size_t)blockIdx.z * Cin * p;
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
        for (int rb = rb0; rb < rb0 + DX_BLOCK; rb += 16) {
            float wa[4][4], zb[2][4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                const float4 v = *reinterpret_cast<const float4*>(wt + (size_t)(ci0 + 16 * a + l16) * R + rb + 4 * q);
                wa[a][0] = v.x; wa[a][1] = v.y; wa[a][2] = v.z; wa[a][3] = v.w;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const float* zr = zf + (size_t)(rb + 4 * q + s) * pld;
                zb[0][s] = px0 < p ? zr[px0] : 0.f;
                zb[1][s] = px1 < p ? zr[px1] : 0.f;
            }
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_16x16x4f32(wa[a][s], zb[b][s], acc[a][b], 0, 0, 0);
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

// dst[i] = src[map[i]], 0 where map[i] < 0 (padding of the packed image)
__global__ void __launch_bounds__(256) k_gather1(float* __restrict__ dst, const int32_t* __restrict__ map, int n, const float* __restrict__ src, int nsrc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int m = map[i];
    dst[i] = m < 0 || m >= nsrc ? 0.f : src[m];
}

// the fp32 products of neck_run (neck_train.h): the dx product reads w itself, so there is no weight image
struct neck_fp32 {
    static constexpr int KPIX = 16;
    static int grow_wt(pp_ctx*, neck_ws*, int) { return 0; }
    static void pack_wt(const neck_plan&, neck_ws*, const float*, hipStream_t) {}
    static void dw(const neck_plan& p, const dw_chunk& c, const float* xc, const float* dZ, float* part, int xvec, hipStream_t stream)
    {
        const geom& g = p.g;
        const dim3 gd(g.R / (32 * p.NBt), g.Cin / 64, c.sp);
        if (p.NBt == 4)
            hipLaunchKernelGGL(k_neck_dw<4>, gd, dim3(256), 0, stream, xc, dZ, part, g.Cin, g.R, g.p, g.pld, p.cpf, c.nchunks, c.cps, c.gbase, xvec);
        else
            hipLaunchKernelGGL(k_neck_dw<2>, gd, dim3(256), 0, stream, xc, dZ, part, g.Cin, g.R, g.p, g.pld, p.cpf, c.nchunks, c.cps, c.gbase, xvec);
    }
    static void dx(const neck_plan& p, const neck_ws*, const float* wt, const float* dZ, float* dxc, int fn, hipStream_t stream)
    {
        const geom& g = p.g;
        if (g.Cin == 64)
            hipLaunchKernelGGL(k_neck_dx<1>, dim3(pp_div_up(g.p, 128), 1, fn), dim3(256), 0, stream, wt, dZ, dxc, g.Cin, g.R, g.p, g.pld);
        else if (g.Cin == 128)
            hipLaunchKernelGGL(k_neck_dx<2>, dim3(pp_div_up(g.p, 64), 1, fn), dim3(256), 0, stream, wt, dZ, dxc, g.Cin, g.R, g.p, g.pld);
        else
            hipLaunchKernelGGL(k_neck_dx<4>, dim3(pp_div_up(g.p, 32), 1, fn), dim3(256), 0, stream, wt, dZ, dxc, g.Cin, g.R, g.p, g.pld);
    }
};

int neck_entry(pp_ctx* ctx, const char* entry, norm_form form, int branch, const neck_args& a)
{
    if (!ctx) return PP_E_ARG;
    if (int rc = neck_check(ctx, entry, NECK_CHK_ALL, form, branch, a)) return rc;
    return neck_run<neck_fp32>(ctx, form, branch, a);
}

} // namespace

void pp_neck_destroy(pp_ctx* ctx)
{
    neck_ws* w = (neck_ws*)ctx->neck;
    if (!w) return;
    void* q[] = {w->z, w->st, w->part, w->coef, w->w16, w->wmap[0], w->wmap[1], w->wmap[2]};
    for (void* x : q)
        if (x) (void)hipFree(x);
    delete w;
    ctx->neck = nullptr;
}

extern "C" int pp_neck_backward(pp_ctx* ctx, int branch, const float* x, const float* wt, const float* y, const float* dy, int nb, float* dw,
                                float* dx, void* stream_)
{
    neck_args a;
    a.x = x; a.wt = wt; a.y = y; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx; a.stream = (hipStream_t)stream_;
    return neck_entry(ctx, "pp_neck_backward", NORM_INSTANCE, branch, a);
}

// pp_neck_backward with a per-channel affine for the norm: Z recomputed as there, one pass for the sums and dZ where the sibling runs
// two, the same dw / dx products over the same K ranges and frame chunks.  shift is not read (the mask is the given y); it is an
// argument so that the three affine primitives take one (scale, shift) pair.
extern "C" int pp_neck_backward_affine(pp_ctx* ctx, int branch, const float* x, const float* wt, const float* scale, const float* shift,
                                       const float* y, const float* dy, int nb, float* dw, float* dx, double* dscale, double* dshift, void* stream_)
{
    neck_args a;
    a.x = x; a.wt = wt; a.scale = scale; a.shift = shift; a.y = y; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx;
    a.dscale = dscale; a.dshift = dshift; a.stream = (hipStream_t)stream_;
    return neck_entry(ctx, "pp_neck_backward_affine", NORM_AFFINE, branch, a);
}

// pp_neck_backward_affine behind a train-mode BatchNorm: (scale, shift) are the fold of the batch statistics (mean, var) the forward used;
// shift is not read (the mask is the given y).  chunk_frames > 0 caps the frames of a chunk below the workspace rule (dx and the sums do
// not depend on it; dw does within fp32 summation error, through the K ranges).
extern "C" int pp_neck_backward_bn(pp_ctx* ctx, int branch, const float* x, const float* wt, const float* scale, const float* shift,
                                   const float* mean, const float* var, const float* y, const float* dy, int nb, float* dw, float* dx,
                                   double* dscale, double* dshift, int chunk_frames, void* stream_)
{
    neck_args a;
    a.x = x; a.wt = wt; a.scale = scale; a.shift = shift; a.mean = mean; a.var = var; a.y = y; a.dy = dy; a.nb = nb; a.dw = dw; a.dx = dx;
    a.dscale = dscale; a.dshift = dshift; a.chunk_frames = chunk_frames; a.stream = (hipStream_t)stream_;
    return neck_entry(ctx, "pp_neck_backward_bn", NORM_BATCH, branch, a);
}

namespace {
// mode 0: pp_update_neck_weights (an fp32 plan); 1 | 2 | 3: the _mp entry for a plan committed in that 16-bit mode, where an upsampler on
// a 16-bit tiling goes through k_image16 (image16.hip) and one that keeps an fp32 tiling through k_gather1
int neck_update(pp_ctx* ctx, const char* who, int mode, const float* w1, const float* w2, const float* w3, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_ARG, (std::string(who) + ": no committed weights to update (pp_commit_weights first)").c_str());
    if (!w1 || !w2 || !w3) return pp_fail(ctx, PP_E_ARG, (std::string(who) + ": null pointer").c_str());
    if (mode == 0 && pp_effective_precision(ctx) != 0)
        return pp_fail(ctx, PP_E_ARG, "pp_update_neck_weights: fp32 mode only (the committed plan packs the upsamplers in a 16-bit format)");
    if (mode != 0)
        if (int rc = pp_mp_mode_check(ctx, who, mode)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    neck_ws* ws = workspace(ctx);
    const float* src[3] = {w1, w2, w3};
    bool is16[3] = {false, false, false};
    if (mode != 0)
        for (int b = 0; b < 3; ++b) {
            const size_t elems = (size_t)(64 << b) * (b ? 128 : 64) * (1 << b) * (1 << b);
            if (int rc = pp_update_image16(ctx, pp_net_layer_index(ctx, 1, b), src[b], nullptr, nullptr, (int)elems, 0, 0, stream, &is16[b])) return rc;
        }
    if (ws->img_gen != ctx->commit_gen) { // first update after a commit: read the committed images' layout back (synchronous)
        for (int b = 0; b < 3; ++b) {
            if (ws->wmap[b]) { (void)hipFree(ws->wmap[b]); ws->wmap[b] = nullptr; }
            ws->img[b].wmap.clear();
            if (is16[b]) continue;
            int rc = pp_net_deconv_image(ctx, b, &ws->img[b], mode != 0);
            if (rc) return rc;
            PP_HIP(hipMalloc((void**)&ws->wmap[b], ws->img[b].wmap.size() * sizeof(int32_t)));
            PP_HIP(hipMemcpy(ws->wmap[b], ws->img[b].wmap.data(), ws->img[b].wmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        }
        ws->img_gen = ctx->commit_gen;
    }
    for (int b = 0; b < 3; ++b) {
        if (is16[b]) continue;
        const int n = (int)ws->img[b].wmap.size();
        hipLaunchKernelGGL(k_gather1, dim3(pp_div_up(n, 256)), dim3(256), 0, stream, ws->img[b].w, ws->wmap[b], n, src[b], (int)ws->img[b].elems);
    }
    PP_HIP(hipGetLastError());
    return 0;
}
} // namespace

extern "C" int pp_update_neck_weights(pp_ctx* ctx, const float* w1, const float* w2, const float* w3, void* stream_)
{
    return neck_update(ctx, "pp_update_neck_weights", 0, w1, w2, w3, stream_);
}

extern "C" int pp_update_neck_weights_mp(pp_ctx* ctx, int mode, const float* w1, const float* w2, const float* w3, void* stream_)
{
    return neck_update(ctx, "pp_update_neck_weights_mp", mode, w1, w2, w3, stream_);
}
