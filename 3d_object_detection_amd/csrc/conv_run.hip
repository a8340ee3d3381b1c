// 2D backbone (RPN) + shared head, host side: what runs per frame.  launch_conv (one layer of the committed plan: the kernel parameters,
// the family's grid rule, the region launches of wino4 / wino6), the norm launches, pp_run_backbone, the head in its three forms (fused,
// cls-only, materialised on demand) and the entry points pp_backbone, pp_head, pp_backbone_*taps and pp_backbone_train_taps_bn (the
// lock-step training pass of the BatchNorm backbone with batch statistics).  The types are in conv_net.h; its
// own kernels are the three small ones around the layers: norm_relu_stats, norm_finalize and f32_to_f16.
#include <cstring>
#include "conv_net.h"

namespace ppc {
namespace {

// y = relu(x*scale+shift) (scale/shift from the producer's statistics), plus statistics of y.
// Used for the [conv, norm, relu] head of each block, whose output is both a residual and the
// input of the next InstanceNorm (pointpillars8_shared.py:133-137).
// x16: the input tensor is fp16 (the concat buffer under pp_set_precision 4); y is fp32 either way
__global__ void __launch_bounds__(256) norm_relu_stats(const float* __restrict__ x, float* __restrict__ y, int C, int HW,
                                                       int pre, const double* __restrict__ pre_acc,
                                                       const float* __restrict__ pre_scale, const float* __restrict__ pre_shift,
                                                       double inv_n, float eps, double* __restrict__ stat_acc,
                                                       size_t x_fs, size_t acc_fs, int x16, int y16)
{
    const int c = blockIdx.y;
    const _Float16* xh = reinterpret_cast<const _Float16*>(x) + blockIdx.z * x_fs;
    _Float16* yh = reinterpret_cast<_Float16*>(y) + blockIdx.z * x_fs;
    x += blockIdx.z * x_fs;
    y += blockIdx.z * x_fs;
    if (pre_acc) pre_acc += blockIdx.z * acc_fs;
    if (stat_acc) stat_acc += blockIdx.z * acc_fs;
    float sc, sh;
    if (pre == PRE_STATS) {
        double s = 0.0, q = 0.0;
        for (int r = 0; r < NREP; ++r) {
            s += pre_acc[((size_t)r * C + c) * 2];
            q += pre_acc[((size_t)r * C + c) * 2 + 1];
        }
        double mean = s * inv_n, var = q * inv_n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        double rstd = 1.0 / sqrt(var + (double)eps);
        sc = (float)rstd;
        sh = (float)(-mean * rstd);
    } else {
        sc = pre_scale[c];
        sh = pre_shift[c];
    }
    float s = 0.f, q = 0.f;
    double ds = 0.0, dq = 0.0;
    int it = 0;
    if ((HW & 3) == 0) { // planes of every shipped configuration: 16-byte aligned rows of float4
        const float4* xi = reinterpret_cast<const float4*>(x + (size_t)c * HW);
        float4* yo = reinterpret_cast<float4*>(y + (size_t)c * HW);
        const int n4 = HW >> 2;
        const uint2* xi16 = reinterpret_cast<const uint2*>(xh + (size_t)c * HW);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
            float4 v;
            if (x16) {
                const f16x4_t h = __builtin_bit_cast(f16x4_t, xi16[i]);
                v = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
            } else v = xi[i];
            v.x = fmaxf(fmaf(v.x, sc, sh), 0.f);
            v.y = fmaxf(fmaf(v.y, sc, sh), 0.f);
            v.z = fmaxf(fmaf(v.z, sc, sh), 0.f);
            v.w = fmaxf(fmaf(v.w, sc, sh), 0.f);
            if (y16) reinterpret_cast<uint2*>(yh + (size_t)c * HW)[i] = (uint2){pk_f16(v.x, v.y), pk_f16(v.z, v.w)}; // statistics below: of the fp32 values
            else yo[i] = v;
            s += (v.x + v.y) + (v.z + v.w);
            q += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
            if (++it == 8) { ds += s; dq += q; s = 0.f; q = 0.f; it = 0; }
        }
    } else { // odd planes (e.g. a 9 x 11 level-2 map): channel c starts at a 4-byte aligned address only -> scalar loop
        const float* xi = x + (size_t)c * HW;
        float* yo = y + (size_t)c * HW;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
            const float v = fmaxf(fmaf(x16 ? (float)xh[(size_t)c * HW + i] : xi[i], sc, sh), 0.f);
            if (y16) yh[(size_t)c * HW + i] = (_Float16)v; else yo[i] = v;
            s += v;
            q += v * v;
            if (++it == 32) { ds += s; dq += q; s = 0.f; q = 0.f; it = 0; }
        }
    }
    ds += s;
    dq += q;
    if (!stat_acc) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ds += __shfl_xor(ds, o);
        dq += __shfl_xor(dq, o);
    }
    __shared__ double rs[4], rq[4];
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = ds; rq[threadIdx.x >> 6] = dq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* dst = stat_acc + ((size_t)(blockIdx.x % NREP) * C + c) * 2;
        atomicAdd(dst, rs[0] + rs[1] + rs[2] + rs[3]);
        atomicAdd(dst + 1, rq[0] + rq[1] + rq[2] + rq[3]);
    }
}

// InstanceNorm statistics -> (scale, shift) once per frame and layer, instead of once per workgroup of the
// consuming conv (same fp64 formula the kernels' PRE_STATS prologue uses, so results are bit-identical)
__global__ void __launch_bounds__(320) norm_finalize(const double* __restrict__ acc, size_t acc_fs, int C, double inv_n, float eps,
                                                     float* __restrict__ aff, size_t aff_fs)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    const double* pa = acc + (size_t)blockIdx.x * acc_fs;
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int r = 0; r < NREP; ++r) { s += pa[((size_t)r * C + c) * 2]; q += pa[((size_t)r * C + c) * 2 + 1]; }
    const double mean = s * inv_n;
    double var = q * inv_n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    aff[(size_t)blockIdx.x * aff_fs + c] = (float)rstd;
    aff[(size_t)blockIdx.x * aff_fs + 320 + c] = (float)(-mean * rstd);
}

// Train-mode BatchNorm: the per-frame accumulators of one site pooled in frame order in fp64 over n = frames x positions, mean and the
// biased variance rounded once to fp32, and the (scale, shift) that pp_bn_fold's fp64 expression gives for (gamma, beta, mean32, var32)
__global__ void __launch_bounds__(256) bn_batch_finalize(const double* __restrict__ acc, size_t acc_fs, int nb, int C, int stat_C, double n,
                                                         const float* __restrict__ gamma, const float* __restrict__ beta, float* __restrict__ mean,
                                                         float* __restrict__ var, float* __restrict__ scale, float* __restrict__ shift,
                                                         float* __restrict__ pass_scale, float* __restrict__ pass_shift)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    double s = 0.0, q = 0.0;
    for (int f = 0; f < nb; ++f) {
        const double* pa = acc + (size_t)f * acc_fs;
#pragma unroll
        for (int r = 0; r < NREP; ++r) { s += pa[((size_t)r * stat_C + c) * 2]; q += pa[((size_t)r * stat_C + c) * 2 + 1]; }
    }
    const double m = s / n;
    double v = q / n - m * m;
    v = v > 0.0 ? v : 0.0;
    const float mf = (float)m, vf = (float)v;
    const double sc = (double)gamma[c] / sqrt((double)vf + 1e-3);
    const float scf = (float)sc, shf = (float)((double)beta[c] - (double)mf * sc);
    mean[c] = mf; var[c] = vf; scale[c] = scf; shift[c] = shf;
    pass_scale[c] = scf; pass_shift[c] = shf;
}

__global__ void __launch_bounds__(256) f32_to_f16(const float* __restrict__ x, _Float16* __restrict__ y, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = (_Float16)x[i];
}

} // namespace

// The kernel parameters of one launch of L.  launch_conv redirects the prologue when it finalises the statistics itself, and the
// region launches add their rectangle and item list.
static ConvP conv_params(pp_ctx* ctx, const Layer& L, const ConvCall& c)
{
    pp_net* net = (pp_net*)ctx->net;
    const NormRef& pre = c.pre;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.in = c.in; p.w = L.w; p.out = c.out; p.res = c.res;
    p.Cin = L.cin; p.Hin = c.Hin; p.Win = c.Win;
    p.Cout = L.rows; p.Hout = c.Hout; p.Wout = c.Wout;
    p.pre = pre.mode; p.pre_acc = pre.acc; p.pre_scale = pre.scale; p.pre_shift = pre.shift;
    p.pre_inv_n = pre.inv_n; p.eps = 1e-3f; p.aff_fs = pre.aff_fs;
    p.stat_acc = c.stat; p.stat_C = c.stat_C;
    p.bias = (L.kind == 2 && L.var.family == Family::Gemm1x1) ? net->head_bias_perm : net->head_bias; p.out_box = c.out_box; p.out_dir = c.out_dir;
    { const int na = ctx->cfg.num_anchor_per_loc; p.n_cls = na; p.n_box = 7 * na; p.n_rows = 10 * na; }
    p.w_bm = net->layers.back().var.bm; p.w_bmp = net->layers.back().var.bmp;
    // frame strides of a batched launch (every per-frame tensor is stored [B][...])
    const size_t hw = (size_t)c.Hout * c.Wout;
    p.in_fs = (size_t)L.cin * c.Hin * c.Win;
    p.out_fs = c.out_fs ? c.out_fs : (L.kind == 2 ? (size_t)p.n_cls * hw : (size_t)L.rows * hw);
    p.res_fs = p.out_fs;
    p.box_fs = (size_t)p.n_box * hw;
    p.dir_fs = (size_t)2 * p.n_cls * hw;
    p.pre_fs = pre.fs;
    p.stat_fs = STAT_FS;
    p.pmap = c.pmap; p.feat = c.feat;
    p.pmap_fs = (size_t)c.Hin * c.Win;
    p.feat_fs = (size_t)ctx->cfg.max_voxels * 64;
    p.nb = c.nb;
    return p;
}

// profile bracket (pp_profile_begin) of the level-0 stride-1 layers: one event pair around the layer's launches, and its flops
static bool prof_tagged(const pp_ctx* ctx, const Layer& L) { return ctx->prof_on && L.kind == 0 && L.level == 0 && L.stride == 1; }
static int prof_mark(pp_ctx* ctx, const Layer& L, const ConvCall& c, hipStream_t stream, bool end)
{
    if (!prof_tagged(ctx, L)) return 0;
    if (end) {
        PP_HIP(hipEventRecord(ctx->prof_ev[ctx->prof_used + 1], stream));
        ctx->prof_used += 2;
        return 0;
    }
    if (ctx->prof_used + 2 > ctx->prof_ev.size()) {
        hipEvent_t a, b;
        PP_HIP(hipEventCreate(&a));
        PP_HIP(hipEventCreate(&b));
        ctx->prof_ev.push_back(a);
        ctx->prof_ev.push_back(b);
    }
    ctx->prof_flops = 2.0 * c.Hout * c.Wout * (double)L.cin * L.cout * 9.0 * c.nb;
    PP_HIP(hipEventRecord(ctx->prof_ev[ctx->prof_used], stream));
    return 0;
}

// wino4 / wino6: persistent, ONE 4-wave workgroup per CU (512 registers per lane, 3-deep LDS ring), a multiple of the 8 XCDs.
// Whole main tiles first; what they leave uncovered goes to strip launches of thin tiles when that needs fewer tiles
// than rounding the main grid up (same weight image: it depends on the 64-row block and the chunk only).
static int launch_regions(pp_ctx* ctx, const Layer& L, const ConvCall& c, const ConvP& p, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    const Variant& v = L.var;
    const int Hout = c.Hout, Wout = c.Wout, B = c.nb, ts_k = c.ts_k;
    if ((size_t)L.rows * Hout * Wout * 4 >= 0x80000000ull) return PP_E_ARG; // the epilogue parks idle lanes' offsets 2 GB out (W4_FAR)
    // these two kernels always normalise (every stride-1 convolution of the network follows a norm): with PRE_RAW they would read a null table
    if (p.pre == PRE_RAW) return pp_fail(ctx, PP_E_ARG, "wino4 / wino6 tilings have no raw prologue: give the layer a (scale, shift)");
    const int ncb = pp_div_up(L.rows, v.bm);
    // Tile skipping (tile_skip.hip): ts_k = the layer's ordinal among level 0's stride-1 layers, handed over by a pass whose first conv
    // ran sparse (or by the single-layer hook).  Listed launch + fill only for the fp32 wino6 main tile on a map of whole main tiles
    // (no strip launches) with lists for exactly these B frames in place; today's launch in every other case.
    const int2* ts_items = nullptr;
    const int32_t* ts_count = nullptr;
    const bool listed = ts_k > 0 && v.family == Family::Wino6 && v.kern2 && v.pw == 16 && v.ph == 16 && net->eff_prec == 0 && !net->up16 &&
                        L.kind == 0 && L.level == 0 && L.stride == 1 && Wout % v.pw == 0 && Hout % v.ph == 0 && Hout == ctx->H && Wout == ctx->W &&
                        pp_ts_list(ctx, ts_k, B, &ts_items, &ts_count);
    if (prof_tagged(ctx, L)) {
        const double dense = (double)(Wout / v.pw) * (Hout / v.ph) * ncb * B;
        ctx->prof_items_dense += dense;
        if (listed) ctx->prof_ts_layer.push_back(ts_k | (ncb << 8)); else ctx->prof_items += dense;
    }
    if (int rc = prof_mark(ctx, L, c, stream, false)) return rc;
    auto launch_region = [&](const Variant& rv, int x0, int y0, int x1, int y1) {
        ConvP q = p;
        q.rx0 = x0; q.ry0 = y0; q.rx1 = x1; q.ry1 = y1;
        q.rnbx = pp_div_up(x1 - x0, rv.pw); q.rnby = pp_div_up(y1 - y0, rv.ph);
        const int total = q.rnbx * q.rnby * ncb * B;
        int g = net->num_cu;
        if (g > total) g = total;
        g = (g + 7) & ~7;
        if (listed) { q.items = ts_items; q.item_count = ts_count; } // same grid as the dense total: the kernel reads its own
        hipLaunchKernelGGL(listed ? rv.kern2 : rv.kern, dim3(g), dim3(rv.threads), rv.lds, stream, q);
    };
    const int mw = (Wout / v.pw) * v.pw, mh = (Hout / v.ph) * v.ph;
    const Variant &sv = strip_v(v.family), &sh = strip_h(v.family);
    // cost of the slowest workgroup: items are dealt evenly over min(CUs, items) persistent workgroups, a tile takes about
    // 2.4 us per 8-channel chunk + 5 us of epilogue, and a strip launch adds its own rounds plus ~30 us of launch gap and
    // pipeline prologue (at batch 1 the 20 extra launches of a frame cost more than the empty tile area they save: 3.4 ms
    // against 2.2 ms per frame; at 16+ frames per launch the strips win: 979 against 1114 us on the 100 x 100 layers)
    // The split is decided for the context's max_batch, NOT for the frames of this launch: full tiles and main + strip
    // launches group the fp32 partial sums of the InstanceNorm statistics differently (~3e-5 on the logits), and a frame's
    // result must not depend on how many frames ride in its pass.
    const int plan_b = ctx->max_batch;
    auto rounds = [&](int tiles) { return tiles > 0 ? pp_div_up((int64_t)tiles * ncb * plan_b, net->num_cu) : 0; };
    const int t_main = (mw / v.pw) * (mh / v.ph);
    const int t_right = Wout > mw ? pp_div_up(Wout - mw, sv.pw) * pp_div_up(Hout, sv.ph) : 0;
    const int t_bottom = Hout > mh ? pp_div_up(mw, sh.pw) * pp_div_up(Hout - mh, sh.ph) : 0;
    const double tile_us = v.family == Family::Wino6 ? 1.9 * (L.cin / 8) + 3.5 : 2.4 * (L.cin / 8) + 5.0;
    const double full = rounds(pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph)) * tile_us;
    const double split = (rounds(t_main) + rounds(t_right) + rounds(t_bottom)) * tile_us + 30.0 * ((t_right > 0) + (t_bottom > 0));
    const bool no_strips = net->w4_strips == 0, all_strips = net->w4_strips == 2;
    if ((split < full || all_strips) && mw > 0 && mh > 0 && !no_strips && (Wout > mw || Hout > mh)) {
        launch_region(v, 0, 0, mw, mh);
        if (Wout > mw) launch_region(sv, mw, 0, Wout, Hout);
        if (Hout > mh) launch_region(sh, 0, mh, mw, Hout);
    } else {
        launch_region(v, 0, 0, Wout, Hout);
        if (listed)
            if (int rc = pp_ts_fill(ctx, ts_k, B, c.out, p.out_fs, L.rows, stream)) return rc;
    }
    if (int rc = prof_mark(ctx, L, c, stream, true)) return rc;
    PP_HIP(hipGetLastError());
    return 0;
}

// One layer of the committed plan: L.var's kernel on L.w over the tensors of `c`
int launch_conv(pp_ctx* ctx, const Layer& L, const ConvCall& c, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    const Variant& v = L.var;
    const int Hin = c.Hin, Win = c.Win, Hout = c.Hout, Wout = c.Wout, B = c.nb;
    ConvP p = conv_params(ctx, L, c);
    const bool fin_in_kernel = B == 1 && finalises_in_prologue(v.family);
    if (c.pre.mode == PRE_STATS && net->aff && L.cin <= 320 && !fin_in_kernel) {
        hipLaunchKernelGGL(norm_finalize, dim3(B), dim3(320), 0, stream, c.pre.acc, c.pre.fs, L.cin, c.pre.inv_n, p.eps, net->aff, (size_t)640);
        p.pre = PRE_AFFINE; p.pre_scale = net->aff; p.pre_shift = net->aff + 320; p.aff_fs = 640;
    }
    // the family's grid rule
    dim3 grid(pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph), pp_div_up(L.rows, v.bm), B);
    switch (v.family) {
    case Family::Gemm1x1: { // persistent: one workgroup per CU, a multiple of the row-block count
        if ((Hin * Win) & 3) return PP_E_ARG; // gemm1x1 reads pixel quads (choose_variant never offers it for such a plane)
        const int ncb = pp_div_up(L.rows, v.bm);
        int g = (net->num_cu * v.wpc / ncb) * ncb;
        if (g < ncb) g = ncb;
        grid = dim3(g, 1, 1);
        break;
    }
    case Family::Conv16: { // conv16: persistent, one 4-wave workgroup per CU, XCD-contiguous item ranges (grid a multiple of 8)
        if ((size_t)L.rows * Hout * Wout * 4 >= 0x80000000ull || (size_t)L.cin * Hin * Win * 4 >= 0x80000000ull) return PP_E_ARG; // buffer offsets are 32-bit, idle lanes park 2 GB out
        if (p.pre == PRE_STATS) return pp_fail(ctx, PP_E_STATE, "conv16: the producer's statistics must be finalised to (scale, shift)");
        if ((Win & 3) || (Wout & 3) || (L.cin & 15) || (L.rows % v.bm)) return PP_E_ARG;
        const int total = pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph) * (L.rows / v.bm) * B;
        int g = net->num_cu * (v.waves * 64 / v.threads); // workgroups per CU the variant is built for
        if (g > total) g = total;
        g = (g + 7) & ~7;
        grid = dim3(g, 1, 1);
        break;
    }
    case Family::Wino4:
    case Family::Wino6: return launch_regions(ctx, L, c, p, stream);
    case Family::Wino: { // persistent Winograd: two workgroups per CU (LDS and registers allow exactly two), a multiple of the 8 XCDs
        const int total = (int)grid.x * (int)grid.y * B;
        int g = (v.threads >= 512 ? 1 : 2) * net->num_cu; // 8-wave workgroups fill a CU's registers alone
        if (g > total) g = total;
        g = (g + 7) & ~7;
        grid = dim3(g, 1, 1);
        break;
    }
    case Family::Direct: break; // one workgroup per (tile, row block, frame)
    }
    if (int rc = prof_mark(ctx, L, c, stream, false)) return rc;
    hipLaunchKernelGGL((c.pmap && v.kern2) ? v.kern2 : v.kern, grid, dim3(v.threads), layer_lds(v, L.cin), stream, p);
    if (int rc = prof_mark(ctx, L, c, stream, true)) return rc;
    PP_HIP(hipGetLastError());
    return 0;
}

// The cls-only head pass as a launch: the head layer with the cls tiling and one 16-row block; the weights stay the head's image.
int launch_head_cls(pp_ctx* ctx, const Variant& v, const float* in, const NormRef& pre, float* cls, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    Layer L = net->layers.back(); // shares the device image (no ownership: Layer has no destructor)
    L.var = v;
    L.rows = 16;
    ConvCall c;
    c.in = in; c.Hin = ctx->H; c.Win = ctx->W;
    c.out = cls; c.Hout = ctx->H; c.Wout = ctx->W;
    c.pre = pre; c.nb = nb;
    return launch_conv(ctx, L, c, stream);
}

// statistics slot / folded-BN arrays for a site
NormRef norm_ref(pp_ctx* ctx, int site, int C, int coff, size_t count)
{
    pp_net* net = (pp_net*)ctx->net;
    NormRef r;
    r.C = C;
    if (ctx->cfg.norm_kind == 1) {
        r.mode = PRE_AFFINE;
        r.scale = (net->bn_pass ? net->bnp_scale : net->bn_scale) + (size_t)site * 320 + coff;
        r.shift = (net->bn_pass ? net->bnp_shift : net->bn_shift) + (size_t)site * 320 + coff;
    } else {
        r.mode = PRE_STATS;
        r.acc = net->stats + (size_t)site * NREP * 320 * 2;
        r.inv_n = 1.0 / (double)count;
        r.fs = STAT_FS;
    }
    return r;
}

double* stat_slot(pp_ctx* ctx, int site)
{
    pp_net* net = (pp_net*)ctx->net;
    if (ctx->cfg.norm_kind == 1 && !net->bn_pass) return nullptr;
    return net->stats + (size_t)site * NREP * 320 * 2;
}

int launch_norm_relu(pp_ctx* ctx, const float* x, float* y, int C, int HW, const NormRef& pre, double* stat, hipStream_t stream,
                     int B, int x16, int y16)
{
    int bx = pp_div_up(HW / 4, 256 * 4);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(norm_relu_stats, dim3(bx, C, B), dim3(256), 0, stream, x, y, C, HW, pre.mode, pre.acc, pre.scale,
                       pre.shift, pre.inv_n, 1e-3f, stat, (size_t)C * HW, STAT_FS, x16, y16);
    PP_HIP(hipGetLastError());
    return 0;
}

bool level0_main_wino6(const pp_net* net, int h, int w)
{
    int n = 0;
    for (const Layer& L : net->layers)
        if (L.kind == 0 && L.level == 0 && L.stride == 1) {
            ++n;
            if (L.var.family != Family::Wino6 || !L.var.kern2 || L.var.pw != 16 || L.var.ph != 16 || (w % 16) || (h % 16)) return false;
        }
    return n >= 1 && n <= 3 && net->eff_prec == 0;
}

} // namespace ppc

using namespace ppc;

// pp_backbone_train_taps_bn: the producer of block b's norm `k` has been launched over nb frames (k = 0 .. 5: site_block(b, k); k = 7:
// the upsampler's channel slice of site 7): pool its statistics and write the pass's fold.  Inert outside such a pass.
static int bn_pass_finalize(pp_ctx* ctx, int b, int k, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    if (!net->bn_pass) return 0;
    const bool up = k == 7;
    const int nconv = 1 + (b == 0 ? 3 : 5);                            // norms of the block's convolutions; the upsampler's follows them
    const int idx = (b == 0 ? 0 : b == 1 ? 5 : 12) + (up ? nconv : k); // the layer in bn_sites() order
    const int C = up ? (b == 0 ? 64 : 128) : kC[b], coff = up ? (b == 0 ? 0 : b == 1 ? 64 : 192) : 0;
    const int site = up ? 7 : site_block(b, k), stat_C = up ? 320 : kC[b];
    const double n = (double)nb * (up ? (double)ctx->H * ctx->W : (double)(ctx->H >> b) * (ctx->W >> b));
    const size_t o = (size_t)site * 320 + coff;
    hipLaunchKernelGGL(bn_batch_finalize, dim3(1), dim3(256), 0, stream, net->stats + (size_t)site * NREP * 320 * 2 + (size_t)coff * 2, STAT_FS, nb, C,
                       stat_C, n, net->bnp_gb[2 * idx], net->bnp_gb[2 * idx + 1], net->bnp_out[0] + idx * 256, net->bnp_out[1] + idx * 256,
                       net->bnp_out[2] + idx * 256, net->bnp_out[3] + idx * 256, net->bnp_scale + o, net->bnp_shift + o);
    PP_HIP(hipGetLastError());
    return 0;
}

// deconv L of block b on the raw block output x -> channel slice of up[320,H,W] + stats (site 7, channel offset)
static int run_upsampler(pp_ctx* ctx, const Layer& L, int b, const float* x, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    const int H = ctx->H, W = ctx->W, coff = b == 0 ? 0 : b == 1 ? 64 : 192;
    double* st = stat_slot(ctx, 7);
    ConvCall k;
    k.in = x; k.Hin = k.Hout = H >> b; k.Win = k.Wout = W >> b;
    // the block's channel slice of the concat buffer (element offsets: the buffer holds fp16 under pp_set_precision 4)
    k.out = net->up16 ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(net->up) + (size_t)coff * H * W) : net->up + (size_t)coff * H * W;
    k.stat = st ? st + (size_t)coff * 2 : nullptr; k.stat_C = 320; k.nb = nb; k.out_fs = (size_t)320 * H * W;
    return launch_conv(ctx, L, k, stream);
}

// canvas [64,gx,gy] -> up [320,H,W] PRE-norm (+ statistics); the head (or pp_backbone's final pass)
// applies the last norm + ReLU.
int pp_run_backbone(pp_ctx* ctx, const float* canvas, int nb, hipStream_t stream, const int32_t* pmap, const float* feat)
{
    pp_net* net = (pp_net*)ctx->net;
    const int H = ctx->H, W = ctx->W;
    if ((H % 4) || (W % 4)) return pp_fail(ctx, PP_E_ARG, "backbone: BEV grid must be a multiple of 8 in x and y");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "backbone: batch exceeds cfg.max_batch");
    ctx->sc1_last_nb = 0;
    pp_ts_begin_pass(ctx);
    if (ctx->cfg.norm_kind == 0 || net->bn_pass) PP_HIP(hipMemsetAsync(net->stats, 0, STAT_FS * sizeof(double) * nb, stream));
    const float* x = canvas;
    int Hin = ctx->gx, Win = ctx->gy;
    size_t li = 0;
    for (int b = 0; b < 3; ++b) {
        const int c = kC[b];
        const int h = H >> b, w = W >> b;
        const size_t cnt = (size_t)h * w;
        float** Bf = net->buf[b];
        int rc;
        // strided conv (raw input) -> Bf[0] + stats(site 0); the fused fp32 path runs the first one over the active pixels only
        if (b == 0 && pmap && net->eff_prec == 0 && pp_sc1_usable(ctx)) {
            ++li;
            if ((rc = pp_sc1_run(ctx, pmap, feat, Bf[0], stat_slot(ctx, site_block(0, 0)), STAT_FS, nb, stream))) return rc;
            // the map is exactly zero outside the active set now: lists of the tiles level 0's stride-1 layers need not recompute
            if (ctx->sc1_last_nb == nb && !net->up16 && pp_ts_usable(ctx, 3) && level0_main_wino6(net, h, w)) {
                if ((rc = pp_ts_build(ctx, nb, nullptr, stream))) return rc;
                pp_ts_mark_pass(ctx, nb);
            }
        } else {
            ConvCall k;
            k.in = x; k.Hin = Hin; k.Win = Win; k.out = Bf[0]; k.Hout = h; k.Wout = w;
            k.stat = stat_slot(ctx, site_block(b, 0)); k.stat_C = c; k.nb = nb;
            if (b == 0) { k.pmap = pmap; k.feat = feat; }
            if ((rc = launch_conv(ctx, net->layers[li++], k, stream))) return rc;
        }
        if ((rc = bn_pass_finalize(ctx, b, 0, nb, stream))) return rc;
        // the level's pre-norm conv output z leaves through its own copy hook: the first unit reuses Bf[0] as a spare.  The hooks copy
        // one frame, or every frame of the lock-step training pass (z [nb][C][h][w], units [n_b][nb][C][h][w]: a unit's frames together)
        const bool hooks = nb == 1 || net->bn_pass;
        const size_t ubytes = (size_t)nb * c * cnt * sizeof(float);
        if (hooks && net->z_tap[b]) PP_HIP(hipMemcpyAsync(net->z_tap[b], Bf[0], ubytes, hipMemcpyDeviceToDevice, stream));
        // y = relu(norm(Bf[0])) -> Bf[1] + stats(site 1) (the first Resnet2 unit's leading norm)
        if ((rc = pp_stage_mark(ctx, stream, PP_ST_NORM))) return rc;
        if ((rc = launch_norm_relu(ctx, Bf[0], Bf[1], c, (int)cnt, norm_ref(ctx, site_block(b, 0), c, 0, cnt),
                                   stat_slot(ctx, site_block(b, 1)), stream, nb, net->up16 ? 1 : 0, net->up16 ? 1 : 0))) return rc;
        if ((rc = bn_pass_finalize(ctx, b, 1, nb, stream))) return rc;
        if ((rc = pp_stage_mark(ctx, stream, PP_ST_CONV))) return rc;
        float* cur = Bf[1];
        float* spare[3] = {Bf[0], Bf[2], Bf[3]};
        // the unit inputs (h, m, r at level 0; h, m3, r3, m4, r4 at levels 1 and 2) leave through the copy hook behind the launch that
        // produces each: the level buffers are reused before the pass ends
        float* utap = hooks ? net->unit_tap[b] : nullptr;
        int ucount = 0;
        if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * nb * c * cnt, cur, ubytes, hipMemcpyDeviceToDevice, stream));
        int ts_k = 0; // level 0: ordinal of the next stride-1 layer (launch_conv ignores it unless this pass built tile lists)
        // the level's next stride-1 layer: out = conv(relu(norm_site(in))) + res, with the statistics of out
        auto conv = [&](const float* in, float* out, const float* res, int site, double* stat) {
            ConvCall k;
            k.in = in; k.Hin = h; k.Win = w; k.out = out; k.Hout = h; k.Wout = w;
            k.res = res; k.pre = norm_ref(ctx, site_block(b, site), c, 0, cnt); k.stat = stat; k.stat_C = c;
            k.nb = nb; k.ts_k = b == 0 ? ++ts_k : 0;
            return launch_conv(ctx, net->layers[li++], k, stream);
        };
        for (int u = 0; u < block_units(b); ++u) {
            float* t1 = spare[0];
            float* t2 = spare[1];
            // stats for the NEXT unit's leading norm are produced by this unit's output
            double* out_stat = u == block_units(b) - 1 ? nullptr : stat_slot(ctx, site_block(b, 1 + 2 * (u + 1)));
            if (unit_two_convs(b, u)) {
                if ((rc = conv(cur, t1, nullptr, 1 + 2 * u, stat_slot(ctx, site_block(b, 2 + 2 * u))))) return rc;
                if ((rc = bn_pass_finalize(ctx, b, 2 + 2 * u, nb, stream))) return rc;
                if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * nb * c * cnt, t1, ubytes, hipMemcpyDeviceToDevice, stream));
                if ((rc = conv(t1, t2, cur, 2 + 2 * u, out_stat))) return rc;
                if (out_stat && (rc = bn_pass_finalize(ctx, b, 1 + 2 * (u + 1), nb, stream))) return rc;
                if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * nb * c * cnt, t2, ubytes, hipMemcpyDeviceToDevice, stream));
                spare[1] = cur; // t2 becomes current; old current and t1 are free
                cur = t2;
            } else {
                if ((rc = conv(cur, t1, cur, 1 + 2 * u, out_stat))) return rc;
                spare[0] = cur;
                cur = t1;
            }
        }
        net->tap[b] = cur;
        if ((rc = run_upsampler(ctx, net->layers[li++], b, cur, nb, stream))) return rc;
        if ((rc = bn_pass_finalize(ctx, b, 7, nb, stream))) return rc;
        x = cur;
        Hin = h;
        Win = w;
    }
    return 0;
}

static int pp_head_impl(pp_ctx* ctx, const float* in, const NormRef& pre, float* cls, float* box, float* dir, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    ConvCall c;
    c.in = in; c.Hin = ctx->H; c.Win = ctx->W;
    c.out = cls; c.Hout = ctx->H; c.Wout = ctx->W; c.out_box = box; c.out_dir = dir;
    c.pre = pre; c.nb = nb;
    return launch_conv(ctx, net->layers.back(), c, stream);
}

int pp_run_head_fused(pp_ctx* ctx, float* cls, float* box, float* dir, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    NormRef pre = norm_ref(ctx, 7, 320, 0, (size_t)ctx->H * ctx->W);
    return pp_head_impl(ctx, net->up, pre, cls, box, dir, nb, stream);
}

// ---- deferred head (pp_infer_batch): cls rows for every pixel, box / dir logits for the selected candidates only ----
bool pp_head_defer_on(pp_ctx* ctx)
{
    const pp_net* net = (const pp_net*)ctx->net;
    return ctx->head_defer && net && ctx->weights_ready && net->defer_ok;
}

int pp_run_head_cls(pp_ctx* ctx, float* cls, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    NormRef pre = norm_ref(ctx, 7, 320, 0, (size_t)ctx->H * ctx->W);
    int rc = launch_head_cls(ctx, net->cls_var, net->up, pre, cls, nb, stream);
    if (rc) return rc;
    ctx->head_stale = true;
    ctx->stale_nb = nb;
    ctx->stale_stream = stream;
    return 0;
}

// What the candidate head (postprocess.hip) reads: the head image and the concat buffer with the normalisation the cls pass of
// `nb` frames just used (a batched launch finalised the statistics into net->aff, a single frame finalises them in the kernel).
int pp_net_head_gather(pp_ctx* ctx, int nb, pp_head_gather* g)
{
    pp_net* net = (pp_net*)ctx->net;
    const Layer& head = net->layers.back();
    if (!net->defer_ok) return pp_fail(ctx, PP_E_STATE, "candidate head: the committed plan has no fp32 gemm1x1 head image");
    const NormRef pre = norm_ref(ctx, 7, 320, 0, (size_t)ctx->H * ctx->W);
    g->w = head.w; g->bm = head.var.bm; g->bmp = head.var.bmp; g->K = head.cin;
    g->bias_perm = net->head_bias_perm;
    g->in = net->up; g->in_fs = (size_t)head.cin * ctx->H * ctx->W; g->HW = ctx->H * ctx->W;
    g->pre = pre.mode; g->pre_acc = pre.acc; g->pre_fs = pre.fs; g->pre_inv_n = pre.inv_n;
    g->pre_scale = pre.scale; g->pre_shift = pre.shift; g->aff_fs = 0; g->eps = 1e-3f;
    if (pre.mode == PRE_STATS && nb > 1) { g->pre = PRE_AFFINE; g->pre_scale = net->aff; g->pre_shift = net->aff + 320; g->aff_fs = 640; }
    return 0;
}

// Full box / dir (and cls) tensors of the last deferred pass: today's head over the retained concat buffer and statistics.
int pp_head_materialise(pp_ctx* ctx, hipStream_t stream)
{
    if (!ctx->head_stale) return 0;
    ctx->head_stale = false;
    return pp_run_head_fused(ctx, ctx->f_cls, ctx->f_box, ctx->f_dir, ctx->stale_nb, stream);
}

extern "C" int pp_set_head_defer(pp_ctx* ctx, int on)
{
    if (!ctx) return PP_E_ARG;
    ctx->head_defer = on && !ctx->head_defer_env_off;
    return 0;
}

extern "C" int pp_head_defer_active(pp_ctx* ctx)
{
    if (!ctx) return 0;
    return pp_head_defer_on(ctx) ? 1 : 0;
}

extern "C" int pp_backbone(pp_ctx* ctx, const float* canvas, float* rpn_out, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone: weights not committed");
    if (!canvas || !rpn_out) return pp_fail(ctx, PP_E_ARG, "pp_backbone: null pointer");
    if (int rc0 = pp_head_materialise(ctx, stream)) return rc0; // the concat buffer and its statistics are about to be overwritten
    int rc = pp_run_backbone(ctx, canvas, 1, stream, nullptr, nullptr);
    if (rc) return rc;
    pp_net* net = (pp_net*)ctx->net;
    const int HW = ctx->H * ctx->W;
    // stand-alone API: materialise relu(norm(up)) as the reference's RPN.forward returns it
    return launch_norm_relu(ctx, net->up, rpn_out, 320, HW, norm_ref(ctx, 7, 320, 0, (size_t)HW), nullptr, stream, 1, net->up16 ? 1 : 0);
}

extern "C" int pp_head(pp_ctx* ctx, const float* rpn_out, float* cls, float* box, float* dir, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_head: weights not committed");
    if (!rpn_out || !cls || !box || !dir) return pp_fail(ctx, PP_E_ARG, "pp_head: null pointer");
    NormRef raw; // rpn_out is already normalised + ReLU'd
    pp_net* net = (pp_net*)ctx->net;
    if (net->up16) { // the head's tiling reads an fp16 tensor: round the caller's fp32 features into the (idle) concat buffer first
        const size_t n = (size_t)320 * ctx->H * ctx->W;
        hipLaunchKernelGGL(f32_to_f16, dim3(2048), dim3(256), 0, stream, rpn_out, reinterpret_cast<_Float16*>(net->up), n);
        return pp_head_impl(ctx, net->up, raw, cls, box, dir, 1, stream);
    }
    return pp_head_impl(ctx, rpn_out, raw, cls, box, dir, 1, stream);
}

// pp_backbone plus the block outputs x1..x3 and, where given, the copy hooks of pp_run_backbone: units[b] f32[3 | 5 | 5][C_b][H>>b][W>>b]
// and z[b] f32[C_b][H>>b][W>>b] per level b (either array, or any entry, may be null).  The hooks are armed for this one pass only.
// who: the entry point; null_in: the entry point one of whose own pointer arguments is null (or nullptr)
// mode: 0 an fp32 plan (the four fp32 entries), 1 | 2 | 3 a plan committed in that 16-bit mode (pp_backbone_train_taps_mp): the level buffers
// are fp32 there too and the copy hooks sit behind the launches whatever tiling runs, so the pass is the same with the other guard
static int backbone_taps(pp_ctx* ctx, const char* who, const char* null_in, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3,
                         float* const* units, float* const* z, void* stream_, int mode = 0)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, (std::string(who) + ": weights not committed").c_str());
    if (null_in) return pp_fail(ctx, PP_E_ARG, (std::string(null_in) + ": null pointer").c_str());
    if (!canvas || !rpn_out || !x1 || !x2 || !x3) return pp_fail(ctx, PP_E_ARG, "pp_backbone_taps: null pointer");
    pp_net* net = (pp_net*)ctx->net;
    if (mode == 0 && (net->eff_prec != 0 || net->up16))
        return pp_fail(ctx, PP_E_ARG, "pp_backbone_taps: fp32 mode only (in the 16-bit modes the level buffers may hold fp16)");
    if (mode != 0)
        if (int rc0 = pp_mp_mode_check(ctx, who, mode)) return rc0;
    for (int b = 0; b < 3; ++b) { net->unit_tap[b] = units ? units[b] : nullptr; net->z_tap[b] = z ? z[b] : nullptr; }
    int rc = pp_backbone(ctx, canvas, rpn_out, stream_);
    for (int b = 0; b < 3; ++b) net->unit_tap[b] = net->z_tap[b] = nullptr;
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    float* dst[3] = {x1, x2, x3};
    for (int b = 0; b < 3; ++b)
        PP_HIP(hipMemcpyAsync(dst[b], net->tap[b], (size_t)kC[b] * (ctx->H >> b) * (ctx->W >> b) * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

extern "C" int pp_backbone_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, void* stream_)
{
    return backbone_taps(ctx, "pp_backbone_taps", nullptr, canvas, rpn_out, x1, x2, x3, nullptr, nullptr, stream_);
}

// level 2's unit inputs
extern "C" int pp_backbone_block_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* units, void* stream_)
{
    float* const u[3] = {nullptr, nullptr, units};
    return backbone_taps(ctx, "pp_backbone_block_taps", units ? nullptr : "pp_backbone_block_taps", canvas, rpn_out, x1, x2, x3, u, nullptr, stream_);
}

// and the raw output of level 2's strided conv
extern "C" int pp_backbone_stage_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* units, float* z3,
                                      void* stream_)
{
    float* const u[3] = {nullptr, nullptr, units};
    float* const z[3] = {nullptr, nullptr, z3};
    const char* null_in = !z3 ? "pp_backbone_stage_taps" : !units ? "pp_backbone_block_taps" : nullptr;
    return backbone_taps(ctx, "pp_backbone_stage_taps", null_in, canvas, rpn_out, x1, x2, x3, u, z, stream_);
}

// every level's hooks at once: units[b] f32[3 | 5 | 5][C_b][H>>b][W>>b], z[b] f32[C_b][H>>b][W>>b]
extern "C" int pp_backbone_train_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* const* units,
                                      float* const* z, void* stream_)
{
    bool null = !units || !z;
    for (int b = 0; b < 3 && !null; ++b) null = !units[b] || !z[b];
    return backbone_taps(ctx, "pp_backbone_train_taps", null ? "pp_backbone_train_taps" : nullptr, canvas, rpn_out, x1, x2, x3, units, z, stream_);
}

// pp_backbone_train_taps on a plan committed in 16-bit mode `mode`: the taps are the fp32 activations of that 16-bit forward
extern "C" int pp_backbone_train_taps_mp(pp_ctx* ctx, int mode, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3,
                                         float* const* units, float* const* z, void* stream_)
{
    bool null = !units || !z;
    for (int b = 0; b < 3 && !null; ++b) null = !units[b] || !z[b];
    return backbone_taps(ctx, "pp_backbone_train_taps_mp", null ? "pp_backbone_train_taps_mp" : nullptr, canvas, rpn_out, x1, x2, x3, units, z, stream_,
                         mode);
}

// The lock-step training forward of the BatchNorm backbone: the dense backbone layer by layer over all nb frames, every BatchNorm2d
// normalising with the statistics of the batch.  gamma_beta: the 38 device pointers (weight, bias) of the nineteen layers in
// state_dict order.  Outputs (caller memory): rpn_out [nb][320][H][W]; x1 .. x3 [nb][C_b][H>>b][W>>b]; units[b] [3 | 5 | 5][nb][C_b][H>>b][W>>b]
// (a unit's frames together) and z[b] [nb][C_b][H>>b][W>>b] (either array, or any entry, may be null: a tap nobody needs); mean, var (biased), scale, shift
// f32[19][256] in the same layer order, a row filled up to its layer's channels.  The committed fold of the running statistics is not
// touched: inference between steps sees what it saw.
extern "C" int pp_backbone_train_taps_bn(pp_ctx* ctx, const float* canvas, int nb, const float* const* gamma_beta, float* rpn_out, float* x1,
                                         float* x2, float* x3, float* const* units, float* const* z, float* mean, float* var, float* scale,
                                         float* shift, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone_train_taps_bn: weights not committed");
    if (ctx->cfg.norm_kind != 1) return pp_fail(ctx, PP_E_ARG, "pp_backbone_train_taps_bn: the BatchNorm backbone only");
    if (!canvas || !gamma_beta || !rpn_out || !x1 || !x2 || !x3 || !mean || !var || !scale || !shift)
        return pp_fail(ctx, PP_E_ARG, "pp_backbone_train_taps_bn: null pointer");
    for (int i = 0; i < 38; ++i)
        if (!gamma_beta[i] || ((uintptr_t)gamma_beta[i] & 3))
            return pp_fail(ctx, PP_E_ARG, "pp_backbone_train_taps_bn: null or misaligned weight / bias pointer");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_backbone_train_taps_bn: nb must be 1 .. max_batch");
    pp_net* net = (pp_net*)ctx->net;
    if (net->eff_prec != 0 || net->up16)
        return pp_fail(ctx, PP_E_ARG, "pp_backbone_train_taps_bn: fp32 mode only (in the 16-bit modes the level buffers may hold fp16)");
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    if (int rc0 = pp_head_materialise(ctx, stream)) return rc0; // the concat buffer is about to be overwritten
    if (!net->bnp_scale) PP_HIP(hipMalloc((void**)&net->bnp_scale, (size_t)24 * 320 * sizeof(float)));
    if (!net->bnp_shift) PP_HIP(hipMalloc((void**)&net->bnp_shift, (size_t)24 * 320 * sizeof(float)));
    net->bn_pass = true;
    net->bnp_gb = gamma_beta;
    net->bnp_out[0] = mean; net->bnp_out[1] = var; net->bnp_out[2] = scale; net->bnp_out[3] = shift;
    for (int b = 0; b < 3; ++b) { net->unit_tap[b] = units ? units[b] : nullptr; net->z_tap[b] = z ? z[b] : nullptr; }
    int rc = pp_run_backbone(ctx, canvas, nb, stream, nullptr, nullptr);
    const int HW = ctx->H * ctx->W;
    if (!rc) rc = launch_norm_relu(ctx, net->up, rpn_out, 320, HW, norm_ref(ctx, 7, 320, 0, (size_t)HW), nullptr, stream, nb, 0);
    net->bn_pass = false;
    net->bnp_gb = nullptr;
    for (int b = 0; b < 3; ++b) net->unit_tap[b] = net->z_tap[b] = nullptr;
    if (rc) return rc;
    float* dst[3] = {x1, x2, x3};
    for (int b = 0; b < 3; ++b)
        PP_HIP(hipMemcpyAsync(dst[b], net->tap[b], (size_t)nb * kC[b] * (ctx->H >> b) * (ctx->W >> b) * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}
