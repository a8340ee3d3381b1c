// 2D backbone (RPN) + shared head: the host side.  The MFMA kernels live one family per file -- conv_direct.hip (conv_mfma),
// wino2.hip (wino_mfma), wino4.hip (wino4_mfma), gemm1x1.hip (gemm1x1), conv16.hip and wino6.hip -- and export their tilings as
// menu functions through conv_common.h.  This file holds everything that is per network and not per kernel: the layer table
// (Layer, NormRef, pp_net), layer_menu (the families' menus composed per layer shape and precision), the per-family rules of the
// tuner and the launcher, the weight packer (pack_layer: every family's image, read back as a map by the training code), launch_conv,
// the tuner and its cache, create / commit / run, the C ABI and the debug and profile hooks.  Its own kernels are the five small
// ones around the layers: norm_relu_stats, norm_finalize, f32_to_f16, fill_pattern and dbg_reduce_stats.
#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include "pp_common.h"
#include "conv_common.h"

namespace {

using namespace ppc;

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

// ------------------------------------------------------------------------------------------
// network description, weight packing, launch plans
// ------------------------------------------------------------------------------------------
struct Layer {
    std::string wkey;
    int kind;   // 0 conv3x3, 1 deconv(up), 2 head
    int cin, cout, stride, up;
    int level;  // pixel grid of the GEMM: 0 = H,W ; 1 = H/2 ; 2 = H/4 (input grid for deconv)
    Variant var;
    float* w = nullptr; // packed device weights
    size_t w_bytes = 0; // size of that image (pack_layer)
    int rows = 0;       // GEMM rows (virtual channels)
};

struct NormRef { // where a consumer finds the producer's normalisation
    int mode = PRE_RAW;
    double* acc = nullptr;
    float* scale = nullptr;
    float* shift = nullptr;
    int C = 0;
    double inv_n = 0.0;
    size_t fs = 0; // doubles between frames of `acc`
    size_t aff_fs = 0; // floats between frames of `scale` / `shift` (0: shared by all frames)
};

struct pp_net {
    std::vector<Layer> layers; // 16 convs, 3 deconvs, head in execution order
    float* buf[3][4] = {};     // per level: 4 activation buffers [C,H,W]
    float* up = nullptr;       // [320,H,W] pre-norm upsampled maps (concat)
    double* stats = nullptr;   // all statistics accumulators, one memset per frame
    float* aff = nullptr;      // [max_batch][2][320] (scale, shift) of the layer about to run (norm_finalize)
    size_t stats_bytes = 0;
    float* bn_scale = nullptr; // BatchNorm variant: all folded (scale, shift) arrays
    float* bn_shift = nullptr;
    float* head_bias = nullptr;
    float* head_bias_perm = nullptr; // head bias in gemm1x1's row order (head_tile_row)
    float* ones = nullptr;
    float* zeros = nullptr;
    int num_cu = 256;
    int eff_prec = 0;   // the precision the launch plan is built for: ctx->precision, except 4 -> 3 when the concat buffer cannot be fp16
    bool up16 = false;  // pp_set_precision 4 with every layer on a 16-bit-tensor tiling: the level buffers and the concat buffer `up` hold fp16
    bool defer_ok = false; // the committed plan can run the deferred head: fp32 mode, 9-anchor head on a gemm1x1 tiling
    Variant cls_var;       // tiling of the cls-only head pass (chosen at pp_commit_weights when defer_ok)
    const float* tap[3] = {}; // block outputs of the last pp_run_backbone pass (what the three upsamplers read): pp_backbone_taps
    // copy hooks of the tap entry points, one per level b (null: inert; armed for one single-frame pass):
    float* unit_tap[3] = {}; // caller memory f32[n_b][C_b][H>>b][W>>b] for the inputs of block b + 1's units (n_b = 3, 5, 5); pp_backbone_block_taps arms level 2
    float* z_tap[3] = {};    // caller memory f32[C_b][H>>b][W>>b] for the raw output of level b's strided conv; pp_backbone_stage_taps arms level 2
    double* dbg_stats = nullptr; // statistics accumulators of pp_debug_layer (allocated on its first call that asks for statistics)
    int w4_strips = -1; // PP_W4_STRIPS, read once at pp_create: -1 cost model, 0 never, 2 whenever whole main tiles exist (parity tests of the strip tiles)
};

const int kC[3] = {64, 128, 256};

// The tilings a layer may run, composed from what the families export (conv_common.h).  Content and order are part of the plan: the
// order decides menu[0], the tuner's ties and what PP_AUTOTUNE=0 takes, and menu.size() is in the tune-cache key (autotune_layer).
void layer_menu(int kind, int stride, int up, std::vector<Variant>& menu, int cin = 0, bool roofline_layer = false, bool head9 = true, int prec = 0,
                bool first_conv = false)
{
    const bool g1ok = cin % 32 == 0; // gemm1x1 runs K in rings of 8 quad-steps without a tail
    // reduced-precision modes (pp_set_precision): the 1x1 contractions -- the three ConvTranspose(k = s) upsamplers and the
    // 9-anchor head -- run their bf16x3 / bf16 / fp16 gemm1x1 tilings, the 3x3 convolutions the 16-bit operand kernels of
    // conv16.hip.  A layer whose shape none of them takes (autotune_layer checks variant_ok / shape_ok) falls back to the
    // fp32 menu below, and pp_layer_tilings shows it.
    if (prec && g1ok && (kind == 1 || (kind == 2 && head9))) {
        gemm1x1_menu(kind, up, prec, menu);
        return;
    }
    if (prec && kind == 0 && cin % 16 == 0) {
        // fp16s: the fp16-operand kernels on fp16 tensors; the first conv reads the fp32 PFN rows / canvas and writes fp16
        if (prec == 4) conv16_menu(stride, 3, menu, first_conv ? 2 : 3);
        else conv16_menu(stride, prec, menu);
        return;
    }
    if (kind == 2) {
        // the persistent 1x1 GEMM's head epilogue (head_tile_row) is laid out for the reference's 9 anchors per location
        if (g1ok && head9) gemm1x1_menu(kind, up, 0, menu);
        conv_direct_menu(kind, stride, up, menu);
    } else if (kind == 1) {
        conv_direct_menu(kind, stride, up, menu);
        if (g1ok) gemm1x1_menu(kind, up, 0, menu);
    } else {
        conv_direct_menu(kind, stride, up, menu);
        if (stride != 2) {
            wino2_menu(menu, roofline_layer);
            wino4_menu(menu, roofline_layer);
            if (cin % 32 == 0) wino6_menu(menu, roofline_layer); // Winograd F(4x4,3x3), 16x16 px (wino6.hip)
        }
    }
}

// strip tilings of wino4 / wino6 (launch_conv): a map that is not a multiple of the main tile (16x16 px) is covered by whole main
// tiles plus a right strip of 4 x 64 px tiles and a bottom strip of 64 x 4 px tiles -- 100 x 100: 36 + 2 + 2 tiles instead of
// 49 mostly-empty ones
static const Variant& strip_v(Family f) // 4 px wide, 64 px tall
{
    static const Variant w4 = wino4_strip_v(), w6 = wino6_strip_v();
    return f == Family::Wino6 ? w6 : w4;
}
static const Variant& strip_h(Family f) // 64 px wide, 4 px tall
{
    static const Variant w4 = wino4_strip_h(), w6 = wino6_strip_h();
    return f == Family::Wino6 ? w6 : w4;
}

// cost model: wavefronts are dealt to 1024 SIMDs; a SIMD's time ~ (its wave count) x (tile pairs per wave).
double model_cost(const Variant& v, int rows, int Hout, int Wout)
{
    const double blocks = (double)pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph) * pp_div_up(rows, v.bm);
    const double waves = blocks * v.waves;
    double cost = std::ceil(waves / 1024.0) * v.pairs;
    if (waves < 1536.0) cost *= 1.15;          // a lone wave per SIMD cannot hide its own staging
    cost *= 1.0 + 0.02 * (20.0 / v.pairs);     // smaller wave tiles re-read operands more often
    return cost;
}

// ---- the per-family rules of the tuner and the launcher ----
// rows: wino4, conv16 and wino6 tile whole row blocks; the others clip their last block
bool variant_ok(const Variant& v, int rows)
{
    switch (v.family) {
    case Family::Wino4:
    case Family::Conv16:
    case Family::Wino6: return rows % v.bm == 0;
    default: return v.bm <= ((rows + 63) / 64) * 64;
    }
}
// shape limits of a tiling family
bool shape_ok(const Variant& v, int Hin, int Win, int Wout)
{
    switch (v.family) {
    case Family::Wino4: return !(Wout & 1); // float2 row stores (even output width)
    // gemm1x1 feeds four N-tiles from one dwordx4 of 4 consecutive pixels of the input plane (pixel count a multiple of 4 -- a
    // 9 x 11 map has 99); with a 16-bit tensor it has no path for maps that are not a multiple of 4 wide
    case Family::Gemm1x1: return !((Hin * Win) & 3) && !(v.io16 && (Wout & 3));
    // conv16 fetches its patches as aligned pixel quads and stores pixel quads (input and output width multiples of 4)
    case Family::Conv16: return !((Win & 3) || (Wout & 3));
    // wino6 works on whole 4x4 output tiles and dwordx4 rows (maps a multiple of 4 in both directions; stride 1: Hin = Hout)
    case Family::Wino6: return !((Wout & 3) || (Hin & 3));
    default: return true;
    }
}
// LDS bytes of a launch of v on a layer with cin input channels (gemm1x1 keeps the whole [K][BM] weight slab)
size_t layer_lds(const Variant& v, int cin) { return v.family == Family::Gemm1x1 ? g1_lds(v, cin) : v.lds; }
// One frame per launch: the families that finalise the producer's statistics in their own prologue, instead of a norm_finalize
// launch in front of the layer -- 14 launches of 4.7 us + a boundary each per frame at batch 1.  (Batched launches keep
// norm_finalize: a persistent workgroup would redo the fp64 finalisation at every frame change.)
bool finalises_in_prologue(Family f)
{
    switch (f) {
    case Family::Direct:
    case Family::Gemm1x1:
    case Family::Wino4:
    case Family::Wino6: return true;
    default: return false;
    }
}
// MFMA flops a tiling executes per algorithmic flop of the direct convolution
double executed_ratio(const Variant& v)
{
    switch (v.family) {
    case Family::Wino6: return 0.25;
    case Family::Wino:
    case Family::Wino4: return 4.0 / 9.0;
    case Family::Conv16: return v.prec == 1 ? 3.0 : 1.0; // bf16x3: three MFMAs per product
    default: return 1.0;
    }
}

Variant pick_variant(int kind, int stride, int up, int rows, int Hout, int Wout, bool head9 = true)
{
    std::vector<Variant> menu;
    layer_menu(kind, stride, up, menu, 0, false, head9, 0);
    double best = 1e30;
    Variant bv = menu[0];
    for (const Variant& v : menu) {
        if (!variant_ok(v, rows) || (v.family != Family::Direct && v.family != Family::Wino)) continue; // persistent kernels are only chosen by measurement
        const double c = model_cost(v, rows, Hout, Wout);
        if (c < best) { best = c; bv = v; }
    }
    // Without on-device tuning (PP_AUTOTUNE=0) prefer what the tuner settles on for these layer kinds on MI355X;
    // the cost model above only ranks the direct tilings.
    const char* prefer = (kind == 0 && stride == 1) ? "wino tw8 w1x4 bx1 kc8"
                         : (kind == 1 && up == 2)   ? "g1x1 m4 n4 e1"
                         : (kind == 1 && up == 4)   ? "g1x1 m4 n4 e2"
                         : (kind == 2 && head9)     ? "g1x1 m6 n4 e3"
                                                    : nullptr;
    if (prefer)
        for (const Variant& v : menu)
            if (variant_ok(v, rows) && shape_ok(v, Hout, Wout, Wout) && !strcmp(v.name, prefer)) return v;
    return bv;
}

// Row order of the head inside gemm1x1.  A lane of the 16x16 MFMA tile owns 4 CONSECUTIVE tile rows (kq*4 + r), so
// the 90 head rows are dealt to the 24 four-row groups such that a group's values are adjacent in the output:
//   groups 0..8   box (a = g)      k = 0..3                      -> one 16-byte store per pixel
//   groups 9..17  box (a = g - 9)  k = 4..6, then cls(a)         -> one 12-byte store per pixel + cls as a pixel quad
//   groups 18..22 dir (a = 2d, 2d+1), both logits each           -> two 8-byte stores per pixel
//   group 23      padding
// (natural order: cls 0..8, box 9 + 7a + k, dir 72 + 2a + k, head rows 90..95 are zero).  With the natural order
// the 81 box/dir rows cost 4 scalar stores each per lane -- 333 scattered store instructions per 64 pixels, whose
// completion the next item's first loads had to wait for (vmcnt is in order): 38 % of the head's wave time.
// GEMM rows of the head for na anchors per location: cls na | box 7 na | dir 2 na, padded to whole 96-row blocks (the
// head tilings are 96 rows tall; the reference's 9 anchors give 90 -> 96)
static inline int head_rows(int na) { return ((10 * na + 95) / 96) * 96; }

static inline int head_tile_row(int t)
{
    const int g = t >> 2, r = t & 3;
    if (g < 9) return 9 + 7 * g + r;
    if (g < 18) return r < 3 ? 9 + 7 * (g - 9) + 4 + r : (g - 9);
    if (g < 23) {
        const int a = 2 * (g - 18) + (r >> 1);
        return a < 9 ? 72 + 2 * a + (r & 1) : -1;
    }
    return -1;
}

// index_positions: the transform (U = G g G^T of the Winograd families, the identity elsewhere) is replaced by position indices --
// element k of the transformed [rows][cin][taps_eff] array holds the float k + 1 -- so the image that comes out is the layout alone
// (layer_position_map); conv3x3 layers on fp32 tilings only
int pack_layer(pp_ctx* ctx, Layer& L, bool index_positions = false)
{
    const Variant& v = L.var;
    const int ks = (L.kind == 0) ? 3 : 1;
    const int taps = ks * ks;
    auto it = ctx->host_w.find(L.wkey);
    std::vector<float> rowsW; // [rows][cin][taps]
    int rows = 0;
    if (L.kind == 0) {
        if (it == ctx->host_w.end() || (int64_t)it->second.data.size() != (int64_t)L.cout * L.cin * 9)
            return pp_fail(ctx, PP_E_NAME, ("missing/mis-shaped weight " + L.wkey).c_str());
        rows = L.cout;
        rowsW = it->second.data; // [cout][cin][3][3]
    } else if (L.kind == 1) {
        const int u2 = L.up * L.up;
        if (it == ctx->host_w.end() || (int64_t)it->second.data.size() != (int64_t)L.cin * L.cout * u2)
            return pp_fail(ctx, PP_E_NAME, ("missing/mis-shaped weight " + L.wkey).c_str());
        rows = L.cout * u2; // ConvTranspose weight [cin][cout][k][k] -> row (co*u2 + dy*u + dx)
        rowsW.resize((size_t)rows * L.cin);
        const std::vector<float>& s = it->second.data;
        for (int ci = 0; ci < L.cin; ++ci)
            for (int co = 0; co < L.cout; ++co)
                for (int d = 0; d < u2; ++d) rowsW[((size_t)co * u2 + d) * L.cin + ci] = s[((size_t)ci * L.cout + co) * u2 + d];
    } else {
        const int na = ctx->cfg.num_anchor_per_loc;
        rows = head_rows(na);
        rowsW.assign((size_t)rows * L.cin, 0.f);
        const char* names[3] = {"heads.conv_cls.weight", "heads.conv_box.weight", "heads.conv_dir.weight"};
        const int cnt[3] = {na, 7 * na, 2 * na};
        int r0 = 0;
        for (int h = 0; h < 3; ++h) {
            auto w = ctx->host_w.find(names[h]);
            if (w == ctx->host_w.end() || (int64_t)w->second.data.size() != (int64_t)cnt[h] * L.cin)
                return pp_fail(ctx, PP_E_NAME, (std::string("missing/mis-shaped weight ") + names[h]).c_str());
            memcpy(&rowsW[(size_t)r0 * L.cin], w->second.data.data(), sizeof(float) * cnt[h] * L.cin);
            r0 += cnt[h];
        }
    }
    L.rows = rows;
    auto upload = [&](const void* image, size_t bytes) -> int { // the finished image replaces the layer's device copy
        if (L.w) (void)hipFree(L.w);
        PP_HIP(hipMalloc((void**)&L.w, bytes));
        L.w_bytes = bytes;
        PP_HIP(hipMemcpy(L.w, image, bytes, hipMemcpyHostToDevice));
        return 0;
    };
    if (v.family == Family::Wino6) { // F(4x4,3x3): U = G g G^T in the order the four waves fetch their positions (wino6.hip)
        std::vector<float> pk6;
        wino6_pack(rowsW.data(), rows, L.cin, pk6, index_positions);
        return upload(pk6.data(), pk6.size() * sizeof(float));
    }
    int taps_eff = taps;
    if (v.family == Family::Wino || v.family == Family::Wino4) { // U = G g G^T per (cout, cin), fp64 on the host; position xi = 4*a + b
        static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
        std::vector<float> u((size_t)rows * L.cin * 16);
        for (size_t rc = 0; rc < (size_t)rows * L.cin; ++rc) {
            const float* g = &rowsW[rc * 9];
            double t[4][3];
            for (int a = 0; a < 4; ++a)
                for (int j = 0; j < 3; ++j) t[a][j] = G[a][0] * g[0 * 3 + j] + G[a][1] * g[1 * 3 + j] + G[a][2] * g[2 * 3 + j];
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) u[rc * 16 + a * 4 + b] = (float)(t[a][0] * G[b][0] + t[a][1] * G[b][1] + t[a][2] * G[b][2]);
        }
        rowsW.swap(u);
        taps_eff = 16;
    }
    if (index_positions)
        for (size_t k = 0; k < rowsW.size(); ++k) rowsW[k] = (float)(k + 1);
    if (v.family == Family::Gemm1x1 && L.kind == 2) { // head under gemm1x1: rows in head_tile_row order
        std::vector<float> perm((size_t)96 * L.cin, 0.f);
        for (int t = 0; t < 96; ++t) {
            const int src = head_tile_row(t);
            if (src >= 0) memcpy(&perm[(size_t)t * L.cin], &rowsW[(size_t)src * L.cin], sizeof(float) * L.cin);
        }
        rowsW.swap(perm);
    }
    // bf16 images (conv16, gemm1x1): round to nearest even, and back
    auto bf16 = [](float f) -> uint16_t { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); };
    auto bf16f = [](uint16_t h) -> float { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
    if (v.family == Family::Conv16) { // conv16: [row block][cin/16][image: hi (| lo for bf16x3)][tap][k-half][BM rows][8 x 16 bit] = the LDS image of a step
        auto f16 = [](float f) -> uint16_t { const _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }; // round to nearest even
        const int nimg = (v.prec == 1) ? 2 : 1, nblk = rows / v.bm, nch = L.cin / 16;
        std::vector<uint16_t> pk((size_t)nblk * nch * nimg * 9 * 2 * v.bm * 8, 0);
        for (int b = 0; b < nblk; ++b)
            for (int ch = 0; ch < nch; ++ch)
                for (int t = 0; t < 9; ++t)
                    for (int h = 0; h < 2; ++h)
                        for (int mm = 0; mm < v.bm; ++mm)
                            for (int j = 0; j < 8; ++j) {
                                const float w = rowsW[((size_t)(b * v.bm + mm) * L.cin + ch * 16 + h * 8 + j) * 9 + t];
                                const size_t o = (((size_t)(t * 2 + h)) * v.bm + mm) * 8 + j;
                                const size_t img0 = (((size_t)b * nch + ch) * nimg) * (size_t)(9 * 2 * v.bm * 8);
                                if (v.prec == 3) pk[img0 + o] = f16(w);
                                else {
                                    const uint16_t hi = bf16(w);
                                    pk[img0 + o] = hi;
                                    if (nimg == 2) pk[img0 + (size_t)(9 * 2 * v.bm * 8) + o] = bf16(w - bf16f(hi));
                                }
                            }
        return upload(pk.data(), pk.size() * sizeof(uint16_t));
    }
    if (v.family == Family::Gemm1x1 && v.prec) { // [row block][K/16][hi|lo][k-group][BMP][4 bf16]: the byte count of the fp32 slab
        const int nb_ = pp_div_up(rows, v.bm), nkb = L.cin / 16;
        std::vector<uint16_t> pk4((size_t)nb_ * nkb * 2 * 4 * v.bmp * 4, 0);
        for (int b = 0; b < nb_; ++b)
            for (int kb = 0; kb < nkb; ++kb)
                for (int q = 0; q < 4; ++q)
                    for (int mm = 0; mm < v.bm; ++mm) {
                        const int row = b * v.bm + mm;
                        if (row >= rows) continue;
                        for (int t = 0; t < 4; ++t) {
                            const float w = rowsW[(size_t)row * L.cin + kb * 16 + q * 4 + t];
                            uint16_t hi = bf16(w);
                            if (v.prec == 3) { const _Float16 h16 = (_Float16)w; memcpy(&hi, &h16, 2); } // fp16 operands: the hi image alone is used
                            const uint16_t lo = bf16(w - bf16f(hi));
                            pk4[(((((size_t)b * nkb + kb) * 2 + 0) * 4 + q) * v.bmp + mm) * 4 + t] = hi;
                            pk4[(((((size_t)b * nkb + kb) * 2 + 1) * 4 + q) * v.bmp + mm) * 4 + t] = lo;
                        }
                    }
        return upload(pk4.data(), pk4.size() * sizeof(uint16_t));
    }
    if (v.family == Family::Gemm1x1) { // [row block][K][BMP]
        const int nb_ = pp_div_up(rows, v.bm);
        std::vector<float> pk3((size_t)nb_ * L.cin * v.bmp, 0.f);
        for (int b = 0; b < nb_; ++b)
            for (int c = 0; c < L.cin; ++c)
                for (int mm = 0; mm < v.bm; ++mm) {
                    const int row = b * v.bm + mm;
                    if (row < rows) pk3[((size_t)b * L.cin + c) * v.bmp + mm] = rowsW[(size_t)row * L.cin + c];
                }
        return upload(pk3.data(), pk3.size() * sizeof(float));
    }
    const int nblk = pp_div_up(rows, v.bm), nchunk = L.cin / v.kc;
    std::vector<float> pk((size_t)nblk * nchunk * taps_eff * v.kc * v.bmp, 0.f); // LDS image incl. row padding
    for (int b = 0; b < nblk; ++b)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int t = 0; t < taps_eff; ++t)
                for (int k = 0; k < v.kc; ++k)
                    for (int mm = 0; mm < v.bm; ++mm) {
                        const int row = b * v.bm + mm;
                        if (row >= rows) continue;
                        // Winograd image: row = [wm][m][M-tile] so a lane's two A operands are adjacent (ds_read_b64)
                        // wino4 image: row = [m][M-tile 0..3] so a lane's four A operands are one ds_read_b128
                        const int col = (v.family == Family::Wino) ? ((mm >> 5) * 32 + (mm & 15) * 2 + ((mm >> 4) & 1)) : (v.family == Family::Wino4) ? ((mm & 15) * 4 + (mm >> 4)) : mm;
                        pk[((((size_t)b * nchunk + ch) * taps_eff + t) * v.kc + k) * v.bmp + col] =
                            rowsW[((size_t)row * L.cin + ch * v.kc + k) * taps_eff + t];
                    }
    return upload(pk.data(), pk.size() * sizeof(float));
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

constexpr size_t STAT_FS = (size_t)24 * NREP * 320 * 2; // doubles of statistics per frame

int launch_conv(pp_ctx* ctx, const Layer& L, const float* in, int Hin, int Win, float* out, const float* res,
                const NormRef& pre, double* stat_acc, int stat_C, int Hout, int Wout, hipStream_t stream,
                float* out_box = nullptr, float* out_dir = nullptr, int B = 1, size_t out_fs = 0, size_t in_fs = 0,
                const int32_t* pmap = nullptr, const float* feat = nullptr, int ts_k = 0)
{
    pp_net* net = (pp_net*)ctx->net;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.in = in; p.w = L.w; p.out = out; p.res = res;
    p.Cin = L.cin; p.Hin = Hin; p.Win = Win;
    p.Cout = L.rows; p.Hout = Hout; p.Wout = Wout;
    p.pre = pre.mode; p.pre_acc = pre.acc; p.pre_scale = pre.scale; p.pre_shift = pre.shift;
    p.pre_inv_n = pre.inv_n; p.eps = 1e-3f; p.aff_fs = pre.aff_fs;
    p.stat_acc = stat_acc; p.stat_C = stat_C;
    p.bias = (L.kind == 2 && L.var.family == Family::Gemm1x1) ? net->head_bias_perm : net->head_bias; p.out_box = out_box; p.out_dir = out_dir;
    { const int na = ctx->cfg.num_anchor_per_loc; p.n_cls = na; p.n_box = 7 * na; p.n_rows = 10 * na; }
    p.w_bm = net->layers.back().var.bm; p.w_bmp = net->layers.back().var.bmp;
    {   // frame strides of a batched launch (every per-frame tensor is stored [B][...])
        const size_t hw = (size_t)Hout * Wout;
        p.in_fs = in_fs ? in_fs : (size_t)L.cin * Hin * Win;
        p.out_fs = out_fs ? out_fs : (L.kind == 2 ? (size_t)p.n_cls * hw : (size_t)L.rows * hw);
        p.res_fs = p.out_fs;
        p.box_fs = (size_t)p.n_box * hw;
        p.dir_fs = (size_t)2 * p.n_cls * hw;
        p.pre_fs = pre.fs;
        p.stat_fs = STAT_FS;
        p.pmap = pmap; p.feat = feat;
        p.pmap_fs = (size_t)Hin * Win;
        p.feat_fs = (size_t)ctx->cfg.max_voxels * 64;
    }
    const bool fin_in_kernel = B == 1 && finalises_in_prologue(L.var.family);
    if (pre.mode == PRE_STATS && net->aff && L.cin <= 320 && !fin_in_kernel) {
        hipLaunchKernelGGL(norm_finalize, dim3(B), dim3(320), 0, stream, pre.acc, pre.fs, L.cin, pre.inv_n, p.eps, net->aff, (size_t)640);
        p.pre = PRE_AFFINE; p.pre_scale = net->aff; p.pre_shift = net->aff + 320; p.aff_fs = 640;
    }
    const Variant& v = L.var;
    // profile bracket (pp_profile_begin) of the level-0 stride-1 layers: one event pair around the layer's launches, and its flops
    const bool tag = ctx->prof_on && L.kind == 0 && L.level == 0 && L.stride == 1;
    auto prof_begin = [&]() -> int {
        if (!tag) return 0;
        if (ctx->prof_used + 2 > ctx->prof_ev.size()) {
            hipEvent_t a, b;
            PP_HIP(hipEventCreate(&a));
            PP_HIP(hipEventCreate(&b));
            ctx->prof_ev.push_back(a);
            ctx->prof_ev.push_back(b);
        }
        ctx->prof_flops = 2.0 * Hout * Wout * (double)L.cin * L.cout * 9.0 * B;
        PP_HIP(hipEventRecord(ctx->prof_ev[ctx->prof_used], stream));
        return 0;
    };
    auto prof_end = [&]() -> int {
        if (!tag) return 0;
        PP_HIP(hipEventRecord(ctx->prof_ev[ctx->prof_used + 1], stream));
        ctx->prof_used += 2;
        return 0;
    };
    dim3 grid(pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph), pp_div_up(L.rows, v.bm), B);
    p.nb = B;
    const size_t lds_bytes = layer_lds(v, L.cin);
    if (v.family == Family::Gemm1x1 && ((Hin * Win) & 3)) return PP_E_ARG; // gemm1x1 reads pixel quads (choose_variant never offers it for such a plane)
    if (v.family == Family::Gemm1x1) { // persistent: one workgroup per CU, a multiple of the row-block count
        const int ncb = pp_div_up(L.rows, v.bm);
        int g = (net->num_cu * v.wpc / ncb) * ncb;
        if (g < ncb) g = ncb;
        grid = dim3(g, 1, 1);
    }
    if (v.family == Family::Conv16) { // conv16: persistent, one 4-wave workgroup per CU, XCD-contiguous item ranges (grid a multiple of 8)
        if ((size_t)L.rows * Hout * Wout * 4 >= 0x80000000ull || (size_t)L.cin * Hin * Win * 4 >= 0x80000000ull) return PP_E_ARG; // buffer offsets are 32-bit, idle lanes park 2 GB out
        if (p.pre == PRE_STATS) return pp_fail(ctx, PP_E_STATE, "conv16: the producer's statistics must be finalised to (scale, shift)");
        if ((Win & 3) || (Wout & 3) || (L.cin & 15) || (L.rows % v.bm)) return PP_E_ARG;
        const int total = pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph) * (L.rows / v.bm) * B;
        int g = net->num_cu * (v.waves * 64 / v.threads); // workgroups per CU the variant is built for

        if (g > total) g = total;
        g = (g + 7) & ~7;
        grid = dim3(g, 1, 1);
    }
    if (v.family == Family::Wino4 || v.family == Family::Wino6) {
        // persistent, ONE 4-wave workgroup per CU (512 registers per lane, 3-deep LDS ring), a multiple of the 8 XCDs.
        // Whole main tiles first; what they leave uncovered goes to strip launches of thin tiles when that needs fewer tiles
        // than rounding the main grid up (same weight image: it depends on the 64-row block and the chunk only).
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
        if (tag) {
            const double dense = (double)(Wout / v.pw) * (Hout / v.ph) * ncb * B;
            ctx->prof_items_dense += dense;
            if (listed) ctx->prof_ts_layer.push_back(ts_k | (ncb << 8)); else ctx->prof_items += dense;
        }
        if (int rc = prof_begin()) return rc;
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
                if (int rc = pp_ts_fill(ctx, ts_k, B, out, p.out_fs, L.rows, stream)) return rc;
        }
        if (int rc = prof_end()) return rc;
        PP_HIP(hipGetLastError());
        return 0;
    }
    if (v.family == Family::Wino) { // persistent Winograd: two workgroups per CU (LDS and registers allow exactly two), a multiple of the 8 XCDs
        const int total = (int)grid.x * (int)grid.y * B;
        int g = (v.threads >= 512 ? 1 : 2) * net->num_cu; // 8-wave workgroups fill a CU's registers alone
        if (g > total) g = total;
        g = (g + 7) & ~7;
        grid = dim3(g, 1, 1);
    }
    if (int rc = prof_begin()) return rc;
    hipLaunchKernelGGL((pmap && v.kern2) ? v.kern2 : v.kern, grid, dim3(v.threads), lds_bytes, stream, p);
    if (int rc = prof_end()) return rc;
    PP_HIP(hipGetLastError());
    return 0;
}


__global__ void __launch_bounds__(256) f32_to_f16(const float* __restrict__ x, _Float16* __restrict__ y, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = (_Float16)x[i];
}

__global__ void __launch_bounds__(256) fill_pattern(float* __restrict__ x, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        x[i] = (float)(h & 0xFFFF) * (1.0f / 65536.0f); // [0,1): random-looking, not zeros (zeros raise the clock)
    }
}

std::map<std::string, std::string>& tune_cache()
{
    // layer signature -> variant name, per process; PP_TUNE_CACHE=<file> persists it across processes
    static std::map<std::string, std::string> c;
    static bool loaded = false;
    if (!loaded) {
        loaded = true;
        if (const char* path = getenv("PP_TUNE_CACHE")) {
            if (FILE* f = fopen(path, "r")) {
                char line[512];
                while (fgets(line, sizeof(line), f)) {
                    char* tab = strchr(line, '\t');
                    if (!tab) continue;
                    *tab = 0;
                    char* val = tab + 1;
                    val[strcspn(val, "\r\n")] = 0;
                    c[line] = val;
                }
                fclose(f);
            }
        }
    }
    return c;
}

// Merge with what other processes wrote meanwhile, write to a temp file, rename() over the target: concurrent ranks can
// neither tear the file nor drop each other's entries (the last rename wins with a superset of what it read).
void tune_cache_save()
{
    const char* path = getenv("PP_TUNE_CACHE");
    if (!path) return;
    std::map<std::string, std::string> merged;
    if (FILE* f = fopen(path, "r")) {
        char line[512];
        while (fgets(line, sizeof(line), f)) {
            char* tab = strchr(line, '\t');
            if (!tab) continue;
            *tab = 0;
            char* val = tab + 1;
            val[strcspn(val, "\r\n")] = 0;
            merged[line] = val;
        }
        fclose(f);
    }
    for (auto& kv : tune_cache()) merged[kv.first] = kv.second;
    char tmp[1024];
    snprintf(tmp, sizeof(tmp), "%s.tmp.%d", path, (int)getpid());
    if (FILE* f = fopen(tmp, "w")) {
        for (auto& kv : merged) fprintf(f, "%s\t%s\n", kv.first.c_str(), kv.second.c_str());
        fclose(f);
        if (rename(tmp, path) != 0) remove(tmp);
    }
}

// Measure every admissible tiling of one layer on the device (1 warm-up + 3 timed launches with
// hipEvents) and keep the fastest.  Weights are really packed for each candidate, the prologue /
// statistics epilogue run as in production.
constexpr int TUNE_FRAMES = 16;         // frames per timed launch of the tuner (half the default bench pass of 32; the picks do not change beyond 16)
constexpr size_t TUNE_OUT_FS = 0, TUNE_IN_FS = 0; // 0: natural per-frame strides

int autotune_layer(pp_ctx* ctx, Layer& L, int Hin, int Win, int Hout, int Wout, float* tin, float* tout, bool verbose, bool measure = true)
{
    pp_net* net = (pp_net*)ctx->net;
    const int eprec = net->eff_prec;
    char sig[160];
    std::vector<Variant> menu;
    const int rows_ = (L.kind == 2) ? head_rows(ctx->cfg.num_anchor_per_loc) : (L.kind == 1 ? L.cout * L.up * L.up : L.cout);
    auto legal = [&](const Variant& v) {
        return variant_ok(v, rows_) && shape_ok(v, Hin, Win, Wout) && layer_lds(v, L.cin) <= (size_t)160 * 1024;
    };
    const bool first_conv = L.kind == 0 && L.stride == 2 && L.level == 0;
    layer_menu(L.kind, L.stride, L.up, menu, L.cin, L.kind == 0 && L.stride == 1 && L.level == 0, ctx->cfg.num_anchor_per_loc == 9, eprec, first_conv);
    if (eprec) {
        // a shape none of the reduced-precision tilings takes (odd maps, Cin not a multiple of 16 / 32) runs its fp32 tilings:
        // pp_layer_tilings reports what really runs
        bool any = false;
        for (const Variant& v : menu) any = any || legal(v);
        if (!any) {
            menu.clear();
            layer_menu(L.kind, L.stride, L.up, menu, L.cin, L.kind == 0 && L.stride == 1 && L.level == 0, ctx->cfg.num_anchor_per_loc == 9, 0);
        }
    }
    if (!measure) { // no on-device tuning (PP_AUTOTUNE=0 / maps the tuner's buffers do not fit): fp32 keeps pick_variant's choice,
                    // a reduced-precision mode takes the first legal entry of its menu
        if (eprec)
            for (const Variant& v : menu)
                if (legal(v) && v.prec == (eprec == 4 ? 3 : eprec)) { L.var = v; return 0; }
        return 0;
    }
    // the key carries the library version and the menu size (an entry of another build's menu is not trusted), not the
    // device index: the GPUs of a node are identical, and ranks must be able to share rank 0's table
    snprintf(sig, sizeof(sig), "v%d m%d k%d s%d u%d c%d r%d %dx%d n%d b%d p%d", pp_version(), (int)menu.size(), L.kind, L.stride, L.up, L.cin, L.cout, Hout, Wout,
             ctx->cfg.norm_kind, ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES, eprec);
    const int rows = (L.kind == 2) ? head_rows(ctx->cfg.num_anchor_per_loc) : (L.kind == 1 ? L.cout * L.up * L.up : L.cout);
    if (const char* force = getenv("PP_FORCE_VARIANT")) { // tests: pin a tiling family by name substring; "a;b": a where a layer has one, else b
        const std::string all(force);
        for (size_t p = 0; p <= all.size();) {
            const size_t e = std::min(all.find(';', p), all.size());
            const std::string one = all.substr(p, e - p);
            for (const Variant& v : menu)
                if (variant_ok(v, rows) && shape_ok(v, Hin, Win, Wout) && strstr(v.name, one.c_str())) { L.var = v; return 0; }
            p = e + 1;
        }
    }
    auto hit = tune_cache().find(sig);
    if (hit != tune_cache().end()) {
        for (const Variant& v : menu)
            if (hit->second == v.name) { L.var = v; return 0; }
    }
    hipEvent_t e0, e1;
    PP_HIP(hipEventCreate(&e0));
    PP_HIP(hipEventCreate(&e1));
    NormRef pre;
    if (L.kind == 2 || (L.kind == 0 && L.stride == 1)) { pre.mode = PRE_AFFINE; pre.scale = net->ones; pre.shift = net->zeros; }
    double* st = (ctx->cfg.norm_kind == 0 && L.kind != 2) ? net->stats + (size_t)23 * NREP * 320 * 2 : nullptr;
    const int stC = (L.kind == 1) ? 320 : L.cout;
    // batched like production, every frame with its own buffers: a launch then streams more than the 256 MB
    // Infinity Cache holds, as in production (aliased frames would hide a tiling's HBM re-reads)
    const int tb = ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES;
    auto time_variant = [&](const Variant& v, int reps, double& out_ms) -> int {
        const size_t need = layer_lds(v, L.cin);
        L.var = v;
        PP_HIP(hipFuncSetAttribute((const void*)v.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        if (v.kern2) PP_HIP(hipFuncSetAttribute((const void*)v.kern2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        int rc = pack_layer(ctx, L);
        if (rc) return rc;
        float ms = 0.f;
        for (int it = 0; it <= reps; ++it) {
            if (it == 1) PP_HIP(hipEventRecord(e0, 0));
            rc = launch_conv(ctx, L, tin, Hin, Win, (L.kind == 2) ? ctx->f_cls : tout, nullptr, pre, st, stC, Hout, Wout, 0, ctx->f_box, ctx->f_dir, tb, TUNE_OUT_FS, TUNE_IN_FS);
            if (rc) return rc;
        }
        PP_HIP(hipEventRecord(e1, 0));
        PP_HIP(hipEventSynchronize(e1));
        PP_HIP(hipEventElapsedTime(&ms, e0, e1));
        out_ms = ms / reps;
        return 0;
    };
    // pass 1: every legal tiling, 3 timed launches
    std::vector<std::pair<double, const Variant*>> timed;
    for (const Variant& v : menu) {
        if (!variant_ok(v, rows)) continue;
        if (!shape_ok(v, Hin, Win, Wout)) continue;
        const size_t need = layer_lds(v, L.cin);
        if (need > 160 * 1024) continue;
        double ms;
        int rc = time_variant(v, 3, ms);
        if (rc) return rc;
        if (verbose) fprintf(stderr, "[pp autotune] %-28s %-34s %8.1f us\n", sig, v.name, ms * 1e3);
        timed.push_back({ms, &v});
    }
    if (timed.empty()) return pp_fail(ctx, PP_E_STATE, "autotune: no legal tiling");
    std::sort(timed.begin(), timed.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    // pass 2: the contenders within 8 % of the best are re-timed twice with 8 launches each (clocks are warm
    // by now and the order effect of pass 1 is gone); best of the three readings decides
    double best = timed[0].first;
    Variant bv = *timed[0].second;
    size_t ncont = 0;
    while (ncont < timed.size() && ncont < 4 && timed[ncont].first <= timed[0].first * 1.08) ++ncont;
    if (ncont > 1) {
        std::vector<double> score(ncont);
        for (size_t i = 0; i < ncont; ++i) score[i] = timed[i].first;
        for (int round = 0; round < 2; ++round)
            for (size_t i = 0; i < ncont; ++i) {
                double ms;
                int rc = time_variant(*timed[i].second, 8, ms);
                if (rc) return rc;
                score[i] = (round == 0) ? ms : std::min(score[i], ms); // pass-1 reading is replaced, not kept
            }
        size_t bi = 0;
        for (size_t i = 1; i < ncont; ++i)
            if (score[i] < score[bi]) bi = i;
        best = score[bi];
        bv = *timed[bi].second;
        if (verbose)
            for (size_t i = 0; i < ncont; ++i) fprintf(stderr, "[pp autotune] %-28s   retime %-26s %8.1f us\n", sig, timed[i].second->name, score[i] * 1e3);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    L.var = bv;
    tune_cache()[sig] = bv.name;
    if (verbose) fprintf(stderr, "[pp autotune] %-28s -> %s (%.1f us)\n", sig, bv.name, best * 1e3);
    return 0;
}

// The cls-only head pass as a launch: the head layer with the cls tiling and one 16-row block; the weights stay the head's image.
int launch_head_cls(pp_ctx* ctx, const Variant& v, const float* in, const NormRef& pre, float* cls, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    Layer L = net->layers.back(); // shares the device image (no ownership: Layer has no destructor)
    L.var = v;
    L.rows = 16;
    return launch_conv(ctx, L, in, ctx->H, ctx->W, cls, nullptr, pre, nullptr, 0, ctx->H, ctx->W, stream, nullptr, nullptr, nb);
}

// Shapes of the cls-only pass, timed like a layer's tilings (3 launches after a warm-up, the fastest is kept and cached).
int autotune_head_cls(pp_ctx* ctx, float* tin, bool verbose, bool measure)
{
    pp_net* net = (pp_net*)ctx->net;
    std::vector<Variant> menu;
    gemm1x1_cls_menu(menu);
    for (const Variant& v : menu)
        PP_HIP(hipFuncSetAttribute((const void*)v.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g1_lds(v, 320)));
    net->cls_var = menu[0];
    if (!measure) return 0;
    const int tb = ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES;
    char sig[160];
    snprintf(sig, sizeof(sig), "v%d m%d headcls %s %dx%d n%d b%d", pp_version(), (int)menu.size(), net->layers.back().var.name, ctx->H, ctx->W, ctx->cfg.norm_kind, tb);
    auto hit = tune_cache().find(sig);
    if (hit != tune_cache().end())
        for (const Variant& v : menu)
            if (hit->second == v.name) { net->cls_var = v; return 0; }
    hipEvent_t e0, e1;
    PP_HIP(hipEventCreate(&e0));
    PP_HIP(hipEventCreate(&e1));
    NormRef pre;
    pre.mode = PRE_AFFINE; pre.scale = net->ones; pre.shift = net->zeros;
    double best = 1e30;
    for (const Variant& v : menu) {
        float ms = 0.f;
        for (int it = 0; it <= 3; ++it) {
            if (it == 1) PP_HIP(hipEventRecord(e0, 0));
            int rc = launch_head_cls(ctx, v, tin, pre, ctx->f_cls, tb, 0);
            if (rc) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return rc; }
        }
        PP_HIP(hipEventRecord(e1, 0));
        PP_HIP(hipEventSynchronize(e1));
        PP_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (verbose) fprintf(stderr, "[pp autotune] %-28s %-34s %8.1f us\n", sig, v.name, ms / 3 * 1e3);
        if (ms < best) { best = ms; net->cls_var = v; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    tune_cache()[sig] = net->cls_var.name;
    return 0;
}

} // namespace

int pp_net_create(pp_ctx* ctx)
{
    pp_net* net = new pp_net();
    ctx->net = net;
    const int H = ctx->H, W = ctx->W;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) net->num_cu = prop.multiProcessorCount;
        if (const char* e = getenv("PP_W4_STRIPS")) net->w4_strips = (e[0] == '0') ? 0 : (e[0] == '2') ? 2 : -1;
    }
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < 4; ++b)
        {   // W6_FRONT_PAD floats in front: wino6's dwordx4 patch pieces start one float before a row (row 0 of channel 0 of frame 0 included)
            PP_HIP(hipMalloc((void**)&net->buf[l][b], ((size_t)ctx->max_batch * kC[l] * ((H >> l) + 1) * ((W >> l) + 1) + W6_FRONT_PAD) * sizeof(float)));
            net->buf[l][b] += W6_FRONT_PAD;
        }
    PP_HIP(hipMalloc((void**)&net->up, (size_t)ctx->max_batch * 320 * H * W * sizeof(float)));
    // statistics accumulators: one slot of [NREP][256][2] doubles per normalisation site (<= 24 sites)
    net->stats_bytes = (size_t)ctx->max_batch * 24 * NREP * 320 * 2 * sizeof(double);
    PP_HIP(hipMalloc((void**)&net->stats, net->stats_bytes));
    PP_HIP(hipMalloc((void**)&net->aff, (size_t)ctx->max_batch * 640 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->bn_scale, (size_t)24 * 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->bn_shift, (size_t)24 * 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->head_bias, (size_t)head_rows(ctx->cfg.num_anchor_per_loc) * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->head_bias_perm, 96 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->ones, 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->zeros, 320 * sizeof(float)));
    std::vector<float> one(320, 1.f);
    PP_HIP(hipMemcpy(net->ones, one.data(), 320 * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP(hipMemset(net->zeros, 0, 320 * sizeof(float)));
    // layer list in execution order
    int cin = 64;
    for (int b = 0; b < 3; ++b) {
        const int c = kC[b];
        const int nres[3] = {1, 1, 0};
        const int nunits = (b == 0) ? 2 : 3;
        char key[128];
        snprintf(key, sizeof(key), "rpn.block%d.0.weight", b + 1);
        net->layers.push_back(Layer{key, 0, cin, c, 2, 1, b, pick_variant(0, 2, 1, c, H >> b, W >> b)});
        for (int u = 0; u < nunits; ++u) {
            const int nl = (b == 0) ? (u == 0 ? 1 : 0) : nres[u];
            snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.2.weight", b + 1, 3 + u);
            net->layers.push_back(Layer{key, 0, c, c, 1, 1, b, pick_variant(0, 1, 1, c, H >> b, W >> b)});
            if (nl == 1) {
                snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.5.weight", b + 1, 3 + u);
                net->layers.push_back(Layer{key, 0, c, c, 1, 1, b, pick_variant(0, 1, 1, c, H >> b, W >> b)});
            }
        }
        const int up = 1 << b;
        snprintf(key, sizeof(key), "rpn.deconv%d.0.weight", b + 1);
        net->layers.push_back(Layer{key, 1, c, (b == 0) ? 64 : 128, 1, up, b, pick_variant(1, 1, up, ((b == 0) ? 64 : 128) * up * up, H >> b, W >> b)});
        cin = c;
    }
    net->layers.push_back(Layer{"heads", 2, 320, 10 * ctx->cfg.num_anchor_per_loc, 1, 1, 0,
                                pick_variant(2, 1, 1, head_rows(ctx->cfg.num_anchor_per_loc), H, W, ctx->cfg.num_anchor_per_loc == 9)});
    for (Layer& L : net->layers)
        PP_HIP(hipFuncSetAttribute((const void*)L.var.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.var.lds));
    for (Family f : {Family::Wino4, Family::Wino6})
        for (const Variant* sv : {&strip_v(f), &strip_h(f)})
            PP_HIP(hipFuncSetAttribute((const void*)sv->kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sv->lds));
    return 0;
}

void pp_net_destroy(pp_ctx* ctx)
{
    pp_net* net = (pp_net*)ctx->net;
    if (!net) return;
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < 4; ++b)
            if (net->buf[l][b]) (void)hipFree(net->buf[l][b] - W6_FRONT_PAD);
    for (Layer& L : net->layers)
        if (L.w) (void)hipFree(L.w);
    void* ptrs[] = {net->dbg_stats, net->up, net->stats, net->aff, net->bn_scale, net->bn_shift, net->head_bias, net->head_bias_perm, net->ones, net->zeros};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    delete net;
    ctx->net = nullptr;
}

// BatchNorm2d(eval, eps 1e-3) of the _export/_trt nets folded to (scale, shift) for norm site `site`
static int fold_bn(pp_ctx* ctx, const std::string& prefix, int C, int site)
{
    pp_net* net = (pp_net*)ctx->net;
    auto get = [&](const char* s) -> const std::vector<float>* {
        auto it = ctx->host_w.find(prefix + s);
        if (it == ctx->host_w.end() || (int)it->second.data.size() != C) return nullptr;
        return &it->second.data;
    };
    const std::vector<float>*g = get(".weight"), *b = get(".bias"), *rm = get(".running_mean"), *rv = get(".running_var");
    if (!g || !b || !rm || !rv) return pp_fail(ctx, PP_E_NAME, ("missing BatchNorm tensors for " + prefix).c_str());
    std::vector<float> sc(C), sh(C);
    for (int c = 0; c < C; ++c) {
        double s = (double)(*g)[c] / std::sqrt((double)(*rv)[c] + 1e-3);
        sc[c] = (float)s;
        sh[c] = (float)((double)(*b)[c] - (double)(*rm)[c] * s);
    }
    PP_HIP(hipMemcpy(net->bn_scale + (size_t)site * 320, sc.data(), C * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(net->bn_shift + (size_t)site * 320, sh.data(), C * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// Normalisation sites, numbered in execution order.  Per block b (0..2):
//   site 8b+0: norm after the strided conv (.1)        site 8b+1+2u: Resnet2 unit u first norm (.0)
//   site 8b+2+2u: unit u second norm (.3)              site 8b+7: norm after the deconv
static inline int site_block(int b, int k) { return 8 * b + k; }

int pp_net_commit(pp_ctx* ctx)
{
    pp_net* net = (pp_net*)ctx->net;
    const int na = ctx->cfg.num_anchor_per_loc;
    std::vector<float> hbv((size_t)head_rows(na), 0.f);
    float* hb = hbv.data();
    const char* names[3] = {"heads.conv_cls.bias", "heads.conv_box.bias", "heads.conv_dir.bias"};
    const int cnt[3] = {na, 7 * na, 2 * na};
    int r0 = 0;
    for (int h = 0; h < 3; ++h) {
        auto w = ctx->host_w.find(names[h]);
        if (w == ctx->host_w.end() || (int)w->second.data.size() != cnt[h])
            return pp_fail(ctx, PP_E_NAME, (std::string("missing/mis-shaped ") + names[h]).c_str());
        memcpy(hb + r0, w->second.data.data(), sizeof(float) * cnt[h]);
        r0 += cnt[h];
    }
    PP_HIP(hipMemcpy(net->head_bias, hb, hbv.size() * sizeof(float), hipMemcpyHostToDevice));
    if (na == 9) {
        float hp[96];
        for (int t = 0; t < 96; ++t) hp[t] = head_tile_row(t) >= 0 ? hb[head_tile_row(t)] : 0.f;
        PP_HIP(hipMemcpy(net->head_bias_perm, hp, sizeof(hp), hipMemcpyHostToDevice));
    }
    {
        const char* at = getenv("PP_AUTOTUNE");
        const char* vb = getenv("PP_VERBOSE");
        const bool tune = !(at && at[0] == '0');
        const bool verbose = vb && vb[0] != '0';
        const int H = ctx->H, W = ctx->W;
        float *tin = nullptr, *tout = nullptr;
        const bool can_tune = tune && (H % 4 == 0) && (W % 4 == 0);
        // fp16 storage of the activations needs every conv on conv16's and every upsampler / the head on gemm1x1's 16-bit-tensor
        // tilings: maps a multiple of 4 wide at all three levels and the 9-anchor head; otherwise mode 4 runs as mode 3 (fp32 tensors)
        net->up16 = ctx->precision == 4 && (W % 16 == 0) && ((H * W) % 64 == 0) && ctx->cfg.num_anchor_per_loc == 9;
        net->eff_prec = (ctx->precision == 4 && !net->up16) ? 3 : ctx->precision;
        if (can_tune) {
            const size_t nin = std::max((size_t)64 * ctx->gx * ctx->gy, (size_t)320 * H * W);
            const int tb = ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES;
            PP_HIP(hipMalloc((void**)&tin, ((size_t)tb * nin + 256 + W6_FRONT_PAD) * sizeof(float)));
            tin += W6_FRONT_PAD;
            PP_HIP(hipMalloc((void**)&tout, ((size_t)tb * 320 * H * W + 256) * sizeof(float)));
            hipLaunchKernelGGL(fill_pattern, dim3(2048), dim3(256), 0, 0, tin, (size_t)tb * nin);
        }
        for (Layer& L : net->layers) {
            int rc = 0;
            {
                const int h = H >> L.level, w = W >> L.level;
                const int hin = (L.kind == 0 && L.stride == 2) ? h * 2 : h, win = (L.kind == 0 && L.stride == 2) ? w * 2 : w;
                if (!can_tune && net->eff_prec == 0) L.var = pick_variant(L.kind, L.stride, L.up, (L.kind == 2) ? head_rows(ctx->cfg.num_anchor_per_loc) : (L.kind == 1 ? L.cout * L.up * L.up : L.cout), h, w, ctx->cfg.num_anchor_per_loc == 9);
                rc = autotune_layer(ctx, L, hin, win, h, w, tin, tout, verbose, can_tune);
                if (rc) { if (tin) { (void)hipFree(tin - W6_FRONT_PAD); (void)hipFree(tout); } return rc; }
            }
            PP_HIP(hipFuncSetAttribute((const void*)L.var.kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)layer_lds(L.var, L.cin)));
            if (L.var.kern2) PP_HIP(hipFuncSetAttribute((const void*)L.var.kern2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.var.lds));
            rc = pack_layer(ctx, L);
            if (rc) { if (tin) { (void)hipFree(tin - W6_FRONT_PAD); (void)hipFree(tout); } return rc; }
        }
        ctx->sc1_kc = (net->layers[0].var.family == Family::Direct && net->layers[0].var.kc == 8) ? 8 : 4;
        {   // deferred head: fp32 plan with the 9-anchor head on a gemm1x1 tiling (its image is what the cls pass and the candidate head read)
            const Layer& head = net->layers.back();
            net->defer_ok = net->eff_prec == 0 && na == 9 && head.var.family == Family::Gemm1x1 && head.var.prec == 0 && head.var.io16 == 0;
            if (net->defer_ok) {
                const int rc = autotune_head_cls(ctx, tin, verbose, can_tune);
                if (rc) { if (tin) { (void)hipFree(tin - W6_FRONT_PAD); (void)hipFree(tout); } return rc; }
            }
        }
        if (tin) { PP_HIP(hipDeviceSynchronize()); (void)hipFree(tin - W6_FRONT_PAD); (void)hipFree(tout); tune_cache_save(); }
        if (net->up16)
            for (const Layer& L : net->layers)
                if ((L.kind == 1 && L.var.io16 != 3) || (L.kind == 2 && L.var.io16 != 1) ||
                    (L.kind == 0 && L.var.io16 != ((L.stride == 2 && L.level == 0) ? 2 : 3)))
                    return pp_fail(ctx, PP_E_STATE, "fp16s: a layer did not get a 16-bit-tensor tiling (PP_FORCE_VARIANT?)");
    }
    if (ctx->cfg.norm_kind == 1) {
        for (int b = 0; b < 3; ++b) {
            char key[128];
            const int c = kC[b];
            snprintf(key, sizeof(key), "rpn.block%d.1", b + 1);
            int rc = fold_bn(ctx, key, c, site_block(b, 0));
            if (rc) return rc;
            const int nunits = (b == 0) ? 2 : 3;
            for (int u = 0; u < nunits; ++u) {
                const int nl = (u == nunits - 1) ? 0 : 1;
                snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.0", b + 1, 3 + u);
                if ((rc = fold_bn(ctx, key, c, site_block(b, 1 + 2 * u)))) return rc;
                if (nl) {
                    snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.3", b + 1, 3 + u);
                    if ((rc = fold_bn(ctx, key, c, site_block(b, 2 + 2 * u)))) return rc;
                }
            }
            snprintf(key, sizeof(key), "rpn.deconv%d.1", b + 1);
            // deconv norms are stored contiguously at site 7 (block 0), channels [0,64),[64,192),[192,320)
            const int coff = (b == 0) ? 0 : (b == 1 ? 64 : 192);
            const int cc = (b == 0) ? 64 : 128;
            pp_net* n2 = net;
            {
                auto get = [&](const char* s) -> const std::vector<float>* {
                    auto it = ctx->host_w.find(std::string(key) + s);
                    if (it == ctx->host_w.end() || (int)it->second.data.size() != cc) return nullptr;
                    return &it->second.data;
                };
                const std::vector<float>*g = get(".weight"), *bb = get(".bias"), *rm = get(".running_mean"), *rv = get(".running_var");
                if (!g || !bb || !rm || !rv) return pp_fail(ctx, PP_E_NAME, (std::string("missing BatchNorm tensors for ") + key).c_str());
                std::vector<float> sc(cc), sh(cc);
                for (int q = 0; q < cc; ++q) {
                    double s = (double)(*g)[q] / std::sqrt((double)(*rv)[q] + 1e-3);
                    sc[q] = (float)s;
                    sh[q] = (float)((double)(*bb)[q] - (double)(*rm)[q] * s);
                }
                PP_HIP(hipMemcpy(n2->bn_scale + (size_t)7 * 320 + coff, sc.data(), cc * sizeof(float), hipMemcpyHostToDevice));
                PP_HIP(hipMemcpy(n2->bn_shift + (size_t)7 * 320 + coff, sh.data(), cc * sizeof(float), hipMemcpyHostToDevice));
            }
        }
    }
    return 0;
}

namespace {

// statistics slot / folded-BN arrays for a site
NormRef norm_ref(pp_ctx* ctx, int site, int C, int coff, size_t count)
{
    pp_net* net = (pp_net*)ctx->net;
    NormRef r;
    r.C = C;
    if (ctx->cfg.norm_kind == 1) {
        r.mode = PRE_AFFINE;
        r.scale = net->bn_scale + (size_t)site * 320 + coff;
        r.shift = net->bn_shift + (size_t)site * 320 + coff;
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
    if (ctx->cfg.norm_kind == 1) return nullptr;
    return ((pp_net*)ctx->net)->stats + (size_t)site * NREP * 320 * 2;
}

int launch_norm_relu(pp_ctx* ctx, const float* x, float* y, int C, int HW, const NormRef& pre, double* stat, hipStream_t stream,
                     int B = 1, int x16 = 0, int y16 = 0)
{
    int bx = pp_div_up(HW / 4, 256 * 4);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(norm_relu_stats, dim3(bx, C, B), dim3(256), 0, stream, x, y, C, HW, pre.mode, pre.acc, pre.scale,
                       pre.shift, pre.inv_n, 1e-3f, stat, (size_t)C * HW, STAT_FS, x16, y16);
    PP_HIP(hipGetLastError());
    return 0;
}

} // namespace

// do all stride-1 layers of level 0 (at most three: tile_skip.hip's rule) run the fp32 wino6 main tile on a map of whole main tiles?
static bool level0_main_wino6(const pp_net* net, int h, int w)
{
    int n = 0;
    for (const Layer& L : net->layers)
        if (L.kind == 0 && L.level == 0 && L.stride == 1) {
            ++n;
            if (L.var.family != Family::Wino6 || !L.var.kern2 || L.var.pw != 16 || L.var.ph != 16 || (w % 16) || (h % 16)) return false;
        }
    return n >= 1 && n <= 3 && net->eff_prec == 0;
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
    if (ctx->cfg.norm_kind == 0) PP_HIP(hipMemsetAsync(net->stats, 0, STAT_FS * sizeof(double) * nb, stream));
    NormRef raw;
    const float* x = canvas;
    int Hin = ctx->gx, Win = ctx->gy;
    size_t li = 0;
    const int up_coff[3] = {0, 64, 192};
    const size_t up_fs = (size_t)320 * H * W;
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
        } else if ((rc = launch_conv(ctx, net->layers[li++], x, Hin, Win, Bf[0], nullptr, raw, stat_slot(ctx, site_block(b, 0)), c, h, w, stream,
                              nullptr, nullptr, nb, 0, 0, b == 0 ? pmap : nullptr, b == 0 ? feat : nullptr))) return rc;
        // the level's pre-norm conv output z leaves through its own copy hook: the first unit reuses Bf[0] as a spare
        if (nb == 1 && net->z_tap[b])
            PP_HIP(hipMemcpyAsync(net->z_tap[b], Bf[0], (size_t)c * cnt * sizeof(float), hipMemcpyDeviceToDevice, stream));
        // y = relu(norm(Bf[0])) -> Bf[1] + stats(site 1) (the first Resnet2 unit's leading norm)
        if ((rc = pp_stage_mark(ctx, stream, PP_ST_NORM))) return rc;
        if ((rc = launch_norm_relu(ctx, Bf[0], Bf[1], c, (int)cnt, norm_ref(ctx, site_block(b, 0), c, 0, cnt),
                                   stat_slot(ctx, site_block(b, 1)), stream, nb, net->up16 ? 1 : 0, net->up16 ? 1 : 0))) return rc;
        if ((rc = pp_stage_mark(ctx, stream, PP_ST_CONV))) return rc;
        float* cur = Bf[1];
        float* spare[3] = {Bf[0], Bf[2], Bf[3]};
        // the unit inputs (h, m, r at level 0; h, m3, r3, m4, r4 at levels 1 and 2) leave through the copy hook behind the launch that
        // produces each: the level buffers are reused before the pass ends
        float* utap = nb == 1 ? net->unit_tap[b] : nullptr;
        const size_t ubytes = (size_t)c * cnt * sizeof(float);
        int ucount = 0;
        if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * c * cnt, cur, ubytes, hipMemcpyDeviceToDevice, stream));
        const int nunits = (b == 0) ? 2 : 3;
        int ts_k = 0; // level 0: ordinal of the next stride-1 layer (launch_conv ignores it unless this pass built tile lists)
        for (int u = 0; u < nunits; ++u) {
            const int nl = (u == nunits - 1) ? 0 : 1;
            const bool last = (u == nunits - 1);
            float* t1 = spare[0];
            float* t2 = spare[1];
            // stats for the NEXT unit's leading norm are produced by this unit's output
            double* out_stat = last ? nullptr : stat_slot(ctx, site_block(b, 1 + 2 * (u + 1)));
            if (nl == 1) {
                if ((rc = launch_conv(ctx, net->layers[li++], cur, h, w, t1, nullptr, norm_ref(ctx, site_block(b, 1 + 2 * u), c, 0, cnt),
                                      stat_slot(ctx, site_block(b, 2 + 2 * u)), c, h, w, stream, nullptr, nullptr, nb, 0, 0, nullptr, nullptr,
                                      b == 0 ? ++ts_k : 0))) return rc;
                if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * c * cnt, t1, ubytes, hipMemcpyDeviceToDevice, stream));
                if ((rc = launch_conv(ctx, net->layers[li++], t1, h, w, t2, cur, norm_ref(ctx, site_block(b, 2 + 2 * u), c, 0, cnt),
                                      out_stat, c, h, w, stream, nullptr, nullptr, nb, 0, 0, nullptr, nullptr, b == 0 ? ++ts_k : 0))) return rc;
                if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * c * cnt, t2, ubytes, hipMemcpyDeviceToDevice, stream));
                spare[1] = cur; // t2 becomes current; old current and t1 are free
                cur = t2;
            } else {
                if ((rc = launch_conv(ctx, net->layers[li++], cur, h, w, t1, cur, norm_ref(ctx, site_block(b, 1 + 2 * u), c, 0, cnt),
                                      out_stat, c, h, w, stream, nullptr, nullptr, nb, 0, 0, nullptr, nullptr, b == 0 ? ++ts_k : 0))) return rc;
                spare[0] = cur;
                cur = t1;
            }
        }
        net->tap[b] = cur;
        // deconv on the raw block output -> channel slice of up[320,H,W] + stats (site 7, channel offset)
        {
            const Layer& L = net->layers[li++];
            double* st = stat_slot(ctx, 7);
            // the block's channel slice of the concat buffer (element offsets: the buffer holds fp16 under pp_set_precision 4)
            float* slice = net->up16 ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(net->up) + (size_t)up_coff[b] * H * W)
                                     : net->up + (size_t)up_coff[b] * H * W;
            if ((rc = launch_conv(ctx, L, cur, h, w, slice, nullptr, raw, st ? st + (size_t)up_coff[b] * 2 : nullptr,
                                  320, h, w, stream, nullptr, nullptr, nb, up_fs))) return rc;
        }
        x = cur;
        Hin = h;
        Win = w;
    }
    return 0;
}

static int pp_head_impl(pp_ctx* ctx, const float* in, const NormRef& pre, float* cls, float* box, float* dir, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    return launch_conv(ctx, net->layers.back(), in, ctx->H, ctx->W, cls, nullptr, pre, nullptr, 0, ctx->H, ctx->W, stream, box, dir, nb);
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

// A packed weight image as an index map (pp_common.h): pack_layer itself packs an index-valued weight (element i of the
// concatenation of the named host tensors holds the float i + 1; exact below 2^24) into a scratch image with the layer's committed
// tiling, so whatever row order (head_tile_row), row padding and K blocking that tiling uses is read back, not restated.  fp32 images
// only: the 16-bit images round their elements, the indices would not survive.  Synchronous; called once per commit by train.hip.
static int layer_index_map(pp_ctx* ctx, const Layer& L, const std::vector<std::string>& names, std::vector<int32_t>& wmap)
{
    std::vector<std::vector<float>> saved(names.size());
    float idx = 1.f;
    for (size_t h = 0; h < names.size(); ++h) {
        auto w = ctx->host_w.find(names[h]);
        if (w == ctx->host_w.end()) {
            for (size_t g = 0; g < h; ++g) ctx->host_w[names[g]].data.swap(saved[g]);
            return pp_fail(ctx, PP_E_NAME, ("missing weight " + names[h]).c_str());
        }
        saved[h] = w->second.data;
        for (float& v : w->second.data) v = idx++;
    }
    Layer scratch = L;
    scratch.w = nullptr;
    int rc = idx > 16777216.f ? pp_fail(ctx, PP_E_ARG, "weight too large for an index map") : pack_layer(ctx, scratch);
    for (size_t h = 0; h < names.size(); ++h) ctx->host_w[names[h]].data.swap(saved[h]);
    if (rc) { if (scratch.w) (void)hipFree(scratch.w); return rc; }
    std::vector<float> image(scratch.w_bytes / sizeof(float));
    const hipError_t e = hipMemcpy(image.data(), scratch.w, scratch.w_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(scratch.w);
    PP_HIP(e);
    wmap.resize(image.size());
    for (size_t i = 0; i < image.size(); ++i) wmap[i] = (int32_t)image[i] - 1;
    return 0;
}

// The layout of a conv3x3 layer's fp32 image as a map onto the TRANSFORMED weights: pmap[i] = (row cin + c) T + position of the element
// of [rows][cin][T] that image element i holds (T = 36 wino6, 16 wino / wino4: position a n + b of U = G g G^T; 9 direct: the tap),
// -1 for padding.  The Winograd images hold U, not permuted copies of g, so layer_index_map cannot describe them.
static int layer_position_map(pp_ctx* ctx, const Layer& L, std::vector<int32_t>& pmap, int* T)
{
    const Family f = L.var.family;
    *T = f == Family::Wino6 ? 36 : (f == Family::Wino || f == Family::Wino4) ? 16 : 9;
    if ((size_t)L.cout * L.cin * *T >= 16777216) return pp_fail(ctx, PP_E_ARG, "weight too large for a position map");
    Layer scratch = L;
    scratch.w = nullptr;
    int rc = pack_layer(ctx, scratch, true);
    if (rc) { if (scratch.w) (void)hipFree(scratch.w); return rc; }
    std::vector<float> image(scratch.w_bytes / sizeof(float));
    const hipError_t e = hipMemcpy(image.data(), scratch.w, scratch.w_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(scratch.w);
    PP_HIP(e);
    pmap.resize(image.size());
    for (size_t i = 0; i < image.size(); ++i) pmap[i] = (int32_t)image[i] - 1;
    return 0;
}

// Unit `unit` (0..4) of Resnet block `block` of the committed plan, for pp_update_block_weights (block_train.hip)
int pp_net_block_image(pp_ctx* ctx, int block, int unit, pp_block_image* img)
{
    pp_net* net = (pp_net*)ctx->net;
    int seen = 0;
    for (Layer& L : net->layers) {
        if (L.kind != 0 || L.level != block || L.stride != 1 || seen++ != unit) continue;
        if (net->eff_prec != 0 || L.var.prec != 0 || L.var.io16 != 0 || L.var.family == Family::Conv16)
            return pp_fail(ctx, PP_E_ARG, "block weights can be rewritten in place in the fp32 mode only (the committed plan packs them in a 16-bit format)");
        int rc = layer_position_map(ctx, L, img->pmap, &img->T);
        if (rc) return rc;
        img->w = L.w;
        img->C = L.cin;
        img->rows = L.cout;
        return L.cin == L.cout ? 0 : pp_fail(ctx, PP_E_ARG, "pp_net_block_image: not a C -> C unit");
    }
    return pp_fail(ctx, PP_E_ARG, "pp_net_block_image: no such unit");
}

// The strided convolution in front of block `level` of the committed plan, for pp_update_down_weight (down_train.hip)
int pp_net_down_image(pp_ctx* ctx, int level, pp_block_image* img)
{
    pp_net* net = (pp_net*)ctx->net;
    for (Layer& L : net->layers) {
        if (L.kind != 0 || L.level != level || L.stride != 2) continue;
        if (net->eff_prec != 0 || L.var.prec != 0 || L.var.io16 != 0 || L.var.family == Family::Conv16)
            return pp_fail(ctx, PP_E_ARG, "the strided convolution can be rewritten in place in the fp32 mode only (the committed plan packs it in a 16-bit format)");
        if (L.var.family != Family::Direct) return pp_fail(ctx, PP_E_ARG, "pp_net_down_image: the strided convolution does not run a direct tiling");
        int rc = layer_position_map(ctx, L, img->pmap, &img->T);
        if (rc) return rc;
        img->w = L.w;
        img->C = L.cin;
        img->rows = L.cout;
        return 0;
    }
    return pp_fail(ctx, PP_E_ARG, "pp_net_down_image: no such layer");
}

int pp_net_head_image(pp_ctx* ctx, pp_head_image* img)
{
    pp_net* net = (pp_net*)ctx->net;
    Layer& head = net->layers.back();
    if (net->eff_prec != 0 || head.var.prec != 0 || head.var.io16 != 0)
        return pp_fail(ctx, PP_E_ARG, "head weights can be rewritten in place in the fp32 mode only (the committed plan packs the head in a 16-bit format)");
    const int na = ctx->cfg.num_anchor_per_loc;
    const char* names[3] = {"heads.conv_cls.weight", "heads.conv_box.weight", "heads.conv_dir.weight"};
    const int cnt[3] = {na, 7 * na, 2 * na};
    for (int h = 0; h < 3; ++h) {
        auto w = ctx->host_w.find(names[h]);
        if (w == ctx->host_w.end() || (int64_t)w->second.data.size() != (int64_t)cnt[h] * head.cin)
            return pp_fail(ctx, PP_E_NAME, (std::string("missing/mis-shaped weight ") + names[h]).c_str());
    }
    int rc = layer_index_map(ctx, head, {names[0], names[1], names[2]}, img->wmap);
    if (rc) return rc;
    img->w = head.w;
    img->bias = net->head_bias;
    img->bmap.assign((size_t)head_rows(na), -1);
    for (int r = 0; r < 10 * na; ++r) img->bmap[r] = r;
    img->bias_perm = nullptr;
    img->bpmap.clear();
    if (na == 9) {
        img->bias_perm = net->head_bias_perm;
        img->bpmap.resize(96);
        for (int t = 0; t < 96; ++t) img->bpmap[t] = head_tile_row(t);
    }
    return 0;
}

// The packed image of upsampler `branch` (0..2) of the committed plan, described the same way: wmap[i] is the element of the
// state_dict tensor rpn.deconv<branch+1>.0.weight [Cin][Cup][s][s] that image element i holds, -1 for padding.
int pp_net_deconv_image(pp_ctx* ctx, int branch, pp_layer_image* img)
{
    pp_net* net = (pp_net*)ctx->net;
    int seen = 0;
    for (Layer& L : net->layers) {
        if (L.kind != 1 || seen++ != branch) continue;
        if (net->eff_prec != 0 || L.var.prec != 0 || L.var.io16 != 0)
            return pp_fail(ctx, PP_E_ARG, "upsampler weights can be rewritten in place in the fp32 mode only (the committed plan packs them in a 16-bit format)");
        int rc = layer_index_map(ctx, L, {L.wkey}, img->wmap);
        if (rc) return rc;
        img->w = L.w;
        img->elems = (size_t)L.cin * L.cout * L.up * L.up;
        return 0;
    }
    return pp_fail(ctx, PP_E_ARG, "pp_net_deconv_image: no such upsampler");
}

extern "C" int pp_backbone_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone_taps: weights not committed");
    if (!canvas || !rpn_out || !x1 || !x2 || !x3) return pp_fail(ctx, PP_E_ARG, "pp_backbone_taps: null pointer");
    pp_net* net = (pp_net*)ctx->net;
    if (net->eff_prec != 0 || net->up16)
        return pp_fail(ctx, PP_E_ARG, "pp_backbone_taps: fp32 mode only (in the 16-bit modes the level buffers may hold fp16)");
    int rc = pp_backbone(ctx, canvas, rpn_out, stream_);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    float* dst[3] = {x1, x2, x3};
    for (int b = 0; b < 3; ++b)
        PP_HIP(hipMemcpyAsync(dst[b], net->tap[b], (size_t)kC[b] * (ctx->H >> b) * (ctx->W >> b) * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

extern "C" int pp_backbone_block_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* units, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone_block_taps: weights not committed");
    if (!units) return pp_fail(ctx, PP_E_ARG, "pp_backbone_block_taps: null pointer");
    pp_net* net = (pp_net*)ctx->net;
    net->unit_tap[2] = units; // pp_backbone_taps checks the rest; the hook is armed for this one pass only
    int rc = pp_backbone_taps(ctx, canvas, rpn_out, x1, x2, x3, stream_);
    net->unit_tap[2] = nullptr;
    return rc;
}

extern "C" int pp_backbone_stage_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* units, float* z3,
                                      void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone_stage_taps: weights not committed");
    if (!z3) return pp_fail(ctx, PP_E_ARG, "pp_backbone_stage_taps: null pointer");
    pp_net* net = (pp_net*)ctx->net;
    net->z_tap[2] = z3; // pp_backbone_block_taps checks the rest; the hook is armed for this one pass only
    int rc = pp_backbone_block_taps(ctx, canvas, rpn_out, x1, x2, x3, units, stream_);
    net->z_tap[2] = nullptr;
    return rc;
}

// every level's hooks at once: units[b] f32[3 | 5 | 5][C_b][H>>b][W>>b], z[b] f32[C_b][H>>b][W>>b]
extern "C" int pp_backbone_train_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* const* units,
                                      float* const* z, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone_train_taps: weights not committed");
    if (!units || !z) return pp_fail(ctx, PP_E_ARG, "pp_backbone_train_taps: null pointer");
    for (int b = 0; b < 3; ++b)
        if (!units[b] || !z[b]) return pp_fail(ctx, PP_E_ARG, "pp_backbone_train_taps: null pointer");
    pp_net* net = (pp_net*)ctx->net;
    for (int b = 0; b < 3; ++b) { net->unit_tap[b] = units[b]; net->z_tap[b] = z[b]; } // pp_backbone_taps checks the rest; armed for this one pass only
    int rc = pp_backbone_taps(ctx, canvas, rpn_out, x1, x2, x3, stream_);
    for (int b = 0; b < 3; ++b) net->unit_tap[b] = net->z_tap[b] = nullptr;
    return rc;
}

// Test / inspection hook: copy one tensor of frame `frame` of the LAST pp_infer_batch / pp_infer_frame pass out of the
// context's internal frame buffers (device -> device, on `stream`).  kind: 0 cls f32[A], 1 box f32[A,7], 2 dir f32[A,2],
// 3 anchor mask u8[A], 4 rpn output f32[320,H,W] = relu(norm(concat)) as RPN.forward returns it
// (pointpillars8_shared.py:173-181; materialised here, the fused path never stores it), 5 PFN rows f32[max_voxels,64],
// 6 coors i32[max_voxels,3], 7 pillar count i32[1], 8 active list of the sparse first conv i32[1 + min(4 max_voxels, H W)]
// (count, then the active output pixels in ascending order; PP_E_STATE when the pass ran the dense first conv), 9 tile flags of the
// tile-skipping path u8[3][(H / 16) (W / 16)] (1 = skippable at layer 1, 2, 3; PP_E_STATE when the pass built none).
extern "C" int pp_fetch_frame_tensor(pp_ctx* ctx, int frame, int kind, void* dst, void* stream_)
{
    if (!ctx || !dst) return pp_fail(ctx, PP_E_ARG, "pp_fetch_frame_tensor: null pointer");
    if (frame < 0 || frame >= ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_fetch_frame_tensor: frame out of range");
    hipStream_t stream = (hipStream_t)stream_;
    pp_net* net = (pp_net*)ctx->net;
    const size_t A = (size_t)ctx->A, mv = (size_t)ctx->cfg.max_voxels, HW = (size_t)ctx->H * ctx->W;
    const void* src = nullptr;
    size_t bytes = 0;
    if (kind == 1 || kind == 2)
        if (int rc0 = pp_head_materialise(ctx, stream)) return rc0;
    switch (kind) {
    case 0: src = ctx->f_cls + frame * A; bytes = A * 4; break;
    case 1: src = ctx->f_box + frame * A * 7; bytes = A * 28; break;
    case 2: src = ctx->f_dir + frame * A * 2; bytes = A * 8; break;
    case 3: src = ctx->f_mask + frame * A; bytes = A; break;
    case 4: {
        NormRef pre = norm_ref(ctx, 7, 320, 0, HW);
        if (pre.mode == PRE_STATS) pre.acc += (size_t)frame * STAT_FS;
        const float* src_ = net->up16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(net->up) + (size_t)frame * 320 * HW)
                                      : net->up + (size_t)frame * 320 * HW;
        return launch_norm_relu(ctx, src_, (float*)dst, 320, (int)HW, pre, nullptr, stream, 1, net->up16 ? 1 : 0);
    }
    case 5: src = ctx->f_feat + frame * mv * 64; bytes = mv * 64 * 4; break;
    case 6: src = ctx->f_coors + frame * mv * 3; bytes = mv * 12; break;
    case 7: src = ctx->f_num + frame * 4; bytes = 4; break;
    case 8: return pp_sc1_fetch_list(ctx, frame, dst, stream);
    case 9: return pp_ts_fetch_flags(ctx, frame, dst, stream);
    default: return pp_fail(ctx, PP_E_ARG, "pp_fetch_frame_tensor: unknown kind");
    }
    PP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
    return 0;
}

namespace {
// out[f][c][k] = sum over the NREP replicated accumulators (k = 0 sum, 1 sum of squares)
__global__ void __launch_bounds__(256) dbg_reduce_stats(const double* __restrict__ acc, size_t acc_fs, int C, double* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * C) return;
    const double* a = acc + (size_t)blockIdx.y * acc_fs;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < NREP; ++r) s += a[(size_t)r * C * 2 + i];
    out[(size_t)blockIdx.y * 2 * C + i] = s;
}
} // namespace

// Test hook: ONE layer of the committed plan (kernel, tiling and weight image as pp_layer_tilings reports them) through launch_conv on
// caller tensors -- see include/pp_hip.h.  Reads the plan and the weight images, writes only caller memory and its own statistics
// scratch: nothing a later pass reads changes.
extern "C" int pp_debug_layer(pp_ctx* ctx, int layer, int nb, const void* in, const void* res, int pre_mode, const float* scale, const float* shift,
                              const int32_t* pmap, const float* feat, void* out, float* out_box, float* out_dir, double* stats, void* stream_)
{
    return pp_debug_layer_skip(ctx, layer, nb, in, res, pre_mode, scale, shift, pmap, feat, out, out_box, out_dir, stats, nullptr, 0, stream_);
}

// pp_debug_layer with the tile-skipping form: active u8[nb][H][W] (the pixels the sparse first conv would have computed) and the layer's
// ordinal skip_k (1..3) build the lists with the pass's own builder; the layer then runs as the listed launch plus the fill.
extern "C" int pp_debug_layer_skip(pp_ctx* ctx, int layer, int nb, const void* in, const void* res, int pre_mode, const float* scale, const float* shift,
                                   const int32_t* pmap, const float* feat, void* out, float* out_box, float* out_dir, double* stats,
                                   const uint8_t* active, int skip_k, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->net || !ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_debug_layer: weights not committed");
    pp_net* net = (pp_net*)ctx->net;
    if (layer < 0 || layer >= (int)net->layers.size()) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: layer index out of range");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: nb must be 1 .. cfg.max_batch");
    const Layer& L = net->layers[layer];
    const bool sparse = pmap || feat;
    if (sparse && layer != 0) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the sparse input form belongs to layer 0");
    if (sparse && (!pmap || !feat || in)) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: layer 0 takes either `in` or pmap + feat");
    if (!sparse && !in) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: null input");
    if (!out) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: null output");
    if (res && L.kind != 0) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: only a convolution takes a residual");
    if (pre_mode < 0 || pre_mode > 2) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: pre_mode must be 0 (raw), 1 (shared affine) or 2 (per-frame affine)");
    if ((pre_mode != 0) != (scale != nullptr) || (pre_mode != 0) != (shift != nullptr))
        return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: scale and shift go with pre_mode 1 / 2 and with nothing else");
    if (L.kind == 2 && (!out_box || !out_dir)) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the head needs out_box and out_dir");
    if (L.kind != 2 && (out_box || out_dir)) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: out_box / out_dir belong to the head");
    if (L.kind == 2 && stats) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the head accumulates no statistics");
    if (pre_mode == 0 && (L.var.family == Family::Wino4 || L.var.family == Family::Wino6))
        return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the committed tiling (wino4 / wino6) has no raw prologue, give it a (scale, shift)");
    if ((active != nullptr) != (skip_k != 0)) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer_skip: the activity bitmap and the layer ordinal come together");
    if (active && (skip_k < 1 || skip_k > 3 || L.kind != 0 || L.level != 0 || L.stride != 1 || !pp_ts_usable(ctx, 3) || !level0_main_wino6(net, ctx->H, ctx->W)))
        return pp_fail(ctx, PP_E_ARG, "pp_debug_layer_skip: tile skipping serves the stride-1 layers of level 0 (ordinal 1..3) on the fp32 wino6 main tile, whole tiles, switch on");
    hipStream_t stream = (hipStream_t)stream_;
    const int h = ctx->H >> L.level, w = ctx->W >> L.level;
    const bool s2 = L.kind == 0 && L.stride == 2;
    const int hin = s2 ? 2 * h : h, win = s2 ? 2 * w : w;
    NormRef pre;
    if (pre_mode) { pre.mode = PRE_AFFINE; pre.scale = const_cast<float*>(scale); pre.shift = const_cast<float*>(shift); pre.C = L.cin; pre.aff_fs = pre_mode == 2 ? (size_t)L.cin : 0; }
    double* st = nullptr;
    if (stats) {
        if (!net->dbg_stats) PP_HIP(hipMalloc((void**)&net->dbg_stats, (size_t)ctx->max_batch * STAT_FS * sizeof(double)));
        st = net->dbg_stats;
        PP_HIP(hipMemsetAsync(st, 0, (size_t)nb * STAT_FS * sizeof(double), stream));
    }
    pp_ts_begin_hook(ctx, active != nullptr);
    if (active)
        if (int rc0 = pp_ts_build_from_bitmap(ctx, nb, active, stream)) return rc0;
    const int rc = launch_conv(ctx, L, (const float*)in, hin, win, (float*)out, (const float*)res, pre, st, L.cout, h, w, stream, out_box, out_dir, nb, 0, 0,
                               pmap, feat, active ? skip_k : 0);
    if (active) pp_ts_end_hook(ctx);
    if (rc == PP_E_ARG) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the committed tiling does not take this layer's shape");
    if (rc) return rc;
    if (stats) {
        hipLaunchKernelGGL(dbg_reduce_stats, dim3(pp_div_up(2 * L.cout, 256), nb), dim3(256), 0, stream, st, STAT_FS, L.cout, stats);
        PP_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int pp_profile_begin(pp_ctx* ctx)
{
    if (!ctx) return PP_E_ARG;
    ctx->prof_on = true;
    ctx->prof_used = 0;
    ctx->prof_ts_layer.clear();
    ctx->prof_items = ctx->prof_items_dense = 0.0;
    return 0;
}

extern "C" int pp_profile_end(pp_ctx* ctx, double* avg_ms, int32_t* launches, double* flops)
{
    if (!ctx || !avg_ms || !launches || !flops) return PP_E_ARG;
    ctx->prof_on = false;
    double tot = 0.0;
    const size_t n = ctx->prof_used / 2;
    for (size_t i = 0; i < n; ++i) {
        PP_HIP(hipEventSynchronize(ctx->prof_ev[2 * i + 1]));
        float ms = 0.f;
        PP_HIP(hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]));
        tot += ms;
    }
    // items the listed launches really ran (their counts live on the device; the loop above has synchronised).  Every pass rebuilds the
    // lists, so the counts are those of the last profiled pass: exact when the profiled passes see the same frames.
    for (int e : ctx->prof_ts_layer) {
        int32_t cnt = 0;
        if (int rc = pp_ts_read_count(ctx, e & 0xFF, &cnt)) return rc;
        ctx->prof_items += (double)cnt * (e >> 8);
    }
    ctx->prof_ts_layer.clear();
    *avg_ms = n ? tot / (double)n : 0.0;
    *launches = (int32_t)n;
    *flops = ctx->prof_flops;
    ctx->prof_used = 0;
    return 0;
}

extern "C" int pp_effective_precision(pp_ctx* ctx)
{
    if (!ctx || !ctx->net || !ctx->weights_ready) return -1;
    const pp_net* net = (const pp_net*)ctx->net;
    return net->up16 ? 4 : net->eff_prec;
}

extern "C" const char* pp_dominant_kernel(pp_ctx* ctx)
{
    if (!ctx || !ctx->net) return "";
    pp_net* net = (pp_net*)ctx->net;
    for (const Layer& L : net->layers)
        if (L.kind == 0 && L.level == 0 && L.stride == 1) return L.var.name;
    return "";
}

// Executed MFMA flops / algorithmic (direct-convolution) flops of the dominant layer's tiling: Winograd F(2x2,3x3)
// issues 16 multiplications per 2x2 output tile where the direct form needs 36, F(4x4,3x3) 36 per 4x4 tile against 144;
// split-bf16 issues three MFMAs per product.
extern "C" double pp_dominant_executed_ratio(pp_ctx* ctx)
{
    if (!ctx || !ctx->net) return 1.0;
    pp_net* net = (pp_net*)ctx->net;
    for (const Layer& L : net->layers)
        if (L.kind == 0 && L.level == 0 && L.stride == 1) // x the share of the dense work items the profiled launches ran (tile skipping)
            return executed_ratio(L.var) * (ctx->prof_items_dense > 0.0 ? ctx->prof_items / ctx->prof_items_dense : 1.0);
    return 1.0;
}

// Test / inspection hook: the packed weight image of layer `layer` of the committed plan (0 .. 19), or of the sparse first convolution
// (layer = -1), copied device -> device on `stream`.  Returns the image's size in bytes through `bytes`; dst may be NULL to query.
extern "C" int pp_weight_image(pp_ctx* ctx, int layer, void* dst, size_t cap, size_t* bytes, void* stream_)
{
    if (!ctx || !bytes) return pp_fail(ctx, PP_E_ARG, "pp_weight_image: null pointer");
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_weight_image: weights not committed");
    PP_HIP(hipSetDevice(ctx->device));
    pp_net* net = (pp_net*)ctx->net;
    const void* src = nullptr;
    if (layer == -1) src = pp_first_conv_image(ctx, bytes);
    else if (layer >= 0 && layer < (int)net->layers.size()) { src = net->layers[layer].w; *bytes = net->layers[layer].w_bytes; }
    if (!src) return pp_fail(ctx, PP_E_ARG, "pp_weight_image: no such image");
    if (!dst) return 0;
    if (cap < *bytes) return pp_fail(ctx, PP_E_ARG, "pp_weight_image: dst too small");
    PP_HIP(hipMemcpyAsync(dst, src, *bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream_));
    return 0;
}

// The network's launch plan as text, one line per conv / deconv / head layer in execution order:
//   "<index> kind=<0 conv3x3|1 deconv|2 head> cin=<> cout=<> stride=<> up=<> level=<> wino=<family number> tiling=<name>"
// (bench.py derives the executed MFMA flops of a frame from it and records it in its JSON line).
extern "C" int pp_layer_tilings(pp_ctx* ctx, char* buf, int cap)
{
    if (!ctx || !ctx->net) return 0;
    pp_net* net = (pp_net*)ctx->net;
    std::string t;
    char line[256];
    int i = 0;
    for (const Layer& L : net->layers) {
        snprintf(line, sizeof(line), "%d kind=%d cin=%d cout=%d stride=%d up=%d level=%d wino=%d tiling=%s\n", i++, L.kind, L.cin, L.cout, L.stride, L.up, L.level,
                 (int)L.var.family, L.var.name);
        t += line;
    }
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int)t.size();
}

// The tuner's table (layer signature -> tiling name) as text, one "signature<TAB>tiling" line each: rank 0 of a
// multi-GPU job tunes, exports and broadcasts it, the other ranks import it before they create their context, so
// every rank runs identical kernels.  pp_tune_export returns the length needed (excluding the NUL).
extern "C" int pp_tune_export(char* buf, int cap)
{
    std::string t;
    for (auto& kv : tune_cache()) t += kv.first + "\t" + kv.second + "\n";
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int)t.size();
}

extern "C" int pp_tune_import(const char* text)
{
    if (!text) return PP_E_ARG;
    int n = 0;
    const char* p = text;
    while (*p) {
        const char* e = strchr(p, '\n');
        const size_t len = e ? (size_t)(e - p) : strlen(p);
        std::string line(p, len);
        const size_t tab = line.find('\t');
        if (tab != std::string::npos && tab > 0 && tab + 1 < line.size()) { tune_cache()[line.substr(0, tab)] = line.substr(tab + 1); ++n; }
        p += len + (e ? 1 : 0);
    }
    return n;
}
