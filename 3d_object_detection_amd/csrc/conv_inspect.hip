// 2D backbone (RPN) + shared head, host side: what tests, training and tools read back from a committed plan.  The weight images as
// index maps (the in-place weight updates of the training code), the tensors of the last pass, one layer on caller tensors
// (pp_debug_layer), the profile bracket's totals, the plan as text and the tuner's table.  The types are in conv_net.h; its one kernel
// is dbg_reduce_stats.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include "conv_net.h"

using namespace ppc;

// L's host weights packed into a scratch image with its committed tiling and read back: map[i] = (int)image[i] - 1
static int packed_indices(pp_ctx* ctx, const Layer& L, bool index_positions, std::vector<int32_t>& map)
{
    Layer scratch = L;
    scratch.w = nullptr;
    int rc = pack_layer(ctx, scratch, index_positions);
    if (rc) { if (scratch.w) (void)hipFree(scratch.w); return rc; }
    std::vector<float> image(scratch.w_bytes / sizeof(float));
    const hipError_t e = hipMemcpy(image.data(), scratch.w, scratch.w_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(scratch.w);
    PP_HIP(e);
    map.resize(image.size());
    for (size_t i = 0; i < image.size(); ++i) map[i] = (int32_t)image[i] - 1;
    return 0;
}

// A packed weight image as an index map (pp_common.h): pack_layer itself packs an index-valued weight (element i of the
// concatenation of the named host tensors holds the float i + 1; exact below 2^24) into a scratch image with the layer's committed
// tiling, so whatever row order (head_tile_row), row padding and K blocking that tiling uses is read back, not restated.  fp32 images
// only: the 16-bit images round their elements, the indices would not survive (pp_net_image16 below reads those back digit by digit).
// Synchronous; called once per commit by train.hip.
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
    const int rc = idx > 16777216.f ? pp_fail(ctx, PP_E_ARG, "weight too large for an index map") : packed_indices(ctx, L, false, wmap);
    for (size_t h = 0; h < names.size(); ++h) ctx->host_w[names[h]].data.swap(saved[h]);
    return rc;
}

// The layout of a conv3x3 layer's fp32 image as a map onto the TRANSFORMED weights: pmap[i] = (row cin + c) T + position of the element
// of [rows][cin][T] that image element i holds (T = 36 wino6, 16 wino / wino4: position a n + b of U = G g G^T; 9 direct: the tap),
// -1 for padding.  The Winograd images hold U, not permuted copies of g, so layer_index_map cannot describe them.
static int layer_position_map(pp_ctx* ctx, const Layer& L, std::vector<int32_t>& pmap, int* T)
{
    const Family f = L.var.family;
    *T = f == Family::Wino6 ? 36 : (f == Family::Wino || f == Family::Wino4) ? 16 : 9;
    if ((size_t)L.cout * L.cin * *T >= 16777216) return pp_fail(ctx, PP_E_ARG, "weight too large for a position map");
    return packed_indices(ctx, L, true, pmap);
}

// The k-th 3 x 3 convolution of the committed plan in execution order (0 .. 15: per level its strided convolution, then its units'),
// for pp_update_conv_image (block_train.hip)
int pp_net_conv_image(pp_ctx* ctx, int k, pp_block_image* img, bool any_plan)
{
    pp_net* net = (pp_net*)ctx->net;
    int seen = 0;
    for (Layer& L : net->layers) {
        if (L.kind != 0 || seen++ != k) continue;
        if ((!any_plan && net->eff_prec != 0) || L.var.prec != 0 || L.var.io16 != 0 || L.var.family == Family::Conv16)
            return pp_fail(ctx, PP_E_ARG, L.stride == 2 ? "the strided convolution can be rewritten in place in the fp32 mode only (the committed plan packs it in a 16-bit format)"
                                                        : "block weights can be rewritten in place in the fp32 mode only (the committed plan packs them in a 16-bit format)");
        if (L.stride == 2 && L.var.family != Family::Direct)
            return pp_fail(ctx, PP_E_ARG, "pp_net_conv_image: the strided convolution does not run a direct tiling");
        int rc = layer_position_map(ctx, L, img->pmap, &img->T);
        if (rc) return rc;
        img->w = L.w;
        img->C = L.cin;
        img->rows = L.cout;
        return 0;
    }
    return pp_fail(ctx, PP_E_ARG, "pp_net_conv_image: no such convolution");
}

int pp_net_head_image(pp_ctx* ctx, pp_head_image* img, bool any_plan)
{
    pp_net* net = (pp_net*)ctx->net;
    Layer& head = net->layers.back();
    if ((!any_plan && net->eff_prec != 0) || head.var.prec != 0 || head.var.io16 != 0)
        return pp_fail(ctx, PP_E_ARG, "head weights can be rewritten in place in the fp32 mode only (the committed plan packs the head in a 16-bit format)");
    const int na = ctx->cfg.num_anchor_per_loc;
    std::vector<std::string> names;
    for (const HeadPart& part : kHead) {
        auto w = ctx->host_w.find(part.weight);
        if (w == ctx->host_w.end() || (int64_t)w->second.data.size() != (int64_t)part.rows_per_anchor * na * head.cin)
            return pp_fail(ctx, PP_E_NAME, (std::string("missing/mis-shaped weight ") + part.weight).c_str());
        names.push_back(part.weight);
    }
    int rc = layer_index_map(ctx, head, names, img->wmap);
    if (rc) return rc;
    img->w = head.w;
    return pp_net_head_bias(ctx, img);
}

// the bias part of pp_net_head_image: it does not depend on the head's tiling or on the precision mode
int pp_net_head_bias(pp_ctx* ctx, pp_head_image* img)
{
    pp_net* net = (pp_net*)ctx->net;
    const int na = ctx->cfg.num_anchor_per_loc;
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
int pp_net_deconv_image(pp_ctx* ctx, int branch, pp_layer_image* img, bool any_plan)
{
    pp_net* net = (pp_net*)ctx->net;
    int seen = 0;
    for (Layer& L : net->layers) {
        if (L.kind != 1 || seen++ != branch) continue;
        if ((!any_plan && net->eff_prec != 0) || L.var.prec != 0 || L.var.io16 != 0)
            return pp_fail(ctx, PP_E_ARG, "upsampler weights can be rewritten in place in the fp32 mode only (the committed plan packs them in a 16-bit format)");
        int rc = layer_index_map(ctx, L, {L.wkey}, img->wmap);
        if (rc) return rc;
        img->w = L.w;
        img->elems = (size_t)L.cin * L.cout * L.up * L.up;
        return 0;
    }
    return pp_fail(ctx, PP_E_ARG, "pp_net_deconv_image: no such upsampler");
}

int pp_net_layer_index(pp_ctx* ctx, int kind, int ordinal)
{
    pp_net* net = (pp_net*)ctx->net;
    int seen = 0;
    for (size_t i = 0; i < net->layers.size(); ++i)
        if (net->layers[i].kind == kind && seen++ == ordinal) return (int)i;
    return -1;
}

// A 16-bit image as an element map (pp_common.h).  An index does not survive one 16-bit rounding, so it goes through the packer digit
// by digit: in pass p element e of the concatenated host tensors holds digit_value((e / 128^p) % 128), a value whose rounded part and
// whose bf16 residual are both exact, non-zero and different for every digit, and an image element is recognised by its bits.  The
// two tables come from the packers' own conversions (conv_common.h), so the part of an element -- rounded value or residual -- is
// read back with its index; zero bits in every pass are padding.
static const int kDigits = 128;
static inline float digit_value(int d) { return (float)(d + 1) * (1.f / 256.f) * (1.f + 1.f / 512.f); }

int pp_net_image16(pp_ctx* ctx, int layer, pp_image16* img)
{
    pp_net* net = (pp_net*)ctx->net;
    if (layer < 0 || layer >= (int)net->layers.size()) return pp_fail(ctx, PP_E_ARG, "pp_net_image16: no such layer");
    const Layer& L = net->layers[layer];
    img->w = L.w;
    img->bytes = L.w_bytes;
    img->map.clear();
    img->fp16 = L.var.prec == 3;
    img->is16 = L.var.family == Family::Conv16 || (L.var.family == Family::Gemm1x1 && L.var.prec != 0); // pack_layer's own rule
    if (!img->is16) return 0;
    if (L.var.io16 != 0) return pp_fail(ctx, PP_E_ARG, "pp_net_image16: the committed plan runs fp16 tensors (fp16s)");
    std::vector<std::string> names;
    if (L.kind == 2)
        for (const HeadPart& part : kHead) names.push_back(part.weight);
    else
        names.push_back(L.wkey);
    // the two parts of every digit, by the packers' conversions
    std::map<uint16_t, int> hi_of, lo_of;
    for (int d = 0; d < kDigits; ++d) {
        const float x = digit_value(d);
        uint16_t hi = to_bf16(x);
        if (img->fp16) { const _Float16 h16 = (_Float16)x; memcpy(&hi, &h16, 2); }
        const uint16_t lo = to_bf16(x - from_bf16(hi));
        hi_of[hi] = d; lo_of[lo] = d;
    }
    bool distinct = (int)hi_of.size() == kDigits && (int)lo_of.size() == kDigits && !hi_of.count(0) && !lo_of.count(0);
    for (auto& kv : hi_of) distinct = distinct && !lo_of.count(kv.first);
    if (!distinct) return pp_fail(ctx, PP_E_STATE, "pp_net_image16: the digit values do not round to distinct parts");
    std::vector<std::vector<float>> saved(names.size());
    size_t total = 0;
    for (size_t h = 0; h < names.size(); ++h) {
        auto w = ctx->host_w.find(names[h]);
        if (w == ctx->host_w.end()) return pp_fail(ctx, PP_E_NAME, ("missing weight " + names[h]).c_str());
        total += w->second.data.size();
    }
    if (total > (size_t)kDigits * kDigits * kDigits) return pp_fail(ctx, PP_E_ARG, "pp_net_image16: weight too large for three base-128 digits");
    for (size_t h = 0; h < names.size(); ++h) saved[h] = ctx->host_w[names[h]].data;
    const size_t n = L.w_bytes / sizeof(uint16_t);
    std::vector<uint16_t> image(n);
    std::vector<int32_t> idx(n, 0), part(n, -1); // part: -1 padding so far
    int rc = 0;
    size_t div = 1;
    for (int p = 0; p < 3 && !rc; ++p, div *= kDigits) {
        size_t e = 0;
        for (size_t h = 0; h < names.size(); ++h)
            for (float& v : ctx->host_w[names[h]].data) v = digit_value((int)((e++ / div) % kDigits));
        Layer scratch = L;
        scratch.w = nullptr;
        rc = pack_layer(ctx, scratch);
        if (!rc && scratch.w_bytes != L.w_bytes) rc = pp_fail(ctx, PP_E_STATE, "pp_net_image16: the scratch image has another size");
        if (!rc) {
            const hipError_t e = hipMemcpy(image.data(), scratch.w, scratch.w_bytes, hipMemcpyDeviceToHost);
            if (e != hipSuccess) rc = pp_fail_hip(ctx, e, "hipMemcpy (pp_net_image16)", __FILE__, __LINE__);
        }
        if (scratch.w) (void)hipFree(scratch.w);
        for (size_t i = 0; i < n && !rc; ++i) {
            const uint16_t b = image[i];
            const auto hi = hi_of.find(b), lo = lo_of.find(b);
            const int pt = b == 0 ? -1 : hi != hi_of.end() ? 0 : lo != lo_of.end() ? 1 : -2;
            if (pt == -2 || (p > 0 && pt != part[i])) { rc = pp_fail(ctx, PP_E_STATE, "pp_net_image16: an image element is no part of a digit"); break; }
            part[i] = pt;
            if (pt >= 0) idx[i] += (int32_t)((pt ? lo->second : hi->second) * div);
        }
    }
    for (size_t h = 0; h < names.size(); ++h) ctx->host_w[names[h]].data.swap(saved[h]);
    if (rc) return rc;
    img->map.resize(n);
    for (size_t i = 0; i < n; ++i) {
        if (part[i] >= 0 && (size_t)idx[i] >= total) return pp_fail(ctx, PP_E_STATE, "pp_net_image16: an image element names no weight");
        img->map[i] = part[i] < 0 ? -1 : 2 * idx[i] + part[i];
    }
    return 0;
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
    ConvCall c;
    c.in = (const float*)in; c.Hin = hin; c.Win = win; c.out = (float*)out; c.Hout = h; c.Wout = w; c.res = (const float*)res;
    c.pre = pre; c.stat = st; c.stat_C = L.cout; c.out_box = out_box; c.out_dir = out_dir; c.nb = nb;
    c.pmap = pmap; c.feat = feat; c.ts_k = active ? skip_k : 0;
    const int rc = launch_conv(ctx, L, c, stream);
    if (active) pp_ts_end_hook(ctx);
    if (rc == PP_E_ARG) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the committed tiling does not take this layer's shape");
    if (rc) return rc;
    if (stats) {
        hipLaunchKernelGGL(dbg_reduce_stats, dim3(pp_div_up(2 * L.cout, 256), nb), dim3(256), 0, stream, st, STAT_FS, L.cout, stats);
        PP_HIP(hipGetLastError());
    }
    return 0;
}

// Test hook: the cls-only head pass of the deferred head -- launch_head_cls with the committed cls tiling on the head's image -- on
// caller tensors; see include/pp_hip.h.  Writes only cls_out.
extern "C" int pp_debug_head_cls(pp_ctx* ctx, int nb, const void* in, int pre_mode, const float* scale, const float* shift, float* cls_out, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->net || !ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_debug_head_cls: weights not committed");
    pp_net* net = (pp_net*)ctx->net;
    if (!net->defer_ok) return pp_fail(ctx, PP_E_STATE, "pp_debug_head_cls: the committed plan has no deferred head (fp32 mode, 9-anchor head on a gemm1x1 tiling)");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_debug_head_cls: nb must be 1 .. cfg.max_batch");
    if (!in) return pp_fail(ctx, PP_E_ARG, "pp_debug_head_cls: null input");
    if (!cls_out) return pp_fail(ctx, PP_E_ARG, "pp_debug_head_cls: null output");
    if (pre_mode < 0 || pre_mode > 2) return pp_fail(ctx, PP_E_ARG, "pp_debug_head_cls: pre_mode must be 0 (raw), 1 (shared affine) or 2 (per-frame affine)");
    if ((pre_mode != 0) != (scale != nullptr) || (pre_mode != 0) != (shift != nullptr))
        return pp_fail(ctx, PP_E_ARG, "pp_debug_head_cls: scale and shift go with pre_mode 1 / 2 and with nothing else");
    const int cin = net->layers.back().cin;
    NormRef pre;
    if (pre_mode) { pre.mode = PRE_AFFINE; pre.scale = const_cast<float*>(scale); pre.shift = const_cast<float*>(shift); pre.C = cin; pre.aff_fs = pre_mode == 2 ? (size_t)cin : 0; }
    const int rc = launch_head_cls(ctx, net->cls_var, (const float*)in, pre, cls_out, nb, (hipStream_t)stream_);
    if (rc == PP_E_ARG) return pp_fail(ctx, PP_E_ARG, "pp_debug_head_cls: the cls tiling does not take the head's map");
    return rc;
}

// The committed tiling of the cls-only head pass ("" when the plan has no deferred head)
extern "C" const char* pp_head_cls_tiling(pp_ctx* ctx)
{
    if (!ctx || !ctx->net || !ctx->weights_ready) return "";
    const pp_net* net = (const pp_net*)ctx->net;
    return net->defer_ok ? net->cls_var.name : "";
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
