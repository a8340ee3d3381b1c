// In-place rewrite of the 16-bit weight images (gfx950): what lets a network train with a 16-bit forward, and lets weights that were
// stepped in fp32 reach a plan committed in a 16-bit mode without a reload.  The 16-bit images hold no transform: they are permutations
// of the weight elements, each rounded to nearest even to bf16 or fp16, and for the split form a second image of the bf16 residuals
// lo = bf16(x - hi) (conv16_pack: [row block][cin/16][hi | lo][tap][k-half][BM][8]; gemm1x1_pack16: [row block][K/16][hi | lo][k-group]
// [BMP][4], which writes the residual image in every mode).  k_image16 writes image element i from the fp32 master tensors on the
// device by the element map of pp_net_image16 (conv_inspect.hip), with the packers' own conversions: the integer rounding of to_bf16,
// the residual as one fp32 subtraction, fp16 through _Float16.  The library is built -ffp-contract=off on both sides, so the image is the
// one a fresh commit of the same values packs, bit for bit.  A layer that keeps an fp32 tiling in a 16-bit plan (a shape no 16-bit
// tiling takes) keeps its fp32 writer: pp_update_image16 reports it and writes nothing.
#include "pp_common.h"

namespace {

constexpr int LAYERS = 20; // 16 convolutions, 3 upsamplers, the head

struct img16_ws {
    pp_image16 img[LAYERS];
    uint64_t gen[LAYERS] = {}; // ctx->commit_gen the entry belongs to (0: none)
    int32_t* map[LAYERS] = {};
};

img16_ws* workspace(pp_ctx* ctx)
{
    if (!ctx->img16) ctx->img16 = new img16_ws();
    return (img16_ws*)ctx->img16;
}

__device__ __forceinline__ uint16_t dev_to_bf16(float f) // to_bf16 of conv_common.h
{
    const uint32_t u = __float_as_uint(f);
    return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// dst[i] = the part map[i] & 1 of element map[i] >> 1 of the concatenation s0 | s1 | s2, 0 where map[i] < 0
template <bool FP16>
__global__ void __launch_bounds__(256) k_image16(uint16_t* __restrict__ dst, const int32_t* __restrict__ map, int n, const float* __restrict__ s0,
                                                 const float* __restrict__ s1, const float* __restrict__ s2, int n0, int n1, int n2)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int m = map[i];
    const int e = m >> 1;
    if (m < 0 || e >= n0 + n1 + n2) { dst[i] = 0; return; }
    const float x = e < n0 ? s0[e] : e < n0 + n1 ? s1[e - n0] : s2[e - n0 - n1];
    uint16_t hi;
    if (FP16) {
        const _Float16 h = (_Float16)x;
        hi = __builtin_bit_cast(uint16_t, h);
    } else {
        hi = dev_to_bf16(x);
    }
    dst[i] = (m & 1) ? dev_to_bf16(x - __uint_as_float((uint32_t)hi << 16)) : hi;
}

// the cached map of `layer`, read back on the first call after a commit
int layer_map(pp_ctx* ctx, int layer, img16_ws** out)
{
    if (layer < 0 || layer >= LAYERS) return pp_fail(ctx, PP_E_ARG, "16-bit image: no such layer");
    img16_ws* ws = workspace(ctx);
    *out = ws;
    if (ws->gen[layer] == ctx->commit_gen) return 0;
    ws->gen[layer] = 0;
    if (int rc = pp_net_image16(ctx, layer, &ws->img[layer])) return rc;
    if (ws->map[layer]) { (void)hipFree(ws->map[layer]); ws->map[layer] = nullptr; }
    const std::vector<int32_t>& m = ws->img[layer].map;
    if (!m.empty()) {
        PP_HIP(hipMalloc((void**)&ws->map[layer], m.size() * sizeof(int32_t)));
        PP_HIP(hipMemcpy(ws->map[layer], m.data(), m.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    ws->gen[layer] = ctx->commit_gen;
    return 0;
}

int write_image(pp_ctx* ctx, const pp_image16& im, const int32_t* map, void* dst, const float* s0, const float* s1, const float* s2, int n0, int n1,
                int n2, hipStream_t stream)
{
    const int n = (int)im.map.size();
    if (im.fp16)
        hipLaunchKernelGGL(k_image16<true>, dim3(pp_div_up(n, 256)), dim3(256), 0, stream, (uint16_t*)dst, map, n, s0, s1, s2, n0, n1, n2);
    else
        hipLaunchKernelGGL(k_image16<false>, dim3(pp_div_up(n, 256)), dim3(256), 0, stream, (uint16_t*)dst, map, n, s0, s1, s2, n0, n1, n2);
    PP_HIP(hipGetLastError());
    return 0;
}

} // namespace

void pp_image16_destroy(pp_ctx* ctx)
{
    img16_ws* ws = (img16_ws*)ctx->img16;
    if (!ws) return;
    for (int32_t* m : ws->map)
        if (m) (void)hipFree(m);
    delete ws;
    ctx->img16 = nullptr;
}

int pp_mp_mode_check(pp_ctx* ctx, const char* who, int mode)
{
    static const char* const names[5] = {"fp32", "bf16x3", "bf16", "fp16", "fp16s"};
    if (mode < 1 || mode > 3)
        return pp_fail(ctx, PP_E_ARG, (std::string(who) + ": mode must be 1 (bf16x3), 2 (bf16) or 3 (fp16); fp16s keeps fp16 tensors, which the taps cannot hand out").c_str());
    const int eff = pp_effective_precision(ctx);
    if (eff != mode)
        return pp_fail(ctx, PP_E_ARG, (std::string(who) + ": called for mode " + names[mode] + ", the committed plan runs " +
                                       (eff >= 0 && eff < 5 ? names[eff] : "nothing")).c_str());
    return 0;
}

int pp_update_image16(pp_ctx* ctx, int layer, const float* s0, const float* s1, const float* s2, int n0, int n1, int n2, hipStream_t stream,
                      bool* is16)
{
    img16_ws* ws = nullptr;
    if (int rc = layer_map(ctx, layer, &ws)) return rc;
    const pp_image16& im = ws->img[layer];
    *is16 = im.is16;
    if (!im.is16) return 0;
    return write_image(ctx, im, ws->map[layer], im.w, s0, s1, s2, n0, n1, n2, stream);
}

// Test hook: k_image16 for layer `layer` of the committed plan into caller memory -- see include/pp_hip.h
extern "C" int pp_debug_image16(pp_ctx* ctx, int layer, const float* w0, const float* w1, const float* w2, void* dst, size_t cap, size_t* bytes,
                                void* stream_)
{
    if (!ctx || !bytes) return pp_fail(ctx, PP_E_ARG, "pp_debug_image16: null pointer");
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_debug_image16: weights not committed");
    PP_HIP(hipSetDevice(ctx->device));
    img16_ws* ws = nullptr;
    if (int rc = layer_map(ctx, layer, &ws)) return rc;
    const pp_image16& im = ws->img[layer];
    if (!im.is16) return pp_fail(ctx, PP_E_ARG, "pp_debug_image16: the layer keeps an fp32 image in the committed plan");
    *bytes = im.bytes;
    if (!dst) return 0;
    if (cap < im.bytes) return pp_fail(ctx, PP_E_ARG, "pp_debug_image16: dst too small");
    if (((uintptr_t)dst & 1) || !w0) return pp_fail(ctx, PP_E_ARG, "pp_debug_image16: null weight or misaligned dst");
    const bool head = layer == LAYERS - 1;
    if (head != (w1 != nullptr) || head != (w2 != nullptr)) return pp_fail(ctx, PP_E_ARG, "pp_debug_image16: w1 and w2 go with the head and with nothing else");
    int total = 0;
    for (int32_t m : im.map)
        if (m >= 0 && (m >> 1) >= total) total = (m >> 1) + 1;
    const int na = ctx->cfg.num_anchor_per_loc;
    const int n0 = head ? na * 320 : total, n1 = head ? 7 * na * 320 : 0, n2 = head ? 2 * na * 320 : 0;
    return write_image(ctx, im, ws->map[layer], dst, w0, w1, w2, n0, n1, n2, (hipStream_t)stream_);
}
