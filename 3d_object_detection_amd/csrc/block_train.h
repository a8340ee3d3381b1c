// What block_train.hip (the fp32 Resnet unit backward) and block_train16.hip (its 16-bit operand twins) share: the workspace of a
// context and its budget rules, the K ranges of a wgrad launch and the reduction of the dw partials.  One copy, so that both files
// cut K and sum the partials the same way.
#pragma once
#include "pp_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr size_t WS_BUDGET = (size_t)256 << 20; // bytes of one frame's a + dz planes: a larger map is refused
constexpr size_t WS_CHUNK = (size_t)1 << 30;    // bytes of the planes of one chunk of frames: larger batches run in frame chunks
constexpr int DW_WGS = 512;                     // workgroups a wgrad launch aims at (output tiles x K ranges)
constexpr int DW_MAX_SPLIT = 256;
constexpr int DA_BLOCK = 64;                    // k-terms that k_unit_dgrad sums in one accumulator before adding the block to the total

struct block_ws {
    float* planes = nullptr; size_t planes_elems = 0; // a [fc][C][PS], then dz [fc][C][PS]
    float* stm = nullptr;    size_t stm_elems = 0;    // [fc][C][2]: mean, rstd as the forward rounds them
    double* pst = nullptr;   size_t pst_elems = 0;    // [fc][C][segments][2]: a plane's segment sums (statistics, then the norm backward's)
    float* wT = nullptr;     size_t wT_elems = 0;
    float* part = nullptr;   size_t part_elems = 0;
    uint16_t* img16 = nullptr; size_t img16_elems = 0; // the 16-bit operand images of pp_unit_backward_mp (block_train16.hip)
    uint16_t* wT16 = nullptr;  size_t wT16_elems = 0;  // [part][9][ci][co] bf16
    // pp_update_conv_image: the committed images of the sixteen 3 x 3 convolutions in execution order and their position maps on
    // the device, each entry read back on its first use after a commit
    uint64_t img_gen[16] = {}; // ctx->commit_gen the entry belongs to (0: none)
    pp_block_image img[16];
    int32_t* pmap[16] = {};
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

// partials added in index order, four loads in flight: 64-thread workgroups, so that a 64 x 64 weight spreads over all compute units
__global__ void __launch_bounds__(64) k_unit_dw_reduce(const float* __restrict__ part, int G, int n, float* __restrict__ dw)
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

inline block_ws* workspace(pp_ctx* ctx)
{
    if (!ctx->blk) ctx->blk = new block_ws();
    return (block_ws*)ctx->blk;
}

// K ranges of one wgrad launch over `nchunks` chunks of positions (16 per chunk in the fp32 kernels, 32 in the 16-bit ones)
inline void dw_ranges(int tiles, int nchunks, int* splits, int* cps)
{
    int sp = DW_WGS / tiles;
    sp = sp < 1 ? 1 : sp > DW_MAX_SPLIT ? DW_MAX_SPLIT : sp;
    if (sp > nchunks) sp = nchunks;
    *cps = (nchunks + sp - 1) / sp;
    *splits = (nchunks + *cps - 1) / *cps;
}

} // namespace
