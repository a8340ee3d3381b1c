// Host side that the three training backwards share (block_train, down_train, neck_train and their 16-bit twins): the refusal of an
// argument, workspace growth, the padded-plane geometry of the unit and stage backwards, the frame chunks of a call with the K ranges
// of each chunk's wgrad launch, and the reduction of the dw partials.  One copy, so that every entry cuts the batch and K and sums
// the partials the same way; the family headers keep their workspace struct, their constants and their kernels.
#pragma once
#include <string>
#include "pp_common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int DW_WGS = 512; // workgroups a wgrad launch aims at (output tiles x K ranges)
constexpr int DW_MAX_SPLIT = 256;

enum norm_form { NORM_INSTANCE, NORM_AFFINE, NORM_BATCH }; // InstanceNorm, a frozen BatchNorm's affine, a train-mode BatchNorm

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// "<entry>: <what>" as the context's last error
inline int train_fail(pp_ctx* ctx, const char* entry, const char* what) { return pp_fail(ctx, PP_E_ARG, (std::string(entry) + ": " + what).c_str()); }

// Waits for the device, not for the caller's stream alone: a kernel of an earlier call, on this stream or another, may still read the
// old buffer.  Only the rare call that grows a buffer pays for it.
template <typename T>
int grow(pp_ctx* ctx, T** buf, size_t* have, size_t need)
{
    if (need <= *have) return 0;
    PP_HIP(hipDeviceSynchronize());
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *have = 0;
    PP_HIP(hipMalloc((void**)buf, need * sizeof(T)));
    *have = need;
    return 0;
}

// ---- the padded plane of an h x w map (block_train.hip, down_train.hip at half resolution): the (h + 2) x wp zero-haloed image, wp =
// w + 2, PP = (h + 2) wp elements, between two guard bands of G >= wp + 17 zeros, PS elements in all (G and PS multiples of 4).  elems
// is PS before it is narrowed: the budget test of a call reads it, and a map that passes it fits the ints ----------------------------
struct pad_geom { int wp, PP, G, PS; uint64_t elems; };
inline pad_geom padded_plane(int64_t h, int64_t w)
{
    const int64_t wp = w + 2, PP = (h + 2) * wp, G = ((wp + 1 + 3) & ~(int64_t)3) + 16, PS = (2 * G + PP + 3) & ~(int64_t)3;
    return pad_geom{(int)wp, (int)PP, (int)G, (int)PS, (uint64_t)PS};
}

// K ranges of one wgrad launch over `nchunks` chunks of positions (16 per chunk in the fp32 kernels, 32 in the 16-bit ones)
inline void dw_ranges(int tiles, int nchunks, int* splits, int* cps, int wgs = DW_WGS)
{
    int sp = wgs / tiles;
    sp = sp < 1 ? 1 : sp > DW_MAX_SPLIT ? DW_MAX_SPLIT : sp;
    if (sp > nchunks) sp = nchunks;
    *cps = (nchunks + sp - 1) / sp;
    *splits = (nchunks + *cps - 1) / *cps;
}

// ---- the frame chunks of a call: nb frames in runs of fc, each with the K ranges of its wgrad launch over fn x cpf chunks of positions
// (sp ranges of cps chunks) and the index gbase of its first dw partial.  body(chunk) runs once per chunk in frame order; the return
// value is the number of partials.  A plan counts them with an empty body and the driver launches from the same walk, so the two cannot
// disagree about fn or the ranges ------------------------------------------------------------------------------------------------------
struct dw_walk { int nb, fc, tiles, cpf, wgs; };
struct dw_chunk { int f0, fn, nchunks, sp, cps, gbase; };
template <typename F>
int for_chunks(const dw_walk& k, F body)
{
    int gbase = 0;
    for (int f0 = 0; f0 < k.nb; f0 += k.fc) {
        dw_chunk c;
        c.f0 = f0; c.fn = k.nb - f0 < k.fc ? k.nb - f0 : k.fc; c.nchunks = c.fn * k.cpf; c.gbase = gbase;
        dw_ranges(k.tiles, c.nchunks, &c.sp, &c.cps, k.wgs);
        body(c);
        gbase += c.sp;
    }
    return gbase;
}
inline int count_partials(const dw_walk& k) { return for_chunks(k, [](const dw_chunk&) {}); }

// partials added in index order (double, rounded once), four loads in flight: 64-thread workgroups, so that a 64 x 64 weight spreads
// over all compute units
__global__ void __launch_bounds__(64) k_dw_reduce(const float* __restrict__ part, int G, int n, float* __restrict__ dw)
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
inline void launch_dw_reduce(const float* part, int Gp, int nw, float* dw, hipStream_t stream)
{
    hipLaunchKernelGGL(k_dw_reduce, dim3(pp_div_up(nw, 64)), dim3(64), 0, stream, part, Gp, nw, dw);
}

} // namespace
