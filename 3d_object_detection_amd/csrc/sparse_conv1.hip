// Sparse first convolution of the fused path (fp32): 3x3, stride 2, 64 -> 64 from the pillar map to the level-0 map, computed for
// the output pixels that see a pillar only (about 5 % of an 800 x 800 LiDAR frame; conv_mfma skips whole 16 x 10 patches and still
// executes 37 % of the dense MFMAs).
//
//   sc1_ballot_b   one thread per output pixel: does one of its in-image 3x3 input cells hold a pillar?  A ballot word per 64
//                  pixels and the popcount of every 256-pixel block.
//   sc1_write_b    the active list in ASCENDING pixel index: a block's base rank is the sum of the block counts in front of it, a
//                  pixel's rank the set bits below it.  Integer sums only, so list and count are the same on every run (an atomic
//                  append would reorder the list from run to run, and with it the fp32 grouping of the statistics).  Next to the
//                  list: the byte offsets of the 9 PFN rows of every active pixel, stored XOR SC1_PARK (0 = a tap without a pillar,
//                  which is also what a parked read of the table returns).
//   sc1_gather     D[64 cout, pixel] = sum over (tap, cin) W . feat[pid(tap, pixel)][cin] on v_mfma_f32_16x16x4_f32.  A wave owns 64
//                  consecutive list entries (4 N-tiles x 4 M-tiles, 64 accumulator registers) and works alone: no LDS, no barrier.
//                  B operands are gathered with buffer loads (a lane whose tap has no pillar, or whose entry is past the count,
//                  loads through an offset parked out of range and receives 0: no branch per element).  The 144 steps run in the K
//                  order of the committed dense tiling (see sc1_c4 / sc1_tap), so the convolution's output is the dense one's bit
//                  for bit.  A operands come from L2: the weight image [step][lane][M-tile] makes every step one coalesced 1 KB
//                  dwordx4 load per wave, shared by the 4 N-tiles; operands run a group of 4 steps (64 MFMAs) ahead.
//                  Epilogue: scatter into the zero-filled dense [64, H, W] map; per-channel sum / sum of squares of the wave's 64
//                  pixels in fp64, then one fp64 atomic per channel and wave into the replicated slots (replica = wave index).
//
// Work assignment and partial-sum grouping depend on the frame's own list alone: a frame computes the same whatever the batch is.
#include <algorithm>
#include <cstring>
#include "pp_common.h"
#include "conv_common.h"

namespace {

using namespace ppc;

constexpr unsigned SC1_PARK = 0x80000000u; // buffer offset no descriptor of this file reaches: loads return 0, stores are dropped
constexpr int SC1_NT = 4;                  // N-tiles (16 list entries each) per wave
constexpr int SC1_WAVE_PX = 16 * SC1_NT;
constexpr int SC1_W_FLOATS = 9 * 64 * 64;

struct Sc1 {
    float* w = nullptr;        // [step][lane][M-tile], steps in the K order of `kc` (sc1_c4 / sc1_tap)
    int kc = 4;
    uint64_t* words = nullptr; // [max_batch][nblk * 4] ballot words
    int32_t* bcnt = nullptr;   // [max_batch][nblk] active pixels per 256-pixel block
    int32_t* list = nullptr;   // [max_batch][cap_pad] active pixel indices, ascending
    uint32_t* tab = nullptr;   // [max_batch][9][cap_pad] byte offset of the PFN row of (tap, entry) ^ SC1_PARK; 0 = no pillar
    int32_t* count = nullptr;  // [max_batch]
    int cap = 0, cap_pad = 0, nblk = 0;
    bool weights = false;
};

struct Sc1P {
    const int32_t* pmap; size_t pmap_fs;
    const float* feat; size_t feat_fs; unsigned feat_bytes;
    const float* w;
    float* out; size_t out_fs;
    double* stat; size_t stat_fs;
    uint64_t* words; int32_t* bcnt; int32_t* list; uint32_t* tab; int32_t* count;
    int Hin, Win, Hout, Wout, cap, cap_pad, nblk, max_voxels;
};

__global__ void __launch_bounds__(256) sc1_ballot_b(const Sc1P p)
{
    __shared__ int wc[4];
    const int f = blockIdx.z;
    const int32_t* __restrict__ gmap = p.pmap + (size_t)f * p.pmap_fs;
    const int pix = blockIdx.x * 256 + threadIdx.x;
    bool act = false;
    if (pix < p.Hout * p.Wout) {
        const int oy = pix / p.Wout, ox = pix - oy * p.Wout;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky) {
            const int iy = 2 * oy - 1 + ky;
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                const int ix = 2 * ox - 1 + kx;
                if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) act |= gmap[(size_t)iy * p.Win + ix] >= 0;
            }
        }
    }
    const uint64_t b = __ballot(act);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
        p.words[((size_t)f * p.nblk + blockIdx.x) * 4 + wave] = b;
        wc[wave] = __popcll(b);
    }
    __syncthreads();
    if (threadIdx.x == 0) p.bcnt[(size_t)f * p.nblk + blockIdx.x] = wc[0] + wc[1] + wc[2] + wc[3];
}

__global__ void __launch_bounds__(256) sc1_write_b(const Sc1P p)
{
    __shared__ int red[4];
    const int f = blockIdx.z, blk = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t* __restrict__ wd = p.words + ((size_t)f * p.nblk + blk) * 4;
    const int32_t* __restrict__ bc = p.bcnt + (size_t)f * p.nblk;
    const uint64_t w0 = wd[0], w1 = wd[1], w2 = wd[2], w3 = wd[3];
    const int c0 = __popcll(w0), c1 = __popcll(w1), c2 = __popcll(w2), c3 = __popcll(w3);
    const int own = c0 + c1 + c2 + c3;
    const bool last = blk == p.nblk - 1;
    if (own == 0 && !last) return; // block-uniform
    int s = 0;
    for (int i = tid; i < blk; i += 256) s += bc[i];
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) s += __shfl_xor(s, d);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    const int prefix = red[0] + red[1] + red[2] + red[3];
    if (last && tid == 0) {
        const int total = prefix + own;
        p.count[f] = total < p.cap ? total : p.cap;
    }
    const uint64_t mw = wave == 0 ? w0 : wave == 1 ? w1 : wave == 2 ? w2 : w3;
    const int before = prefix + (wave > 0 ? c0 : 0) + (wave > 1 ? c1 : 0) + (wave > 2 ? c2 : 0);
    const int rank = before + __popcll(mw & ((1ull << lane) - 1ull));
    if (!((mw >> lane) & 1ull) || rank >= p.cap) return;
    const int pix = blk * 256 + tid;
    const int oy = pix / p.Wout, ox = pix - oy * p.Wout;
    const int32_t* __restrict__ gmap = p.pmap + (size_t)f * p.pmap_fs;
    p.list[(size_t)f * p.cap_pad + rank] = pix;
    uint32_t* __restrict__ tb = p.tab + (size_t)f * 9 * p.cap_pad + rank;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = 2 * oy - 1 + ky;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = 2 * ox - 1 + kx;
            int id = -1;
            if (iy >= 0 && iy < p.Hin && ix >= 0 && ix < p.Win) id = gmap[(size_t)iy * p.Win + ix];
            tb[(size_t)(ky * 3 + kx) * p.cap_pad] = (id >= 0 && id < p.max_voxels) ? ((unsigned)id * 256u) ^ SC1_PARK : 0u;
        }
    }
}

// K order of the gather-GEMM: the 144 MFMA steps (input-channel quad c4, tap) in the order the committed DENSE tiling of the first
// conv (conv_mfma with KC channels per chunk) accumulates them -- chunk, tap, quad within the chunk -- so that switching the sparse
// path on or off changes no bit of the convolution's output (empty taps add exact zeros on both sides); what is left between the
// two modes is the grouping of the statistics' partial sums.
template <int KC> constexpr int sc1_c4(int q) { return KC == 8 ? (q / 18) * 2 + (q % 18) % 2 : q / 9; }
template <int KC> constexpr int sc1_tap(int q) { return KC == 8 ? (q % 18) / 2 : q % 9; }

template <int KC>
__global__ void __launch_bounds__(256) sc1_gather(const Sc1P p)
{
    constexpr int NT = SC1_NT;
    const int f = blockIdx.z;
    const int lane = threadIdx.x & 63, n = lane & 15, kq = lane >> 4;
    const int wv = blockIdx.x * 4 + (threadIdx.x >> 6); // wave index within the frame
    const int cnt = p.count[f];
    const int e0 = wv * SC1_WAVE_PX;
    if (e0 >= cnt) return; // wave-uniform; e0 + 63 < cap_pad from here on
    const __amdgpu_buffer_rsrc_t rf = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.feat + (size_t)f * p.feat_fs), 0, p.feat_bytes, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, SC1_W_FLOATS * 4, 0x00020000);
    // list and table are read through descriptors as well: an entry past the count parks its offset, reads 0 = "no pillar" and
    // costs no branch (a guarded plain load is compiled to a branch with a full s_waitcnt, which drains the operand prefetch)
    const __amdgpu_buffer_rsrc_t rt = __builtin_amdgcn_make_buffer_rsrc(p.tab + (size_t)f * 9 * p.cap_pad, 0, (unsigned)p.cap_pad * 36u, 0x00020000);
    const __amdgpu_buffer_rsrc_t rl = __builtin_amdgcn_make_buffer_rsrc(p.list + (size_t)f * p.cap_pad, 0, (unsigned)p.cap_pad * 4u, 0x00020000);
    bool valid[NT];
    unsigned eo[NT]; // byte offset of the lane's entry in the list / in one tap's row of the table
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        valid[t] = e0 + t * 16 + n < cnt;
        eo[t] = valid[t] ? (unsigned)(e0 + t * 16 + n) * 4u : SC1_PARK;
    }
    // byte offset of the lane's channel (kq of a quad) in the PFN row of every (N-tile, tap)
    const unsigned tap_b = (unsigned)p.cap_pad * 4u;
    unsigned vo[NT][9];
#pragma unroll
    for (int tap = 0; tap < 9; ++tap)
#pragma unroll
        for (int t = 0; t < NT; ++t) vo[t][tap] = (__builtin_amdgcn_raw_buffer_load_b32(rt, eo[t], (unsigned)tap * tap_b, 0) ^ SC1_PARK) + (unsigned)kq * 4u;

    f32x4 a[2][4];
    float b[2][4][NT];
    f32x4 acc[4][NT];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[i][t] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // operands of group G = MFMA steps 4 G .. 4 G + 3
#define SC1_LOAD_OPS(G, SET)                                                                                   \
    pp_steps<0, 4>([&](auto S_) {                                                                              \
        constexpr int q_ = (G) * 4 + decltype(S_)::value, sl_ = decltype(S_)::value;                           \
        _Pragma("unroll") for (int t = 0; t < NT; ++t)                                                         \
            b[SET][sl_][t] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rf, vo[t][sc1_tap<KC>(q_)] + sc1_c4<KC>(q_) * 16, 0, 0)); \
        a[SET][sl_] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (unsigned)lane * 16u, q_ * 1024, 0)); \
    });
    SC1_LOAD_OPS(0, 0)
    pp_steps<0, 36>([&](auto G) {
        constexpr int g_ = decltype(G)::value;
        constexpr int cur = g_ & 1;
        if constexpr (g_ + 1 < 36) SC1_LOAD_OPS(g_ + 1, cur ^ 1)
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < 4; ++s)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int t = 0; t < NT; ++t)
                    acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur][s][i], b[cur][s][t], acc[i][t], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    });
#undef SC1_LOAD_OPS

    // ---- epilogue: lane holds rows 16 i + 4 kq + r of pixel (N-tile t, column n) ----
    const unsigned plane_b = (unsigned)(p.Hout * p.Wout) * 4u;
    const __amdgpu_buffer_rsrc_t ro = __builtin_amdgcn_make_buffer_rsrc(p.out + (size_t)f * p.out_fs, 0, plane_b * 64u, 0x00020000);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
        const unsigned pix = __builtin_amdgcn_raw_buffer_load_b32(rl, eo[t], 0, 0);
        const unsigned oo = valid[t] ? pix * 4u + (unsigned)kq * 4u * plane_b : SC1_PARK;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float x = acc[i][t][r]; // a copy: __builtin_bit_cast on a vector element reads element 0
                __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(unsigned, x), ro, oo, (unsigned)(i * 16 + r) * plane_b, 0);
            }
    }
    if (p.stat) {
        // Sum and sum of the fp32 squares, accumulated in fp64 from the first addition: the 64 pixels of a wave are list neighbours, not
        // map neighbours, so an fp32 partial sum here would round differently from any tiling of the map.  Entries past the count
        // accumulated zeros and add nothing.
        double* __restrict__ gs = p.stat + (size_t)f * p.stat_fs + (size_t)(wv % NREP) * 64 * 2;
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double s = 0.0, q = 0.0;
#pragma unroll
                for (int t = 0; t < NT; ++t) { const float x = acc[i][t][r]; const float xx = x * x; s += (double)x; q += (double)xx; }
#pragma unroll
                for (int d = 1; d < 16; d <<= 1) { s += __shfl_xor(s, d); q += __shfl_xor(q, d); }
                if (n == 0) {
                    double* dst = gs + (size_t)(i * 16 + kq * 4 + r) * 2;
                    atomicAdd(dst, s);
                    atomicAdd(dst + 1, q);
                }
            }
    }
}

// the (step, lane, i) map of pp_sc1_commit on the device: image element e = (q 64 + lane) 4 + i of the weight image from the state_dict
// tensor w [64][64][3][3]
template <int KC>
__global__ void __launch_bounds__(256) first_conv_image(const float* __restrict__ w, float* __restrict__ img)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= SC1_W_FLOATS) return;
    const int i = e & 3, lane = (e >> 2) & 63, q = e >> 8;
    const int co = 16 * i + (lane & 15), ci = 4 * sc1_c4<KC>(q) + (lane >> 4);
    img[e] = w[((size_t)co * 64 + ci) * 9 + sc1_tap<KC>(q)];
}

template <typename T>
hipError_t sc1_alloc(T** q, size_t count) { return hipMalloc((void**)q, count * sizeof(T) + 256); }

} // namespace

int pp_sc1_create(pp_ctx* ctx)
{
    Sc1* S = new Sc1();
    ctx->sc1 = S;
    const size_t HW = (size_t)ctx->H * ctx->W, mb = (size_t)ctx->max_batch;
    const size_t cap = std::min((size_t)4 * ctx->cfg.max_voxels, HW); // a pillar is seen by at most 2 x 2 output pixels
    S->cap = (int)cap;
    S->cap_pad = (int)((cap + SC1_WAVE_PX - 1) / SC1_WAVE_PX) * SC1_WAVE_PX;
    S->nblk = pp_div_up((int64_t)HW, 256);
    PP_HIP(sc1_alloc(&S->w, (size_t)SC1_W_FLOATS));
    PP_HIP(sc1_alloc(&S->words, mb * S->nblk * 4));
    PP_HIP(sc1_alloc(&S->bcnt, mb * S->nblk));
    PP_HIP(sc1_alloc(&S->list, mb * S->cap_pad));
    PP_HIP(sc1_alloc(&S->tab, mb * 9 * S->cap_pad));
    PP_HIP(sc1_alloc(&S->count, mb));
    PP_HIP(hipMemset(S->list, 0, mb * S->cap_pad * sizeof(int32_t)));
    PP_HIP(hipMemset(S->tab, 0, mb * 9 * S->cap_pad * sizeof(uint32_t)));
    PP_HIP(hipMemset(S->count, 0, mb * sizeof(int32_t)));
    return 0;
}

void pp_sc1_destroy(pp_ctx* ctx)
{
    Sc1* S = (Sc1*)ctx->sc1;
    if (!S) return;
    void* ptrs[] = {S->w, S->words, S->bcnt, S->list, S->tab, S->count};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    delete S;
    ctx->sc1 = nullptr;
}

// first conv's weight [cout][cin][3][3] -> [step][lane][M-tile]: cout = 16 i + (lane & 15), cin = 4 c4(step) + (lane >> 4), tap(step)
int pp_sc1_commit(pp_ctx* ctx)
{
    Sc1* S = (Sc1*)ctx->sc1;
    S->weights = false;
    auto it = ctx->host_w.find("rpn.block1.0.weight");
    if (it == ctx->host_w.end() || it->second.data.size() != (size_t)SC1_W_FLOATS)
        return pp_fail(ctx, PP_E_NAME, "missing/mis-shaped weight rpn.block1.0.weight");
    const std::vector<float>& w = it->second.data;
    std::vector<float> img((size_t)SC1_W_FLOATS);
    S->kc = ctx->sc1_kc == 8 ? 8 : 4;
    for (int q = 0; q < 144; ++q) {
        const int c4 = S->kc == 8 ? sc1_c4<8>(q) : sc1_c4<4>(q), tap = S->kc == 8 ? sc1_tap<8>(q) : sc1_tap<4>(q);
        for (int lane = 0; lane < 64; ++lane)
            for (int i = 0; i < 4; ++i) {
                const int co = 16 * i + (lane & 15), ci = 4 * c4 + (lane >> 4);
                img[((size_t)q * 64 + lane) * 4 + i] = w[((size_t)co * 64 + ci) * 9 + tap];
            }
    }
    PP_HIP(hipMemcpy(S->w, img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    S->weights = true;
    return 0;
}

// rpn.block1.0.weight on the device -> the committed image, in its K order, on `stream` (pp_update_rpn_weights).  No-op before the
// first commit: there is no image to keep in step.
int pp_sc1_update(pp_ctx* ctx, const float* w, hipStream_t stream)
{
    Sc1* S = (Sc1*)ctx->sc1;
    if (!S || !S->weights) return 0;
    hipLaunchKernelGGL(S->kc == 8 ? first_conv_image<8> : first_conv_image<4>, dim3(pp_div_up(SC1_W_FLOATS, 256)), dim3(256), 0, stream, w, S->w);
    PP_HIP(hipGetLastError());
    return 0;
}

const float* pp_first_conv_image(pp_ctx* ctx, size_t* bytes)
{
    const Sc1* S = (const Sc1*)ctx->sc1;
    if (!S || !S->weights) return nullptr;
    *bytes = (size_t)SC1_W_FLOATS * sizeof(float);
    return S->w;
}

// The sparse path serves maps whose dense output a 32-bit buffer offset can address (the parked offset sits 2 GB out).
bool pp_sc1_usable(pp_ctx* ctx)
{
    const Sc1* S = (const Sc1*)ctx->sc1;
    return ctx->sparse_conv1 && S && S->weights && (size_t)64 * ctx->H * ctx->W * 4 < 0x7F000000ull &&
           (size_t)ctx->cfg.max_voxels * 256 < 0x7F000000ull;
}

// nb pillar maps [gx, gy] + PFN rows -> zero-filled dense out [nb][64, H, W] with the active pixels computed, statistics added to
// `stat` (nullable: the BatchNorm variant has no statistics slot).  Enqueued on `stream`.
int pp_sc1_run(pp_ctx* ctx, const int32_t* pmap, const float* feat, float* out, double* stat, size_t stat_fs, int nb, hipStream_t stream)
{
    Sc1* S = (Sc1*)ctx->sc1;
    const size_t HW = (size_t)ctx->H * ctx->W;
    ctx->sc1_last_nb = 0;
    PP_HIP(hipMemsetAsync(out, 0, (size_t)nb * 64 * HW * sizeof(float), stream));
    for (int b0 = 0; b0 < nb; b0 += PP_GROUP) {
        const int g = nb - b0 < PP_GROUP ? nb - b0 : PP_GROUP;
        Sc1P p;
        memset(&p, 0, sizeof(p));
        p.pmap_fs = (size_t)ctx->gx * ctx->gy; p.pmap = pmap + b0 * p.pmap_fs;
        p.feat_fs = (size_t)ctx->cfg.max_voxels * 64; p.feat = feat + b0 * p.feat_fs;
        p.feat_bytes = (unsigned)(p.feat_fs * 4);
        p.w = S->w;
        p.out_fs = 64 * HW; p.out = out + b0 * p.out_fs;
        p.stat_fs = stat_fs; p.stat = stat ? stat + b0 * stat_fs : nullptr;
        p.words = S->words + (size_t)b0 * S->nblk * 4; p.bcnt = S->bcnt + (size_t)b0 * S->nblk;
        p.list = S->list + (size_t)b0 * S->cap_pad; p.tab = S->tab + (size_t)b0 * 9 * S->cap_pad; p.count = S->count + b0;
        p.Hin = ctx->gx; p.Win = ctx->gy; p.Hout = ctx->H; p.Wout = ctx->W;
        p.cap = S->cap; p.cap_pad = S->cap_pad; p.nblk = S->nblk; p.max_voxels = ctx->cfg.max_voxels;
        hipLaunchKernelGGL(sc1_ballot_b, dim3(S->nblk, 1, g), dim3(256), 0, stream, p);
        hipLaunchKernelGGL(sc1_write_b, dim3(S->nblk, 1, g), dim3(256), 0, stream, p);
        hipLaunchKernelGGL(S->kc == 8 ? sc1_gather<8> : sc1_gather<4>, dim3(pp_div_up(S->cap_pad, 4 * SC1_WAVE_PX), 1, g), dim3(256), 0, stream, p);
    }
    PP_HIP(hipGetLastError());
    ctx->sc1_last_nb = nb;
    return 0;
}

// inspection: i32[1 + cap] = count, then the active pixel indices (entries past the count are unspecified)
int pp_sc1_fetch_list(pp_ctx* ctx, int frame, void* dst, hipStream_t stream)
{
    const Sc1* S = (const Sc1*)ctx->sc1;
    if (!S || frame >= ctx->sc1_last_nb) return pp_fail(ctx, PP_E_STATE, "pp_fetch_frame_tensor: the last pass did not build an active list for this frame");
    PP_HIP(hipMemcpyAsync(dst, S->count + frame, sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    PP_HIP(hipMemcpyAsync((int32_t*)dst + 1, S->list + (size_t)frame * S->cap_pad, (size_t)S->cap * sizeof(int32_t), hipMemcpyDeviceToDevice, stream));
    return 0;
}

const uint64_t* pp_sc1_words(pp_ctx* ctx, int* nblk)
{
    const Sc1* S = (const Sc1*)ctx->sc1;
    if (!S || ctx->sc1_last_nb < 1) return nullptr;
    *nblk = S->nblk;
    return S->words;
}

extern "C" int pp_set_sparse_conv1(pp_ctx* ctx, int on)
{
    if (!ctx) return PP_E_ARG;
    ctx->sparse_conv1 = on && !ctx->sparse_conv1_env_off;
    return 0;
}
