// Tile skipping for the stride-1 3x3 layers of level 0 (fp32, wino6 main tile; DESIGN section 4 "Constant tiles").
//
// After the sparse first conv the level-0 map is exactly zero outside the active pixel set `a`, so relu(norm(.)) is one constant per
// channel there and wino6_mfma would compute the same 16 x 16 tile over and over.  Winograd F(4x4,3x3) is deterministic: two tiles
// whose 18 x 18 input patch, residual patch, padding mask and (scale, shift) are bit-identical produce bit-identical outputs and
// partial statistics.  One such tile per (frame, layer, border class) is computed, with its statistics weighted by the class's count,
// and copied to the others.
//
//   ts_flags_b   one workgroup per frame, from the sparse conv's ballot words: the tile flags of the three layers (a tile is skippable at
//                layer k iff it holds no B_k block; B_1 = the 4x4-pixel blocks whose 6x6 input window meets `a`, B_k = B_{k-1} dilated by
//                one block), and per layer and border class (4 bits: top, bottom, left, right edge) the skippable count and the first
//                skippable tile.
//   ts_lists_b   one workgroup per (frame, layer): item list {frame * ntile + tile, mult} and fill list {frame, dst, src} in ascending
//                (frame, tile) order.  Integer prefix sums only: the lists are the same on every run.
//   ts_fill      copies the representative's 16 x 16 x C output tile to every destination of the fill list (dwordx4).
#include <cstring>
#include "pp_common.h"

namespace {

constexpr int TS_LAYERS = 3;   // B_1 .. B_3: the stride-1 layers of level 0
constexpr int TS_TILE_BLOCKS_ = 4; // 4 x 4-pixel blocks along a 16-pixel tile edge
constexpr int TS_MAX_LAYERS = TS_TILE_BLOCKS_; // zero padding travels one block per layer: the border classes hold while it stays inside a tile
constexpr int TS_CLS = 16;     // border classes as 4 edge bits (9 of them occur on a map of 2 x 2 tiles or more)
constexpr int TS_FS = 2 + 2 * TS_CLS; // per (frame, layer): item count, fill count, n[16], representative[16]
constexpr int TS_TILE = 16, TS_BLK = 4;
static_assert(TS_LAYERS <= TS_MAX_LAYERS && TS_TILE == TS_BLK * TS_TILE_BLOCKS_, "the rule's precondition on the number of layers");

struct TileSkip {
    uint8_t* flags = nullptr;   // [max_batch][3][ntile] 1 = skippable
    int32_t* fstat = nullptr;   // [max_batch][3][TS_FS]
    int2* items = nullptr;      // [3][max_batch * ntile]
    int4* fills = nullptr;      // [3][max_batch * ntile] (frame, dst tile, src tile, 0)
    int32_t* counts = nullptr;  // [3][2] items, fills
    uint64_t* dbg_words = nullptr; // ballot words of the single-layer hook's bitmaps (allocated on first use)
    int H = 0, W = 0, ntx = 0, nty = 0, ntile = 0, nwords = 0;
    bool shape_ok = false;
    int built_nb = 0;           // frames the lists were built for (0: none)
    int flags_nb = 0;           // frames of the last PASS whose flags the context holds
    bool used = false;          // a listed launch ran since the last pp_run_backbone began
};

struct TsP {
    const uint64_t* words; size_t words_fs;
    uint8_t* flags; int32_t* fstat; int2* items; int4* fills; int32_t* counts;
    int H, W, ntx, nty, ntile, nwords, nb, cap;
};

__device__ __forceinline__ int ts_class(int t, int ntx, int nty)
{
    const int ty = t / ntx, tx = t - ty * ntx;
    return (ty == 0 ? 1 : 0) | (ty == nty - 1 ? 2 : 0) | (tx == 0 ? 4 : 0) | (tx == ntx - 1 ? 8 : 0);
}

// bits [x0, x0 + n) of pixel row y (n <= 64) from the ballot words
__device__ __forceinline__ uint64_t ts_row_bits(const uint64_t* __restrict__ wd, int W, int y, int x0, int n)
{
    const int pix = y * W + x0, w = pix >> 6, s = pix & 63;
    uint64_t v = wd[w] >> s;
    if (s + n > 64) v |= wd[w + 1] << (64 - s); // s > 0 here; the span ends inside the map, so word w + 1 exists
    return n < 64 ? v & ((1ull << n) - 1ull) : v;
}

// A tile holds no B_k block iff no active pixel lies in its pixel rectangle grown by 1 + 4 (k - 1) pixels (clipped to the image): B_1 is
// the 6 x 6 window of a block = the block grown by 1, every dilation grows it by another block.  So the block maps need not be built:
// a thread walks the 34 rows of its tile's k = 3 rectangle once and tests the three nested column spans of each.
__global__ void __launch_bounds__(256) ts_flags_b(const TsP p)
{
    __shared__ int cn[TS_LAYERS][TS_CLS], cr[TS_LAYERS][TS_CLS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const uint64_t* __restrict__ wd = p.words + (size_t)f * p.words_fs;
    if (tid < TS_LAYERS * TS_CLS) { cn[tid / TS_CLS][tid % TS_CLS] = 0; cr[tid / TS_CLS][tid % TS_CLS] = 0x7FFFFFFF; }
    __syncthreads();
    constexpr int G = 1 + TS_BLK * (TS_LAYERS - 1); // growth of the widest rectangle: 9 pixels
    for (int t = tid; t < p.ntile; t += 256) {
        const int ty = t / p.ntx, tx = t - ty * p.ntx;
        const int y0 = max(0, TS_TILE * ty - G), y1 = min(p.H - 1, TS_TILE * ty + TS_TILE - 1 + G);
        const int x0 = max(0, TS_TILE * tx - G), x1 = min(p.W - 1, TS_TILE * tx + TS_TILE - 1 + G);
        uint64_t cm[TS_LAYERS]; // column span of layer k's rectangle, relative to x0
#pragma unroll
        for (int k = 0; k < TS_LAYERS; ++k) {
            const int g = 1 + TS_BLK * k;
            const int a = max(0, TS_TILE * tx - g) - x0, b = min(p.W - 1, TS_TILE * tx + TS_TILE - 1 + g) - x0;
            cm[k] = ((b - a + 1 < 64) ? ((1ull << (b - a + 1)) - 1ull) : ~0ull) << a;
        }
        uint64_t any[TS_LAYERS] = {0ull, 0ull, 0ull};
        for (int y = y0; y <= y1; ++y) {
            const uint64_t bits = ts_row_bits(wd, p.W, y, x0, x1 - x0 + 1);
#pragma unroll
            for (int k = 0; k < TS_LAYERS; ++k) {
                const int g = 1 + TS_BLK * k;
                if (y >= TS_TILE * ty - g && y <= TS_TILE * ty + TS_TILE - 1 + g) any[k] |= bits & cm[k];
            }
        }
        const int c = ts_class(t, p.ntx, p.nty);
#pragma unroll
        for (int k = 0; k < TS_LAYERS; ++k) {
            const uint8_t sk = any[k] ? 0 : 1;
            p.flags[((size_t)f * TS_LAYERS + k) * p.ntile + t] = sk;
            if (sk) { atomicAdd(&cn[k][c], 1); atomicMin(&cr[k][c], t); } // a count and a minimum: the same in any order
        }
    }
    __syncthreads();
    if (tid < TS_LAYERS * TS_CLS) {
        const int k = tid / TS_CLS, c = tid % TS_CLS;
        int32_t* fs = p.fstat + ((size_t)f * TS_LAYERS + k) * TS_FS;
        fs[2 + c] = cn[k][c];
        fs[2 + TS_CLS + c] = cn[k][c] ? cr[k][c] : -1;
    }
    if (tid < TS_LAYERS) {
        int32_t* fs = p.fstat + ((size_t)f * TS_LAYERS + tid) * TS_FS;
        int skip = 0, reps = 0, fills = 0;
        for (int c = 0; c < TS_CLS; ++c) {
            const int n = cn[tid][c];
            skip += n;
            if (n > 0) { ++reps; fills += n - 1; }
        }
        fs[0] = p.ntile - skip + reps;
        fs[1] = fills;
    }
}

// exclusive prefix of v over the 256 threads of the workgroup (sc = 256 ints of LDS); returns the workgroup's total through `total`
__device__ __forceinline__ int ts_scan256(int v, int* sc, int& total)
{
    const int tid = threadIdx.x;
    sc[tid] = v;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int x = tid >= d ? sc[tid - d] : 0;
        __syncthreads();
        sc[tid] += x;
        __syncthreads();
    }
    const int incl = sc[tid];
    total = sc[255];
    __syncthreads();
    return incl - v;
}

__global__ void __launch_bounds__(256) ts_lists_b(const TsP p)
{
    __shared__ int sc[256];
    __shared__ int cn[TS_CLS], cr[TS_CLS];
    const int f = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
    // items and fills of the frames in front of this one
    int pi = 0, pf = 0;
    for (int g = tid; g < f; g += 256) {
        const int32_t* fs = p.fstat + ((size_t)g * TS_LAYERS + k) * TS_FS;
        pi += fs[0];
        pf += fs[1];
    }
    int base_i, base_f;
    (void)ts_scan256(pi, sc, base_i);
    (void)ts_scan256(pf, sc, base_f);
    const int32_t* fs = p.fstat + ((size_t)f * TS_LAYERS + k) * TS_FS;
    if (tid < TS_CLS) { cn[tid] = fs[2 + tid]; cr[tid] = fs[2 + TS_CLS + tid]; }
    __syncthreads();
    const uint8_t* __restrict__ fl = p.flags + ((size_t)f * TS_LAYERS + k) * p.ntile;
    const int per = (p.ntile + 255) / 256;
    const int t0 = tid * per, t1 = min(p.ntile, t0 + per);
    int ni = 0, nf = 0;
    for (int t = t0; t < t1; ++t) {
        const bool skip = fl[t] != 0;
        const bool rep = skip && cr[ts_class(t, p.ntx, p.nty)] == t;
        if (!skip || rep) ++ni; else ++nf;
    }
    int tot_i, tot_f;
    int ri = base_i + ts_scan256(ni, sc, tot_i);
    int rf = base_f + ts_scan256(nf, sc, tot_f);
    int2* __restrict__ items = p.items + (size_t)k * p.cap;
    int4* __restrict__ fills = p.fills + (size_t)k * p.cap;
    for (int t = t0; t < t1; ++t) {
        const bool skip = fl[t] != 0;
        const int c = ts_class(t, p.ntx, p.nty);
        const bool rep = skip && cr[c] == t;
        if (!skip || rep) { if (ri < p.cap) items[ri] = make_int2(f * p.ntile + t, rep ? cn[c] : 1); ++ri; }
        else { if (rf < p.cap) fills[rf] = make_int4(f, t, cr[c], 0); ++rf; }
    }
    if (f == p.nb - 1 && tid == 0) {
        p.counts[2 * k] = base_i + tot_i;
        p.counts[2 * k + 1] = base_f + tot_f;
    }
}

// pixel-activity bitmaps u8[nb][H W] -> ballot words in the sparse first conv's layout (bit i of word j = pixel 64 j + i)
__global__ void __launch_bounds__(256) ts_bitmap_words(const uint8_t* __restrict__ bm, uint64_t* __restrict__ words, int HW, int nwords)
{
    const int f = blockIdx.y, pix = blockIdx.x * 256 + threadIdx.x;
    const bool act = pix < HW && bm[(size_t)f * HW + pix] != 0;
    const uint64_t b = __ballot(act);
    const int w = pix >> 6;
    if ((threadIdx.x & 63) == 0 && w < nwords) words[(size_t)f * nwords + w] = b;
}

__global__ void __launch_bounds__(256) ts_fill(const int4* __restrict__ fills, const int32_t* __restrict__ count, float* __restrict__ out, size_t out_fs,
                                               int C, int H, int W, int ntx, int cap)
{
    const int n = min(count[0], cap);
    const size_t plane = (size_t)H * W;
    // workgroups are dealt round-robin over the 8 XCDs: XCD k copies the k-th contiguous eighth of the list, so that the 64-byte row
    // pieces of tiles that are neighbours in x (neighbours in the list) meet in one L2 and leave it as whole lines (grid a multiple of 8)
    const int per = (n + 7) >> 3, xk = blockIdx.x & 7, nloc = gridDim.x >> 3;
    const int i_end = min(n, (xk + 1) * per);
    for (int i = xk * per + (blockIdx.x >> 3); i < i_end; i += nloc) {
        const int4 e = fills[i];
        const int dy = (e.y / ntx) * TS_TILE, dx = (e.y % ntx) * TS_TILE, sy = (e.z / ntx) * TS_TILE, sx = (e.z % ntx) * TS_TILE;
        float* __restrict__ fo = out + (size_t)e.x * out_fs;
        // a channel's tile = 16 rows of four dwordx4 pieces: 64 pieces
        for (int q = threadIdx.x; q < C * 64; q += 256) {
            const int c = q >> 6, r = (q >> 2) & 15, x4 = (q & 3) * 4;
            const float4 v = *reinterpret_cast<const float4*>(fo + c * plane + (size_t)(sy + r) * W + sx + x4);
            *reinterpret_cast<float4*>(fo + c * plane + (size_t)(dy + r) * W + dx + x4) = v;
        }
    }
}

TileSkip* ts_of(pp_ctx* ctx) { return (TileSkip*)ctx->ts; }

TsP ts_params(const TileSkip* T, const uint64_t* words, size_t words_fs, int nb, int max_batch)
{
    TsP p;
    memset(&p, 0, sizeof(p));
    p.words = words; p.words_fs = words_fs;
    p.flags = T->flags; p.fstat = T->fstat; p.items = T->items; p.fills = T->fills; p.counts = T->counts;
    p.H = T->H; p.W = T->W; p.ntx = T->ntx; p.nty = T->nty; p.ntile = T->ntile; p.nwords = T->nwords;
    p.nb = nb; p.cap = max_batch * T->ntile;
    return p;
}

} // namespace

int pp_ts_create(pp_ctx* ctx)
{
    TileSkip* T = new TileSkip();
    ctx->ts = T;
    T->H = ctx->H; T->W = ctx->W;
    // the rule's preconditions on the map: a whole number of 16 x 16 tiles (no strip launches, every border class a whole tile)
    T->shape_ok = T->H > 0 && T->W > 0 && T->H % TS_TILE == 0 && T->W % TS_TILE == 0;
    if (!T->shape_ok) return 0;
    T->nty = T->H / TS_TILE; T->ntx = T->W / TS_TILE; T->ntile = T->ntx * T->nty;
    T->nwords = pp_div_up((int64_t)T->H * T->W, 256) * 4; // the sparse first conv's words: four per 256-pixel block
    const size_t mb = (size_t)ctx->max_batch, cap = mb * T->ntile;
    PP_HIP(hipMalloc((void**)&T->flags, mb * TS_LAYERS * T->ntile));
    PP_HIP(hipMalloc((void**)&T->fstat, mb * TS_LAYERS * TS_FS * sizeof(int32_t)));
    PP_HIP(hipMalloc((void**)&T->items, TS_LAYERS * cap * sizeof(int2)));
    PP_HIP(hipMalloc((void**)&T->fills, TS_LAYERS * cap * sizeof(int4)));
    PP_HIP(hipMalloc((void**)&T->counts, TS_LAYERS * 2 * sizeof(int32_t)));
    PP_HIP(hipMemset(T->counts, 0, TS_LAYERS * 2 * sizeof(int32_t)));
    return 0;
}

void pp_ts_destroy(pp_ctx* ctx)
{
    TileSkip* T = ts_of(ctx);
    if (!T) return;
    void* ptrs[] = {T->flags, T->fstat, T->items, T->fills, T->counts, T->dbg_words};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    delete T;
    ctx->ts = nullptr;
}

bool pp_ts_usable(pp_ctx* ctx, int level0_layers)
{
    const TileSkip* T = ts_of(ctx);
    return ctx->tile_skip && T && T->shape_ok && level0_layers >= 1 && level0_layers <= TS_LAYERS;
}

void pp_ts_begin_pass(pp_ctx* ctx)
{
    TileSkip* T = ts_of(ctx);
    if (T) { T->built_nb = 0; T->flags_nb = 0; T->used = false; }
}

// lists of the three layers for nb frames from ballot words (words == nullptr: the sparse first conv's of this pass)
int pp_ts_build(pp_ctx* ctx, int nb, const uint64_t* words, hipStream_t stream)
{
    TileSkip* T = ts_of(ctx);
    T->built_nb = 0;
    size_t words_fs = (size_t)T->nwords;
    if (!words) {
        int nblk = 0;
        words = pp_sc1_words(ctx, &nblk);
        if (!words || nblk * 4 != T->nwords) return pp_fail(ctx, PP_E_STATE, "tile skip: the sparse first conv's ballot words do not match the map");
    }
    const TsP p = ts_params(T, words, words_fs, nb, ctx->max_batch);
    hipLaunchKernelGGL(ts_flags_b, dim3(nb), dim3(256), 0, stream, p);
    hipLaunchKernelGGL(ts_lists_b, dim3(nb, TS_LAYERS), dim3(256), 0, stream, p);
    PP_HIP(hipGetLastError());
    T->built_nb = nb;
    return 0;
}

int pp_ts_build_from_bitmap(pp_ctx* ctx, int nb, const uint8_t* bitmap, hipStream_t stream)
{
    TileSkip* T = ts_of(ctx);
    if (!T->dbg_words) PP_HIP(hipMalloc((void**)&T->dbg_words, (size_t)ctx->max_batch * T->nwords * sizeof(uint64_t)));
    const int HW = T->H * T->W;
    hipLaunchKernelGGL(ts_bitmap_words, dim3(T->nwords / 4, nb), dim3(256), 0, stream, bitmap, T->dbg_words, HW, T->nwords);
    PP_HIP(hipGetLastError());
    return pp_ts_build(ctx, nb, T->dbg_words, stream);
}

void pp_ts_mark_pass(pp_ctx* ctx, int nb) { TileSkip* T = ts_of(ctx); if (T) T->flags_nb = nb; }
// single-layer hook: a call reports its own launch alone; one that builds lists overwrites the last pass's flags
void pp_ts_begin_hook(pp_ctx* ctx, bool builds) { TileSkip* T = ts_of(ctx); if (T) { T->used = false; if (builds) T->flags_nb = 0; } }
void pp_ts_end_hook(pp_ctx* ctx) { TileSkip* T = ts_of(ctx); if (T) T->built_nb = 0; }

// item list of layer ordinal k (1..3) when lists for nb frames are in place
bool pp_ts_list(pp_ctx* ctx, int k, int nb, const int2** items, const int32_t** count)
{
    TileSkip* T = ts_of(ctx);
    if (!T || !T->shape_ok || k < 1 || k > TS_LAYERS || T->built_nb != nb || nb < 1) return false;
    *items = T->items + (size_t)(k - 1) * ctx->max_batch * T->ntile;
    *count = T->counts + 2 * (k - 1);
    return true;
}

int pp_ts_fill(pp_ctx* ctx, int k, int nb, float* out, size_t out_fs, int C, hipStream_t stream)
{
    TileSkip* T = ts_of(ctx);
    const int cap = ctx->max_batch * T->ntile;
    int g = nb * T->ntile;
    if (g > 2048) g = 2048;
    g = (g + 7) & ~7;
    hipLaunchKernelGGL(ts_fill, dim3(g), dim3(256), 0, stream, T->fills + (size_t)(k - 1) * cap, T->counts + 2 * (k - 1) + 1, out, out_fs, C, T->H, T->W,
                       T->ntx, cap);
    PP_HIP(hipGetLastError());
    T->used = true;
    return 0;
}

int pp_ts_dense_items(pp_ctx* ctx, int nb) { const TileSkip* T = ts_of(ctx); return T ? nb * T->ntile : 0; }

// item count of layer ordinal k as last built (synchronous read-back: pp_profile_end)
int pp_ts_read_count(pp_ctx* ctx, int k, int32_t* n)
{
    TileSkip* T = ts_of(ctx);
    PP_HIP(hipMemcpy(n, T->counts + 2 * (k - 1), sizeof(int32_t), hipMemcpyDeviceToHost));
    return 0;
}

// inspection: u8[3][ntile] = a frame's skippable flags at layers 1, 2, 3 (tile = ty * ntx + tx)
int pp_ts_fetch_flags(pp_ctx* ctx, int frame, void* dst, hipStream_t stream)
{
    const TileSkip* T = ts_of(ctx);
    if (!T || !T->shape_ok || frame >= T->flags_nb)
        return pp_fail(ctx, PP_E_STATE, "pp_fetch_frame_tensor: the last pass built no tile flags for this frame");
    PP_HIP(hipMemcpyAsync(dst, T->flags + (size_t)frame * TS_LAYERS * T->ntile, (size_t)TS_LAYERS * T->ntile, hipMemcpyDeviceToDevice, stream));
    return 0;
}

extern "C" int pp_set_tile_skip(pp_ctx* ctx, int on)
{
    if (!ctx) return PP_E_ARG;
    ctx->tile_skip = on && !ctx->tile_skip_env_off;
    return 0;
}

extern "C" int pp_tile_skip_active(pp_ctx* ctx)
{
    const TileSkip* T = ctx ? ts_of(ctx) : nullptr;
    return T && T->used ? 1 : 0;
}
