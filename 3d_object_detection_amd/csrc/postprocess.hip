// Detection post-processing on the device, no host round trips
// (framework/inference.py:26-138 does 4 boolean gathers + topk + 4 D2H + numpy + an NMS round
// trip per class; framework/nms.py:6-150; eval/iou.py:164-473 for the rotated variant).
//
//   Q1 post_filter   per anchor: mask & sigmoid(cls) >= thr -> 64-bit key (score bits | ~anchor)
//                    appended to the class's candidate list + coarse score histogram
//   Q2 post_thresh   per class: histogram suffix scan -> coarse bin holding the K-th best score
//   Q3 post_gather   candidates in bins >= that bin -> short list (K .. K + one bin)
//   Q4 post_topk     per class (one workgroup): exact top-K by bitonic sort of the short list in LDS
//                    (radix-select fallback when a bin is huge), box decode, NMS boxes
//   Q4b post_cand_b  deferred head (pp_infer_batch): post_topk only selects; this kernel computes the box / dir logits of the
//                    selected anchors from the concat buffer (the head's own MFMA arithmetic, 16 candidates per N-tile) and decodes them
//   Q5 nms_mask      64x64 suppression bit tiles, one WAVEFRONT per tile, mask stored TRANSPOSED: the lane owning a column box
//                    builds its own 64-bit word over the tile's row boxes, which are broadcast lane to lane -- no ballot, no
//                    loads in the loop (nms.py:119-150 is a 64-iteration loop per thread)
//   Q6 nms_reduce    greedy sweep, tile-serial (wave-uniform bit tricks inside a tile, vector OR
//                    across tiles), direction flip, range mask, limit_period, compaction
//
// Selection keys make every ordering total: score descending, ties by lower anchor index
// (torch.topk / numpy argsort leave ties unspecified in the reference).
#include <algorithm>
#include <cmath>
#include <cstring>
#include "pp_common.h"

namespace {

constexpr int NBINS = 4096;
constexpr int SHORT_CAP = 4096; // short list capacity per class (K + one coarse bin)
constexpr int MAXK = 4096;      // nms_pre_max upper bound

struct pp_post {
    uint64_t* cand = nullptr;   // [ncls][cand_cap]
    int64_t cand_cap = 0;
    int32_t* counters = nullptr; // [ncls][8]: the CNT_* slots below
    int32_t* hist = nullptr;    // [ncls][NBINS]
    uint64_t* shortl = nullptr; // [ncls][SHORT_CAP]
    uint64_t* sel = nullptr;    // [ncls][K] sorted keys
    float* boxes = nullptr;     // [ncls][K][7] decoded
    float* nbox = nullptr;      // [ncls][K][6] NMS boxes (aabb: x1,y1,x2,y2 ; rotated: cx,cy,dx,dy,r)
    int32_t* dirl = nullptr;    // [ncls][K]
    uint64_t* nmask = nullptr;  // [ncls][K][K/64]
    int K = 0, cb = 0, bin_shift = 14;
    uint32_t thr_bits = 0;
};

// slots of a class's counters[8] (the rest is padding)
enum { CNT_CAND = 0 /* candidates appended */, CNT_SHORT = 1 /* short-list entries */, CNT_THR_BIN = 2 /* coarse bin of the K-th best */, CNT_NSEL = 3 /* selected */ };

// 64-bit selection key: score bits | ~index, so that descending keys are descending scores with ties by lower index
__device__ __forceinline__ uint64_t key_pack(uint32_t score_bits, uint32_t idx) { return ((uint64_t)score_bits << 32) | (uint64_t)(0xFFFFFFFFu - idx); }
__device__ __forceinline__ uint32_t key_index(uint64_t k) { return 0xFFFFFFFFu - (uint32_t)(k & 0xFFFFFFFFull); }
__device__ __forceinline__ uint32_t key_score_bits(uint64_t k) { return (uint32_t)(k >> 32); }

// coarse histogram bin of a score at or above the threshold, clamped
__device__ __forceinline__ int bin_of(uint32_t score_bits, uint32_t thr_bits, int shift)
{
    const int bin = (int)((score_bits - thr_bits) >> shift);
    return bin < NBINS ? bin : NBINS - 1;
}

__device__ __forceinline__ float sigmoid_rn(float x)
{
    // correctly rounded fp32 sigmoid (fp64 inside), same definition as the oracle
    return (float)(1.0 / (1.0 + exp(-(double)x)));
}

// ---------------------------------------------------------------- Q1
constexpr int FILTER_ITEMS = 8; // anchors per thread
__device__ __forceinline__ void post_filter_body(const float* __restrict__ cls, const uint8_t* __restrict__ mask, pp_config cfg,
                                                   float thr, uint32_t thr_bits, int bin_shift, int64_t cand_cap,
                                                   uint64_t* __restrict__ cand, int32_t* __restrict__ counters,
                                                   int32_t* __restrict__ hist)
{
    // * histogram privatised in LDS (scores cluster in a few bins: global atomics on them serialise)
    // * ONE returning global atomic per workgroup for the candidate append (a single counter word
    //   saturates at ~90 returning atomics/us: per-wave appends alone cost > 100 us at 50 % pass rate)
    __shared__ int lh[NBINS];
    __shared__ int wtot[4], wbase[4];
    const int c = blockIdx.y;
    const int begin = cfg.class_begin[c], end = cfg.class_end[c];
    const int base = begin + blockIdx.x * (256 * FILTER_ITEMS);
    if (base >= end) return;
    for (int i = threadIdx.x; i < NBINS; i += 256) lh[i] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t sb[FILTER_ITEMS];
    int pre[FILTER_ITEMS]; // exclusive position inside the wave, -1 = not a candidate
    int wcount = 0;
#pragma unroll
    for (int it = 0; it < FILTER_ITEMS; ++it) {
        const int a = base + it * 256 + threadIdx.x;
        bool pass = false;
        sb[it] = 0;
        if (a < end && mask[a]) {
            const float s = sigmoid_rn(cls[a]);
            pass = s >= thr;
            sb[it] = __float_as_uint(s);
        }
        const unsigned long long bal = __ballot(pass);
        pre[it] = pass ? wcount + __popcll(bal & ((1ull << lane) - 1ull)) : -1;
        wcount += __popcll(bal);
        if (pass) atomicAdd(&lh[bin_of(sb[it], thr_bits, bin_shift)], 1);
    }
    if (lane == 0) wtot[wave] = wcount;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int tot = wtot[0] + wtot[1] + wtot[2] + wtot[3];
        const int b0 = tot ? atomicAdd(&counters[c * 8 + CNT_CAND], tot) : 0;
        wbase[0] = b0; wbase[1] = b0 + wtot[0]; wbase[2] = wbase[1] + wtot[1]; wbase[3] = wbase[2] + wtot[2];
    }
    __syncthreads();
    const int wb = wbase[wave];
#pragma unroll
    for (int it = 0; it < FILTER_ITEMS; ++it) {
        if (pre[it] < 0) continue;
        const int a = base + it * 256 + threadIdx.x;
        const int slot = wb + pre[it];
        if (slot < cand_cap) cand[(size_t)c * cand_cap + slot] = key_pack(sb[it], (uint32_t)a);
    }
    for (int i = threadIdx.x; i < NBINS; i += 256) {
        const int v = lh[i];
        if (v) atomicAdd(&hist[c * NBINS + i], v);
    }
}

// ---------------------------------------------------------------- Q2
__device__ __forceinline__ void post_thresh_body(const int32_t* __restrict__ hist, int32_t* __restrict__ counters, int K)
{
    __shared__ int part[1024];
    const int c = blockIdx.x, t = threadIdx.x;
    // thread t owns bins [4t, 4t+4) counted from the TOP
    int v[4], s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = hist[c * NBINS + (NBINS - 1 - (4 * t + k))]; s += v[k]; }
    part[t] = s;
    __syncthreads();
    for (int o = 1; o < 1024; o <<= 1) { // inclusive Hillis-Steele scan
        int x = (t >= o) ? part[t - o] : 0;
        __syncthreads();
        part[t] += x;
        __syncthreads();
    }
    int before = part[t] - s; // candidates in strictly higher bins than this thread's first
    const int total = part[1023];
    if (total <= K) {
        if (t == 0) counters[c * 8 + CNT_THR_BIN] = 0; // take everything
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (before < K && before + v[k] >= K) counters[c * 8 + CNT_THR_BIN] = NBINS - 1 - (4 * t + k);
        before += v[k];
    }
}

// ---------------------------------------------------------------- Q3
constexpr int GATHER_ITEMS = 16; // candidates per thread
__device__ __forceinline__ void post_gather_body(const uint64_t* __restrict__ cand, int64_t cand_cap, int32_t* __restrict__ counters,
                                                   uint32_t thr_bits, int bin_shift, uint64_t* __restrict__ shortl)
{
    // A workgroup scans 4096 candidates, collects the few that reach the threshold bin in LDS and appends them with
    // ONE returning global atomic: per-key appends put thousands of returning atomics on one counter word (and the
    // counters of the frames of a batch share an L2 channel, so they did not even run in parallel across frames).
    __shared__ uint64_t lbuf[1024];
    __shared__ int lcnt, gbase;
    const int c = blockIdx.y, tid = threadIdx.x;
    int n = counters[c * 8 + CNT_CAND];
    n = n < cand_cap ? n : (int)cand_cap;
    const int base = blockIdx.x * (256 * GATHER_ITEMS);
    if (base >= n) return; // workgroup-uniform
    const int thr_bin = counters[c * 8 + CNT_THR_BIN];
    if (tid == 0) lcnt = 0;
    __syncthreads();
#pragma unroll 4
    for (int it = 0; it < GATHER_ITEMS; ++it) {
        const int i = base + it * 256 + tid;
        if (i < n) {
            const uint64_t key = cand[(size_t)c * cand_cap + i];
            if (bin_of(key_score_bits(key), thr_bits, bin_shift) >= thr_bin) {
                const int s = atomicAdd(&lcnt, 1);
                if (s < 1024) {
                    lbuf[s] = key;
                } else { // more than a quarter of the block selected: append directly
                    const int slot = atomicAdd(&counters[c * 8 + CNT_SHORT], 1);
                    if (slot < SHORT_CAP) shortl[(size_t)c * SHORT_CAP + slot] = key;
                }
            }
        }
    }
    __syncthreads();
    const int m = lcnt < 1024 ? lcnt : 1024;
    if (tid == 0 && m > 0) gbase = atomicAdd(&counters[c * 8 + CNT_SHORT], m);
    __syncthreads();
    for (int j = tid; j < m; j += 256) {
        const int slot = gbase + j;
        if (slot < SHORT_CAP) shortl[(size_t)c * SHORT_CAP + slot] = lbuf[j];
    }
}

// in-LDS bitonic sort, DESCENDING, n2 = power of two
__device__ void bitonic_desc(uint64_t* a, int n2)
{
    for (int k = 2; k <= n2; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < n2; i += blockDim.x) {
                int ixj = i ^ j;
                if (ixj > i) {
                    uint64_t x = a[i], y = a[ixj];
                    bool up = ((i & k) == 0); // descending in "up" halves
                    if (up ? (x < y) : (x > y)) { a[i] = y; a[ixj] = x; }
                }
            }
        }
    __syncthreads();
}

__device__ __forceinline__ void decode_box(const float* __restrict__ t, const float* __restrict__ an, float* __restrict__ o)
{
    // box_decode, box_np_ops.py:406-423, fp32, no contraction (file is built with -ffp-contract=off)
    const float xa = an[0], ya = an[1], la = an[3], wa = an[4], ha = an[5], ra = an[6];
    const float za = an[2] + ha / 2.f;
    const float diag = sqrtf(la * la + wa * wa);
    const float xg = t[0] * diag + xa, yg = t[1] * diag + ya, zg = t[2] * ha + za;
    const float lg = (float)exp((double)t[3]) * la, wg = (float)exp((double)t[4]) * wa, hg = (float)exp((double)t[5]) * ha;
    o[0] = xg; o[1] = yg; o[2] = zg - hg / 2.f; o[3] = lg; o[4] = wg; o[5] = hg; o[6] = t[6] + ra;
}

__device__ __forceinline__ void standup_box(float cx, float cy, float dx, float dy, float ang, float* __restrict__ o)
{
    // center_to_corner_box2d + corner_to_standup_nd (box_np_ops.py:64-99,717-726)
    const float s = (float)sin((double)ang), c = (float)cos((double)ang);
    const float sx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, sy[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
    float x0 = INFINITY, y0 = INFINITY, x1 = -INFINITY, y1 = -INFINITY;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float px = dx * sx[k], py = dy * sy[k];
        const float x = px * c + py * (-s) + cx;
        const float y = px * s + py * c + cy;
        x0 = fminf(x0, x); x1 = fmaxf(x1, x); y0 = fminf(y0, y); y1 = fmaxf(y1, y);
    }
    o[0] = x0; o[1] = y0; o[2] = x1; o[3] = y1;
}

// decoded candidate ci = c * K + i: its box, its direction label and its NMS box in either mode
__device__ __forceinline__ void store_candidate(const float* b, bool dir1, int rotate, size_t ci, float* __restrict__ boxes,
                                                int32_t* __restrict__ dirl, float* __restrict__ nbox)
{
    float* bo = boxes + ci * 7;
#pragma unroll
    for (int q = 0; q < 7; ++q) bo[q] = b[q];
    dirl[ci] = dir1 ? 1 : 0;
    float* nb = nbox + ci * 6;
    if (rotate) { nb[0] = b[0]; nb[1] = b[1]; nb[2] = b[3]; nb[3] = b[4]; nb[4] = b[6]; }
    else standup_box(b[0], b[1], b[3], b[4], b[6], nb);
}

// ---------------------------------------------------------------- Q4
__device__ __forceinline__ void post_topk_body(pp_config cfg, const uint64_t* __restrict__ cand, int64_t cand_cap,
                                                  const uint64_t* __restrict__ shortl, int32_t* __restrict__ counters, int K,
                                                  const float* __restrict__ box, const float* __restrict__ dir,
                                                  const float* __restrict__ anchors, int rotate, uint64_t* __restrict__ sel,
                                                  float* __restrict__ boxes, float* __restrict__ nbox, int32_t* __restrict__ dirl,
                                                  bool decode)
{
    __shared__ uint64_t keys[SHORT_CAP];
    __shared__ int s_hist[2048];
    __shared__ uint64_t s_prefix;
    __shared__ int s_need, s_cnt;
    const int c = blockIdx.x;
    int ncand = counters[c * 8 + CNT_CAND];
    ncand = ncand < cand_cap ? ncand : (int)cand_cap;
    int nshort = counters[c * 8 + CNT_SHORT];
    int n = 0;
    if (nshort <= SHORT_CAP) {
        n = nshort;
        for (int i = threadIdx.x; i < SHORT_CAP; i += blockDim.x) keys[i] = (i < n) ? shortl[(size_t)c * SHORT_CAP + i] : 0ull;
    } else {
        // Fallback (one coarse bin larger than the short list, e.g. thousands of identical scores):
        // exact K-th largest key by MSB-first radix select over the whole candidate list, 11 bits a pass.
        const uint64_t* src = cand + (size_t)c * cand_cap;
        if (threadIdx.x == 0) { s_prefix = 0ull; s_need = K; }
        __syncthreads();
        for (int shift = 53; shift >= -2; shift -= 11) {
            const int sh = shift < 0 ? 0 : shift;
            const int bits = shift < 0 ? 11 + shift : 11;
            const uint64_t himask = (sh + bits >= 64) ? 0ull : (~0ull << (sh + bits));
            for (int i = threadIdx.x; i < 2048; i += blockDim.x) s_hist[i] = 0;
            __syncthreads();
            const uint64_t pf = s_prefix;
            for (int i = threadIdx.x; i < ncand; i += blockDim.x) {
                uint64_t k = src[i];
                if ((k & himask) == (pf & himask)) atomicAdd(&s_hist[(int)((k >> sh) & ((1u << bits) - 1))], 1);
            }
            __syncthreads();
            if (threadIdx.x == 0) {
                int need = s_need, d = (1 << bits) - 1;
                for (; d > 0; --d) {
                    if (s_hist[d] >= need) break;
                    need -= s_hist[d];
                }
                s_need = need;
                s_prefix = pf | ((uint64_t)d << sh);
            }
            __syncthreads();
        }
        const uint64_t kth = s_prefix; // keys are unique, so exactly K keys are >= kth
        if (threadIdx.x == 0) s_cnt = 0;
        __syncthreads();
        for (int i = threadIdx.x; i < ncand; i += blockDim.x) {
            uint64_t k = src[i];
            if (k >= kth) { int sl = atomicAdd(&s_cnt, 1); if (sl < SHORT_CAP) keys[sl] = k; }
        }
        __syncthreads();
        n = s_cnt < SHORT_CAP ? s_cnt : SHORT_CAP;
        for (int i = n + threadIdx.x; i < SHORT_CAP; i += blockDim.x) keys[i] = 0ull;
    }
    __syncthreads();
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    bitonic_desc(keys, n2);
    const int nsel = n < K ? n : K;
    if (threadIdx.x == 0) counters[c * 8 + CNT_NSEL] = nsel;
    for (int i = threadIdx.x; i < nsel; i += blockDim.x) {
        const uint64_t k = keys[i];
        const uint32_t a = key_index(k);
        sel[(size_t)c * K + i] = k;
        if (!decode) continue; // deferred head: post_cand_b computes and decodes the candidates' logits
        float b[7];
        decode_box(box + (size_t)a * 7, anchors + (size_t)a * 7, b);
        store_candidate(b, dir[(size_t)a * 2 + 1] > dir[(size_t)a * 2], rotate, (size_t)c * K + i, boxes, dirl, nbox);
    }
}

// ---------------------------------------------------------------- Q4b
// Candidate head.  One wave = one N-tile of 16 selected anchors of (frame, class): lane (m, kq) gathers channel 4 S + kq of candidate
// m's pixel from the pre-norm concat buffer, normalises it with the frame's (scale, shift) and feeds v_mfma_f32_16x16x4_f32 over the
// channel quads S = 0 .. K/4 - 1 in ascending order from a zero accumulator, against the SAME A values the full head reads from the
// SAME image -- an MFMA output element depends on its own row and column only, so every logit is bit-identical to the full head's.
// All 96 rows are computed (the flops are free; the cost is the gather), each candidate then picks the 7 + 2 rows of its anchor.
// Padding lanes of a partly filled tile gather the class's last candidate (in bounds) and store nothing.
typedef float pc_f32x4 __attribute__((ext_vector_type(4)));
constexpr int CAND_WAVES = 4;   // N-tiles per workgroup
constexpr int CAND_MAXK = 320;  // input channels of the head
__global__ void __launch_bounds__(64 * CAND_WAVES) post_cand_b(const pp_post_frame* __restrict__ tab, int f0, int K, int HW, const float* __restrict__ anchors,
                                                                  int rotate, pp_head_gather h)
{
    __shared__ float s_aff[2][CAND_MAXK];
    __shared__ float s_out[CAND_WAVES][16][12];
    const int c = blockIdx.y, fz = blockIdx.z;
    const pp_post_frame F = tab[fz];
    const int frame = f0 + fz; // index into the pass's concat buffer / statistics
    const int nsel = F.counters[c * 8 + CNT_NSEL];
    if ((int)blockIdx.x * (16 * CAND_WAVES) >= nsel) return; // workgroup-uniform (covers nsel == 0)
    for (int ch = threadIdx.x; ch < h.K; ch += blockDim.x) { // the frame's (scale, shift): gemm1x1's own prologue
        float sc, sh; // the concat buffer is always pre-norm: statistics (InstanceNorm) or a folded affine (BatchNorm)
        if (h.pre == 1) { // PRE_STATS
            const double* pa = h.pre_acc + (size_t)frame * h.pre_fs;
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int r = 0; r < 8; ++r) { s += pa[((size_t)r * h.K + ch) * 2]; q += pa[((size_t)r * h.K + ch) * 2 + 1]; }
            const double mean = s * h.pre_inv_n;
            double var = q * h.pre_inv_n - mean * mean;
            var = var > 0.0 ? var : 0.0;
            const double rstd = 1.0 / sqrt(var + (double)h.eps);
            sc = (float)rstd;
            sh = (float)(-mean * rstd);
        } else { // PRE_AFFINE
            sc = h.pre_scale[(size_t)frame * h.aff_fs + ch];
            sh = h.pre_shift[(size_t)frame * h.aff_fs + ch];
        }
        s_aff[0][ch] = sc;
        s_aff[1][ch] = sh;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, m = lane & 15, kq = lane >> 4;
    const int base = ((int)blockIdx.x * CAND_WAVES + wave) * 16;
    const int i = base + m;
    const bool valid = i < nsel;
    const uint64_t key = F.sel[(size_t)c * K + (valid ? i : nsel - 1)];
    const uint32_t a = key_index(key);
    const int aloc = (int)(a / (uint32_t)HW), pix = (int)(a - (uint32_t)aloc * (uint32_t)HW);
    if (base < nsel) { // wave-uniform
        const float* bp = h.in + (size_t)frame * h.in_fs + (size_t)kq * HW + pix; // + 4 S HW per step
        int aoff[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) aoff[t] = ((t * 16) / h.bm) * h.K * h.bmp + kq * h.bmp + (t * 16) % h.bm + m; // + 4 S bmp per step
        pc_f32x4 acc[6];
#pragma unroll
        for (int t = 0; t < 6; ++t) acc[t] = (pc_f32x4){0.f, 0.f, 0.f, 0.f};
        const int nsteps = h.K / 4;
        constexpr int U = 8; // K % 32 == 0 (gemm1x1's own condition)
        for (int s0 = 0; s0 < nsteps; s0 += U) {
            float x[U], wv[U][6];
#pragma unroll
            for (int u = 0; u < U; ++u) x[u] = bp[(size_t)(s0 + u) * 4 * HW];
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int t = 0; t < 6; ++t) wv[u][t] = h.w[aoff[t] + (s0 + u) * 4 * h.bmp];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const float bb = fmaxf(fmaf(x[u], s_aff[0][(s0 + u) * 4 + kq], s_aff[1][(s0 + u) * 4 + kq]), 0.f);
#pragma unroll
                for (int t = 0; t < 6; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(wv[u][t], bb, acc[t], 0, 0, 0);
            }
        }
        // lane (m, kq) holds tile rows 16 t + 4 kq + r of candidate m: group g = 4 t + kq of head_tile_row
        if (valid) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int g = 4 * t + kq;
                const float b0 = h.bias_perm[4 * g], b1 = h.bias_perm[4 * g + 1], b2 = h.bias_perm[4 * g + 2], b3 = h.bias_perm[4 * g + 3];
                const float v0 = acc[t][0] + b0, v1 = acc[t][1] + b1, v2 = acc[t][2] + b2, v3 = acc[t][3] + b3;
                float* o = s_out[wave][m];
                if (g == aloc) { o[0] = v0; o[1] = v1; o[2] = v2; o[3] = v3; }            // box k = 0..3
                if (g == 9 + aloc) { o[4] = v0; o[5] = v1; o[6] = v2; }                   // box k = 4..6
                if (g == 18 + (aloc >> 1)) { o[7] = (aloc & 1) ? v2 : v0; o[8] = (aloc & 1) ? v3 : v1; } // dir 0, 1
            }
        }
    }
    __syncthreads();
    if (valid && kq == 0) {
        float t7[7], b[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) t7[q] = s_out[wave][m][q];
        const float d0 = s_out[wave][m][7], d1 = s_out[wave][m][8];
        decode_box(t7, anchors + (size_t)a * 7, b);
        store_candidate(b, d1 > d0, rotate, (size_t)c * K + i, F.boxes, F.dirl, F.nbox);
    }
}

// ---------------------------------------------------------------- IoU device functions
__device__ __forceinline__ float iou_plus1(const float* a, const float* b)
{ // iou_device, nms.py:105-116
    const float left = fmaxf(a[0], b[0]), right = fminf(a[2], b[2]);
    const float top = fmaxf(a[1], b[1]), bottom = fminf(a[3], b[3]);
    const float w = fmaxf(right - left + 1.f, 0.f), h = fmaxf(bottom - top + 1.f, 0.f);
    const float inter = w * h;
    const float sa = (a[2] - a[0] + 1.f) * (a[3] - a[1] + 1.f);
    const float sb = (b[2] - b[0] + 1.f) * (b[3] - b[1] + 1.f);
    return inter / (sa + sb - inter);
}

__device__ __forceinline__ void rb_corners(const float* rb, float* c)
{ // rbbox_to_corners, eval/iou.py:351-374
    const float a_cos = cosf(rb[4]), a_sin = sinf(rb[4]);
    const float xs[4] = {-rb[2] / 2, -rb[2] / 2, rb[2] / 2, rb[2] / 2};
    const float ys[4] = {-rb[3] / 2, rb[3] / 2, rb[3] / 2, -rb[3] / 2};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        c[2 * i] = a_cos * xs[i] + a_sin * ys[i] + rb[0];
        c[2 * i + 1] = -a_sin * xs[i] + a_cos * ys[i] + rb[1];
    }
}
__device__ __forceinline__ bool pt_in_quad(float px, float py, const float* c)
{ // point_in_quadrilateral, eval/iou.py:308-324
    const float ab0 = c[2] - c[0], ab1 = c[3] - c[1], ad0 = c[6] - c[0], ad1 = c[7] - c[1];
    const float ap0 = px - c[0], ap1 = py - c[1];
    const float abab = ab0 * ab0 + ab1 * ab1, abap = ab0 * ap0 + ab1 * ap1;
    const float adad = ad0 * ad0 + ad1 * ad1, adap = ad0 * ap0 + ad1 * ap1;
    return abab >= abap && abap >= 0 && adad >= adap && adap >= 0;
}
__device__ __forceinline__ bool seg_inter(const float* p1, const float* p2, int i, int j, float* out)
{ // line_segment_intersection, eval/iou.py:220-263
    const int i1 = (i + 1) & 3, j1 = (j + 1) & 3;
    const float a0 = p1[2 * i], a1 = p1[2 * i + 1], b0 = p1[2 * i1], b1 = p1[2 * i1 + 1];
    const float c0 = p2[2 * j], c1 = p2[2 * j + 1], d0 = p2[2 * j1], d1 = p2[2 * j1 + 1];
    const float ba0 = b0 - a0, ba1 = b1 - a1, da0 = d0 - a0, ca0 = c0 - a0, da1 = d1 - a1, ca1 = c1 - a1;
    const bool acd = da1 * ca0 > ca1 * da0;
    const bool bcd = (d1 - b1) * (c0 - b0) > (c1 - b1) * (d0 - b0);
    if (acd != bcd) {
        const bool abc = ca1 * ba0 > ba1 * ca0, abd = da1 * ba0 > ba1 * da0;
        if (abc != abd) {
            const float dc0 = d0 - c0, dc1 = d1 - c1;
            const float abba = a0 * b1 - b0 * a1, cddc = c0 * d1 - d0 * c1;
            const float dh = ba1 * dc0 - ba0 * dc1;
            out[0] = (abba * dc0 - ba0 * cddc) / dh;
            out[1] = (abba * dc1 - ba1 * cddc) / dh;
            return true;
        }
    }
    return false;
}
__device__ float rotated_inter_dev(const float* r1, const float* r2)
{ // inter, eval/iou.py:377-391
    float p1[8], p2[8], px[16], py[16], vs[16], t[2];
    int n = 0;
    rb_corners(r1, p1);
    rb_corners(r2, p2);
    for (int i = 0; i < 4; ++i) {
        if (pt_in_quad(p1[2 * i], p1[2 * i + 1], p2)) { px[n] = p1[2 * i]; py[n] = p1[2 * i + 1]; ++n; }
        if (pt_in_quad(p2[2 * i], p2[2 * i + 1], p1)) { px[n] = p2[2 * i]; py[n] = p2[2 * i + 1]; ++n; }
    }
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j)
            if (n < 16 && seg_inter(p1, p2, i, j, t)) { px[n] = t[0]; py[n] = t[1]; ++n; }
    float area = 0.f;
    if (n > 0) { // sort_vertex_in_convex_polygon, :180-217
        float cx = 0.f, cy = 0.f;
        for (int i = 0; i < n; ++i) { cx += px[i]; cy += py[i]; }
        cx /= (float)n; cy /= (float)n;
        for (int i = 0; i < n; ++i) {
            float v0 = px[i] - cx, v1 = py[i] - cy;
            const float d = sqrtf(v0 * v0 + v1 * v1);
            v0 = v0 / d; v1 = v1 / d;
            if (v1 < 0) v0 = -2 - v0;
            vs[i] = v0;
        }
        for (int i = 1; i < n; ++i)
            if (vs[i - 1] > vs[i]) {
                const float tv = vs[i], tx = px[i], ty = py[i];
                int j = i;
                while (j > 0 && vs[j - 1] > tv) { vs[j] = vs[j - 1]; px[j] = px[j - 1]; py[j] = py[j - 1]; --j; }
                vs[j] = tv; px[j] = tx; py[j] = ty;
            }
        for (int i = 0; i < n - 2; ++i) // area, :170-177
            area += fabsf(((px[0] - px[i + 2]) * (py[i + 1] - py[i + 2]) - (py[0] - py[i + 2]) * (px[i + 1] - px[i + 2])) / 2.0f);
    }
    return area;
}
__device__ __forceinline__ float rotated_iou_dev(const float* r1, const float* r2)
{ // devRotateIoU, eval/iou.py:394-399
    const float area = rotated_inter_dev(r1, r2);
    return area / (r1[2] * r1[3] + r2[2] * r2[3] - area);
}

// ---------------------------------------------------------------- Q5
// grid (col tile, row tile, class); 64 threads; lane = COLUMN box, loop over the 64 row boxes.
// TRANSPOSED suppression mask, row-tile major: maskT[rt][col] holds, for column box `col`, the bits r of the row boxes
// (rt*64 + r) that suppress it (IoU > thr and row < col).  One wave per (col tile, row tile); the lane owning a
// column accumulates its own word while the row boxes are broadcast with readlane -- no ballot, no loads in the loop.
// nbox [ncls][K][6], n = the class's CNT_NSEL.
__device__ __forceinline__ void nms_mask_body(const int c, const float* __restrict__ nbox, const int32_t* __restrict__ counters, int K, int cb,
                                               float thr, int rotate, uint64_t* __restrict__ maskT)
{
    constexpr int nstride = 6;
    const int n = counters[c * 8 + CNT_NSEL];
    const int ct = blockIdx.x, rt = blockIdx.y;
    if (ct < rt || rt * 64 >= n || ct * 64 >= n) return;
    const int lane = threadIdx.x;
    const int col = ct * 64 + lane;
    const float* base = nbox + (size_t)c * K * nstride;
    float cbx[5] = {0, 0, 0, 0, 0}, rmine[5] = {0, 0, 0, 0, 0};
    const int nq = rotate ? 5 : 4;
    if (col < n)
        for (int q = 0; q < nq; ++q) cbx[q] = base[(size_t)col * nstride + q];
    const int myrow = rt * 64 + lane;
    if (myrow < n)
        for (int q = 0; q < nq; ++q) rmine[q] = base[(size_t)myrow * nstride + q];
    const int rows = min(64, n - rt * 64);
    uint64_t word = 0ull;
    for (int r = 0; r < rows; ++r) {
        const int row = rt * 64 + r;
        float rbx[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) rbx[q] = __shfl(rmine[q], r);
        if (col < n && col > row) {
            const float iou = rotate ? rotated_iou_dev(rbx, cbx) : iou_plus1(rbx, cbx);
            if (iou > thr) word |= 1ull << r;
        }
    }
    if (col < n) maskT[((size_t)c * cb + rt) * K + col] = word;
}

// Greedy sweep (nms_postprocess, nms.py:85-102) for one class by ONE wavefront on the transposed mask.
// Lane j keeps the suppression word of tile j.  Per tile t: every lane loads its column's words for tile t
// (diagonal) and the later tiles need only one load + one ballot each.  Returns #kept (<= max_keep).
__device__ __forceinline__ int nms_greedy_wave(const uint64_t* __restrict__ maskT, int n_, int K_, int cb, int max_keep_, int* __restrict__ keep)
{
    // one wave, wave-uniform control: as an out-of-line function its arguments arrived in VGPRs and the whole sweep -- loop control,
    // find-first, the 64-bit masks -- ran as divergent VALU code under exec masking; inlined, with the scalars pinned, it runs on the
    // scalar unit (and the caller's address spaces reach its loads and stores)
    const int n = __builtin_amdgcn_readfirstlane(n_), K = __builtin_amdgcn_readfirstlane(K_), max_keep = __builtin_amdgcn_readfirstlane(max_keep_);
    // maskT[t * K + col]: all loads of a step are 512 contiguous bytes.  The words of row tile t + 1 (diagonal + the next AH column
    // tiles) are requested BEFORE the serial sweep of tile t: nothing in them depends on the sweep, and fetched in place they were a
    // global-memory round trip per tile on the one wave that does the work (16 tiles of a 1000-box class: ~40 of the 59 us).
    constexpr int AH = 16;
    const int lane = threadIdx.x & 63;
    uint64_t remv = 0ull; // lane j: columns of tile j already suppressed
    int nk = 0;
    const int tiles = (n + 63) >> 6;
    if (n <= 0) return 0;
    // branch-free: clamped addresses + selects.  (Written as `cond ? row[i] : 0` every load sat in a basic block of its own and the
    // compiler, unable to count what is in flight, waited for vmcnt(0) in front of every use.)
    auto fetch = [&](int t, uint64_t (&w)[AH], uint64_t& diag) __attribute__((always_inline)) {
        const bool live = t < tiles;
        const uint64_t* row = maskT + (size_t)(live ? t : tiles - 1) * K;
        const int i = t * 64 + lane;
        const uint64_t d = row[i < n ? i : n - 1];
        diag = (live && i < n) ? d : 0ull; // rows of tile t suppressing column i
#pragma unroll
        for (int u = 0; u < AH; ++u) {
            const int cidx = (t + 1 + u) * 64 + lane;
            const uint64_t x = row[cidx < n ? cidx : n - 1];
            w[u] = (live && t + 1 + u < tiles && cidx < n) ? x : 0ull;
        }
    };
    uint64_t wc[AH], diag;
    fetch(0, wc, diag);
    for (int t = 0; t < tiles && nk < max_keep; ++t) {
        uint64_t wn[AH], dn;
        fetch(t + 1, wn, dn);
        const uint64_t* row = maskT + (size_t)t * K;
        const uint64_t rtv = __shfl(remv, t);
        const uint64_t rt = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(rtv >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)rtv);
        const int valid = min(64, n - t * 64);
        uint64_t alive = ~rt & (valid == 64 ? ~0ull : ((1ull << valid) - 1ull));
        uint64_t kept = 0ull;
        while (alive && nk < max_keep) { // wave-uniform
            const int b = __ffsll((long long)alive) - 1;
            kept |= 1ull << b;
            if (lane == 0) keep[nk] = t * 64 + b;
            ++nk;
            alive &= ~(1ull << b);
            alive &= ~__ballot((diag >> b) & 1ull); // columns of this tile suppressed by row b
        }
        if (nk >= max_keep) break;
        // fold: column (j*64+lane) is suppressed if any kept row of tile t suppresses it
#pragma unroll
        for (int u = 0; u < AH; ++u) {
            const unsigned long long bal = __ballot((wc[u] & kept) != 0ull);
            if (lane == t + 1 + u) remv |= bal;
        }
        for (int j0 = t + 1 + AH; j0 < tiles; j0 += 8) { // more than AH tiles ahead (nms_pre_max > 1088): fetched in place
            uint64_t w[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int cidx = (j0 + u) * 64 + lane;
                w[u] = (j0 + u < tiles && cidx < n) ? row[cidx] : 0ull;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const unsigned long long bal = __ballot((w[u] & kept) != 0ull);
                if (lane == j0 + u) remv |= bal;
            }
        }
#pragma unroll
        for (int u = 0; u < AH; ++u) wc[u] = wn[u];
        diag = dn;
    }
    return nk;
}

// ---------------------------------------------------------------- Q6
__device__ __forceinline__ void nms_reduce_body(pp_config cfg, const uint64_t* __restrict__ mask, const uint64_t* __restrict__ sel,
                                                  const float* __restrict__ boxes, const int32_t* __restrict__ dirl,
                                                  int32_t* __restrict__ counters, int K, int cb,
                                                  float* __restrict__ det, int32_t* __restrict__ det_count)
{
    __shared__ int s_cnt[PP_MAX_CLASSES];
    __shared__ int s_out[PP_MAX_CLASSES][MAXK > 1024 ? 1024 : MAXK]; // kept rows surviving the range mask (post_max <= 1024)
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int ncls = cfg.num_classes;
    if (wave < ncls) {
        const int c = wave;
        const int n = __builtin_amdgcn_readfirstlane(counters[c * 8 + CNT_NSEL]);
        // the kept list goes to LDS (compacted in place below): a global store per kept box inside the sweep put an unknown number of
        // stores into the vmcnt queue, so every tile's fold waited for vmcnt(0) -- the NEXT tile's words included (one memory round
        // trip per tile on the one wave that does the work)
        int* keep = s_out[c];
        const int nk = nms_greedy_wave(mask + (size_t)c * K * cb, n, K, cb, cfg.nms_post_max, keep); // <= 1024 (pp_create)
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
        __builtin_amdgcn_wave_barrier();
        // direction flip + range mask (quirk: dims vs upper limits, inference.py:107-109), stable compaction
        int no = 0;
        for (int k0 = 0; k0 < nk; k0 += 64) {
            const int k = k0 + lane;
            bool ok = false;
            if (k < nk) {
                const int i = keep[k];
                const float* b = boxes + ((size_t)c * K + i) * 7;
                const bool mn = ((double)b[0] > cfg.center_limit[0]) || ((double)b[1] > cfg.center_limit[1]) || ((double)b[2] > cfg.center_limit[2]);
                const bool mx = ((double)b[3] < cfg.center_limit[3]) || ((double)b[4] < cfg.center_limit[4]) || ((double)b[5] < cfg.center_limit[5]);
                ok = mn && mx;
            }
            const int kv = k < nk ? keep[k] : 0; // every lane reads before any lane writes: positions no + prefix <= k0 + lane
            const unsigned long long bal = __ballot(ok);
            if (ok) s_out[c][no + __popcll(bal & ((1ull << lane) - 1ull))] = kv;
            no += __popcll(bal);
        }
        if (lane == 0) s_cnt[c] = no;
    }
    __syncthreads();
    if (wave < ncls) {
        const int c = wave;
        int off = 0;
        for (int q = 0; q < c; ++q) off += s_cnt[q];
        const int no = s_cnt[c];
        for (int k = lane; k < no; k += 64) {
            const int i = s_out[c][k];
            const float* b = boxes + ((size_t)c * K + i) * 7;
            float r = b[6];
            const bool opp = (r > 0.f) != (dirl[(size_t)c * K + i] != 0);
            if (opp) r = (float)((double)r + 3.141592653589793); // f64 add, f32 store (inference.py:101)
            const float two_pi = 6.283185307179586f;               // limit_period(r, 0.5, 2*pi), fp32
            r = r - floorf(r / two_pi + 0.5f) * two_pi;
            float* d = det + (size_t)(off + k) * 9;
            d[0] = b[0]; d[1] = b[1]; d[2] = b[2]; d[3] = b[3]; d[4] = b[4]; d[5] = b[5]; d[6] = r;
            d[7] = __uint_as_float(key_score_bits(sel[(size_t)c * K + i]));
            d[8] = (float)c;
        }
        if (lane == 0) det_count[1 + c] = no;
        if (c == ncls - 1 && lane == 0) det_count[0] = off + no;
    }
}

int shift_for(uint32_t thr_bits)
{
    uint32_t range = 0x3F800000u - thr_bits;
    int s = 0;
    while ((range >> s) >= (uint32_t)NBINS) ++s;
    return s;
}

// ---- the kernels: a frame's buffers come from `src` (pp_common.h) -- blockIdx.z = frame of a batch (nms_mask: z = frame * ncls +
// class), or the one frame of a stage entry.  The bodies above stay device functions: __restrict__ on their parameters is part of
// what the compiler schedules them by. ----
template <class Src> __global__ void __launch_bounds__(256) post_filter(Src src, pp_config cfg, float thr, uint32_t thr_bits, int bin_shift, int64_t cand_cap)
{
    const pp_post_frame F = src.get();
    post_filter_body(F.cls, F.mask, cfg, thr, thr_bits, bin_shift, cand_cap, F.cand, F.counters, F.hist);
}
template <class Src> __global__ void __launch_bounds__(1024) post_thresh(Src src, int K)
{
    const pp_post_frame F = src.get();
    post_thresh_body(F.hist, F.counters, K);
}
template <class Src> __global__ void __launch_bounds__(256) post_gather(Src src, int64_t cand_cap, uint32_t thr_bits, int bin_shift)
{
    const pp_post_frame F = src.get();
    post_gather_body(F.cand, cand_cap, F.counters, thr_bits, bin_shift, F.shortl);
}
template <class Src> __global__ void __launch_bounds__(1024) post_topk(Src src, pp_config cfg, int64_t cand_cap, int K, const float* __restrict__ anchors,
                                                                       int nms_mode, int decode)
{
    const pp_post_frame F = src.get();
    post_topk_body(cfg, F.cand, cand_cap, F.shortl, F.counters, K, F.box, F.dir, anchors, nms_mode, F.sel, F.boxes, F.nbox, F.dirl, decode != 0);
}
template <class Src> __global__ void __launch_bounds__(64) nms_mask(Src src, int ncls, int K, int cb, float thr, int rotate)
{
    const int fr = blockIdx.z / ncls, c = blockIdx.z - fr * ncls;
    const pp_post_frame F = src.at(fr);
    nms_mask_body(c, F.nbox, F.counters, K, cb, thr, rotate, F.nmask);
}
template <class Src> __global__ void __launch_bounds__(64 * PP_MAX_CLASSES) nms_reduce(Src src, pp_config cfg, int K, int cb, float* __restrict__ det, size_t det_fs,
                                                                                       int32_t* __restrict__ det_count, int cnt_fs)
{
    const pp_post_frame F = src.get();
    nms_reduce_body(cfg, F.nmask, F.sel, F.boxes, F.dirl, F.counters, K, cb, det + blockIdx.z * det_fs,
                    det_count + blockIdx.z * cnt_fs);
}

__global__ void __launch_bounds__(256) post_init_b(const pp_post_frame* __restrict__ tab, int nwords)
{
    int32_t* h = tab[blockIdx.z].hist; // hist | counters are one allocation
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nwords; i += gridDim.x * blockDim.x) h[i] = 0;
}

// stage entry pp_select_candidates: the sorted keys of post_topk as (anchor id, score) rows, -1 / 0 beyond a class's count
__global__ void __launch_bounds__(256) post_export_sel(const uint64_t* __restrict__ sel, const int32_t* __restrict__ counters, int K,
                                                       int32_t* __restrict__ idx, float* __restrict__ score, int32_t* __restrict__ count)
{
    const int c = blockIdx.x;
    const int n = counters[c * 8 + CNT_NSEL];
    for (int i = threadIdx.x; i < K; i += blockDim.x) {
        const uint64_t k = i < n ? sel[(size_t)c * K + i] : 0ull;
        idx[(size_t)c * K + i] = i < n ? (int32_t)key_index(k) : -1;
        score[(size_t)c * K + i] = i < n ? __uint_as_float(key_score_bits(k)) : 0.f;
    }
    if (threadIdx.x == 0) count[c] = n;
}

} // namespace

static int post_create_one(pp_ctx* ctx, pp_slot& S)
{
    pp_post* P = new pp_post();
    S.post = P;
    const pp_config& c = ctx->cfg;
    P->K = c.nms_pre_max;
    P->cb = pp_div_up(P->K, 64);
    int64_t cap = 0;
    for (int i = 0; i < c.num_classes; ++i) {
        if (c.class_end[i] < c.class_begin[i]) return pp_fail(ctx, PP_E_ARG, "bad class range");
        cap = std::max<int64_t>(cap, c.class_end[i] - c.class_begin[i]);
    }
    P->cand_cap = cap > 0 ? cap : 1;
    const int n = c.num_classes;
    PP_HIP(hipMalloc((void**)&P->cand, (size_t)n * P->cand_cap * sizeof(uint64_t)));
    // hist | counters share one allocation: one zero fill per frame
    PP_HIP(hipMalloc((void**)&P->hist, (size_t)n * (NBINS + 8) * sizeof(int32_t)));
    P->counters = P->hist + (size_t)n * NBINS;
    PP_HIP(hipMalloc((void**)&P->shortl, (size_t)n * SHORT_CAP * sizeof(uint64_t)));
    PP_HIP(hipMalloc((void**)&P->sel, (size_t)n * P->K * sizeof(uint64_t)));
    PP_HIP(hipMalloc((void**)&P->boxes, (size_t)n * P->K * 7 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&P->nbox, (size_t)n * P->K * 6 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&P->dirl, (size_t)n * P->K * sizeof(int32_t)));
    PP_HIP(hipMalloc((void**)&P->nmask, (size_t)n * P->K * P->cb * sizeof(uint64_t)));
    float thr = c.score_threshold;
    if (!(thr > 0.f && thr < 1.f)) return pp_fail(ctx, PP_E_ARG, "score_threshold must be in (0,1)");
    memcpy(&P->thr_bits, &thr, 4);
    P->bin_shift = shift_for(P->thr_bits);
    return 0;
}

int pp_post_create(pp_ctx* ctx)
{
    for (pp_slot& S : ctx->slot) {
        int rc = post_create_one(ctx, S);
        if (rc) return rc;
    }
    return 0;
}

void pp_post_destroy(pp_ctx* ctx)
{
    for (pp_slot& S : ctx->slot) {
        pp_post* P = (pp_post*)S.post;
        if (!P) continue;
        void* ptrs[] = {P->cand, P->hist, P->shortl, P->sel, P->boxes, P->nbox, P->dirl, P->nmask};
        for (void* q : ptrs)
            if (q) (void)hipFree(q);
        delete P;
        S.post = nullptr;
    }
}

void pp_post_fill_table(pp_ctx* ctx, int slot, pp_post_frame* f)
{
    const pp_post* P = (const pp_post*)ctx->slot[slot].post;
    PP_SET(f->cand, P->cand); PP_SET(f->shortl, P->shortl); PP_SET(f->sel, P->sel); PP_SET(f->nmask, P->nmask);
    PP_SET(f->counters, P->counters); PP_SET(f->hist, P->hist); PP_SET(f->dirl, P->dirl);
    PP_SET(f->boxes, P->boxes); PP_SET(f->nbox, P->nbox);
}

static int post_class_ranges(pp_ctx* ctx)
{
    for (int i = 0; i < ctx->cfg.num_classes; ++i)
        if (ctx->cfg.class_end[i] > ctx->A) return pp_fail(ctx, PP_E_ARG, "class range exceeds anchor count");
    return 0;
}

// The launch sequence, once for the batched pass and the stage entries (the sizes in slot 0's pp_post are those of every slot).
// Selection, Q1 .. Q4, of g frames whose hist | counters are zero; marks: the stage mark in front of Q4
template <class Src> static int post_select_stages(pp_ctx* ctx, Src src, int g, int nms_mode, int decode, bool marks, hipStream_t stream)
{
    const pp_post* P = (const pp_post*)ctx->slot[0].post;
    const pp_config& c = ctx->cfg;
    const int n = c.num_classes;
    hipLaunchKernelGGL(post_filter<Src>, dim3(pp_div_up(P->cand_cap, 256 * FILTER_ITEMS), n, g), dim3(256), 0, stream, src, c, c.score_threshold,
                       P->thr_bits, P->bin_shift, P->cand_cap);
    hipLaunchKernelGGL(post_thresh<Src>, dim3(n, 1, g), dim3(1024), 0, stream, src, P->K);
    hipLaunchKernelGGL(post_gather<Src>, dim3(pp_div_up(P->cand_cap, 256 * GATHER_ITEMS), n, g), dim3(256), 0, stream, src, P->cand_cap, P->thr_bits, P->bin_shift);
    int rc_;
    if (marks && (rc_ = pp_stage_mark(ctx, stream, PP_ST_POST_TOPK))) return rc_;
    hipLaunchKernelGGL(post_topk<Src>, dim3(n, 1, g), dim3(1024), 0, stream, src, c, P->cand_cap, P->K, ctx->anchors, nms_mode, decode);
    return 0;
}

// NMS, Q5 + Q6, behind its stage mark: frame f of the g writes det + f * det_fs and det_count + f * PP_DET_COUNT_STRIDE
template <class Src> static int post_nms_stages(pp_ctx* ctx, Src src, int g, float* det, int32_t* det_count, int nms_mode, hipStream_t stream)
{
    const pp_post* P = (const pp_post*)ctx->slot[0].post;
    const pp_config& c = ctx->cfg;
    const int n = c.num_classes;
    int rc_;
    if ((rc_ = pp_stage_mark(ctx, stream, PP_ST_POST_NMS))) return rc_;
    hipLaunchKernelGGL(nms_mask<Src>, dim3(P->cb, P->cb, n * g), dim3(64), 0, stream, src, n, P->K, P->cb, c.nms_iou_threshold, nms_mode);
    hipLaunchKernelGGL(nms_reduce<Src>, dim3(1, 1, g), dim3(64 * PP_MAX_CLASSES), 0, stream, src, c, P->K, P->cb, det, (size_t)n * c.nms_post_max * 9,
                       det_count, (int)PP_DET_COUNT_STRIDE);
    PP_HIP(hipGetLastError());
    return 0;
}

// What the stage entries pp_postprocess and pp_select_candidates (`who`) share: the checks, and their frame -- slot 0's scratch
// beside the caller's tensors, by value
typedef pp_frames_one<pp_post_frame> post_one;
static int post_entry_frame(pp_ctx* ctx, const char* who, bool have_ptrs, const float* cls, const float* box, const float* dir, const uint8_t* mask,
                            post_one* src)
{
    if (!have_ptrs) return pp_fail(ctx, PP_E_ARG, (std::string(who) + ": null pointer").c_str());
    if (ctx->A == 0) return pp_fail(ctx, PP_E_STATE, (std::string(who) + ": call pp_set_anchors first").c_str());
    int rc = post_class_ranges(ctx);
    if (rc) return rc;
    pp_post_fill_table(ctx, 0, &src->f);
    PP_SET(src->f.cls, cls); PP_SET(src->f.box, box); PP_SET(src->f.dir, dir); PP_SET(src->f.mask, mask);
    return 0;
}
static size_t post_zero_bytes(pp_ctx* ctx) { return (size_t)ctx->cfg.num_classes * (NBINS + 8) * sizeof(int32_t); } // hist | counters

extern "C" int pp_postprocess(pp_ctx* ctx, const float* cls, const float* box, const float* dir, const uint8_t* mask,
                              float* det, int32_t* det_count, int nms_mode, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    post_one src = {};
    int rc;
    if ((rc = post_entry_frame(ctx, "pp_postprocess", cls && box && dir && mask && det && det_count, cls, box, dir, mask, &src))) return rc;
    if ((rc = pp_stage_mark(ctx, stream, PP_ST_POST))) return rc;
    PP_HIP(hipMemsetAsync(src.f.hist, 0, post_zero_bytes(ctx), stream));
    if ((rc = post_select_stages(ctx, src, 1, nms_mode, 1, true, stream))) return rc;
    if ((rc = post_nms_stages(ctx, src, 1, det, det_count, nms_mode, stream))) return rc;
    return pp_stage_mark(ctx, stream, -1);
}

// Stage entry behind Inference.infer_torch (inference.py:140-189: per class mask gather, sigmoid, score threshold, top-k):
// the selection stages of pp_postprocess alone.  idx i32[ncls][nms_pre_max] anchor ids by descending score (ties: lower
// anchor id), score f32[ncls][nms_pre_max], count i32[ncls].
extern "C" int pp_select_candidates(pp_ctx* ctx, const float* cls, const float* box, const float* dir, const uint8_t* mask,
                                    int32_t* idx, float* score, int32_t* count, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    post_one src = {};
    int rc;
    if ((rc = post_entry_frame(ctx, "pp_select_candidates", cls && box && dir && mask && idx && score && count, cls, box, dir, mask, &src))) return rc;
    PP_HIP(hipMemsetAsync(src.f.hist, 0, post_zero_bytes(ctx), stream));
    if ((rc = post_select_stages(ctx, src, 1, 0, 1, false, stream))) return rc;
    const pp_post* P = (const pp_post*)ctx->slot[0].post;
    hipLaunchKernelGGL(post_export_sel, dim3(ctx->cfg.num_classes), dim3(256), 0, stream, P->sel, P->counters, P->K, idx, score, count);
    PP_HIP(hipGetLastError());
    return 0;
}

// post-processing of frames b0 .. b0+g-1 as one launch per stage (blockIdx.z = frame)
int pp_postprocess_group(pp_ctx* ctx, int b0, int g, float* det, int32_t* det_count, int nms_mode, hipStream_t stream, int defer_nb)
{
    const pp_post* P = (const pp_post*)ctx->slot[0].post;
    const int n = ctx->cfg.num_classes;
    int rc_;
    if ((rc_ = post_class_ranges(ctx))) return rc_;
    const pp_frames_tab<pp_post_frame> src = {ctx->d_post + b0};
    hipLaunchKernelGGL(post_init_b, dim3(8, 1, g), dim3(256), 0, stream, src.tab, n * (NBINS + 8));
    if ((rc_ = post_select_stages(ctx, src, g, nms_mode, defer_nb > 0 ? 0 : 1, true, stream))) return rc_;
    if (defer_nb > 0) { // deferred head: the selected anchors' box / dir logits, decoded (same stage mark)
        pp_head_gather hg;
        if ((rc_ = pp_net_head_gather(ctx, defer_nb, &hg))) return rc_;
        if (hg.K > CAND_MAXK || (hg.K & 31)) return pp_fail(ctx, PP_E_STATE, "candidate head: unexpected channel count");
        hipLaunchKernelGGL(post_cand_b, dim3(pp_div_up(P->K, 16 * CAND_WAVES), n, g), dim3(64 * CAND_WAVES), 0, stream, src.tab, b0, P->K,
                           ctx->H * ctx->W, ctx->anchors, nms_mode, hg);
    }
    return post_nms_stages(ctx, src, g, det + (size_t)b0 * n * ctx->cfg.nms_post_max * 9, det_count + (size_t)b0 * PP_DET_COUNT_STRIDE, nms_mode, stream);
}

// ------------------------------------------------------------------------------------------
// stateless box ops (framework/box_torch_ops.py:18-77, framework/nms.py:6-40, eval/iou.py:438-473)
// ------------------------------------------------------------------------------------------
namespace {

// these entries have no context to report through: a launch error comes back as its negated HIP code
int launch_rc()
{
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : -(int)e;
}

__global__ void __launch_bounds__(256) k_box_decode(const float* __restrict__ enc, const float* __restrict__ anc, float* __restrict__ out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float b[7];
    decode_box(enc + i * 7, anc + i * 7, b);
    for (int q = 0; q < 7; ++q) out[i * 7 + q] = b[q];
}

__global__ void __launch_bounds__(256) k_corners2d(const float* __restrict__ ctr, const float* __restrict__ dims,
                                                   const float* __restrict__ ang, float* __restrict__ out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float dx = dims[2 * i], dy = dims[2 * i + 1], cx = ctr[2 * i], cy = ctr[2 * i + 1];
    const float s = ang ? (float)sin((double)ang[i]) : 0.f, c = ang ? (float)cos((double)ang[i]) : 1.f;
    const float sx[4] = {-0.5f, -0.5f, 0.5f, 0.5f}, sy[4] = {-0.5f, 0.5f, 0.5f, -0.5f};
    for (int k = 0; k < 4; ++k) {
        const float px = dx * sx[k], py = dy * sy[k];
        out[i * 8 + 2 * k] = (ang ? (px * c + py * (-s)) : px) + cx;
        out[i * 8 + 2 * k + 1] = (ang ? (px * s + py * c) : py) + cy;
    }
}

__global__ void __launch_bounds__(256) k_standup2d(const float* __restrict__ cor, float* __restrict__ out, int64_t n)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float* c = cor + i * 8;
    out[i * 4 + 0] = fminf(fminf(c[0], c[2]), fminf(c[4], c[6]));
    out[i * 4 + 1] = fminf(fminf(c[1], c[3]), fminf(c[5], c[7]));
    out[i * 4 + 2] = fmaxf(fmaxf(c[0], c[2]), fmaxf(c[4], c[6]));
    out[i * 4 + 3] = fmaxf(fmaxf(c[1], c[3]), fmaxf(c[5], c[7]));
}

__global__ void __launch_bounds__(256) k_rotated_iou(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ iou, int n, int m)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * m) return;
    const int i = (int)(t / m), j = (int)(t % m);
    float r1[5], r2[5];
    for (int q = 0; q < 5; ++q) { r1[q] = a[i * 5 + q]; r2[q] = b[j * 5 + q]; }
    iou[t] = rotated_iou_dev(r1, r2);
}

// rotate_iou_kernel_eval, eval/iou.py:563-603: out[i,j] = devRotateIoUEval(query j, box i, criterion)
__global__ void __launch_bounds__(256) k_rotated_iou_eval(const float* __restrict__ boxes, const float* __restrict__ qboxes, float* __restrict__ out,
                                                          int n, int k, int criterion)
{
    int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (int64_t)n * k) return;
    const int i = (int)(t / k), j = (int)(t % k);
    float r1[5], r2[5];
    for (int q = 0; q < 5; ++q) { r1[q] = qboxes[j * 5 + q]; r2[q] = boxes[i * 5 + q]; }
    const float area1 = r1[2] * r1[3], area2 = r2[2] * r2[3];
    const float ai = rotated_inter_dev(r1, r2);
    float v;
    if (criterion == -1) v = ai / (area1 + area2 - ai);
    else if (criterion == 0) v = ai / area1;
    else if (criterion == 1) v = ai / area2;
    else v = ai;
    out[t] = v;
}

// sort dets by score (desc, ties by lower index) into nbox[n][6] (+ order[n]), n into the one class's counter block; one workgroup, n <= MAXK
__global__ void __launch_bounds__(1024) k_nms_sort(const float* __restrict__ dets, int n, int stride, float* __restrict__ nbox,
                                                   int32_t* __restrict__ order, int32_t* __restrict__ counters)
{
    __shared__ uint64_t keys[MAXK];
    int n2 = 64;
    while (n2 < n) n2 <<= 1;
    for (int i = threadIdx.x; i < n2; i += blockDim.x) {
        uint64_t k = 0ull;
        if (i < n) {
            uint32_t u = __float_as_uint(dets[(size_t)i * stride + stride - 1]);
            u = (u & 0x80000000u) ? ~u : (u | 0x80000000u); // total order on floats
            k = key_pack(u, (uint32_t)i);
            if (k == 0ull) k = 1ull;
        }
        keys[i] = k;
    }
    bitonic_desc(keys, n2);
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const uint32_t src = key_index(keys[i]);
        order[i] = (int32_t)src;
        for (int q = 0; q < stride - 1; ++q) nbox[(size_t)i * 6 + q] = dets[(size_t)src * stride + q];
    }
    if (threadIdx.x == 0) counters[CNT_NSEL] = n;
}

__global__ void __launch_bounds__(64) k_nms_reduce(const uint64_t* __restrict__ mask, const int32_t* __restrict__ order, int n, int cb,
                                                   int32_t* __restrict__ tmp, int32_t* __restrict__ keep, int32_t* __restrict__ nkeep)
{
    const int nk = nms_greedy_wave(mask, n, n, cb, n, tmp);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    for (int k = threadIdx.x; k < nk; k += 64) keep[k] = order[tmp[k]];
    if (threadIdx.x == 0) *nkeep = nk;
}

} // namespace

extern "C" int pp_box_decode(const float* enc, const float* anchors, float* out, int64_t n, void* stream)
{
    if (n < 0 || (n > 0 && (!enc || !anchors || !out))) return PP_E_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_box_decode, dim3(pp_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, enc, anchors, out, n);
    return launch_rc();
}

extern "C" int pp_corners2d(const float* centers, const float* dims, const float* angles, float* corners, int64_t n, void* stream)
{
    if (n < 0 || (n > 0 && (!centers || !dims || !corners))) return PP_E_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_corners2d, dim3(pp_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, centers, dims, angles, corners, n);
    return launch_rc();
}

extern "C" int pp_standup2d(const float* corners, float* boxes, int64_t n, void* stream)
{
    if (n < 0 || (n > 0 && (!corners || !boxes))) return PP_E_ARG;
    if (n == 0) return 0;
    hipLaunchKernelGGL(k_standup2d, dim3(pp_div_up(n, 256)), dim3(256), 0, (hipStream_t)stream, corners, boxes, n);
    return launch_rc();
}

extern "C" int pp_rotated_iou(const float* a, const float* b, float* iou, int n, int m, void* stream)
{
    if (n < 0 || m < 0 || ((int64_t)n * m > 0 && (!a || !b || !iou))) return PP_E_ARG;
    if ((int64_t)n * m == 0) return 0;
    hipLaunchKernelGGL(k_rotated_iou, dim3(pp_div_up((int64_t)n * m, 256)), dim3(256), 0, (hipStream_t)stream, a, b, iou, n, m);
    return launch_rc();
}

extern "C" int pp_rotated_iou_eval(const float* boxes, const float* qboxes, float* out, int n, int k, int criterion, void* stream)
{
    if (n < 0 || k < 0 || criterion < -1 || criterion > 2) return PP_E_ARG;
    if (n == 0 || k == 0) return 0;
    if (!boxes || !qboxes || !out) return PP_E_ARG;
    hipLaunchKernelGGL(k_rotated_iou_eval, dim3(pp_div_up((int64_t)n * k, 256)), dim3(256), 0, (hipStream_t)stream, boxes, qboxes, out, n, k, criterion);
    return launch_rc();
}

extern "C" int pp_nms(const float* dets, int n, int stride, float thresh, int32_t* keep, int32_t* nkeep, int rotate, void* stream_)
{
    hipStream_t stream = (hipStream_t)stream_;
    if (n < 0 || n > MAXK || !nkeep || (n > 0 && (!dets || !keep))) return PP_E_ARG;
    if ((rotate && stride != 6) || (!rotate && stride != 5)) return PP_E_ARG;
    if (n == 0) {
        hipError_t e0 = hipMemsetAsync(nkeep, 0, sizeof(int32_t), stream);
        return e0 == hipSuccess ? 0 : -(int)e0;
    }
    const int cb = pp_div_up(n, 64);
    // stream-ordered scratch: sorted boxes, order, tmp keep, counters[8], mask -- one class of K = n boxes to nms_mask
    size_t bytes = (size_t)n * 6 * 4 + (size_t)n * 4 * 2 + 64 + (size_t)n * cb * 8 + 256;
    char* ws = nullptr;
    hipError_t e = hipMallocAsync((void**)&ws, bytes, stream);
    if (e != hipSuccess) return -(int)e;
    uint64_t* mask = (uint64_t*)ws;
    float* nbox = (float*)(ws + (size_t)n * cb * 8);
    int32_t* order = (int32_t*)(nbox + (size_t)n * 6);
    int32_t* tmp = order + n;
    post_one src = {};
    PP_SET(src.f.nbox, nbox); PP_SET(src.f.counters, tmp + n); PP_SET(src.f.nmask, mask);
    hipLaunchKernelGGL(k_nms_sort, dim3(1), dim3(1024), 0, stream, dets, n, stride, nbox, order, tmp + n);
    hipLaunchKernelGGL(nms_mask<post_one>, dim3(cb, cb, 1), dim3(64), 0, stream, src, 1, n, cb, thresh, rotate);
    hipLaunchKernelGGL(k_nms_reduce, dim3(1), dim3(64), 0, stream, mask, order, n, cb, tmp, keep, nkeep);
    e = hipGetLastError();
    hipError_t e2 = hipFreeAsync(ws, stream);
    if (e != hipSuccess) return -(int)e;
    return e2 == hipSuccess ? 0 : -(int)e2;
}
