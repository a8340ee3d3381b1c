// Ground-truth database sampling (the `# sample` slot of framework/dataset.py:123 of the reference, in front of noise_per_object),
// batched over nb frames with host CSR offsets like the pp_augment_* entries.  The three primitives are the reference's:
// points_in_rbbox (box_np_ops.py:460-467, the planes of aug_geom.h), box_collision_test (augmentation.py:617-697) and
// remove_points_in_boxes (:214-217).
//   C1  count / extract: one workgroup per box walks its frame's cloud in rounds of MEM_THREADS points; the rank of a member is the
//       members of the earlier rounds + the earlier waves of its round + the earlier lanes of its wave (ballots), so the extracted
//       points keep the cloud's order and no atomic decides anything.
//   S1  select: one workgroup per frame, BEV corners of existing + candidate boxes in LDS, the candidates in order; a candidate
//       is tested by all lanes at once against the existing boxes and the earlier ACCEPTED candidates.
//   P1  paste, three launches: the survivors of each chunk of PP_GT_CHUNK scene points are counted (blk), a frame's size is the sum
//       of its chunks + its accepted objects, and the paste writes the objects (candidate order) and then each chunk's survivors at
//       the prefix of the chunk counts.  A candidate whose database index or point range is out of bounds counts as not accepted
//       and nothing of it is read.
//   D1  draw: cand_idx from the keyed Feistel bijection on [0, n_c), key = Philox(seed, epoch, sample index, PP_GT_STREAM, class).
// Every store is guarded by the bounds of the frame's or object's slot, whatever the device-side offsets hold.
#include <cstring>
#include "pp_common.h"
#include "aug_geom.h"

namespace {

constexpr int GT_GROUP = 64;  // frames per launch (kernel-argument table)
constexpr int DRAW_GROUP = 32;
constexpr int MAXB = PP_AUG_MAX_BOXES;
constexpr int MEM_THREADS = 256;
constexpr int SEL_THREADS = MAXB;
constexpr int PST_THREADS = 256;
constexpr int PST_ROUNDS = PP_GT_CHUNK / PST_THREADS;
static_assert(MEM_THREADS == 256 && PST_THREADS == 256 && SEL_THREADS == 256, "four waves: block_sum and the wave-count tables");
static_assert(PP_GT_CHUNK % PST_THREADS == 0 && MAXB <= PST_THREADS, "k_paste_pts: one thread per candidate for the LDS setup");

struct mem_args {
    int32_t boff[GT_GROUP + 1]; // box rows of the group's frames
    int32_t poff[GT_GROUP + 1]; // point rows likewise
    float extra[3];             // added to (l, w, h)
};

struct paste_args {
    int32_t poff[GT_GROUP + 1]; // scene points
    int32_t coff[GT_GROUP + 1]; // candidates
    int32_t bk0[GT_GROUP + 1];  // chunk counts (blk)
    int32_t ooff[GT_GROUP + 1]; // output rows (paste only)
    int32_t f0, remove;
};

struct db_view {
    const int64_t* off; // i64[n + 1]
    int64_t n, T;       // objects, points
};

// sum over the 256 threads of a block; sm: 4 ints of LDS.  Ends with a barrier, so sm may be reused at once.
__device__ __forceinline__ int block_sum(int v, int* sm)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const int r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return r;
}

// rank of a kept lane among the kept threads of the block (in thread order) and their number; wc: 4 ints of LDS.  One barrier in
// front of the reads; the caller puts one behind before wc is written again.
__device__ __forceinline__ int block_rank(bool keep, int* wc, int& total)
{
    const uint64_t m = __ballot(keep);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) wc[wv] = __popcll(m);
    __syncthreads();
    int base = 0;
    total = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        base += q < wv ? wc[q] : 0;
        total += wc[q];
    }
    return base + __popcll(m & ((1ull << lane) - 1ull));
}

// ---- C1 ----------------------------------------------------------------------------------------------------------------------
template <bool EXTRACT>
__global__ void __launch_bounds__(MEM_THREADS) k_member(mem_args p, const float4* __restrict__ pts, const float* __restrict__ boxes,
                                                        int32_t* __restrict__ counts, const int64_t* __restrict__ obj_off, int64_t T,
                                                        float4* __restrict__ out)
{
    __shared__ int wc[4];
    const int z = blockIdx.y, i = blockIdx.x, t = threadIdx.x;
    const int b0 = p.boff[z], nbx = p.boff[z + 1] - b0;
    if (i >= nbx) return; // uniform over the block
    const int g = b0 + i, p0 = p.poff[z], np_ = p.poff[z + 1] - p0;
    float b[7];
#pragma unroll
    for (int q = 0; q < 7; ++q) b[q] = boxes[(size_t)g * 7 + q];
    const float cx = b[0], cy = b[1], cz = b[2];
    if (!EXTRACT)
        for (int q = 0; q < 3; ++q) b[3 + q] = b[3 + q] + p.extra[q];
    float4 pl[6];
    float bb[6];
    box_face_planes(b, pl, bb);
    int64_t o0 = 0, cap = 0;
    if (EXTRACT) {
        o0 = obj_off[g];
        cap = obj_off[g + 1] - o0;
    }
    int run = 0;
    for (int base = 0; base < np_; base += MEM_THREADS) {
        const int k = base + t;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        bool in = false;
        if (k < np_) {
            q = pts[p0 + k];
            in = inside_box(q.x, q.y, q.z, pl, bb);
        }
        int total;
        const int rank = run + block_rank(in, wc, total);
        if (EXTRACT && in) {
            const int64_t dst = o0 + rank;
            if (rank < cap && dst >= 0 && dst < T) out[dst] = make_float4(q.x - cx, q.y - cy, q.z - cz, q.w);
        }
        run += total;
        __syncthreads();
    }
    if (!EXTRACT && t == 0) counts[g] = run;
}

// ---- S1 ----------------------------------------------------------------------------------------------------------------------
struct sel_args {
    int32_t boff[GT_GROUP + 1];
    int32_t coff[GT_GROUP + 1];
};

__global__ void __launch_bounds__(SEL_THREADS) k_select(sel_args p, const float* __restrict__ boxes, const float* __restrict__ cand,
                                                        uint8_t* __restrict__ accept)
{
    __shared__ float cn[MAXB][8];
    __shared__ float sd[MAXB][4];
    const int z = blockIdx.x, t = threadIdx.x;
    const int b0 = p.boff[z], ne = p.boff[z + 1] - b0, c0 = p.coff[z], nc = p.coff[z + 1] - c0;
    if (t < ne + nc) { // ne + nc <= MAXB (host check)
        const float* bx = t < ne ? boxes + (size_t)(b0 + t) * 7 : cand + (size_t)(c0 + t - ne) * 7;
        bev_corners(bx[0], bx[1], bx[3], bx[4], bx[6], cn[t]);
        standup(cn[t], sd[t]);
    }
    __syncthreads();
    bool live = t < ne; // existing boxes block always, a candidate once it is accepted
    for (int j = 0; j < nc; ++j) {
        const bool hit = live && t < ne + j && collide(cn[ne + j], sd[ne + j], cn[t], sd[t]);
        const bool ok = !__syncthreads_or(hit);
        if (t == ne + j) {
            live = ok;
            accept[c0 + j] = ok ? 1 : 0;
        }
    }
}

// ---- P1 ----------------------------------------------------------------------------------------------------------------------
// accepted, and the database rows of the object are in bounds: its first row and size
__device__ __forceinline__ bool cand_ok(int g, const int32_t* __restrict__ cand_idx, const uint8_t* __restrict__ accept, db_view db,
                                        int64_t& s, int& sz)
{
    s = 0;
    sz = 0;
    if (!accept[g]) return false;
    const int64_t idx = cand_idx[g];
    if (idx < 0 || idx >= db.n) return false;
    const int64_t a = db.off[idx], e = db.off[idx + 1];
    if (a < 0 || e < a || e > db.T || e - a > 0x3FFFFFFF) return false;
    s = a;
    sz = (int)(e - a);
    return true;
}

// WRITE = false: blk[chunk] = survivors of the chunk.  WRITE = true: the survivors behind the frame's objects and the earlier chunks.
template <bool WRITE>
__global__ void __launch_bounds__(PST_THREADS) k_paste_pts(paste_args p, const float4* __restrict__ pts, const float* __restrict__ cand,
                                                           const int32_t* __restrict__ cand_idx, const uint8_t* __restrict__ accept,
                                                           db_view db, int32_t* __restrict__ blk, float4* __restrict__ out)
{
    __shared__ float4 pl[MAXB][6];
    __shared__ float bb[MAXB][6];
    __shared__ int16_t list[MAXB];
    __shared__ int wc[4];
    const int z = blockIdx.y, t = threadIdx.x;
    const int p0 = p.poff[z], np_ = p.poff[z + 1] - p0;
    const int64_t first = (int64_t)blockIdx.x * PP_GT_CHUNK;
    if (first >= np_) return; // uniform over the block
    const int c0 = p.coff[z], nc = p.coff[z + 1] - c0;
    bool v = false;
    int sz = 0;
    if (t < nc) {
        int64_t s;
        v = cand_ok(c0 + t, cand_idx, accept, db, s, sz);
        if (v && p.remove) box_face_planes(cand + (size_t)(c0 + t) * 7, pl[t], bb[t]);
    }
    int nv;
    const int lr = block_rank(v, wc, nv);
    if (v) list[lr] = (int16_t)t;
    __syncthreads();
    int64_t dst0 = 0, lo = 0, hi = 0;
    if (WRITE) {
        const int objs = block_sum(v ? sz : 0, wc);
        int before = 0;
        for (int c = t; c < (int)blockIdx.x; c += PST_THREADS) before += blk[p.bk0[z] + c];
        before = block_sum(before, wc);
        lo = p.ooff[z];
        hi = p.ooff[z + 1];
        dst0 = lo + objs + before;
    }
    int run = 0;
    for (int u = 0; u < PST_ROUNDS; ++u) {
        const int64_t k = first + (int64_t)u * PST_THREADS + t;
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        bool keep = false;
        if (k < np_) {
            q = pts[p0 + k];
            keep = true;
            if (p.remove)
                for (int e = 0; e < nv && keep; ++e) keep = !inside_box(q.x, q.y, q.z, pl[list[e]], bb[list[e]]);
        }
        int total;
        const int rank = run + block_rank(keep, wc, total);
        if (WRITE && keep) {
            const int64_t dst = dst0 + rank;
            if (dst >= lo && dst < hi) out[dst] = q; // unchanged bits
        }
        run += total;
        __syncthreads();
    }
    if (!WRITE && t == 0) blk[p.bk0[z] + blockIdx.x] = run;
}

__global__ void __launch_bounds__(PST_THREADS) k_paste_sum(paste_args p, const int32_t* __restrict__ cand_idx, const uint8_t* __restrict__ accept,
                                                           db_view db, const int32_t* __restrict__ blk, int32_t* __restrict__ out_n)
{
    __shared__ int wc[4];
    const int z = blockIdx.x, t = threadIdx.x;
    const int c0 = p.coff[z], nc = p.coff[z + 1] - c0;
    int v = 0;
    if (t < nc) {
        int64_t s;
        int sz;
        if (cand_ok(c0 + t, cand_idx, accept, db, s, sz)) v = sz;
    }
    for (int c = p.bk0[z] + t; c < p.bk0[z + 1]; c += PST_THREADS) v += blk[c];
    v = block_sum(v, wc);
    if (t == 0) out_n[p.f0 + z] = v;
}

// one workgroup per candidate: the object's points + the box centre, behind the earlier accepted objects of the frame
__global__ void __launch_bounds__(PST_THREADS) k_paste_obj(paste_args p, const float* __restrict__ cand, const int32_t* __restrict__ cand_idx,
                                                           const uint8_t* __restrict__ accept, db_view db, const float4* __restrict__ dbp,
                                                           float4* __restrict__ out)
{
    __shared__ int wc[4];
    const int z = blockIdx.y, j = blockIdx.x, t = threadIdx.x;
    const int c0 = p.coff[z], nc = p.coff[z + 1] - c0;
    if (j >= nc) return;
    int64_t s;
    int sz;
    if (!cand_ok(c0 + j, cand_idx, accept, db, s, sz)) return; // uniform over the block
    int v = 0;
    if (t < j) {
        int64_t s2;
        int sz2;
        if (cand_ok(c0 + t, cand_idx, accept, db, s2, sz2)) v = sz2;
    }
    const int before = block_sum(v, wc);
    const float* bx = cand + (size_t)(c0 + j) * 7;
    const float cx = bx[0], cy = bx[1], cz = bx[2];
    const int64_t lo = p.ooff[z], hi = p.ooff[z + 1];
    for (int i = t; i < sz; i += PST_THREADS) {
        const float4 q = dbp[s + i];
        const int64_t dst = lo + before + i;
        if (dst < hi) out[dst] = make_float4(q.x + cx, q.y + cy, q.z + cz, q.w);
    }
}

// ---- D1 ----------------------------------------------------------------------------------------------------------------------
struct gdraw_args {
    int32_t coff[DRAW_GROUP + 1];
    int32_t k[DRAW_GROUP][PP_MAX_CLASSES];
    int64_t sample[DRAW_GROUP];
    int32_t cls_off[PP_MAX_CLASSES + 1];
    int32_t C;
    uint32_t k0, k1, epoch;
};

__global__ void __launch_bounds__(256) k_gt_draw(gdraw_args a, int32_t* __restrict__ cand_idx)
{
    const int z = blockIdx.x, t = threadIdx.x;
    const uint32_t s_lo = (uint32_t)a.sample[z], s_hi = (uint32_t)((uint64_t)a.sample[z] >> 32), ep = a.epoch << 8;
    int run = a.coff[z];
    for (int c = 0; c < a.C; ++c) {
        const int k = a.k[z][c], n = a.cls_off[c + 1] - a.cls_off[c];
        if (k > 0) {
            const u32x4 key = philox(u32x4{(uint32_t)c, ep | PP_GT_STREAM, s_lo, s_hi}, a.k0, a.k1);
            for (int i = t; i < k; i += 256) cand_idx[run + i] = a.cls_off[c] + (int32_t)feistel_keyed((uint32_t)i, (uint32_t)n, key.x, key.y);
        }
        run += k;
    }
}

// ---- host checks -------------------------------------------------------------------------------------------------------------
bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

int check_off(pp_ctx* ctx, const int32_t* off_h, int nb, int64_t cap_total, const char* what)
{
    if (!off_h) return pp_fail(ctx, PP_E_ARG, what);
    if (off_h[0] != 0) return pp_fail(ctx, PP_E_ARG, "gt sampling: offsets must start at 0");
    for (int f = 0; f < nb; ++f)
        if (off_h[f + 1] < off_h[f]) return pp_fail(ctx, PP_E_ARG, "gt sampling: offsets are not monotone");
    if (off_h[nb] > cap_total) return pp_fail(ctx, PP_E_ARG, "gt sampling: more rows than the call's capacity");
    return 0;
}

int max_rows(const int32_t* off, int g)
{
    int m = 0;
    for (int z = 0; z < g; ++z) m = off[z + 1] - off[z] > m ? off[z + 1] - off[z] : m;
    return m;
}

int member_run(pp_ctx* ctx, bool extract, const float* pts, const int32_t* pt_off_h, const float* boxes, const int32_t* box_off_h, int nb,
               const float* extra_h, int32_t* counts, const int64_t* obj_off, int64_t T, float* out, void* stream_, const char* null_msg)
{
    if (nb < 1) return pp_fail(ctx, PP_E_ARG, "gt sampling: nb must be >= 1");
    if (int rc = check_off(ctx, box_off_h, nb, PP_ASSIGN_MAX_GT, null_msg)) return rc;
    if (int rc = check_off(ctx, pt_off_h, nb, 0x7FFFFFFF, null_msg)) return rc;
    const int G = box_off_h[nb];
    if (G == 0) return 0;
    if (!boxes || (pt_off_h[nb] > 0 && !pts) || (extract ? (!obj_off || (T > 0 && !out) || T < 0) : (!counts || !extra_h)))
        return pp_fail(ctx, PP_E_ARG, null_msg);
    if (misaligned(pts, 16) || misaligned(boxes, 4) || misaligned(counts, 4) || misaligned(obj_off, 8) || misaligned(out, 16))
        return pp_fail(ctx, PP_E_ARG, "gt sampling: misaligned pointer (points and outputs are float4 rows)");
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nb; f0 += GT_GROUP) {
        const int g = nb - f0 < GT_GROUP ? nb - f0 : GT_GROUP;
        mem_args a;
        std::memset(&a, 0, sizeof(a));
        for (int z = 0; z <= g; ++z) {
            a.boff[z] = box_off_h[f0 + z];
            a.poff[z] = pt_off_h[f0 + z];
        }
        if (extra_h)
            for (int q = 0; q < 3; ++q) a.extra[q] = extra_h[q];
        const int mb = max_rows(a.boff, g);
        if (mb == 0) continue;
        if (extract)
            hipLaunchKernelGGL(k_member<true>, dim3(mb, g), dim3(MEM_THREADS), 0, stream, a, (const float4*)pts, boxes, counts, obj_off, T, (float4*)out);
        else
            hipLaunchKernelGGL(k_member<false>, dim3(mb, g), dim3(MEM_THREADS), 0, stream, a, (const float4*)pts, boxes, counts, obj_off, T, (float4*)out);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

// the checks the two paste entries share; fills nothing
int paste_check(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* cand, const int32_t* cand_idx, const uint8_t* accept,
                const int32_t* cand_off_h, int nb, const int64_t* db_off, int64_t n_db, int64_t db_T, const int32_t* blk, const char* null_msg)
{
    if (nb < 1) return pp_fail(ctx, PP_E_ARG, "gt sampling: nb must be >= 1");
    if (int rc = check_off(ctx, pt_off_h, nb, 0x7FFFFFFF, null_msg)) return rc;
    if (int rc = check_off(ctx, cand_off_h, nb, PP_ASSIGN_MAX_GT, null_msg)) return rc;
    for (int f = 0; f < nb; ++f)
        if (cand_off_h[f + 1] - cand_off_h[f] > MAXB) return pp_fail(ctx, PP_E_ARG, "gt sampling: more candidates in a frame than PP_AUG_MAX_BOXES");
    if (n_db < 0 || db_T < 0) return pp_fail(ctx, PP_E_ARG, "gt sampling: negative database size");
    if (pt_off_h[nb] > 0 && (!pts || !blk)) return pp_fail(ctx, PP_E_ARG, null_msg);
    if (cand_off_h[nb] > 0 && (!cand || !cand_idx || !accept || !db_off)) return pp_fail(ctx, PP_E_ARG, null_msg);
    if (misaligned(pts, 16) || misaligned(cand, 4) || misaligned(cand_idx, 4) || misaligned(db_off, 8) || misaligned(blk, 4))
        return pp_fail(ctx, PP_E_ARG, "gt sampling: misaligned pointer (points are float4 rows, db_off is int64)");
    return 0;
}

paste_args paste_group(const int32_t* pt_off_h, const int32_t* cand_off_h, const int32_t* out_off_h, int f0, int g, int bk, int remove)
{
    paste_args a;
    std::memset(&a, 0, sizeof(a));
    a.f0 = f0;
    a.remove = remove;
    a.bk0[0] = bk;
    for (int z = 0; z <= g; ++z) {
        a.poff[z] = pt_off_h[f0 + z];
        a.coff[z] = cand_off_h[f0 + z];
        a.ooff[z] = out_off_h ? out_off_h[f0 + z] : 0;
        if (z) a.bk0[z] = a.bk0[z - 1] + pp_div_up(a.poff[z] - a.poff[z - 1], PP_GT_CHUNK);
    }
    return a;
}

} // namespace

extern "C" int pp_gt_count(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* boxes, const int32_t* box_off_h, int nb,
                           const float* extra_h, int32_t* counts, void* stream)
{
    if (!ctx) return PP_E_ARG;
    return member_run(ctx, false, pts, pt_off_h, boxes, box_off_h, nb, extra_h, counts, nullptr, 0, nullptr, stream, "pp_gt_count: null pointer");
}

extern "C" int pp_gt_extract(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* boxes, const int32_t* box_off_h, int nb,
                             const int64_t* obj_off, int64_t T, float* out, void* stream)
{
    if (!ctx) return PP_E_ARG;
    return member_run(ctx, true, pts, pt_off_h, boxes, box_off_h, nb, nullptr, nullptr, obj_off, T, out, stream, "pp_gt_extract: null pointer");
}

extern "C" int pp_gt_select(pp_ctx* ctx, const float* boxes, const int32_t* box_off_h, const float* cand, const int32_t* cand_off_h, int nb,
                            uint8_t* accept, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (nb < 1) return pp_fail(ctx, PP_E_ARG, "pp_gt_select: nb must be >= 1");
    if (int rc = check_off(ctx, box_off_h, nb, PP_ASSIGN_MAX_GT, "pp_gt_select: null box_off_h")) return rc;
    if (int rc = check_off(ctx, cand_off_h, nb, PP_ASSIGN_MAX_GT, "pp_gt_select: null cand_off_h")) return rc;
    for (int f = 0; f < nb; ++f)
        if ((box_off_h[f + 1] - box_off_h[f]) + (cand_off_h[f + 1] - cand_off_h[f]) > MAXB)
            return pp_fail(ctx, PP_E_ARG, "pp_gt_select: more existing + candidate boxes in a frame than PP_AUG_MAX_BOXES");
    if (cand_off_h[nb] == 0) return 0;
    if (!cand || !accept || (box_off_h[nb] > 0 && !boxes)) return pp_fail(ctx, PP_E_ARG, "pp_gt_select: null pointer");
    if (misaligned(boxes, 4) || misaligned(cand, 4)) return pp_fail(ctx, PP_E_ARG, "pp_gt_select: misaligned pointer");
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nb; f0 += GT_GROUP) {
        const int g = nb - f0 < GT_GROUP ? nb - f0 : GT_GROUP;
        sel_args a;
        std::memset(&a, 0, sizeof(a));
        for (int z = 0; z <= g; ++z) {
            a.boff[z] = box_off_h[f0 + z];
            a.coff[z] = cand_off_h[f0 + z];
        }
        if (a.coff[g] == a.coff[0]) continue;
        hipLaunchKernelGGL(k_select, dim3(g), dim3(SEL_THREADS), 0, stream, a, boxes, cand, accept);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_gt_paste_count(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* cand, const int32_t* cand_idx,
                                 const uint8_t* accept, const int32_t* cand_off_h, int nb, const int64_t* db_off, int64_t n_db, int64_t db_T,
                                 int remove, int32_t* blk, int32_t* out_n, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (int rc = paste_check(ctx, pts, pt_off_h, cand, cand_idx, accept, cand_off_h, nb, db_off, n_db, db_T, blk, "pp_gt_paste_count: null pointer"))
        return rc;
    if (!out_n || misaligned(out_n, 4)) return pp_fail(ctx, PP_E_ARG, "pp_gt_paste_count: null or misaligned out_n");
    hipStream_t stream = (hipStream_t)stream_;
    const db_view db{db_off, n_db, db_T};
    int bk = 0;
    for (int f0 = 0; f0 < nb; f0 += GT_GROUP) {
        const int g = nb - f0 < GT_GROUP ? nb - f0 : GT_GROUP;
        const paste_args a = paste_group(pt_off_h, cand_off_h, nullptr, f0, g, bk, remove != 0);
        bk = a.bk0[g];
        const int maxn = max_rows(a.poff, g);
        if (maxn > 0)
            hipLaunchKernelGGL(k_paste_pts<false>, dim3(pp_div_up(maxn, PP_GT_CHUNK), g), dim3(PST_THREADS), 0, stream, a, (const float4*)pts, cand,
                               cand_idx, accept, db, blk, (float4*)nullptr);
        hipLaunchKernelGGL(k_paste_sum, dim3(g), dim3(PST_THREADS), 0, stream, a, cand_idx, accept, db, (const int32_t*)blk, out_n);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_gt_paste(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* cand, const int32_t* cand_idx,
                           const uint8_t* accept, const int32_t* cand_off_h, int nb, const float* db_points, const int64_t* db_off, int64_t n_db,
                           int64_t db_T, int remove, const int32_t* blk, const int32_t* out_off_h, float* out, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (int rc = paste_check(ctx, pts, pt_off_h, cand, cand_idx, accept, cand_off_h, nb, db_off, n_db, db_T, blk, "pp_gt_paste: null pointer")) return rc;
    if (int rc = check_off(ctx, out_off_h, nb, 0x7FFFFFFF, "pp_gt_paste: null out_off_h")) return rc;
    if (out_off_h[nb] == 0) return 0;
    if (!out || (cand_off_h[nb] > 0 && db_T > 0 && !db_points)) return pp_fail(ctx, PP_E_ARG, "pp_gt_paste: null pointer");
    if (misaligned(out, 16) || misaligned(db_points, 16)) return pp_fail(ctx, PP_E_ARG, "pp_gt_paste: misaligned pointer (float4 rows)");
    hipStream_t stream = (hipStream_t)stream_;
    const db_view db{db_off, n_db, db_T};
    int bk = 0;
    for (int f0 = 0; f0 < nb; f0 += GT_GROUP) {
        const int g = nb - f0 < GT_GROUP ? nb - f0 : GT_GROUP;
        const paste_args a = paste_group(pt_off_h, cand_off_h, out_off_h, f0, g, bk, remove != 0);
        bk = a.bk0[g];
        const int maxc = max_rows(a.coff, g), maxn = max_rows(a.poff, g);
        if (maxc > 0)
            hipLaunchKernelGGL(k_paste_obj, dim3(maxc, g), dim3(PST_THREADS), 0, stream, a, cand, cand_idx, accept, db, (const float4*)db_points,
                               (float4*)out);
        if (maxn > 0)
            hipLaunchKernelGGL(k_paste_pts<true>, dim3(pp_div_up(maxn, PP_GT_CHUNK), g), dim3(PST_THREADS), 0, stream, a, (const float4*)pts, cand,
                               cand_idx, accept, db, (int32_t*)blk, (float4*)out);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_gt_draw(pp_ctx* ctx, uint64_t seed, uint32_t epoch, const int64_t* sample_h, const int32_t* class_off_h, int num_classes,
                          const int32_t* k_h, const int32_t* cand_off_h, int nb, int32_t* cand_idx, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (nb < 1) return pp_fail(ctx, PP_E_ARG, "pp_gt_draw: nb must be >= 1");
    if (epoch >= (1u << 24)) return pp_fail(ctx, PP_E_ARG, "pp_gt_draw: epoch must be < 2^24");
    if (num_classes < 1 || num_classes > PP_MAX_CLASSES) return pp_fail(ctx, PP_E_ARG, "pp_gt_draw: num_classes must be 1 .. PP_MAX_CLASSES");
    if (!sample_h || !k_h) return pp_fail(ctx, PP_E_ARG, "pp_gt_draw: null pointer");
    if (int rc = check_off(ctx, class_off_h, num_classes, 0x7FFFFFFF, "pp_gt_draw: null class_off_h")) return rc;
    if (int rc = check_off(ctx, cand_off_h, nb, PP_ASSIGN_MAX_GT, "pp_gt_draw: null cand_off_h")) return rc;
    for (int f = 0; f < nb; ++f) {
        int sum = 0;
        for (int c = 0; c < num_classes; ++c) {
            const int k = k_h[f * num_classes + c];
            if (k < 0 || k > class_off_h[c + 1] - class_off_h[c]) return pp_fail(ctx, PP_E_ARG, "pp_gt_draw: a count outside 0 .. the class's objects");
            sum += k;
        }
        if (sum != cand_off_h[f + 1] - cand_off_h[f]) return pp_fail(ctx, PP_E_ARG, "pp_gt_draw: cand_off_h does not match the counts");
        if (sum > MAXB) return pp_fail(ctx, PP_E_ARG, "pp_gt_draw: more candidates in a frame than PP_AUG_MAX_BOXES");
    }
    if (cand_off_h[nb] == 0) return 0;
    if (!cand_idx || misaligned(cand_idx, 4)) return pp_fail(ctx, PP_E_ARG, "pp_gt_draw: null or misaligned cand_idx");
    hipStream_t stream = (hipStream_t)stream_;
    for (int f0 = 0; f0 < nb; f0 += DRAW_GROUP) {
        const int g = nb - f0 < DRAW_GROUP ? nb - f0 : DRAW_GROUP;
        gdraw_args a;
        std::memset(&a, 0, sizeof(a));
        a.C = num_classes;
        a.k0 = (uint32_t)seed;
        a.k1 = (uint32_t)(seed >> 32);
        a.epoch = epoch;
        for (int c = 0; c <= num_classes; ++c) a.cls_off[c] = class_off_h[c];
        for (int z = 0; z <= g; ++z) a.coff[z] = cand_off_h[f0 + z];
        for (int z = 0; z < g; ++z) {
            a.sample[z] = sample_h[f0 + z];
            for (int c = 0; c < num_classes; ++c) a.k[z][c] = k_h[(f0 + z) * num_classes + c];
        }
        if (a.coff[g] == a.coff[0]) continue;
        hipLaunchKernelGGL(k_gt_draw, dim3(g), dim3(256), 0, stream, a, cand_idx);
    }
    PP_HIP(hipGetLastError());
    return 0;
}
