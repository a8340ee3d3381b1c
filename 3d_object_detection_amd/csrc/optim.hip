// Device optimizer (pp_hip.h: pp_grad_norm, pp_scale_grads, pp_adam_step): clip_grad_norm_ and Adam / AdamW as multi-tensor kernels.
// The tensor lists travel in kernel arguments, PP_OPT_GROUP tensors per launch; one workgroup of 256 lanes per chunk of PP_OPT_CHUNK
// elements.  A lane owns the element groups [4 l, 4 l + 4) and [1024 + 4 l, 1024 + 4 l + 4) of its chunk and issues the loads of both
// before it computes: 16 B per lane and array where the tensor is 16-byte aligned and the group whole (eight 16-byte loads in flight per
// lane in the Adam pass), element by element otherwise -- the same lane owns the same elements on either path, so the reduction order
// of the norm does not depend on alignment.
#include <cmath>
#include <cstdio>
#include "pp_common.h"

namespace {

constexpr int CH = PP_OPT_CHUNK, G = PP_OPT_GROUP, NT = 256, PER = CH / (NT * 4); // PER groups of four per lane
static_assert(PER * NT * 4 == CH, "a chunk is a whole number of 16-byte groups per lane");

struct opt_ws {
    double* part = nullptr; // [PP_OPT_MAX_CHUNKS]
};

// chunk c0[i] .. c0[i + 1] - 1 of a launch belong to tensor i (c0[cnt] = chunks of the launch)
struct mt_head {
    int64_t n[G];
    int32_t c0[G + 1];
    int32_t cnt;
};
struct mt_norm {
    mt_head h;
    const float* g[G];
    int64_t part0; // index of the launch's first partial
};
struct mt_scale {
    mt_head h;
    float* g[G];
};
struct mt_adam {
    mt_head h;
    float* p[G];
    const float* g[G];
    float* m[G];
    float* v[G];
};
struct adam_hp {
    float step_size, bc2_sqrt, beta1, beta2, omb1, omb2, eps, wd, lr_wd;
    int mode; // 0: no weight decay, 1: L2 (Adam), 2: decoupled (AdamW)
};

// tensor of workgroup `c` (uniform: scalar code)
__device__ __forceinline__ int tensor_of(const mt_head& h, int c)
{
    int lo = 0, hi = h.cnt - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (h.c0[mid] <= c) lo = mid; else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// elements [i, i + 4) of a tensor of n elements (i is a multiple of 4); past the end: zeros.  FAST: the workgroup's chunk is whole and
// every pointer of the tensor 16-byte aligned (decided once per workgroup, so the fast body is straight-line code whose loads all issue
// before the first wait); otherwise vec says whether a whole group may still be moved with one 16-byte access.
template <bool FAST>
__device__ __forceinline__ float4 load4(const float* q, int64_t i, int64_t n, bool vec)
{
    if (FAST || (vec && i + 4 <= n)) return *reinterpret_cast<const float4*>(q + i);
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n) r.x = q[i];
    if (i + 1 < n) r.y = q[i + 1];
    if (i + 2 < n) r.z = q[i + 2];
    if (i + 3 < n) r.w = q[i + 3];
    return r;
}
template <bool FAST>
__device__ __forceinline__ void store4(float* q, int64_t i, int64_t n, bool vec, float4 r)
{
    if (FAST || (vec && i + 4 <= n)) { *reinterpret_cast<float4*>(q + i) = r; return; }
    if (i < n) q[i] = r.x;
    if (i + 1 < n) q[i + 1] = r.y;
    if (i + 2 < n) q[i + 2] = r.z;
    if (i + 3 < n) q[i + 3] = r.w;
}

// ---- gradient norm: one fp64 partial per chunk ----
__global__ __launch_bounds__(NT) void k_norm_partial(const mt_norm a, double* __restrict__ part)
{
    __shared__ double sw[NT / 64];
    const int c = blockIdx.x, ti = tensor_of(a.h, c);
    const float* g = a.g[ti];
    const int64_t n = a.h.n[ti], base = (int64_t)(c - a.h.c0[ti]) * CH;
    const bool vec = al16(g);
    float4 x[PER];
    if (vec && base + CH <= n) {
#pragma unroll
        for (int k = 0; k < PER; k++) x[k] = load4<true>(g, base + (int64_t)k * NT * 4 + threadIdx.x * 4, n, vec);
    } else {
#pragma unroll
        for (int k = 0; k < PER; k++) x[k] = load4<false>(g, base + (int64_t)k * NT * 4 + threadIdx.x * 4, n, vec);
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < PER; k++) { // a product of two fp32 values is exact in fp64
        s += (double)x[k].x * (double)x[k].x;
        s += (double)x[k].y * (double)x[k].y;
        s += (double)x[k].z * (double)x[k].z;
        s += (double)x[k].w * (double)x[k].w;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_down(s, d, 64); // fixed lane order
    if ((threadIdx.x & 63) == 0) sw[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = sw[0];
#pragma unroll
        for (int w = 1; w < NT / 64; w++) t += sw[w]; // fixed wave order
        part[a.part0 + c] = t;
    }
}

// one workgroup: lane l adds the partials [l per, (l + 1) per) in index order, lane 0 the lanes' sums in lane order
__global__ __launch_bounds__(NT) void k_norm_finish(const double* __restrict__ part, int64_t npart, float max_norm, float* __restrict__ out)
{
    __shared__ double sl[NT];
    const int64_t per = (npart + NT - 1) / NT, i0 = per * threadIdx.x, i1 = i0 + per < npart ? i0 + per : npart;
    double s = 0.0;
    for (int64_t i = i0; i < i1; i++) s += part[i];
    sl[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double t = sl[0];
    for (int l = 1; l < NT; l++) t += sl[l];
    if (npart == 0) { out[0] = 0.f; out[1] = 1.f; return; }
    const float norm = (float)sqrt(t); // fp64 square root, one rounding to fp32
    float coef = (1.0f / (norm + 1e-6f)) * max_norm; // torch: max_norm / tensor = tensor.reciprocal() * max_norm
    if (coef > 1.0f) coef = 1.0f;                    // a NaN stays a NaN (fminf would return 1)
    out[0] = norm;
    out[1] = coef;
}

template <bool FAST>
__device__ __forceinline__ void scale_chunk(float* g, int64_t base, int64_t n, bool vec, float cf)
{
    float4 x[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) x[k] = load4<FAST>(g, base + (int64_t)k * NT * 4 + threadIdx.x * 4, n, vec);
#pragma unroll
    for (int k = 0; k < PER; k++) {
        x[k].x *= cf; x[k].y *= cf; x[k].z *= cf; x[k].w *= cf;
        store4<FAST>(g, base + (int64_t)k * NT * 4 + threadIdx.x * 4, n, vec, x[k]);
    }
}

__global__ __launch_bounds__(NT) void k_scale(const mt_scale a, const float* __restrict__ coef)
{
    const float cf = coef[0];
    if (cf == 1.0f) return; // every bit stays
    const int c = blockIdx.x, ti = tensor_of(a.h, c);
    float* g = a.g[ti];
    const int64_t n = a.h.n[ti], base = (int64_t)(c - a.h.c0[ti]) * CH;
    const bool vec = al16(g);
    if (vec && base + CH <= n) scale_chunk<true>(g, base, n, vec, cf);
    else scale_chunk<false>(g, base, n, vec, cf);
}

__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float cf, const adam_hp& h)
{
    g = cf * g;
    if (h.mode == 1) g = fmaf(h.wd, p, g);
    if (h.mode == 2) p = fmaf(-h.lr_wd, p, p);
    m = fmaf(h.beta1, m, h.omb1 * g);
    v = fmaf(h.beta2, v, (h.omb2 * g) * g);
    p = p - h.step_size * m / (sqrtf(v) / h.bc2_sqrt + h.eps);
}

template <bool FAST>
__device__ __forceinline__ void adam_chunk(float* p, const float* g, float* m, float* v, int64_t base, int64_t n, bool vec, float cf,
                                           const adam_hp& h)
{
    float4 xp[PER], xg[PER], xm[PER], xv[PER];
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int64_t i = base + (int64_t)k * NT * 4 + threadIdx.x * 4;
        xp[k] = load4<FAST>(p, i, n, vec);
        xg[k] = load4<FAST>(g, i, n, vec);
        xm[k] = load4<FAST>(m, i, n, vec);
        xv[k] = load4<FAST>(v, i, n, vec);
    }
#pragma unroll
    for (int k = 0; k < PER; k++) {
        const int64_t i = base + (int64_t)k * NT * 4 + threadIdx.x * 4;
        adam1(xp[k].x, xg[k].x, xm[k].x, xv[k].x, cf, h);
        adam1(xp[k].y, xg[k].y, xm[k].y, xv[k].y, cf, h);
        adam1(xp[k].z, xg[k].z, xm[k].z, xv[k].z, cf, h);
        adam1(xp[k].w, xg[k].w, xm[k].w, xv[k].w, cf, h);
        store4<FAST>(p, i, n, vec, xp[k]);
        store4<FAST>(m, i, n, vec, xm[k]);
        store4<FAST>(v, i, n, vec, xv[k]);
    }
}

__global__ __launch_bounds__(NT) void k_adam(const mt_adam a, const adam_hp h, const float* __restrict__ coef)
{
    const float cf = coef ? coef[0] : 1.0f;
    const int c = blockIdx.x, ti = tensor_of(a.h, c);
    float* p = a.p[ti];
    const float* g = a.g[ti];
    float* m = a.m[ti];
    float* v = a.v[ti];
    const int64_t n = a.h.n[ti], base = (int64_t)(c - a.h.c0[ti]) * CH;
    const bool vec = al16(p) && al16(g) && al16(m) && al16(v);
    if (vec && base + CH <= n) adam_chunk<true>(p, g, m, v, base, n, vec, cf, h);
    else adam_chunk<false>(p, g, m, v, base, n, vec, cf, h);
}

int ws_get(pp_ctx* ctx, opt_ws** out)
{
    if (!ctx->optim) {
        opt_ws* w = new opt_ws();
        ctx->optim = w;
        PP_HIP(hipMalloc((void**)&w->part, sizeof(double) * PP_OPT_MAX_CHUNKS));
    }
    *out = (opt_ws*)ctx->optim;
    if (!(*out)->part) return pp_fail(ctx, PP_E_STATE, "optimizer: the workspace could not be allocated");
    return 0;
}

inline bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }
inline int64_t chunks_of(int64_t n) { return (n + CH - 1) / CH; }
constexpr int64_t MAX_LEN = (int64_t)1 << 40;         // elements per tensor
constexpr int64_t MAX_LAUNCH_CHUNKS = (int64_t)1 << 30; // workgroups per launch

// Walks the list in order and calls launch(first, h) for every group of at most G tensors with work (skip(i): leave tensor i out).
template <class Skip, class Launch>
int for_groups(const int64_t* lens, int count, Skip skip, Launch launch)
{
    mt_head h;
    int idx[G];
    int i = 0;
    while (i < count) {
        h.cnt = 0;
        h.c0[0] = 0;
        while (i < count && h.cnt < G) {
            if (lens[i] == 0 || skip(i)) { i++; continue; }
            const int64_t nc = chunks_of(lens[i]);
            if (h.cnt > 0 && h.c0[h.cnt] + nc > MAX_LAUNCH_CHUNKS) break;
            h.n[h.cnt] = lens[i];
            idx[h.cnt] = i++;
            h.c0[h.cnt + 1] = (int32_t)(h.c0[h.cnt] + nc);
            h.cnt++;
        }
        if (h.cnt == 0) break;
        for (int k = h.cnt; k < G; k++) { h.n[k] = 0; h.c0[k + 1] = h.c0[h.cnt]; }
        if (int rc = launch(idx, h)) return rc;
    }
    return 0;
}

// the checks the three entry points share; *total = chunks of the tensors with work
int check_list(pp_ctx* ctx, const char* who, const void* const* a, const int64_t* lens, int count, bool null_ok, int64_t* total)
{
    char buf[160];
    for (int i = 0; i < count; i++) {
        const char* bad = nullptr;
        if (lens[i] < 0) bad = "a negative length";
        else if (lens[i] >= MAX_LEN) bad = "a tensor of 2^40 elements or more";
        else if (lens[i] > 0 && !a[i] && !null_ok) bad = "a null pointer";
        else if (!al4(a[i])) bad = "a pointer that is not 4-byte aligned";
        if (bad) {
            snprintf(buf, sizeof(buf), "%s: %s (tensor %d)", who, bad, i);
            return pp_fail(ctx, PP_E_ARG, buf);
        }
        if (total && lens[i] > 0 && (a[i] || !null_ok)) *total += chunks_of(lens[i]);
    }
    return 0;
}

} // namespace

void pp_optim_destroy(pp_ctx* ctx)
{
    opt_ws* w = (opt_ws*)ctx->optim;
    if (!w) return;
    if (w->part) (void)hipFree(w->part);
    delete w;
    ctx->optim = nullptr;
}

extern "C" int pp_grad_norm(pp_ctx* ctx, const float* const* grads, const int64_t* lens, int count, float max_norm, float* out, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (count < 0 || (count > 0 && (!grads || !lens)) || !out || !al4(out)) return pp_fail(ctx, PP_E_ARG, "pp_grad_norm: bad argument");
    int64_t total = 0;
    if (int rc = check_list(ctx, "pp_grad_norm", (const void* const*)grads, lens, count, false, &total)) return rc;
    if (total > PP_OPT_MAX_CHUNKS) return pp_fail(ctx, PP_E_ARG, "pp_grad_norm: more than PP_OPT_MAX_CHUNKS chunks in all");
    opt_ws* ws = nullptr;
    if (int rc = ws_get(ctx, &ws)) return rc;
    int64_t done = 0;
    int rc = for_groups(lens, count, [](int) { return false; }, [&](const int* idx, const mt_head& h) {
        mt_norm a;
        a.h = h;
        for (int k = 0; k < G; k++) a.g[k] = k < h.cnt ? grads[idx[k]] : nullptr;
        a.part0 = done;
        k_norm_partial<<<dim3(h.c0[h.cnt]), dim3(NT), 0, stream>>>(a, ws->part);
        PP_HIP(hipGetLastError());
        done += h.c0[h.cnt];
        return 0;
    });
    if (rc) return rc;
    k_norm_finish<<<dim3(1), dim3(NT), 0, stream>>>(ws->part, done, max_norm, out);
    PP_HIP(hipGetLastError());
    return 0;
}

extern "C" int pp_scale_grads(pp_ctx* ctx, float* const* grads, const int64_t* lens, int count, const float* coef, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (count < 0 || (count > 0 && (!grads || !lens)) || !coef || !al4(coef)) return pp_fail(ctx, PP_E_ARG, "pp_scale_grads: bad argument");
    if (int rc = check_list(ctx, "pp_scale_grads", (const void* const*)grads, lens, count, false, nullptr)) return rc;
    return for_groups(lens, count, [](int) { return false; }, [&](const int* idx, const mt_head& h) {
        mt_scale a;
        a.h = h;
        for (int k = 0; k < G; k++) a.g[k] = k < h.cnt ? grads[idx[k]] : nullptr;
        k_scale<<<dim3(h.c0[h.cnt]), dim3(NT), 0, stream>>>(a, coef);
        PP_HIP(hipGetLastError());
        return 0;
    });
}

extern "C" int pp_adam_step(pp_ctx* ctx, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* lens,
                            int count, int64_t t, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled,
                            const float* coef, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (count < 0 || (count > 0 && (!p || !g || !m || !v || !lens)) || !al4(coef)) return pp_fail(ctx, PP_E_ARG, "pp_adam_step: bad argument");
    if (t < 1) return pp_fail(ctx, PP_E_ARG, "pp_adam_step: the step number must be at least 1");
    if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return pp_fail(ctx, PP_E_ARG, "pp_adam_step: beta must be in [0, 1)");
    if (!(lr >= 0.0) || !(eps >= 0.0) || !(weight_decay >= 0.0)) return pp_fail(ctx, PP_E_ARG, "pp_adam_step: lr, eps and weight_decay must not be negative");
    if (int rc = check_list(ctx, "pp_adam_step (g)", (const void* const*)g, lens, count, true, nullptr)) return rc;
    for (int i = 0; i < count; i++) {
        if (!g[i]) continue; // skipped entirely
        if (lens[i] > 0 && (!p[i] || !m[i] || !v[i])) return pp_fail(ctx, PP_E_ARG, "pp_adam_step: a null pointer");
        if (!al4(p[i]) || !al4(m[i]) || !al4(v[i])) return pp_fail(ctx, PP_E_ARG, "pp_adam_step: a pointer that is not 4-byte aligned");
    }
    adam_hp h;
    h.step_size = (float)(lr / (1.0 - std::pow(beta1, (double)t)));
    h.bc2_sqrt = (float)std::sqrt(1.0 - std::pow(beta2, (double)t));
    h.beta1 = (float)beta1;
    h.beta2 = (float)beta2;
    h.omb1 = (float)(1.0 - beta1);
    h.omb2 = (float)(1.0 - beta2);
    h.eps = (float)eps;
    h.wd = (float)weight_decay;
    h.lr_wd = (float)(lr * weight_decay);
    h.mode = weight_decay != 0.0 ? (decoupled ? 2 : 1) : 0;
    return for_groups(lens, count, [&](int i) { return g[i] == nullptr; }, [&](const int* idx, const mt_head& hd) {
        mt_adam a;
        a.h = hd;
        for (int k = 0; k < G; k++) {
            const bool on = k < hd.cnt;
            a.p[k] = on ? p[idx[k]] : nullptr;
            a.g[k] = on ? g[idx[k]] : nullptr;
            a.m[k] = on ? m[idx[k]] : nullptr;
            a.v[k] = on ? v[idx[k]] : nullptr;
        }
        k_adam<<<dim3(hd.c0[hd.cnt]), dim3(NT), 0, stream>>>(a, h, coef);
        PP_HIP(hipGetLastError());
        return 0;
    });
}
