// Training side of the backbone (gfx950): the backward of one pre-activation Resnet unit, InstanceNorm2d(eps 1e-3, no affine) -> ReLU
// -> Conv2d(C -> C, 3 x 3, pad 1, no bias), the unit every Resnet2 module of RPN is made of (pointpillars8_shared.py:418-431).  fp32
// throughout, InstanceNorm backbone only, generic in C = 64 | 128 | 256 and in the map size.
//
// pp_unit_backward materialises a = relu(xhat) and dz once per call, both in the same padded plane layout: a plane is the
// (h + 2) x (w + 2) zero-haloed image (PP = (h + 2) wp elements, wp = w + 2) between two guard bands of G >= wp + 17 zeros, PS elements
// in all (G and PS multiples of 4).  In that layout a 3 x 3 tap is a shift of the flat index by off_t = (ky - 1) wp + (kx - 1), every
// shifted read stays inside the plane, and halo x anything = 0, so both gradient products are plain GEMMs over flat positions P with
// no branch per tap:
//   k_conv3_wt     wT[t][co][ci] = w[co][ci][t]: the dgrad's A operand, contiguous along its rows (train_conv3.h)
//   k_plane_stats  per (frame, c, segment): sum u, sum u^2 in fp64 over one segment of the plane
//   k_unit_pack    per (frame, c, slice): the segments' sums added in index order, mean / rstd, a and dz into the padded planes (halo and
//                  guards rewritten)
//   k_conv3_wgrad  dw[co][(ci, t)] = sum_{frame, P} dz[co][P] a[ci][P + off_t]      M = C, N = 9 C, K = frames x PP, split into ranges
//                  (train_conv3.h's kernel with the stride-1 taps, taps_s1)
//   k_dw_reduce    partials summed in index order (double, rounded once; train_host.h, shared by the three families)
//   k_unit_dgrad   da[ci][P] = sum_{t, co} wT[t][co][ci] dz[co][P - off_t]           M = C, N = PP, K = 9 C, summed in blocks of DA_BLOCK
//                  (each tap by train_conv3.h's conv3_dgrad_tap)
//   k_plane_gstats per (frame, c, segment): sum Gr, sum Gr xhat in fp64 over one segment of da
//   k_unit_norm    per (frame, c, segment): the segments' sums added in index order, du = rstd (Gr - mean(Gr) - xhat mean(Gr xhat)) (+ dskip)
// A plane is cut into plane_segs(elements) segments, a function of the plane size alone (one segment up to 16384 elements, so block 3's
// 100 x 100 planes run as one workgroup each; the 400 x 400 planes of level 0 as ten), so that the streaming passes fill the device at
// level 0's 64 channels and one frame as well.
// The two products run on v_mfma_f32_16x16x4_f32 with operands straight from global memory, as in neck_train.hip.
//
// Determinism: no atomics at all.  Every reduction has a fixed shape: a workgroup's 256 strided fp64 partials are added in index
// order, a plane's segment sums likewise; segments and K ranges of the wgrad depend on the shapes only.  A frame's a, dz, da and du do not
// depend on the batch it rides in; dw depends on nb within fp32 summation error (the K ranges do).
// pp_unit_backward_affine is the same unit with a per-channel affine (a frozen BatchNorm2d) for the norm: k_affine_unit_pack, the two
// products, k_affine_unit_du and k_affine_reduce; pp_unit_backward itself stays the InstanceNorm backbone's.
// pp_unit_backward_bn is that unit behind a train-mode BatchNorm2d (batch statistics pooled over the frames): k_bn_plane_sums behind the
// dgrad of every chunk, then k_bn_coef and one in-place k_bn_unit_du over all frames.
// block_train16.hip holds the 16-bit operand twins of these kernels (pp_unit_backward_mp and the _affine_mp / _bn_mp entries); what both
// share (the check and the plan of a call, the passes behind the dgrad of the two BatchNorm forms) is in block_train.h, what the unit
// shares with the strided stage in train_planes.h (the streaming passes) and train_conv3.h (the two products), what all three training
// families share in train_host.h.  The three entries are thin wrappers over unit_check and unit_run.
#include <cmath>
#include "pp_common.h"
#include "train_planes.h"
#include "block_train.h"

namespace {

// the Winograd weight transforms' G of wino2_transform (F(2x2,3x3), wino2.hip) and wino6_pack (F(4x4,3x3)), the same constant expressions
__constant__ double kG4[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
__constant__ double kG6[6][3] = {{1.0 / 4, 0, 0}, {-1.0 / 6, -1.0 / 6, -1.0 / 6}, {-1.0 / 6, 1.0 / 6, -1.0 / 6},
                                 {1.0 / 24, 1.0 / 12, 1.0 / 6}, {1.0 / 24, -1.0 / 12, 1.0 / 6}, {0, 0, 1}};

// ---- a + dz: grid (C, frames, SP), one slice of LP elements of the padded planes per workgroup (halo and guards rewritten).
// unit_pack_plane is the body of both pack kernels: act(u) is the form's a ---------------------------------------------------------------
template <typename ACT>
__device__ __forceinline__ void unit_pack_plane(const float* __restrict__ up, const float* __restrict__ dp, float* __restrict__ ao,
                                                float* __restrict__ zo, int h, int w, int wp, int G, int PP, int PS, int LP, ACT act)
{
    const int lo = blockIdx.z * LP, hi = lo + LP < PS ? lo + LP : PS;
    padded_walk(lo, hi, h, w, wp, G, PP, [&](int j, const plane_pos& p) {
        float av = 0.f, dv = 0.f;
        if (p.inside) { av = act(up[p.i]); dv = dp[p.i]; }
        ao[j] = av; zo[j] = dv;
    });
}

__global__ void __launch_bounds__(256) k_unit_pack(const float* __restrict__ u, const float* __restrict__ dy, float* __restrict__ ap,
                                                   float* __restrict__ dzp, float* __restrict__ stm, const double* __restrict__ pst, int C, int h,
                                                   int w, int wp, int G, int PP, int PS, int S, int LP)
{
    const int N = h * w;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    float meanf, rstdf;
    plane_mean_rstd(pst, pl, S, N, meanf, rstdf);
    if (threadIdx.x == 0 && blockIdx.z == 0) { stm[pl * 2] = meanf; stm[pl * 2 + 1] = rstdf; }
    unit_pack_plane(u + pl * N, dy + pl * N, ap + pl * PS, dzp + pl * PS, h, w, wp, G, PP, PS, LP, [&](float v) {
        const float xhat = (v - meanf) * rstdf;
        return xhat > 0.f ? xhat : 0.f;
    });
}

// ---- dgrad: a workgroup covers ALL C channels (WM = C / 64 waves down, 4 / WM across), each wave 64 ci x 32 positions, so dz is read
// once per tap.  K = (t, co): the nine taps in order, each tap's blocked sum over co by conv3_dgrad_tap (2304 terms at C = 256).
// Positions past PP read a clamped index and are never stored; only interior positions are stored, into the tight [C][h][w] plane of
// du.
template <int WM>
__global__ void __launch_bounds__(256) k_unit_dgrad(const float* __restrict__ wT, const float* __restrict__ dzp, float* __restrict__ da, int C, int h,
                                                    int w, int wp, int G, int PP, int PS)
{
    constexpr int WN = 4 / WM;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, l16 = lane & 15, q = lane >> 4;
    const int ci0 = 64 * (wave / WN), p0 = blockIdx.x * (32 * WN) + 32 * (wave % WN);
    const float* zf = dzp + (size_t)blockIdx.z * C * PS + G;
    float* daf = da + (size_t)blockIdx.z * C * h * w;
    f32x4 tot[4][2];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) tot[a][b] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int P0 = p0 + l16, P1 = p0 + 16 + l16;
    const int i0 = P0 < PP ? P0 : 0, i1 = P1 < PP ? P1 : 0;
    for (int t = 0; t < 9; ++t) {
        const int off = (t / 3 - 1) * wp + (t % 3 - 1);
        conv3_dgrad_tap(tot, wT + (size_t)t * C * C + ci0 + l16, zf, -off, i0, i1, q, C, C, PS);
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        const int P = p0 + 16 * b + l16;
        if (P >= PP) continue;
        const int y = P / wp, x = P - y * wp;
        if (y < 1 || y > h || x < 1 || x > w) continue;
        float* o = daf + (size_t)(y - 1) * w + x - 1;
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int i = 0; i < 4; ++i) o[(size_t)(ci0 + 16 * a + 4 * q + i) * h * w] = tot[a][b][i];
    }
}

// ---- norm backward, in place over da (= du).  Gr = da [a > 0] with the a of this call; xhat is re-evaluated by the expression
// k_unit_pack used, so it is the xhat whose sign made the mask.  k_plane_gstats: grid (C, frames, S), sum Gr and sum Gr xhat of one
// segment; k_unit_norm: grid (C, frames, S), the same segments rewritten once every sum is in ----------------------------------------
__global__ void __launch_bounds__(256) k_plane_gstats(const float* __restrict__ ap, const float* __restrict__ du, double* __restrict__ pst, int C,
                                                      int w, int wp, int G, int PS, int N, int L, int S)
{
    __shared__ double red[256][2];
    const int tid = threadIdx.x;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float* ai = ap + pl * PS + G + wp + 1; // interior origin
    const float* dp = du + pl * N;
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    double sg = 0.0, sgx = 0.0;
    strided4(lo, hi, [&](int i) { const int y = i / w, x = i - y * w; return float2{ai[y * wp + x], dp[i]}; },
             [&](float2 v) {
                 if (v.x > 0.f) {
                     const double g = (double)v.y;
                     sg += g; sgx += g * (double)v.x;
                 }
             });
    block_sum2(sg, sgx, red);
    if (tid == 0) { pst[(pl * S + blockIdx.z) * 2] = sg; pst[(pl * S + blockIdx.z) * 2 + 1] = sgx; }
}

__global__ void __launch_bounds__(256) k_unit_norm(const float* __restrict__ u, const float* __restrict__ ap, const float* __restrict__ stm,
                                                   const double* __restrict__ pst, const float* __restrict__ dskip, float* __restrict__ du, int C,
                                                   int h, int w, int wp, int G, int PS, int L, int S)
{
    const int tid = threadIdx.x, N = h * w;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float* up = u + pl * N;
    const float* ai = ap + pl * PS + G + wp + 1; // interior origin
    float* dp = du + pl * N;
    const float meanf = stm[pl * 2], rstdf = stm[pl * 2 + 1];
    double sg = 0.0, sgx = 0.0;
    for (int g = 0; g < S; ++g) { sg += pst[(pl * S + g) * 2]; sgx += pst[(pl * S + g) * 2 + 1]; }
    const double inv_n = 1.0 / (double)N;
    const float c1 = (float)(sg * inv_n), c2 = (float)(sgx * inv_n);
    const int lo = blockIdx.z * L, hi = lo + L < N ? lo + L : N;
    for (int i = lo + tid; i < hi; i += 256) {
        const int y = i / w, x = i - y * w;
        const float g = ai[y * wp + x] > 0.f ? dp[i] : 0.f;
        const float xhat = (up[i] - meanf) * rstdf;
        float v = rstdf * ((g - c1) - xhat * c2);
        if (dskip) v = v + dskip[pl * N + i];
        dp[i] = v;
    }
}

// ---- the unit with a per-channel affine in place of the InstanceNorm (pp_unit_backward_affine): a = max(fma(u, scale, shift), 0), the
// forward prologue's expression, so there are no statistics passes.  k_affine_unit_pack: grid (C, frames, SP) as k_unit_pack.
// The passes behind the dgrad (k_affine_unit_du; k_bn_plane_sums, k_bn_unit_du for the batch form) are block_train.h's and
// train_conv3.h's: the 16-bit twin runs them too -------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_affine_unit_pack(const float* __restrict__ u, const float* __restrict__ dy, float* __restrict__ ap,
                                                          float* __restrict__ dzp, const float* __restrict__ scale, const float* __restrict__ shift,
                                                          int C, int h, int w, int wp, int G, int PP, int PS, int LP)
{
    const int N = h * w;
    const size_t pl = (size_t)blockIdx.y * C + blockIdx.x;
    const float sc = scale[blockIdx.x], sh = shift[blockIdx.x];
    unit_pack_plane(u + pl * N, dy + pl * N, ap + pl * PS, dzp + pl * PS, h, w, wp, G, PP, PS, LP, [&](float v) { return affine_relu(v, sc, sh); });
}

// ---- weight update: image element i holds position pmap[i] % T of the transformed weight of (row, cin) = pmap[i] / T.  U = G g G^T is
// evaluated in fp64 in the host packers' own expression order and rounded once; the library is built with -ffp-contract=off on both
// sides, so the image is the one a fresh commit of the same values packs, bit for bit -------------------------------------------------
__global__ void __launch_bounds__(256) k_unit_image(float* __restrict__ dst, const int32_t* __restrict__ pmap, int n, const float* __restrict__ w,
                                                    int T, int nrc)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int m = pmap[i];
    const int rc = m < 0 ? -1 : m / T;
    if (rc < 0 || rc >= nrc) { dst[i] = 0.f; return; }
    const int pos = m - rc * T;
    const float* g = w + (size_t)rc * 9;
    if (T == 9) { dst[i] = g[pos]; return; }
    const int nn = T == 16 ? 4 : 6, a = pos / nn, b = pos - a * nn;
    const double* Ga = T == 16 ? kG4[a] : kG6[a];
    const double* Gb = T == 16 ? kG4[b] : kG6[b];
    const double ga0 = Ga[0], ga1 = Ga[1], ga2 = Ga[2];
    const double t0 = ga0 * g[0] + ga1 * g[3] + ga2 * g[6];
    const double t1 = ga0 * g[1] + ga1 * g[4] + ga2 * g[7];
    const double t2 = ga0 * g[2] + ga1 * g[5] + ga2 * g[8];
    dst[i] = (float)(t0 * Gb[0] + t1 * Gb[1] + t2 * Gb[2]);
}

} // namespace

void pp_block_destroy(pp_ctx* ctx)
{
    block_ws* w = (block_ws*)ctx->blk;
    if (!w) return;
    void* q[] = {w->planes, w->stm, w->pst, w->wT, w->part, w->img16, w->wT16};
    for (void* x : q)
        if (x) (void)hipFree(x);
    for (int32_t* x : w->pmap)
        if (x) (void)hipFree(x);
    delete w;
    ctx->blk = nullptr;
}

int pp_update_conv_image(pp_ctx* ctx, int k, const float* w, hipStream_t stream, bool any_plan)
{
    if (k < 0 || k >= 16) return pp_fail(ctx, PP_E_ARG, "pp_update_conv_image: k must be 0 .. 15");
    block_ws* ws = workspace(ctx);
    pp_block_image& im = ws->img[k];
    if (ws->img_gen[k] != ctx->commit_gen) { // first update after a commit: read the committed image's layout back (synchronous)
        ws->img_gen[k] = 0;
        if (int rc = pp_net_conv_image(ctx, k, &im, any_plan)) return rc;
        if (ws->pmap[k]) { (void)hipFree(ws->pmap[k]); ws->pmap[k] = nullptr; }
        PP_HIP(hipMalloc((void**)&ws->pmap[k], im.pmap.size() * sizeof(int32_t)));
        PP_HIP(hipMemcpy(ws->pmap[k], im.pmap.data(), im.pmap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        ws->img_gen[k] = ctx->commit_gen;
    }
    const int n = (int)im.pmap.size();
    hipLaunchKernelGGL(k_unit_image, dim3(pp_div_up(n, 256)), dim3(256), 0, stream, im.w, ws->pmap[k], n, w, im.T, im.rows * im.C);
    return 0;
}

namespace {

// ---- the one fp32 driver of the family.  The forms differ in the passes around the two products: InstanceNorm runs the statistics and
// k_unit_pack ahead of them and the two passes of the norm backward behind the dgrad; the affine form k_affine_unit_pack and one pass
// behind the dgrad, with k_affine_reduce behind the chunks; the batch form the affine pack, the sums behind the dgrad of every chunk (raw
// da -> du), and behind the chunks k_bn_coef and one in-place k_bn_unit_du over all frames --------------------------------------------------
int unit_run(pp_ctx* ctx, norm_form form, const unit_shape& s, const unit_args& a)
{
    const int C = s.C, h = s.h, w = s.w, nb = a.nb;
    hipStream_t stream = a.stream;
    PP_HIP(hipSetDevice(ctx->device));
    block_ws* ws = workspace(ctx);
    const pad_geom g = padded_plane(h, w);
    const unit_plan p = unit_make_plan(ctx, s, nb, a.chunk_frames, g, 2 * (size_t)C * g.PS * sizeof(float), 16, 64);
    const int wp = g.wp, PP = g.PP, G = g.G, PS = g.PS, N = p.N, fc = p.fc, S = p.S, L = p.L, SP = p.SP, LP = p.LP;
    // stm: a chunk's mean / rstd (InstanceNorm) or k_bn_coef's coefficients (batch); pst: a chunk's segment sums (InstanceNorm) or
    // every frame's, reduced or pooled once behind the chunks
    const size_t stm_elems = form == NORM_INSTANCE ? (size_t)fc * C * 2 : (size_t)C * 4;
    const size_t pst_elems = (size_t)(form == NORM_INSTANCE ? fc : nb) * C * SEG_MAX * 2;
    int rc;
    if ((rc = grow(ctx, &ws->planes, &ws->planes_elems, 2 * (size_t)fc * p.pf_elems)) ||
        (form != NORM_AFFINE && (rc = grow(ctx, &ws->stm, &ws->stm_elems, stm_elems))) ||
        (rc = grow(ctx, &ws->pst, &ws->pst_elems, pst_elems)) ||
        (rc = grow(ctx, &ws->part, &ws->part_elems, (size_t)p.Gp * p.nw)) ||
        (a.du && (rc = grow(ctx, &ws->wT, &ws->wT_elems, (size_t)p.nw))))
        return rc;
    float* ap = ws->planes;
    float* dzp = ws->planes + (size_t)fc * p.pf_elems;
    if (a.du) hipLaunchKernelGGL(k_conv3_wt, dim3(pp_div_up(p.nw, 256)), dim3(256), 0, stream, a.wgt, ws->wT, C, C);
    for_chunks(p.walk, [&](const dw_chunk& c) {
        const int fn = c.fn;
        const size_t o = (size_t)c.f0 * C * N;
        if (form == NORM_INSTANCE) {
            hipLaunchKernelGGL(k_plane_stats, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, ws->pst, C, N, L, S);
            hipLaunchKernelGGL(k_unit_pack, dim3(C, fn, SP), dim3(256), 0, stream, a.u + o, a.dy + o, ap, dzp, ws->stm, ws->pst, C, h, w, wp, G, PP, PS, S,
                               LP);
        } else {
            hipLaunchKernelGGL(k_affine_unit_pack, dim3(C, fn, SP), dim3(256), 0, stream, a.u + o, a.dy + o, ap, dzp, a.scale, a.shift, C, h, w, wp, G,
                               PP, PS, LP);
        }
        const dim3 gd(p.NC / p.TN, C / 64, c.sp);
        if (C >= 128)
            hipLaunchKernelGGL((k_conv3_wgrad<4, 2, taps_s1>), gd, dim3(256), 0, stream, dzp, ap, ws->part, C, C, wp, G, PS, p.cpf, c.nchunks, c.cps,
                               c.gbase);
        else
            hipLaunchKernelGGL((k_conv3_wgrad<3, 4, taps_s1>), gd, dim3(256), 0, stream, dzp, ap, ws->part, C, C, wp, G, PS, p.cpf, c.nchunks, c.cps,
                               c.gbase);
        if (!a.du) return;
        float* duc = a.du + o;
        if (C == 64)
            hipLaunchKernelGGL(k_unit_dgrad<1>, dim3(pp_div_up(PP, 128), 1, fn), dim3(256), 0, stream, ws->wT, dzp, duc, C, h, w, wp, G, PP, PS);
        else if (C == 128)
            hipLaunchKernelGGL(k_unit_dgrad<2>, dim3(pp_div_up(PP, 64), 1, fn), dim3(256), 0, stream, ws->wT, dzp, duc, C, h, w, wp, G, PP, PS);
        else
            hipLaunchKernelGGL(k_unit_dgrad<4>, dim3(pp_div_up(PP, 32), 1, fn), dim3(256), 0, stream, ws->wT, dzp, duc, C, h, w, wp, G, PP, PS);
        if (form == NORM_INSTANCE) {
            hipLaunchKernelGGL(k_plane_gstats, dim3(C, fn, S), dim3(256), 0, stream, ap, duc, ws->pst, C, w, wp, G, PS, N, L, S);
            hipLaunchKernelGGL(k_unit_norm, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, ap, ws->stm, ws->pst, a.dskip ? a.dskip + o : nullptr, duc, C,
                               h, w, wp, G, PS, L, S);
        } else if (form == NORM_AFFINE) {
            hipLaunchKernelGGL(k_affine_unit_du<false>, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, ap, a.scale, a.shift,
                               a.dskip ? a.dskip + o : nullptr, duc, ws->pst + (size_t)c.f0 * C * S * 2, C, w, wp, G, PS, N, L, S);
        } else {
            hipLaunchKernelGGL(k_bn_plane_sums, dim3(C, fn, S), dim3(256), 0, stream, a.u + o, duc, a.scale, a.shift, ws->pst + (size_t)c.f0 * C * S * 2,
                               C, N, L, S);
        }
    });
    launch_dw_reduce(ws->part, p.Gp, p.nw, a.dw, stream);
    if (form == NORM_AFFINE && a.dscale)
        hipLaunchKernelGGL(k_affine_reduce, dim3(pp_div_up(C, 64)), dim3(64), 0, stream, ws->pst, nb, C, S, a.dscale, a.dshift);
    if (form == NORM_BATCH && a.du) {
        hipLaunchKernelGGL(k_bn_coef, dim3(pp_div_up(C, 64)), dim3(64), 0, stream, ws->pst, nb, C, S, a.mean, a.var, (double)nb * (double)N, ws->stm,
                           a.dscale, a.dshift);
        hipLaunchKernelGGL(k_bn_unit_du, dim3(C, nb, S), dim3(256), 0, stream, a.u, a.scale, a.shift, ws->stm, a.dskip, a.du, C, N, L);
    }
    PP_HIP(hipGetLastError());
    return 0;
}

int unit_entry(pp_ctx* ctx, const char* entry, norm_form form, const unit_shape& s, const unit_args& a)
{
    if (!ctx) return PP_E_ARG;
    if (int rc = unit_check(ctx, entry, UNIT_CHK_ALL, form, s, a)) return rc;
    return unit_run(ctx, form, s, a);
}

} // namespace

extern "C" int pp_unit_backward(pp_ctx* ctx, int C, int h, int w, const float* u, const float* wgt, const float* dy, const float* dskip, int nb,
                                float* dw, float* du, void* stream_)
{
    unit_args a;
    a.u = u; a.wgt = wgt; a.dy = dy; a.dskip = dskip; a.nb = nb; a.dw = dw; a.du = du; a.stream = (hipStream_t)stream_;
    return unit_entry(ctx, "pp_unit_backward", NORM_INSTANCE, unit_shape{C, h, w}, a);
}

// pp_unit_backward with a per-channel affine for the norm: the pack without statistics, the same two products over the same planes, K
// ranges and frame chunks, and one pass behind the dgrad in place of the two of the norm backward.
extern "C" int pp_unit_backward_affine(pp_ctx* ctx, int C, int h, int w, const float* u, const float* wgt, const float* scale, const float* shift,
                                       const float* dy, const float* dskip, int nb, float* dw, float* du, double* dscale, double* dshift,
                                       void* stream_)
{
    unit_args a;
    a.u = u; a.wgt = wgt; a.scale = scale; a.shift = shift; a.dy = dy; a.dskip = dskip; a.nb = nb; a.dw = dw; a.du = du;
    a.dscale = dscale; a.dshift = dshift; a.stream = (hipStream_t)stream_;
    return unit_entry(ctx, "pp_unit_backward_affine", NORM_AFFINE, unit_shape{C, h, w}, a);
}

// pp_unit_backward_affine behind a train-mode BatchNorm: (scale, shift) are the fold of the batch statistics (mean, var) the forward
// used.  Two phases across the frame chunks: the chunks run pack, wgrad and dgrad (raw da -> du) and the segment sums; once every
// frame's sums are in, k_bn_coef pools them and one in-place pass over all frames writes du.  chunk_frames > 0 caps the frames of a
// chunk below the workspace rule (du and the sums do not depend on it; dw does within fp32 summation error, through the K ranges).
extern "C" int pp_unit_backward_bn(pp_ctx* ctx, int C, int h, int w, const float* u, const float* wgt, const float* scale, const float* shift,
                                   const float* mean, const float* var, const float* dy, const float* dskip, int nb, float* dw, float* du,
                                   double* dscale, double* dshift, int chunk_frames, void* stream_)
{
    unit_args a;
    a.u = u; a.wgt = wgt; a.scale = scale; a.shift = shift; a.mean = mean; a.var = var; a.dy = dy; a.dskip = dskip; a.nb = nb; a.dw = dw;
    a.du = du; a.dscale = dscale; a.dshift = dshift; a.chunk_frames = chunk_frames; a.stream = (hipStream_t)stream_;
    return unit_entry(ctx, "pp_unit_backward_bn", NORM_BATCH, unit_shape{C, h, w}, a);
}

extern "C" int pp_update_block_weights(pp_ctx* ctx, int block, const float* const* w, int n, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_ARG, "pp_update_block_weights: no committed weights to update (pp_commit_weights first)");
    if (block != 2 || n != 5)
        return pp_fail(ctx, PP_E_ARG, "pp_update_block_weights: block 3 only (block = 2, n = 5): blocks 1 and 2 have no backward yet, and level 0 "
                                      "carries the tile-skipping path");
    if (!w) return pp_fail(ctx, PP_E_ARG, "pp_update_block_weights: null pointer");
    for (int k = 0; k < n; ++k)
        if (!w[k] || ((uintptr_t)w[k] & 3)) return pp_fail(ctx, PP_E_ARG, "pp_update_block_weights: null or misaligned weight pointer");
    if (pp_effective_precision(ctx) != 0)
        return pp_fail(ctx, PP_E_ARG, "pp_update_block_weights: fp32 mode only (the committed plan packs the convolutions in a 16-bit format)");
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    for (int k = 0; k < 5; ++k) { // block 3's units: images 11 .. 15
        int rc = pp_update_conv_image(ctx, 11 + k, w[k], stream);
        if (rc) return rc;
    }
    PP_HIP(hipGetLastError());
    return 0;
}

// All sixteen 3 x 3 convolutions of the RPN in execution order (= state_dict order): per level its strided convolution, then its 3 | 5 | 5
// unit convolutions.  Level 0's strided weight is also the sparse first convolution's, which keeps an image of its own.
extern "C" int pp_update_rpn_weights(pp_ctx* ctx, const float* const* w, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_ARG, "pp_update_rpn_weights: no committed weights to update (pp_commit_weights first)");
    if (!w) return pp_fail(ctx, PP_E_ARG, "pp_update_rpn_weights: null pointer");
    for (int k = 0; k < 16; ++k)
        if (!w[k] || ((uintptr_t)w[k] & 3)) return pp_fail(ctx, PP_E_ARG, "pp_update_rpn_weights: null or misaligned weight pointer");
    if (pp_effective_precision(ctx) != 0)
        return pp_fail(ctx, PP_E_ARG, "pp_update_rpn_weights: fp32 mode only (the committed plan packs the convolutions in a 16-bit format)");
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    int rc = 0;
    for (int k = 0; k < 16 && !rc; ++k) rc = pp_update_conv_image(ctx, k, w[k], stream);
    if (!rc) rc = pp_sc1_update(ctx, w[0], stream);
    if (rc) return rc;
    PP_HIP(hipGetLastError());
    return 0;
}

// pp_update_rpn_weights for a plan committed in a 16-bit mode (1 bf16x3, 2 bf16, 3 fp16): every convolution on a 16-bit tiling is
// rewritten by k_image16 (image16.hip), one that keeps an fp32 tiling by the fp32 writer above.  The sparse first convolution is fp32
// only and keeps no image a 16-bit pass reads: a return to fp32 commits again.
extern "C" int pp_update_rpn_weights_mp(pp_ctx* ctx, int mode, const float* const* w, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_ARG, "pp_update_rpn_weights_mp: no committed weights to update (pp_commit_weights first)");
    if (!w) return pp_fail(ctx, PP_E_ARG, "pp_update_rpn_weights_mp: null pointer");
    for (int k = 0; k < 16; ++k)
        if (!w[k] || ((uintptr_t)w[k] & 3)) return pp_fail(ctx, PP_E_ARG, "pp_update_rpn_weights_mp: null or misaligned weight pointer");
    if (int rc = pp_mp_mode_check(ctx, "pp_update_rpn_weights_mp", mode)) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    PP_HIP(hipSetDevice(ctx->device));
    for (int k = 0; k < 16; ++k) {
        const int layer = pp_net_layer_index(ctx, 0, k);
        const int cout = k < 4 ? 64 : k < 10 ? 128 : 256, cin = k == 0 || k == 4 ? 64 : k == 10 ? 128 : cout;
        bool is16 = false;
        int rc = pp_update_image16(ctx, layer, w[k], nullptr, nullptr, cout * cin * 9, 0, 0, stream, &is16);
        if (!rc && !is16) rc = pp_update_conv_image(ctx, k, w[k], stream, true);
        if (rc) return rc;
    }
    PP_HIP(hipGetLastError());
    return 0;
}
