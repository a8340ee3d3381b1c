// gemm1x1: the persistent 1x1 GEMM family of the 2D backbone (Family::Gemm1x1), fp32 / bf16x3 / bf16 / fp16 MFMA for gfx950.
//
// 1x1 contractions (the three ConvTranspose(k = s) upsamplers and the shared head) as a persistent,
// barrier-free GEMM:  D[rows, pixel] = W[rows, K] * relu(norm(X[K, pixel]))
// * the [K][BM] weight slab of the workgroup's row block stays in LDS for the whole launch
//   (head: 320 x 96, deconv3: 256 x 128 -> up to 147 KB of the 160 KB)
// * activations never touch LDS: lane (pixel m, channel c+kq) loads its B operand straight from
//   global memory into a 4-step register ring, applies the producer's normalisation + ReLU in
//   registers, and feeds the MFMAs -- every wave streams on its own, no workgroup barrier
// * pixels are flattened (a 1x1 conv has no neighbourhood), N-tile = 16 consecutive pixels
#include <cstdio>
#include "pp_common.h"
#include "conv_common.h"

namespace {

using namespace ppc;

// PREC (the reference's deployed path is TensorRT FP16, framework/trt_utils.py:30): 0 = fp32 MFMA (exact);
// 1 = split-bf16 "bf16x3": x = hi + lo with hi = bf16(x), lo = bf16(x - hi), a*b ~ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on
// v_mfma_f32_16x16x16_bf16 with fp32 accumulation (~2^-16 relative per product: fp32-equivalent for this network, three MFMAs at
// 8x the fp32-MFMA rate); 2 = plain bf16 operands (one MFMA, ~2^-8 per product); 3 = fp16 operands on v_mfma_f32_16x16x16_f16
// (~2^-11 per product: the arithmetic of the reference's TensorRT FP16 engines).
// Activations stay fp32 in HBM: normalise + ReLU in fp32, then split / round while staging.  The weight slab in LDS is
// [K/16][hi|lo][k-group 0..3][BMP rows][4 bf16] -- the same bytes as the fp32 slab.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_bf16(float a, float b) // v_cvt_pk_bf16_f32 (round to nearest even)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
}
// one 16-deep MFMA of the reduced-precision 1x1 path: bf16 operands (PREC 1, 2) or fp16 operands (PREC 3), fp32 accumulate
template <int PREC>
__device__ __forceinline__ f32x4 mfma_lp(const s16x4 a, const s16x4 b, const f32x4 c)
{
    if constexpr (PREC == 3) return __builtin_amdgcn_mfma_f32_16x16x16f16(__builtin_bit_cast(f16x4_t, a), __builtin_bit_cast(f16x4_t, b), c, 0, 0, 0);
    else return __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(a, b, c, 0, 0, 0);
}

// IO16 (pp_set_precision 4, "fp16s": fp16 operands AND fp16 storage of the [320,H,W] concat buffer the upsamplers write and the head
// reads -- the largest tensor of the network, 205 MB per frame in fp32): bit 0 = the input tensor is fp16, bit 1 = the output is.
// EPI_HEAD_CLS (deferred head, MT = 1): the head's `na` cls rows alone -- the slab is gathered out of the committed full head image
// (cls row of anchor a = tile row 4 (9 + a) + 3 of head_tile_row), so there is one weight image and the cls logits are bit-identical to
// the full head's: same A and B values, same channel-quad order, same bias add.  One MFMA per 256 B loaded: the kernel is bound by the
// bytes in flight per CU: it runs two workgroups per CU (a 128-register budget; at the 64 registers of four per CU the ring spills)
// and PDX varies the ring depth.
template <int MT, int NT, int EPI, int PREC = 0, int IO16 = 0, int PDX = 0>
__global__ void __launch_bounds__(512, EPI == EPI_HEAD_CLS ? 4 : 2) gemm1x1(const ConvP p)
{
    constexpr bool IN16 = (IO16 & 1) != 0, OUT16 = (IO16 & 2) != 0;
    static_assert(IO16 == 0 || PREC != 0, "16-bit storage comes with the 16-bit operand path");
    static_assert(!OUT16 || EPI != EPI_HEAD, "the head's logits stay fp32");
    constexpr int BM = MT * 16;
    constexpr int BMP = BM + ((BM % 32 == 0) ? 16 : 0);
    static_assert(EPI != EPI_HEAD_CLS || (MT == 1 && PREC == 0 && IO16 == 0), "the cls-only head pass is one fp32 M-tile");
    constexpr int PD = PDX ? PDX : (MT >= 8) ? 4 : 8; // B-operand ring depth (steps in flight); even, K % (4 * PD) == 0; 128 accumulator registers leave room for 4
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* wl = smem;                         // [K][BMP]
    const int K = p.Cin;
    float* sc_all = wl + (size_t)K * BMP;     // [8 waves][2][K]  wave-private (scale, shift)
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6); // scalar: frame, item and the buffer descriptor stay in SGPRs
    const int m = lane & 15, kq = lane >> 4;
    float* scl = sc_all + (size_t)wave * 2 * K;
    float* shl = scl + K;

    const int ncb = (p.Cout + BM - 1) / BM;
    // XCD-aware: workgroups are dealt round-robin over the 8 XCDs, so the ncb channel blocks that stream the
    // SAME pixels are given ids 8 apart -- they share one L2 instead of fetching the input once per XCD
    const bool xcd_ok = gridDim.x % (8 * ncb) == 0;
    const int xj = blockIdx.x >> 3, xk = blockIdx.x & 7;
    const int cb = xcd_ok ? xj % ncb : blockIdx.x % ncb;
    const int wi = xcd_ok ? xk + 8 * (xj / ncb) : blockIdx.x / ncb, nworkers = gridDim.x / ncb;
    if (wi >= nworkers) return;
    const int co0 = cb * BM;
    if constexpr (EPI == EPI_HEAD_CLS) { // column a of the slab = the cls row of anchor a in the full image [row block][K][w_bmp]; columns na .. 15 are zero
        for (int e = tid; e < K * BMP; e += 512) {
            const int k = e / BMP, a = e - k * BMP, t = 4 * (9 + a) + 3;
            wl[e] = a < p.n_cls ? p.w[((size_t)(t / p.w_bm) * K + k) * p.w_bmp + t % p.w_bm] : 0.f;
        }
    } else {
        const f32x4* g = reinterpret_cast<const f32x4*>(p.w) + (size_t)cb * ((size_t)K * BMP / 4);
        f32x4* d = reinterpret_cast<f32x4*>(wl);
        for (int e = tid; e < K * BMP / 4; e += 512) d[e] = g[e];
    }
    __syncthreads(); // the only workgroup barrier
    __builtin_amdgcn_s_setprio(1); // item prologue / epilogue run at raised priority, the MFMA stream at 0

    const int HW = p.Hout * p.Wout;
    const int items_per_frame = (HW + NT * 16 - 1) / (NT * 16);
    const int total = items_per_frame * p.nb;
    const size_t plane = (size_t)HW;
    const int gw = wi * 8 + wave, gstride = nworkers * 8;

    // per-row partial statistics: the plain epilogue keeps one pair per tile row, the pixel-shuffle epilogues fold a
    // lane's 4 rows (the s^2 positions of ONE output channel) into slot 0 -- 4x fewer live registers at MT = 8
    constexpr int SR = (EPI == EPI_PLAIN) ? 4 : 1;
    float ssum[MT][SR], ssq[MT][SR];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < SR; ++r) { ssum[i][r] = 0.f; ssq[i][r] = 0.f; }
    int stat_frame = -1, pre_frame = -1;
    auto flush_stats = [&](int frame) {
        if (EPI == EPI_HEAD || EPI == EPI_HEAD_CLS || !p.stat_acc || frame < 0) return;
        double* base = p.stat_acc + (size_t)frame * p.stat_fs + ((size_t)((blockIdx.x * 8 + wave) % NREP) * p.stat_C) * 2;
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < SR; ++r) {
                float s = ssum[i][r], q = ssq[i][r];
                s = row16_sum(s);
                q = row16_sum(q);
                const int row = co0 + i * 16 + kq * 4 + r;
                int ch = row;
                bool lead = (m == 0);
                if (EPI == EPI_UP2) { ch = row >> 2; lead = lead && r == 0; }
                if (EPI == EPI_UP4) { ch = row >> 4; lead = lead && r == 0; }
                if (lead && row < p.Cout) {
                    atomicAdd(base + (size_t)ch * 2, (double)s);
                    atomicAdd(base + (size_t)ch * 2 + 1, (double)q);
                }
                ssum[i][r] = 0.f;
                ssq[i][r] = 0.f;
            }
    };

    const int aoff = kq * BMP + m;
    static_assert(NT == 4, "gemm1x1 is written for 4 interleaved N-tiles");
    const int nsteps = K / 4;
    const unsigned bstep = 16u * (unsigned)plane; // bytes between channel quads
    // ---- load-side state of the item whose B quads are being requested.  At an item boundary it runs one item
    //      AHEAD: the next item's first PD-1 quads are requested BEFORE this item's epilogue, so they are older than
    //      its stores in the (in-order) vmcnt queue and their latency hides under the epilogue.
    __amdgpu_buffer_rsrc_t rb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, 0x7FFFFFFF, 0x00020000);
    unsigned bvoff = 0u;
    f32x4 bq[PD];
    auto set_load_item = [&](int it) {
        const int f_ = __builtin_amdgcn_readfirstlane(it / items_per_frame); // the division runs on the VALU: pin the
        const int px_ = __builtin_amdgcn_readfirstlane((it - f_ * items_per_frame) * (NT * 16)) + 4 * m; // results in SGPRs
        // descriptor base pinned to SGPRs (a VGPR-resident descriptor costs a waterfall loop per load)
        const uint64_t bp_ = IN16 ? (uint64_t)(reinterpret_cast<const _Float16*>(p.in) + (size_t)f_ * p.in_fs) : (uint64_t)(p.in + (size_t)f_ * p.in_fs);
        const uint64_t bps_ = ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(bp_ >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)bp_);
        rb = __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<float*>(bps_), 0, 0x7FFFFFFF, 0x00020000);
        bvoff = ((unsigned)kq * (unsigned)plane + (unsigned)(px_ < HW ? px_ : 0)) * (IN16 ? 2u : 4u);
    };
#define G1_LOADB(S, SLOT) bq[SLOT] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, bvoff, (unsigned)(S) * bstep, 0));
#define G1_PREP(S, SLOT, PAR)                                                                    \
    {                                                                                            \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) a[PAR][i] = wl[(S) * 4 * BMP + aoff + i * 16]; \
        if (p.pre != PRE_RAW) {                                                                  \
            const float sc = scl[(S) * 4 + kq], sh = shl[(S) * 4 + kq];                          \
            _Pragma("unroll") for (int j = 0; j < NT; ++j) b[PAR][j] = fmaxf(fmaf(bq[SLOT][j], sc, sh), 0.f); \
        } else {                                                                                 \
            _Pragma("unroll") for (int j = 0; j < NT; ++j) b[PAR][j] = bq[SLOT][j];              \
        }                                                                                        \
    }
#define G1_MFMAS(PAR)                                                                            \
    {                                                                                            \
        __builtin_amdgcn_sched_barrier(0);                                                       \
        _Pragma("unroll") for (int i = 0; i < MT; ++i)                                           \
            _Pragma("unroll") for (int j = 0; j < NT; ++j)                                       \
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[PAR][i], b[PAR][j], acc[i][j], 0, 0, 0); \
        __builtin_amdgcn_sched_barrier(0);                                                       \
    }
    if constexpr (PREC == 0) {
    if (gw < total) {
        set_load_item(gw);
#pragma unroll
        for (int s0 = 0; s0 < PD - 1; ++s0) G1_LOADB(s0, s0)
    }
    }
    for (int item = gw; item < total; item += gstride) {
        const int fr = __builtin_amdgcn_readfirstlane(item / items_per_frame);
        const int pix0 = __builtin_amdgcn_readfirstlane((item - fr * items_per_frame) * (NT * 16));
        if (fr != stat_frame) { flush_stats(stat_frame); stat_frame = fr; }
        if (p.pre != PRE_RAW && fr != pre_frame) {
            for (int c = lane; c < K; c += 64) {
                if (p.pre == PRE_STATS) {
                    const double* pa = p.pre_acc + (size_t)fr * p.pre_fs;
                    double s = 0.0, q = 0.0;
#pragma unroll
                    for (int r = 0; r < NREP; ++r) { s += pa[((size_t)r * K + c) * 2]; q += pa[((size_t)r * K + c) * 2 + 1]; }
                    const double mean = s * p.pre_inv_n;
                    double var = q * p.pre_inv_n - mean * mean;
                    var = var > 0.0 ? var : 0.0;
                    const double rstd = 1.0 / sqrt(var + (double)p.eps);
                    scl[c] = (float)rstd;
                    shl[c] = (float)(-mean * rstd);
                } else {
                    scl[c] = p.pre_scale[(size_t)fr * p.aff_fs + c];
                    shl[c] = p.pre_shift[(size_t)fr * p.aff_fs + c];
                }
            }
            pre_frame = fr;
        }
        // N-tile j of this item = pixels {pix0 + 4m + j}: one dwordx4 per lane and step feeds all four tiles
        const int pxb = pix0 + 4 * m;       // first of this lane's 4 pixels (HW % 4 == 0: all four valid or none)
        const bool pok = pxb < HW;
        f32x4 acc[MT][NT];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

        if constexpr (PREC == 0) {
        // K % (4 * PD) == 0 (layer_menu offers this kernel only then): no tail steps.
        // Per step: the B quad of step st+PD-1 is requested (buffer load: lane offset in a VGPR, the channel-quad
        // offset in an SGPR -- no address VALU), the A fragments and the normalised B values of step st+1 are
        // prepared in the shadow of this step's MT*NT MFMAs, then the MFMAs issue.  The last ring is peeled so
        // that no step carries a run-time condition.
        float a[2][MT], b[2][NT];
        G1_PREP(0, 0, 0)
        __builtin_amdgcn_s_setprio(0); // the MFMA stream yields issue slots to the other wave's short non-MFMA segments
        int sb = 0;
        for (; sb < nsteps - PD; sb += PD) {
#pragma unroll
            for (int u = 0; u < PD; ++u) {
                G1_LOADB(sb + u + PD - 1, (u + PD - 1) % PD)
                G1_PREP(sb + u + 1, (u + 1) % PD, (u + 1) & 1)
                G1_MFMAS(u & 1)
            }
        }
        // last ring: only its first step still has a quad to request, the last one nothing to prepare
        G1_LOADB(sb + PD - 1, PD - 1)
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            if (u + 1 < PD) G1_PREP(sb + u + 1, (u + 1) % PD, (u + 1) & 1)
            G1_MFMAS(u & 1)
        }

        __builtin_amdgcn_s_setprio(1);
        if (item + gstride < total) { // next item's first quads, ahead of this item's stores
            set_load_item(item + gstride);
#pragma unroll
            for (int s0 = 0; s0 < PD - 1; ++s0) G1_LOADB(s0, s0)
        }

        } else {
            // ---- reduced-precision K loop: 16 input channels per block = one bf16 MFMA depth.  Lane (pixel group m, k-group kq)
            //      loads channels kq*4 .. kq*4+3 of the block for its 4 pixels (4 dwordx4, block kb+1 in flight behind block kb),
            //      normalises in fp32, packs 4 channels of one pixel into one B operand (two v_cvt_pk_bf16_f32) ----
            set_load_item(item);
            constexpr unsigned EB = IN16 ? 2u : 4u;                                 // bytes per input element
            const unsigned bvq = bvoff + (unsigned)kq * 3u * (unsigned)plane * EB; // (kq*4*plane + pixel)*EB: bvoff already holds kq*plane
            const unsigned cstep = (unsigned)plane * EB;                            // bytes between channels
            const uint2* wl2 = reinterpret_cast<const uint2*>(wl);
            const int nkb = K / 16;
            f32x4 q0[4], q1[4];
            uint2 g0[4], g1[4]; // fp16 input: a lane's 4 pixels of a channel are 8 bytes, kept as they arrive
#define G1_LP_LOAD(Q, G, KB) _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                                  \
        if constexpr (IN16) G[t] = __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(rb, bvq, (unsigned)((KB) * 16 + t) * cstep, 0)); \
        else Q[t] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rb, bvq, (unsigned)((KB) * 16 + t) * cstep, 0)); \
    }
            // RAW (compile-time twin of the loop, chosen per launch: the upsamplers read raw block outputs, the fused head normalises):
            // no (scale, shift) reads and no fma / max; an fp16 raw input is already the operand's arithmetic -- channel pairs of
            // pixel j are picked out of the (pixel-pair) words with two v_perm_b32, no conversion at all
#define G1_LP_BLOCK(Q, G, KB, RAW)                                                               \
    {                                                                                            \
        f32x4 sc4 = (f32x4){1.f, 1.f, 1.f, 1.f}, sh4 = (f32x4){0.f, 0.f, 0.f, 0.f};              \
        if constexpr (!(RAW)) { sc4 = *reinterpret_cast<const f32x4*>(scl + (KB) * 16 + kq * 4); sh4 = *reinterpret_cast<const f32x4*>(shl + (KB) * 16 + kq * 4); } \
        s16x4 bh[NT], bl[NT];                                                                    \
        _Pragma("unroll") for (int j = 0; j < NT; ++j) {                                         \
            if constexpr (IN16 && (RAW)) {                                                       \
                const unsigned sel_ = (j & 1) ? 0x07060302u : 0x05040100u;                       \
                const unsigned h0 = __builtin_amdgcn_perm((j & 2) ? G[1].y : G[1].x, (j & 2) ? G[0].y : G[0].x, sel_); \
                const unsigned h1 = __builtin_amdgcn_perm((j & 2) ? G[3].y : G[3].x, (j & 2) ? G[2].y : G[2].x, sel_); \
                bh[j] = __builtin_bit_cast(s16x4, (uint2){h0, h1});                              \
            } else {                                                                             \
                float v_[4];                                                                     \
                _Pragma("unroll") for (int t = 0; t < 4; ++t) {                                  \
                    float x_;                                                                    \
                    if constexpr (IN16) x_ = (float)__builtin_bit_cast(f16x4_t, G[t])[j]; else x_ = Q[t][j]; \
                    v_[t] = (RAW) ? x_ : fmaxf(fmaf(x_, sc4[t], sh4[t]), 0.f);                   \
                }                                                                                \
                const unsigned h0 = (PREC == 3) ? pk_f16(v_[0], v_[1]) : pk_bf16(v_[0], v_[1]);  \
                const unsigned h1 = (PREC == 3) ? pk_f16(v_[2], v_[3]) : pk_bf16(v_[2], v_[3]);  \
                bh[j] = __builtin_bit_cast(s16x4, (uint2){h0, h1});                              \
                if constexpr (PREC == 1) {                                                       \
                    const float l0 = v_[0] - __uint_as_float(h0 << 16), l1 = v_[1] - __uint_as_float(h0 & 0xFFFF0000u); \
                    const float l2 = v_[2] - __uint_as_float(h1 << 16), l3 = v_[3] - __uint_as_float(h1 & 0xFFFF0000u); \
                    bl[j] = __builtin_bit_cast(s16x4, (uint2){pk_bf16(l0, l1), pk_bf16(l2, l3)}); \
                }                                                                                \
            }                                                                                    \
        }                                                                                        \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) {                                         \
            const s16x4 ah = __builtin_bit_cast(s16x4, wl2[(((KB) * 2 + 0) * 4 + kq) * BMP + i * 16 + m]); \
            s16x4 al = ah;                                                                       \
            if constexpr (PREC == 1) al = __builtin_bit_cast(s16x4, wl2[(((KB) * 2 + 1) * 4 + kq) * BMP + i * 16 + m]); \
            _Pragma("unroll") for (int j = 0; j < NT; ++j) {                                     \
                acc[i][j] = mfma_lp<PREC>(ah, bh[j], acc[i][j]);                                 \
                if constexpr (PREC == 1) {                                                       \
                    acc[i][j] = mfma_lp<PREC>(ah, bl[j], acc[i][j]);                             \
                    acc[i][j] = mfma_lp<PREC>(al, bh[j], acc[i][j]);                             \
                }                                                                                \
            }                                                                                    \
        }                                                                                        \
    }
#define G1_LP_LOOP(RAW)                                                                          \
    G1_LP_LOAD(q0, g0, 0)                                                                        \
    for (int kb = 0; kb < nkb; kb += 2) { /* K % 32 == 0: whole pairs of blocks */               \
        G1_LP_LOAD(q1, g1, kb + 1)                                                               \
        G1_LP_BLOCK(q0, g0, kb, RAW)                                                             \
        if (kb + 2 < nkb) G1_LP_LOAD(q0, g0, kb + 2)                                             \
        G1_LP_BLOCK(q1, g1, kb + 1, RAW)                                                         \
    }
            __builtin_amdgcn_s_setprio(0);
            if (p.pre == PRE_RAW) { G1_LP_LOOP(true) } else { G1_LP_LOOP(false) }
            __builtin_amdgcn_s_setprio(1);
#undef G1_LP_LOOP
#undef G1_LP_LOAD
#undef G1_LP_BLOCK
        }

        // ---- epilogue of this item (lane m owns pixels pxb .. pxb+3, one per N-tile) ----
        // OUT16: `gout` counts in ELEMENTS of the output tensor either way; st4 rounds four values to fp16 and stores 8 bytes
        float* gout = OUT16 ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(p.out) + (size_t)fr * p.out_fs) : p.out + (size_t)fr * p.out_fs;
        auto st4 = [&](size_t off, const f32x4 v) __attribute__((always_inline)) {
            if constexpr (OUT16) {
                const uint2 h = {pk_f16(v[0], v[1]), pk_f16(v[2], v[3])};
                *reinterpret_cast<uint2*>(reinterpret_cast<_Float16*>(gout) + off) = h;
            } else {
                *reinterpret_cast<f32x4*>(gout + off) = v;
            }
        };
        float* gbox = p.out_box ? p.out_box + (size_t)fr * p.box_fs : nullptr;
        float* gdir = p.out_dir ? p.out_dir + (size_t)fr * p.dir_fs : nullptr;
        bool up4_done = false;
        if constexpr (EPI == EPI_UP4) {
            if ((p.Wout & 3) == 0) {
                // ConvTranspose k = s = 4: a lane's 4 pixels x 4 dx are 64 CONTIGUOUS output bytes (out[co][4y+dy][4x .. 4x+15]), but stored
                // as it stands (one 16-byte piece per N-tile j) an instruction writes 16 bytes of each of 16 runs -- 64 scattered
                // 16-byte requests.  The four lanes of a quad transpose their 4 x 4 pieces (out[k] on lane t = piece t of lane
                // 4q + k's run: two butterfly stages of DPP quad permutes) so that instruction k writes WHOLE 64-byte runs, four
                // lanes each.  All lanes take part (a DPP source must be live); a run beyond the map is dropped at the store.
                up4_done = true;
                int kq_e = kq;
                asm volatile("" : "+v"(kq_e));
                const int t_ = m & 3;
                size_t ko[4];
                bool kok[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int pk = pix0 + 4 * ((m & ~3) + k); // first pixel of lane 4q + k
                    const int yk = pk / p.Wout, xk = pk - yk * p.Wout;
                    kok[k] = pk < HW;
                    ko[k] = (size_t)(4 * yk) * ((size_t)p.Wout * 4) + 4 * (size_t)xk + 4 * t_; // run of lane 4q + k starts at output x = 4 xk; this lane writes its piece t
                }
#pragma unroll
                for (int i = 0; i < MT; ++i) {
                    const int row0 = co0 + i * 16 + kq_e * 4;
                    if (row0 >= p.Cout) continue; // wave-uniform per kq group of 16 lanes: quads stay whole
                    const int co = row0 >> 4, dy = (row0 >> 2) & 3;
                    f32x4 o4[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float a0 = acc[i][0][r], a1 = acc[i][1][r], a2 = acc[i][2][r], a3 = acc[i][3][r];
                        if (pok) {
                            ssum[i][0] += (a0 + a1) + (a2 + a3);
                            ssq[i][0] += (a0 * a0 + a1 * a1) + (a2 * a2 + a3 * a3);
                        }
                        // stage 1: swap the low bit of (register j, lane t); stage 2: the high bit
                        const float x0 = dpp_f32<0xB1>(a1), x1 = dpp_f32<0xB1>(a0), x2 = dpp_f32<0xB1>(a3), x3 = dpp_f32<0xB1>(a2); // lane ^ 1
                        const bool odd = t_ & 1, hi = t_ & 2;
                        const float c0 = odd ? x0 : a0, c1 = odd ? a1 : x1, c2 = odd ? x2 : a2, c3 = odd ? a3 : x3;
                        const float z0 = dpp_f32<0x4E>(c2), z1 = dpp_f32<0x4E>(c3), z2 = dpp_f32<0x4E>(c0), z3 = dpp_f32<0x4E>(c1); // lane ^ 2
                        o4[0][r] = hi ? z0 : c0; o4[1][r] = hi ? z1 : c1; o4[2][r] = hi ? c2 : z2; o4[3][r] = hi ? c3 : z3;
                    }
                    const size_t ob = (size_t)co * plane * 16 + (size_t)dy * ((size_t)p.Wout * 4);
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (kok[k]) st4(ob + ko[k], o4[k]);
                }
            }
        }
        if (pok && !up4_done) {
            // the row-dependent addresses and biases are lane constants: without this the compiler hoists all of
            // them out of the item loop and spills them around the MFMA loop; recomputing per item is ~free
            int kq_e = kq;
            asm volatile("" : "+v"(kq_e));
            // pixel-shuffle epilogues: pxb is a multiple of 4, so with Wout % 4 == 0 (workgroup-uniform test; every map of
            // the shipped configurations) the lane's 4 pixels lie in one row and one division per item does
            const bool row4 = (p.Wout & 3) == 0;
            const int py_ = pxb / p.Wout, px_ = pxb - py_ * p.Wout;
            (void)row4; (void)py_; (void)px_;
#pragma unroll
            for (int i = 0; i < MT; ++i) {
                const int row0 = co0 + i * 16 + kq_e * 4;
                if (row0 >= p.Cout) continue;
                if (EPI == EPI_PLAIN) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const f32x4 x = (f32x4){acc[i][0][r], acc[i][1][r], acc[i][2][r], acc[i][3][r]};
                        st4((size_t)(row0 + r) * plane + pxb, x);
                        ssum[i][r] += (x[0] + x[1]) + (x[2] + x[3]);
                        ssq[i][r] += (x[0] * x[0] + x[1] * x[1]) + (x[2] * x[2] + x[3] * x[3]);
                    }
                } else if (EPI == EPI_UP2) {
                    const int co = row0 >> 2;
                    const size_t W2 = (size_t)p.Wout * 2;
                    if (row4) {
                        // the lane's 4 pixels are 8 consecutive floats of output rows 2y and 2y+1: two dwordx4 per row,
                        // 512 contiguous bytes per 16 lanes (the per-pixel float2 stores left 8 of every 32 bytes per instruction)
                        const size_t o = (size_t)co * plane * 4 + (size_t)(2 * py_) * W2 + 2 * px_;
                        st4(o, (f32x4){acc[i][0][0], acc[i][0][1], acc[i][1][0], acc[i][1][1]});
                        st4(o + 4, (f32x4){acc[i][2][0], acc[i][2][1], acc[i][3][0], acc[i][3][1]});
                        st4(o + W2, (f32x4){acc[i][0][2], acc[i][0][3], acc[i][1][2], acc[i][1][3]});
                        st4(o + W2 + 4, (f32x4){acc[i][2][2], acc[i][2][3], acc[i][3][2], acc[i][3][3]});
#pragma unroll
                        for (int j = 0; j < NT; ++j)
#pragma unroll
                            for (int r = 0; r < 4; ++r) { ssum[i][0] += acc[i][j][r]; ssq[i][0] += acc[i][j][r] * acc[i][j][r]; }
                    } else {
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            const int y = (pxb + j) / p.Wout, xx = (pxb + j) - y * p.Wout;
                            const f32x4 v = acc[i][j];
                            float* o = gout + (size_t)co * plane * 4 + (size_t)(2 * y) * W2 + 2 * xx;
                            *reinterpret_cast<float2*>(o) = make_float2(v[0], v[1]);
                            *reinterpret_cast<float2*>(o + W2) = make_float2(v[2], v[3]);
#pragma unroll
                            for (int r = 0; r < 4; ++r) { ssum[i][0] += v[r]; ssq[i][0] += v[r] * v[r]; }
                        }
                    }
                } else if (EPI == EPI_UP4) {
                    const int co = row0 >> 4, dy = (row0 >> 2) & 3;
                    const size_t W4o = (size_t)p.Wout * 4;
#pragma unroll
                    for (int j = 0; j < NT; ++j) {
                        const int y = row4 ? py_ : (pxb + j) / p.Wout, xx = row4 ? px_ + j : (pxb + j) - y * p.Wout;
                        const f32x4 v = acc[i][j];
                        float* o = gout + (size_t)co * plane * 16 + (size_t)(4 * y + dy) * W4o + 4 * xx;
                        *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll
                        for (int r = 0; r < 4; ++r) { ssum[i][0] += v[r]; ssq[i][0] += v[r] * v[r]; }
                    }
                } else if (EPI == EPI_HEAD_CLS) { // row = anchor: cls(a) over the lane's 4 pixels, as the full head stores it
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int a_ = row0 + r;
                        if (a_ < p.n_cls) {
                            const float bs = p.bias[4 * (9 + a_) + 3];
                            *reinterpret_cast<f32x4*>(gout + (size_t)a_ * plane + pxb) =
                                (f32x4){acc[i][0][r] + bs, acc[i][1][r] + bs, acc[i][2][r] + bs, acc[i][3][r] + bs};
                        }
                    }
                } else {
                    // head rows in head_tile_row order: this lane's 4 rows are one output run (see the host helper)
                    const int g = row0 >> 2;
                    const f32x4 bs = *reinterpret_cast<const f32x4*>(p.bias + row0);
                    if (g < 9) { // box(a = g), k = 0..3
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            f32x4u* o = reinterpret_cast<f32x4u*>(gbox + ((size_t)g * plane + pxb + j) * 7);
                            *o = (f32x4u){acc[i][j][0] + bs[0], acc[i][j][1] + bs[1], acc[i][j][2] + bs[2], acc[i][j][3] + bs[3]};
                        }
                    } else if (g < 18) { // box(a = g - 9), k = 4..6 ; cls(a) over the lane's 4 pixels
                        const int a_ = g - 9;
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            float* o = gbox + ((size_t)a_ * plane + pxb + j) * 7 + 4;
                            *reinterpret_cast<f32x2u*>(o) = (f32x2u){acc[i][j][0] + bs[0], acc[i][j][1] + bs[1]};
                            o[2] = acc[i][j][2] + bs[2];
                        }
                        *reinterpret_cast<f32x4*>(gout + (size_t)a_ * plane + pxb) =
                            (f32x4){acc[i][0][3] + bs[3], acc[i][1][3] + bs[3], acc[i][2][3] + bs[3], acc[i][3][3] + bs[3]};
                    } else if (g < 23) { // dir(a0 = 2d), dir(a0 + 1)
                        const int a0 = 2 * (g - 18);
#pragma unroll
                        for (int j = 0; j < NT; ++j) {
                            *reinterpret_cast<float2*>(gdir + ((size_t)a0 * plane + pxb + j) * 2) = make_float2(acc[i][j][0] + bs[0], acc[i][j][1] + bs[1]);
                            if (a0 + 1 < 9)
                                *reinterpret_cast<float2*>(gdir + ((size_t)(a0 + 1) * plane + pxb + j) * 2) = make_float2(acc[i][j][2] + bs[2], acc[i][j][3] + bs[3]);
                        }
                    }
                }
            }
        }
    }
    flush_stats(stat_frame);
#undef G1_MFMAS
#undef G1_PREP
#undef G1_LOADB
}

template <int MT, int NT, int EPI, int PREC = 0, int IO16 = 0>
Variant make_g1()
{
    Variant v;
    v.kern = gemm1x1<MT, NT, EPI, PREC, IO16>;
    v.prec = PREC;
    v.io16 = IO16;
    v.bm = MT * 16; v.bmp = v.bm + ((v.bm % 32 == 0) ? 16 : 0); v.pw = NT * 16; v.ph = 1; v.kc = 4; v.threads = 512;
    v.waves = 8; v.pairs = MT * NT;
    v.lds = 0; // depends on K: set per layer
    v.family = Family::Gemm1x1;
    if (IO16) snprintf(v.name, sizeof(v.name), "g1x1 m%d n%d e%d h%d p%d", MT, NT, EPI, IO16, PREC);
    else if (PREC) snprintf(v.name, sizeof(v.name), "g1x1 m%d n%d e%d p%d", MT, NT, EPI, PREC);
    else snprintf(v.name, sizeof(v.name), "g1x1 m%d n%d e%d", MT, NT, EPI);
    return v;
}

// cls-only head pass (EPI_HEAD_CLS): ring depth PD, two workgroups per CU
template <int PD>
Variant make_g1_cls()
{
    Variant v;
    v.kern = gemm1x1<1, 4, EPI_HEAD_CLS, 0, 0, PD>;
    v.bm = 16; v.bmp = 16; v.pw = 64; v.ph = 1; v.kc = 4; v.threads = 512;
    v.waves = 8; v.pairs = 4;
    v.lds = 0; // depends on K (g1_lds)
    v.family = Family::Gemm1x1;
    v.wpc = 2;
    snprintf(v.name, sizeof(v.name), "g1x1 cls pd%d wg%d", PD, v.wpc);
    return v;
}

// S16 (pp_set_precision 4): every activation tensor behind the first conv is stored in fp16 -- the upsamplers read fp16 block
// outputs and write the fp16 concat buffer (io16 3), the head reads it (io16 1; its logits stay fp32)
template <int PREC, bool S16 = false>
void lp_menu(int kind, int up, std::vector<Variant>& menu)
{
    constexpr int HI = S16 ? 1 : 0, DO = S16 ? 3 : 0;
    if (kind == 2) { menu.push_back(make_g1<6, 4, EPI_HEAD, PREC, HI>()); menu.push_back(make_g1<3, 4, EPI_HEAD, PREC, HI>()); }
    else if (up == 1) { menu.push_back(make_g1<4, 4, EPI_PLAIN, PREC, DO>()); menu.push_back(make_g1<2, 4, EPI_PLAIN, PREC, DO>()); }
    else if (up == 2) { menu.push_back(make_g1<4, 4, EPI_UP2, PREC, DO>()); menu.push_back(make_g1<8, 4, EPI_UP2, PREC, DO>()); }
    else { menu.push_back(make_g1<4, 4, EPI_UP4, PREC, DO>()); menu.push_back(make_g1<8, 4, EPI_UP4, PREC, DO>()); }
}

} // namespace

namespace ppc {

// kind 2: the two head tilings; kind 1: the two tilings of the ConvTranspose(k = s = up) upsampler.  prec as pp_set_precision: 0 fp32,
// 1 bf16x3, 2 bf16, 3 fp16 operands, 4 fp16 operands on fp16 tensors
void gemm1x1_menu(int kind, int up, int prec, std::vector<Variant>& menu)
{
    switch (prec) {
    case 0: lp_menu<0>(kind, up, menu); break;
    case 1: lp_menu<1>(kind, up, menu); break;
    case 2: lp_menu<2>(kind, up, menu); break;
    case 3: lp_menu<3>(kind, up, menu); break;
    default: lp_menu<3, true>(kind, up, menu); break;
    }
}
// shapes of the cls-only head pass -- every shape without scratch: a 16-deep ring spills
void gemm1x1_cls_menu(std::vector<Variant>& menu)
{
    menu.push_back(make_g1_cls<8>());
    menu.push_back(make_g1_cls<10>());
    menu.push_back(make_g1_cls<4>());
}
// LDS bytes of a persistent 1x1 GEMM for a given K
size_t g1_lds(const Variant& v, int K) { return ((size_t)K * v.bmp + (size_t)8 * 2 * K) * sizeof(float); }

// Row order of the head inside gemm1x1.  A lane of the 16x16 MFMA tile owns 4 CONSECUTIVE tile rows (kq*4 + r), so
// the 90 head rows are dealt to the 24 four-row groups such that a group's values are adjacent in the output:
//   groups 0..8   box (a = g)      k = 0..3                      -> one 16-byte store per pixel
//   groups 9..17  box (a = g - 9)  k = 4..6, then cls(a)         -> one 12-byte store per pixel + cls as a pixel quad
//   groups 18..22 dir (a = 2d, 2d+1), both logits each           -> two 8-byte stores per pixel
//   group 23      padding
// (natural order: cls 0..8, box 9 + 7a + k, dir 72 + 2a + k, head rows 90..95 are zero).  With the natural order
// the 81 box/dir rows cost 4 scalar stores each per lane -- 333 scattered store instructions per 64 pixels, whose
// completion the next item's first loads had to wait for (vmcnt is in order): 38 % of the head's wave time.
int head_tile_row(int t)
{
    const int g = t >> 2, r = t & 3;
    if (g < 9) return 9 + 7 * g + r;
    if (g < 18) return r < 3 ? 9 + 7 * (g - 9) + 4 + r : (g - 9);
    if (g < 23) {
        const int a = 2 * (g - 18) + (r >> 1);
        return a < 9 ? 72 + 2 * a + (r & 1) : -1;
    }
    return -1;
}
// head under gemm1x1: rows in head_tile_row order
void gemm1x1_head_order(std::vector<float>& w, int cin)
{
    std::vector<float> perm((size_t)96 * cin, 0.f);
    for (int t = 0; t < 96; ++t) {
        const int src = head_tile_row(t);
        if (src >= 0) memcpy(&perm[(size_t)t * cin], &w[(size_t)src * cin], sizeof(float) * cin);
    }
    w.swap(perm);
}
// fp32 image: [row block][K][BMP], the weight slab a workgroup keeps resident, zero in the row padding
void gemm1x1_pack(const std::vector<float>& w, int rows, int cin, const Variant& v, std::vector<float>& out)
{
    const int nb_ = pp_div_up(rows, v.bm);
    out.assign((size_t)nb_ * cin * v.bmp, 0.f);
    for (int b = 0; b < nb_; ++b)
        for (int c = 0; c < cin; ++c)
            for (int mm = 0; mm < v.bm; ++mm) {
                const int row = b * v.bm + mm;
                if (row < rows) out[((size_t)b * cin + c) * v.bmp + mm] = w[(size_t)row * cin + c];
            }
}
// 16-bit operand image: [row block][K/16][hi|lo][k-group][BMP][4 bf16]: the byte count of the fp32 slab
void gemm1x1_pack16(const std::vector<float>& w, int rows, int cin, const Variant& v, std::vector<uint16_t>& out)
{
    const int nb_ = pp_div_up(rows, v.bm), nkb = cin / 16;
    out.assign((size_t)nb_ * nkb * 2 * 4 * v.bmp * 4, 0);
    for (int b = 0; b < nb_; ++b)
        for (int kb = 0; kb < nkb; ++kb)
            for (int q = 0; q < 4; ++q)
                for (int mm = 0; mm < v.bm; ++mm) {
                    const int row = b * v.bm + mm;
                    if (row >= rows) continue;
                    for (int t = 0; t < 4; ++t) {
                        const float x = w[(size_t)row * cin + kb * 16 + q * 4 + t];
                        uint16_t hi = to_bf16(x);
                        if (v.prec == 3) { const _Float16 h16 = (_Float16)x; memcpy(&hi, &h16, 2); } // fp16 operands: the hi image alone is used
                        const uint16_t lo = to_bf16(x - from_bf16(hi));
                        out[(((((size_t)b * nkb + kb) * 2 + 0) * 4 + q) * v.bmp + mm) * 4 + t] = hi;
                        out[(((((size_t)b * nkb + kb) * 2 + 1) * 4 + q) * v.bmp + mm) * 4 + t] = lo;
                    }
                }
}

} // namespace ppc
