// wino4_mfma: Winograd F(2x2,3x3) re-structured around ONE wave per SIMD with the whole 512-register file.
// What the counters said about wino_mfma (profiles/r01_pmc_sq_waits_and_mix.txt): 3.4 VALU + 1.1 LDS instructions
// per MFMA, two waves per SIMD waiting on each other for issue (53 % of wave time), the matrix pipe 50 % busy;
// the non-MFMA phases (chunk opening, epilogue) of two independent workgroups overlap only by chance.  Here:
//  * MT = 4: a wave owns 16 tiles x ALL 64 output channels of the block (256 accumulator registers = the AGPR half).
//    Each transformed B operand now feeds 4 MFMAs instead of 2, each A fetch is one ds_read_b128 for 4 MFMAs: per MFMA
//    the transform VALU, the LDS reads and the staging work all halve, and a 64-channel layer transforms its
//    input ONCE instead of once per 32-row block.
//  * a THREE-deep LDS ring (input patch + weight image per channel chunk): chunk g+2 is written while chunk g is
//    multiplied, so chunk g+1 is complete one barrier EARLIER than it is needed and its first operands (raw patch,
//    A fragments, column pass) are fetched during the last steps of chunk g.  The MFMA stream runs across chunk
//    boundaries without the opening bubble (LDS round trip -> normalise -> column pass -> first MFMA) that cost
//    wino_mfma ~1 k of every ~7 k cycles; the one barrier per chunk has nothing waiting right behind it.
//  * the staging pipeline runs across TILE boundaries too: the load side simply walks the (item, chunk) stream two
//    chunks ahead of the compute side, whatever tile that is.
//  * InstanceNorm (scale, shift) of the staged chunk come through the scalar cache (wave-uniform address), not LDS.
//  * the statistics' cross-wave reduction is deferred behind the next tile's first chunk barrier: no extra barrier.
// One workgroup (4 waves) per CU, persistent over the (cout block, tile, frame) list like wino_mfma.
#include <cstdio>
#include "pp_common.h"
#include "conv_common.h"

namespace {

using namespace ppc;

// The 256 accumulator registers of wino4_mfma are NOT C++ values: its MFMAs name a[0:255] literally.  Handing hipcc 64 live
// accumulator quads next to ~130 asm statements per chunk ends in accumulators scattered over both register halves, AGPR
// permutations at the loop edge and scratch spills of just-loaded operands; with the accumulators out of its sight it
// allocates < 256 plain VGPRs and nothing else.  Every such statement clobbers the whole AGPR half, so the compiler can never
// park a value there (audit: no v_accvgpr_* outside these statements in the ISA, tools/isa_stats.py).
#define W4_A10(b) "a" #b "0", "a" #b "1", "a" #b "2", "a" #b "3", "a" #b "4", "a" #b "5", "a" #b "6", "a" #b "7", "a" #b "8", "a" #b "9"
#define W4_A100(h) W4_A10(h##0), W4_A10(h##1), W4_A10(h##2), W4_A10(h##3), W4_A10(h##4), W4_A10(h##5), W4_A10(h##6), W4_A10(h##7), W4_A10(h##8), W4_A10(h##9)
#define W4_AGPRS "a0", "a1", "a2", "a3", "a4", "a5", "a6", "a7", "a8", "a9", W4_A10(1), W4_A10(2), W4_A10(3), W4_A10(4), W4_A10(5), W4_A10(6), W4_A10(7), W4_A10(8), W4_A10(9), \
                 W4_A100(1), W4_A10(20), W4_A10(21), W4_A10(22), W4_A10(23), W4_A10(24), "a250", "a251", "a252", "a253", "a254", "a255"
// the 16 Winograd positions of (M-tile I, accumulator row R) in ONE statement: hipcc pads every asm boundary with an s_nop
// before a VALU may touch its outputs -- one pad per 16 reads instead of one per read
template <int I, int R>
__device__ __forceinline__ void w4_acc_read16(float (&v)[16])
{
    asm volatile("v_accvgpr_read_b32 %0, a%c16\n\tv_accvgpr_read_b32 %1, a%c17\n\tv_accvgpr_read_b32 %2, a%c18\n\tv_accvgpr_read_b32 %3, a%c19\n\t"
                 "v_accvgpr_read_b32 %4, a%c20\n\tv_accvgpr_read_b32 %5, a%c21\n\tv_accvgpr_read_b32 %6, a%c22\n\tv_accvgpr_read_b32 %7, a%c23\n\t"
                 "v_accvgpr_read_b32 %8, a%c24\n\tv_accvgpr_read_b32 %9, a%c25\n\tv_accvgpr_read_b32 %10, a%c26\n\tv_accvgpr_read_b32 %11, a%c27\n\t"
                 "v_accvgpr_read_b32 %12, a%c28\n\tv_accvgpr_read_b32 %13, a%c29\n\tv_accvgpr_read_b32 %14, a%c30\n\tv_accvgpr_read_b32 %15, a%c31"
                 : "=v"(v[0]), "=v"(v[1]), "=v"(v[2]), "=v"(v[3]), "=v"(v[4]), "=v"(v[5]), "=v"(v[6]), "=v"(v[7]), "=v"(v[8]), "=v"(v[9]),
                   "=v"(v[10]), "=v"(v[11]), "=v"(v[12]), "=v"(v[13]), "=v"(v[14]), "=v"(v[15])
                 : "i"((0 * 4 + I) * 4 + R), "i"((1 * 4 + I) * 4 + R), "i"((2 * 4 + I) * 4 + R), "i"((3 * 4 + I) * 4 + R), "i"((4 * 4 + I) * 4 + R),
                   "i"((5 * 4 + I) * 4 + R), "i"((6 * 4 + I) * 4 + R), "i"((7 * 4 + I) * 4 + R), "i"((8 * 4 + I) * 4 + R), "i"((9 * 4 + I) * 4 + R),
                   "i"((10 * 4 + I) * 4 + R), "i"((11 * 4 + I) * 4 + R), "i"((12 * 4 + I) * 4 + R), "i"((13 * 4 + I) * 4 + R), "i"((14 * 4 + I) * 4 + R),
                   "i"((15 * 4 + I) * 4 + R)
                 : W4_AGPRS);
}

// rows R and R + 1 (R even) of M-tile I at the 16 Winograd positions, as 16 (row R, row R + 1) pairs for v_pk_* arithmetic:
// position xi's quad starts at a[xi*16 + I*4]
template <int I, int R>
__device__ __forceinline__ void w4_acc_read32(float __attribute__((ext_vector_type(2))) (&v)[16])
{
    float l[16], u[16];
    // operands %0..%15 = row R at position 0..15, %16..%31 = row R + 1 (operand numbers are spelled out: %1K would be ambiguous)
    asm volatile("v_accvgpr_read_b32 %0, a[%c32+0]\n\tv_accvgpr_read_b32 %16, a[%c32+1]\n\t"
                 "v_accvgpr_read_b32 %1, a[%c32+16]\n\tv_accvgpr_read_b32 %17, a[%c32+17]\n\t"
                 "v_accvgpr_read_b32 %2, a[%c32+32]\n\tv_accvgpr_read_b32 %18, a[%c32+33]\n\t"
                 "v_accvgpr_read_b32 %3, a[%c32+48]\n\tv_accvgpr_read_b32 %19, a[%c32+49]\n\t"
                 "v_accvgpr_read_b32 %4, a[%c32+64]\n\tv_accvgpr_read_b32 %20, a[%c32+65]\n\t"
                 "v_accvgpr_read_b32 %5, a[%c32+80]\n\tv_accvgpr_read_b32 %21, a[%c32+81]\n\t"
                 "v_accvgpr_read_b32 %6, a[%c32+96]\n\tv_accvgpr_read_b32 %22, a[%c32+97]\n\t"
                 "v_accvgpr_read_b32 %7, a[%c32+112]\n\tv_accvgpr_read_b32 %23, a[%c32+113]\n\t"
                 "v_accvgpr_read_b32 %8, a[%c32+128]\n\tv_accvgpr_read_b32 %24, a[%c32+129]\n\t"
                 "v_accvgpr_read_b32 %9, a[%c32+144]\n\tv_accvgpr_read_b32 %25, a[%c32+145]\n\t"
                 "v_accvgpr_read_b32 %10, a[%c32+160]\n\tv_accvgpr_read_b32 %26, a[%c32+161]\n\t"
                 "v_accvgpr_read_b32 %11, a[%c32+176]\n\tv_accvgpr_read_b32 %27, a[%c32+177]\n\t"
                 "v_accvgpr_read_b32 %12, a[%c32+192]\n\tv_accvgpr_read_b32 %28, a[%c32+193]\n\t"
                 "v_accvgpr_read_b32 %13, a[%c32+208]\n\tv_accvgpr_read_b32 %29, a[%c32+209]\n\t"
                 "v_accvgpr_read_b32 %14, a[%c32+224]\n\tv_accvgpr_read_b32 %30, a[%c32+225]\n\t"
                 "v_accvgpr_read_b32 %15, a[%c32+240]\n\tv_accvgpr_read_b32 %31, a[%c32+241]"
                 : "=v"(l[0]), "=v"(l[1]), "=v"(l[2]), "=v"(l[3]), "=v"(l[4]), "=v"(l[5]), "=v"(l[6]), "=v"(l[7]), "=v"(l[8]), "=v"(l[9]), "=v"(l[10]),
                   "=v"(l[11]), "=v"(l[12]), "=v"(l[13]), "=v"(l[14]), "=v"(l[15]), "=v"(u[0]), "=v"(u[1]), "=v"(u[2]), "=v"(u[3]), "=v"(u[4]), "=v"(u[5]),
                   "=v"(u[6]), "=v"(u[7]), "=v"(u[8]), "=v"(u[9]), "=v"(u[10]), "=v"(u[11]), "=v"(u[12]), "=v"(u[13]), "=v"(u[14]), "=v"(u[15])
                 : "i"(I * 4 + R)
                 : W4_AGPRS);
#pragma unroll
    for (int k = 0; k < 16; ++k) { v[k][0] = l[k]; v[k][1] = u[k]; }
}
// Row pass of the Winograd input transform, middle positions: tb = (t1, t3), ta = (t0, t2) of one row of B^T d  ->  (t1 + t2, t2 - t1)
__device__ __forceinline__ float __attribute__((ext_vector_type(2))) w4_row_mid(float __attribute__((ext_vector_type(2))) tb, float __attribute__((ext_vector_type(2))) ta)
{
    float __attribute__((ext_vector_type(2))) r;
    asm("v_pk_add_f32 %0, %1, %2 op_sel:[0,1] op_sel_hi:[0,1] neg_hi:[1,0]" : "=v"(r) : "v"(tb), "v"(ta));
    return r;
}
// Lanes 2j (tile x) and 2j+1 (tile x+1) hold the 2x2 outputs (y0 y1 / y2 y3) of neighbouring tiles.  Returns, in the even lane,
// row y of both tiles (own y0 y1, partner's y0 y1) and in the odd lane row y+1 (partner's y2 y3, own y2 y3): v_cndmask_b32 with
// its first source permuted over DPP (quad_perm [1,0,3,2] = lane ^ 1) -- 4 VALU instead of 2 selects + 2 DPP moves + 4 selects.
// s_nop 1: a DPP source written by the VALU instruction before needs 2 wait states, and hipcc does not look inside asm.
__device__ __forceinline__ f32x4 w4_pair_rows(float y0, float y1, float y2, float y3)
{
    float v0, v1, v2, v3;
    asm volatile("s_mov_b32 vcc_lo, 0x55555555\n\ts_mov_b32 vcc_hi, 0x55555555\n\ts_nop 1\n\t"
                 "v_cndmask_b32_dpp %0, %6, %4, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_cndmask_b32_dpp %1, %7, %5, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "s_not_b64 vcc, vcc\n\t"
                 "v_cndmask_b32_dpp %2, %4, %6, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
                 "v_cndmask_b32_dpp %3, %5, %7, vcc quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
                 : "=&v"(v0), "=&v"(v1), "=&v"(v2), "=&v"(v3)
                 : "v"(y0), "v"(y1), "v"(y2), "v"(y3)
                 : "vcc", "scc");
    return (f32x4){v0, v1, v2, v3};
}

template <int TWT, int BTX, int KC>
struct Wino4Cfg {
    static constexpr int WN = 4, MT = 4;
    static constexpr int THT = 16 / TWT;
    static constexpr int BTY = WN / BTX;
    static constexpr int PW = BTX * TWT * 2, PH = BTY * THT * 2;
    static constexpr int IW = PW + 2, IH = PH + 2;
    static constexpr int HALF = (IW + 1) / 2;
    static constexpr int iwp()
    {
        int v = IW;
        if (TWT == 16) return v;
        if (TWT == 2 && BTX == 1) return 6; // 4 x 64 strip tile: rows 12 banks apart (0,12,24,4,...) keep a wave's 8 tile rows on distinct banks
        while ((2 * v) % 32 != TWT) ++v;
        return v;
    }
    static constexpr int IWP = iwp();
    static constexpr int cs()
    {
        int v = IH * IWP;
        while (v % 32 != 16) ++v;
        return v;
    }
    static constexpr int CS = cs();
    static constexpr int BM = 64;  // rows per block = MT * 16; A image row = [m 0..15][M-tile 0..3]: one ds_read_b128 per lane, the
                                   // 64 lanes of a step read 1 KB contiguous (kq*64 + m*4 floats) -- conflict-free without padding
    static constexpr int THREADS = 256;
    static constexpr int NPOS = IH * IW;
    static constexpr int PR = (NPOS + THREADS - 1) / THREADS;
    static constexpr int W4 = 16 * KC * BM / 4;
    static constexpr int WR = (W4 + THREADS - 1) / THREADS;
    static constexpr int LDS_IN = KC * CS;
    static constexpr int LDS_W = 16 * KC * BM;
    static constexpr int NSTAGE = 3;
    static constexpr int LDS_FLOATS = NSTAGE * (LDS_IN + LDS_W) + 2 * WN * BM + 2 * 640;
    static_assert(LDS_FLOATS * 4 <= 160 * 1024, "must fit the 160 KB LDS");
    static_assert(WN % BTX == 0, "tiles must form a rectangle");
    static_assert(KC == 8, "the step schedule assumes two channel quads per chunk (tq parity, A ring)");
    static_assert(W4 % THREADS == 0, "weight image is a whole number of float4 per thread");
};

template <int TWT, int BTX, int KC, int ROOFLINE = 0>
__global__ void __launch_bounds__(256, 1) wino4_mfma(const ConvP p)
{
    using C = Wino4Cfg<TWT, BTX, KC>;
    constexpr int WN = 4;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* il = smem;                               // [3][KC][CS]
    float* wl = il + C::NSTAGE * C::LDS_IN;         // [3][16][KC][64]
    float* red = wl + C::NSTAGE * C::LDS_W;         // [WN][BM][2]
    float* aff = red + 2 * WN * C::BM;              // [2 frame parities][2: scale, shift][320]
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wn = tid >> 6;
    const int m = lane & 15, kq = lane >> 4;

    const int nbx = p.rnbx, nby = p.rnby; // tiles of this launch's region [rx0, rx1) x [ry0, ry1)
    const int ntile = nbx * nby, ncb = (p.Cout + C::BM - 1) / C::BM;
    const int total = ntile * ncb * p.nb;
    const int per = (total + 7) >> 3;
    const int xk = blockIdx.x & 7, xj = blockIdx.x >> 3, nloc = gridDim.x >> 3;
    const int lin_end = min(total, (xk + 1) * per);
    const int lin0 = xk * per + xj;
    if (lin0 >= lin_end) return;
    const int nchunk = p.Cin / KC;

    // ---------------- load side: walks the (item, chunk) stream two chunks ahead of the compute side ----------------
    int goff[C::PR], loff[C::PR];
    unsigned vmask = 0u;
    __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, 0x7FFFFFFF, 0x00020000);
    const unsigned plane_b = (unsigned)(p.Hin * p.Win) * 4u;
    unsigned wbase_b = 0u;
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    f32x2 xv[C::PR][KC / 2]; // staging registers: channel pairs (2k, 2k+1), so one v_pk_fma_f32 normalises two pieces
    f32x4 wv[C::WR];
#pragma unroll
    for (int r = 0; r < C::PR; ++r) {
        const int pos = min(tid + r * C::THREADS, C::NPOS - 1); // tail threads duplicate the last position: unconditional staging
        const int iy = pos / C::IW, ix = pos - iy * C::IW;
        loff[r] = iy * C::IWP + (ix & 1) * C::HALF + (ix >> 1);
    }
    int s_lin = lin0, s_ch = 0, s_frame = 0; // chunk the NEXT load request is for, and its frame
    int r_c0 = 0;                            // first channel of the chunk held in the registers (its table slot: r_tab)
    unsigned r_vmask = 0u;
    auto set_load_tile = [&](int l) {
        const int cb_ = l % ncb, t_ = (l / ncb) % ntile, f_ = l / (ncb * ntile);
        const int iy0_ = p.ry0 + (t_ / nbx) * C::PH - 1, ix0_ = p.rx0 + (t_ % nbx) * C::PW - 1;
        vmask = 0u;
#pragma unroll
        for (int r = 0; r < C::PR; ++r) {
            const int pos = min(tid + r * C::THREADS, C::NPOS - 1);
            const int iy = pos / C::IW, ix = pos - iy * C::IW;
            const int gy = iy0_ + iy, gx = ix0_ + ix;
            const bool inb = gy >= 0 && gy < p.Hin && gx >= 0 && gx < p.Win;
            goff[r] = inb ? (gy * p.Win + gx) * 4 : 0;
            vmask |= (inb ? 1u : 0u) << r;
        }
        rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in + (size_t)f_ * p.in_fs), 0, 0x7FFFFFFF, 0x00020000);
        wbase_b = (unsigned)((size_t)cb_ * nchunk * C::W4 * 16);
        s_frame = f_;
    };
    // The load side: advance() -- uniform branches, possibly a new tile's offsets and a new frame's (scale, shift) table --
    // runs at the top of a chunk, outside the MFMA stream (a branch between MFMA steps makes hipcc shuffle accumulators);
    // the requests themselves are spread over the chunk's steps, each right behind the LDS write that frees its register, so
    // every load has a whole chunk (> 4 k cycles) to land.  Past the end of this workgroup's list the load side stays on its
    // last chunk (harmless duplicates into ring slots nobody reads; every request stays inside the tensors).
    // (scale, shift) of the producer's normalisation live in LDS in TWO table slots: the load side may already be in another
    // frame while older chunks are still being normalised.  A frame change of the load side flips the slot, writes the new
    // frame's table there, and the chunk barrier that follows publishes it (that slot's previous table belongs to a frame
    // whose last chunk was normalised at least a whole tile ago).
    int s_tab = 0, r_tab = 0;
    auto load_aff = [&](int f_) {
        float* dst = aff + s_tab * 640;
        if (p.pre == PRE_STATS) {
            // one-frame launches (launch_conv, B == 1): the producer's fp64 sums are finalised HERE, once per workgroup, instead of by a
            // norm_finalize launch in front of every layer (4.7 us + a launch boundary each, 14 per frame at batch 1) -- same fp64
            // formula, bit-identical (scale, shift)
            const double* pa = p.pre_acc + (size_t)f_ * p.pre_fs;
            for (int c = tid; c < p.Cin; c += C::THREADS) {
                double s = 0.0, q = 0.0;
#pragma unroll
                for (int r = 0; r < NREP; ++r) { s += pa[((size_t)r * p.Cin + c) * 2]; q += pa[((size_t)r * p.Cin + c) * 2 + 1]; }
                const double mean = s * p.pre_inv_n;
                double var = q * p.pre_inv_n - mean * mean;
                var = var > 0.0 ? var : 0.0;
                const double rstd = 1.0 / sqrt(var + (double)p.eps);
                dst[c] = (float)rstd;
                dst[320 + c] = (float)(-mean * rstd);
            }
            return;
        }
        for (int c = tid; c < p.Cin; c += C::THREADS) {
            dst[c] = p.pre_scale[(size_t)f_ * p.aff_fs + c];
            dst[320 + c] = p.pre_shift[(size_t)f_ * p.aff_fs + c];
        }
    };
    auto advance = [&]() {
        if (s_ch + 1 < nchunk) ++s_ch;
        else if (s_lin + nloc < lin_end) {
            const int f_old = s_frame;
            s_lin += nloc; s_ch = 0; set_load_tile(s_lin);
            if (s_frame != f_old) { s_tab ^= 1; load_aff(s_frame); }
        }
    };
// request piece E of chunk (s_lin, s_ch) into its register
#define W4_LOAD_PIECE(E)                                                                         \
    {                                                                                            \
        if constexpr ((E) < C::PR * KC) {                                                        \
            constexpr int r_ = (E) / KC, c_ = (E) % KC;                                          \
            xv[r_][c_ / 2][c_ & 1] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, goff[r_], (unsigned)(s_ch * KC + c_) * plane_b, 0)); \
        } else if constexpr ((E) < C::PR * KC + C::WR) {                                         \
            constexpr int r_ = (E) - C::PR * KC;                                                 \
            wv[r_] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (tid + r_ * C::THREADS) * 16, wbase_b + (unsigned)s_ch * (C::W4 * 16), 0)); \
        }                                                                                        \
    }
// normalise + ReLU + zero padding of input pieces E, E+1 (E even: one channel pair) in place.  SC/SH: this chunk's KC scales /
// shifts, MASK: upper clamp per position (+inf inside the image = plain ReLU, 0 on the zero padding) -- v_pk_fma_f32 + 2 v_med3_f32
#define W4_NORM_PAIR(E, SC, SH, MASK)                                                            \
    {                                                                                            \
        if constexpr ((E) < C::PR * KC && (E) % 2 == 0) {                                        \
            constexpr int r_ = (E) / KC, c_ = (E) % KC;                                          \
            const f32x2 t_ = __builtin_elementwise_fma(xv[r_][c_ / 2], (f32x2){SC[c_], SC[c_ + 1]}, (f32x2){SH[c_], SH[c_ + 1]}); \
            xv[r_][c_ / 2][0] = __builtin_amdgcn_fmed3f(t_[0], 0.f, MASK[r_]);                   \
            xv[r_][c_ / 2][1] = __builtin_amdgcn_fmed3f(t_[1], 0.f, MASK[r_]);                   \
        }                                                                                        \
    }
#define W4_READ_AFF(SC, SH, TAB, C0)                                                             \
    {                                                                                            \
        const float* t_ = aff + (TAB) * 640 + (C0);                                              \
        _Pragma("unroll") for (int c = 0; c < KC; c += 4) {                                      \
            const f32x4 a_ = *reinterpret_cast<const f32x4*>(t_ + c);                            \
            const f32x4 b_ = *reinterpret_cast<const f32x4*>(t_ + 320 + c);                      \
            _Pragma("unroll") for (int q = 0; q < 4; ++q) { SC[c + q] = a_[q]; SH[c + q] = b_[q]; } \
        }                                                                                        \
    }
#define W4_WRITE_PIECE(E, IB, WB)                                                                \
    {                                                                                            \
        if constexpr ((E) < C::PR * KC) {                                                        \
            constexpr int r_ = (E) / KC, c_ = (E) % KC;                                          \
            (IB)[c_ * C::CS + loff[r_]] = xv[r_][c_ / 2][c_ & 1];                                \
        } else if constexpr ((E) < C::PR * KC + C::WR) {                                         \
            constexpr int r_ = (E) - C::PR * KC;                                                 \
            reinterpret_cast<f32x4*>(WB)[tid + r_ * C::THREADS] = wv[r_];                        \
        }                                                                                        \
    }
// one row (4 values) of the raw 4x4 patch of the quad whose element index inside the ring is QB.  QB is made opaque once per
// quad: otherwise hipcc folds the quad's offset into every row address and spends a v_add per ds_read2 on constants that no
// longer fit the instruction's 8-bit offsets (the row offsets alone do: <= 3*IWP + HALF + 1 dwords)
#define W4_READ_RAW_ROW(DST, QB, I)                                                              \
    {                                                                                            \
        DST[(I) * 2] = (f32x2){il[(QB) + (I) * C::IWP], il[(QB) + (I) * C::IWP + 1]};            \
        DST[(I) * 2 + 1] = (f32x2){il[(QB) + (I) * C::IWP + C::HALF], il[(QB) + (I) * C::IWP + C::HALF + 1]}; \
    }
// Input transform V = B^T d B on column PAIRS: the patch rows sit in LDS with even and odd columns de-interleaved, so a row is
// two ds_read2_b32 = the register pairs (d0, d2) and (d1, d3).  Packed arithmetic because a lone wave pays 4 cycles per VALU
// instruction, MFMA shadow or not (tools/issue_probe.hip).
// column pass, term K2 = 2*row + pair of T = B^T d (rows of pairs TA = (t0, t2), TB = (t1, t3)):
#define W4_COLPASS2(T, D, K2)                                                                    \
    {                                                                                            \
        constexpr int a_ = (K2) / 2, h_ = (K2) % 2;                                              \
        if constexpr (a_ == 0) T[0 + h_] = D[0 + h_] - D[4 + h_];                                \
        else if constexpr (a_ == 1) T[2 + h_] = D[2 + h_] + D[4 + h_];                           \
        else if constexpr (a_ == 2) T[4 + h_] = D[4 + h_] - D[2 + h_];                           \
        else T[6 + h_] = D[2 + h_] - D[6 + h_];                                                  \
    }
// row pass of patch row A: the B operands of steps 4A .. 4A+3 = t0 - t2 | (t1 + t2, t2 - t1) in one v_pk_add_f32 | t1 - t3
#define W4_ROW_ALL(T, A)                                                                         \
    {                                                                                            \
        o0[(A) & 1] = T[((A) & 3) * 2][0] - T[((A) & 3) * 2][1];                                 \
        p12[(A) & 1] = w4_row_mid(T[((A) & 3) * 2 + 1], T[((A) & 3) * 2]);                       \
        o3[(A) & 1] = T[((A) & 3) * 2 + 1][0] - T[((A) & 3) * 2 + 1][1];                         \
    }

    constexpr int NQ = KC / 4;                // 2
    constexpr int NSTEP = NQ * 16;            // 32 steps of 4 MFMAs
    constexpr int AD = 4;                     // A fragments in flight (3 steps = 384 matrix-pipe cycles ahead); NSTEP % AD == 0
    constexpr int NPIECE = C::PR * KC + C::WR;
    static_assert(NPIECE + 2 <= NSTEP, "staging does not fit the chunk's steps");

    // this lane's tile inside the block patch (constant over items) and operand bases
    const int btx = wn % BTX, bty = wn / BTX;
    const int ttx = btx * TWT + (m % TWT), tty = bty * C::THT + (m / TWT);
    const int rbase = (2 * tty) * C::IWP + ttx + kq * C::CS;
    const int aoff = kq * C::BM + m * 4;

    // ---------------- pipeline prologue: chunks 0 and 1 into ring slots 0 and 1, chunk 2 into the registers ----------------
    set_load_tile(lin0);
    load_aff(s_frame);
    __syncthreads();
    {
        float sc_[KC], sh_[KC];
        pp_steps<0, NPIECE>([&](auto E) { W4_LOAD_PIECE(decltype(E)::value) });
        W4_READ_AFF(sc_, sh_, s_tab, s_ch * KC)
        float mk_[C::PR];
#pragma unroll
        for (int r = 0; r < C::PR; ++r) mk_[r] = ((vmask >> r) & 1u) ? __builtin_inff() : 0.f;
        pp_steps<0, NPIECE>([&](auto E) { W4_NORM_PAIR(decltype(E)::value, sc_, sh_, mk_) W4_WRITE_PIECE(decltype(E)::value, il, wl) });
        advance();
        __syncthreads(); // a new frame's table (if the second chunk is already there)
        pp_steps<0, NPIECE>([&](auto E) { W4_LOAD_PIECE(decltype(E)::value) });
        W4_READ_AFF(sc_, sh_, s_tab, s_ch * KC)
#pragma unroll
        for (int r = 0; r < C::PR; ++r) mk_[r] = ((vmask >> r) & 1u) ? __builtin_inff() : 0.f;
        pp_steps<0, NPIECE>([&](auto E) { W4_NORM_PAIR(decltype(E)::value, sc_, sh_, mk_) W4_WRITE_PIECE(decltype(E)::value, il + C::LDS_IN, wl + C::LDS_W) });
        advance();
        pp_steps<0, NPIECE>([&](auto E) { W4_LOAD_PIECE(decltype(E)::value) });
        r_tab = s_tab; r_c0 = s_ch * KC; r_vmask = vmask;
    }
    __syncthreads();

    f32x2 draw[8], tq[2][8]; // raw 4x4 patch and its column pass, as column pairs [row][pair]
    f32x4 a[AD];
    float vcur;
    float o0[2], o3[2];      // B operands of the steps 4A (o0), 4A+1 / 4A+2 (p12) and 4A+3 (o3) of patch row A: slot A & 1
    f32x2 p12[2];
    // first operands of the very first chunk (later chunks get theirs during their predecessor's last steps)
    int qb = rbase;
    pp_steps<0, 4>([&](auto I) { W4_READ_RAW_ROW(draw, qb, decltype(I)::value) });
#pragma unroll
    for (int s0 = 0; s0 < AD - 1; ++s0) a[s0] = *reinterpret_cast<const f32x4*>(wl + (s0 * KC) * C::BM + aoff);
    pp_steps<0, 8>([&](auto K) { W4_COLPASS2(tq[0], draw, decltype(K)::value) });
    o0[1] = o3[1] = 0.f;
    p12[1] = (f32x2){0.f, 0.f};
    W4_ROW_ALL(tq[0], 0)

    int buf = 0;                 // ring slot of the chunk being multiplied
    bool pending = false;        // statistics of the previous tile wait in `red` for their cross-wave reduction
    double* pend_dst = nullptr;
    const size_t out_plane = (size_t)p.Hout * p.Wout;

    for (int lin = lin0; lin < lin_end; lin += nloc) {
        const int cb = lin % ncb, tile = (lin / ncb) % ntile;
        const size_t fz = lin / (ncb * ntile);
        const int co0 = cb * C::BM;
        const int ox0 = p.rx0 + (tile % nbx) * C::PW, oy0 = p.ry0 + (tile / nbx) * C::PH;
        const int opx = ox0 + 2 * ttx, opy = oy0 + 2 * tty;

        // Output / residual addressing of the epilogue (needed from the tile's LAST chunk on, which requests the first half's
        // residual rows).  Offsets cost no VALU: the lane part (row co0 + 4 kq of the frame at this lane's pixels) is the
        // instruction's VGPR offset, the (M-tile, accumulator row) part a wave-uniform multiple of the plane in its SGPR offset.
        // Lanes with nothing to store start 2 GB out -- past any frame (launch_conv refuses larger ones) -- so the descriptor
        // drops their accesses and returns zeros for their loads; a layer without a residual has a zero-record descriptor.
        constexpr unsigned W4_FAR = 0x80000000u;
        const bool x4_map = ((p.Wout | p.rx0 | p.rx1) & 3) == 0;
        const int par = m & 1;
        const bool pix_ok = (opx < p.rx1) && (opy < p.ry1); // pixels past the region's end belong to another launch (or to nobody)
        const bool two_y = opy + 1 < p.ry1;
        const unsigned plane_ob = (unsigned)out_plane * 4u;
        const unsigned rowb = (unsigned)(co0 + kq * 4) * plane_ob + (unsigned)(((size_t)opy * p.Wout + opx) * 4);
        // x4 form: even lane = row y at its own pixels, odd lane = row y+1 starting at the even partner's pixels
        const bool ok0 = x4_map ? (pix_ok && (par == 0 || two_y)) : pix_ok;
        const unsigned lb0 = ok0 ? ((x4_map && par) ? rowb + (unsigned)p.Wout * 4u - 8u : rowb) : W4_FAR;
        const unsigned lb1 = (pix_ok && two_y) ? rowb + (unsigned)p.Wout * 4u : W4_FAR; // second row of the dwordx2 form
        f32x4 rq[2][2][4]; // residual rows [half][M-tile of the half][accumulator row] (x4 form)
        auto res_desc = [&]() {
            const float* gres = p.res ? p.res + fz * p.res_fs : p.out;
            return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gres), 0, p.res ? (unsigned)((size_t)p.Cout * out_plane * 4) : 0u, 0x00020000);
        };
        auto request_res = [&](auto HALF, auto II) { // the 4 residual rows of M-tile 2h+ii: dwordx4 requests
            constexpr int h = decltype(HALF)::value, ii = decltype(II)::value;
            const __amdgpu_buffer_rsrc_t rres_ = res_desc();
#pragma unroll
            for (int r = 0; r < 4; ++r)
                rq[h][ii][r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rres_, lb0, (unsigned)((h * 2 + ii) * 16 + r) * plane_ob, 0));
        };

        // accumulator quad of (M-tile i, Winograd position xi): a[(xi*4 + i)*4 .. +3].  The tile's first 16 steps take 0 as C:
        // no zeroing pass over 256 registers; hence the chunk body exists twice (first chunk / accumulating chunks).
        auto chunk_body = [&](auto FIRST, int ch) {
            constexpr bool first_ = decltype(FIRST)::value;
            const int nbuf = buf == 2 ? 0 : buf + 1, wbuf = buf == 0 ? 2 : buf - 1; // (buf+1)%3, (buf+2)%3
            const float* wb = wl + buf * C::LDS_W;
            const float* wbn = wl + nbuf * C::LDS_W;
            float* ibw = il + wbuf * C::LDS_IN;
            float* wbw = wl + wbuf * C::LDS_W;
            // the registers hold chunk g+2 (each piece requested a whole chunk ago): its (scale, shift) and in-image mask;
            // then the load side moves on to chunk g+3, whose pieces are requested as the registers are freed
            float sc_[KC], sh_[KC];
            W4_READ_AFF(sc_, sh_, r_tab, r_c0)
            float q_mask[C::PR]; // upper clamp of the normalised value: +inf inside the image, 0 on the zero padding (v_med3_f32 does ReLU and padding in one)
#pragma unroll
            for (int r = 0; r < C::PR; ++r) q_mask[r] = ((r_vmask >> r) & 1u) ? __builtin_inff() : 0.f;
            advance();
            r_tab = s_tab; r_c0 = s_ch * KC; r_vmask = vmask;
            // One wave per SIMD issues IN ORDER and nothing of its own hides behind an fp32 MFMA (tools/issue_probe.hip): a VALU
            // instruction costs its 4 issue cycles wherever it stands and every MFMA -> VALU -> MFMA turn ~12 more; SALU 0.5 cycle;
            // the first LDS / VMEM instruction of a gap ~6.  The step = 4 MFMAs of one Winograd position and channel quad:
            //   MFMA 0 | gap A: the A fragment of step s+3 (one ds_read_b128)
            //   MFMA 1 | gap B (steps 0..3 of a quad): one raw patch row of the next quad (two ds_read2_b32)
            //   MFMA 2 | gap C (first step of a patch row only): ALL the VALU work of four steps, packed (see gap_c_body)
            //   MFMA 3 | gap D (steps 0..23): LDS write of staging piece s + the request that refills its register
            // MFMAs with an empty gap between them share one asm statement.  A B operand is written >= 1 step before its first
            // use and the A fragments come from LDS behind hipcc's own lgkmcnt wait, so the asm MFMAs need no s_nop pad.
            // (All memory instructions in ONE gap behind MFMA 3 measured slower, 872 against 890 frames/s.)
// N MFMAs of one step (M-tiles I .. I+N-1) in ONE asm statement: hipcc pads every boundary between two asm statements
// with an s_nop, so MFMAs with nothing to put between them are issued from one statement
#define W4_ACC(I) "i"((xi * 4 + (I)) * 4), "i"((xi * 4 + (I)) * 4 + 3)
#define W4_MFMA_1(I)                                                                             \
            if constexpr (first_ && s_ < 16) {                                                   \
                asm volatile("v_mfma_f32_16x16x4_f32 a[%c2:%c3], %0, %1, 0" :: "v"(a[s_ % AD][I]), "v"(vcur), W4_ACC(I) : W4_AGPRS); \
            } else {                                                                             \
                asm volatile("v_mfma_f32_16x16x4_f32 a[%c2:%c3], %0, %1, a[%c2:%c3]" :: "v"(a[s_ % AD][I]), "v"(vcur), W4_ACC(I) : W4_AGPRS); \
            }                                                                                    \
            __builtin_amdgcn_sched_barrier(0);
#define W4_MFMA_2(I)                                                                             \
            if constexpr (first_ && s_ < 16) {                                                   \
                asm volatile("v_mfma_f32_16x16x4_f32 a[%c3:%c4], %0, %2, 0\n\tv_mfma_f32_16x16x4_f32 a[%c5:%c6], %1, %2, 0"                  \
                             :: "v"(a[s_ % AD][I]), "v"(a[s_ % AD][(I) + 1]), "v"(vcur), W4_ACC(I), W4_ACC((I) + 1) : W4_AGPRS); \
            } else {                                                                             \
                asm volatile("v_mfma_f32_16x16x4_f32 a[%c3:%c4], %0, %2, a[%c3:%c4]\n\tv_mfma_f32_16x16x4_f32 a[%c5:%c6], %1, %2, a[%c5:%c6]" \
                             :: "v"(a[s_ % AD][I]), "v"(a[s_ % AD][(I) + 1]), "v"(vcur), W4_ACC(I), W4_ACC((I) + 1) : W4_AGPRS); \
            }                                                                                    \
            __builtin_amdgcn_sched_barrier(0);
#define W4_MFMA_3(I)                                                                             \
            if constexpr (first_ && s_ < 16) {                                                   \
                asm volatile("v_mfma_f32_16x16x4_f32 a[%c4:%c5], %0, %3, 0\n\tv_mfma_f32_16x16x4_f32 a[%c6:%c7], %1, %3, 0\n\t"            \
                             "v_mfma_f32_16x16x4_f32 a[%c8:%c9], %2, %3, 0"                                                                 \
                             :: "v"(a[s_ % AD][I]), "v"(a[s_ % AD][(I) + 1]), "v"(a[s_ % AD][(I) + 2]), "v"(vcur), W4_ACC(I), W4_ACC((I) + 1), W4_ACC((I) + 2) : W4_AGPRS); \
            } else {                                                                             \
                asm volatile("v_mfma_f32_16x16x4_f32 a[%c4:%c5], %0, %3, a[%c4:%c5]\n\tv_mfma_f32_16x16x4_f32 a[%c6:%c7], %1, %3, a[%c6:%c7]\n\t" \
                             "v_mfma_f32_16x16x4_f32 a[%c8:%c9], %2, %3, a[%c8:%c9]"                                                        \
                             :: "v"(a[s_ % AD][I]), "v"(a[s_ % AD][(I) + 1]), "v"(a[s_ % AD][(I) + 2]), "v"(vcur), W4_ACC(I), W4_ACC((I) + 1), W4_ACC((I) + 2) : W4_AGPRS); \
            }                                                                                    \
            __builtin_amdgcn_sched_barrier(0);
#define W4_MFMA_4(I)                                                                             \
            if constexpr (first_ && s_ < 16) {                                                   \
                asm volatile("v_mfma_f32_16x16x4_f32 a[%c5:%c6], %0, %4, 0\n\tv_mfma_f32_16x16x4_f32 a[%c7:%c8], %1, %4, 0\n\t"            \
                             "v_mfma_f32_16x16x4_f32 a[%c9:%c10], %2, %4, 0\n\tv_mfma_f32_16x16x4_f32 a[%c11:%c12], %3, %4, 0"             \
                             :: "v"(a[s_ % AD][I]), "v"(a[s_ % AD][(I) + 1]), "v"(a[s_ % AD][(I) + 2]), "v"(a[s_ % AD][(I) + 3]), "v"(vcur), \
                                W4_ACC(I), W4_ACC((I) + 1), W4_ACC((I) + 2), W4_ACC((I) + 3) : W4_AGPRS);                                    \
            } else {                                                                             \
                asm volatile("v_mfma_f32_16x16x4_f32 a[%c5:%c6], %0, %4, a[%c5:%c6]\n\tv_mfma_f32_16x16x4_f32 a[%c7:%c8], %1, %4, a[%c7:%c8]\n\t" \
                             "v_mfma_f32_16x16x4_f32 a[%c9:%c10], %2, %4, a[%c9:%c10]\n\tv_mfma_f32_16x16x4_f32 a[%c11:%c12], %3, %4, a[%c11:%c12]" \
                             :: "v"(a[s_ % AD][I]), "v"(a[s_ % AD][(I) + 1]), "v"(a[s_ % AD][(I) + 2]), "v"(a[s_ % AD][(I) + 3]), "v"(vcur), \
                                W4_ACC(I), W4_ACC((I) + 1), W4_ACC((I) + 2), W4_ACC((I) + 3) : W4_AGPRS);                                    \
            }                                                                                    \
            __builtin_amdgcn_sched_barrier(0);
            pp_steps<0, NSTEP>([&](auto S) {
                constexpr int s_ = decltype(S)::value;
                constexpr int c4 = s_ / 16, xi = s_ % 16, row = s_ / 4;
                constexpr bool gap_b = xi < 4;                      // raw patch rows of the next quad
                constexpr bool gap_c = (xi & 3) == 0;               // the VALU work of four steps
                vcur = (xi & 3) == 0 ? o0[row & 1] : (xi & 3) == 3 ? o3[row & 1] : p12[row & 1][(xi & 3) - 1];
                __builtin_amdgcn_sched_barrier(0);
                auto gap_a_body = [&]() {   // the A fragment of step s_+AD-1 (this chunk, or the next chunk's first steps from ring slot nbuf)
                    constexpr int sa = s_ + AD - 1;
                    if constexpr (sa < NSTEP) {
                        constexpr int n4_ = sa / 16, nx_ = sa % 16;
                        a[sa % AD] = *reinterpret_cast<const f32x4*>(wb + (nx_ * KC + n4_ * 4) * C::BM + aoff);
                    } else {
                        constexpr int sb = sa - NSTEP, n4_ = sb / 16, nx_ = sb % 16;
                        a[sa % AD] = *reinterpret_cast<const f32x4*>(wbn + (nx_ * KC + n4_ * 4) * C::BM + aoff);
                    }
                };
                // gap B (steps 0..3 of a quad): one raw patch row of the next quad (the next CHUNK's first quad from ring slot nbuf
                // when this is the chunk's last quad)
                auto gap_b_body = [&]() {
                    if constexpr (xi == 0) {
                        qb = (c4 + 1 < NQ) ? buf * C::LDS_IN + rbase + (c4 + 1) * 4 * C::CS : nbuf * C::LDS_IN + rbase;
                        asm volatile("" : "+v"(qb));
                    }
                    if constexpr (xi < 4) { W4_READ_RAW_ROW(draw, qb, xi) }
                };
                // gap C (first step of every patch row) carries the VALU work of FOUR steps -- every MFMA -> VALU -> MFMA turn costs
                // a lone wave ~12 cycles on top of 4 per instruction (tools/issue_probe.hip) -- all of it packed: the B operands of the
                // next patch row's four steps (3 instructions), the normalisation of staging pieces s_ .. s_+3 (2 v_pk_fma_f32 +
                // 4 v_med3_f32), and in rows 1 and 2 four column-pass terms of the next quad
                auto gap_c_body = [&]() {
                    constexpr int rn = row + 1; // next patch row; & 3 inside its quad, whose column pass sits in tq[(rn / 4) & 1]
                    W4_ROW_ALL(tq[(rn / 4) & 1], rn)
                    W4_NORM_PAIR(s_, sc_, sh_, q_mask) W4_NORM_PAIR(s_ + 2, sc_, sh_, q_mask)
                    if constexpr (xi == 4 || xi == 8) {
                        W4_COLPASS2(tq[(c4 + 1) & 1], draw, xi - 4)
                        W4_COLPASS2(tq[(c4 + 1) & 1], draw, xi - 4 + 1)
                        W4_COLPASS2(tq[(c4 + 1) & 1], draw, xi - 4 + 2)
                        W4_COLPASS2(tq[(c4 + 1) & 1], draw, xi - 4 + 3)
                    }
                    __builtin_amdgcn_sched_barrier(0);
                };
                W4_MFMA_1(0)
                gap_a_body();
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (gap_b && gap_c) { W4_MFMA_1(1) gap_b_body(); __builtin_amdgcn_sched_barrier(0); W4_MFMA_1(2) gap_c_body(); W4_MFMA_1(3) }
                else if constexpr (gap_b) { W4_MFMA_1(1) gap_b_body(); __builtin_amdgcn_sched_barrier(0); W4_MFMA_2(2) }
                else if constexpr (gap_c) { W4_MFMA_2(1) gap_c_body(); W4_MFMA_1(3) }
                else { W4_MFMA_3(1) }
                // gap D: staging of chunk g+2 into ring slot wbuf, and the request that refills the register with chunk g+3's piece
                if constexpr (s_ < NPIECE) {
                    W4_WRITE_PIECE(s_, ibw, wbw)
                    W4_LOAD_PIECE(s_)
                }
                __builtin_amdgcn_sched_barrier(0);
            });
#undef W4_MFMA_1
#undef W4_MFMA_2
#undef W4_MFMA_3
#undef W4_MFMA_4
#undef W4_ACC
            __syncthreads();
            buf = nbuf;
            if (ch == 0 && pending) { // previous tile's statistics: every wave's partial sums are in `red` since before this barrier
                if (tid < C::BM) {
                    double s = 0.0, q = 0.0;
#pragma unroll
                    for (int w = 0; w < WN; ++w) {
                        s += (double)red[(w * C::BM + tid) * 2];
                        q += (double)red[(w * C::BM + tid) * 2 + 1];
                    }
                    atomicAdd(pend_dst + (size_t)tid * 2, s);
                    atomicAdd(pend_dst + (size_t)tid * 2 + 1, q);
                }
                pending = false;
            }
        };
        chunk_body(std::true_type{}, 0);
#pragma unroll 1
        for (int ch = 1; ch < nchunk; ++ch) chunk_body(std::false_type{}, ch);

        // ---------------- epilogue: Y = A^T M A per lane, residual, float2 row stores, statistics ----------------
        // an 8-pass MFMA's D needs 12 wait states before anything but the next accumulating MFMA touches it (hipcc pads nothing
        // behind an asm statement)
        asm volatile("s_nop 11" ::: W4_AGPRS);
        float* __restrict__ gout = p.out + fz * p.out_fs;
        const unsigned frame_bytes = (unsigned)((size_t)p.Cout * out_plane * 4);
        const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(gout, 0, frame_bytes, 0x00020000);
        // Two halves (M-tiles 0-1, then 2-3), each in two phases.  Phase 1: the output transform of the half's 32 (row, tile)
        // pairs into registers, two accumulator rows at a time on v_pk_add_f32 (a lone wave pays 4 cycles per VALU instruction,
        // MFMA shadow or not: tools/issue_probe.hip).  Phase 2: residual add, stores, statistics.  The residual rows are
        // requested long before they are added: the first half's at the top of the tile's last chunk, the second half's
        // between the first half's two phases -- older than every store of the epilogue, so waiting for them never waits for
        // a store (loads and stores share vmcnt).  The live state of the chunk pipeline (~130 VGPRs) leaves room for both
        // halves' residual rows and one half's outputs.
        // X4 (maps whose width is a multiple of 4): the tile's epilogue is bound by the CU's store ISSUE rate -- four waves x 32
        // dwordx2 stores of 4 x 128-byte segments each took ~11 k cycles per tile (stamps).  Neighbouring lanes (tiles x, x+1)
        // swap half their 2x2 outputs (w4_pair_rows: four v_cndmask_b32_dpp) so that the even lane owns row y and the odd lane
        // row y+1 of the pair's 4 pixels: one dwordx4 store (and one dwordx4 residual load) per lane and row instead of two dwordx2.
        f32x2 y2[2][2][4]; // [M-tile of the half][row pair][output pixel of the 2x2 tile], .x = row 2 rp, .y = row 2 rp + 1
        auto transform_half = [&](auto HALF) {
            constexpr int h = decltype(HALF)::value;
            pp_steps<0, 2>([&](auto II) {
                constexpr int ii = decltype(II)::value, i = h * 2 + ii;
                pp_steps<0, 2>([&](auto RP) {
                    constexpr int rp = decltype(RP)::value;
                    f32x2 mm[16], t0[4], t1[4];
                    w4_acc_read32<i, 2 * rp>(mm);
#pragma unroll
                    for (int a_ = 0; a_ < 4; ++a_) {
                        t0[a_] = mm[a_ * 4 + 0] + mm[a_ * 4 + 1] + mm[a_ * 4 + 2];
                        t1[a_] = mm[a_ * 4 + 1] - mm[a_ * 4 + 2] - mm[a_ * 4 + 3];
                    }
                    y2[ii][rp][0] = t0[0] + t0[1] + t0[2]; y2[ii][rp][1] = t1[0] + t1[1] + t1[2];
                    y2[ii][rp][2] = t0[1] - t0[2] - t0[3]; y2[ii][rp][3] = t1[1] - t1[2] - t1[3];
                });
            });
        };
        auto finish_mt = [&](auto HALF, auto II0, auto II1, auto X4) { // M-tiles 2h+II0 .. 2h+II1-1
            constexpr int h = decltype(HALF)::value, ii0 = decltype(II0)::value, ii1 = decltype(II1)::value;
            constexpr bool x4 = decltype(X4)::value;
            f32x2 r0[2][4], r1[2][4];
            if constexpr (!x4) { // maps whose width is not a multiple of 4: two dwordx2 rows per lane, requested here
                const __amdgpu_buffer_rsrc_t rres_ = res_desc();
#pragma unroll
                for (int ii = 0; ii < 2; ++ii)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const unsigned so = (unsigned)((h * 2 + ii) * 16 + r) * plane_ob;
                        r0[ii][r] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rres_, lb0, so, 0));
                        r1[ii][r] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rres_, lb1, so, 0));
                    }
            }
#pragma unroll
            for (int ii = ii0; ii < ii1; ++ii) {
                float ssum[4], ssq[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const unsigned so = (unsigned)((h * 2 + ii) * 16 + r) * plane_ob;
                    const float y_0 = y2[ii][r >> 1][0][r & 1], y_1 = y2[ii][r >> 1][1][r & 1], y_2 = y2[ii][r >> 1][2][r & 1], y_3 = y2[ii][r >> 1][3][r & 1];
                    if constexpr (x4) {
                        f32x4 v = w4_pair_rows(y_0, y_1, y_2, y_3);
                        v += rq[h][ii][r];
                        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b128(rout, 0u, 0, 0)), v), rout, lb0, so, 0);
                        const f32x2 lo = {v[0], v[1]}, hi = {v[2], v[3]};
                        const f32x2 s2 = lo + hi, q2 = __builtin_elementwise_fma(hi, hi, lo * lo);
                        ssum[r] = ok0 ? s2[0] + s2[1] : 0.f;
                        ssq[r] = ok0 ? q2[0] + q2[1] : 0.f;
                    } else {
                        const float y00 = y_0 + r0[ii][r][0], y01 = y_1 + r0[ii][r][1];
                        const float y10 = y_2 + r1[ii][r][0], y11 = y_3 + r1[ii][r][1];
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b64(rout, 0u, 0, 0)), (f32x2){y00, y01}), rout, lb0, so, 0);
                        __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b64(rout, 0u, 0, 0)), (f32x2){y10, y11}), rout, lb1, so, 0);
                        float s_ = y00 + y01, q_ = y00 * y00 + y01 * y01; // same summation order as wino_mfma: row y, then row y+1
                        if (lb1 != W4_FAR) { s_ += y10; q_ += y10 * y10; s_ += y11; q_ += y11 * y11; }
                        ssum[r] = ok0 ? s_ : 0.f;
                        ssq[r] = ok0 ? q_ : 0.f;
                    }
                }
                if (p.stat_acc) {
                    float rs[4], rqq[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) { rs[r] = row16_sum(ssum[r]); rqq[r] = row16_sum(ssq[r]); }
                    if (m == 0) { // rows (h*2+ii)*16 + kq*4 + 0..3: 8 consecutive floats of `red`
                        float* dst = red + (wn * C::BM + (h * 2 + ii) * 16 + kq * 4) * 2;
                        *reinterpret_cast<f32x4*>(dst) = (f32x4){rs[0], rqq[0], rs[1], rqq[1]};
                        *reinterpret_cast<f32x4*>(dst + 4) = (f32x4){rs[2], rqq[2], rs[3], rqq[3]};
                    }
                }
            }
        };
        {
            using I0 = std::integral_constant<int, 0>;
            using I1 = std::integral_constant<int, 1>;
            using I2 = std::integral_constant<int, 2>;
            if (x4_map) {
                // every residual request is >= one transform + one M-tile's finish (~3.5 k cycles) ahead of its add; 32 registers
                // rotate through the four M-tiles' rows
                request_res(I0{}, I0{});
                request_res(I0{}, I1{});
                transform_half(I0{});
                finish_mt(I0{}, I0{}, I1{}, std::true_type{});
                request_res(I1{}, I0{});
                finish_mt(I0{}, I1{}, I2{}, std::true_type{});
                request_res(I1{}, I1{});
                transform_half(I1{});
                finish_mt(I1{}, I0{}, I2{}, std::true_type{});
            } else {
                transform_half(I0{});
                finish_mt(I0{}, I0{}, I2{}, std::false_type{});
                transform_half(I1{});
                finish_mt(I1{}, I0{}, I2{}, std::false_type{});
            }
        }
        if (p.stat_acc) {
            pending = true;
            pend_dst = p.stat_acc + fz * p.stat_fs + ((size_t)(blockIdx.x % NREP) * p.stat_C + co0) * 2;
        }
    }
    if (pending) {
        __syncthreads();
        if (tid < C::BM && blockIdx.x >= 0) {
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int w = 0; w < WN; ++w) {
                s += (double)red[(w * C::BM + tid) * 2];
                q += (double)red[(w * C::BM + tid) * 2 + 1];
            }
            atomicAdd(pend_dst + (size_t)tid * 2, s);
            atomicAdd(pend_dst + (size_t)tid * 2 + 1, q);
        }
    }
#undef W4_LOAD_PIECE
#undef W4_NORM_PAIR
#undef W4_READ_AFF
#undef W4_READ_RAW_ROW
#undef W4_WRITE_PIECE
#undef W4_COLPASS2
#undef W4_ROW_ALL
}

template <int TWT, int BTX, int KC>
Variant make_wino4(bool roofline_layer)
{
    using C = Wino4Cfg<TWT, BTX, KC>;
    Variant v;
    v.kern = roofline_layer ? wino4_mfma<TWT, BTX, KC, 1> : wino4_mfma<TWT, BTX, KC, 0>;
    v.bm = C::BM; v.bmp = C::BM; v.pw = C::PW; v.ph = C::PH; v.kc = KC; v.threads = C::THREADS;
    v.waves = 4; v.pairs = 4 * 16;
    v.lds = (size_t)C::LDS_FLOATS * sizeof(float);
    v.family = Family::Wino4;
    snprintf(v.name, sizeof(v.name), "wino4 tw%d bx%d kc%d", TWT, BTX, KC);
    return v;
}

} // namespace

namespace ppc {

// one wave per SIMD, 64 rows, 3-deep ring (even maps, Cout a multiple of 64 only -- see variant_ok)
void wino4_menu(std::vector<Variant>& menu, bool roofline_layer)
{
    menu.push_back(make_wino4<4, 2, 8>(roofline_layer));       // 16x16 px
    menu.push_back(make_wino4<8, 1, 8>(roofline_layer));       // 16x16 px, 8x2-tile N-tiles
    menu.push_back(make_wino4<8, 2, 8>(roofline_layer));       // 32x8 px
}
// strip tilings of the region launches (launch_conv): a map that is no multiple of 16 x 16 is covered by whole main tiles plus thin tiles
Variant wino4_strip_v() { return make_wino4<2, 1, 8>(false); }  // 4 px wide, 64 px tall
Variant wino4_strip_h() { return make_wino4<16, 2, 8>(false); } // 64 px wide, 4 px tall
// The image wino4_mfma stages, from U of wino2_transform: [row block][cin chunk][position 0..15][k][bmp], a block's rows in the order
// [m][M-tile 0..3] so a lane's four A operands are one ds_read_b128.  It depends on the 64-row block and the chunk only: the strip
// tilings read the main tile's image
void wino4_pack(const std::vector<float>& u, int rows, int cin, const Variant& v, std::vector<float>& out)
{
    pack_blocked(u, rows, cin, 16, v, [](int mm) { return (mm & 15) * 4 + (mm >> 4); }, out);
}

} // namespace ppc
