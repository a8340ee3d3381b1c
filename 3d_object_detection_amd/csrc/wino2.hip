// wino_mfma: the first Winograd family of the 2D backbone (Family::Wino), fp32 MFMA for gfx950, persistent, two workgroups per CU.
//
// Winograd F(2x2, 3x3) for the stride-1 3x3 convs (13 of the 16 convs, 141 of the 203 GFLOP):
//   Y = A^T [ sum_cin (G g G^T) (.) (B^T d B) ] A      -> 16 MFMA "positions" instead of 9 taps per
// 2x2 output tile, i.e. 2.25x fewer MFMAs, still exact-fp32 MFMA accumulation.
// * one lane = one 2x2 output tile (N-tile = 16 tiles, TWT x 16/TWT), M = 16 output channels
// * the weights are transformed on the host (fp64) and staged as a [16][KC][rows] LDS image
// * the INPUT transform runs in registers: each lane reads the 4x4 raw patch of its tile from the
//   same normalised/ReLU'd/zero-padded LDS patch the direct kernel uses (columns de-interleaved so the
//   stride-2 tile walk is bank-conflict free) and forms its 16 B-operands with 32 adds -- no second
//   LDS pass, no extra barrier
// * the OUTPUT transform is per lane too (the 16 positions of a tile are 16 accumulators of one lane)
#include <cstdio>
#include "pp_common.h"
#include "conv_common.h"

namespace {

using namespace ppc;

constexpr int WINO_PER = 2;  // minimum LDS write pieces per MFMA step of the staging pipeline (2: +0.3 % over 1, 4: -1.5 %)
constexpr int WINO_AD = 6;   // steps the A-operand LDS reads run ahead of their MFMA pair
constexpr int WINO_PRIO = 1; // s_setprio level of the NON-MFMA segments (chunk opening, epilogue, tile prologue) of the Winograd loop
template <int TWT, int WM, int WN, int BTX, int KC>
struct WinoCfg {
    static constexpr int THT = 16 / TWT;
    static constexpr int MT = 2;
    static constexpr int BTY = WN / BTX;
    static constexpr int PW = BTX * TWT * 2, PH = BTY * THT * 2;
    static constexpr int IW = PW + 2, IH = PH + 2;
    static constexpr int HALF = (IW + 1) / 2;
    static constexpr int iwp()
    {
        int v = IW;
        if (TWT == 16) return v;
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
    static constexpr int BM = WM * MT * 16;
    // A image row = [wm][m 0..15][M-tile 0/1]: one ds_read_b64 fetches a lane's two A operands; a 32-float row needs no
    // padding (kq and kq+1 fall on opposite 32-bank halves of the 64-bank b64 access), a 64-float row is padded by 32
    static constexpr int BMP = (BM == 32) ? 32 : BM + 32;
    static constexpr int THREADS = 64 * WM * WN;
    static constexpr int NPOS = IH * IW;
    static constexpr int PR = (NPOS + THREADS - 1) / THREADS;
    static constexpr int W4 = 16 * KC * BMP / 4;
    static constexpr int WR = (W4 + THREADS - 1) / THREADS;
    static constexpr int LDS_IN = KC * CS;
    static constexpr int LDS_W = 16 * KC * BMP;
    static constexpr int LDS_FLOATS = 2 * (LDS_IN + LDS_W) + 2 * 320 + 2 * WN * BM;
    static_assert(WN % BTX == 0, "tiles must form a rectangle");
};

// ROOFLINE: 1 instantiates a second, identical copy of the kernel for the roofline layer (3x3 s1 64->64 on the level-0
// map) only, so that a kernel trace / --stats summary has that layer's launches under their own symbol instead of
// averaged with the other layers the tuner gives the same tiling.
template <int TWT, int WM, int WN, int BTX, int KC, int ROOFLINE = 0>
__global__ void __launch_bounds__(64 * WM * WN, (WM * WN >= 8) ? 2 : 2) wino_mfma(const ConvP p)
{
    using C = WinoCfg<TWT, WM, WN, BTX, KC>;
    constexpr int MT = 2;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* il = smem;
    float* wl = il + 2 * C::LDS_IN;
    float* scl = wl + 2 * C::LDS_W;
    float* shl = scl + 320;
    float* red = shl + 320;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m = lane & 15, kq = lane >> 4;

    // PERSISTENT: two workgroups per CU walk the (cout block, tile, frame) list.  Workgroups are dealt round-robin
    // over the 8 XCDs, so XCD k takes the k-th contiguous eighth of the list (cout blocks of a tile and
    // neighbouring tiles meet in one L2) and its workgroups stride through that eighth.  Per tile this saves the
    // launch slot + scale/shift prologue of a fresh workgroup, and the next tile's first loads are in flight while
    // the stores of this tile's epilogue drain.
    const int nbx = (p.Wout + C::PW - 1) / C::PW, nby = (p.Hout + C::PH - 1) / C::PH;
    const int ntile = nbx * nby, ncb = (p.Cout + C::BM - 1) / C::BM;
    const int total = ntile * ncb * p.nb;
    const int per = (total + 7) >> 3;
    const int xk = blockIdx.x & 7, xj = blockIdx.x >> 3, nloc = gridDim.x >> 3;
    const int lin_end = min(total, (xk + 1) * per);
    // ---- load-side state: the tile whose global loads are being issued.  It runs one tile AHEAD of the compute
    //      side at a tile boundary: the next tile's first chunk is requested before this tile's epilogue, so its
    //      latency hides under the output transform and stores.
    int goff[C::PR], loff[C::PR];
    unsigned vmask = 0u;
    bool all_in = false;
    __amdgpu_buffer_rsrc_t rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in), 0, 0x7FFFFFFF, 0x00020000);
    const __amdgpu_buffer_rsrc_t rw = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.w), 0, 0x7FFFFFFF, 0x00020000);
    const unsigned plane_b = (unsigned)(p.Hin * p.Win) * 4u;
    unsigned wbase_b = 0u;
    float xv[C::PR][KC];
    f32x4 wv[C::WR];
#pragma unroll
    for (int r = 0; r < C::PR; ++r) {
        // threads past the patch's last position duplicate it (same load, same value to the same LDS word):
        // every staging instruction is unconditional, the MFMA stream stays one basic block
        const int pos = min(tid + r * C::THREADS, C::NPOS - 1);
        const int iy = pos / C::IW, ix = pos - iy * C::IW;
        loff[r] = iy * C::IWP + (ix & 1) * C::HALF + (ix >> 1);
    }
    auto set_load_tile = [&](int l) {
        const int cb_ = l % ncb, t_ = (l / ncb) % ntile, f_ = l / (ncb * ntile);
        const int iy0_ = (t_ / nbx) * C::PH - 1, ix0_ = (t_ % nbx) * C::PW - 1;
        vmask = 0u;
#pragma unroll
        for (int r = 0; r < C::PR; ++r) {
            const int pos = min(tid + r * C::THREADS, C::NPOS - 1);
            const int iy = pos / C::IW, ix = pos - iy * C::IW;
            const int gy = iy0_ + iy, gx = ix0_ + ix;
            const bool inb = gy >= 0 && gy < p.Hin && gx >= 0 && gx < p.Win;
            goff[r] = inb ? (gy * p.Win + gx) * 4 : 0; // byte offset inside a channel plane (SGPR base + 32-bit VGPR offset)
            vmask |= (inb ? 1u : 0u) << r;
        }
        // interior patches (the vast majority) need no zero-padding select at all: workgroup-uniform fast path
        all_in = (iy0_ >= 0) && (ix0_ >= 0) && (iy0_ + C::IH <= p.Hin) && (ix0_ + C::IW <= p.Win);
        rin = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p.in + (size_t)f_ * p.in_fs), 0, 0x7FFFFFFF, 0x00020000);
        wbase_b = (unsigned)((size_t)cb_ * (p.Cin / KC) * C::W4 * 16);
    };
#define WN_LOAD_X(CH, R)                                                                         \
    {                                                                                            \
        const unsigned cb_ = (unsigned)((CH) * KC) * plane_b;                                    \
        _Pragma("unroll") for (int c = 0; c < KC; ++c)                                           \
            xv[R][c] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rin, goff[R], cb_ + (unsigned)c * plane_b, 0)); \
    }
#define WN_LOAD_W(CH)                                                                            \
    {                                                                                            \
        const unsigned wb_ = wbase_b + (unsigned)(CH) * (C::W4 * 16);                            \
        _Pragma("unroll") for (int r = 0; r < C::WR; ++r) {                                      \
            const int e_ = tid + r * C::THREADS;                                                 \
            wv[r] = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rw, (e_ < C::W4 ? e_ : C::W4 - 1) * 16, wb_, 0)); \
        }                                                                                        \
    }
#define WN_LOAD_CHUNK(CH)                                                                        \
    {                                                                                            \
        _Pragma("unroll") for (int r = 0; r < C::PR; ++r) WN_LOAD_X(CH, r)                       \
        WN_LOAD_W(CH)                                                                            \
    }
    int cur_frame = -1;
    {
        const int lin0 = xk * per + xj;
        if (lin0 < lin_end) {
            set_load_tile(lin0);
            WN_LOAD_CHUNK(0)
        }
    }
    for (int lin = xk * per + xj; lin < lin_end; lin += nloc) {
    BlockId bid;
    bid.y = lin % ncb;
    bid.x = (lin / ncb) % ntile;
    bid.z = lin / (ncb * ntile);
    const size_t fz = bid.z;
    float* __restrict__ gout = p.out + fz * p.out_fs;
    const float* __restrict__ gres = p.res ? p.res + fz * p.res_fs : nullptr;
    double* __restrict__ gstat = p.stat_acc ? p.stat_acc + fz * p.stat_fs : nullptr;

    const int bx = bid.x % nbx, by = bid.x / nbx;
    const int co0 = bid.y * C::BM;
    const int ox0 = bx * C::PW, oy0 = by * C::PH;

    // (scale, shift) of the producer's normalisation: per frame, written by norm_finalize (PRE_AFFINE) -- reloaded
    // only when this workgroup moves to another frame.  Every wave is past the previous tile's last chunk barrier
    // here, so nobody still reads the arrays; the prologue's first barrier publishes them.
    if (p.pre != PRE_RAW && bid.z != cur_frame) {
        for (int c = tid; c < p.Cin; c += C::THREADS) {
            scl[c] = p.pre_scale[fz * p.aff_fs + c];
            shl[c] = p.pre_shift[fz * p.aff_fs + c];
        }
        cur_frame = bid.z;
    }

    // this lane's tile: block-local tile coords -> top-left output pixel and raw-patch base
    const int btx = wn % BTX, bty = wn / BTX;
    const int ttx = btx * TWT + (m % TWT), tty = bty * C::THT + (m / TWT);
    const int opx = ox0 + 2 * ttx, opy = oy0 + 2 * tty;
    const int rbase = (2 * tty) * C::IWP + ttx + kq * C::CS;
    const int aoff = kq * C::BMP + wm * 32 + m * 2; // float2 {M-tile 0, M-tile 1}

    f32x4 acc[MT][16];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int x = 0; x < 16; ++x) acc[i][x] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int nchunk = p.Cin / KC;

    // ---- software-pipelined chunk loop ------------------------------------------------------------
    // One register set holds the NEXT chunk's raw loads.  Per chunk (after its opening barrier):
    //   * LDS reads of this chunk's first channel quad are issued first, and the staged registers are
    //     normalised (VALU that needs no LDS) while those reads are in flight
    //   * the normalised registers are written to the OTHER LDS buffer one piece per MFMA step, then the
    //     loads of chunk ch+2 are re-issued -- they have until the next barrier (> half a chunk) to land
    //   * the input transform is cut in two: the column pass of quad q+1 is spread over the steps of
    //     quad q, the row pass is one add per step right before its MFMA pair
    // so a wave keeps issuing MFMAs by itself instead of relying on another wave being out of phase.
// normalise + ReLU + zero padding of the staged registers (chunk CH), in place
#define WN_NORM_CHUNK(CH)                                                                        \
    {                                                                                            \
        const int c0_ = (CH) * KC;                                                               \
        if (p.pre != PRE_RAW) {                                                                  \
            float sc_[KC], sh_[KC];                                                              \
            _Pragma("unroll") for (int c = 0; c < KC; c += 4) {                                  \
                const f32x4 a_ = *reinterpret_cast<const f32x4*>(scl + c0_ + c);                 \
                const f32x4 b_ = *reinterpret_cast<const f32x4*>(shl + c0_ + c);                 \
                _Pragma("unroll") for (int q = 0; q < 4; ++q) { sc_[c + q] = a_[q]; sh_[c + q] = b_[q]; } \
            }                                                                                    \
            _Pragma("unroll") for (int r = 0; r < C::PR; ++r)                                    \
                _Pragma("unroll") for (int c = 0; c < KC; ++c) xv[r][c] = fmaxf(fmaf(xv[r][c], sc_[c], sh_[c]), 0.f); \
        }                                                                                        \
        if (!all_in) { /* border patch: positions outside the image are zero AFTER the normalisation */ \
            _Pragma("unroll") for (int r = 0; r < C::PR; ++r) {                                  \
                const bool inb_ = (vmask >> r) & 1u;                                             \
                _Pragma("unroll") for (int c = 0; c < KC; ++c) xv[r][c] = inb_ ? xv[r][c] : 0.f; \
            }                                                                                    \
        }                                                                                        \
    }
// piece E of the LDS write of the staged chunk into buffer BUF: E < PR*KC one input element, then the weight quads
#define WN_WRITE_PIECE(E, BUF)                                                                   \
    {                                                                                            \
        if constexpr ((E) < C::PR * KC) {                                                        \
            constexpr int r_ = (E) / KC, c_ = (E) % KC;                                          \
            (il + (BUF) * C::LDS_IN)[c_ * C::CS + loff[r_]] = xv[r_][c_];                        \
        } else if constexpr ((E) < C::PR * KC + C::WR) {                                         \
            constexpr int r_ = (E) - C::PR * KC;                                                 \
            const int e_ = tid + r_ * C::THREADS;                                                \
            reinterpret_cast<f32x4*>(wl + (BUF) * C::LDS_W)[e_ < C::W4 ? e_ : C::W4 - 1] = wv[r_]; /* clamped lanes repeat the last quad */ \
        }                                                                                        \
    }
// raw 4x4 patch of this lane's tile for channel quad C4 (this lane: channel C4*4 + kq)
#define WN_READ_RAW(DST, C4)                                                                     \
    _Pragma("unroll") for (int i_ = 0; i_ < 4; ++i_)                                             \
        _Pragma("unroll") for (int j_ = 0; j_ < 4; ++j_)                                         \
            DST[i_ * 4 + j_] = ib[rbase + (C4) * 4 * C::CS + i_ * C::IWP + (j_ & 1) * C::HALF + (j_ >> 1)];
// V = B^T d B in two passes.  Column pass, piece K (0..15): T = B^T d
#define WN_COLPASS(T, D, K)                                                                      \
    {                                                                                            \
        constexpr int a_ = (K) / 4, j_ = (K) % 4;                                                \
        if constexpr (a_ == 0) T[0 + j_] = D[0 + j_] - D[8 + j_];                                \
        else if constexpr (a_ == 1) T[4 + j_] = D[4 + j_] + D[8 + j_];                           \
        else if constexpr (a_ == 2) T[8 + j_] = D[8 + j_] - D[4 + j_];                           \
        else T[12 + j_] = D[4 + j_] - D[12 + j_];                                                \
    }
// row pass for Winograd point XI
#define WN_ROWPASS(T, XI)                                                                        \
    (((XI) & 3) == 0 ? T[(XI)] - T[((XI) + 2) & 15] : ((XI) & 3) == 1 ? T[(XI)] + T[((XI) + 1) & 15] : ((XI) & 3) == 2 ? T[(XI)] - T[((XI) - 1) & 15] : T[((XI) - 2) & 15] - T[(XI)]) /* & 15: keeps the untaken arms in range */

    constexpr int NQ = KC / 4;
    constexpr int NSTEP = NQ * 16;
    constexpr int NPIECE = C::PR * KC + C::WR;                       // LDS write pieces of one chunk
    constexpr int LOAD_STEPS = C::PR + 1;                            // re-issue: one x row or the weights per step
    constexpr int PER_MIN = (NPIECE + (NSTEP - LOAD_STEPS - 1) - 1) / (NSTEP - LOAD_STEPS - 1);
    constexpr int PER = PER_MIN > WINO_PER ? PER_MIN : WINO_PER; // write pieces per step (more per step = the next loads go out earlier)
    constexpr int WSTEPS = (NPIECE + PER - 1) / PER;
    static_assert(WSTEPS + LOAD_STEPS <= NSTEP, "staging does not fit the chunk's MFMA steps");
    // A operands run AD steps ahead of their MFMAs (a step is only 2 MFMAs = 64 cycles; LDS latency is 2-3x that)
    constexpr int AD = WINO_AD;

    // chunk 0 of this tile was requested before the previous tile's epilogue (or ahead of the loop)
    __syncthreads(); // scl / shl visible
    WN_NORM_CHUNK(0)
    pp_steps<0, NPIECE>([&](auto E) { WN_WRITE_PIECE(decltype(E)::value, 0) });
    if (nchunk > 1) WN_LOAD_CHUNK(1)
    __syncthreads();

    for (int ch = 0; ch < nchunk; ++ch) {
        const int buf = ch & 1;
        const float* ib = il + buf * C::LDS_IN;
        const float* wb = wl + buf * C::LDS_W;
        float draw[16], tq[2][16];
        float2 a[AD];
        float vcur, vnext;
        __builtin_amdgcn_s_setprio(WINO_PRIO); // the short non-MFMA segments first: back to the matrix pipe sooner
        WN_READ_RAW(draw, 0)
#define WN_LOAD_A(S)                                                                             \
    {                                                                                            \
        constexpr int n4_ = (S) / 16, nx_ = (S) % 16;                                            \
        a[(S) % AD] = *reinterpret_cast<const float2*>(wb + (nx_ * KC + n4_ * 4) * C::BMP + aoff); \
    }
        pp_steps<0, (AD - 1 < NSTEP ? AD - 1 : NSTEP)>([&](auto S) { WN_LOAD_A(decltype(S)::value) });
        // registers of chunk ch+1: normalise while the LDS reads above are in flight (at the last chunk this
        // re-normalises stale registers whose LDS copy nobody reads)
        {
            const int chn = ch + 1 < nchunk ? ch + 1 : ch;
            WN_NORM_CHUNK(chn)
        }
        pp_steps<0, 16>([&](auto K) { WN_COLPASS(tq[0], draw, decltype(K)::value) });
        vnext = WN_ROWPASS(tq[0], 0);
        __builtin_amdgcn_s_setprio(0);
        pp_steps<0, NSTEP>([&](auto S) {
            constexpr int s_ = decltype(S)::value;
            constexpr int c4 = s_ / 16, xi = s_ % 16;
            vcur = vnext;
            // next quad: raw reads at its predecessor's first step, column pass over steps 6..13
            if constexpr (xi == 0 && c4 + 1 < NQ) WN_READ_RAW(draw, c4 + 1)
            if constexpr (c4 + 1 < NQ && xi >= 6 && xi < 14) {
                WN_COLPASS(tq[(c4 + 1) & 1], draw, (xi - 6) * 2)
                WN_COLPASS(tq[(c4 + 1) & 1], draw, (xi - 6) * 2 + 1)
            }
            if constexpr (s_ + 1 < NSTEP) {
                constexpr int c4n = (s_ + 1) / 16, xin = (s_ + 1) % 16;
                vnext = WN_ROWPASS(tq[c4n & 1], xin);
            }
            if constexpr (s_ + AD - 1 < NSTEP) WN_LOAD_A(s_ + AD - 1)
            // staging of chunk ch+1: LDS writes first, then the loads of chunk ch+2 into the freed registers
            if constexpr (s_ < WSTEPS) {
                pp_steps<0, PER>([&](auto Q) { WN_WRITE_PIECE(s_ * PER + decltype(Q)::value, buf ^ 1) });
            } else if constexpr (s_ - WSTEPS < C::PR) {
                if (ch + 2 < nchunk) WN_LOAD_X(ch + 2, s_ - WSTEPS)
            } else if constexpr (s_ - WSTEPS == C::PR) {
                if (ch + 2 < nchunk) WN_LOAD_W(ch + 2)
            }
            __builtin_amdgcn_sched_barrier(0);
            acc[0][xi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s_ % AD].x, vcur, acc[0][xi], 0, 0, 0);
            acc[1][xi] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s_ % AD].y, vcur, acc[1][xi], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
#undef WN_LOAD_A
        __syncthreads();
    }
#undef WN_NORM_CHUNK
#undef WN_WRITE_PIECE
#undef WN_READ_RAW
#undef WN_COLPASS
#undef WN_ROWPASS

    __builtin_amdgcn_s_setprio(WINO_PRIO);
    if (lin + nloc < lin_end) { // next tile's first chunk: in flight during the epilogue below
        set_load_tile(lin + nloc);
        WN_LOAD_CHUNK(0)
    }
    // ---- epilogue: Y = A^T M A per lane, residual, store (float2 rows), statistics ----
    const size_t out_plane = (size_t)p.Hout * p.Wout;
    float ssum[MT][4], ssq[MT][4];
    const bool pix_ok = (opx < p.Wout) && (opy < p.Hout);
    if (!(p.Wout & 1)) {
        // Even width (every map of this network): a lane's two output columns are one aligned float2.  Branch-free: the
        // residual rows are requested up front and everything goes through buffer descriptors whose bounds check drops
        // the lanes that have no pixel / row (offset 0xFFFFFFFF).  The per-row `load -> s_waitcnt vmcnt(0) -> add ->
        // store` chains of the branchy form made every row wait for the previous row's STORES and for the next tile's
        // prefetch as well (vmcnt is in order): 5.5 k of a tile's 113 k cycles by the stamps.
        const unsigned frame_bytes = (unsigned)((size_t)p.Cout * out_plane * 4);
        const __amdgpu_buffer_rsrc_t rout = __builtin_amdgcn_make_buffer_rsrc(gout, 0, frame_bytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rres_ = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gres ? gres : gout), 0, gres ? frame_bytes : 0u, 0x00020000);
        const bool two_y = opy + 1 < p.Hout;
        unsigned off0[MT][4], off1[MT][4];
        typedef float f32x2 __attribute__((ext_vector_type(2)));
        f32x2 r0[MT][4], r1[MT][4];
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = co0 + wm * MT * 16 + i * 16 + kq * 4 + r;
                const bool ok = pix_ok && row < p.Cout;
                const unsigned o = (unsigned)(((size_t)row * out_plane + (size_t)opy * p.Wout + opx) * 4);
                off0[i][r] = ok ? o : 0xFFFFFFFFu;
                off1[i][r] = (ok && two_y) ? o + (unsigned)p.Wout * 4u : 0xFFFFFFFFu;
                r0[i][r] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rres_, off0[i][r], 0, 0)); // zero records when the layer has no residual
                r1[i][r] = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(rres_, off1[i][r], 0, 0));
            }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float t0[4], t1[4];
#pragma unroll
                for (int a_ = 0; a_ < 4; ++a_) {
                    const float m0 = acc[i][a_ * 4 + 0][r], m1 = acc[i][a_ * 4 + 1][r], m2 = acc[i][a_ * 4 + 2][r], m3 = acc[i][a_ * 4 + 3][r];
                    t0[a_] = m0 + m1 + m2;
                    t1[a_] = m1 - m2 - m3;
                }
                float y00 = t0[0] + t0[1] + t0[2], y01 = t1[0] + t1[1] + t1[2];
                float y10 = t0[1] - t0[2] - t0[3], y11 = t1[1] - t1[2] - t1[3];
                y00 += r0[i][r][0]; y01 += r0[i][r][1];
                y10 += r1[i][r][0]; y11 += r1[i][r][1];
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b64(rout, 0u, 0, 0)), (f32x2){y00, y01}), rout, off0[i][r], 0, 0);
                __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(decltype(__builtin_amdgcn_raw_buffer_load_b64(rout, 0u, 0, 0)), (f32x2){y10, y11}), rout, off1[i][r], 0, 0);
                const bool ok0 = off0[i][r] != 0xFFFFFFFFu, ok1 = off1[i][r] != 0xFFFFFFFFu;
                // same summation order as the reference form below: row y, then row y+1
                float s_ = y00 + y01, q_ = y00 * y00 + y01 * y01;
                if (ok1) { s_ += y10; q_ += y10 * y10; s_ += y11; q_ += y11 * y11; }
                ssum[i][r] = ok0 ? s_ : 0.f;
                ssq[i][r] = ok0 ? q_ : 0.f;
            }
    } else {
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int row0 = co0 + wm * MT * 16 + i * 16 + kq * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float t0[4], t1[4];
#pragma unroll
            for (int a_ = 0; a_ < 4; ++a_) {
                const float m0 = acc[i][a_ * 4 + 0][r], m1 = acc[i][a_ * 4 + 1][r], m2 = acc[i][a_ * 4 + 2][r], m3 = acc[i][a_ * 4 + 3][r];
                t0[a_] = m0 + m1 + m2;
                t1[a_] = m1 - m2 - m3;
            }
            float y00 = t0[0] + t0[1] + t0[2], y01 = t1[0] + t1[1] + t1[2];
            float y10 = t0[1] - t0[2] - t0[3], y11 = t1[1] - t1[2] - t1[3];
            ssum[i][r] = 0.f;
            ssq[i][r] = 0.f;
            if (pix_ok && row0 + r < p.Cout) {
                const size_t o = (size_t)(row0 + r) * out_plane + (size_t)opy * p.Wout + opx;
                const bool two_x = opx + 1 < p.Wout, two_y = opy + 1 < p.Hout;
                if (gres) {
                    if (two_x) {
                        const float2 r0 = *reinterpret_cast<const float2*>(gres + o);
                        y00 += r0.x; y01 += r0.y;
                        if (two_y) { const float2 r1 = *reinterpret_cast<const float2*>(gres + o + p.Wout); y10 += r1.x; y11 += r1.y; }
                    } else {
                        y00 += gres[o];
                        if (two_y) y10 += gres[o + p.Wout];
                    }
                }
                if (two_x) {
                    *reinterpret_cast<float2*>(gout + o) = make_float2(y00, y01);
                    if (two_y) *reinterpret_cast<float2*>(gout + o + p.Wout) = make_float2(y10, y11);
                } else {
                    gout[o] = y00;
                    if (two_y) gout[o + p.Wout] = y10;
                }
                float s_ = y00, q_ = y00 * y00;
                if (two_x) { s_ += y01; q_ += y01 * y01; }
                if (two_y) { s_ += y10; q_ += y10 * y10; if (two_x) { s_ += y11; q_ += y11 * y11; } }
                ssum[i][r] = s_;
                ssq[i][r] = q_;
            }
        }
    }
    }
    if (gstat) {
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = ssum[i][r], q = ssq[i][r];
                s = row16_sum(s);
                q = row16_sum(q);
                if (m == 0) {
                    const int lr = wm * MT * 16 + i * 16 + kq * 4 + r;
                    red[(wn * C::BM + lr) * 2] = s;
                    red[(wn * C::BM + lr) * 2 + 1] = q;
                }
            }
        __syncthreads();
        for (int lr = tid; lr < C::BM; lr += C::THREADS) {
            const int row = co0 + lr;
            if (row >= p.Cout) continue;
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int w = 0; w < WN; ++w) {
                s += (double)red[(w * C::BM + lr) * 2];
                q += (double)red[(w * C::BM + lr) * 2 + 1];
            }
            double* dst = gstat + ((size_t)(blockIdx.x % NREP) * p.stat_C + row) * 2;
            atomicAdd(dst, s);
            atomicAdd(dst + 1, q);
        }
    }
    } // tile loop
#undef WN_LOAD_X
#undef WN_LOAD_W
#undef WN_LOAD_CHUNK
}

template <int TWT, int WM, int WN, int BTX, int KC>
Variant make_wino(bool roofline_layer)
{
    using C = WinoCfg<TWT, WM, WN, BTX, KC>;
    Variant v;
    v.kern = roofline_layer ? wino_mfma<TWT, WM, WN, BTX, KC, 1> : wino_mfma<TWT, WM, WN, BTX, KC, 0>;
    v.bm = C::BM; v.bmp = C::BMP; v.pw = C::PW; v.ph = C::PH; v.kc = KC; v.threads = C::THREADS;
    v.waves = WM * WN; v.pairs = 2 * 16;
    v.lds = (size_t)C::LDS_FLOATS * sizeof(float);
    v.family = Family::Wino;
    snprintf(v.name, sizeof(v.name), "wino tw%d w%dx%d bx%d kc%d", TWT, WM, WN, BTX, KC);
    return v;
}

} // namespace

namespace ppc {

void wino2_menu(std::vector<Variant>& menu, bool roofline_layer)
{
    //                     TWT WM WN BTX KC      output patch, rows
    menu.push_back(make_wino<8, 1, 4, 1, 8>(roofline_layer));  // 16x16 px, 32 rows
    menu.push_back(make_wino<8, 1, 4, 2, 8>(roofline_layer));  // 32x8 px, 32 rows
    menu.push_back(make_wino<8, 2, 2, 1, 8>(roofline_layer));  // 16x8 px, 64 rows
    menu.push_back(make_wino<8, 2, 4, 1, 8>(roofline_layer));  // 16x16 px, 64 rows, 8 waves
    menu.push_back(make_wino<4, 1, 4, 2, 8>(roofline_layer));  // 16x16 px, 32 rows
    menu.push_back(make_wino<4, 2, 2, 1, 8>(roofline_layer));  // 8x16 px, 64 rows
    menu.push_back(make_wino<4, 2, 4, 2, 8>(roofline_layer));  // 16x16 px, 64 rows, 8 waves
    menu.push_back(make_wino<4, 1, 4, 1, 8>(roofline_layer));  // 8x32 px, 32 rows
    menu.push_back(make_wino<2, 1, 4, 2, 8>(roofline_layer));  // 8x32 px (2x8-tile N-tiles), 32 rows
    // (8-wave 32-row tilings, WN = 8, were tried: 6-15 % slower than their 4-wave twins -- two lock-stepped waves per SIMD)
    menu.push_back(make_wino<8, 1, 4, 1, 4>(roofline_layer));
    menu.push_back(make_wino<4, 1, 4, 2, 4>(roofline_layer));
}
// U = G g G^T per (cout, cin), fp64 on the host, rounded once; position xi = 4*a + b
void wino2_transform(std::vector<float>& w)
{
    static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
    std::vector<float> u(w.size() / 9 * 16);
    for (size_t rc = 0; rc < w.size() / 9; ++rc) {
        const float* g = &w[rc * 9];
        double t[4][3];
        for (int a = 0; a < 4; ++a)
            for (int j = 0; j < 3; ++j) t[a][j] = G[a][0] * g[0 * 3 + j] + G[a][1] * g[1 * 3 + j] + G[a][2] * g[2 * 3 + j];
        for (int a = 0; a < 4; ++a)
            for (int b = 0; b < 4; ++b) u[rc * 16 + a * 4 + b] = (float)(t[a][0] * G[b][0] + t[a][1] * G[b][1] + t[a][2] * G[b][2]);
    }
    w.swap(u);
}
// The image wino_mfma stages: [row block][cin chunk][position 0..15][k][bmp], a block's rows in the order [wm][m][M-tile] so a lane's
// two A operands are adjacent (ds_read_b64)
void wino2_pack(const std::vector<float>& u, int rows, int cin, const Variant& v, std::vector<float>& out)
{
    pack_blocked(u, rows, cin, 16, v, [](int mm) { return (mm >> 5) * 32 + (mm & 15) * 2 + ((mm >> 4) & 1); }, out);
}

} // namespace ppc
