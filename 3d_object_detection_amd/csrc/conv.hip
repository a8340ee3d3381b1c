// 2D backbone (RPN) + shared head as fp32 MFMA implicit GEMMs for gfx950.
// Reference: networks/pointpillars8_shared.py:114-181 (RPN), :299-343 (SharedHead),
// :418-431 (Resnet2); BatchNorm variant networks/pointpillars8_export.py:54-119.
//
// One kernel template covers conv3x3 (stride 1/2), ConvTranspose(k == stride) and the 1x1 head:
//
//   D[cout, pixel] = sum_k  Wt[cout, k] * X[k, pixel]        k = (tap, cin)
//
// * MFMA: v_mfma_f32_16x16x4_f32 (exact fp32, k-ordered fma chain).  M = 16 output channels,
//   N = 16 output pixels, K = 4 input channels of one filter tap.  Pixels sit on the LANE axis of
//   the C/D layout (col = lane&15), channels in the 4 accumulator registers, so one store
//   instruction writes 16 consecutive pixels of a channel (NCHW, coalesced) and the per-channel
//   InstanceNorm statistics reduce with 4 xor-shuffles.
// * Tensors stay NCHW (the reference layout): for a fixed (cin, tap) the 16 pixels of an N-tile are
//   contiguous in the LDS patch, so the B-operand read is one conflict-free ds_read_b32.
// * No im2col: each workgroup stages a [KC][IH][IW] input patch with halo ONCE per channel chunk
//   and walks the 9 taps as shifted windows of it.  Zero padding, the producer's normalisation
//   (InstanceNorm / folded BatchNorm as x*scale+shift) and ReLU are applied while staging, so
//   normalised activations are never materialised in HBM.
// * InstanceNorm2d(eps=1e-3, affine=False) needs full-plane statistics of every conv output: the
//   epilogue reduces sum / sum-of-squares per channel (fp32 over <= 64 pixels, then fp64) and adds
//   them to 8 replicated fp64 accumulators; the CONSUMER kernel turns them into (scale, shift) in
//   its prologue.  No separate statistics pass, no finalize launch.
// * ConvTranspose(k = s, stride = s) is a 1x1 conv onto Cout*s*s virtual channels whose epilogue
//   pixel-shuffles (float2 / float4 stores); the three upsampled maps land in one [320,H,W]
//   buffer, so the concat is free and the head normalises + ReLUs them in its prologue.
#include <algorithm>
#include <type_traits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <unistd.h>
#include "pp_common.h"
#include "conv_common.h"

namespace {

using namespace ppc;

template <int KS, int STRIDE, int TW, int WM, int WN, int MT, int NT, int BTX, int KC, int EPI>
struct ConvCfg {
    static constexpr int TH = 16 / TW;
    static constexpr int TILES = WN * NT;
    static constexpr int BTY = TILES / BTX;
    static constexpr int PW = BTX * TW, PH = BTY * TH;
    static constexpr int IW = (PW - 1) * STRIDE + KS, IH = (PH - 1) * STRIDE + KS;
    static constexpr int HALF = (IW + 1) / 2; // stride 2: even columns first, odd columns after (de-interleaved)
    static constexpr int iwp()
    {
        int v = IW;
        if (TW == 16) return v;
        while ((STRIDE * v) % 32 != TW) ++v; // the TH rows of an N-tile land on disjoint bank groups
        return v;
    }
    static constexpr int IWP = iwp();
    static constexpr int cs()
    {
        int v = IH * IWP;
        while (v % 32 != 16) ++v; // channel c+1 (lanes 16-31 / 48-63) is 16 banks away from channel c
        return v;
    }
    static constexpr int CS = cs();
    static constexpr int BM = WM * MT * 16;
    static constexpr int BMP = BM + ((BM % 32 == 0) ? 16 : 0);
    static constexpr int THREADS = 64 * WM * WN;
    static constexpr int NPOS = IH * IW;                          // patch positions per channel
    static constexpr int PR = (NPOS + THREADS - 1) / THREADS;     // positions per thread
    static constexpr int W4 = KS * KS * KC * BMP / 4;             // float4 per weight chunk image
    static constexpr int WR = (W4 + THREADS - 1) / THREADS;
    static constexpr int LDS_IN = KC * CS;
    static constexpr int LDS_W = KS * KS * KC * BMP;
    static constexpr int LDS_FLOATS = 2 * (LDS_IN + LDS_W) + 2 * 320 + 2 * WN * BM;
    static_assert(TILES % BTX == 0, "tiles must form a rectangle");
    static_assert(KC % 4 == 0, "KC multiple of the MFMA K");
    static_assert((KS * KS * KC * BMP) % 4 == 0 && LDS_IN % 4 == 0, "float4 staging");
};

// Software pipeline per channel chunk (one barrier per chunk):
//   global loads of chunk c+1 -> registers   (in flight during the MFMAs)
//   MFMAs of chunk c from LDS buffer c&1
//   registers -> LDS buffer (c+1)&1 (normalise + ReLU + zero padding applied here)
//   barrier
template <int KS, int STRIDE, int TW, int WM, int WN, int MT, int NT, int BTX, int KC, int EPI>
__global__ void __launch_bounds__(64 * WM * WN) conv_mfma(const ConvP p)
{
    using C = ConvCfg<KS, STRIDE, TW, WM, WN, MT, NT, BTX, KC, EPI>;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* il = smem;                          // [2][KC][CS]
    float* wl = il + 2 * C::LDS_IN;            // [2][KS*KS][KC][BMP]
    float* scl = wl + 2 * C::LDS_W;            // [320] scale
    float* shl = scl + 320;                    // [320] shift
    float* red = shl + 320;                    // [WN][BM][2]
    // frame of this workgroup (batched launch)
    const BlockId bid = xcd_block_id();
    const size_t fz = bid.z;
    const float* __restrict__ gin = p.in + fz * p.in_fs;
    float* __restrict__ gout = p.out + fz * p.out_fs;
    const float* __restrict__ gres = p.res ? p.res + fz * p.res_fs : nullptr;
    const double* __restrict__ gpre = p.pre_acc ? p.pre_acc + fz * p.pre_fs : nullptr;
    double* __restrict__ gstat = p.stat_acc ? p.stat_acc + fz * p.stat_fs : nullptr;
    float* __restrict__ gbox = p.out_box ? p.out_box + fz * p.box_fs : nullptr;
    float* __restrict__ gdir = p.out_dir ? p.out_dir + fz * p.dir_fs : nullptr;
    (void)gbox; (void)gdir;

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int m = lane & 15, kq = lane >> 4;

    const int nbx = (p.Wout + C::PW - 1) / C::PW;
    const int bx = bid.x % nbx, by = bid.x / nbx;
    const int co0 = bid.y * C::BM;
    const int ox0 = bx * C::PW, oy0 = by * C::PH;
    const int ix0 = ox0 * STRIDE - KS / 2, iy0 = oy0 * STRIDE - KS / 2;

    // ---- prologue: per-input-channel (scale, shift) of the producer's normalisation ----
    if (p.pre == PRE_STATS) {
        for (int c = tid; c < p.Cin; c += C::THREADS) {
            double s = 0.0, q = 0.0;
#pragma unroll
            for (int r = 0; r < NREP; ++r) {
                s += gpre[((size_t)r * p.Cin + c) * 2];
                q += gpre[((size_t)r * p.Cin + c) * 2 + 1];
            }
            double mean = s * p.pre_inv_n;
            double var = q * p.pre_inv_n - mean * mean;
            var = var > 0.0 ? var : 0.0;
            double rstd = 1.0 / sqrt(var + (double)p.eps);
            scl[c] = (float)rstd;
            shl[c] = (float)(-mean * rstd);
        }
    } else if (p.pre == PRE_AFFINE) {
        for (int c = tid; c < p.Cin; c += C::THREADS) {
            scl[c] = p.pre_scale[fz * p.aff_fs + c];
            shl[c] = p.pre_shift[fz * p.aff_fs + c];
        }
    }

    // ---- per-thread staging map: position -> (global offset in a channel plane, LDS offset) ----
    // Loads are UNCONDITIONAL (out-of-image positions read offset 0 of the plane and are zeroed when
    // written to LDS): a per-element "load or 0" select makes hipcc branch around every load.
    int goff[C::PR], loff[C::PR];
    unsigned vmask = 0u;
#pragma unroll
    for (int r = 0; r < C::PR; ++r) {
        const int pos = tid + r * C::THREADS;
        const int iy = pos / C::IW, ix = pos - iy * C::IW;
        const int gy = iy0 + iy, gx = ix0 + ix;
        const bool inb = pos < C::NPOS && gy >= 0 && gy < p.Hin && gx >= 0 && gx < p.Win;
        goff[r] = inb ? gy * p.Win + gx : 0;
        vmask |= (inb ? 1u : 0u) << r;
        const int col = (STRIDE == 2) ? ((ix & 1) * C::HALF + (ix >> 1)) : ix;
        loff[r] = pos < C::NPOS ? iy * C::IWP + col : -1;
    }

    // lane's pixel base inside the LDS patch for each of its N-tiles
    int toff[NT];
    int opx[NT], opy[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int t = wn * NT + nt;
        const int tx = t % BTX, ty = t / BTX;
        const int px = tx * TW + (m % TW), py = ty * C::TH + (m / TW);
        opx[nt] = ox0 + px;
        opy[nt] = oy0 + py;
        toff[nt] = (py * STRIDE) * C::IWP + px + kq * C::CS; // stride 2: px indexes the even-column plane
    }
    const int aoff = kq * C::BMP + wm * MT * 16 + m;

    f32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const size_t in_plane = (size_t)p.Hin * p.Win;
    int nchunk = p.Cin / KC;
    // Sparse BEV input (first conv): each staged position carries the pillar id of its cell; channels come from
    // the [P][64] PFN rows.  A workgroup whose whole halo patch is empty has an all-zero output: skip its MFMA loop.
    const bool sparse = p.pmap != nullptr;
    int pid[C::PR];
    const float* gfeat = nullptr;
    if (sparse) {
        const int32_t* gmap = p.pmap + fz * p.pmap_fs;
        gfeat = p.feat + fz * p.feat_fs;
        int any = 0;
#pragma unroll
        for (int r = 0; r < C::PR; ++r) {
            pid[r] = ((vmask >> r) & 1u) ? gmap[goff[r]] : -1;
            any |= (pid[r] >= 0);
            if (pid[r] < 0) vmask &= ~(1u << r);
            goff[r] = pid[r] >= 0 ? pid[r] * 64 : 0; // reuse goff as the row offset into feat
        }
        if (!__syncthreads_or(any)) nchunk = 0;
    }
    const float4* wsrc = reinterpret_cast<const float4*>(p.w) + (size_t)bid.y * (p.Cin / KC) * C::W4;

    float xv[C::PR][KC];
    f32x4 wv[C::WR];
    const f32x4* wsrc4 = reinterpret_cast<const f32x4*>(wsrc);

#define PP_LOAD_CHUNK(CH)                                                                        \
    {                                                                                            \
        if (sparse) {                                                                            \
            const float* fb_ = gfeat + (CH) * KC;                                                \
            _Pragma("unroll") for (int r = 0; r < C::PR; ++r)                                    \
                _Pragma("unroll") for (int c = 0; c < KC; ++c) xv[r][c] = fb_[goff[r] + c];      \
        } else {                                                                                 \
            const float* base_ = gin + (size_t)((CH) * KC) * in_plane;                           \
            _Pragma("unroll") for (int r = 0; r < C::PR; ++r)                                    \
                _Pragma("unroll") for (int c = 0; c < KC; ++c) xv[r][c] = base_[(size_t)c * in_plane + goff[r]]; \
        }                                                                                        \
        const f32x4* g_ = wsrc4 + (size_t)(CH) * C::W4;                                          \
        _Pragma("unroll") for (int r = 0; r < C::WR; ++r) {                                      \
            const int e_ = tid + r * C::THREADS;                                                 \
            wv[r] = g_[e_ < C::W4 ? e_ : C::W4 - 1];                                             \
        }                                                                                        \
    }
#define PP_STORE_CHUNK(CH, BUF)                                                                  \
    {                                                                                            \
        float* ib_ = il + (BUF) * C::LDS_IN;                                                     \
        const int c0_ = (CH) * KC;                                                               \
        _Pragma("unroll") for (int r = 0; r < C::PR; ++r) {                                      \
            if (loff[r] >= 0) {                                                                  \
                const bool inb_ = (vmask >> r) & 1u;                                             \
                _Pragma("unroll") for (int c = 0; c < KC; ++c) {                                 \
                    float v_ = xv[r][c];                                                         \
                    if (p.pre != PRE_RAW) v_ = fmaxf(fmaf(v_, scl[c0_ + c], shl[c0_ + c]), 0.f); \
                    ib_[c * C::CS + loff[r]] = inb_ ? v_ : 0.f;                                  \
                }                                                                                \
            }                                                                                    \
        }                                                                                        \
        f32x4* wb_ = reinterpret_cast<f32x4*>(wl + (BUF) * C::LDS_W);                            \
        _Pragma("unroll") for (int r = 0; r < C::WR; ++r) {                                      \
            const int e_ = tid + r * C::THREADS;                                                 \
            if (e_ < C::W4) wb_[e_] = wv[r];                                                     \
        }                                                                                        \
    }

    // One register set holds the NEXT chunk: it is written to the other LDS buffer right AFTER the barrier that opens a
    // chunk (its loads were issued a whole chunk earlier, so the wait is free), and the loads of chunk ch+2 are
    // re-issued at once -- they have the MFMA steps of this chunk plus the barrier to land.  (Writing at the END of
    // the chunk, as the first version did, gave the loads only the chunk's own MFMA time and exposed the rest.)
    if (nchunk > 0) PP_LOAD_CHUNK(0)
    __syncthreads(); // scl/shl visible
    if (nchunk > 0) PP_STORE_CHUNK(0, 0)
    if (nchunk > 1) PP_LOAD_CHUNK(1)
    __syncthreads();

    for (int ch = 0; ch < nchunk; ++ch) {
        const int buf = ch & 1;
        __builtin_amdgcn_s_setprio(1);
        if (ch + 1 < nchunk) {
            PP_STORE_CHUNK(ch + 1, buf ^ 1)
            if (ch + 2 < nchunk) PP_LOAD_CHUNK(ch + 2)
        }
        const float* ib = il + buf * C::LDS_IN;
        const float* wb = wl + buf * C::LDS_W;
        // Operand reads run ONE STEP AHEAD of the MFMAs that consume them (two register sets, order
        // pinned with sched_barrier): left alone, hipcc issues each step's ds_reads right before its
        // MFMAs and every step eats the LDS latency.
        constexpr int NS = KS * KS * (KC / 4);
        float a[2][MT], b[2][NT];
#define PP_LOAD_OPS(S, SET)                                                                          \
    {                                                                                                \
        constexpr int tap_ = (S) / (KC / 4), c4_ = (S) % (KC / 4);                                   \
        constexpr int ky_ = tap_ / KS, kx_ = tap_ % KS;                                              \
        constexpr int tapoff_ = ky_ * C::IWP + ((STRIDE == 2) ? ((kx_ & 1) * C::HALF + (kx_ >> 1)) : kx_); \
        _Pragma("unroll") for (int i = 0; i < MT; ++i) a[SET][i] = wb[(tap_ * KC + c4_ * 4) * C::BMP + aoff + i * 16]; \
        _Pragma("unroll") for (int j = 0; j < NT; ++j) b[SET][j] = ib[toff[j] + c4_ * 4 * C::CS + tapoff_]; \
    }
        PP_LOAD_OPS(0, 0)
        __builtin_amdgcn_s_setprio(0);
        pp_steps<0, NS>([&](auto S) {
            constexpr int s_ = decltype(S)::value;
            constexpr int cur = s_ & 1;
            if constexpr (s_ + 1 < NS) PP_LOAD_OPS(s_ + 1, cur ^ 1)
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int j = 0; j < NT; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[cur][i], b[cur][j], acc[i][j], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        });
#undef PP_LOAD_OPS
        __syncthreads();
    }
    __builtin_amdgcn_s_setprio(1); // epilogue

    // ---- epilogue ----
    const size_t out_plane = (size_t)p.Hout * p.Wout;
    float ssum[MT][4], ssq[MT][4];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) { ssum[i][r] = 0.f; ssq[i][r] = 0.f; }

#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int row0 = co0 + wm * MT * 16 + i * 16 + kq * 4; // first of this lane's 4 rows
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const bool ok = (opx[j] < p.Wout) && (opy[j] < p.Hout) && (row0 < p.Cout);
            if (!ok) continue;
            const size_t pix = (size_t)opy[j] * p.Wout + opx[j];
            f32x4 v = acc[i][j];
            if (EPI == EPI_PLAIN) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const size_t o = (size_t)(row0 + r) * out_plane + pix;
                    float x = v[r];
                    if (gres) x += gres[o];
                    gout[o] = x;
                    ssum[i][r] += x;
                    ssq[i][r] += x * x;
                }
            } else if (EPI == EPI_UP2) { // rows (co*4 + dy*2 + dx) -> out[co][2y+dy][2x+dx]
                const int co = row0 >> 2;
                const size_t W2 = (size_t)p.Wout * 2;
                float* o = gout + (size_t)co * out_plane * 4 + (size_t)(2 * opy[j]) * W2 + 2 * opx[j];
                *reinterpret_cast<float2*>(o) = make_float2(v[0], v[1]);
                *reinterpret_cast<float2*>(o + W2) = make_float2(v[2], v[3]);
#pragma unroll
                for (int r = 0; r < 4; ++r) { ssum[i][0] += v[r]; ssq[i][0] += v[r] * v[r]; }
            } else if (EPI == EPI_UP4) { // rows (co*16 + dy*4 + dx) -> out[co][4y+dy][4x+dx]
                const int co = row0 >> 4, dy = (row0 >> 2) & 3;
                const size_t W4o = (size_t)p.Wout * 4;
                float* o = gout + (size_t)co * out_plane * 16 + (size_t)(4 * opy[j] + dy) * W4o + 4 * opx[j];
                *reinterpret_cast<float4*>(o) = make_float4(v[0], v[1], v[2], v[3]);
#pragma unroll
                for (int r = 0; r < 4; ++r) { ssum[i][0] += v[r]; ssq[i][0] += v[r] * v[r]; }
            } else { // EPI_HEAD: rows = [cls 9 | box 63 | dir 18], outputs ordered (anchor, x, y[, code])
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = row0 + r;
                    if (row >= p.n_rows) continue;
                    const float x = v[r] + p.bias[row];
                    if (row < p.n_cls) {
                        gout[(size_t)row * out_plane + pix] = x;
                    } else if (row < p.n_cls + p.n_box) {
                        const int q = row - p.n_cls, a = q / 7, k = q - a * 7;
                        gbox[((size_t)a * out_plane + pix) * 7 + k] = x;
                    } else {
                        const int q = row - p.n_cls - p.n_box, a = q >> 1, k = q & 1;
                        gdir[((size_t)a * out_plane + pix) * 2 + k] = x;
                    }
                }
            }
        }
    }

    if (EPI != EPI_HEAD && gstat) {
        // reduce over the 16 pixel lanes, then over the WN waves through LDS, then fp64 atomics
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float s = ssum[i][r], q = ssq[i][r];
                s = row16_sum(s);
                q = row16_sum(q);
                if (m == 0) {
                    const int lr = wm * MT * 16 + i * 16 + kq * 4 + r; // local row
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
            int ch;
            if (EPI == EPI_UP2) { if (lr & 3) continue; ch = row >> 2; }
            else if (EPI == EPI_UP4) { if (lr & 3) continue; ch = row >> 4; }
            else ch = row;
            double* dst = gstat + ((size_t)(blockIdx.x % NREP) * p.stat_C + ch) * 2;
            atomicAdd(dst, s);
            atomicAdd(dst + 1, q);
        }
    }
}

// ------------------------------------------------------------------------------------------
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
// ------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------
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
// ------------------------------------------------------------------------------------------
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

// ------------------------------------------------------------------------------------------
// 1x1 contractions (the three ConvTranspose(k = s) upsamplers and the shared head) as a persistent,
// barrier-free GEMM:  D[rows, pixel] = W[rows, K] * relu(norm(X[K, pixel]))
// * the [K][BM] weight slab of the workgroup's row block stays in LDS for the whole launch
//   (head: 320 x 96, deconv3: 256 x 128 -> up to 147 KB of the 160 KB)
// * activations never touch LDS: lane (pixel m, channel c+kq) loads its B operand straight from
//   global memory into a 4-step register ring, applies the producer's normalisation + ReLU in
//   registers, and feeds the MFMAs -- every wave streams on its own, no workgroup barrier
// * pixels are flattened (a 1x1 conv has no neighbourhood), N-tile = 16 consecutive pixels
// ------------------------------------------------------------------------------------------
// PREC (the reference's deployed path is TensorRT FP16, framework/trt_utils.py:30): 0 = fp32 MFMA (exact);
// 1 = split-bf16 "bf16x3": x = hi + lo with hi = bf16(x), lo = bf16(x - hi), a*b ~ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi on
// v_mfma_f32_16x16x16_bf16 with fp32 accumulation (~2^-16 relative per product: fp32-equivalent for this network, three MFMAs at
// 8x the fp32-MFMA rate); 2 = plain bf16 operands (one MFMA, ~2^-8 per product); 3 = fp16 operands on v_mfma_f32_16x16x16_f16
// (~2^-11 per product: the arithmetic of the reference's TensorRT FP16 engines).
// Activations stay fp32 in HBM: normalise + ReLU in fp32, then split / round while staging.  The weight slab in LDS is
// [K/16][hi|lo][k-group 0..3][BMP rows][4 bf16] -- the same bytes as the fp32 slab.
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pk_bf16(float a, float b) // v_cvt_pk_bf16_f32 (round to nearest even)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){a, b}, bf16x2_t));
}
__device__ __forceinline__ unsigned pk_f16(float a, float b) // round to nearest even (v_cvt_pk_f16_f32 on gfx950)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){a, b}, f16x2_t));
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

// y = relu(x*scale+shift) (scale/shift from the producer's statistics), plus statistics of y.
// Used for the [conv, norm, relu] head of each block, whose output is both a residual and the
// input of the next InstanceNorm (pointpillars8_shared.py:133-137).
// x16: the input tensor is fp16 (the concat buffer under pp_set_precision 4); y is fp32 either way
__global__ void __launch_bounds__(256) norm_relu_stats(const float* __restrict__ x, float* __restrict__ y, int C, int HW,
                                                       int pre, const double* __restrict__ pre_acc,
                                                       const float* __restrict__ pre_scale, const float* __restrict__ pre_shift,
                                                       double inv_n, float eps, double* __restrict__ stat_acc,
                                                       size_t x_fs, size_t acc_fs, int x16, int y16)
{
    const int c = blockIdx.y;
    const _Float16* xh = reinterpret_cast<const _Float16*>(x) + blockIdx.z * x_fs;
    _Float16* yh = reinterpret_cast<_Float16*>(y) + blockIdx.z * x_fs;
    x += blockIdx.z * x_fs;
    y += blockIdx.z * x_fs;
    if (pre_acc) pre_acc += blockIdx.z * acc_fs;
    if (stat_acc) stat_acc += blockIdx.z * acc_fs;
    float sc, sh;
    if (pre == PRE_STATS) {
        double s = 0.0, q = 0.0;
        for (int r = 0; r < NREP; ++r) {
            s += pre_acc[((size_t)r * C + c) * 2];
            q += pre_acc[((size_t)r * C + c) * 2 + 1];
        }
        double mean = s * inv_n, var = q * inv_n - mean * mean;
        var = var > 0.0 ? var : 0.0;
        double rstd = 1.0 / sqrt(var + (double)eps);
        sc = (float)rstd;
        sh = (float)(-mean * rstd);
    } else {
        sc = pre_scale[c];
        sh = pre_shift[c];
    }
    float s = 0.f, q = 0.f;
    double ds = 0.0, dq = 0.0;
    int it = 0;
    if ((HW & 3) == 0) { // planes of every shipped configuration: 16-byte aligned rows of float4
        const float4* xi = reinterpret_cast<const float4*>(x + (size_t)c * HW);
        float4* yo = reinterpret_cast<float4*>(y + (size_t)c * HW);
        const int n4 = HW >> 2;
        const uint2* xi16 = reinterpret_cast<const uint2*>(xh + (size_t)c * HW);
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += gridDim.x * blockDim.x) {
            float4 v;
            if (x16) {
                const f16x4_t h = __builtin_bit_cast(f16x4_t, xi16[i]);
                v = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
            } else v = xi[i];
            v.x = fmaxf(fmaf(v.x, sc, sh), 0.f);
            v.y = fmaxf(fmaf(v.y, sc, sh), 0.f);
            v.z = fmaxf(fmaf(v.z, sc, sh), 0.f);
            v.w = fmaxf(fmaf(v.w, sc, sh), 0.f);
            if (y16) reinterpret_cast<uint2*>(yh + (size_t)c * HW)[i] = (uint2){pk_f16(v.x, v.y), pk_f16(v.z, v.w)}; // statistics below: of the fp32 values
            else yo[i] = v;
            s += (v.x + v.y) + (v.z + v.w);
            q += (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
            if (++it == 8) { ds += s; dq += q; s = 0.f; q = 0.f; it = 0; }
        }
    } else { // odd planes (e.g. a 9 x 11 level-2 map): channel c starts at a 4-byte aligned address only -> scalar loop
        const float* xi = x + (size_t)c * HW;
        float* yo = y + (size_t)c * HW;
        for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < HW; i += gridDim.x * blockDim.x) {
            const float v = fmaxf(fmaf(x16 ? (float)xh[(size_t)c * HW + i] : xi[i], sc, sh), 0.f);
            if (y16) yh[(size_t)c * HW + i] = (_Float16)v; else yo[i] = v;
            s += v;
            q += v * v;
            if (++it == 32) { ds += s; dq += q; s = 0.f; q = 0.f; it = 0; }
        }
    }
    ds += s;
    dq += q;
    if (!stat_acc) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        ds += __shfl_xor(ds, o);
        dq += __shfl_xor(dq, o);
    }
    __shared__ double rs[4], rq[4];
    if ((threadIdx.x & 63) == 0) { rs[threadIdx.x >> 6] = ds; rq[threadIdx.x >> 6] = dq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* dst = stat_acc + ((size_t)(blockIdx.x % NREP) * C + c) * 2;
        atomicAdd(dst, rs[0] + rs[1] + rs[2] + rs[3]);
        atomicAdd(dst + 1, rq[0] + rq[1] + rq[2] + rq[3]);
    }
}

// ------------------------------------------------------------------------------------------
// host side: network description, weight packing, launch plans
// ------------------------------------------------------------------------------------------
template <int KS, int STRIDE, int TW, int WM, int WN, int MT, int NT, int BTX, int KC, int EPI>
Variant make_variant()
{
    using C = ConvCfg<KS, STRIDE, TW, WM, WN, MT, NT, BTX, KC, EPI>;
    Variant v;
    v.kern = conv_mfma<KS, STRIDE, TW, WM, WN, MT, NT, BTX, KC, EPI>;
    v.bm = C::BM; v.bmp = C::BMP; v.pw = C::PW; v.ph = C::PH; v.kc = KC; v.threads = C::THREADS;
    v.waves = WM * WN; v.pairs = MT * NT;
    v.lds = (size_t)C::LDS_FLOATS * sizeof(float);
    snprintf(v.name, sizeof(v.name), "k%ds%d tw%d w%dx%d t%dx%d bx%d kc%d e%d", KS, STRIDE, TW, WM, WN, MT, NT, BTX, KC, EPI);
    return v;
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

struct Layer {
    std::string wkey;
    int kind;   // 0 conv3x3, 1 deconv(up), 2 head
    int cin, cout, stride, up;
    int level;  // pixel grid of the GEMM: 0 = H,W ; 1 = H/2 ; 2 = H/4 (input grid for deconv)
    Variant var;
    float* w = nullptr; // packed device weights
    size_t w_bytes = 0; // size of that image (pack_layer)
    int rows = 0;       // GEMM rows (virtual channels)
};

struct NormRef { // where a consumer finds the producer's normalisation
    int mode = PRE_RAW;
    double* acc = nullptr;
    float* scale = nullptr;
    float* shift = nullptr;
    int C = 0;
    double inv_n = 0.0;
    size_t fs = 0; // doubles between frames of `acc`
    size_t aff_fs = 0; // floats between frames of `scale` / `shift` (0: shared by all frames)
};

struct pp_net {
    std::vector<Layer> layers; // 16 convs, 3 deconvs, head in execution order
    float* buf[3][4] = {};     // per level: 4 activation buffers [C,H,W]
    float* up = nullptr;       // [320,H,W] pre-norm upsampled maps (concat)
    double* stats = nullptr;   // all statistics accumulators, one memset per frame
    float* aff = nullptr;      // [max_batch][2][320] (scale, shift) of the layer about to run (norm_finalize)
    size_t stats_bytes = 0;
    float* bn_scale = nullptr; // BatchNorm variant: all folded (scale, shift) arrays
    float* bn_shift = nullptr;
    float* head_bias = nullptr;
    float* head_bias_perm = nullptr; // head bias in gemm1x1's row order (head_tile_row)
    float* ones = nullptr;
    float* zeros = nullptr;
    int num_cu = 256;
    int eff_prec = 0;   // the precision the launch plan is built for: ctx->precision, except 4 -> 3 when the concat buffer cannot be fp16
    bool up16 = false;  // pp_set_precision 4 with every layer on a 16-bit-tensor tiling: the level buffers and the concat buffer `up` hold fp16
    bool defer_ok = false; // the committed plan can run the deferred head: fp32 mode, 9-anchor head on a gemm1x1 tiling
    Variant cls_var;       // tiling of the cls-only head pass (chosen at pp_commit_weights when defer_ok)
    const float* tap[3] = {}; // block outputs of the last pp_run_backbone pass (what the three upsamplers read): pp_backbone_taps
    float* unit_tap = nullptr; // copy hook of pp_backbone_block_taps: caller memory f32[5][256][H/4][W/4] for block 3's unit inputs (null: inert)
    double* dbg_stats = nullptr; // statistics accumulators of pp_debug_layer (allocated on its first call that asks for statistics)
    int w4_strips = -1; // PP_W4_STRIPS, read once at pp_create: -1 cost model, 0 never, 2 whenever whole main tiles exist (parity tests of the strip tiles)
};

const int kC[3] = {64, 128, 256};

// Tiling menu.  The 16-pixel N-tile is TW x (16/TW); a workgroup covers BTX x BTY tiles.  The maps of
// eight_20cm are 400/200/100 = 16*25 / 8*25 / 4*25, so NT=5 shapes tile them exactly; the 4x4 / 2x2 shapes
// are the general fallback (edge tiles masked).  Which entry runs a layer is MEASURED on the device at
// pp_commit_weights (autotune below); the cost model only breaks ties / serves PP_AUTOTUNE=0.
template <int KS, int STRIDE, int KC, int EPI>
void conv_menu(std::vector<Variant>& m)
{
    constexpr int KH = (KC >= 8) ? KC / 2 : KC;
    //                            TW WM WN MT NT BTX
    m.push_back(make_variant<KS, STRIDE, 16, 1, 4, 4, 5, 1, KC, EPI>()); // 16x20 px, 64 rows
    m.push_back(make_variant<KS, STRIDE, 16, 1, 4, 4, 5, 1, KH, EPI>());
    m.push_back(make_variant<KS, STRIDE, 16, 1, 4, 4, 4, 1, KC, EPI>()); // 16x16 px, 64 rows
    m.push_back(make_variant<KS, STRIDE, 16, 2, 2, 2, 5, 1, KH, EPI>()); // 16x10 px, 64 rows, light waves
    m.push_back(make_variant<KS, STRIDE, 16, 1, 4, 2, 5, 1, KC, EPI>()); // 16x20 px, 32 rows
    m.push_back(make_variant<KS, STRIDE, 8, 2, 2, 4, 5, 5, KC, EPI>());  // 40x4 px, 128 rows
    m.push_back(make_variant<KS, STRIDE, 8, 2, 2, 4, 5, 5, KH, EPI>());
    m.push_back(make_variant<KS, STRIDE, 8, 4, 1, 2, 5, 5, KC, EPI>());  // 40x2 px, 128 rows, light waves
    m.push_back(make_variant<KS, STRIDE, 8, 2, 2, 4, 2, 2, KC, EPI>());  // 16x4 px, 128 rows
    m.push_back(make_variant<KS, STRIDE, 8, 1, 4, 4, 4, 2, KC, EPI>());  // 16x16 px, 64 rows
    m.push_back(make_variant<KS, STRIDE, 4, 4, 1, 2, 5, 5, KC, EPI>());  // 20x4 px, 128 rows
    m.push_back(make_variant<KS, STRIDE, 4, 4, 1, 2, 5, 5, KH, EPI>());
    m.push_back(make_variant<KS, STRIDE, 4, 8, 1, 1, 5, 5, KC, EPI>());  // 20x4 px, 128 rows, 8 light waves
    m.push_back(make_variant<KS, STRIDE, 4, 2, 2, 4, 5, 5, KC, EPI>());  // 20x8 px, 128 rows
    m.push_back(make_variant<KS, STRIDE, 4, 2, 2, 4, 2, 2, KC, EPI>());  // 8x8 px, 128 rows
    m.push_back(make_variant<KS, STRIDE, 4, 2, 2, 2, 2, 2, KC, EPI>());  // 8x8 px, 64 rows
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

void layer_menu(int kind, int stride, int up, std::vector<Variant>& menu, int cin = 0, bool roofline_layer = false, bool head9 = true, int prec = 0,
                bool first_conv = false)
{
    const bool g1ok = cin % 32 == 0; // gemm1x1 runs K in rings of 8 quad-steps without a tail
    // reduced-precision modes (pp_set_precision): the 1x1 contractions -- the three ConvTranspose(k = s) upsamplers and the
    // 9-anchor head -- run their bf16x3 / bf16 / fp16 gemm1x1 tilings, the 3x3 convolutions the 16-bit operand kernels of
    // conv16.hip.  A layer whose shape none of them takes (autotune_layer checks variant_ok / shape_ok) falls back to the
    // fp32 menu below, and pp_layer_tilings shows it.
    if (prec && g1ok && (kind == 1 || (kind == 2 && head9))) {
        if (prec == 1) lp_menu<1>(kind, up, menu); else if (prec == 2) lp_menu<2>(kind, up, menu); else if (prec == 3) lp_menu<3>(kind, up, menu);
        else lp_menu<3, true>(kind, up, menu);
        return;
    }
    if (prec && kind == 0 && cin % 16 == 0) {
        // fp16s: the fp16-operand kernels on fp16 tensors; the first conv reads the fp32 PFN rows / canvas and writes fp16
        if (prec == 4) conv16_menu(stride, 3, menu, first_conv ? 2 : 3);
        else conv16_menu(stride, prec, menu);
        return;
    }
    if (kind == 2) {
        // the persistent 1x1 GEMM's head epilogue (head_tile_row) is laid out for the reference's 9 anchors per location
        if (g1ok && head9) { menu.push_back(make_g1<6, 4, EPI_HEAD>()); menu.push_back(make_g1<3, 4, EPI_HEAD>()); }
        menu.push_back(make_variant<1, 1, 16, 1, 4, 6, 5, 1, 16, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 16, 1, 4, 6, 2, 1, 16, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 16, 2, 2, 3, 5, 1, 16, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 16, 2, 4, 3, 5, 1, 32, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 8, 1, 4, 6, 2, 1, 16, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 8, 2, 2, 3, 4, 2, 16, EPI_HEAD>());
    } else if (kind == 1) {
        if (up == 1) { conv_menu<1, 1, 16, EPI_PLAIN>(menu); if (g1ok) { menu.push_back(make_g1<4, 4, EPI_PLAIN>()); menu.push_back(make_g1<2, 4, EPI_PLAIN>()); } }
        else if (up == 2) { conv_menu<1, 1, 16, EPI_UP2>(menu); if (g1ok) { menu.push_back(make_g1<4, 4, EPI_UP2>()); menu.push_back(make_g1<8, 4, EPI_UP2>()); } }
        else { conv_menu<1, 1, 16, EPI_UP4>(menu); if (g1ok) { menu.push_back(make_g1<4, 4, EPI_UP4>()); menu.push_back(make_g1<8, 4, EPI_UP4>()); } }
    } else if (stride == 2) {
        conv_menu<3, 2, 8, EPI_PLAIN>(menu);
    } else {
        conv_menu<3, 1, 8, EPI_PLAIN>(menu);
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
        // one wave per SIMD, 64 rows, 3-deep ring (even maps, Cout a multiple of 64 only -- see variant_ok)
        menu.push_back(make_wino4<4, 2, 8>(roofline_layer));       // 16x16 px
        menu.push_back(make_wino4<8, 1, 8>(roofline_layer));       // 16x16 px, 8x2-tile N-tiles
        menu.push_back(make_wino4<8, 2, 8>(roofline_layer));       // 32x8 px
        if (cin % 32 == 0) wino6_menu(menu, roofline_layer);       // Winograd F(4x4,3x3), 16x16 px (wino6.hip)
    }
}

// strip tilings of wino4 / wino6 (launch_conv): a map that is not a multiple of the main tile (16x16 px) is covered by whole main
// tiles plus a right strip of 4 x 64 px tiles and a bottom strip of 64 x 4 px tiles -- 100 x 100: 36 + 2 + 2 tiles instead of
// 49 mostly-empty ones
static const Variant& strip_v(Family f) // 4 px wide, 64 px tall
{
    static const Variant w4 = make_wino4<2, 1, 8>(false), w6 = wino6_strip_v();
    return f == Family::Wino6 ? w6 : w4;
}
static const Variant& strip_h(Family f) // 64 px wide, 4 px tall
{
    static const Variant w4 = make_wino4<16, 2, 8>(false), w6 = wino6_strip_h();
    return f == Family::Wino6 ? w6 : w4;
}

// cost model: wavefronts are dealt to 1024 SIMDs; a SIMD's time ~ (its wave count) x (tile pairs per wave).
double model_cost(const Variant& v, int rows, int Hout, int Wout)
{
    const double blocks = (double)pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph) * pp_div_up(rows, v.bm);
    const double waves = blocks * v.waves;
    double cost = std::ceil(waves / 1024.0) * v.pairs;
    if (waves < 1536.0) cost *= 1.15;          // a lone wave per SIMD cannot hide its own staging
    cost *= 1.0 + 0.02 * (20.0 / v.pairs);     // smaller wave tiles re-read operands more often
    return cost;
}

// ---- the per-family rules of the tuner and the launcher ----
// rows: wino4, conv16 and wino6 tile whole row blocks; the others clip their last block
bool variant_ok(const Variant& v, int rows)
{
    switch (v.family) {
    case Family::Wino4:
    case Family::Conv16:
    case Family::Wino6: return rows % v.bm == 0;
    default: return v.bm <= ((rows + 63) / 64) * 64;
    }
}
// shape limits of a tiling family
bool shape_ok(const Variant& v, int Hin, int Win, int Wout)
{
    switch (v.family) {
    case Family::Wino4: return !(Wout & 1); // float2 row stores (even output width)
    // gemm1x1 feeds four N-tiles from one dwordx4 of 4 consecutive pixels of the input plane (pixel count a multiple of 4 -- a
    // 9 x 11 map has 99); with a 16-bit tensor it has no path for maps that are not a multiple of 4 wide
    case Family::Gemm1x1: return !((Hin * Win) & 3) && !(v.io16 && (Wout & 3));
    // conv16 fetches its patches as aligned pixel quads and stores pixel quads (input and output width multiples of 4)
    case Family::Conv16: return !((Win & 3) || (Wout & 3));
    // wino6 works on whole 4x4 output tiles and dwordx4 rows (maps a multiple of 4 in both directions; stride 1: Hin = Hout)
    case Family::Wino6: return !((Wout & 3) || (Hin & 3));
    default: return true;
    }
}
// LDS bytes of a persistent 1x1 GEMM for a given K
size_t g1_lds(const Variant& v, int K) { return ((size_t)K * v.bmp + (size_t)8 * 2 * K) * sizeof(float); }
// LDS bytes of a launch of v on a layer with cin input channels (gemm1x1 keeps the whole [K][BM] weight slab)
size_t layer_lds(const Variant& v, int cin) { return v.family == Family::Gemm1x1 ? g1_lds(v, cin) : v.lds; }
// One frame per launch: the families that finalise the producer's statistics in their own prologue, instead of a norm_finalize
// launch in front of the layer -- 14 launches of 4.7 us + a boundary each per frame at batch 1.  (Batched launches keep
// norm_finalize: a persistent workgroup would redo the fp64 finalisation at every frame change.)
bool finalises_in_prologue(Family f)
{
    switch (f) {
    case Family::Direct:
    case Family::Gemm1x1:
    case Family::Wino4:
    case Family::Wino6: return true;
    default: return false;
    }
}
// MFMA flops a tiling executes per algorithmic flop of the direct convolution
double executed_ratio(const Variant& v)
{
    switch (v.family) {
    case Family::Wino6: return 0.25;
    case Family::Wino:
    case Family::Wino4: return 4.0 / 9.0;
    case Family::Conv16: return v.prec == 1 ? 3.0 : 1.0; // bf16x3: three MFMAs per product
    default: return 1.0;
    }
}

Variant pick_variant(int kind, int stride, int up, int rows, int Hout, int Wout, bool head9 = true)
{
    std::vector<Variant> menu;
    layer_menu(kind, stride, up, menu, 0, false, head9, 0);
    double best = 1e30;
    Variant bv = menu[0];
    for (const Variant& v : menu) {
        if (!variant_ok(v, rows) || (v.family != Family::Direct && v.family != Family::Wino)) continue; // persistent kernels are only chosen by measurement
        const double c = model_cost(v, rows, Hout, Wout);
        if (c < best) { best = c; bv = v; }
    }
    // Without on-device tuning (PP_AUTOTUNE=0) prefer what the tuner settles on for these layer kinds on MI355X;
    // the cost model above only ranks the direct tilings.
    const char* prefer = (kind == 0 && stride == 1) ? "wino tw8 w1x4 bx1 kc8"
                         : (kind == 1 && up == 2)   ? "g1x1 m4 n4 e1"
                         : (kind == 1 && up == 4)   ? "g1x1 m4 n4 e2"
                         : (kind == 2 && head9)     ? "g1x1 m6 n4 e3"
                                                    : nullptr;
    if (prefer)
        for (const Variant& v : menu)
            if (variant_ok(v, rows) && shape_ok(v, Hout, Wout, Wout) && !strcmp(v.name, prefer)) return v;
    return bv;
}

// Row order of the head inside gemm1x1.  A lane of the 16x16 MFMA tile owns 4 CONSECUTIVE tile rows (kq*4 + r), so
// the 90 head rows are dealt to the 24 four-row groups such that a group's values are adjacent in the output:
//   groups 0..8   box (a = g)      k = 0..3                      -> one 16-byte store per pixel
//   groups 9..17  box (a = g - 9)  k = 4..6, then cls(a)         -> one 12-byte store per pixel + cls as a pixel quad
//   groups 18..22 dir (a = 2d, 2d+1), both logits each           -> two 8-byte stores per pixel
//   group 23      padding
// (natural order: cls 0..8, box 9 + 7a + k, dir 72 + 2a + k, head rows 90..95 are zero).  With the natural order
// the 81 box/dir rows cost 4 scalar stores each per lane -- 333 scattered store instructions per 64 pixels, whose
// completion the next item's first loads had to wait for (vmcnt is in order): 38 % of the head's wave time.
// GEMM rows of the head for na anchors per location: cls na | box 7 na | dir 2 na, padded to whole 96-row blocks (the
// head tilings are 96 rows tall; the reference's 9 anchors give 90 -> 96)
static inline int head_rows(int na) { return ((10 * na + 95) / 96) * 96; }

static inline int head_tile_row(int t)
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

// index_positions: the transform (U = G g G^T of the Winograd families, the identity elsewhere) is replaced by position indices --
// element k of the transformed [rows][cin][taps_eff] array holds the float k + 1 -- so the image that comes out is the layout alone
// (layer_position_map); conv3x3 layers on fp32 tilings only
int pack_layer(pp_ctx* ctx, Layer& L, bool index_positions = false)
{
    const Variant& v = L.var;
    const int ks = (L.kind == 0) ? 3 : 1;
    const int taps = ks * ks;
    auto it = ctx->host_w.find(L.wkey);
    std::vector<float> rowsW; // [rows][cin][taps]
    int rows = 0;
    if (L.kind == 0) {
        if (it == ctx->host_w.end() || (int64_t)it->second.data.size() != (int64_t)L.cout * L.cin * 9)
            return pp_fail(ctx, PP_E_NAME, ("missing/mis-shaped weight " + L.wkey).c_str());
        rows = L.cout;
        rowsW = it->second.data; // [cout][cin][3][3]
    } else if (L.kind == 1) {
        const int u2 = L.up * L.up;
        if (it == ctx->host_w.end() || (int64_t)it->second.data.size() != (int64_t)L.cin * L.cout * u2)
            return pp_fail(ctx, PP_E_NAME, ("missing/mis-shaped weight " + L.wkey).c_str());
        rows = L.cout * u2; // ConvTranspose weight [cin][cout][k][k] -> row (co*u2 + dy*u + dx)
        rowsW.resize((size_t)rows * L.cin);
        const std::vector<float>& s = it->second.data;
        for (int ci = 0; ci < L.cin; ++ci)
            for (int co = 0; co < L.cout; ++co)
                for (int d = 0; d < u2; ++d) rowsW[((size_t)co * u2 + d) * L.cin + ci] = s[((size_t)ci * L.cout + co) * u2 + d];
    } else {
        const int na = ctx->cfg.num_anchor_per_loc;
        rows = head_rows(na);
        rowsW.assign((size_t)rows * L.cin, 0.f);
        const char* names[3] = {"heads.conv_cls.weight", "heads.conv_box.weight", "heads.conv_dir.weight"};
        const int cnt[3] = {na, 7 * na, 2 * na};
        int r0 = 0;
        for (int h = 0; h < 3; ++h) {
            auto w = ctx->host_w.find(names[h]);
            if (w == ctx->host_w.end() || (int64_t)w->second.data.size() != (int64_t)cnt[h] * L.cin)
                return pp_fail(ctx, PP_E_NAME, (std::string("missing/mis-shaped weight ") + names[h]).c_str());
            memcpy(&rowsW[(size_t)r0 * L.cin], w->second.data.data(), sizeof(float) * cnt[h] * L.cin);
            r0 += cnt[h];
        }
    }
    L.rows = rows;
    if (v.family == Family::Wino6) { // F(4x4,3x3): U = G g G^T in the order the four waves fetch their positions (wino6.hip)
        std::vector<float> pk6;
        wino6_pack(rowsW.data(), rows, L.cin, pk6, index_positions);
        if (L.w) (void)hipFree(L.w);
        PP_HIP(hipMalloc((void**)&L.w, pk6.size() * sizeof(float)));
        L.w_bytes = pk6.size() * sizeof(float);
        PP_HIP(hipMemcpy(L.w, pk6.data(), pk6.size() * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
    int taps_eff = taps;
    if (v.family == Family::Wino || v.family == Family::Wino4) { // U = G g G^T per (cout, cin), fp64 on the host; position xi = 4*a + b
        static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
        std::vector<float> u((size_t)rows * L.cin * 16);
        for (size_t rc = 0; rc < (size_t)rows * L.cin; ++rc) {
            const float* g = &rowsW[rc * 9];
            double t[4][3];
            for (int a = 0; a < 4; ++a)
                for (int j = 0; j < 3; ++j) t[a][j] = G[a][0] * g[0 * 3 + j] + G[a][1] * g[1 * 3 + j] + G[a][2] * g[2 * 3 + j];
            for (int a = 0; a < 4; ++a)
                for (int b = 0; b < 4; ++b) u[rc * 16 + a * 4 + b] = (float)(t[a][0] * G[b][0] + t[a][1] * G[b][1] + t[a][2] * G[b][2]);
        }
        rowsW.swap(u);
        taps_eff = 16;
    }
    if (index_positions)
        for (size_t k = 0; k < rowsW.size(); ++k) rowsW[k] = (float)(k + 1);
    if (v.family == Family::Gemm1x1 && L.kind == 2) { // head under gemm1x1: rows in head_tile_row order
        std::vector<float> perm((size_t)96 * L.cin, 0.f);
        for (int t = 0; t < 96; ++t) {
            const int src = head_tile_row(t);
            if (src >= 0) memcpy(&perm[(size_t)t * L.cin], &rowsW[(size_t)src * L.cin], sizeof(float) * L.cin);
        }
        rowsW.swap(perm);
    }
    if (v.family == Family::Conv16) { // conv16: [row block][cin/16][image: hi (| lo for bf16x3)][tap][k-half][BM rows][8 x 16 bit] = the LDS image of a step
        auto bf16 = [](float f) -> uint16_t { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); };
        auto bf16f = [](uint16_t h) -> float { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
        auto f16 = [](float f) -> uint16_t { const _Float16 h = (_Float16)f; uint16_t u; memcpy(&u, &h, 2); return u; }; // round to nearest even
        const int nimg = (v.prec == 1) ? 2 : 1, nblk = rows / v.bm, nch = L.cin / 16;
        std::vector<uint16_t> pk((size_t)nblk * nch * nimg * 9 * 2 * v.bm * 8, 0);
        for (int b = 0; b < nblk; ++b)
            for (int ch = 0; ch < nch; ++ch)
                for (int t = 0; t < 9; ++t)
                    for (int h = 0; h < 2; ++h)
                        for (int mm = 0; mm < v.bm; ++mm)
                            for (int j = 0; j < 8; ++j) {
                                const float w = rowsW[((size_t)(b * v.bm + mm) * L.cin + ch * 16 + h * 8 + j) * 9 + t];
                                const size_t o = (((size_t)(t * 2 + h)) * v.bm + mm) * 8 + j;
                                const size_t img0 = (((size_t)b * nch + ch) * nimg) * (size_t)(9 * 2 * v.bm * 8);
                                if (v.prec == 3) pk[img0 + o] = f16(w);
                                else {
                                    const uint16_t hi = bf16(w);
                                    pk[img0 + o] = hi;
                                    if (nimg == 2) pk[img0 + (size_t)(9 * 2 * v.bm * 8) + o] = bf16(w - bf16f(hi));
                                }
                            }
        if (L.w) (void)hipFree(L.w);
        PP_HIP(hipMalloc((void**)&L.w, pk.size() * sizeof(uint16_t)));
        L.w_bytes = pk.size() * sizeof(uint16_t);
        PP_HIP(hipMemcpy(L.w, pk.data(), pk.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        return 0;
    }
    if (v.family == Family::Gemm1x1 && v.prec) { // [row block][K/16][hi|lo][k-group][BMP][4 bf16]: the byte count of the fp32 slab
        auto bf16 = [](float f) -> uint16_t { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); };
        auto bf16f = [](uint16_t h) -> float { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; };
        const int nb_ = pp_div_up(rows, v.bm), nkb = L.cin / 16;
        std::vector<uint16_t> pk4((size_t)nb_ * nkb * 2 * 4 * v.bmp * 4, 0);
        for (int b = 0; b < nb_; ++b)
            for (int kb = 0; kb < nkb; ++kb)
                for (int q = 0; q < 4; ++q)
                    for (int mm = 0; mm < v.bm; ++mm) {
                        const int row = b * v.bm + mm;
                        if (row >= rows) continue;
                        for (int t = 0; t < 4; ++t) {
                            const float w = rowsW[(size_t)row * L.cin + kb * 16 + q * 4 + t];
                            uint16_t hi = bf16(w);
                            if (v.prec == 3) { const _Float16 h16 = (_Float16)w; memcpy(&hi, &h16, 2); } // fp16 operands: the hi image alone is used
                            const uint16_t lo = bf16(w - bf16f(hi));
                            pk4[(((((size_t)b * nkb + kb) * 2 + 0) * 4 + q) * v.bmp + mm) * 4 + t] = hi;
                            pk4[(((((size_t)b * nkb + kb) * 2 + 1) * 4 + q) * v.bmp + mm) * 4 + t] = lo;
                        }
                    }
        if (L.w) (void)hipFree(L.w);
        PP_HIP(hipMalloc((void**)&L.w, pk4.size() * sizeof(uint16_t)));
        L.w_bytes = pk4.size() * sizeof(uint16_t);
        PP_HIP(hipMemcpy(L.w, pk4.data(), pk4.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        return 0;
    }
    if (v.family == Family::Gemm1x1) { // [row block][K][BMP]
        const int nb_ = pp_div_up(rows, v.bm);
        std::vector<float> pk3((size_t)nb_ * L.cin * v.bmp, 0.f);
        for (int b = 0; b < nb_; ++b)
            for (int c = 0; c < L.cin; ++c)
                for (int mm = 0; mm < v.bm; ++mm) {
                    const int row = b * v.bm + mm;
                    if (row < rows) pk3[((size_t)b * L.cin + c) * v.bmp + mm] = rowsW[(size_t)row * L.cin + c];
                }
        if (L.w) (void)hipFree(L.w);
        PP_HIP(hipMalloc((void**)&L.w, pk3.size() * sizeof(float)));
        L.w_bytes = pk3.size() * sizeof(float);
        PP_HIP(hipMemcpy(L.w, pk3.data(), pk3.size() * sizeof(float), hipMemcpyHostToDevice));
        return 0;
    }
    const int nblk = pp_div_up(rows, v.bm), nchunk = L.cin / v.kc;
    std::vector<float> pk((size_t)nblk * nchunk * taps_eff * v.kc * v.bmp, 0.f); // LDS image incl. row padding
    for (int b = 0; b < nblk; ++b)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int t = 0; t < taps_eff; ++t)
                for (int k = 0; k < v.kc; ++k)
                    for (int mm = 0; mm < v.bm; ++mm) {
                        const int row = b * v.bm + mm;
                        if (row >= rows) continue;
                        // Winograd image: row = [wm][m][M-tile] so a lane's two A operands are adjacent (ds_read_b64)
                        // wino4 image: row = [m][M-tile 0..3] so a lane's four A operands are one ds_read_b128
                        const int col = (v.family == Family::Wino) ? ((mm >> 5) * 32 + (mm & 15) * 2 + ((mm >> 4) & 1)) : (v.family == Family::Wino4) ? ((mm & 15) * 4 + (mm >> 4)) : mm;
                        pk[((((size_t)b * nchunk + ch) * taps_eff + t) * v.kc + k) * v.bmp + col] =
                            rowsW[((size_t)row * L.cin + ch * v.kc + k) * taps_eff + t];
                    }
    if (L.w) (void)hipFree(L.w);
    PP_HIP(hipMalloc((void**)&L.w, pk.size() * sizeof(float)));
    L.w_bytes = pk.size() * sizeof(float);
    PP_HIP(hipMemcpy(L.w, pk.data(), pk.size() * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// InstanceNorm statistics -> (scale, shift) once per frame and layer, instead of once per workgroup of the
// consuming conv (same fp64 formula the kernels' PRE_STATS prologue uses, so results are bit-identical)
__global__ void __launch_bounds__(320) norm_finalize(const double* __restrict__ acc, size_t acc_fs, int C, double inv_n, float eps,
                                                     float* __restrict__ aff, size_t aff_fs)
{
    const int c = threadIdx.x;
    if (c >= C) return;
    const double* pa = acc + (size_t)blockIdx.x * acc_fs;
    double s = 0.0, q = 0.0;
#pragma unroll
    for (int r = 0; r < NREP; ++r) { s += pa[((size_t)r * C + c) * 2]; q += pa[((size_t)r * C + c) * 2 + 1]; }
    const double mean = s * inv_n;
    double var = q * inv_n - mean * mean;
    var = var > 0.0 ? var : 0.0;
    const double rstd = 1.0 / sqrt(var + (double)eps);
    aff[(size_t)blockIdx.x * aff_fs + c] = (float)rstd;
    aff[(size_t)blockIdx.x * aff_fs + 320 + c] = (float)(-mean * rstd);
}

constexpr size_t STAT_FS = (size_t)24 * NREP * 320 * 2; // doubles of statistics per frame

int launch_conv(pp_ctx* ctx, const Layer& L, const float* in, int Hin, int Win, float* out, const float* res,
                const NormRef& pre, double* stat_acc, int stat_C, int Hout, int Wout, hipStream_t stream,
                float* out_box = nullptr, float* out_dir = nullptr, int B = 1, size_t out_fs = 0, size_t in_fs = 0,
                const int32_t* pmap = nullptr, const float* feat = nullptr, int ts_k = 0)
{
    pp_net* net = (pp_net*)ctx->net;
    ConvP p;
    memset(&p, 0, sizeof(p));
    p.in = in; p.w = L.w; p.out = out; p.res = res;
    p.Cin = L.cin; p.Hin = Hin; p.Win = Win;
    p.Cout = L.rows; p.Hout = Hout; p.Wout = Wout;
    p.pre = pre.mode; p.pre_acc = pre.acc; p.pre_scale = pre.scale; p.pre_shift = pre.shift;
    p.pre_inv_n = pre.inv_n; p.eps = 1e-3f; p.aff_fs = pre.aff_fs;
    p.stat_acc = stat_acc; p.stat_C = stat_C;
    p.bias = (L.kind == 2 && L.var.family == Family::Gemm1x1) ? net->head_bias_perm : net->head_bias; p.out_box = out_box; p.out_dir = out_dir;
    { const int na = ctx->cfg.num_anchor_per_loc; p.n_cls = na; p.n_box = 7 * na; p.n_rows = 10 * na; }
    p.w_bm = net->layers.back().var.bm; p.w_bmp = net->layers.back().var.bmp;
    {   // frame strides of a batched launch (every per-frame tensor is stored [B][...])
        const size_t hw = (size_t)Hout * Wout;
        p.in_fs = in_fs ? in_fs : (size_t)L.cin * Hin * Win;
        p.out_fs = out_fs ? out_fs : (L.kind == 2 ? (size_t)p.n_cls * hw : (size_t)L.rows * hw);
        p.res_fs = p.out_fs;
        p.box_fs = (size_t)p.n_box * hw;
        p.dir_fs = (size_t)2 * p.n_cls * hw;
        p.pre_fs = pre.fs;
        p.stat_fs = STAT_FS;
        p.pmap = pmap; p.feat = feat;
        p.pmap_fs = (size_t)Hin * Win;
        p.feat_fs = (size_t)ctx->cfg.max_voxels * 64;
    }
    const bool fin_in_kernel = B == 1 && finalises_in_prologue(L.var.family);
    if (pre.mode == PRE_STATS && net->aff && L.cin <= 320 && !fin_in_kernel) {
        hipLaunchKernelGGL(norm_finalize, dim3(B), dim3(320), 0, stream, pre.acc, pre.fs, L.cin, pre.inv_n, p.eps, net->aff, (size_t)640);
        p.pre = PRE_AFFINE; p.pre_scale = net->aff; p.pre_shift = net->aff + 320; p.aff_fs = 640;
    }
    const Variant& v = L.var;
    dim3 grid(pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph), pp_div_up(L.rows, v.bm), B);
    p.nb = B;
    const size_t lds_bytes = layer_lds(v, L.cin);
    if (v.family == Family::Gemm1x1 && ((Hin * Win) & 3)) return PP_E_ARG; // gemm1x1 reads pixel quads (choose_variant never offers it for such a plane)
    if (v.family == Family::Gemm1x1) { // persistent: one workgroup per CU, a multiple of the row-block count
        const int ncb = pp_div_up(L.rows, v.bm);
        int g = (net->num_cu * v.wpc / ncb) * ncb;
        if (g < ncb) g = ncb;
        grid = dim3(g, 1, 1);
    }
    if (v.family == Family::Conv16) { // conv16: persistent, one 4-wave workgroup per CU, XCD-contiguous item ranges (grid a multiple of 8)
        if ((size_t)L.rows * Hout * Wout * 4 >= 0x80000000ull || (size_t)L.cin * Hin * Win * 4 >= 0x80000000ull) return PP_E_ARG; // buffer offsets are 32-bit, idle lanes park 2 GB out
        if (p.pre == PRE_STATS) return pp_fail(ctx, PP_E_STATE, "conv16: the producer's statistics must be finalised to (scale, shift)");
        if ((Win & 3) || (Wout & 3) || (L.cin & 15) || (L.rows % v.bm)) return PP_E_ARG;
        const int total = pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph) * (L.rows / v.bm) * B;
        int g = net->num_cu * (v.waves * 64 / v.threads); // workgroups per CU the variant is built for

        if (g > total) g = total;
        g = (g + 7) & ~7;
        grid = dim3(g, 1, 1);
    }
    if (v.family == Family::Wino4 || v.family == Family::Wino6) {
        // persistent, ONE 4-wave workgroup per CU (512 registers per lane, 3-deep LDS ring), a multiple of the 8 XCDs.
        // Whole main tiles first; what they leave uncovered goes to strip launches of thin tiles when that needs fewer tiles
        // than rounding the main grid up (same weight image: it depends on the 64-row block and the chunk only).
        if ((size_t)L.rows * Hout * Wout * 4 >= 0x80000000ull) return PP_E_ARG; // the epilogue parks idle lanes' offsets 2 GB out (W4_FAR)
        // these two kernels always normalise (every stride-1 convolution of the network follows a norm): with PRE_RAW they would read a null table
        if (p.pre == PRE_RAW) return pp_fail(ctx, PP_E_ARG, "wino4 / wino6 tilings have no raw prologue: give the layer a (scale, shift)");
        const bool tag4 = ctx->prof_on && L.kind == 0 && L.level == 0 && L.stride == 1;
        const int ncb = pp_div_up(L.rows, v.bm);
        // Tile skipping (tile_skip.hip): ts_k = the layer's ordinal among level 0's stride-1 layers, handed over by a pass whose first conv
        // ran sparse (or by the single-layer hook).  Listed launch + fill only for the fp32 wino6 main tile on a map of whole main tiles
        // (no strip launches) with lists for exactly these B frames in place; today's launch in every other case.
        const int2* ts_items = nullptr;
        const int32_t* ts_count = nullptr;
        const bool listed = ts_k > 0 && v.family == Family::Wino6 && v.kern2 && v.pw == 16 && v.ph == 16 && net->eff_prec == 0 && !net->up16 &&
                            L.kind == 0 && L.level == 0 && L.stride == 1 && Wout % v.pw == 0 && Hout % v.ph == 0 && Hout == ctx->H && Wout == ctx->W &&
                            pp_ts_list(ctx, ts_k, B, &ts_items, &ts_count);
        if (tag4) {
            const double dense = (double)(Wout / v.pw) * (Hout / v.ph) * ncb * B;
            ctx->prof_items_dense += dense;
            if (listed) ctx->prof_ts_layer.push_back(ts_k | (ncb << 8)); else ctx->prof_items += dense;
            if (ctx->prof_used + 2 > ctx->prof_ev.size()) {
                hipEvent_t a, b;
                PP_HIP(hipEventCreate(&a));
                PP_HIP(hipEventCreate(&b));
                ctx->prof_ev.push_back(a);
                ctx->prof_ev.push_back(b);
            }
            ctx->prof_flops = 2.0 * Hout * Wout * (double)L.cin * L.cout * 9.0 * B;
            PP_HIP(hipEventRecord(ctx->prof_ev[ctx->prof_used], stream));
        }
        auto launch_region = [&](const Variant& rv, int x0, int y0, int x1, int y1) {
            ConvP q = p;
            q.rx0 = x0; q.ry0 = y0; q.rx1 = x1; q.ry1 = y1;
            q.rnbx = pp_div_up(x1 - x0, rv.pw); q.rnby = pp_div_up(y1 - y0, rv.ph);
            const int total = q.rnbx * q.rnby * ncb * B;
            int g = net->num_cu;
            if (g > total) g = total;
            g = (g + 7) & ~7;
            if (listed) { q.items = ts_items; q.item_count = ts_count; } // same grid as the dense total: the kernel reads its own
            hipLaunchKernelGGL(listed ? rv.kern2 : rv.kern, dim3(g), dim3(rv.threads), rv.lds, stream, q);
        };
        const int mw = (Wout / v.pw) * v.pw, mh = (Hout / v.ph) * v.ph;
        const Variant &sv = strip_v(v.family), &sh = strip_h(v.family);
        // cost of the slowest workgroup: items are dealt evenly over min(CUs, items) persistent workgroups, a tile takes about
        // 2.4 us per 8-channel chunk + 5 us of epilogue, and a strip launch adds its own rounds plus ~30 us of launch gap and
        // pipeline prologue (at batch 1 the 20 extra launches of a frame cost more than the empty tile area they save: 3.4 ms
        // against 2.2 ms per frame; at 16+ frames per launch the strips win: 979 against 1114 us on the 100 x 100 layers)
        // The split is decided for the context's max_batch, NOT for the frames of this launch: full tiles and main + strip
        // launches group the fp32 partial sums of the InstanceNorm statistics differently (~3e-5 on the logits), and a frame's
        // result must not depend on how many frames ride in its pass.
        const int plan_b = ctx->max_batch;
        auto rounds = [&](int tiles) { return tiles > 0 ? pp_div_up((int64_t)tiles * ncb * plan_b, net->num_cu) : 0; };
        const int t_main = (mw / v.pw) * (mh / v.ph);
        const int t_right = Wout > mw ? pp_div_up(Wout - mw, sv.pw) * pp_div_up(Hout, sv.ph) : 0;
        const int t_bottom = Hout > mh ? pp_div_up(mw, sh.pw) * pp_div_up(Hout - mh, sh.ph) : 0;
        const double tile_us = v.family == Family::Wino6 ? 1.9 * (L.cin / 8) + 3.5 : 2.4 * (L.cin / 8) + 5.0;
        const double full = rounds(pp_div_up(Wout, v.pw) * pp_div_up(Hout, v.ph)) * tile_us;
        const double split = (rounds(t_main) + rounds(t_right) + rounds(t_bottom)) * tile_us + 30.0 * ((t_right > 0) + (t_bottom > 0));
        const bool no_strips = net->w4_strips == 0, all_strips = net->w4_strips == 2;
        if ((split < full || all_strips) && mw > 0 && mh > 0 && !no_strips && (Wout > mw || Hout > mh)) {
            launch_region(v, 0, 0, mw, mh);
            if (Wout > mw) launch_region(sv, mw, 0, Wout, Hout);
            if (Hout > mh) launch_region(sh, 0, mh, mw, Hout);
        } else {
            launch_region(v, 0, 0, Wout, Hout);
            if (listed)
                if (int rc = pp_ts_fill(ctx, ts_k, B, out, p.out_fs, L.rows, stream)) return rc;
        }
        if (tag4) {
            PP_HIP(hipEventRecord(ctx->prof_ev[ctx->prof_used + 1], stream));
            ctx->prof_used += 2;
        }
        PP_HIP(hipGetLastError());
        return 0;
    }
    if (v.family == Family::Wino) { // persistent Winograd: two workgroups per CU (LDS and registers allow exactly two), a multiple of the 8 XCDs
        const int total = (int)grid.x * (int)grid.y * B;
        int g = (v.threads >= 512 ? 1 : 2) * net->num_cu; // 8-wave workgroups fill a CU's registers alone
        if (g > total) g = total;
        g = (g + 7) & ~7;
        grid = dim3(g, 1, 1);
    }
    const bool tag = ctx->prof_on && L.kind == 0 && L.level == 0 && L.stride == 1;
    if (tag) {
        if (ctx->prof_used + 2 > ctx->prof_ev.size()) {
            hipEvent_t a, b;
            PP_HIP(hipEventCreate(&a));
            PP_HIP(hipEventCreate(&b));
            ctx->prof_ev.push_back(a);
            ctx->prof_ev.push_back(b);
        }
        ctx->prof_flops = 2.0 * Hout * Wout * (double)L.cin * L.cout * 9.0 * B;
        PP_HIP(hipEventRecord(ctx->prof_ev[ctx->prof_used], stream));
    }
    hipLaunchKernelGGL((pmap && v.kern2) ? v.kern2 : v.kern, grid, dim3(v.threads), lds_bytes, stream, p);
    if (tag) {
        PP_HIP(hipEventRecord(ctx->prof_ev[ctx->prof_used + 1], stream));
        ctx->prof_used += 2;
    }
    PP_HIP(hipGetLastError());
    return 0;
}


__global__ void __launch_bounds__(256) f32_to_f16(const float* __restrict__ x, _Float16* __restrict__ y, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = (_Float16)x[i];
}

__global__ void __launch_bounds__(256) fill_pattern(float* __restrict__ x, size_t n)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned h = (unsigned)i * 2654435761u;
        h ^= h >> 15; h *= 2246822519u; h ^= h >> 13;
        x[i] = (float)(h & 0xFFFF) * (1.0f / 65536.0f); // [0,1): random-looking, not zeros (zeros raise the clock)
    }
}

std::map<std::string, std::string>& tune_cache()
{
    // layer signature -> variant name, per process; PP_TUNE_CACHE=<file> persists it across processes
    static std::map<std::string, std::string> c;
    static bool loaded = false;
    if (!loaded) {
        loaded = true;
        if (const char* path = getenv("PP_TUNE_CACHE")) {
            if (FILE* f = fopen(path, "r")) {
                char line[512];
                while (fgets(line, sizeof(line), f)) {
                    char* tab = strchr(line, '\t');
                    if (!tab) continue;
                    *tab = 0;
                    char* val = tab + 1;
                    val[strcspn(val, "\r\n")] = 0;
                    c[line] = val;
                }
                fclose(f);
            }
        }
    }
    return c;
}

// Merge with what other processes wrote meanwhile, write to a temp file, rename() over the target: concurrent ranks can
// neither tear the file nor drop each other's entries (the last rename wins with a superset of what it read).
void tune_cache_save()
{
    const char* path = getenv("PP_TUNE_CACHE");
    if (!path) return;
    std::map<std::string, std::string> merged;
    if (FILE* f = fopen(path, "r")) {
        char line[512];
        while (fgets(line, sizeof(line), f)) {
            char* tab = strchr(line, '\t');
            if (!tab) continue;
            *tab = 0;
            char* val = tab + 1;
            val[strcspn(val, "\r\n")] = 0;
            merged[line] = val;
        }
        fclose(f);
    }
    for (auto& kv : tune_cache()) merged[kv.first] = kv.second;
    char tmp[1024];
    snprintf(tmp, sizeof(tmp), "%s.tmp.%d", path, (int)getpid());
    if (FILE* f = fopen(tmp, "w")) {
        for (auto& kv : merged) fprintf(f, "%s\t%s\n", kv.first.c_str(), kv.second.c_str());
        fclose(f);
        if (rename(tmp, path) != 0) remove(tmp);
    }
}

// Measure every admissible tiling of one layer on the device (1 warm-up + 3 timed launches with
// hipEvents) and keep the fastest.  Weights are really packed for each candidate, the prologue /
// statistics epilogue run as in production.
constexpr int TUNE_FRAMES = 16;         // frames per timed launch of the tuner (half the default bench pass of 32; the picks do not change beyond 16)
constexpr size_t TUNE_OUT_FS = 0, TUNE_IN_FS = 0; // 0: natural per-frame strides

int autotune_layer(pp_ctx* ctx, Layer& L, int Hin, int Win, int Hout, int Wout, float* tin, float* tout, bool verbose, bool measure = true)
{
    pp_net* net = (pp_net*)ctx->net;
    const int eprec = net->eff_prec;
    char sig[160];
    std::vector<Variant> menu;
    const int rows_ = (L.kind == 2) ? head_rows(ctx->cfg.num_anchor_per_loc) : (L.kind == 1 ? L.cout * L.up * L.up : L.cout);
    auto legal = [&](const Variant& v) {
        return variant_ok(v, rows_) && shape_ok(v, Hin, Win, Wout) && layer_lds(v, L.cin) <= (size_t)160 * 1024;
    };
    const bool first_conv = L.kind == 0 && L.stride == 2 && L.level == 0;
    layer_menu(L.kind, L.stride, L.up, menu, L.cin, L.kind == 0 && L.stride == 1 && L.level == 0, ctx->cfg.num_anchor_per_loc == 9, eprec, first_conv);
    if (eprec) {
        // a shape none of the reduced-precision tilings takes (odd maps, Cin not a multiple of 16 / 32) runs its fp32 tilings:
        // pp_layer_tilings reports what really runs
        bool any = false;
        for (const Variant& v : menu) any = any || legal(v);
        if (!any) {
            menu.clear();
            layer_menu(L.kind, L.stride, L.up, menu, L.cin, L.kind == 0 && L.stride == 1 && L.level == 0, ctx->cfg.num_anchor_per_loc == 9, 0);
        }
    }
    if (!measure) { // no on-device tuning (PP_AUTOTUNE=0 / maps the tuner's buffers do not fit): fp32 keeps pick_variant's choice,
                    // a reduced-precision mode takes the first legal entry of its menu
        if (eprec)
            for (const Variant& v : menu)
                if (legal(v) && v.prec == (eprec == 4 ? 3 : eprec)) { L.var = v; return 0; }
        return 0;
    }
    // the key carries the library version and the menu size (an entry of another build's menu is not trusted), not the
    // device index: the GPUs of a node are identical, and ranks must be able to share rank 0's table
    snprintf(sig, sizeof(sig), "v%d m%d k%d s%d u%d c%d r%d %dx%d n%d b%d p%d", pp_version(), (int)menu.size(), L.kind, L.stride, L.up, L.cin, L.cout, Hout, Wout,
             ctx->cfg.norm_kind, ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES, eprec);
    const int rows = (L.kind == 2) ? head_rows(ctx->cfg.num_anchor_per_loc) : (L.kind == 1 ? L.cout * L.up * L.up : L.cout);
    if (const char* force = getenv("PP_FORCE_VARIANT")) { // tests: pin a tiling family by name substring
        for (const Variant& v : menu)
            if (variant_ok(v, rows) && shape_ok(v, Hin, Win, Wout) && strstr(v.name, force)) { L.var = v; return 0; }
    }
    auto hit = tune_cache().find(sig);
    if (hit != tune_cache().end()) {
        for (const Variant& v : menu)
            if (hit->second == v.name) { L.var = v; return 0; }
    }
    hipEvent_t e0, e1;
    PP_HIP(hipEventCreate(&e0));
    PP_HIP(hipEventCreate(&e1));
    NormRef pre;
    if (L.kind == 2 || (L.kind == 0 && L.stride == 1)) { pre.mode = PRE_AFFINE; pre.scale = net->ones; pre.shift = net->zeros; }
    double* st = (ctx->cfg.norm_kind == 0 && L.kind != 2) ? net->stats + (size_t)23 * NREP * 320 * 2 : nullptr;
    const int stC = (L.kind == 1) ? 320 : L.cout;
    // batched like production, every frame with its own buffers: a launch then streams more than the 256 MB
    // Infinity Cache holds, as in production (aliased frames would hide a tiling's HBM re-reads)
    const int tb = ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES;
    auto time_variant = [&](const Variant& v, int reps, double& out_ms) -> int {
        const size_t need = layer_lds(v, L.cin);
        L.var = v;
        PP_HIP(hipFuncSetAttribute((const void*)v.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        if (v.kern2) PP_HIP(hipFuncSetAttribute((const void*)v.kern2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)need));
        int rc = pack_layer(ctx, L);
        if (rc) return rc;
        float ms = 0.f;
        for (int it = 0; it <= reps; ++it) {
            if (it == 1) PP_HIP(hipEventRecord(e0, 0));
            rc = launch_conv(ctx, L, tin, Hin, Win, (L.kind == 2) ? ctx->f_cls : tout, nullptr, pre, st, stC, Hout, Wout, 0, ctx->f_box, ctx->f_dir, tb, TUNE_OUT_FS, TUNE_IN_FS);
            if (rc) return rc;
        }
        PP_HIP(hipEventRecord(e1, 0));
        PP_HIP(hipEventSynchronize(e1));
        PP_HIP(hipEventElapsedTime(&ms, e0, e1));
        out_ms = ms / reps;
        return 0;
    };
    // pass 1: every legal tiling, 3 timed launches
    std::vector<std::pair<double, const Variant*>> timed;
    for (const Variant& v : menu) {
        if (!variant_ok(v, rows)) continue;
        if (!shape_ok(v, Hin, Win, Wout)) continue;
        const size_t need = layer_lds(v, L.cin);
        if (need > 160 * 1024) continue;
        double ms;
        int rc = time_variant(v, 3, ms);
        if (rc) return rc;
        if (verbose) fprintf(stderr, "[pp autotune] %-28s %-34s %8.1f us\n", sig, v.name, ms * 1e3);
        timed.push_back({ms, &v});
    }
    if (timed.empty()) return pp_fail(ctx, PP_E_STATE, "autotune: no legal tiling");
    std::sort(timed.begin(), timed.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    // pass 2: the contenders within 8 % of the best are re-timed twice with 8 launches each (clocks are warm
    // by now and the order effect of pass 1 is gone); best of the three readings decides
    double best = timed[0].first;
    Variant bv = *timed[0].second;
    size_t ncont = 0;
    while (ncont < timed.size() && ncont < 4 && timed[ncont].first <= timed[0].first * 1.08) ++ncont;
    if (ncont > 1) {
        std::vector<double> score(ncont);
        for (size_t i = 0; i < ncont; ++i) score[i] = timed[i].first;
        for (int round = 0; round < 2; ++round)
            for (size_t i = 0; i < ncont; ++i) {
                double ms;
                int rc = time_variant(*timed[i].second, 8, ms);
                if (rc) return rc;
                score[i] = (round == 0) ? ms : std::min(score[i], ms); // pass-1 reading is replaced, not kept
            }
        size_t bi = 0;
        for (size_t i = 1; i < ncont; ++i)
            if (score[i] < score[bi]) bi = i;
        best = score[bi];
        bv = *timed[bi].second;
        if (verbose)
            for (size_t i = 0; i < ncont; ++i) fprintf(stderr, "[pp autotune] %-28s   retime %-26s %8.1f us\n", sig, timed[i].second->name, score[i] * 1e3);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    L.var = bv;
    tune_cache()[sig] = bv.name;
    if (verbose) fprintf(stderr, "[pp autotune] %-28s -> %s (%.1f us)\n", sig, bv.name, best * 1e3);
    return 0;
}

// The cls-only head pass as a launch: the head layer with the cls tiling and one 16-row block; the weights stay the head's image.
int launch_head_cls(pp_ctx* ctx, const Variant& v, const float* in, const NormRef& pre, float* cls, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    Layer L = net->layers.back(); // shares the device image (no ownership: Layer has no destructor)
    L.var = v;
    L.rows = 16;
    return launch_conv(ctx, L, in, ctx->H, ctx->W, cls, nullptr, pre, nullptr, 0, ctx->H, ctx->W, stream, nullptr, nullptr, nb);
}

// Shapes of the cls-only pass, timed like a layer's tilings (3 launches after a warm-up, the fastest is kept and cached).
int autotune_head_cls(pp_ctx* ctx, float* tin, bool verbose, bool measure)
{
    pp_net* net = (pp_net*)ctx->net;
    const std::vector<Variant> menu = {make_g1_cls<8>(), make_g1_cls<10>(), make_g1_cls<4>()}; // every shape without scratch: a 16-deep ring spills
    for (const Variant& v : menu)
        PP_HIP(hipFuncSetAttribute((const void*)v.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g1_lds(v, 320)));
    net->cls_var = menu[0];
    if (!measure) return 0;
    const int tb = ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES;
    char sig[160];
    snprintf(sig, sizeof(sig), "v%d m%d headcls %s %dx%d n%d b%d", pp_version(), (int)menu.size(), net->layers.back().var.name, ctx->H, ctx->W, ctx->cfg.norm_kind, tb);
    auto hit = tune_cache().find(sig);
    if (hit != tune_cache().end())
        for (const Variant& v : menu)
            if (hit->second == v.name) { net->cls_var = v; return 0; }
    hipEvent_t e0, e1;
    PP_HIP(hipEventCreate(&e0));
    PP_HIP(hipEventCreate(&e1));
    NormRef pre;
    pre.mode = PRE_AFFINE; pre.scale = net->ones; pre.shift = net->zeros;
    double best = 1e30;
    for (const Variant& v : menu) {
        float ms = 0.f;
        for (int it = 0; it <= 3; ++it) {
            if (it == 1) PP_HIP(hipEventRecord(e0, 0));
            int rc = launch_head_cls(ctx, v, tin, pre, ctx->f_cls, tb, 0);
            if (rc) { (void)hipEventDestroy(e0); (void)hipEventDestroy(e1); return rc; }
        }
        PP_HIP(hipEventRecord(e1, 0));
        PP_HIP(hipEventSynchronize(e1));
        PP_HIP(hipEventElapsedTime(&ms, e0, e1));
        if (verbose) fprintf(stderr, "[pp autotune] %-28s %-34s %8.1f us\n", sig, v.name, ms / 3 * 1e3);
        if (ms < best) { best = ms; net->cls_var = v; }
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    tune_cache()[sig] = net->cls_var.name;
    return 0;
}

} // namespace

int pp_net_create(pp_ctx* ctx)
{
    pp_net* net = new pp_net();
    ctx->net = net;
    const int H = ctx->H, W = ctx->W;
    {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, ctx->device) == hipSuccess && prop.multiProcessorCount > 0) net->num_cu = prop.multiProcessorCount;
        if (const char* e = getenv("PP_W4_STRIPS")) net->w4_strips = (e[0] == '0') ? 0 : (e[0] == '2') ? 2 : -1;
    }
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < 4; ++b)
        {   // W6_FRONT_PAD floats in front: wino6's dwordx4 patch pieces start one float before a row (row 0 of channel 0 of frame 0 included)
            PP_HIP(hipMalloc((void**)&net->buf[l][b], ((size_t)ctx->max_batch * kC[l] * ((H >> l) + 1) * ((W >> l) + 1) + W6_FRONT_PAD) * sizeof(float)));
            net->buf[l][b] += W6_FRONT_PAD;
        }
    PP_HIP(hipMalloc((void**)&net->up, (size_t)ctx->max_batch * 320 * H * W * sizeof(float)));
    // statistics accumulators: one slot of [NREP][256][2] doubles per normalisation site (<= 24 sites)
    net->stats_bytes = (size_t)ctx->max_batch * 24 * NREP * 320 * 2 * sizeof(double);
    PP_HIP(hipMalloc((void**)&net->stats, net->stats_bytes));
    PP_HIP(hipMalloc((void**)&net->aff, (size_t)ctx->max_batch * 640 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->bn_scale, (size_t)24 * 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->bn_shift, (size_t)24 * 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->head_bias, (size_t)head_rows(ctx->cfg.num_anchor_per_loc) * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->head_bias_perm, 96 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->ones, 320 * sizeof(float)));
    PP_HIP(hipMalloc((void**)&net->zeros, 320 * sizeof(float)));
    std::vector<float> one(320, 1.f);
    PP_HIP(hipMemcpy(net->ones, one.data(), 320 * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP(hipMemset(net->zeros, 0, 320 * sizeof(float)));
    // layer list in execution order
    int cin = 64;
    for (int b = 0; b < 3; ++b) {
        const int c = kC[b];
        const int nres[3] = {1, 1, 0};
        const int nunits = (b == 0) ? 2 : 3;
        char key[128];
        snprintf(key, sizeof(key), "rpn.block%d.0.weight", b + 1);
        net->layers.push_back(Layer{key, 0, cin, c, 2, 1, b, pick_variant(0, 2, 1, c, H >> b, W >> b)});
        for (int u = 0; u < nunits; ++u) {
            const int nl = (b == 0) ? (u == 0 ? 1 : 0) : nres[u];
            snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.2.weight", b + 1, 3 + u);
            net->layers.push_back(Layer{key, 0, c, c, 1, 1, b, pick_variant(0, 1, 1, c, H >> b, W >> b)});
            if (nl == 1) {
                snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.5.weight", b + 1, 3 + u);
                net->layers.push_back(Layer{key, 0, c, c, 1, 1, b, pick_variant(0, 1, 1, c, H >> b, W >> b)});
            }
        }
        const int up = 1 << b;
        snprintf(key, sizeof(key), "rpn.deconv%d.0.weight", b + 1);
        net->layers.push_back(Layer{key, 1, c, (b == 0) ? 64 : 128, 1, up, b, pick_variant(1, 1, up, ((b == 0) ? 64 : 128) * up * up, H >> b, W >> b)});
        cin = c;
    }
    net->layers.push_back(Layer{"heads", 2, 320, 10 * ctx->cfg.num_anchor_per_loc, 1, 1, 0,
                                pick_variant(2, 1, 1, head_rows(ctx->cfg.num_anchor_per_loc), H, W, ctx->cfg.num_anchor_per_loc == 9)});
    for (Layer& L : net->layers)
        PP_HIP(hipFuncSetAttribute((const void*)L.var.kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.var.lds));
    for (Family f : {Family::Wino4, Family::Wino6})
        for (const Variant* sv : {&strip_v(f), &strip_h(f)})
            PP_HIP(hipFuncSetAttribute((const void*)sv->kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)sv->lds));
    return 0;
}

void pp_net_destroy(pp_ctx* ctx)
{
    pp_net* net = (pp_net*)ctx->net;
    if (!net) return;
    for (int l = 0; l < 3; ++l)
        for (int b = 0; b < 4; ++b)
            if (net->buf[l][b]) (void)hipFree(net->buf[l][b] - W6_FRONT_PAD);
    for (Layer& L : net->layers)
        if (L.w) (void)hipFree(L.w);
    void* ptrs[] = {net->dbg_stats, net->up, net->stats, net->aff, net->bn_scale, net->bn_shift, net->head_bias, net->head_bias_perm, net->ones, net->zeros};
    for (void* q : ptrs)
        if (q) (void)hipFree(q);
    delete net;
    ctx->net = nullptr;
}

// BatchNorm2d(eval, eps 1e-3) of the _export/_trt nets folded to (scale, shift) for norm site `site`
static int fold_bn(pp_ctx* ctx, const std::string& prefix, int C, int site)
{
    pp_net* net = (pp_net*)ctx->net;
    auto get = [&](const char* s) -> const std::vector<float>* {
        auto it = ctx->host_w.find(prefix + s);
        if (it == ctx->host_w.end() || (int)it->second.data.size() != C) return nullptr;
        return &it->second.data;
    };
    const std::vector<float>*g = get(".weight"), *b = get(".bias"), *rm = get(".running_mean"), *rv = get(".running_var");
    if (!g || !b || !rm || !rv) return pp_fail(ctx, PP_E_NAME, ("missing BatchNorm tensors for " + prefix).c_str());
    std::vector<float> sc(C), sh(C);
    for (int c = 0; c < C; ++c) {
        double s = (double)(*g)[c] / std::sqrt((double)(*rv)[c] + 1e-3);
        sc[c] = (float)s;
        sh[c] = (float)((double)(*b)[c] - (double)(*rm)[c] * s);
    }
    PP_HIP(hipMemcpy(net->bn_scale + (size_t)site * 320, sc.data(), C * sizeof(float), hipMemcpyHostToDevice));
    PP_HIP(hipMemcpy(net->bn_shift + (size_t)site * 320, sh.data(), C * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}

// Normalisation sites, numbered in execution order.  Per block b (0..2):
//   site 8b+0: norm after the strided conv (.1)        site 8b+1+2u: Resnet2 unit u first norm (.0)
//   site 8b+2+2u: unit u second norm (.3)              site 8b+7: norm after the deconv
static inline int site_block(int b, int k) { return 8 * b + k; }

int pp_net_commit(pp_ctx* ctx)
{
    pp_net* net = (pp_net*)ctx->net;
    const int na = ctx->cfg.num_anchor_per_loc;
    std::vector<float> hbv((size_t)head_rows(na), 0.f);
    float* hb = hbv.data();
    const char* names[3] = {"heads.conv_cls.bias", "heads.conv_box.bias", "heads.conv_dir.bias"};
    const int cnt[3] = {na, 7 * na, 2 * na};
    int r0 = 0;
    for (int h = 0; h < 3; ++h) {
        auto w = ctx->host_w.find(names[h]);
        if (w == ctx->host_w.end() || (int)w->second.data.size() != cnt[h])
            return pp_fail(ctx, PP_E_NAME, (std::string("missing/mis-shaped ") + names[h]).c_str());
        memcpy(hb + r0, w->second.data.data(), sizeof(float) * cnt[h]);
        r0 += cnt[h];
    }
    PP_HIP(hipMemcpy(net->head_bias, hb, hbv.size() * sizeof(float), hipMemcpyHostToDevice));
    if (na == 9) {
        float hp[96];
        for (int t = 0; t < 96; ++t) hp[t] = head_tile_row(t) >= 0 ? hb[head_tile_row(t)] : 0.f;
        PP_HIP(hipMemcpy(net->head_bias_perm, hp, sizeof(hp), hipMemcpyHostToDevice));
    }
    {
        const char* at = getenv("PP_AUTOTUNE");
        const char* vb = getenv("PP_VERBOSE");
        const bool tune = !(at && at[0] == '0');
        const bool verbose = vb && vb[0] != '0';
        const int H = ctx->H, W = ctx->W;
        float *tin = nullptr, *tout = nullptr;
        const bool can_tune = tune && (H % 4 == 0) && (W % 4 == 0);
        // fp16 storage of the activations needs every conv on conv16's and every upsampler / the head on gemm1x1's 16-bit-tensor
        // tilings: maps a multiple of 4 wide at all three levels and the 9-anchor head; otherwise mode 4 runs as mode 3 (fp32 tensors)
        net->up16 = ctx->precision == 4 && (W % 16 == 0) && ((H * W) % 64 == 0) && ctx->cfg.num_anchor_per_loc == 9;
        net->eff_prec = (ctx->precision == 4 && !net->up16) ? 3 : ctx->precision;
        if (can_tune) {
            const size_t nin = std::max((size_t)64 * ctx->gx * ctx->gy, (size_t)320 * H * W);
            const int tb = ctx->max_batch < TUNE_FRAMES ? ctx->max_batch : TUNE_FRAMES;
            PP_HIP(hipMalloc((void**)&tin, ((size_t)tb * nin + 256 + W6_FRONT_PAD) * sizeof(float)));
            tin += W6_FRONT_PAD;
            PP_HIP(hipMalloc((void**)&tout, ((size_t)tb * 320 * H * W + 256) * sizeof(float)));
            hipLaunchKernelGGL(fill_pattern, dim3(2048), dim3(256), 0, 0, tin, (size_t)tb * nin);
        }
        for (Layer& L : net->layers) {
            int rc = 0;
            {
                const int h = H >> L.level, w = W >> L.level;
                const int hin = (L.kind == 0 && L.stride == 2) ? h * 2 : h, win = (L.kind == 0 && L.stride == 2) ? w * 2 : w;
                if (!can_tune && net->eff_prec == 0) L.var = pick_variant(L.kind, L.stride, L.up, (L.kind == 2) ? head_rows(ctx->cfg.num_anchor_per_loc) : (L.kind == 1 ? L.cout * L.up * L.up : L.cout), h, w, ctx->cfg.num_anchor_per_loc == 9);
                rc = autotune_layer(ctx, L, hin, win, h, w, tin, tout, verbose, can_tune);
                if (rc) { if (tin) { (void)hipFree(tin - W6_FRONT_PAD); (void)hipFree(tout); } return rc; }
            }
            PP_HIP(hipFuncSetAttribute((const void*)L.var.kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)layer_lds(L.var, L.cin)));
            if (L.var.kern2) PP_HIP(hipFuncSetAttribute((const void*)L.var.kern2, hipFuncAttributeMaxDynamicSharedMemorySize, (int)L.var.lds));
            rc = pack_layer(ctx, L);
            if (rc) { if (tin) { (void)hipFree(tin - W6_FRONT_PAD); (void)hipFree(tout); } return rc; }
        }
        ctx->sc1_kc = (net->layers[0].var.family == Family::Direct && net->layers[0].var.kc == 8) ? 8 : 4;
        {   // deferred head: fp32 plan with the 9-anchor head on a gemm1x1 tiling (its image is what the cls pass and the candidate head read)
            const Layer& head = net->layers.back();
            net->defer_ok = net->eff_prec == 0 && na == 9 && head.var.family == Family::Gemm1x1 && head.var.prec == 0 && head.var.io16 == 0;
            if (net->defer_ok) {
                const int rc = autotune_head_cls(ctx, tin, verbose, can_tune);
                if (rc) { if (tin) { (void)hipFree(tin - W6_FRONT_PAD); (void)hipFree(tout); } return rc; }
            }
        }
        if (tin) { PP_HIP(hipDeviceSynchronize()); (void)hipFree(tin - W6_FRONT_PAD); (void)hipFree(tout); tune_cache_save(); }
        if (net->up16)
            for (const Layer& L : net->layers)
                if ((L.kind == 1 && L.var.io16 != 3) || (L.kind == 2 && L.var.io16 != 1) ||
                    (L.kind == 0 && L.var.io16 != ((L.stride == 2 && L.level == 0) ? 2 : 3)))
                    return pp_fail(ctx, PP_E_STATE, "fp16s: a layer did not get a 16-bit-tensor tiling (PP_FORCE_VARIANT?)");
    }
    if (ctx->cfg.norm_kind == 1) {
        for (int b = 0; b < 3; ++b) {
            char key[128];
            const int c = kC[b];
            snprintf(key, sizeof(key), "rpn.block%d.1", b + 1);
            int rc = fold_bn(ctx, key, c, site_block(b, 0));
            if (rc) return rc;
            const int nunits = (b == 0) ? 2 : 3;
            for (int u = 0; u < nunits; ++u) {
                const int nl = (u == nunits - 1) ? 0 : 1;
                snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.0", b + 1, 3 + u);
                if ((rc = fold_bn(ctx, key, c, site_block(b, 1 + 2 * u)))) return rc;
                if (nl) {
                    snprintf(key, sizeof(key), "rpn.block%d.%d.conv_block.3", b + 1, 3 + u);
                    if ((rc = fold_bn(ctx, key, c, site_block(b, 2 + 2 * u)))) return rc;
                }
            }
            snprintf(key, sizeof(key), "rpn.deconv%d.1", b + 1);
            // deconv norms are stored contiguously at site 7 (block 0), channels [0,64),[64,192),[192,320)
            const int coff = (b == 0) ? 0 : (b == 1 ? 64 : 192);
            const int cc = (b == 0) ? 64 : 128;
            pp_net* n2 = net;
            {
                auto get = [&](const char* s) -> const std::vector<float>* {
                    auto it = ctx->host_w.find(std::string(key) + s);
                    if (it == ctx->host_w.end() || (int)it->second.data.size() != cc) return nullptr;
                    return &it->second.data;
                };
                const std::vector<float>*g = get(".weight"), *bb = get(".bias"), *rm = get(".running_mean"), *rv = get(".running_var");
                if (!g || !bb || !rm || !rv) return pp_fail(ctx, PP_E_NAME, (std::string("missing BatchNorm tensors for ") + key).c_str());
                std::vector<float> sc(cc), sh(cc);
                for (int q = 0; q < cc; ++q) {
                    double s = (double)(*g)[q] / std::sqrt((double)(*rv)[q] + 1e-3);
                    sc[q] = (float)s;
                    sh[q] = (float)((double)(*bb)[q] - (double)(*rm)[q] * s);
                }
                PP_HIP(hipMemcpy(n2->bn_scale + (size_t)7 * 320 + coff, sc.data(), cc * sizeof(float), hipMemcpyHostToDevice));
                PP_HIP(hipMemcpy(n2->bn_shift + (size_t)7 * 320 + coff, sh.data(), cc * sizeof(float), hipMemcpyHostToDevice));
            }
        }
    }
    return 0;
}

namespace {

// statistics slot / folded-BN arrays for a site
NormRef norm_ref(pp_ctx* ctx, int site, int C, int coff, size_t count)
{
    pp_net* net = (pp_net*)ctx->net;
    NormRef r;
    r.C = C;
    if (ctx->cfg.norm_kind == 1) {
        r.mode = PRE_AFFINE;
        r.scale = net->bn_scale + (size_t)site * 320 + coff;
        r.shift = net->bn_shift + (size_t)site * 320 + coff;
    } else {
        r.mode = PRE_STATS;
        r.acc = net->stats + (size_t)site * NREP * 320 * 2;
        r.inv_n = 1.0 / (double)count;
        r.fs = STAT_FS;
    }
    return r;
}

double* stat_slot(pp_ctx* ctx, int site)
{
    if (ctx->cfg.norm_kind == 1) return nullptr;
    return ((pp_net*)ctx->net)->stats + (size_t)site * NREP * 320 * 2;
}

int launch_norm_relu(pp_ctx* ctx, const float* x, float* y, int C, int HW, const NormRef& pre, double* stat, hipStream_t stream,
                     int B = 1, int x16 = 0, int y16 = 0)
{
    int bx = pp_div_up(HW / 4, 256 * 4);
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(norm_relu_stats, dim3(bx, C, B), dim3(256), 0, stream, x, y, C, HW, pre.mode, pre.acc, pre.scale,
                       pre.shift, pre.inv_n, 1e-3f, stat, (size_t)C * HW, STAT_FS, x16, y16);
    PP_HIP(hipGetLastError());
    return 0;
}

} // namespace

// do all stride-1 layers of level 0 (at most three: tile_skip.hip's rule) run the fp32 wino6 main tile on a map of whole main tiles?
static bool level0_main_wino6(const pp_net* net, int h, int w)
{
    int n = 0;
    for (const Layer& L : net->layers)
        if (L.kind == 0 && L.level == 0 && L.stride == 1) {
            ++n;
            if (L.var.family != Family::Wino6 || !L.var.kern2 || L.var.pw != 16 || L.var.ph != 16 || (w % 16) || (h % 16)) return false;
        }
    return n >= 1 && n <= 3 && net->eff_prec == 0;
}

// canvas [64,gx,gy] -> up [320,H,W] PRE-norm (+ statistics); the head (or pp_backbone's final pass)
// applies the last norm + ReLU.
int pp_run_backbone(pp_ctx* ctx, const float* canvas, int nb, hipStream_t stream, const int32_t* pmap, const float* feat)
{
    pp_net* net = (pp_net*)ctx->net;
    const int H = ctx->H, W = ctx->W;
    if ((H % 4) || (W % 4)) return pp_fail(ctx, PP_E_ARG, "backbone: BEV grid must be a multiple of 8 in x and y");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "backbone: batch exceeds cfg.max_batch");
    ctx->sc1_last_nb = 0;
    pp_ts_begin_pass(ctx);
    if (ctx->cfg.norm_kind == 0) PP_HIP(hipMemsetAsync(net->stats, 0, STAT_FS * sizeof(double) * nb, stream));
    NormRef raw;
    const float* x = canvas;
    int Hin = ctx->gx, Win = ctx->gy;
    size_t li = 0;
    const int up_coff[3] = {0, 64, 192};
    const size_t up_fs = (size_t)320 * H * W;
    for (int b = 0; b < 3; ++b) {
        const int c = kC[b];
        const int h = H >> b, w = W >> b;
        const size_t cnt = (size_t)h * w;
        float** Bf = net->buf[b];
        int rc;
        // strided conv (raw input) -> Bf[0] + stats(site 0); the fused fp32 path runs the first one over the active pixels only
        if (b == 0 && pmap && net->eff_prec == 0 && pp_sc1_usable(ctx)) {
            ++li;
            if ((rc = pp_sc1_run(ctx, pmap, feat, Bf[0], stat_slot(ctx, site_block(0, 0)), STAT_FS, nb, stream))) return rc;
            // the map is exactly zero outside the active set now: lists of the tiles level 0's stride-1 layers need not recompute
            if (ctx->sc1_last_nb == nb && !net->up16 && pp_ts_usable(ctx, 3) && level0_main_wino6(net, h, w)) {
                if ((rc = pp_ts_build(ctx, nb, nullptr, stream))) return rc;
                pp_ts_mark_pass(ctx, nb);
            }
        } else if ((rc = launch_conv(ctx, net->layers[li++], x, Hin, Win, Bf[0], nullptr, raw, stat_slot(ctx, site_block(b, 0)), c, h, w, stream,
                              nullptr, nullptr, nb, 0, 0, b == 0 ? pmap : nullptr, b == 0 ? feat : nullptr))) return rc;
        // y = relu(norm(Bf[0])) -> Bf[1] + stats(site 1) (the first Resnet2 unit's leading norm)
        if ((rc = pp_stage_mark(ctx, stream, PP_ST_NORM))) return rc;
        if ((rc = launch_norm_relu(ctx, Bf[0], Bf[1], c, (int)cnt, norm_ref(ctx, site_block(b, 0), c, 0, cnt),
                                   stat_slot(ctx, site_block(b, 1)), stream, nb, net->up16 ? 1 : 0, net->up16 ? 1 : 0))) return rc;
        if ((rc = pp_stage_mark(ctx, stream, PP_ST_CONV))) return rc;
        float* cur = Bf[1];
        float* spare[3] = {Bf[0], Bf[2], Bf[3]};
        // block 3's unit inputs h, m3, r3, m4, r4 leave through the copy hook behind the launch that produces each: the level
        // buffers are reused before the pass ends
        float* utap = (b == 2 && nb == 1) ? net->unit_tap : nullptr;
        const size_t ubytes = (size_t)c * cnt * sizeof(float);
        int ucount = 0;
        if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * c * cnt, cur, ubytes, hipMemcpyDeviceToDevice, stream));
        const int nunits = (b == 0) ? 2 : 3;
        int ts_k = 0; // level 0: ordinal of the next stride-1 layer (launch_conv ignores it unless this pass built tile lists)
        for (int u = 0; u < nunits; ++u) {
            const int nl = (u == nunits - 1) ? 0 : 1;
            const bool last = (u == nunits - 1);
            float* t1 = spare[0];
            float* t2 = spare[1];
            // stats for the NEXT unit's leading norm are produced by this unit's output
            double* out_stat = last ? nullptr : stat_slot(ctx, site_block(b, 1 + 2 * (u + 1)));
            if (nl == 1) {
                if ((rc = launch_conv(ctx, net->layers[li++], cur, h, w, t1, nullptr, norm_ref(ctx, site_block(b, 1 + 2 * u), c, 0, cnt),
                                      stat_slot(ctx, site_block(b, 2 + 2 * u)), c, h, w, stream, nullptr, nullptr, nb, 0, 0, nullptr, nullptr,
                                      b == 0 ? ++ts_k : 0))) return rc;
                if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * c * cnt, t1, ubytes, hipMemcpyDeviceToDevice, stream));
                if ((rc = launch_conv(ctx, net->layers[li++], t1, h, w, t2, cur, norm_ref(ctx, site_block(b, 2 + 2 * u), c, 0, cnt),
                                      out_stat, c, h, w, stream, nullptr, nullptr, nb, 0, 0, nullptr, nullptr, b == 0 ? ++ts_k : 0))) return rc;
                if (utap) PP_HIP(hipMemcpyAsync(utap + (size_t)ucount++ * c * cnt, t2, ubytes, hipMemcpyDeviceToDevice, stream));
                spare[1] = cur; // t2 becomes current; old current and t1 are free
                cur = t2;
            } else {
                if ((rc = launch_conv(ctx, net->layers[li++], cur, h, w, t1, cur, norm_ref(ctx, site_block(b, 1 + 2 * u), c, 0, cnt),
                                      out_stat, c, h, w, stream, nullptr, nullptr, nb, 0, 0, nullptr, nullptr, b == 0 ? ++ts_k : 0))) return rc;
                spare[0] = cur;
                cur = t1;
            }
        }
        net->tap[b] = cur;
        // deconv on the raw block output -> channel slice of up[320,H,W] + stats (site 7, channel offset)
        {
            const Layer& L = net->layers[li++];
            double* st = stat_slot(ctx, 7);
            // the block's channel slice of the concat buffer (element offsets: the buffer holds fp16 under pp_set_precision 4)
            float* slice = net->up16 ? reinterpret_cast<float*>(reinterpret_cast<_Float16*>(net->up) + (size_t)up_coff[b] * H * W)
                                     : net->up + (size_t)up_coff[b] * H * W;
            if ((rc = launch_conv(ctx, L, cur, h, w, slice, nullptr, raw, st ? st + (size_t)up_coff[b] * 2 : nullptr,
                                  320, h, w, stream, nullptr, nullptr, nb, up_fs))) return rc;
        }
        x = cur;
        Hin = h;
        Win = w;
    }
    return 0;
}

static int pp_head_impl(pp_ctx* ctx, const float* in, const NormRef& pre, float* cls, float* box, float* dir, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    return launch_conv(ctx, net->layers.back(), in, ctx->H, ctx->W, cls, nullptr, pre, nullptr, 0, ctx->H, ctx->W, stream, box, dir, nb);
}

int pp_run_head_fused(pp_ctx* ctx, float* cls, float* box, float* dir, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    NormRef pre = norm_ref(ctx, 7, 320, 0, (size_t)ctx->H * ctx->W);
    return pp_head_impl(ctx, net->up, pre, cls, box, dir, nb, stream);
}

// ---- deferred head (pp_infer_batch): cls rows for every pixel, box / dir logits for the selected candidates only ----
bool pp_head_defer_on(pp_ctx* ctx)
{
    const pp_net* net = (const pp_net*)ctx->net;
    return ctx->head_defer && net && ctx->weights_ready && net->defer_ok;
}

int pp_run_head_cls(pp_ctx* ctx, float* cls, int nb, hipStream_t stream)
{
    pp_net* net = (pp_net*)ctx->net;
    NormRef pre = norm_ref(ctx, 7, 320, 0, (size_t)ctx->H * ctx->W);
    int rc = launch_head_cls(ctx, net->cls_var, net->up, pre, cls, nb, stream);
    if (rc) return rc;
    ctx->head_stale = true;
    ctx->stale_nb = nb;
    ctx->stale_stream = stream;
    return 0;
}

// What the candidate head (postprocess.hip) reads: the head image and the concat buffer with the normalisation the cls pass of
// `nb` frames just used (a batched launch finalised the statistics into net->aff, a single frame finalises them in the kernel).
int pp_net_head_gather(pp_ctx* ctx, int nb, pp_head_gather* g)
{
    pp_net* net = (pp_net*)ctx->net;
    const Layer& head = net->layers.back();
    if (!net->defer_ok) return pp_fail(ctx, PP_E_STATE, "candidate head: the committed plan has no fp32 gemm1x1 head image");
    const NormRef pre = norm_ref(ctx, 7, 320, 0, (size_t)ctx->H * ctx->W);
    g->w = head.w; g->bm = head.var.bm; g->bmp = head.var.bmp; g->K = head.cin;
    g->bias_perm = net->head_bias_perm;
    g->in = net->up; g->in_fs = (size_t)head.cin * ctx->H * ctx->W; g->HW = ctx->H * ctx->W;
    g->pre = pre.mode; g->pre_acc = pre.acc; g->pre_fs = pre.fs; g->pre_inv_n = pre.inv_n;
    g->pre_scale = pre.scale; g->pre_shift = pre.shift; g->aff_fs = 0; g->eps = 1e-3f;
    if (pre.mode == PRE_STATS && nb > 1) { g->pre = PRE_AFFINE; g->pre_scale = net->aff; g->pre_shift = net->aff + 320; g->aff_fs = 640; }
    return 0;
}

// Full box / dir (and cls) tensors of the last deferred pass: today's head over the retained concat buffer and statistics.
int pp_head_materialise(pp_ctx* ctx, hipStream_t stream)
{
    if (!ctx->head_stale) return 0;
    ctx->head_stale = false;
    return pp_run_head_fused(ctx, ctx->f_cls, ctx->f_box, ctx->f_dir, ctx->stale_nb, stream);
}

extern "C" int pp_set_head_defer(pp_ctx* ctx, int on)
{
    if (!ctx) return PP_E_ARG;
    ctx->head_defer = on && !ctx->head_defer_env_off;
    return 0;
}

extern "C" int pp_head_defer_active(pp_ctx* ctx)
{
    if (!ctx) return 0;
    return pp_head_defer_on(ctx) ? 1 : 0;
}

extern "C" int pp_backbone(pp_ctx* ctx, const float* canvas, float* rpn_out, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone: weights not committed");
    if (!canvas || !rpn_out) return pp_fail(ctx, PP_E_ARG, "pp_backbone: null pointer");
    if (int rc0 = pp_head_materialise(ctx, stream)) return rc0; // the concat buffer and its statistics are about to be overwritten
    int rc = pp_run_backbone(ctx, canvas, 1, stream, nullptr, nullptr);
    if (rc) return rc;
    pp_net* net = (pp_net*)ctx->net;
    const int HW = ctx->H * ctx->W;
    // stand-alone API: materialise relu(norm(up)) as the reference's RPN.forward returns it
    return launch_norm_relu(ctx, net->up, rpn_out, 320, HW, norm_ref(ctx, 7, 320, 0, (size_t)HW), nullptr, stream, 1, net->up16 ? 1 : 0);
}

extern "C" int pp_head(pp_ctx* ctx, const float* rpn_out, float* cls, float* box, float* dir, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_head: weights not committed");
    if (!rpn_out || !cls || !box || !dir) return pp_fail(ctx, PP_E_ARG, "pp_head: null pointer");
    NormRef raw; // rpn_out is already normalised + ReLU'd
    pp_net* net = (pp_net*)ctx->net;
    if (net->up16) { // the head's tiling reads an fp16 tensor: round the caller's fp32 features into the (idle) concat buffer first
        const size_t n = (size_t)320 * ctx->H * ctx->W;
        hipLaunchKernelGGL(f32_to_f16, dim3(2048), dim3(256), 0, stream, rpn_out, reinterpret_cast<_Float16*>(net->up), n);
        return pp_head_impl(ctx, net->up, raw, cls, box, dir, 1, stream);
    }
    return pp_head_impl(ctx, rpn_out, raw, cls, box, dir, 1, stream);
}

// A packed weight image as an index map (pp_common.h): pack_layer itself packs an index-valued weight (element i of the
// concatenation of the named host tensors holds the float i + 1; exact below 2^24) into a scratch image with the layer's committed
// tiling, so whatever row order (head_tile_row), row padding and K blocking that tiling uses is read back, not restated.  fp32 images
// only: the 16-bit images round their elements, the indices would not survive.  Synchronous; called once per commit by train.hip.
static int layer_index_map(pp_ctx* ctx, const Layer& L, const std::vector<std::string>& names, std::vector<int32_t>& wmap)
{
    std::vector<std::vector<float>> saved(names.size());
    float idx = 1.f;
    for (size_t h = 0; h < names.size(); ++h) {
        auto w = ctx->host_w.find(names[h]);
        if (w == ctx->host_w.end()) {
            for (size_t g = 0; g < h; ++g) ctx->host_w[names[g]].data.swap(saved[g]);
            return pp_fail(ctx, PP_E_NAME, ("missing weight " + names[h]).c_str());
        }
        saved[h] = w->second.data;
        for (float& v : w->second.data) v = idx++;
    }
    Layer scratch = L;
    scratch.w = nullptr;
    int rc = idx > 16777216.f ? pp_fail(ctx, PP_E_ARG, "weight too large for an index map") : pack_layer(ctx, scratch);
    for (size_t h = 0; h < names.size(); ++h) ctx->host_w[names[h]].data.swap(saved[h]);
    if (rc) { if (scratch.w) (void)hipFree(scratch.w); return rc; }
    std::vector<float> image(scratch.w_bytes / sizeof(float));
    const hipError_t e = hipMemcpy(image.data(), scratch.w, scratch.w_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(scratch.w);
    PP_HIP(e);
    wmap.resize(image.size());
    for (size_t i = 0; i < image.size(); ++i) wmap[i] = (int32_t)image[i] - 1;
    return 0;
}

// The layout of a conv3x3 layer's fp32 image as a map onto the TRANSFORMED weights: pmap[i] = (row cin + c) T + position of the element
// of [rows][cin][T] that image element i holds (T = 36 wino6, 16 wino / wino4: position a n + b of U = G g G^T; 9 direct: the tap),
// -1 for padding.  The Winograd images hold U, not permuted copies of g, so layer_index_map cannot describe them.
static int layer_position_map(pp_ctx* ctx, const Layer& L, std::vector<int32_t>& pmap, int* T)
{
    const Family f = L.var.family;
    *T = f == Family::Wino6 ? 36 : (f == Family::Wino || f == Family::Wino4) ? 16 : 9;
    if ((size_t)L.cout * L.cin * *T >= 16777216) return pp_fail(ctx, PP_E_ARG, "weight too large for a position map");
    Layer scratch = L;
    scratch.w = nullptr;
    int rc = pack_layer(ctx, scratch, true);
    if (rc) { if (scratch.w) (void)hipFree(scratch.w); return rc; }
    std::vector<float> image(scratch.w_bytes / sizeof(float));
    const hipError_t e = hipMemcpy(image.data(), scratch.w, scratch.w_bytes, hipMemcpyDeviceToHost);
    (void)hipFree(scratch.w);
    PP_HIP(e);
    pmap.resize(image.size());
    for (size_t i = 0; i < image.size(); ++i) pmap[i] = (int32_t)image[i] - 1;
    return 0;
}

// Unit `unit` (0..4) of Resnet block `block` of the committed plan, for pp_update_block_weights (block_train.hip)
int pp_net_block_image(pp_ctx* ctx, int block, int unit, pp_block_image* img)
{
    pp_net* net = (pp_net*)ctx->net;
    int seen = 0;
    for (Layer& L : net->layers) {
        if (L.kind != 0 || L.level != block || L.stride != 1 || seen++ != unit) continue;
        if (net->eff_prec != 0 || L.var.prec != 0 || L.var.io16 != 0 || L.var.family == Family::Conv16)
            return pp_fail(ctx, PP_E_ARG, "block weights can be rewritten in place in the fp32 mode only (the committed plan packs them in a 16-bit format)");
        int rc = layer_position_map(ctx, L, img->pmap, &img->T);
        if (rc) return rc;
        img->w = L.w;
        img->C = L.cin;
        return L.cin == L.cout ? 0 : pp_fail(ctx, PP_E_ARG, "pp_net_block_image: not a C -> C unit");
    }
    return pp_fail(ctx, PP_E_ARG, "pp_net_block_image: no such unit");
}

int pp_net_head_image(pp_ctx* ctx, pp_head_image* img)
{
    pp_net* net = (pp_net*)ctx->net;
    Layer& head = net->layers.back();
    if (net->eff_prec != 0 || head.var.prec != 0 || head.var.io16 != 0)
        return pp_fail(ctx, PP_E_ARG, "head weights can be rewritten in place in the fp32 mode only (the committed plan packs the head in a 16-bit format)");
    const int na = ctx->cfg.num_anchor_per_loc;
    const char* names[3] = {"heads.conv_cls.weight", "heads.conv_box.weight", "heads.conv_dir.weight"};
    const int cnt[3] = {na, 7 * na, 2 * na};
    for (int h = 0; h < 3; ++h) {
        auto w = ctx->host_w.find(names[h]);
        if (w == ctx->host_w.end() || (int64_t)w->second.data.size() != (int64_t)cnt[h] * head.cin)
            return pp_fail(ctx, PP_E_NAME, (std::string("missing/mis-shaped weight ") + names[h]).c_str());
    }
    int rc = layer_index_map(ctx, head, {names[0], names[1], names[2]}, img->wmap);
    if (rc) return rc;
    img->w = head.w;
    img->bias = net->head_bias;
    img->bmap.assign((size_t)head_rows(na), -1);
    for (int r = 0; r < 10 * na; ++r) img->bmap[r] = r;
    img->bias_perm = nullptr;
    img->bpmap.clear();
    if (na == 9) {
        img->bias_perm = net->head_bias_perm;
        img->bpmap.resize(96);
        for (int t = 0; t < 96; ++t) img->bpmap[t] = head_tile_row(t);
    }
    return 0;
}

// The packed image of upsampler `branch` (0..2) of the committed plan, described the same way: wmap[i] is the element of the
// state_dict tensor rpn.deconv<branch+1>.0.weight [Cin][Cup][s][s] that image element i holds, -1 for padding.
int pp_net_deconv_image(pp_ctx* ctx, int branch, pp_layer_image* img)
{
    pp_net* net = (pp_net*)ctx->net;
    int seen = 0;
    for (Layer& L : net->layers) {
        if (L.kind != 1 || seen++ != branch) continue;
        if (net->eff_prec != 0 || L.var.prec != 0 || L.var.io16 != 0)
            return pp_fail(ctx, PP_E_ARG, "upsampler weights can be rewritten in place in the fp32 mode only (the committed plan packs them in a 16-bit format)");
        int rc = layer_index_map(ctx, L, {L.wkey}, img->wmap);
        if (rc) return rc;
        img->w = L.w;
        img->elems = (size_t)L.cin * L.cout * L.up * L.up;
        return 0;
    }
    return pp_fail(ctx, PP_E_ARG, "pp_net_deconv_image: no such upsampler");
}

extern "C" int pp_backbone_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone_taps: weights not committed");
    if (!canvas || !rpn_out || !x1 || !x2 || !x3) return pp_fail(ctx, PP_E_ARG, "pp_backbone_taps: null pointer");
    pp_net* net = (pp_net*)ctx->net;
    if (net->eff_prec != 0 || net->up16)
        return pp_fail(ctx, PP_E_ARG, "pp_backbone_taps: fp32 mode only (in the 16-bit modes the level buffers may hold fp16)");
    int rc = pp_backbone(ctx, canvas, rpn_out, stream_);
    if (rc) return rc;
    hipStream_t stream = (hipStream_t)stream_;
    float* dst[3] = {x1, x2, x3};
    for (int b = 0; b < 3; ++b)
        PP_HIP(hipMemcpyAsync(dst[b], net->tap[b], (size_t)kC[b] * (ctx->H >> b) * (ctx->W >> b) * sizeof(float), hipMemcpyDeviceToDevice, stream));
    return 0;
}

extern "C" int pp_backbone_block_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* units, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_backbone_block_taps: weights not committed");
    if (!units) return pp_fail(ctx, PP_E_ARG, "pp_backbone_block_taps: null pointer");
    pp_net* net = (pp_net*)ctx->net;
    net->unit_tap = units; // pp_backbone_taps checks the rest; the hook is armed for this one pass only
    int rc = pp_backbone_taps(ctx, canvas, rpn_out, x1, x2, x3, stream_);
    net->unit_tap = nullptr;
    return rc;
}

// Test / inspection hook: copy one tensor of frame `frame` of the LAST pp_infer_batch / pp_infer_frame pass out of the
// context's internal frame buffers (device -> device, on `stream`).  kind: 0 cls f32[A], 1 box f32[A,7], 2 dir f32[A,2],
// 3 anchor mask u8[A], 4 rpn output f32[320,H,W] = relu(norm(concat)) as RPN.forward returns it
// (pointpillars8_shared.py:173-181; materialised here, the fused path never stores it), 5 PFN rows f32[max_voxels,64],
// 6 coors i32[max_voxels,3], 7 pillar count i32[1], 8 active list of the sparse first conv i32[1 + min(4 max_voxels, H W)]
// (count, then the active output pixels in ascending order; PP_E_STATE when the pass ran the dense first conv), 9 tile flags of the
// tile-skipping path u8[3][(H / 16) (W / 16)] (1 = skippable at layer 1, 2, 3; PP_E_STATE when the pass built none).
extern "C" int pp_fetch_frame_tensor(pp_ctx* ctx, int frame, int kind, void* dst, void* stream_)
{
    if (!ctx || !dst) return pp_fail(ctx, PP_E_ARG, "pp_fetch_frame_tensor: null pointer");
    if (frame < 0 || frame >= ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_fetch_frame_tensor: frame out of range");
    hipStream_t stream = (hipStream_t)stream_;
    pp_net* net = (pp_net*)ctx->net;
    const size_t A = (size_t)ctx->A, mv = (size_t)ctx->cfg.max_voxels, HW = (size_t)ctx->H * ctx->W;
    const void* src = nullptr;
    size_t bytes = 0;
    if (kind == 1 || kind == 2)
        if (int rc0 = pp_head_materialise(ctx, stream)) return rc0;
    switch (kind) {
    case 0: src = ctx->f_cls + frame * A; bytes = A * 4; break;
    case 1: src = ctx->f_box + frame * A * 7; bytes = A * 28; break;
    case 2: src = ctx->f_dir + frame * A * 2; bytes = A * 8; break;
    case 3: src = ctx->f_mask + frame * A; bytes = A; break;
    case 4: {
        NormRef pre = norm_ref(ctx, 7, 320, 0, HW);
        if (pre.mode == PRE_STATS) pre.acc += (size_t)frame * STAT_FS;
        const float* src_ = net->up16 ? reinterpret_cast<const float*>(reinterpret_cast<const _Float16*>(net->up) + (size_t)frame * 320 * HW)
                                      : net->up + (size_t)frame * 320 * HW;
        return launch_norm_relu(ctx, src_, (float*)dst, 320, (int)HW, pre, nullptr, stream, 1, net->up16 ? 1 : 0);
    }
    case 5: src = ctx->f_feat + frame * mv * 64; bytes = mv * 64 * 4; break;
    case 6: src = ctx->f_coors + frame * mv * 3; bytes = mv * 12; break;
    case 7: src = ctx->f_num + frame * 4; bytes = 4; break;
    case 8: return pp_sc1_fetch_list(ctx, frame, dst, stream);
    case 9: return pp_ts_fetch_flags(ctx, frame, dst, stream);
    default: return pp_fail(ctx, PP_E_ARG, "pp_fetch_frame_tensor: unknown kind");
    }
    PP_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, stream));
    return 0;
}

namespace {
// out[f][c][k] = sum over the NREP replicated accumulators (k = 0 sum, 1 sum of squares)
__global__ void __launch_bounds__(256) dbg_reduce_stats(const double* __restrict__ acc, size_t acc_fs, int C, double* __restrict__ out)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= 2 * C) return;
    const double* a = acc + (size_t)blockIdx.y * acc_fs;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < NREP; ++r) s += a[(size_t)r * C * 2 + i];
    out[(size_t)blockIdx.y * 2 * C + i] = s;
}
} // namespace

// Test hook: ONE layer of the committed plan (kernel, tiling and weight image as pp_layer_tilings reports them) through launch_conv on
// caller tensors -- see include/pp_hip.h.  Reads the plan and the weight images, writes only caller memory and its own statistics
// scratch: nothing a later pass reads changes.
extern "C" int pp_debug_layer(pp_ctx* ctx, int layer, int nb, const void* in, const void* res, int pre_mode, const float* scale, const float* shift,
                              const int32_t* pmap, const float* feat, void* out, float* out_box, float* out_dir, double* stats, void* stream_)
{
    return pp_debug_layer_skip(ctx, layer, nb, in, res, pre_mode, scale, shift, pmap, feat, out, out_box, out_dir, stats, nullptr, 0, stream_);
}

// pp_debug_layer with the tile-skipping form: active u8[nb][H][W] (the pixels the sparse first conv would have computed) and the layer's
// ordinal skip_k (1..3) build the lists with the pass's own builder; the layer then runs as the listed launch plus the fill.
extern "C" int pp_debug_layer_skip(pp_ctx* ctx, int layer, int nb, const void* in, const void* res, int pre_mode, const float* scale, const float* shift,
                                   const int32_t* pmap, const float* feat, void* out, float* out_box, float* out_dir, double* stats,
                                   const uint8_t* active, int skip_k, void* stream_)
{
    if (!ctx) return PP_E_ARG;
    if (!ctx->net || !ctx->weights_ready) return pp_fail(ctx, PP_E_STATE, "pp_debug_layer: weights not committed");
    pp_net* net = (pp_net*)ctx->net;
    if (layer < 0 || layer >= (int)net->layers.size()) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: layer index out of range");
    if (nb < 1 || nb > ctx->max_batch) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: nb must be 1 .. cfg.max_batch");
    const Layer& L = net->layers[layer];
    const bool sparse = pmap || feat;
    if (sparse && layer != 0) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the sparse input form belongs to layer 0");
    if (sparse && (!pmap || !feat || in)) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: layer 0 takes either `in` or pmap + feat");
    if (!sparse && !in) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: null input");
    if (!out) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: null output");
    if (res && L.kind != 0) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: only a convolution takes a residual");
    if (pre_mode < 0 || pre_mode > 2) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: pre_mode must be 0 (raw), 1 (shared affine) or 2 (per-frame affine)");
    if ((pre_mode != 0) != (scale != nullptr) || (pre_mode != 0) != (shift != nullptr))
        return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: scale and shift go with pre_mode 1 / 2 and with nothing else");
    if (L.kind == 2 && (!out_box || !out_dir)) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the head needs out_box and out_dir");
    if (L.kind != 2 && (out_box || out_dir)) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: out_box / out_dir belong to the head");
    if (L.kind == 2 && stats) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the head accumulates no statistics");
    if (pre_mode == 0 && (L.var.family == Family::Wino4 || L.var.family == Family::Wino6))
        return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the committed tiling (wino4 / wino6) has no raw prologue, give it a (scale, shift)");
    if ((active != nullptr) != (skip_k != 0)) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer_skip: the activity bitmap and the layer ordinal come together");
    if (active && (skip_k < 1 || skip_k > 3 || L.kind != 0 || L.level != 0 || L.stride != 1 || !pp_ts_usable(ctx, 3) || !level0_main_wino6(net, ctx->H, ctx->W)))
        return pp_fail(ctx, PP_E_ARG, "pp_debug_layer_skip: tile skipping serves the stride-1 layers of level 0 (ordinal 1..3) on the fp32 wino6 main tile, whole tiles, switch on");
    hipStream_t stream = (hipStream_t)stream_;
    const int h = ctx->H >> L.level, w = ctx->W >> L.level;
    const bool s2 = L.kind == 0 && L.stride == 2;
    const int hin = s2 ? 2 * h : h, win = s2 ? 2 * w : w;
    NormRef pre;
    if (pre_mode) { pre.mode = PRE_AFFINE; pre.scale = const_cast<float*>(scale); pre.shift = const_cast<float*>(shift); pre.C = L.cin; pre.aff_fs = pre_mode == 2 ? (size_t)L.cin : 0; }
    double* st = nullptr;
    if (stats) {
        if (!net->dbg_stats) PP_HIP(hipMalloc((void**)&net->dbg_stats, (size_t)ctx->max_batch * STAT_FS * sizeof(double)));
        st = net->dbg_stats;
        PP_HIP(hipMemsetAsync(st, 0, (size_t)nb * STAT_FS * sizeof(double), stream));
    }
    pp_ts_begin_hook(ctx, active != nullptr);
    if (active)
        if (int rc0 = pp_ts_build_from_bitmap(ctx, nb, active, stream)) return rc0;
    const int rc = launch_conv(ctx, L, (const float*)in, hin, win, (float*)out, (const float*)res, pre, st, L.cout, h, w, stream, out_box, out_dir, nb, 0, 0,
                               pmap, feat, active ? skip_k : 0);
    if (active) pp_ts_end_hook(ctx);
    if (rc == PP_E_ARG) return pp_fail(ctx, PP_E_ARG, "pp_debug_layer: the committed tiling does not take this layer's shape");
    if (rc) return rc;
    if (stats) {
        hipLaunchKernelGGL(dbg_reduce_stats, dim3(pp_div_up(2 * L.cout, 256), nb), dim3(256), 0, stream, st, STAT_FS, L.cout, stats);
        PP_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int pp_profile_begin(pp_ctx* ctx)
{
    if (!ctx) return PP_E_ARG;
    ctx->prof_on = true;
    ctx->prof_used = 0;
    ctx->prof_ts_layer.clear();
    ctx->prof_items = ctx->prof_items_dense = 0.0;
    return 0;
}

extern "C" int pp_profile_end(pp_ctx* ctx, double* avg_ms, int32_t* launches, double* flops)
{
    if (!ctx || !avg_ms || !launches || !flops) return PP_E_ARG;
    ctx->prof_on = false;
    double tot = 0.0;
    const size_t n = ctx->prof_used / 2;
    for (size_t i = 0; i < n; ++i) {
        PP_HIP(hipEventSynchronize(ctx->prof_ev[2 * i + 1]));
        float ms = 0.f;
        PP_HIP(hipEventElapsedTime(&ms, ctx->prof_ev[2 * i], ctx->prof_ev[2 * i + 1]));
        tot += ms;
    }
    // items the listed launches really ran (their counts live on the device; the loop above has synchronised).  Every pass rebuilds the
    // lists, so the counts are those of the last profiled pass: exact when the profiled passes see the same frames.
    for (int e : ctx->prof_ts_layer) {
        int32_t cnt = 0;
        if (int rc = pp_ts_read_count(ctx, e & 0xFF, &cnt)) return rc;
        ctx->prof_items += (double)cnt * (e >> 8);
    }
    ctx->prof_ts_layer.clear();
    *avg_ms = n ? tot / (double)n : 0.0;
    *launches = (int32_t)n;
    *flops = ctx->prof_flops;
    ctx->prof_used = 0;
    return 0;
}

extern "C" int pp_effective_precision(pp_ctx* ctx)
{
    if (!ctx || !ctx->net || !ctx->weights_ready) return -1;
    const pp_net* net = (const pp_net*)ctx->net;
    return net->up16 ? 4 : net->eff_prec;
}

extern "C" const char* pp_dominant_kernel(pp_ctx* ctx)
{
    if (!ctx || !ctx->net) return "";
    pp_net* net = (pp_net*)ctx->net;
    for (const Layer& L : net->layers)
        if (L.kind == 0 && L.level == 0 && L.stride == 1) return L.var.name;
    return "";
}

// Executed MFMA flops / algorithmic (direct-convolution) flops of the dominant layer's tiling: Winograd F(2x2,3x3)
// issues 16 multiplications per 2x2 output tile where the direct form needs 36, F(4x4,3x3) 36 per 4x4 tile against 144;
// split-bf16 issues three MFMAs per product.
extern "C" double pp_dominant_executed_ratio(pp_ctx* ctx)
{
    if (!ctx || !ctx->net) return 1.0;
    pp_net* net = (pp_net*)ctx->net;
    for (const Layer& L : net->layers)
        if (L.kind == 0 && L.level == 0 && L.stride == 1) // x the share of the dense work items the profiled launches ran (tile skipping)
            return executed_ratio(L.var) * (ctx->prof_items_dense > 0.0 ? ctx->prof_items / ctx->prof_items_dense : 1.0);
    return 1.0;
}

// The network's launch plan as text, one line per conv / deconv / head layer in execution order:
//   "<index> kind=<0 conv3x3|1 deconv|2 head> cin=<> cout=<> stride=<> up=<> level=<> wino=<family number> tiling=<name>"
// (bench.py derives the executed MFMA flops of a frame from it and records it in its JSON line).
extern "C" int pp_layer_tilings(pp_ctx* ctx, char* buf, int cap)
{
    if (!ctx || !ctx->net) return 0;
    pp_net* net = (pp_net*)ctx->net;
    std::string t;
    char line[256];
    int i = 0;
    for (const Layer& L : net->layers) {
        snprintf(line, sizeof(line), "%d kind=%d cin=%d cout=%d stride=%d up=%d level=%d wino=%d tiling=%s\n", i++, L.kind, L.cin, L.cout, L.stride, L.up, L.level,
                 (int)L.var.family, L.var.name);
        t += line;
    }
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int)t.size();
}

// The tuner's table (layer signature -> tiling name) as text, one "signature<TAB>tiling" line each: rank 0 of a
// multi-GPU job tunes, exports and broadcasts it, the other ranks import it before they create their context, so
// every rank runs identical kernels.  pp_tune_export returns the length needed (excluding the NUL).
extern "C" int pp_tune_export(char* buf, int cap)
{
    std::string t;
    for (auto& kv : tune_cache()) t += kv.first + "\t" + kv.second + "\n";
    if (buf && cap > 0) {
        const size_t n = std::min((size_t)cap - 1, t.size());
        memcpy(buf, t.data(), n);
        buf[n] = 0;
    }
    return (int)t.size();
}

extern "C" int pp_tune_import(const char* text)
{
    if (!text) return PP_E_ARG;
    int n = 0;
    const char* p = text;
    while (*p) {
        const char* e = strchr(p, '\n');
        const size_t len = e ? (size_t)(e - p) : strlen(p);
        std::string line(p, len);
        const size_t tab = line.find('\t');
        if (tab != std::string::npos && tab > 0 && tab + 1 < line.size()) { tune_cache()[line.substr(0, tab)] = line.substr(tab + 1); ++n; }
        p += len + (e ? 1 : 0);
    }
    return n;
}
