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
#include <cstdio>
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

// Tiling menu.  The 16-pixel N-tile is TW x (16/TW); a workgroup covers BTX x BTY tiles.  The maps of
// eight_20cm are 400/200/100 = 16*25 / 8*25 / 4*25, so NT=5 shapes tile them exactly; the 4x4 / 2x2 shapes
// are the general fallback (edge tiles masked).  Which entry runs a layer is MEASURED on the device at
// pp_commit_weights (autotune_layer, conv_plan.hip); the cost model only breaks ties / serves PP_AUTOTUNE=0.
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

} // namespace

namespace ppc {

// kind 0: the 16 tilings of a conv3x3 (stride 1 / 2); kind 1: of a ConvTranspose(k = s = up) as a 1x1 conv with the pixel-shuffle
// epilogue; kind 2: the six 96-row tilings of the head
void conv_direct_menu(int kind, int stride, int up, std::vector<Variant>& menu)
{
    if (kind == 2) {
        menu.push_back(make_variant<1, 1, 16, 1, 4, 6, 5, 1, 16, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 16, 1, 4, 6, 2, 1, 16, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 16, 2, 2, 3, 5, 1, 16, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 16, 2, 4, 3, 5, 1, 32, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 8, 1, 4, 6, 2, 1, 16, EPI_HEAD>());
        menu.push_back(make_variant<1, 1, 8, 2, 2, 3, 4, 2, 16, EPI_HEAD>());
    } else if (kind == 1) {
        if (up == 1) conv_menu<1, 1, 16, EPI_PLAIN>(menu);
        else if (up == 2) conv_menu<1, 1, 16, EPI_UP2>(menu);
        else conv_menu<1, 1, 16, EPI_UP4>(menu);
    } else if (stride == 2) {
        conv_menu<3, 2, 8, EPI_PLAIN>(menu);
    } else {
        conv_menu<3, 1, 8, EPI_PLAIN>(menu);
    }
}
// The image conv_mfma stages: [row block][cin chunk][tap][k][bmp], row mm of a block in column mm (taps: 9 conv3x3, 1 upsampler / head)
void conv_direct_pack(const std::vector<float>& w, int rows, int cin, int taps, const Variant& v, std::vector<float>& out)
{
    pack_blocked(w, rows, cin, taps, v, [](int mm) { return mm; }, out);
}

} // namespace ppc
