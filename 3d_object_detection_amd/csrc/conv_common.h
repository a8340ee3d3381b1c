// Shared by the conv kernels' translation units -- one per kernel family (conv_direct.hip, wino2.hip, wino4.hip, gemm1x1.hip,
// conv16.hip, wino6.hip) and the host side that composes their menus, packs their weights and launches them (conv_plan.hip, conv_run.hip,
// conv_inspect.hip; conv_net.h): kernel parameter block, launch-plan entry, XCD-aware block numbering, the small device helpers and what
// each family exports -- its menu and the weight image its kernel reads.  gfx950 only.
#pragma once
#include <cstring>
#include <type_traits>
#include "pp_common.h"

namespace ppc {

// Workgroups of a launch are dealt round-robin over the 8 XCDs in linear-id order (x fastest), each XCD with
// its own 4 MB L2.  Re-number them so that XCD k works through the k-th CONTIGUOUS eighth of the
// (cout-block fastest, then tile, then frame) order: the cout blocks of one tile (same input patch) and
// neighbouring tiles (shared halo lines) then meet in one L2 instead of each fetching across the fabric.
struct BlockId { int x, y, z; };
static __device__ __forceinline__ BlockId xcd_block_id()
{
    const unsigned gx = gridDim.x, gy = gridDim.y, gz = gridDim.z;
    const unsigned n = gx * gy * gz;
    const unsigned lin = blockIdx.x + gx * (blockIdx.y + gy * blockIdx.z);
    const unsigned per = n >> 3;
    const unsigned l2 = (lin < per * 8) ? (lin & 7) * per + (lin >> 3) : lin;
    BlockId b;
    b.y = (int)(l2 % gy);
    const unsigned t = l2 / gy;
    b.x = (int)(t % gx);
    b.z = (int)(t / gx);
    return b;
}

typedef float f32x4 __attribute__((ext_vector_type(4)));
// dword-aligned vector stores (global memory takes multi-dword accesses at dword alignment)
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef float f32x2u __attribute__((ext_vector_type(2), aligned(4)));
typedef _Float16 f16x4_t __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2_t __attribute__((ext_vector_type(2)));
typedef float f32x2_t __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ unsigned pk_f16(float a, float b) // round to nearest even (v_cvt_pk_f16_f32 on gfx950)
{
    return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_t){a, b}, f16x2_t));
}

// Sum over the 16 lanes that share lane >> 4 (one row of the 16x16 MFMA tile = one DPP row), on the VALU: two quad
// permutes, row_half_mirror, row_mirror.  After each step all lanes of the merged group hold the same value, so the
// result is bit-identical to the xor-shuffle butterfly (1, 2, 4, 8) it replaces -- which hipcc turned into four
// dependent ds_bpermute per value (64 LDS round trips per Winograd tile and wave).
template <int CTRL>
static __device__ __forceinline__ float dpp_f32(float v)
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}
static __device__ __forceinline__ float row16_sum(float v)
{
    v += dpp_f32<0xB1>(v);  // quad_perm [1,0,3,2]
    v += dpp_f32<0x4E>(v);  // quad_perm [2,3,0,1]
    v += dpp_f32<0x141>(v); // row_half_mirror
    v += dpp_f32<0x140>(v); // row_mirror
    return v;
}

constexpr int NREP = 8; // replicated statistics accumulators (spreads atomic contention)

// compile-time for: f(integral_constant<int, I>) for I in [B, E)
template <int B, int E, typename F>
static __device__ __forceinline__ void pp_steps(F&& f)
{
    if constexpr (B < E) {
        f(std::integral_constant<int, B>{});
        pp_steps<B + 1, E>(f);
    }
}

enum { EPI_PLAIN = 0, EPI_UP2 = 1, EPI_UP4 = 2, EPI_HEAD = 3, EPI_HEAD_CLS = 4 /* the head's cls rows alone (deferred head) */ };
enum { PRE_RAW = 0, PRE_STATS = 1, PRE_AFFINE = 2 };

struct ConvP {
    const float* in;
    const float* w;   // the layer's weight image, as the tiling's family lays it out (the *_pack functions below)
    float* out;
    const float* res; // residual, same layout as out (nullable)
    int Cin, Hin, Win;
    int Cout;         // rows of the GEMM (virtual channels for deconv, 96 for the head)
    int Hout, Wout;   // pixel grid of the GEMM
    int pre;
    const double* pre_acc; // [NREP][Cin][2]
    const float* pre_scale;
    const float* pre_shift;
    double pre_inv_n;
    float eps;
    double* stat_acc; // [NREP][Cstat][2] (nullable)
    int stat_C;       // channels in stat_acc
    // head
    const float* bias;
    float* out_box;
    float* out_dir;
    int n_cls, n_box; // na, 7 na (dir = rest up to n_rows) for na anchors per location (reference: 9, 63)
    int n_rows;       // 10 na (reference: 90)
    int w_bm, w_bmp;  // EPI_HEAD_CLS: row-block height and padded width of the committed full head image `w` points to
    // batch: blockIdx.z = frame; strides in elements between consecutive frames
    size_t in_fs, out_fs, res_fs, box_fs, dir_fs; // floats
    size_t pre_fs, stat_fs;                        // doubles
    size_t aff_fs;                                 // floats between frames of pre_scale / pre_shift (0: shared)
    int nb;                                        // frames (persistent kernels loop over them; others use grid.z)
    // sparse BEV input of the first conv: pillar-index map [Hin*Win] (-1 = empty) + PFN rows [P][64]
    const int32_t* pmap;
    const float* feat;
    size_t pmap_fs, feat_fs;
    // wino4_mfma: the rectangle of output pixels this launch tiles (a layer whose map is not a multiple of the tile is
    // covered by a main launch of whole tiles plus strip launches of thin tiles): origin, exclusive end, tiles in x / y
    int rx0, ry0, rx1, ry1, rnbx, rnby;
    // wino6_mfma's list twin (tile skipping, tile_skip.hip): work item l / ncb is entry {frame * ntile + tile, mult} of `items` instead of
    // (frame, tile) = l / ncb itself, the item count comes from the device, and the tile's statistics are added `mult` times
    const int2* items;
    const int32_t* item_count;
};

// Kernel family of a tiling.  The numbers are part of pp_layer_tilings' text ("wino=<n>").
enum class Family : int {
    Direct = 0,  // conv_mfma: direct convolution
    Wino = 1,    // wino_mfma: Winograd F(2x2,3x3) image
    Gemm1x1 = 3, // gemm1x1: persistent 1x1 GEMM (weights resident)
    Wino4 = 4,   // wino4_mfma: Winograd F(2x2,3x3), one wave per SIMD
    Conv16 = 5,  // conv16.hip: 16-bit operand 3x3 convolutions
    Wino6 = 6,   // wino6.hip: Winograd F(4x4,3x3), positions split over the waves
};

struct Variant { // one compiled tiling
    void (*kern)(const ConvP);
    void (*kern2)(const ConvP) = nullptr; // conv16, stride 2: twin for the sparse BEV input of the first conv (ConvP::pmap); wino6 main tile: the list twin (ConvP::items)
    int bm, bmp, pw, ph, kc, threads, waves, pairs; // pairs = MT*NT tile pairs per wave
    size_t lds;
    char name[48];
    Family family = Family::Direct;
    int prec = 0; // Gemm1x1 / Conv16: 0 fp32 MFMA, 1 split-bf16 (bf16x3), 2 plain bf16, 3 fp16 operands
    int io16 = 0; // Gemm1x1 / Conv16: bit 0 = the input tensor is fp16, bit 1 = the output tensor (and residual) is (pp_set_precision 4)
    int wpc = 1;  // Gemm1x1: persistent workgroups per CU
};

// Every family's translation unit exports its tilings as menu functions that append to `menu` in a fixed order: the order decides
// menu[0], ties of the tuner and the entry PP_AUTOTUNE=0 takes, and menu.size() is part of the tune-cache key (conv_plan.hip: layer_menu).
// It also exports the weight image of its tilings, next to the kernel whose LDS reads define it: a plain host function from the layer's
// weights w [rows][cin][taps] (rows = GEMM rows; pack_layer, conv_plan.hip, gathers them) to the image that is uploaded as ConvP::w.

// The blocking conv_mfma, wino_mfma and wino4_mfma share: [row block of bm][cin chunk of kc][tap][k][bmp columns], a chunk of one block
// being one LDS fill, zero in the padding; col(mm) is the column row mm of a block lands in, the family's own
template <typename Col>
inline void pack_blocked(const std::vector<float>& w, int rows, int cin, int taps, const Variant& v, Col col, std::vector<float>& out)
{
    const int nblk = pp_div_up(rows, v.bm), nchunk = cin / v.kc;
    out.assign((size_t)nblk * nchunk * taps * v.kc * v.bmp, 0.f); // LDS image incl. row padding
    for (int b = 0; b < nblk; ++b)
        for (int ch = 0; ch < nchunk; ++ch)
            for (int t = 0; t < taps; ++t)
                for (int k = 0; k < v.kc; ++k)
                    for (int mm = 0; mm < v.bm; ++mm) {
                        const int row = b * v.bm + mm;
                        if (row >= rows) continue;
                        out[((((size_t)b * nchunk + ch) * taps + t) * v.kc + k) * v.bmp + col(mm)] = w[((size_t)row * cin + ch * v.kc + k) * taps + t];
                    }
}
// bf16 images (conv16, gemm1x1): round to nearest even, and back
inline uint16_t to_bf16(float f) { uint32_t u; memcpy(&u, &f, 4); return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16); }
inline float from_bf16(uint16_t h) { uint32_t u = (uint32_t)h << 16; float f; memcpy(&f, &u, 4); return f; }

// conv_direct.hip: conv_mfma -- kind 0: conv3x3 (stride 1 / 2), kind 1: ConvTranspose(k = s = up) for up 1 / 2 / 4, kind 2: the head
void conv_direct_menu(int kind, int stride, int up, std::vector<Variant>& menu);
void conv_direct_pack(const std::vector<float>& w, int rows, int cin, int taps, const Variant& v, std::vector<float>& out);

// wino2.hip: wino_mfma, Winograd F(2x2,3x3), two workgroups per CU; the F(2x2,3x3) weight transform of wino_mfma and wino4_mfma:
// w [n][3][3] -> U = G g G^T [n][4][4] in place
void wino2_menu(std::vector<Variant>& menu, bool roofline_layer);
void wino2_transform(std::vector<float>& w);
void wino2_pack(const std::vector<float>& u /*[rows][cin][16]*/, int rows, int cin, const Variant& v, std::vector<float>& out);

// wino4.hip: wino4_mfma, Winograd F(2x2,3x3), one wave per SIMD -- menu entries and the strip tilings of its region launches
void wino4_menu(std::vector<Variant>& menu, bool roofline_layer);
Variant wino4_strip_v(); // 4 px wide, 64 px tall
Variant wino4_strip_h(); // 64 px wide, 4 px tall
void wino4_pack(const std::vector<float>& u /*[rows][cin][16]*/, int rows, int cin, const Variant& v, std::vector<float>& out);

// gemm1x1.hip: persistent 1x1 GEMM -- the upsamplers (kind 1) and the 9-anchor head (kind 2) at precision prec (0 fp32 ... 4 fp16 tensors),
// the shapes of the cls-only head pass, and the LDS bytes of a launch with K input channels (Variant::lds is 0 for this family).
// head_tile_row: the natural head row (cls 0..8, box 9 + 7a + k, dir 72 + 2a + k) that tile row t of the 96-row head block holds, -1
// for padding; gemm1x1_head_order: the head's weights [>= 90][cin] -> [96][cin] in that order.  Images: fp32 and the 16-bit operand pair
int head_tile_row(int t);
void gemm1x1_menu(int kind, int up, int prec, std::vector<Variant>& menu);
void gemm1x1_cls_menu(std::vector<Variant>& menu);
size_t g1_lds(const Variant& v, int K);
void gemm1x1_head_order(std::vector<float>& w, int cin);
void gemm1x1_pack(const std::vector<float>& w /*[rows][cin]*/, int rows, int cin, const Variant& v, std::vector<float>& out);
void gemm1x1_pack16(const std::vector<float>& w /*[rows][cin]*/, int rows, int cin, const Variant& v, std::vector<uint16_t>& out);

// conv16.hip: 16-bit operand 3x3 convolutions (fp16 / bf16 / split-bf16) -- menu entries for one layer shape and precision
void conv16_menu(int stride, int prec, std::vector<Variant>& menu, int io16 = 0);
void conv16_pack(const std::vector<float>& w /*[rows][cin][9]*/, int rows, int cin, const Variant& v, std::vector<uint16_t>& out);

// wino6.hip: Winograd F(4x4,3x3) on fp32 MFMA -- menu entry, the strip tilings of its region launches, the weight image
void wino6_menu(std::vector<Variant>& menu, bool roofline_layer);
Variant wino6_strip_v(); // 4 px wide, 64 px tall
Variant wino6_strip_h(); // 64 px wide, 4 px tall
// index_positions: instead of U, element k of (row, cin)'s 6 x 6 block holds the float (row cin + c) 36 + k + 1 (the layout read back as a map)
void wino6_pack(const float* w /*[rows][cin][3][3]*/, int rows, int cin, std::vector<float>& out, bool index_positions = false);
constexpr int W6_FRONT_PAD = 64; // floats in front of every tensor a wino6 launch reads: its dwordx4 patch pieces start one float before a row

} // namespace ppc
