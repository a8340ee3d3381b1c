// Private to the host side of the 2D backbone (RPN) + shared head: the network's types and what its three files share.
//   conv_plan.hip    what a context decides once: menus, the families' rules, the weight packer, the tuner, create / commit
//   conv_run.hip     what runs per frame: launch_conv, the norm kernels, the backbone pass, the head, the tap entry points
//   conv_inspect.hip what tests, training and tools read back: image maps, frame tensors, single layers, profile, plan text
// The kernels live one family per file and export menus and weight images through conv_common.h.
#pragma once
#include "pp_common.h"
#include "conv_common.h"

namespace ppc {

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
    // copy hooks of the tap entry points, one per level b (null: inert; armed for one single-frame pass):
    float* unit_tap[3] = {}; // caller memory f32[n_b][C_b][H>>b][W>>b] for the inputs of block b + 1's units (n_b = 3, 5, 5); pp_backbone_block_taps arms level 2
    float* z_tap[3] = {};    // caller memory f32[C_b][H>>b][W>>b] for the raw output of level b's strided conv; pp_backbone_stage_taps arms level 2
    // the lock-step training pass of the BatchNorm backbone (pp_backbone_train_taps_bn), armed for one pass: every norm site accumulates
    // its statistics as on the InstanceNorm backbone, bn_pass_finalize pools them over the frames behind the producer, and consumers read
    // the pass's own fold (bnp_scale / bnp_shift, laid out as bn_scale / bn_shift, which the pass leaves alone)
    bool bn_pass = false;
    float* bnp_scale = nullptr;
    float* bnp_shift = nullptr;
    const float* const* bnp_gb = nullptr; // the 38 device pointers (gamma, beta) of the nineteen layers in bn_sites() order
    float* bnp_out[4] = {};               // caller memory f32[19][256] each: mean, var, scale, shift
    double* dbg_stats = nullptr; // statistics accumulators of pp_debug_layer (allocated on its first call that asks for statistics)
    int w4_strips = -1; // PP_W4_STRIPS, read once at pp_create: -1 cost model, 0 never, 2 whenever whole main tiles exist (parity tests of the strip tiles)
};

constexpr int kC[3] = {64, 128, 256};
constexpr size_t STAT_FS = (size_t)24 * NREP * 320 * 2; // doubles of statistics per frame

// Block b (0..2) of the RPN: a strided conv, block_units(b) Resnet units, an upsampler.  Every unit but the block's last has two convs.
inline int block_units(int b) { return b == 0 ? 2 : 3; }
inline bool unit_two_convs(int b, int u) { return u != block_units(b) - 1; }

// Normalisation sites, numbered in execution order.  Per block b (0..2):
//   site 8b+0: norm after the strided conv (.1)        site 8b+1+2u: Resnet2 unit u first norm (.0)
//   site 8b+2+2u: unit u second norm (.3)              site 8b+7: norm after the deconv
inline int site_block(int b, int k) { return 8 * b + k; }

// The head's three convolutions in the row order of its GEMM: cls na | box 7 na | dir 2 na for na anchors per location
struct HeadPart { const char *weight, *bias; int rows_per_anchor; };
constexpr HeadPart kHead[3] = {{"heads.conv_cls.weight", "heads.conv_cls.bias", 1},
                               {"heads.conv_box.weight", "heads.conv_box.bias", 7},
                               {"heads.conv_dir.weight", "heads.conv_dir.bias", 2}};
// GEMM rows of the head, padded to whole 96-row blocks (the head tilings are 96 rows tall; the reference's 9 anchors give 90 -> 96)
inline int head_rows(int na) { return ((10 * na + 95) / 96) * 96; }
// GEMM rows of a layer (virtual channels of an upsampler: cout up^2)
inline int layer_rows(const pp_ctx* ctx, const Layer& L)
{
    return L.kind == 2 ? head_rows(ctx->cfg.num_anchor_per_loc) : L.kind == 1 ? L.cout * L.up * L.up : L.cout;
}

// One launch of a layer: what launch_conv reads beside the layer itself.  A call site names what it sets.
struct ConvCall {
    const float* in = nullptr;
    int Hin = 0, Win = 0;
    float* out = nullptr;       // the head's cls tensor
    int Hout = 0, Wout = 0;
    const float* res = nullptr; // residual, laid out like `out`
    NormRef pre;                // the producer's normalisation (default: raw input)
    double* stat = nullptr;     // statistics of the output, for stat_C channels
    int stat_C = 0;
    float* out_box = nullptr;   // head
    float* out_dir = nullptr;
    int nb = 1;                 // frames
    size_t out_fs = 0;          // floats between frames of `out` (0: the natural stride)
    const int32_t* pmap = nullptr; // sparse BEV input of the first conv: pillar-index maps + PFN rows
    const float* feat = nullptr;
    int ts_k = 0;               // tile skipping: ordinal (1..3) of the layer among level 0's stride-1 layers, 0: dense
};

// ---- conv_plan.hip ----
const Variant& strip_v(Family f); // strip tilings of the wino4 / wino6 region launches: 4 px wide, 64 px tall
const Variant& strip_h(Family f); // 64 px wide, 4 px tall
// the per-family rules of the tuner and the launcher
bool variant_ok(const Variant& v, int rows);
bool shape_ok(const Variant& v, int Hin, int Win, int Wout);
size_t layer_lds(const Variant& v, int cin);
bool tiling_legal(const Variant& v, int rows, int cin, int Hin, int Win, int Wout); // variant_ok, shape_ok and the LDS budget: the tuner's rule
bool finalises_in_prologue(Family f);
double executed_ratio(const Variant& v);
// L.var's image of the layer's host weights -> L.w (replaces the device copy).  index_positions: the transform (U = G g G^T of the
// Winograd families, the identity elsewhere) is replaced by position indices -- element k of the transformed [rows][cin][taps_eff]
// array holds the float k + 1 -- so the image that comes out is the layout alone (layer_position_map); conv3x3 layers on fp32 tilings only
int pack_layer(pp_ctx* ctx, Layer& L, bool index_positions = false);
std::map<std::string, std::string>& tune_cache(); // layer signature -> tiling name, per process

// ---- conv_run.hip ----
int launch_conv(pp_ctx* ctx, const Layer& L, const ConvCall& call, hipStream_t stream);
// the cls-only head pass as a launch: the head layer with the cls tiling v and one 16-row block
int launch_head_cls(pp_ctx* ctx, const Variant& v, const float* in, const NormRef& pre, float* cls, int nb, hipStream_t stream);
int launch_norm_relu(pp_ctx* ctx, const float* x, float* y, int C, int HW, const NormRef& pre, double* stat, hipStream_t stream,
                     int B = 1, int x16 = 0, int y16 = 0);
NormRef norm_ref(pp_ctx* ctx, int site, int C, int coff, size_t count); // statistics slot / folded-BN arrays for a site
double* stat_slot(pp_ctx* ctx, int site);
// do all stride-1 layers of level 0 (at most three: tile_skip.hip's rule) run the fp32 wino6 main tile on a map of whole main tiles?
bool level0_main_wino6(const pp_net* net, int h, int w);

} // namespace ppc
