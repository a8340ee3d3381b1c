// Internal definitions shared by the HIP sources of libpp_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <map>
#include <string>
#include <vector>
#include "../../include/pp_hip.h"

#define PP_EMPTY 0x7F7F7F7F  // "no index" sentinel; hipMemsetAsync(…, 0x7F, …) produces it

#define PP_HIP(call)                                                         \
    do {                                                                     \
        hipError_t e_ = (call);                                              \
        if (e_ != hipSuccess) return pp_fail_hip(ctx, e_, #call, __FILE__, __LINE__); \
    } while (0)

// ---- frames of the integer stages ------------------------------------------------------------------
// The voxeliser / mask / PFN / post-processing kernels of a batch (pp_infer_batch) run as ONE launch per stage with
// blockIdx.z = frame; each frame's buffers are looked up in a device-resident table built once.  A stage kernel is a template on
// where its frame comes from (pp_frames_tab / pp_frames_one below): the table, or one entry passed by value for the single-stage
// entry points (grid.z = 1), which put the caller's pointers beside slot 0's scratch.
// Device side: the table entries are typed as GLOBAL pointers.  A pointer loaded from memory carries no address space, so every
// access through these tables used to be flat_load / flat_store (both wait counters, conservative s_waitcnt 0 around each); typed,
// the inlined stage bodies get global_load / global_store.  Same 8-byte layout on the host, which fills the tables.
#if defined(__HIP_DEVICE_COMPILE__)
#define PP_GP __attribute__((address_space(1)))
#else
#define PP_GP
#endif
#define PP_SET(dst, src) dst = (decltype(dst))(src) // host-side fill (the host functions are parsed in the device pass as well)
struct pp_pre_frame {
    int32_t PP_GP *pt_cell, *cell_first, *wave_cnt, *pt_rank, *slots, *scalars, *occ;
    float PP_GP* voxels;
    int32_t PP_GP *coors, *npts, *num;
    uint8_t PP_GP* mask;
    float PP_GP* feat;
    int32_t PP_GP* pmap;
};
struct pp_post_frame {
    const float PP_GP *cls, *box, *dir;
    const uint8_t PP_GP* mask;
    uint64_t PP_GP *cand, *shortl, *sel, *nmask;
    int32_t PP_GP *counters, *hist, *dirl;
    float PP_GP *boxes, *nbox;
};
// frame source of a stage kernel, its first argument (the voxeliser's second, behind the clouds): `const F f = src.get();`, or
// src.at(fr) where blockIdx.z is not the frame alone
template <class F> struct pp_frames_tab { // pp_infer_batch: entries of ctx->d_pre / d_post
    const F* tab;
    __device__ F at(int fr) const { return tab[fr]; }
    __device__ F get() const { return tab[blockIdx.z]; }
};
template <class F> struct pp_frames_one { // the single-stage entry points
    F f;
    __device__ F at(int) const { return f; }
    __device__ F get() const { return f; }
};
#define PP_GROUP 32 // frames per batched launch of the integer stages (kernel-argument table size: 384 B of the 4 KB)
struct pp_in_group {
    const float* pts[PP_GROUP];
    int32_t n[PP_GROUP];
};

struct pp_tensor_h {
    std::vector<int64_t> shape;
    std::vector<float> data;
};

// one conv-like layer after packing (see conv_net.h)
struct pp_layer {
    float* w = nullptr;        // packed weights on device
    int cin = 0, cout = 0;     // logical channels (cout = virtual channels for deconv)
    int ks = 1, stride = 1;    // conv kernel / stride (deconv: ks = 1, up = upsample factor)
    int up = 1;
    float* bn_scale = nullptr; // BatchNorm variant: per-input-channel affine folded for the prologue
    float* bn_shift = nullptr;
};

struct pp_slot {
    int32_t* cell_first = nullptr;  // [gx*gy*gz] first point index per cell
    int32_t* pt_cell = nullptr;     // [max_points]
    int32_t* pt_rank = nullptr;     // [max_points] pillar rank of first points
    int32_t* wave_cnt = nullptr;    // [max_points/64 + 8]
    int32_t* slots = nullptr;       // [max_voxels*T] ordered point indices per pillar
    int32_t* vox_scalars = nullptr; // [4]: istar, P_all
    int32_t* occ = nullptr;         // [gx*gy] occupancy -> summed-area table
    void* post = nullptr;           // pp_post workspace (postprocess.hip)
};

struct pp_ctx {
    pp_config cfg;
    int device = 0;
    std::string err;
    // ---- geometry ----
    int gx = 0, gy = 0, H = 0, W = 0; // BEV grid and level-1 feature map (H = gx/2 along x, W = gy/2 along y)
    int max_batch = 1;                // frames per batched launch (cfg.max_batch)
    int64_t A = 0;                    // anchors
    // ---- per-frame scratch of the integer stages: one slot per frame of a batch (the batched stage kernels look a frame's
    //      buffers up in device tables built from these) ----
    std::vector<pp_slot> slot;     // [max_batch]; the single-stage entry points use slot 0
    pp_pre_frame* d_pre = nullptr;   // [max_batch] device tables (built by pp_build_tables for the current anchor count)
    pp_post_frame* d_post = nullptr;
    int64_t tab_A = -1;
    float* anchors = nullptr;      // [A,7]
    int32_t* rect_x = nullptr;     // separable cell rectangles: [types, H, 2] (minx,maxx) / [types, W, 2] (miny,maxy)
    int32_t* rect_y = nullptr;
    int32_t* rects = nullptr;      // full [A,4] table (fallback when not separable)
    int rect_separable = 0;
    // ---- frame buffers (pp_infer_frame) ----
    float* f_voxels = nullptr; int32_t* f_coors = nullptr; int32_t* f_npts = nullptr; int32_t* f_num = nullptr;
    float* f_feat = nullptr; float* f_canvas = nullptr; uint8_t* f_mask = nullptr; int32_t* f_pmap = nullptr;
    float* f_cls = nullptr; float* f_box = nullptr; float* f_dir = nullptr;
    // ---- network ----
    std::map<std::string, pp_tensor_h> host_w;
    bool weights_ready = false;
    float* pfn_w = nullptr;     // [9][64] transposed
    float* pfn_scale = nullptr; // [64]
    float* pfn_shift = nullptr; // [64]
    void* net = nullptr;        // opaque pp_net (conv_net.h)
    int precision = 0;          // pp_set_precision: 0 fp32 MFMA, 1 split-bf16 (bf16x3), 2 bf16, 3 fp16 operands -- convs, upsamplers and head
    // ---- measurement (pp_profile_begin/end) ----
    bool prof_on = false;
    std::vector<hipEvent_t> prof_ev; // start/stop pairs
    size_t prof_used = 0;
    double prof_flops = 0.0;
    // ---- per-stage timing (pp_stage_profile_begin/end): one event per stage boundary on the caller's stream ----
    bool stage_on = false;
    std::vector<hipEvent_t> stage_ev;
    std::vector<int> stage_id; // stage that FOLLOWS event i (-1: end of the pass)
    std::vector<hipStream_t> stage_stream; // stream event i was recorded on (an interval needs both ends on one stream)
    size_t stage_used = 0;
    int last_nb = 0;                  // frames of the last completed pp_infer_batch / pp_infer_frame pass (pp_batch_loss reads them)
    // ---- target assignment / loss (assign.hip): per-class IoU thresholds (pp_set_assign_thresholds; host side) and the device
    //      workspace, allocated on the first assignment or loss call ----
    bool asg_thr_set = false;
    float asg_thr_m[PP_MAX_CLASSES] = {}, asg_thr_u[PP_MAX_CLASSES] = {};
    void* asg = nullptr;
    // ---- loss gradient / head backward (train.hip): workspace allocated on first use; commit_gen counts pp_commit_weights calls so
    //      the natural-order copy of the head weights and the index map of the head's packed image are rebuilt after a commit ----
    uint64_t commit_gen = 0;
    void* trn = nullptr;
    void* neck = nullptr;            // neck backward (neck_ws, neck_train.h): dZ workspace, dW partials, index maps of the upsampler images
    void* blk = nullptr;             // Resnet unit backward (block_ws, block_train.h): padded a / dz planes, transposed weights, dW partials
    void* down = nullptr;            // strided stage backward (down_ws, down_train.h): parity planes of x, dz planes, transposed weights, dW partials
    void* pfnt = nullptr;            // PFN training (pfn_train.hip): fp64 partials of both reductions, the batch-statistics scale / shift
    void* img16 = nullptr;           // in-place writer of the 16-bit weight images (image16.hip): the element maps of the twenty layers
    void* optim = nullptr;           // device optimizer (optim.hip): fp64 partials of the gradient norm, one per chunk
    int train_chunk_frames = 0;      // pp_set_train_chunk_frames: cap on the frames of a chunk of every training backward (0: the workspace rule alone)
    // ---- deferred head (pp_set_head_defer): the passes of pp_infer_batch run the cls rows for every pixel and the box / dir logits for
    //      the selected candidates only; f_box / f_dir are then stale until pp_head_materialise runs the full head over the retained
    //      concat buffer and statistics of that pass ----
    bool head_defer = true;          // the switch (default on; PP_HEAD_DEFER=0 forces it off)
    bool head_defer_env_off = false;
    bool head_stale = false;         // f_box / f_dir do not hold the last pass
    int stale_nb = 0;                // frames of that pass
    hipStream_t stale_stream = nullptr;
    // ---- sparse first convolution (sparse_conv1.hip; pp_set_sparse_conv1): the fused fp32 path computes the first conv for the output
    //      pixels that see a pillar only ----
    bool sparse_conv1 = true;        // the switch (default on; PP_SPARSE_CONV1=0 forces it off)
    bool sparse_conv1_env_off = false;
    void* sc1 = nullptr;             // weight image, active lists and their workspace
    int sc1_kc = 4;                  // channels per chunk of the committed dense first-conv tiling: the sparse kernel walks K in its order
    int sc1_last_nb = 0;             // frames of the last pass whose active lists the context holds (0: that pass ran the dense first conv)
    // ---- tile skipping (tile_skip.hip; pp_set_tile_skip): behind the sparse first conv, the fp32 wino6 launches of level 0's stride-1
    //      layers compute one tile per (frame, layer, border class) of those whose input is constant and copy it to the others ----
    bool tile_skip = true;           // the switch (default on; PP_TILE_SKIP=0 forces it off)
    bool tile_skip_env_off = false;
    void* ts = nullptr;              // flags, item and fill lists
    std::vector<int> prof_ts_layer;  // per profiled launch: the layer ordinal (1..3) of a listed launch, 0 for a dense one
    double prof_items = 0.0, prof_items_dense = 0.0; // items launched / dense items over the profiled launches (pp_profile_end)
};
// stage ids of pp_stage_mark / pp_stage_profile_end
enum { PP_ST_VOXELIZE = 0, PP_ST_MASK = 1, PP_ST_PFN = 2, PP_ST_CONV = 3, PP_ST_NORM = 4, PP_ST_HEAD = 5, PP_ST_POST = 6 /* filter + threshold + gather */,
       PP_ST_POST_TOPK = 7 /* exact top-k + decode */, PP_ST_POST_NMS = 8 /* mask + greedy sweep + flip / range / compaction */, PP_ST_COUNT = 12 };
int pp_stage_mark(pp_ctx* ctx, hipStream_t stream, int id); // no-op unless stage profiling is on

int pp_fail_hip(pp_ctx* ctx, hipError_t e, const char* what, const char* file, int line);
int pp_fail(pp_ctx* ctx, int code, const char* msg);

// stage entry points implemented per file (all enqueue on stream, no sync)
int pp_net_create(pp_ctx* ctx);
void pp_net_destroy(pp_ctx* ctx);
int pp_net_commit(pp_ctx* ctx);
int pp_post_create(pp_ctx* ctx);
// nb canvases (or, when pmap != nullptr, nb sparse BEV inputs: pillar-index maps + PFN rows) -> pre-norm [nb,320,H,W] + stats
int pp_run_backbone(pp_ctx* ctx, const float* canvas, int nb, hipStream_t stream, const int32_t* pmap, const float* feat);
int pp_pillar_map(pp_ctx* ctx, const int32_t* coors, const int32_t* num_pillars, int32_t* pmap, hipStream_t stream);
// batched integer stages: frames b0 .. b0+g-1 of a batch, one launch per stage (blockIdx.z = frame)
int pp_build_tables(pp_ctx* ctx);
void pp_post_fill_table(pp_ctx* ctx, int slot, pp_post_frame* f);
int pp_voxelize_group(pp_ctx* ctx, int b0, int g, const pp_in_group& in, hipStream_t stream);
int pp_anchor_mask_group(pp_ctx* ctx, int b0, int g, hipStream_t stream);
int pp_pfn_pmap_group(pp_ctx* ctx, int b0, int g, hipStream_t stream);
int pp_postprocess_group(pp_ctx* ctx, int b0, int g, float* det, int32_t* det_count, int nms_mode, hipStream_t stream,
                         int defer_nb = 0); // defer_nb > 0: box / dir logits come from the candidate head (a deferred pass of defer_nb frames)
int pp_run_head_fused(pp_ctx* ctx, float* cls, float* box, float* dir, int nb, hipStream_t stream); // norm+ReLU fused in the prologue
// deferred head (conv_run.hip): is it what pp_infer_batch runs; the cls-only pass (marks f_box / f_dir stale); the full tensors on demand
// (no-op unless stale) -- to be called by whatever reads f_box / f_dir or overwrites the concat buffer, its statistics or the head weights
bool pp_head_defer_on(pp_ctx* ctx);
int pp_run_head_cls(pp_ctx* ctx, float* cls, int nb, hipStream_t stream);
int pp_head_materialise(pp_ctx* ctx, hipStream_t stream);
struct pp_head_gather { // inputs of the candidate head (postprocess.hip)
    const float* w; int bm, bmp, K;  // the head image [row block][K][bmp] in head_tile_row order
    const float* bias_perm;
    const float* in; size_t in_fs; int HW; // concat buffer [nb][K][HW], pre-norm
    int pre; const double* pre_acc; size_t pre_fs; double pre_inv_n; const float *pre_scale, *pre_shift; size_t aff_fs; float eps;
};
int pp_net_head_gather(pp_ctx* ctx, int nb, pp_head_gather* g);
// sparse first convolution (sparse_conv1.hip): workspace at pp_create, weight image at pp_commit_weights; usable = switched on, image
// committed, offsets fit 32 bits.  pp_sc1_run: nb pillar maps + PFN rows -> dense pre-norm [nb][64,H,W] (+ statistics; stat nullable)
int pp_sc1_create(pp_ctx* ctx);
void pp_sc1_destroy(pp_ctx* ctx);
int pp_sc1_commit(pp_ctx* ctx);
int pp_sc1_update(pp_ctx* ctx, const float* w, hipStream_t stream); // the device tensor rpn.block1.0.weight -> the committed image, in place
const float* pp_first_conv_image(pp_ctx* ctx, size_t* bytes); // the committed weight image (null before a commit): pp_weight_image
bool pp_sc1_usable(pp_ctx* ctx);
int pp_sc1_run(pp_ctx* ctx, const int32_t* pmap, const float* feat, float* out, double* stat, size_t stat_fs, int nb, hipStream_t stream);
int pp_sc1_fetch_list(pp_ctx* ctx, int frame, void* dst, hipStream_t stream);
const uint64_t* pp_sc1_words(pp_ctx* ctx, int* nblk); // ballot words [max_batch][nblk * 4] of the last pp_sc1_run (complete even when the list is capped)
// tile skipping (tile_skip.hip): workspace at pp_create (sized for max_batch).  usable = switched on, the map is a whole number of
// 16 x 16 tiles and level 0 has at most three stride-1 layers.  pp_ts_build: flags, item lists and fill lists of the three layers for
// nb frames, from the sparse first conv's ballot words of this pass (words == nullptr) or from given ones.  pp_ts_list: the item list
// and device count of layer ordinal k (1..3) if lists for nb frames are in place.  pp_ts_fill: copy the representatives' tiles of
// layer k in `out` [nb][C][H][W] to the skipped tiles.
int pp_ts_create(pp_ctx* ctx);
void pp_ts_destroy(pp_ctx* ctx);
bool pp_ts_usable(pp_ctx* ctx, int level0_layers);
void pp_ts_begin_pass(pp_ctx* ctx);
int pp_ts_build(pp_ctx* ctx, int nb, const uint64_t* words, hipStream_t stream);
int pp_ts_build_from_bitmap(pp_ctx* ctx, int nb, const uint8_t* bitmap, hipStream_t stream);
void pp_ts_mark_pass(pp_ctx* ctx, int nb);
void pp_ts_begin_hook(pp_ctx* ctx, bool builds);
void pp_ts_end_hook(pp_ctx* ctx);
bool pp_ts_list(pp_ctx* ctx, int k, int nb, const int2** items, const int32_t** count);
int pp_ts_fill(pp_ctx* ctx, int k, int nb, float* out, size_t out_fs, int C, hipStream_t stream);
int pp_ts_dense_items(pp_ctx* ctx, int nb);
int pp_ts_read_count(pp_ctx* ctx, int k, int32_t* n);
int pp_ts_fetch_flags(pp_ctx* ctx, int frame, void* dst, hipStream_t stream);
void pp_post_destroy(pp_ctx* ctx);
void pp_assign_destroy(pp_ctx* ctx);
void pp_train_destroy(pp_ctx* ctx);
// The head's packed weight image and biases of the committed plan (conv_inspect.hip), described for pp_update_head_weights (train.hip):
// wmap[i] is the element of the natural [cls | box | dir][320] weight (state_dict order, rows concatenated) that image element i
// holds, -1 for padding; bmap / bpmap likewise for the bias in natural order and in gemm1x1's head_tile_row order (bias_perm is
// null when the plan has no such copy).  PP_E_ARG when the committed plan packs the head in a 16-bit format.
struct pp_head_image {
    float *w = nullptr, *bias = nullptr, *bias_perm = nullptr;
    std::vector<int32_t> wmap, bmap, bpmap;
};
int pp_net_head_image(pp_ctx* ctx, pp_head_image* img, bool any_plan = false);
int pp_net_head_bias(pp_ctx* ctx, pp_head_image* img); // bias, bmap, bias_perm and bpmap alone (any plan)
// The same for upsampler `branch` (0..2), for pp_update_neck_weights (neck_train.hip): wmap[i] is the element of the state_dict tensor
// rpn.deconv<branch+1>.0.weight [Cin][Cup][s][s] (elems in all) that image element i holds, -1 for padding.
struct pp_layer_image {
    float* w = nullptr;
    size_t elems = 0;
    std::vector<int32_t> wmap;
};
int pp_net_deconv_image(pp_ctx* ctx, int branch, pp_layer_image* img, bool any_plan = false);
void pp_neck_destroy(pp_ctx* ctx);
// 3 x 3 convolution k (0 .. 15) of the RPN in execution order, for pp_update_conv_image (block_train.hip): pmap[i] = (row C + c) T + pos
// names the element of the TRANSFORMED weight [rows][C][T] that image element i holds (T = 36 | 16: position of U = G g G^T of the
// Winograd families; 9: the tap of the direct tilings), -1 for padding.  fp32 images only (PP_E_ARG otherwise); a strided convolution
// must run a direct tiling, so T = 9 there.
struct pp_block_image {
    float* w = nullptr;
    int C = 0, T = 0; // C: input channels
    int rows = 0;     // output channels (= C for a unit)
    std::vector<int32_t> pmap;
};
int pp_net_conv_image(pp_ctx* ctx, int k, pp_block_image* img, bool any_plan = false);
void pp_block_destroy(pp_ctx* ctx);
void pp_down_destroy(pp_ctx* ctx);
void pp_pfn_train_destroy(pp_ctx* ctx);
void pp_optim_destroy(pp_ctx* ctx);
// The one writer behind pp_update_{block,down,rpn}_weights (block_train.hip): the committed image of 3 x 3 convolution k of the RPN's
// sixteen in execution = state_dict order (per level its strided convolution, then its 3 | 5 | 5 units; so 10 is block 3's strided
// convolution and 11 .. 15 its units) <- the state_dict tensor w [rows][cin][3][3] on the device, in place on `stream`.  Image element
// i becomes position pmap[i] % T of the transformed weight of (row, cin) = pmap[i] / T, 0 for padding; the map is read back once per
// commit, on the image's first update.  The callers check their arguments, the precision mode and set the device.
// any_plan: the committed plan may run a 16-bit mode, in which convolution k keeps an fp32 tiling (the _mp updates: a shape no 16-bit
// tiling takes); the default refuses every plan but an fp32 one, as pp_net_conv_image / _deconv_image / _head_image do.
int pp_update_conv_image(pp_ctx* ctx, int k, const float* w, hipStream_t stream, bool any_plan = false);

// ---- the 16-bit weight images (image16.hip; the maps by conv_inspect.hip) ----
// Layer `layer` (0 .. 19) of the committed plan as the in-place writer sees it.  is16: the image holds 16-bit elements (conv16_pack,
// gemm1x1_pack16); otherwise it is an fp32 image and map stays empty (the fp32 writers own it).  map[i] = 2 e + part for image element i:
// e the element of the concatenation of the layer's state_dict tensors (a convolution's or an upsampler's weight; cls | box | dir of the
// head), part 0 the rounded value (bf16, or fp16 when fp16 is set), 1 the bf16 residual lo = bf16(x - hi); -1 for padding.  Read back
// from the packers themselves: three passes of base-128 digits, each digit a value whose two parts are both exact and non-zero.
struct pp_image16 {
    void* w = nullptr;
    size_t bytes = 0;
    bool is16 = false, fp16 = false;
    std::vector<int32_t> map;
};
int pp_net_layer_index(pp_ctx* ctx, int kind, int ordinal); // conv3x3 k | upsampler branch | the head -> 0 .. 19, -1: no such layer
int pp_net_image16(pp_ctx* ctx, int layer, pp_image16* img);
// Rewrite layer `layer`'s 16-bit image in place on `stream` from the device tensors s0 | s1 | s2 (n0, n1, n2 elements; one tensor for a
// convolution or an upsampler).  *is16 = false and nothing written when the layer keeps an fp32 image.  The map is read back on the
// first call after a commit (synchronous) and cached per commit_gen.
int pp_update_image16(pp_ctx* ctx, int layer, const float* s0, const float* s1, const float* s2, int n0, int n1, int n2, hipStream_t stream,
                      bool* is16);
void pp_image16_destroy(pp_ctx* ctx);
// The guard of the four _mp entries: mode 1 | 2 | 3 and the committed plan's effective precision equals it (so fp16 tensors are off)
int pp_mp_mode_check(pp_ctx* ctx, const char* who, int mode);

// Frames per chunk of a training backward (the twelve pp_{unit,down,neck}_backward* chunk loops and the three _bn entries): as many
// frames as fit `budget` bytes at frame_bytes each, at least 1 and at most nb; then at most the entry's own chunk_frames (0 where the
// entry has none) and at most the context's cap (pp_set_train_chunk_frames), where those are non-zero.  A cap never raises the rule.
static inline int pp_chunk_frames(const pp_ctx* ctx, size_t budget, size_t frame_bytes, int nb, int chunk_frames)
{
    int fc = (int)(budget / frame_bytes);
    fc = fc < 1 ? 1 : fc > nb ? nb : fc;
    if (chunk_frames > 0 && chunk_frames < fc) fc = chunk_frames;
    if (ctx->train_chunk_frames > 0 && ctx->train_chunk_frames < fc) fc = ctx->train_chunk_frames;
    return fc;
}

static inline int pp_div_up(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }
