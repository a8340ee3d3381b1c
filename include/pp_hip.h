/* pp_hip.h -- C ABI of libpp_hip.so: the MI355X (gfx950) PointPillars inference hot path.
 *
 * The reference (1005088h/3d_object_detection) is pure Python and has no FFI; the
 * boundary it offers is the Python call surface of train.py:192-196,224-230.  Each entry
 * point below is what a ctypes binding for that surface binds (INTEGRATION.md shows the
 * stubs); the "replaces" note cites the reference function it stands in for.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in _h (host);
 *  - the caller allocates every output; functions only enqueue work on `stream`
 *    (a hipStream_t passed as void*; NULL = the default stream) and never synchronise,
 *    except where noted;
 *  - return value: 0 = ok, <0 = -(hipError_t), >0 = argument/state error (PP_E_*);
 *    pp_last_error(ctx) returns a static, human readable message for the last failure;
 *  - one pp_ctx per GPU/stream; a ctx is not re-entrant, different ctxs are independent.
 */
#ifndef PP_HIP_H
#define PP_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PP_MAX_CLASSES 12 /* class ranges of the anchor table (reference: 3; the build-side nuScenes table: 10) */
#define PP_E_ARG 1      /* bad argument (null pointer, size out of range) */
#define PP_E_STATE 2    /* weights / anchors not loaded yet */
#define PP_E_NAME 3     /* unknown weight name or wrong shape */

typedef struct pp_ctx pp_ctx;

/* Geometry and limits.  Filled by the Python VoxelGenerator/AnchorAssigner mirrors from
 * the same config keys the reference reads (voxel_generator.py:6-26, inference.py:13-19). */
typedef struct pp_config {
    float voxel_size[3];
    float offset[3];          /* detection_offset */
    int32_t grid_size[3];     /* gx, gy, gz (gz must be 1 for the BEV path) */
    int32_t max_voxels;
    int32_t max_num_points;   /* T */
    int32_t num_point_features; /* F: must be 4 for the PFN (its 9 input features x, y, z, i, 3 offsets from the pillar mean, 2 from the
                                 * pillar centre -- pointpillars8_shared.py:30-60 -- and the (64, 9, 1) weight of the state_dict fix it:
                                 * pp_pfn / pp_infer_* refuse other values); pp_voxelize alone takes any F >= 3 */
    int32_t max_points;       /* capacity of the per-point workspace (N upper bound) */
    int32_t num_anchor_per_loc; /* anchors per BEV location = head geometry: cls na, box 7*na, dir 2*na rows (reference: 9) */
    int32_t num_classes;      /* <= PP_MAX_CLASSES (reference: 3) */
    int32_t class_begin[PP_MAX_CLASSES]; /* anchor index ranges, class_masks of anchor_assigner.py:289 */
    int32_t class_end[PP_MAX_CLASSES];
    double center_limit[6];   /* compared in fp64 like inference.py:105-109 (python floats) */
    int32_t norm_kind;        /* 0 = InstanceNorm2d(eps 1e-3) backbone (_shared), 1 = BatchNorm2d (_export/_trt) */
    int32_t nms_pre_max;      /* 1000 */
    int32_t nms_post_max;     /* 300 (<= 1024) */
    float nms_iou_threshold;  /* 0.1  */
    float score_threshold;    /* 0.05 */
    int32_t max_batch;        /* frames per batched launch of pp_infer_batch (>= 1; 0 is read as 1) */
} pp_config;

/* Lifetime.  pp_create allocates all device workspace for the configured sizes. */
pp_ctx* pp_create(int device, const pp_config* cfg);
void pp_destroy(pp_ctx* ctx);
const char* pp_last_error(pp_ctx* ctx); /* ctx may be NULL: last pp_create failure */

/* Weights by state_dict key (replaces net.load_state_dict, train.py:201-202; key names of
 * networks/pointpillars8_shared.py:346-357).  host_ptr is fp32, contiguous.  Call
 * pp_commit_weights once after the last tensor: it folds BN, repacks for the kernels
 * and uploads.  Synchronous. */
int pp_load_weights(pp_ctx* ctx, const char* name, const void* host_ptr_h, const int64_t* shape_h, int ndim);
int pp_commit_weights(pp_ctx* ctx);

/* MFMA operand type of the network behind the PFN -- every 3x3 convolution (stride 1 and 2), the three ConvTranspose(k = s)
 * upsamplers and the head -- SURVEY 8(f).4; the reference's deployed path is TensorRT FP16 (framework/trt_utils.py:30,
 * networks/pointpillars8_trt.py:208-223,295-314):
 *   0 fp32 MFMA (default, exact, the parity path);
 *   1 split-bf16 "bf16x3" (x = hi + lo, three bf16 MFMAs per product, fp32 accumulation: fp32-equivalent for this network,
 *     meets the fp32 parity bar -- DESIGN.md);
 *   2 bf16 operands;   3 fp16 operands (the reference's deploy arithmetic) -- own tolerance table in DESIGN.md;
 *   4 "fp16s": mode 3 plus fp16 STORAGE of every activation tensor behind the first convolution -- the level buffers (block-head
 *     outputs, Resnet2 intermediates, residuals) and the [320,H,W] concat buffer between the upsamplers and the head; TensorRT FP16
 *     engines keep fp16 tensors between layers.  The first conv still reads the fp32 PFN rows / canvas, the logits stay fp32, and the
 *     InstanceNorm statistics are accumulated from the UNROUNDED fp32 values of a layer while its consumer normalises the fp16-rounded
 *     tensor (DESIGN.md tolerance table).  Needs maps that are multiples of 4 pixels wide at all three levels (W a multiple of 16,
 *     H * W of 64) and the 9-anchor head; otherwise the context runs mode 3 -- pp_effective_precision tells which.
 * Modes 1 - 3: accumulation is fp32 and every activation stays fp32 NCHW in HBM (normalise + ReLU in fp32, round while staging).
 * A layer whose shape none of the 16-bit tilings takes (maps not a multiple of 4 wide, Cin not a multiple of 16 / 32) keeps its
 * fp32 tiling: pp_layer_tilings reports what runs.  Call before pp_commit_weights (a change of mode invalidates the committed
 * weights until the next commit). */
int pp_set_precision(pp_ctx* ctx, int mode);
/* The mode the committed launch plan really runs (pp_set_precision's value, except 4 -> 3 where the fp16 tensors are not possible);
 * valid after pp_commit_weights, -1 before. */
int pp_effective_precision(pp_ctx* ctx);

/* Anchor table built by the host mirror of AnchorAssigner.__init__ (anchor_assigner.py:221-298):
 * anchors f32[A,7], cell rectangles i32[A,4] from get_anchor_coor (box_np_ops.py:288-305). Synchronous. */
int pp_set_anchors(pp_ctx* ctx, const float* anchors_h, const int32_t* anchor_rects_h, int64_t num_anchors);

/* replaces VoxelGenerator.generate / points_to_voxels (voxel_generator.py:28-40,82-106).
 * pts f32[n,nfeat] -> voxels f32[max_voxels,T,F] (rows >= *num_pillars untouched), coors i32[max_voxels,3]
 * (x,y,z), npts i32[max_voxels], num_pillars i32[1]. Bit-exact incl. the max_voxels break. */
int pp_voxelize(pp_ctx* ctx, const float* pts, int n, int nfeat, float* voxels, int32_t* coors,
                int32_t* npts, int32_t* num_pillars, void* stream);

/* replaces AnchorAssigner.create_mask (anchor_assigner.py:322-335; box_np_ops.py:168-257).
 * mask u8[A] (0/1). */
int pp_anchor_mask(pp_ctx* ctx, const int32_t* coors, const int32_t* num_pillars, uint8_t* mask, void* stream);

/* replaces PointNet.forward (pointpillars8_shared.py:30-60). feat f32[max_voxels,64], rows < *num_pillars written. */
int pp_pfn(pp_ctx* ctx, const float* voxels, const int32_t* coors, const int32_t* npts,
           const int32_t* num_pillars, float* feat, void* stream);

/* replaces PointPillarsScatter.forward (pointpillars8_shared.py:76-111; CUDA scatter of
 * pointpillars8_trt.py:176-193). canvas f32[64,gx,gy], fully written (zero fill + scatter). */
int pp_scatter(pp_ctx* ctx, const float* feat, const int32_t* coors, const int32_t* num_pillars,
               float* canvas, void* stream);

/* replaces RPN.forward (pointpillars8_shared.py:173-181). canvas f32[64,gx,gy] -> rpn_out f32[320,gx/2,gy/2]. */
int pp_backbone(pp_ctx* ctx, const float* canvas, float* rpn_out, void* stream);

/* replaces SharedHead.forward (pointpillars8_shared.py:323-343). rpn_out f32[320,H,W] ->
 * cls f32[A] , box f32[A,7], dir f32[A,2], ordered (anchor type, x, y). */
int pp_head(pp_ctx* ctx, const float* rpn_out, float* cls, float* box, float* dir, void* stream);

/* replaces Inference.infer_gpu (inference.py:26-138). det f32[num_classes*nms_post_max, 9] rows
 * (x,y,z,l,w,h,r,score,class) grouped by class in class order, det_count i32[1+num_classes]
 * (total, then per class). nms_mode 0 = axis-aligned "+1" NMS (nms.py), 1 = rotated (eval/iou.py). */
int pp_postprocess(pp_ctx* ctx, const float* cls, const float* box, const float* dir, const uint8_t* mask,
                   float* det, int32_t* det_count, int nms_mode, void* stream);

/* First half of pp_postprocess as a stage of its own, behind Inference.infer_torch (inference.py:140-189: per class
 * mask gather, sigmoid, score >= 0.05, top-nms_pre_max).  idx i32[num_classes][nms_pre_max] anchor ids by descending score
 * (ties: lower anchor id; -1 beyond a class's count), score f32[num_classes][nms_pre_max], count i32[num_classes]. */
int pp_select_candidates(pp_ctx* ctx, const float* cls, const float* box, const float* dir, const uint8_t* mask,
                         int32_t* idx, float* score, int32_t* count, void* stream);

/* Fused frame: voxelise -> mask -> PFN -> BEV -> backbone -> head -> post-process, no host sync. */
int pp_infer_frame(pp_ctx* ctx, const float* pts, int n, float* det, int32_t* det_count, int nms_mode, void* stream);

/* nb <= cfg.max_batch independent frames in ONE pass: the conv/deconv/head launches carry the frame as grid.z
 * (per-frame InstanceNorm statistics; same detections as nb calls of pp_infer_frame, logits equal up to the
 * fp32 summation order of those statistics, ~3e-5), the small integer
 * stages run per frame on the same stream.  pts_h / n_h: HOST arrays of nb device pointers / point counts.
 * det f32[nb][num_classes*nms_post_max][9], det_count i32[nb][PP_DET_COUNT_STRIDE] (total, then per class). */
#define PP_DET_COUNT_STRIDE (1 + PP_MAX_CLASSES)
int pp_infer_batch(pp_ctx* ctx, const float* const* pts_h, const int32_t* n_h, int nb, float* det, int32_t* det_count,
                   int nms_mode, void* stream);

/* Inspection hook for the parity tests: copies one tensor of frame `frame` of the LAST pp_infer_batch / pp_infer_frame
 * pass out of the context's internal buffers into caller memory (device pointer, enqueued on stream).
 * kind 0 cls f32[A] | 1 box f32[A,7] | 2 dir f32[A,2] | 3 anchor mask u8[A] | 4 rpn output f32[320,H,W] as RPN.forward
 * returns it (pointpillars8_shared.py:173-181; the fused path never stores it, it is materialised for the copy) |
 * 5 PFN rows f32[max_voxels,64] | 6 coors i32[max_voxels,3] | 7 pillar count i32[1] |
 * 8 active list of the sparse first convolution i32[1 + min(4 max_voxels, H W)]: the count, then the active output pixels
 * (index = x * W + y on the level-0 map) in ascending order, entries past the count unspecified; PP_E_STATE when the last pass
 * ran the dense first convolution |
 * 9 tile flags of the tile-skipping path u8[3][(H / 16) (W / 16)]: 1 = the 16 x 16 tile (index = (x / 16) * (W / 16) + y / 16) is
 * skippable at the first, second, third stride-1 layer of level 0; PP_E_STATE when the last pass built none (see pp_set_tile_skip). */
int pp_fetch_frame_tensor(pp_ctx* ctx, int frame, int kind, void* dst, void* stream);

/* Single-layer hook for the layer tests: runs ONE layer of the committed launch plan -- the kernel, tiling and packed weight image
 * pp_layer_tilings reports for it, whatever PP_FORCE_VARIANT and pp_set_precision selected -- on caller tensors, nb frames
 * (1 <= nb <= cfg.max_batch) in one launch.  layer: 0 .. 19 in plan order (16 convs, 3 upsamplers, the head).  Map sizes are the
 * context's own for the layer's level (h, w = H >> level, W >> level; a stride-2 conv reads 2h x 2w); H, W multiples of 4.
 *   in    [nb][cin][hin][win]; res (NULL or, for a conv, [nb][cout][h][w]) is added before the store and the statistics;
 *   out   conv [nb][cout][h][w] | upsampler [nb][cout][h up][w up], dense (not a slice of the 320-channel buffer) |
 *         head: cls f32[nb][A], with out_box f32[nb][A][7] and out_dir f32[nb][A][2] as pp_head returns them (NULL for other layers);
 *   element types follow the committed tiling's `h<n>` tag in pp_layer_tilings: bit 0 of n = `in` is fp16, bit 1 = `out` and `res`
 *         are fp16; fp32 without the tag.  The head's outputs are always fp32.
 *   pre_mode 0: the kernel reads `in` as it is (scale = shift = NULL); 1: relu(in * scale[c] + shift[c]) with scale / shift f32[cin]
 *         shared by the frames (folded BatchNorm); 2: scale / shift f32[nb][cin], one row per frame (finalised InstanceNorm).
 *         The wino4 / wino6 tilings of the stride-1 convolutions always normalise (in the network such a layer always follows a norm):
 *         pre_mode 0 on a layer that runs one of them is PP_E_ARG.
 *   layer 0 alternatively takes the sparse form of the fused path: in = NULL, pmap i32[nb][gx gy] (pillar index per BEV cell, -1 =
 *         empty) and feat f32[nb][max_voxels][64] (PFN rows), which runs the tiling's sparse twin.
 *   stats (NULL or f64[nb][cout][2]): per frame and output channel the sum and the sum of squares the epilogue accumulates for the
 *         consumer's InstanceNorm (of the fp32 values, before a 16-bit store), summed over the replicated accumulators; not the head.
 * `in` must be readable 256 bytes in front of its first and 256 bytes behind its last element, whatever its element type: the
 * wino6 tilings fetch a patch row as whole 16-byte pieces, which start one float in front of a map row and end up to 63 floats behind
 * it (the context's own buffers carry at least this slack).  Every other kernel family, the 16-bit ones on fp16 tensors included,
 * keeps the fetches of its masked-out lanes inside `in`.  What lies in that slack, and anywhere else outside the tensors handed in,
 * influences no result (tests/test_layer_arena_gpu.py).  No other argument needs slack.  Every argument is checked
 * before anything is launched (PP_E_ARG; PP_E_STATE before pp_commit_weights).  The call changes nothing a later pass reads; the
 * first call that asks for statistics allocates their scratch accumulators (synchronous), later calls only enqueue. */
int pp_debug_layer(pp_ctx* ctx, int layer, int nb, const void* in, const void* res, int pre_mode, const float* scale, const float* shift,
                   const int32_t* pmap, const float* feat, void* out, float* out_box, float* out_dir, double* stats, void* stream);

/* pp_debug_layer with the tile-skipping form of a stride-1 layer of level 0 (see pp_set_tile_skip): active u8[nb][H][W] marks the
 * pixels the sparse first convolution would have computed, skip_k = 1..3 is the layer's ordinal among those layers.  The lists are
 * built by the pass's own builder and the layer runs as the listed launch plus the fill.  `in` and `res` must satisfy the rule's
 * precondition (constant per channel outside the layer's non-constant blocks): produce them by running the previous layers.
 * active = NULL and skip_k = 0 is pp_debug_layer.  PP_E_ARG when the path does not serve the layer (tiling, precision, map not a
 * whole number of 16 x 16 tiles, switch off). */
int pp_debug_layer_skip(pp_ctx* ctx, int layer, int nb, const void* in, const void* res, int pre_mode, const float* scale, const float* shift,
                        const int32_t* pmap, const float* feat, void* out, float* out_box, float* out_dir, double* stats,
                        const uint8_t* active, int skip_k, void* stream);

/* Test hook next to pp_debug_layer: the cls-only pass of the deferred head -- the committed cls tiling (pp_head_cls_tiling) on the
 * head's committed weight image -- on caller tensors, nb frames in one launch.  in f32[nb][320][H][W], padded like pp_debug_layer's;
 * pre_mode, scale and shift as there; cls_out f32[nb][A] as the head's cls output.  Every argument is checked before anything is
 * launched (PP_E_ARG); PP_E_STATE before pp_commit_weights and when the committed plan has no deferred head (a 16-bit mode, a head of
 * other than 9 anchors, or the head on a direct tiling).  Writes only cls_out. */
int pp_debug_head_cls(pp_ctx* ctx, int nb, const void* in, int pre_mode, const float* scale, const float* shift, float* cls_out, void* stream);
/* The committed tiling of that pass, "" when the plan has no deferred head.  PP_FORCE_VARIANT pins it like a layer's tiling. */
const char* pp_head_cls_tiling(pp_ctx* ctx);

/* Deferred head (default on).  Post-processing reads the box / dir logits of at most nms_pre_max anchors per class, so a pass of
 * pp_infer_batch / pp_infer_frame computes the cls rows of the head for every pixel and the box / dir logits for the selected
 * candidates only (bit-identical to the full head: same MFMA arithmetic on the same weight image).  The context's full box / dir
 * tensors are then stale; whatever reads them (pp_batch_loss, pp_fetch_frame_tensor kinds 1 and 2) or would overwrite their inputs
 * (pp_backbone, pp_update_head_weights, pp_commit_weights) first runs the full head over the retained concat buffer of that pass, so
 * results never differ -- but a caller that needs the full tensors after EVERY pass (a loss per pass) should switch the mode off and
 * not pay for both heads.  on = 0 / 1; the environment variable PP_HEAD_DEFER=0 (read at pp_create) forces it off.
 * Active means: switched on AND the committed plan is the fp32 mode with the 9-anchor head on a gemm1x1 tiling; every other plan
 * (16-bit modes, other anchor counts, a head on a direct tiling) runs the full head as before.  pp_head_defer_active: 1 / 0. */
int pp_set_head_defer(pp_ctx* ctx, int on);
int pp_head_defer_active(pp_ctx* ctx);

/* Sparse first convolution (default on).  In the fp32 mode a pass of pp_infer_batch / pp_infer_frame computes the first convolution
 * (3x3, stride 2, on the pillar map) only for the output pixels with a pillar among their 3x3 input cells: a per-frame list of these
 * pixels in ascending order, a gather-GEMM over the list, and a scatter into the zero-filled dense map the rest of the network reads.
 * Same values up to the fp32 summation order inside the convolution and its InstanceNorm statistics (~3e-5 on the logits).  A
 * frame's result does not depend on the batch it rides in.  on = 0 / 1; the environment variable PP_SPARSE_CONV1=0 (read at
 * pp_create) forces it off.  The 16-bit modes and the dense-canvas entry points (pp_scatter + pp_backbone) are not affected. */
int pp_set_sparse_conv1(pp_ctx* ctx, int on);

/* Tile skipping (default on).  Behind the sparse first convolution the level-0 map is exactly zero outside the active pixels, so
 * relu(norm(.)) is one constant per channel there and the three stride-1 3x3 layers of level 0 would compute the same 16 x 16 tile
 * hundreds of times per frame.  fp32 passes whose first convolution ran sparse, on the wino6 main tile and a map of whole 16 x 16
 * tiles, compute one such tile per (frame, layer, border class), weight its statistics by the class's count (exact in fp64) and copy
 * it to the others: outputs are bit-identical to the dense launches', the fp64 statistics differ in addition order only (as they do
 * from run to run).  Every other case runs the dense launches.  on = 0 / 1; PP_TILE_SKIP=0 in the environment (read at pp_create)
 * forces it off.  pp_tile_skip_active: did the last pass (or single-layer call) run a listed launch. */
int pp_set_tile_skip(pp_ctx* ctx, int on);
int pp_tile_skip_active(pp_ctx* ctx);

/* ---- training targets and loss (anchor_assigner.py:337-457, loss_generator.py:26-253, metrics.py:14-69) ----
 * Ground truth of nb frames: gt f32[G][7] (x,y,z,l,w,h,r), gt_cls i32[G] 1-based class id in detect_class order,
 * gt_off_h HOST i32[nb+1] (frame f owns rows gt_off_h[f] .. gt_off_h[f+1]-1; non-decreasing, gt_off_h[nb] <= PP_ASSIGN_MAX_GT).
 * 1 <= nb <= cfg.max_batch.  Class ids outside 1 .. num_classes are the caller's error (the Python layer refuses them before any
 * launch; the kernels treat such rows as belonging to no class).  Labels follow the reference bit for bit: per class, IoU of the
 * near BEV boxes in float32, forced anchors (IoU == a box's maximum over inside anchors, every tie), matched / unmatched
 * thresholds of pp_set_assign_thresholds, -1 outside the mask, 0 for every inside anchor of a class without boxes. */
#define PP_ASSIGN_MAX_GT 4096 /* ground-truth rows per call, all frames together */
/* per-frame terms of pp_target_loss / pp_batch_loss: [0] npos = #(label > 0); [1] loc, [2] cls_pos, [3] cls_neg, [4] dir: the
 * reference's per-frame sums, each divided by max(npos, 1) (NormByNumPositives; not yet scaled by the loss weights or 1/B);
 * [5 + 4*i + j]: metric count j (0 tp, 1 tn, 2 fp, 3 fn) at threshold i (0.1, 0.3, 0.5, 0.7) of sigmoid(cls), label != -1 */
#define PP_LOSS_TERMS 21
/* per-class matched / unmatched IoU thresholds (HOST f32[num_classes]; AnchorAssigner reads them from the class table);
 * defaults 0.6 / 0.45.  Host-side only (no device work, no allocation).  Labels follow the reference's order: forced -> 1, else
 * max < unmatched -> 0, else max >= matched -> 1, else -1 (so a matched threshold below the unmatched one behaves as there). */
int pp_set_assign_thresholds(pp_ctx* ctx, const float* matched_h, const float* unmatched_h);
/* replaces AnchorAssigner.assign (anchor_assigner.py:337-457) for nb frames at once.  mask u8[nb][A].  Outputs labels i32[nb][A],
 * bbox_targets f32[nb][A][7], outside_w f32[nb][A], dir_targets i32[nb][A], all fully written. */
int pp_assign_targets(pp_ctx* ctx, const uint8_t* mask, const float* gt, const int32_t* gt_cls, const int32_t* gt_off_h, int nb,
                      int32_t* labels, float* bbox_targets, float* outside_w, int32_t* dir_targets, void* stream);
/* replaces LossGenerator.generate + Metric.update's counts, per frame: cls f32[nb][A], box f32[nb][A][7], dir f32[nb][A][2] and the
 * targets of pp_assign_targets -> terms f64[nb][PP_LOSS_TERMS].  Deterministic (no float atomics): two runs are bit-identical.
 * Counts only (Metric.update): box, dir, bbox_targets and dir_targets all NULL -> npos, cls_pos, cls_neg and the 16 counts as
 * above, loc and dir 0.  The assignment / loss workspace is allocated on the first call of the three functions below. */
int pp_target_loss(pp_ctx* ctx, const float* cls, const float* box, const float* dir, const int32_t* labels,
                   const float* bbox_targets, const int32_t* dir_targets, int nb, double* terms, void* stream);
/* fused: assignment + loss for frames 0 .. nb-1 of the LAST pp_infer_batch / pp_infer_frame pass, read from the context's own
 * anchor masks and head outputs; no [A,7] target tensor is materialised.  Same terms, bit for bit, as pp_assign_targets on the
 * fetched masks followed by pp_target_loss on the fetched logits.  nb must not exceed the frames of that pass (PP_E_ARG);
 * PP_E_STATE before the first pass. */
int pp_batch_loss(pp_ctx* ctx, const float* gt, const int32_t* gt_cls, const int32_t* gt_off_h, int nb, double* terms, void* stream);

/* ---- loss gradient and head backward (train.hip): head-only fine-tuning, the backbone is frozen ----
 * Gradients are fp32 whatever pp_set_precision says.  Deterministic: no float atomics, two runs on the same inputs are bit-identical.
 *
 * pp_target_loss_grad: gradient of the `loss` value of LossGenerator.generate (loss_generator.py:26-72; loc 0.25, cls 1.0, dir 0.2,
 * NormByNumPositives) with respect to the head outputs.  Inputs as pp_target_loss (all required); dcls f32[nb][A], dbox f32[nb][A][7],
 * ddir f32[nb][A][2], fully written.  The result is scaled by grad_scale / batch_div: grad_scale is the upstream dL/dloss (1 for
 * loss.backward()), batch_div the batch size of the loss's 1/B mean -- nb, or the whole batch when the caller passes it in chunks of
 * at most max_batch frames (batch_div >= nb).  Per anchor, npos = max(#(label > 0) of the frame, 1), counted on the device:
 * sigmoid focal derivative (gamma 2, alpha 0.25; target label > 0) / npos where label >= 0; smooth-L1 (sigma 3) derivative with the
 * sin-difference angle code / npos and softmax - onehot / npos where label > 0.  Rows with label == -1 are exact zeros in all three,
 * rows with label <= 0 in dbox and ddir.  dir and ddir must be 8-byte aligned; 16-byte aligned box tensors and A % 4 == 0 take the
 * 16-byte path. */
int pp_target_loss_grad(pp_ctx* ctx, const float* cls, const float* box, const float* dir, const int32_t* labels,
                        const float* bbox_targets, const int32_t* dir_targets, int nb, int batch_div, float grad_scale, float* dcls,
                        float* dbox, float* ddir, void* stream);
/* backward of SharedHead.forward (pointpillars8_shared.py:323-343) for nb frames: rpn_out f32[nb][320][H][W] (what pp_head consumed),
 * dcls / dbox / ddir in the head's OUTPUT layout (anchor type, x, y; codes innermost) -> dw_cls f32[na][320], dw_box f32[7 na][320],
 * dw_dir f32[2 na][320], db_cls f32[na], db_box f32[7 na], db_dir f32[2 na] in state_dict order (channel a * 7 + k of conv_box,
 * a * 2 + k of conv_dir), summed over the nb frames, and dx f32[nb][320][H][W] = dL/d(rpn_out) (NULL: skipped).  fp32-input MFMA, fp32
 * accumulation.  Each workgroup owns a pixel range of one frame; its [10 na][320] partial is summed with the others in a fixed order,
 * so the result depends on nb (the ranges do) only within fp32 summation error.  dx uses the committed head weights, or those of the
 * last pp_update_head_weights.  1 .. 24 anchors per location (24 = PP_MAX_CLASSES x 1 size x 2 rotations; PP_E_ARG above): up to 9 the
 * 96-row kernels, from 10 on the row-blocked dW and channel-blocked dX kernels over 10 na rows rounded up to 16, same contract.
 * PP_E_STATE before pp_commit_weights. */
int pp_head_backward(pp_ctx* ctx, const float* rpn_out, const float* dcls, const float* dbox, const float* ddir, int nb, float* dw_cls,
                     float* dw_box, float* dw_dir, float* db_cls, float* db_box, float* db_dir, float* dx, void* stream);
/* After an optimizer step: six DEVICE tensors in state_dict layout (heads.conv_{cls,box,dir}.{weight,bias}: [na][320], [na], [7 na][320],
 * [7 na], [2 na][320], [2 na]) -> the head's packed weight image and biases of the committed launch plan, rewritten in place on
 * `stream` (no host copy, no re-tuning).  pp_head, pp_infer_frame and pp_infer_batch read that image, so all three see the new weights.
 * The first call after a commit reads the image's layout back once (synchronous).  The host copies of pp_load_weights are NOT changed:
 * a later pp_commit_weights packs those again.  fp32 mode only: in the 16-bit modes (pp_effective_precision != 0) the packed image
 * holds rounded / split operands and this returns PP_E_ARG.  PP_E_ARG before the first commit. */
int pp_update_head_weights(pp_ctx* ctx, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box, const float* w_dir,
                           const float* b_dir, void* stream);

/* ---- neck backward (neck_train.hip): the three upsampling branches of RPN train with the head ----
 * Each branch is ConvTranspose2d(k = s, no bias) -> InstanceNorm2d(eps 1e-3, no affine) -> ReLU (pointpillars8_shared.py:139-171) on a
 * block output; branch b (0..2) has Cin = 64 << b, Cup = 64 | 128 | 128, s = 1 << b, reads x f32[Cin][H >> b][W >> b] and fills channels
 * [0,64) | [64,192) | [192,320) of rpn_out.  fp32, InstanceNorm backbone only.  Deterministic: no atomics, two runs are bit-identical.
 *
 * pp_backbone_taps: exactly pp_backbone (same rpn_out, bit for bit), and also copies the three block outputs -- the tensors the
 * upsamplers consume, raw residual sums -- to caller memory: x1 f32[64][H][W], x2 f32[128][H/2][W/2], x3 f32[256][H/4][W/4].  fp32 mode
 * only: in the 16-bit modes the level buffers may hold fp16 and this returns PP_E_ARG. */
int pp_backbone_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, void* stream);
/* Backward of branch `branch` for nb <= max_batch frames.  Stateless: the result depends on the arguments only, not on the context's
 * last pass or committed weights.  x f32[nb][Cin][h][w] (the block output), w DEVICE f32[Cin][Cup][s][s] (state_dict layout, 16-byte
 * aligned), y / dy f32[nb][320][H][W] = the full rpn_out and dL/d(rpn_out), of which the branch's channel slice is read ->
 * dw f32[Cin][Cup][s][s] summed over the frames, fully written, and dx f32[nb][Cin][h][w] (NULL: skipped).  Per frame and output
 * channel, N = H W: Z = ConvT(x, w) is recomputed, mean and rstd = 1 / sqrt(biased var + 1e-3) come from fp64 sums over Z,
 * Gr = dy [y > 0] (the mask is the given y, never a recomputed sign), dZ = rstd (Gr - sum(Gr) / N - xhat sum(Gr xhat) / N),
 * dw[ci][co][ky][kx] = sum_{frames, q} x[ci, q] dZ[co, s q + (ky, kx)], dx[ci, q] = sum_{co, ky, kx} w[ci][co][ky][kx] dZ[co, s q + (ky, kx)].
 * The three products are fp32-input MFMA GEMMs; dZ is materialised once in a workspace (allocated on first use, at most 256 MB: larger
 * batches run in frame chunks).  dw is tiled over workgroups and its K range (frames x pixels) split into a fixed number of ranges
 * whose partials are summed in index order, so dw depends on nb within fp32 summation error; a frame's dx does not depend on nb at all.
 * PP_E_ARG for a null pointer, branch outside 0..2, nb outside 1..max_batch, a misaligned w and the BatchNorm backbone. */
int pp_neck_backward(pp_ctx* ctx, int branch, const float* x, const float* w, const float* y, const float* dy, int nb, float* dw, float* dx,
                     void* stream);
/* pp_neck_backward with 16-bit GEMM operands (neck_train16.hip): mixed-precision training, the modes of pp_unit_backward_mp with the same
 * numbering: 0 fp32 (exactly pp_neck_backward, bit for bit), 1 "bf16x3" (operands split hi + lo, a product is hi hi + hi lo + lo hi),
 * 2 "bf16" (operands rounded once), both on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.  The recomputed forward Z, the statistics,
 * the mask and dZ are the fp32 kernels in every mode; only the operands of dw = sum x dZ and dx = sum w dZ are 16-bit.  x and dZ are read
 * as fp32 and rounded or split in registers (no 16-bit image is kept; w is packed once per call), so the workspace and the frame chunks are
 * pp_neck_backward's and every branch runs in the mode asked for.  The dx product keeps the blocked sum (64 rows from zero, block sums
 * added in row order).  Stateless and deterministic as pp_neck_backward: no atomics, two runs are bit-identical, a frame's dx does not
 * depend on nb, dw does not depend on whether dx is asked for and depends on nb through the fixed K ranges (32-pixel chunks) only.
 * PP_E_ARG as pp_neck_backward, and for a mode outside 0..2. */
int pp_neck_backward_mp(pp_ctx* ctx, int mode, int branch, const float* x, const float* w, const float* y, const float* dy, int nb, float* dw,
                        float* dx /* may be NULL */, void* stream);
/* The mode pp_neck_backward_mp really runs for this branch: `mode`.  Launches nothing.  An error is negative: -PP_E_ARG for a null context,
 * a mode outside 0..2, a branch outside 0..2, a BEV grid that is no multiple of 8 and the BatchNorm backbone. */
int pp_neck_backward_path(pp_ctx* ctx, int mode, int branch);
/* After an optimizer step: three DEVICE tensors in state_dict layout (rpn.deconv{1,2,3}.0.weight: [64][64][1][1], [128][128][2][2],
 * [256][128][4][4]) -> the packed weight images of the three upsamplers of the committed launch plan, rewritten in place on `stream` (no
 * host copy, no re-tuning).  pp_backbone, pp_backbone_taps, pp_infer_frame and pp_infer_batch read those images, so all see the new
 * weights.  The first call after a commit reads the images' layout back once (synchronous).  The host copies of pp_load_weights are
 * NOT changed: a later pp_commit_weights packs those again.  The call touches neither the concat buffer nor the head image, so a
 * deferred head pass that is still pending keeps its inputs and needs nothing here.  fp32 mode only: PP_E_ARG when
 * pp_effective_precision != 0, and before the first commit. */
int pp_update_neck_weights(pp_ctx* ctx, const float* w1, const float* w2, const float* w3, void* stream);

/* ---- Resnet unit backward (block_train.hip): the primitive of every Resnet2 module's backward ----
 * The backbone's stride-1 layers are all one unit, InstanceNorm2d(eps 1e-3, no affine) -> ReLU -> Conv2d(C -> C, 3 x 3, pad 1, no bias)
 * (pointpillars8_shared.py:418-431).  Per frame and input channel, N = h w: mean and rstd = 1 / sqrt(biased var + 1e-3) come from fp64
 * sums over u, xhat = (u - mean) rstd, a = max(xhat, 0), z = conv(a, w).  fp32 whatever pp_set_precision says, InstanceNorm backbone
 * only.  Deterministic: no atomics, two runs are bit-identical.
 *
 * pp_unit_backward: backward of one unit for nb <= max_batch frames.  Stateless: the result depends on the arguments only, not on the
 * context's last pass or committed weights.  C is 64, 128 or 256; h, w >= 1 with h w >= 2.  u (the unit's input), dy (= dL/dz), dskip
 * and du are f32[nb][C][h][w], w DEVICE f32[C][C][3][3] (state_dict layout, 16-byte aligned) ->
 * dw[co][ci][ky][kx] = sum_{frames, p} dy[co, p] a[ci, py + ky - 1, px + kx - 1], f32[C][C][3][3] summed over the frames, fully written,
 * and du = rstd (Gr - sum(Gr) / N - xhat sum(Gr xhat) / N) + dskip with da[ci, q] = sum_{co, ky, kx} w[co][ci][ky][kx] dy[co, qy - ky + 1,
 * qx - kx + 1] and Gr = da [a > 0]; the mask is that of the a this call materialises, so dw and du see the same activation.  dskip may
 * be NULL (nothing is added; otherwise it is one fp32 add behind the rounded norm backward: the gradient of a residual connection
 * around the unit).  du NULL: the dgrad product and the norm backward are not run.  Both products are fp32-input MFMA GEMMs over
 * zero-haloed copies of a and dy in a workspace (allocated on first use, at most 1 GB: larger batches run in frame chunks; a map
 * whose single frame takes more than 256 MB of it is PP_E_ARG).  dw is tiled over workgroups and its K range (frames x positions) split into a fixed
 * number of ranges whose partials are summed in index order in double, so dw depends on nb within fp32 summation error; a frame's du
 * does not depend on nb at all.  The dgrad sums its K = 9 C terms in blocks of 64 from zero and adds the block sums in a fixed order.
 * The workspace belongs to the context, so "stateless" is about values, not about concurrency: calls on one context must be issued in
 * order on one stream (or ordered by events), like every other call that takes a pp_ctx.  A call that has to enlarge the workspace
 * waits for the whole device before it frees the old one.
 * PP_E_ARG for a null pointer, C outside the three, sizes out of range, nb outside 1..max_batch, a misaligned w and the BatchNorm
 * backbone. */
int pp_unit_backward(pp_ctx* ctx, int C, int h, int w, const float* u, const float* wgt, const float* dy, const float* dskip /* may be NULL */,
                     int nb, float* dw, float* du /* NULL: skipped */, void* stream);
/* pp_unit_backward with 16-bit GEMM operands: mixed-precision training.  mode follows the numbering of pp_set_precision: 0 fp32 (exactly
 * pp_unit_backward, bit for bit), 1 "bf16x3" (every operand of the two products split as x = hi + lo, hi = bf16(x), lo = bf16(x - hi),
 * round to nearest even; a product is hi hi + hi lo + lo hi, issued in that order into one fp32 accumulator: relative error 3 x 2^-16
 * per product), 2 "bf16" (every operand rounded once: 2^-7 per product).  Both run on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
 * Only the operand streams of the wgrad and dgrad products are 16-bit: u, w, dy, dskip, dw and du are fp32 as above, and so are the
 * statistics (fp64 sums), the ReLU mask (that of the fp32 xhat: rounding a positive fp32 to bf16 never gives 0), the norm backward, the
 * reduction of the dw partials in double and the dskip add.  bf16 has fp32's exponent range: no loss scaling.  Stateless as
 * pp_unit_backward: neither pp_set_precision nor the committed plan is read.  Deterministic in the same sense: no atomics, two runs
 * are bit-identical, a frame's du does not depend on nb, dw depends on nb through the fixed K ranges only.  The 16-bit images (a, dz,
 * and dz once more with the channel innermost; a hi and a lo image of each under bf16x3) live in the same workspace under the same
 * rules: a chunk of frames takes at most 1 GB, so a batch may run in more chunks than under fp32; a shape whose single frame would
 * take more than 256 MB runs the fp32 kernels instead (pp_unit_backward_path tells).  The dgrad keeps the blocked sum: 64 k-terms from
 * zero, block sums added in (tap, co) order.
 * PP_E_ARG as pp_unit_backward, and for a mode outside 0..2. */
int pp_unit_backward_mp(pp_ctx* ctx, int mode, int C, int h, int w, const float* u, const float* wgt, const float* dy,
                        const float* dskip /* may be NULL */, int nb, float* dw, float* du /* NULL: skipped */, void* stream);
/* The mode pp_unit_backward_mp really runs for this shape: `mode`, or 0 where no 16-bit tiling takes the shape.  Launches nothing.
 * An error is negative: -PP_E_ARG for a null context, a mode outside 0..2, C outside the three, h or w out of range and the BatchNorm
 * backbone. */
int pp_unit_backward_path(pp_ctx* ctx, int mode, int C, int h, int w);
/* pp_backbone_taps plus the inputs of the five units of block 3 (the deepest block: h -> r3 = h + U_b(U_a(h)), r4 = r3 + U_d(U_c(r3)),
 * x3 = r4 + U_e(r4), weights rpn.block3.{3,3,4,4,5}.conv_block.{2,5,2,5,2}.weight): units f32[5][256][H/4][W/4] = h, m3 = U_a(h), r3,
 * m4 = U_c(r3), r4, each copied out behind the launch that produces it (the level buffers are reused inside a block).  rpn_out, x1, x2
 * and x3 match pp_backbone bit for bit.  fp32 mode only, as pp_backbone_taps. */
int pp_backbone_block_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* units, void* stream);
/* After an optimizer step: the five DEVICE tensors f32[256][256][3][3] of block 3 in unit order a..e (state_dict layout) -> the packed
 * weight images of those five layers of the committed launch plan, rewritten in place on `stream` (no host copy, no re-tuning).  block
 * must be 2 (block 3) and n 5: PP_E_ARG for the other blocks, which pp_update_rpn_weights rewrites with all the others.
 * The Winograd tilings' images hold U = G g G^T, which a device kernel evaluates from g in fp64 in the host packer's own expression
 * order and rounds once, so the images equal those of a fresh commit of the same values bit for bit; the direct tilings' images are
 * permuted copies.  The strip tilings share the main image.  pp_backbone*, pp_infer_frame and pp_infer_batch all see the new weights.
 * The first call after a commit reads the images' layout back once (synchronous).  The host copies of pp_load_weights are NOT changed.
 * fp32 mode only: PP_E_ARG when pp_effective_precision != 0, and before the first commit. */
int pp_update_block_weights(pp_ctx* ctx, int block, const float* const* w, int n, void* stream);

/* ---- strided stage backward (down_train.hip): the head of every backbone block ----
 * Conv2d(Cin -> Cout, 3 x 3, stride 2, pad 1, no bias) -> InstanceNorm2d(eps 1e-3, no affine) -> ReLU (pointpillars8_shared.py:143-161).
 * The stage input x f32[nb][Cin][Hin][Win] is raw (no norm in front of this conv); with ho = (Hin + 1) / 2, wo = (Win + 1) / 2,
 * z[co, oy, ox] = sum w[co][ci][ky][kx] x[ci, 2 oy + ky - 1, 2 ox + kx - 1] (zero padding), and per plane of z, N = ho wo: mean and
 * rstd = 1 / sqrt(biased var + 1e-3) from fp64 sums, rounded to fp32 as the forward rounds them, xhat = (z - mean) rstd, h = max(xhat, 0).
 *
 * pp_down_backward: backward of one stage for nb <= max_batch frames, from the conv output z and dy = dL/dh, both f32[nb][Cout][ho][wo].
 * Stateless, fp32 whatever pp_set_precision says, InstanceNorm backbone only.  (cin, cout) is (64, 64), (64, 128) or (128, 256);
 * hin, win >= 1 with ho wo >= 2.  w DEVICE f32[Cout][Cin][3][3] (state_dict layout, 16-byte aligned) ->
 * dz = rstd (Gr - sum(Gr) / N - xhat sum(Gr xhat) / N) with Gr = dy [xhat > 0] (sums in fp64),
 * dw[co][ci][ky][kx] = sum_{frames, oy, ox} dz[co, oy, ox] x[ci, 2 oy + ky - 1, 2 ox + kx - 1], f32[Cout][Cin][3][3], fully written, and
 * dx[ci, iy, ix] = sum_{co, ky, kx} w[co][ci][ky][kx] dz[co, (iy + 1 - ky) / 2, (ix + 1 - kx) / 2] over the taps whose quotients are whole
 * and in range, f32[nb][Cin][Hin][Win], fully written.  dx NULL: the dgrad product is not run, and dw is the same bits.  Both products
 * are fp32-input MFMA GEMMs over zero-haloed half-resolution copies of dz and of the four row / column parity planes of x in a workspace
 * of its own (allocated on first use, at most 1 GB: larger batches run in frame chunks; a map whose single frame takes more than 256 MB
 * of it is PP_E_ARG).  Deterministic: no atomics; dw's K range (frames x positions) is split by the shapes alone and the partials are summed in
 * index order in double, so dw depends on nb within fp32 summation error; a frame's dx does not depend on nb at all.  The dgrad sums its
 * K = Cout x {1, 2, 2, 4} taps per output parity class in blocks of 64 from zero and adds the block sums in a fixed order.  Calls on one
 * context must be issued in order on one stream, as for pp_unit_backward.
 * PP_E_ARG for a null pointer, a channel pair outside the three, sizes out of range, nb outside 1..max_batch, a misaligned w and the
 * BatchNorm backbone. */
int pp_down_backward(pp_ctx* ctx, int cin, int cout, int hin, int win, const float* x, const float* w, const float* z, const float* dy, int nb,
                     float* dw, float* dx /* NULL: skipped */, void* stream);
/* pp_down_backward with 16-bit GEMM operands (down_train16.hip): mixed-precision training, the modes of pp_unit_backward_mp with the same
 * numbering: 0 fp32 (exactly pp_down_backward, bit for bit), 1 "bf16x3", 2 "bf16", both on v_mfma_f32_16x16x32_bf16 with fp32 accumulation.
 * The parity planes of x, the plane statistics (fp64 sums), the mask xhat > 0, the norm backward that writes dz and the reduction of the
 * dw partials in double are the fp32 kernels in every mode; only the operands of the wgrad and dgrad products are 16-bit.  The planes stay
 * fp32 and are rounded or split in registers as they are loaded (no 16-bit image is kept; w is packed once per call), so the workspace,
 * its budgets and the frame chunks are pp_down_backward's and every shape it takes runs in the mode asked for.  The dgrad keeps the
 * blocked sum (64 k-terms from zero, block sums added in (tap, co) order).  Stateless and deterministic as pp_down_backward: no atomics,
 * two runs are bit-identical, a frame's dx does not depend on nb, dw does not depend on whether dx is asked for and depends on nb through
 * the fixed K ranges (32-position chunks) only.
 * PP_E_ARG as pp_down_backward, and for a mode outside 0..2. */
int pp_down_backward_mp(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win, const float* x, const float* w, const float* z,
                        const float* dy, int nb, float* dw, float* dx /* may be NULL */, void* stream);
/* The mode pp_down_backward_mp really runs for this shape: `mode`.  Launches nothing.  An error is negative: -PP_E_ARG for a null context,
 * a mode outside 0..2, a channel pair outside the three, sizes out of range (a frame past the 256 MB budget included) and the BatchNorm
 * backbone. */
int pp_down_backward_path(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win);
/* pp_backbone_block_taps plus z3 f32[256][H/4][W/4], the raw (pre-norm) output of block 3's strided convolution, copied out behind
 * that launch (units[0] = relu(norm(z3)); the first unit reuses the buffer).  fp32 mode only, as pp_backbone_taps. */
int pp_backbone_stage_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* units, float* z3,
                           void* stream);
/* After an optimizer step: the DEVICE tensor f32[256][128][3][3] rpn.block3.0.weight (state_dict layout) -> the packed image of the
 * strided convolution of `level` of the committed launch plan, rewritten in place on `stream`; the image equals that of a fresh commit
 * of the same values bit for bit (a direct tiling: a permuted copy).  level must be 2: PP_E_ARG for levels 0 and 1, which are
 * rewritten by pp_update_rpn_weights (level 0 also carries the sparse first-conv packing).  The first call after a commit reads the image's layout back once
 * (synchronous).  The host copies of pp_load_weights are NOT changed.  fp32 mode only: PP_E_ARG when pp_effective_precision != 0, and
 * before the first commit. */
int pp_update_down_weight(pp_ctx* ctx, int level, const float* w, void* stream);

/* ---- training the whole RPN: taps and the weight update for all three levels (conv.hip, block_train.hip, sparse_conv1.hip) ----
 * pp_backbone_train_taps: pp_backbone_stage_taps for every level b = 0, 1, 2 (C_b = 64, 128, 256 on the (H >> b) x (W >> b) map).
 * units[b] f32[n_b][C_b][H>>b][W>>b], n_b = 3, 5, 5: the inputs of the block's unit convolutions in unit order (level 0: h, m = U_a(h),
 * r = h + U_b(m); x1 = r + U_c(r); levels 1 and 2 as pp_backbone_block_taps describes block 3).  z[b] f32[C_b][H>>b][W>>b]: the raw
 * (pre-norm) output of the level's strided convolution, units[b][0] = relu(norm(z[b])).  units and z are HOST arrays of three device
 * pointers.  Every tensor leaves through a copy hook behind the launch that produces it; the hooks are armed for this pass only, and a
 * pass with no hook armed is bit for bit what it was.  rpn_out, x1, x2 and x3 match pp_backbone bit for bit.  One frame per call; fp32
 * mode only, as pp_backbone_taps. */
int pp_backbone_train_taps(pp_ctx* ctx, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3, float* const* units,
                           float* const* z, void* stream);
/* After an optimizer step: the sixteen DEVICE tensors of the RPN's 3 x 3 convolutions in execution (= state_dict) order -- per level
 * rpn.block<b+1>.0.weight f32[C_b][C_{b-1}][3][3], then the level's 3 | 5 | 5 unit convolutions f32[C_b][C_b][3][3] -- -> the packed
 * images of those layers of the committed launch plan, rewritten in place on `stream`, whatever tiling family each layer runs (as
 * pp_update_block_weights does for block 3).  Level 0's strided weight also rewrites the image of the sparse first convolution, in the
 * K order of the committed dense tiling, so the fused inference path sees the same rpn.block1.0.weight; tile skipping holds nothing
 * derived from the weights and stays active.  Every image equals that of a fresh commit of the same values bit for bit.  The first call
 * after a commit reads the images' layouts back once (synchronous); later calls do not synchronise.  The host copies of pp_load_weights
 * are NOT changed.  fp32 mode only: PP_E_ARG when pp_effective_precision != 0, and before the first commit. */
int pp_update_rpn_weights(pp_ctx* ctx, const float* const* w /* 16 */, void* stream);

/* ---- the training forward on 16-bit MFMA operands: the _mp forms of the taps and of the three weight updates (conv_run.hip,
 *      image16.hip, block_train.hip, neck_train.hip, train.hip) ----
 * mode is 1 (bf16x3), 2 (bf16) or 3 (fp16), the numbering of pp_set_precision.  Each entry returns PP_E_ARG unless
 * pp_effective_precision(ctx) == mode, so a plan that keeps fp16 tensors (4, fp16s) is refused throughout: the taps are fp32 tensors.
 * The fp32 entries above keep refusing every plan but an fp32 one.
 * pp_backbone_train_taps_mp: pp_backbone_train_taps on that plan.  In modes 1 - 3 the level buffers are fp32 and the copy hooks sit
 * behind the launches whatever tiling runs, so the taps are the fp32 activations of the 16-bit forward (the norms and ReLUs are fp32
 * in every mode); rpn_out, x1, x2, x3 match pp_backbone bit for bit, and a pass with no hook armed is bit for bit what it was.
 * The three updates rewrite the committed images in place on `stream` from fp32 DEVICE tensors, as their fp32 forms do.  A 16-bit image
 * holds no transform: it is a permutation of the weight elements, each rounded to nearest even to bf16 (modes 1, 2) or fp16 (mode 3),
 * with a second image of the residuals bf16(x - hi) where the packer writes one; the element map -- which element, which part, or
 * padding -- is read back from the packers once per commit (three passes of base-128 digits; synchronous, on the first update after a
 * commit), and every image equals that of a fresh commit of the same values in that mode bit for bit.  A layer whose shape no 16-bit
 * tiling takes keeps its fp32 tiling in a 16-bit plan (pp_layer_tilings says so) and its fp32 writer.
 * pp_update_rpn_weights_mp: the sixteen convolutions; the sparse first convolution is fp32 only and keeps no image these modes read
 * (a return to fp32 commits again).  pp_update_neck_weights_mp: the three upsamplers.  pp_update_head_weights_mp: the head; the bias
 * stays fp32, in natural order and, where the plan keeps that copy, in head_tile_row order; the natural-order copy of the weights that
 * pp_head_backward's dX product reads is refreshed too.  The host copies of pp_load_weights are NOT changed. */
int pp_backbone_train_taps_mp(pp_ctx* ctx, int mode, const float* canvas, float* rpn_out, float* x1, float* x2, float* x3,
                              float* const* units, float* const* z, void* stream);
int pp_update_rpn_weights_mp(pp_ctx* ctx, int mode, const float* const* w /* 16 */, void* stream);
int pp_update_neck_weights_mp(pp_ctx* ctx, int mode, const float* w1, const float* w2, const float* w3, void* stream);
int pp_update_head_weights_mp(pp_ctx* ctx, int mode, const float* w_cls, const float* b_cls, const float* w_box, const float* b_box,
                              const float* w_dir, const float* b_dir, void* stream);
/* Test hook: the in-place writer of the 16-bit images on caller memory.  The image of layer `layer` (0 .. 19 of pp_layer_tilings) of the
 * committed plan is written into dst (cap bytes) from the fp32 DEVICE tensor w0 (a convolution's or an upsampler's state_dict weight;
 * the head: w0 | w1 | w2 = cls | box | dir, NULL otherwise) on `stream`; *bytes gets the image's size, and dst = NULL only queries it.
 * Writes exactly *bytes bytes of dst and nothing else; reads the plan and its cached element map.  PP_E_ARG when the layer keeps an fp32
 * image in the committed plan; PP_E_STATE before pp_commit_weights. */
int pp_debug_image16(pp_ctx* ctx, int layer, const float* w0, const float* w1, const float* w2, void* dst, size_t cap, size_t* bytes,
                     void* stream);

/* ---- fine-tuning the BatchNorm backbone with frozen statistics (block_train.hip, down_train.hip, neck_train.hip, conv_plan.hip) ----
 * Every BatchNorm2d(eps 1e-3) of the RPN in eval mode is a per-channel affine, norm(v)_c = scale_c v + shift_c with
 * scale = gamma / sqrt(running_var + 1e-3), shift = beta - running_mean scale: the fold of pp_commit_weights, which the forward applies as
 * max(fma(v, scale_c, shift_c), 0) in the prologue of the consuming layer.  The three primitives below are the siblings of
 * pp_unit_backward, pp_down_backward and pp_neck_backward for that norm: the same layers, arguments, workspaces, frame chunks, MFMA
 * products, K ranges and dw reduction, without the statistics passes.  Each takes DEVICE scale, shift f32[C] -- the folded values the
 * forward used -- and returns, beside dw and du / dx, the two per-channel sums of the norm's backward as DEVICE doubles,
 * dscale_c = sum_{frames, positions} g v and dshift_c = sum g (g: the gradient behind the ReLU, v: the norm's input), f64[C], both
 * NULL: not written.  They are left in fp64 because dgamma = (dscale - running_mean dshift) / sqrt(running_var + 1e-3) is a difference that
 * cancels (pp_bn_affine_grad).  Stateless: the result depends on the arguments only, and a context of either norm kind takes them.  fp32,
 * no atomics, two runs are bit-identical; per-segment partial sums are added in index order, frames in frame order.  A frame's du / dx
 * does not depend on the batch it rides in nor on the frame chunks; dw depends on nb through the fixed K ranges only.
 * PP_E_ARG as the siblings (null pointer, sizes, nb outside 1..max_batch, misaligned w), for dscale without dshift or the reverse, and
 * for sums that are not 8-byte aligned.
 *
 * pp_unit_backward_affine: the unit scale/shift -> ReLU -> Conv2d(C -> C, 3 x 3, pad 1).  a = max(fma(u, scale_c, shift_c), 0),
 * dw = sum dy (*) a, da = dgrad(dy, w) with the blocked sum, g = da [a > 0], du = scale_c g (+ dskip: one fp32 add), dscale_c = sum g u,
 * dshift_c = sum g.  du NULL: the dgrad is not run, and dscale / dshift must be NULL too (they are sums over it).
 * pp_down_backward_affine: the stage Conv2d(3 x 3, stride 2) -> scale/shift -> ReLU.  g = dy [fma(z, scale_c, shift_c) > 0], dz = scale_c g,
 * then the wgrad / dgrad of pp_down_backward over dz and the parity planes of x; dscale_c = sum g z, dshift_c = sum g.
 * pp_neck_backward_affine: the branch ConvTranspose2d(k = s) -> scale/shift -> ReLU.  Z is recomputed, the mask is the given y > 0,
 * dZ = scale_c g, dscale_c = sum g Z, dshift_c = sum g; scale / shift are those of the branch's Cup channels; shift is not read. */
int pp_unit_backward_affine(pp_ctx* ctx, int C, int h, int w, const float* u, const float* wgt, const float* scale, const float* shift,
                            const float* dy, const float* dskip /* may be NULL */, int nb, float* dw, float* du /* NULL: skipped */,
                            double* dscale /* may be NULL */, double* dshift /* may be NULL */, void* stream);
int pp_down_backward_affine(pp_ctx* ctx, int cin, int cout, int hin, int win, const float* x, const float* w, const float* z, const float* scale,
                            const float* shift, const float* dy, int nb, float* dw, float* dx /* NULL: skipped */, double* dscale /* may be NULL */,
                            double* dshift /* may be NULL */, void* stream);
int pp_neck_backward_affine(pp_ctx* ctx, int branch, const float* x, const float* w, const float* scale, const float* shift, const float* y,
                            const float* dy, int nb, float* dw, float* dx /* NULL: skipped */, double* dscale /* may be NULL */,
                            double* dshift /* may be NULL */, void* stream);
/* The fold of one BatchNorm2d layer on the device: DEVICE gamma, beta, running_mean, running_var f32[C], C <= 256 -> scale, shift f32[C] by
 * the fp64 expression of pp_commit_weights, each value rounded once.  Stateless. */
int pp_bn_fold(pp_ctx* ctx, int C, const float* gamma, const float* beta, const float* running_mean, const float* running_var, float* scale,
               float* shift, void* stream);
/* The sums of an affine primitive -> the gradients of the BatchNorm2d layer's weight and bias: dgamma = r (dscale - running_mean dshift),
 * dbeta = dshift, r = 1 / sqrt(running_var + 1e-3), evaluated in fp64 and rounded once.  Stateless. */
int pp_bn_affine_grad(pp_ctx* ctx, int C, const double* dscale, const double* dshift, const float* running_mean, const float* running_var,
                      float* dgamma, float* dbeta, void* stream);
/* After an optimizer step: the nineteen BatchNorm2d layers of the RPN in state_dict order (per block its strided convolution's norm, the
 * norms of its units, its upsampler's norm), four DEVICE tensors each -- bn[4 i + {0, 1, 2, 3}] = weight, bias, running_mean, running_var
 * of layer i -- -> the folded (scale, shift) arrays of the committed plan, rewritten in place on `stream` by pp_bn_fold's kernel: bit for
 * bit what a fresh pp_commit_weights of the same values holds.  Every pass reads those arrays when it runs (pp_backbone*, pp_infer_frame,
 * pp_infer_batch, with the sparse first convolution and tile skipping: nothing derived from them is kept between passes), so all see the
 * new values.  The host copies of pp_load_weights are NOT changed.  PP_E_STATE before the first commit, PP_E_ARG on an InstanceNorm
 * context and for a null or misaligned pointer. */
int pp_update_bn_fold(pp_ctx* ctx, const float* const* bn /* 76 */, void* stream);

/* ---- training the BatchNorm backbone with batch statistics (conv_run.hip, block_train.hip, down_train.hip, neck_train.hip) ----
 * In train mode a BatchNorm2d(eps 1e-3) normalises with the statistics of the batch: per channel, over N = nb h w elements of all frames,
 * mean = s / N and the biased var = max(q / N - mean^2, 0), each rounded once to fp32; the layer is then the affine that pp_bn_fold gives for
 * (gamma, beta, mean, var).
 *
 * pp_backbone_train_taps_bn: the lock-step training forward, BatchNorm contexts in fp32 mode only.  Canvases f32[nb][64][gx][gy], 1 <= nb <=
 * max_batch, run the dense backbone (no sparse first convolution, no tile skipping) layer by layer over all frames; behind each of the
 * nineteen norm sites the per-frame fp64 accumulators of the producer's epilogue are pooled in frame order and folded, and the consumers
 * read that fold.  The arrays belong to the pass: the committed fold of the running statistics (pp_commit_weights, pp_update_bn_fold) is
 * not touched, and inference between two such passes sees the running statistics.  gamma_beta: 38 DEVICE pointers, [2 i] = weight and
 * [2 i + 1] = bias of layer i in pp_update_bn_fold's layer order.  Outputs, all caller memory: rpn_out f32[nb][320][H][W] (normalised,
 * ReLU); x1, x2, x3 f32[nb][C_b][H >> b][W >> b]; units[b] f32[n_b][nb][C_b][H >> b][W >> b] (n_b = 3, 5, 5: the frames of a unit
 * input together, at nb = 1 the layout of pp_backbone_train_taps) and z[b] f32[nb][C_b][H >> b][W >> b], where either array or any entry may be NULL (a tap nobody needs); mean,
 * var, scale, shift f32[19][256], row i filled up to layer i's channels.  PP_E_STATE before the first commit, PP_E_ARG on an InstanceNorm
 * context, in a 16-bit mode, for nb outside 1..max_batch and for a null pointer.
 *
 * pp_unit_backward_bn, pp_down_backward_bn, pp_neck_backward_bn: the siblings of the _affine entries for that norm, with the same
 * arguments plus DEVICE mean, var f32[C] (the batch statistics whose fold scale / shift are) and chunk_frames.  With r = 1 / sqrt(var +
 * 1e-3), g and v as above and the sums pooled over all frames in fp64 (segments in index order, frames in frame order),
 *   c1 = dshift / N, c2 = r (dscale - mean dshift) / N   (fp64, rounded once each),   vhat = (v - mean) r,
 *   dv = scale_c ((g - c1) - vhat c2)
 * takes the place of the affine's scale_c g: du of the unit (+ dskip, one fp32 add), dz of the stage, dZ of the branch, which feed the
 * same products.  Every frame's dv depends on the sums of all frames, so each entry is two-phase across its frame chunks: the unit leaves
 * the raw dgrad product in du and rewrites it in place once the sums are in (the mask re-evaluated from u by the same fma); the stage
 * forms its sums from z and dy ahead of the chunks; the branch recomputes each chunk's Z a second time when there is more than one.
 * dscale / dshift (may be NULL) are the sums themselves: pp_bn_affine_grad(dscale, dshift, mean, var) yields dgamma, dbeta.
 * chunk_frames: 0 = the workspace rule, k > 0 = at most min(k, rule) frames per chunk; du / dx and the sums do not depend on it, dw does
 * within fp32 summation error (the K ranges).  Stateless, either norm kind, fp32, no atomics, two runs are bit-identical.  PP_E_ARG as the
 * _affine entries and for chunk_frames < 0.
 *
 * pp_set_train_chunk_frames: a cap on the frames of a chunk for the whole context, so that small tests reach the chunked paths of EVERY
 * training backward: pp_{unit,down,neck}_backward, their _affine and _mp forms (modes 1 and 2) and the three _bn entries.  All of them
 * take their frames per chunk from one rule: as many frames as fit the entry's workspace budget, at least 1, at most nb.  k = 0 (the
 * default of a fresh context) leaves that rule alone; k > 0 means at most min(k, rule) frames per chunk, in the _bn entries together with
 * their own argument as the smaller of the non-zero values.  The cap never raises the rule and changes no result beyond what chunk_frames
 * changes: du / dx, dscale / dshift keep their bits, dw moves within fp32 summation error (the K ranges follow the chunks).  Host side,
 * takes effect from the next call.  PP_E_ARG for k < 0, and the earlier value stays. */
int pp_set_train_chunk_frames(pp_ctx* ctx, int k);
int pp_backbone_train_taps_bn(pp_ctx* ctx, const float* canvas, int nb, const float* const* gamma_beta /* 38 */, float* rpn_out, float* x1,
                              float* x2, float* x3, float* const* units /* 3, may be NULL */, float* const* z /* 3, may be NULL */, float* mean,
                              float* var, float* scale, float* shift, void* stream);
int pp_unit_backward_bn(pp_ctx* ctx, int C, int h, int w, const float* u, const float* wgt, const float* scale, const float* shift,
                        const float* mean, const float* var, const float* dy, const float* dskip /* may be NULL */, int nb, float* dw,
                        float* du /* NULL: skipped */, double* dscale /* may be NULL */, double* dshift /* may be NULL */, int chunk_frames,
                        void* stream);
int pp_down_backward_bn(pp_ctx* ctx, int cin, int cout, int hin, int win, const float* x, const float* w, const float* z, const float* scale,
                        const float* shift, const float* mean, const float* var, const float* dy, int nb, float* dw, float* dx /* NULL: skipped */,
                        double* dscale /* may be NULL */, double* dshift /* may be NULL */, int chunk_frames, void* stream);
int pp_neck_backward_bn(pp_ctx* ctx, int branch, const float* x, const float* w, const float* scale, const float* shift, const float* mean,
                        const float* var, const float* y, const float* dy, int nb, float* dw, float* dx /* NULL: skipped */,
                        double* dscale /* may be NULL */, double* dshift /* may be NULL */, int chunk_frames, void* stream);

/* ---- mixed-precision training of the BatchNorm networks (block_train16.hip, down_train16.hip, neck_train16.hip) ----
 * The six _affine / _bn entries above with `int mode` behind the context, numbered as pp_unit_backward_mp numbers it: 0 fp32 (a call of
 * the fp32 sibling, bit for bit), 1 bf16x3, 2 bf16; any other mode is PP_E_ARG under the entry's name.  Modes 1 and 2 run only the two
 * gradient products of the call on v_mfma_f32_16x16x32_bf16 with fp32 accumulation, with the operand images, tiles and K ranges of the
 * InstanceNorm _mp entries; every tensor in and out, the ReLU mask, the dw partial reduction in double, the fp64 per-channel sums,
 * their reduction (affine) or pooling into c1, c2 (batch) and chunk_frames stay as they are.
 *   Stage and branch: the products read the fp32 dz / dZ that the form's own fp32 pass writes, so the mask, dz and the two sums (dscale,
 *   dshift) are the fp32 entry's bits in every mode; only dw and dx move, within the bounds of pp_down_backward_mp / pp_neck_backward_mp.
 *   Unit: a = max(fma(u, scale_c, shift_c), 0) is evaluated in fp32 and rounded (bf16) or split (bf16x3) into the 16-bit image, dy
 *   likewise; no fp32 image of a is kept, and the pass behind the dgrad takes its mask from fma(u, scale_c, shift_c) > 0 re-evaluated
 *   from u, which is the fp32 path's mask bit for bit (fma rounds once and keeps the sign).  dscale / dshift are sums over the dgrad
 *   product, so they move with du, within the bound of the form's own expressions.  A shape whose 16-bit images of one frame exceed
 *   256 MB runs the fp32 kernels (pp_unit_backward_bn_path tells).  A chunk of frames holds fewer frames than under fp32 (bf16x3: 8 against
 *   12 at level 0); the batch form's second phase reads u and du alone, so du and the sums do not depend on the chunks.
 * Stateless, either norm kind, no atomics; K ranges, segments and chunks are functions of shape, mode and chunk_frames alone, two runs are
 * bit-identical; under the affine form a frame's du / dx depends on neither nb nor the chunks; under the batch form du / dx and the sums
 * do not depend on the chunking, dw does within its bound.  PP_E_ARG as the fp32 siblings.
 * pp_{unit,down,neck}_backward_bn_path: the mode the _affine_mp and the _bn_mp entry really run at this shape (the path depends on shape
 * and mode, not on the form), on a context of either norm kind; launches nothing; an error is the negated code, as pp_unit_backward_path.
 * The stage and branch queries return `mode`; the unit query returns 0 where the images exceed the budget. */
int pp_unit_backward_affine_mp(pp_ctx* ctx, int mode, int C, int h, int w, const float* u, const float* wgt, const float* scale,
                               const float* shift, const float* dy, const float* dskip /* may be NULL */, int nb, float* dw,
                               float* du /* NULL: skipped */, double* dscale /* may be NULL */, double* dshift /* may be NULL */, void* stream);
int pp_unit_backward_bn_mp(pp_ctx* ctx, int mode, int C, int h, int w, const float* u, const float* wgt, const float* scale, const float* shift,
                           const float* mean, const float* var, const float* dy, const float* dskip /* may be NULL */, int nb, float* dw,
                           float* du /* NULL: skipped */, double* dscale /* may be NULL */, double* dshift /* may be NULL */, int chunk_frames,
                           void* stream);
int pp_down_backward_affine_mp(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win, const float* x, const float* w, const float* z,
                               const float* scale, const float* shift, const float* dy, int nb, float* dw, float* dx /* NULL: skipped */,
                               double* dscale /* may be NULL */, double* dshift /* may be NULL */, void* stream);
int pp_down_backward_bn_mp(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win, const float* x, const float* w, const float* z,
                           const float* scale, const float* shift, const float* mean, const float* var, const float* dy, int nb, float* dw,
                           float* dx /* NULL: skipped */, double* dscale /* may be NULL */, double* dshift /* may be NULL */, int chunk_frames,
                           void* stream);
int pp_neck_backward_affine_mp(pp_ctx* ctx, int mode, int branch, const float* x, const float* w, const float* scale, const float* shift,
                               const float* y, const float* dy, int nb, float* dw, float* dx /* NULL: skipped */,
                               double* dscale /* may be NULL */, double* dshift /* may be NULL */, void* stream);
int pp_neck_backward_bn_mp(pp_ctx* ctx, int mode, int branch, const float* x, const float* w, const float* scale, const float* shift,
                           const float* mean, const float* var, const float* y, const float* dy, int nb, float* dw, float* dx /* NULL: skipped */,
                           double* dscale /* may be NULL */, double* dshift /* may be NULL */, int chunk_frames, void* stream);
int pp_unit_backward_bn_path(pp_ctx* ctx, int mode, int C, int h, int w);
int pp_down_backward_bn_path(pp_ctx* ctx, int mode, int cin, int cout, int hin, int win);
int pp_neck_backward_bn_path(pp_ctx* ctx, int mode, int branch);

/* ---- training the pillar feature net: PointNet in train mode, its backward and the scatter's (pfn_train.hip) ----
 * PointNet.forward (pointpillars8_shared.py:30-60) with BatchNorm1d normalising by BATCH statistics.  Notation: f[p][t][0:9] the nine
 * decorated features of slot t of pillar p (x, y, z, r, x - mx, y - my, z - mz, x - cx, y - cy; arithmetic as pp_pfn: mean over all T
 * slots divided by n, cell centre by a separate multiply and add), all zero for padded slots t >= n_p = min(npts[p], T);
 * P = min(*num_pillars, max_batch * max_voxels) pillars of ALL frames of a batch, T = max_num_points, N = P T (BatchNorm1d sees the
 * padded slots as zeros).  z[p][t][c] = sum_k w[c][k] f[p][t][k].
 *
 * pp_pfn_train_forward: w f32[64][9] (state_dict layout of pfn_layers.0.weight), gamma / beta f32[64] are DEVICE tensors taken from the
 * call; ctx->pfn_* is not read (stateless, as pp_unit_backward).  Pass 1: s[k] = sum f[.][.][k] and M[j][k] = sum f[.][.][j] f[.][.][k]
 * in fp64 from the fp32 features (per-block partials in a fixed order, one finishing block in block order: no atomics, two runs agree
 * bit for bit), then mean_c = w_c s / N, var_c = w_c M w_c^T / N - mean_c^2 (biased), scale_c = gamma_c / sqrt(var_c + 1e-5),
 * shift_c = beta_c - mean_c scale_c, all fp64, scale / shift rounded to fp32 as pp_commit_weights rounds the eval-mode fold.
 * Pass 2: pp_pfn's kernel with that scale / shift -> feat f32[P][64] = max_t relu(scale z + shift) over all T slots (a padded slot has
 * z = 0) and arg u8[P][64], the FIRST slot that attains the maximum (n_p when a padded slot wins).
 * stats f64[218] = mean[64], var[64], s[9], M[9][9].  The partials and the folded scale / shift live in a workspace of the context
 * (allocated on first use): calls on one context must be issued in order on one stream.  The call reads *num_pillars back
 * (synchronises `stream` once) so that it can refuse before anything is launched: PP_E_ARG for a null pointer, F != 4, T > 255 (arg is
 * a byte) and P T < 2 (no unbiased variance: torch raises there too).
 *
 * pp_scatter_backward: the backward of pp_scatter for one frame is a gather, dfeat[p][c] = dcanvas[c][cx gy + cy] for
 * p < min(*num_pillars, max_voxels), zero for a coordinate outside the grid (which the forward skips).  dcanvas f32[64][gx][gy],
 * dfeat f32[P][64].
 *
 * pp_pfn_backward: from dfeat = dL/dfeat f32[P][64], with feat / arg / stats of the forward of the SAME voxels and weights.  One pass
 * over the pillars, lane = channel: g = dfeat where feat > 0 (else 0), t* = arg, zhat* = (z[p][t*][c] - mean_c) invstd_c recomputed
 * from the pillar's rows; S1_c = sum_p g, S2_c = sum_p g zhat*, G[c][k] = sum_p g f[p][t*][k] in fp64 (per-block partials in a fixed
 * order, one finishing block).  dbeta = S1, dgamma = S2,
 * dw[c][k] = gamma_c invstd_c (G[c][k] - S1_c s_k / N - S2_c invstd_c ((w M)[c][k] - mean_c s_k) / N), evaluated in fp64 and rounded.
 * dw f32[64][9], dgamma / dbeta f32[64], fully written.  No gradient with respect to the points.  Deterministic; does not synchronise.
 * PP_E_ARG for a null pointer, F != 4 and T > 255.
 *
 * pp_update_pfn_weights: after an optimizer step (or a move of the running statistics), the DEVICE tensors w f32[64][9], gamma, beta,
 * running_mean, running_var f32[64] -> the eval-mode PFN of the context (transposed weight, scale, shift), rewritten in place on
 * `stream` with the fp64 fold of pp_commit_weights: bit for bit what a fresh commit of the same values holds.  pp_pfn and the fused
 * passes read those buffers.  The host copies of pp_load_weights are NOT changed.  PP_E_STATE before the first commit. */
#define PP_PFN_STATS 218 /* doubles in stats: mean[64], var[64], s[9], M[9][9] */
int pp_pfn_train_forward(pp_ctx* ctx, const float* voxels, const int32_t* coors, const int32_t* npts, const int32_t* num_pillars,
                         const float* w, const float* gamma, const float* beta, float* feat, uint8_t* arg, double* stats, void* stream);
int pp_scatter_backward(pp_ctx* ctx, const float* dcanvas, const int32_t* coors, const int32_t* num_pillars, float* dfeat, void* stream);
int pp_pfn_backward(pp_ctx* ctx, const float* voxels, const int32_t* coors, const int32_t* npts, const int32_t* num_pillars, const float* w,
                    const float* gamma, const double* stats, const float* feat, const uint8_t* arg, const float* dfeat, float* dw,
                    float* dgamma, float* dbeta, void* stream);
int pp_update_pfn_weights(pp_ctx* ctx, const float* w, const float* gamma, const float* beta, const float* running_mean,
                          const float* running_var, void* stream);

/* ---- device optimizer: gradient-norm clipping and Adam / AdamW over a list of fp32 tensors (optim.hip) ----
 * torch.nn.utils.clip_grad_norm_ and torch.optim.Adam / AdamW (the reference's train.py:100-108) as multi-tensor kernels.  The lists
 * (device pointers and element counts) are HOST arrays of `count` entries; the library passes them to its kernels by value, in kernel
 * arguments, PP_OPT_GROUP tensors per launch: no copy to the device, no allocation per call, no host synchronisation, all work on
 * `stream`.  Every tensor is cut into chunks of PP_OPT_CHUNK elements (the last one short), one workgroup per chunk; within a chunk a
 * lane owns fixed groups of four consecutive elements, moved with 16-byte accesses where every pointer of the tensor is 16-byte
 * aligned and the group is whole, element by element otherwise.
 *
 * pp_grad_norm: out f32[2] (device) = {total_norm, coef}.  total_norm = sqrt(sum g^2) over all tensors: the squares are exact in
 * fp64 and are added in fp64, per chunk in a fixed lane / wave order into one partial per chunk (a workspace of the context, allocated
 * on the first call: calls on one context must be issued in order on one stream), the partials by one finishing workgroup (every lane a
 * contiguous run in index order, the lanes' sums in lane order), then the square root, rounded once to fp32.  No atomics: two runs agree
 * bit for bit, and neither the split into launches nor a pointer's alignment enters the order.  coef = min(1, (1 / (total_norm + 1e-6))
 * * max_norm) in fp32 (torch evaluates max_norm / tensor as reciprocal times scalar); a NaN norm gives a NaN coef, as torch.clamp does.
 * count == 0 or all lengths 0: {0, 1}.  PP_E_ARG for more than PP_OPT_MAX_CHUNKS chunks in all.
 *
 * pp_scale_grads: g *= coef[0] in place, coef on the device (out + 1 of pp_grad_norm); a coef of exactly 1 writes nothing.
 *
 * pp_adam_step: one step of Adam for the tensors whose g is not NULL (the others are skipped entirely), all at step number t >= 1.
 * Per element in fp32: g' = coef[0] g (coef NULL: g; g is not written); weight_decay != 0: g' = fma(wd, p, g') (decoupled == 0, L2) or
 * p = fma(-lr wd, p, p) (decoupled != 0, AdamW); m = fma(beta1, m, (1 - beta1) g'); v = fma(beta2, v, ((1 - beta2) g') g');
 * p = p - (lr / (1 - beta1^t)) m / (sqrt(v) / sqrt(1 - beta2^t) + eps).  The bias corrections, 1 - beta and lr wd are computed on the
 * host in double and rounded to fp32.  One pass: p, g, m, v read once, p, m, v written once.
 *
 * All three: PP_E_ARG for a null list, a null pointer with a non-zero length (g of pp_adam_step excepted), a negative length, a
 * pointer that is not 4-byte aligned, t < 1, beta outside [0, 1) and negative lr / eps / weight_decay; refused before anything is
 * launched. */
#define PP_OPT_CHUNK 2048        /* elements per workgroup */
#define PP_OPT_GROUP 32          /* tensors per launch */
#define PP_OPT_MAX_CHUNKS 262144 /* partials of pp_grad_norm (2 MB): 2^29 elements in whole chunks */
int pp_grad_norm(pp_ctx* ctx, const float* const* grads, const int64_t* lens, int count, float max_norm, float* out, void* stream);
int pp_scale_grads(pp_ctx* ctx, float* const* grads, const int64_t* lens, int count, const float* coef, void* stream);
int pp_adam_step(pp_ctx* ctx, float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* lens, int count,
                 int64_t t, double lr, double beta1, double beta2, double eps, double weight_decay, int decoupled, const float* coef,
                 void* stream);

/* Stateless box ops (replace framework/box_torch_ops.py:18-77 and framework/nms.py:6-40,
 * eval/iou.py:438-473). */
int pp_box_decode(const float* enc, const float* anchors, float* out, int64_t n, void* stream);
int pp_corners2d(const float* centers, const float* dims, const float* angles /* may be NULL */, float* corners /*[n,4,2]*/,
                 int64_t n, void* stream);
int pp_standup2d(const float* corners /*[n,4,2]*/, float* boxes /*[n,4]*/, int64_t n, void* stream);
/* dets f32[n,stride] (stride 5: x1,y1,x2,y2,score; 6: cx,cy,dx,dy,angle,score); keep i32[n], nkeep i32[1].
 * Sorts by score (desc, ties by lower index), builds the 64x64 bitmask tiles, greedy sweep on device. */
int pp_nms(const float* dets, int n, int stride, float thresh, int32_t* keep, int32_t* nkeep, int rotate, void* stream);
int pp_rotated_iou(const float* boxes_a /*[n,5]*/, const float* boxes_b /*[m,5]*/, float* iou /*[n,m]*/, int n, int m, void* stream);

/* ---- ROS ingest ----
 * pp_unpack_points replaces `np.asarray(list(pc2.read_points(msg)))[:, :4].astype(np.float32)` (ros_node.py:55-59):
 * the first four fields of a sensor_msgs/PointCloud2 payload -> f32[n,4] on the device.  `data` is the message's byte
 * buffer in device memory; point i sits at (i / width) * row_step + (i % width) * point_step; offs/dtypes are HOST
 * arrays of the four fields' byte offsets and PointField datatype codes (1 INT8, 2 UINT8, 3 INT16, 4 UINT16,
 * 5 INT32, 6 UINT32, 7 FLOAT32, 8 FLOAT64). */
int pp_unpack_points(const void* data, int64_t n, int64_t width, int64_t row_step, int point_step, const int32_t* offs /*[4]*/,
                     const int32_t* dtypes /*[4]*/, int big_endian, float* out /*[n,4]*/, void* stream);

/* ---- training-input augmentation (framework/dataset.py:121-146, augmentation.py, box_np_ops.py:6-16,102-104,460-467) ----
 * All three run nb frames on `stream` with no host synchronisation.  box_off_h / pt_off_h: HOST i32[nb+1] CSR offsets (frame f owns
 * box rows box_off_h[f] .. box_off_h[f+1]-1; at most PP_AUG_MAX_BOXES per frame and PP_ASSIGN_MAX_GT in all).  boxes f32[G][7]
 * (x, y, z, l, w, h, r) as the reference's gt_boxes, valid u8[G] its valid_mask (GenericDataset passes the class mask of ALL
 * annotations, so box i reads entry i of the unfiltered list).  prm f64[nb][PP_AUG_PARAMS] per frame: PP_AUG_ON holds step bits
 * (1 box noise move, 2 flip, 4 rotations, 8 scaling, 16 translation, 32 range filter + limit_period, 64 permutation from the
 * keyed Feistel bijection of prm[PP_AUG_KEY_LO / _HI] instead of perm; 0: points only permuted by perm), then flip, pitch / roll /
 * yaw in radians (the reference's `deg / 180 * np.pi`), the three scales and the three translations, as the reference draws them. */
#define PP_AUG_MAX_BOXES 256 /* boxes per frame (LDS of the noise and points kernels) */
#define PP_AUG_MAX_TRIES 128 /* noise tries per box (one lane each; the reference uses 100) */
#define PP_AUG_PARAMS 16
enum { PP_AUG_ON = 0, PP_AUG_FLIP = 1, PP_AUG_PITCH = 2, PP_AUG_ROLL = 3, PP_AUG_YAW = 4, PP_AUG_SX = 5, PP_AUG_SY = 6, PP_AUG_SZ = 7,
       PP_AUG_TX = 8, PP_AUG_TY = 9, PP_AUG_TZ = 10, PP_AUG_KEY_LO = 11, PP_AUG_KEY_HI = 12 };
/* device random mode: fills loc f64[G][num_try][3], rot / grot f64[G][num_try] and prm f64[nb][PP_AUG_PARAMS] (steps -> PP_AUG_ON;
 * the permutation key in PP_AUG_KEY_LO / _HI) from Philox4x32-10 keyed by seed, counter (element, stream | epoch << 8, sample_h[f]):
 * HOST i64[nb] sample indices, epoch < 2^24.  53-bit uniforms, float64 Box-Muller normals, the reference's ranges.  A frame's draws
 * depend only on (seed, epoch, sample index).  Replaces the host draws and the permutation upload of the numpy mode. */
int pp_augment_draw(pp_ctx* ctx, uint64_t seed, uint32_t epoch, const int64_t* sample_h, int steps, int num_try, const int32_t* box_off_h,
                    int nb, double* loc, double* rot, double* grot, double* prm, void* stream);
/* replaces noise_per_box_v2_ + box_collision_test (augmentation.py:122-175,617-697) as noise_per_object (:177-212) calls them:
 * loc f64[G][num_try][3], rot and grot f64[G][num_try] (the reference's loc_noises, rot_noises, global_rot_noises) -> sel i32[G]
 * (chosen try, -1 if none or not valid), sel_loc f64[G][3], sel_rot f64[G] (_select_transform's loc / rot rows with the
 * dst_pos / dst_grot corrections; 0 when sel is -1).  Containment without an edge crossing is a collision (numba semantics). */
int pp_augment_noise(pp_ctx* ctx, const float* boxes, const uint8_t* valid, const double* loc, const double* rot, const double* grot,
                     int num_try, const int32_t* box_off_h, int nb, int32_t* sel, double* sel_loc, double* sel_rot, void* stream);
/* replaces box3d_transform_ (:419-425), random_flip, global_rotation_v2, global_scaling_v2, global_translate on the boxes, then
 * filter_gt_box_outside_range against range_h (HOST f32[4]: x0, y0, x1, y1) and limit_period(r, 0.5, 2 pi) (dataset.py:136-143).
 * Outputs: keep u8[G]; the kept boxes f32[G][7] and their classes i32[G] (from cls i32[G]) compacted in order at the start of each
 * frame's slot, zero behind; kept i32[nb] per frame. */
int pp_augment_boxes(pp_ctx* ctx, const float* boxes, const int32_t* cls, const uint8_t* valid, const double* sel_loc,
                     const double* sel_rot, const double* prm, const float* range_h, const int32_t* box_off_h, int nb, float* out,
                     int32_t* out_cls, uint8_t* keep, int32_t* kept, void* stream);
/* replaces points_in_rbbox + points_transform_ (box_np_ops.py:460-467, augmentation.py:400-416), the global functions on the points
 * and np.random.shuffle (dataset.py:146): out row k (f32[P][4], P = pt_off_h[nb]) of frame f is frame f's input row perm[k]
 * (i32[P], frame-local, not validated: an entry outside [0, n) reads row k; NULL: identity) moved by the first VALID box (original boxes, before the noise) containing it, then by the
 * global chain.  Feature 3 passes through. */
int pp_augment_points(pp_ctx* ctx, const float* pts, const int32_t* perm, const int32_t* pt_off_h, const float* boxes,
                      const uint8_t* valid, const double* sel_loc, const double* sel_rot, const double* prm, const int32_t* box_off_h,
                      int nb, float* out, void* stream);

/* ---- ground-truth database sampling (the `# sample` slot of framework/dataset.py:123; a build-side extension: the reference has the
 * slot and the helpers -- points_in_rbbox, box_collision_test, remove_points_in_boxes -- but no sampler) ----
 * All entries run nb frames on `stream` with no host synchronisation; *_off_h are HOST i32[nb+1] CSR offsets, box rows are
 * (x, y, z, l, w, h, r), points f32[.][4] (16-byte aligned).  Membership is points_in_rbbox with origin (0.5, 0.5, 0.5): inside at
 * sign < 0 on all six faces, the planes pp_augment_points builds.  Collision is box_collision_test on the BEV corners as
 * pp_augment_noise evaluates it (containment collides), the candidate as `boxes`, the other box as `qboxes`.  At most
 * PP_ASSIGN_MAX_GT box / candidate rows per call.  PP_E_ARG for null or misaligned pointers, offsets that do not start at 0 or
 * decrease, and counts above the capacities; nothing is launched then.  Two runs are bit-identical: every order comes from ballots
 * and prefix counts, never from atomics. */
#define PP_GT_CHUNK 1024 /* scene points per entry of `blk` (pp_gt_paste_count / pp_gt_paste) */
/* counts i32[G]: per box the points of its frame inside it after extra_h (HOST f32[3]) is added to (l, w, h) in float32; a point
 * inside two boxes counts in both.  extra (0, 0, 0): annos["num_points"] of create_info.py:175-177; (1.2, 0.5, 8): its "difficulty". */
int pp_gt_count(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* boxes, const int32_t* box_off_h, int nb,
                const float* extra_h, int32_t* counts, void* stream);
/* out f32[T][4]: box g's member points (extra 0) in the cloud's order at rows obj_off[g] .. obj_off[g+1]-1 (DEVICE i64[G+1], the
 * counts' exclusive scan with the total behind), xyz minus the box centre (one float32 subtraction each), feature 3 copied.  No row
 * outside an object's range or outside [0, T) is written, whatever obj_off holds. */
int pp_gt_extract(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* boxes, const int32_t* box_off_h, int nb,
                  const int64_t* obj_off, int64_t T, float* out, void* stream);
/* accept u8[Gc]: per frame the candidates (cand f32[Gc][7], cand_off_h, already in decision order) taken in order: candidate j is
 * accepted iff it collides with no existing box of the frame (boxes f32[G][7], box_off_h; valid or not) and with no earlier ACCEPTED
 * candidate.  existing + candidates of a frame <= PP_AUG_MAX_BOXES. */
int pp_gt_select(pp_ctx* ctx, const float* boxes, const int32_t* box_off_h, const float* cand, const int32_t* cand_off_h, int nb,
                 uint8_t* accept, void* stream);
/* The database is device-resident: db_points f32[db_T][4] (object-local xyz), db_off i64[n_db+1]; candidate g is object
 * cand_idx[g] (i32[Gc]).  A candidate whose index lies outside [0, n_db) or whose rows lie outside [0, db_T) counts as NOT accepted
 * in both entries, and nothing of it is read.  At most PP_AUG_MAX_BOXES candidates per frame.
 * pp_gt_paste_count: out_n i32[nb] = the points of the frame's accepted objects + its surviving scene points; remove != 0 drops a
 * scene point inside any accepted candidate box (remove_points_in_boxes).  blk i32[sum_f ceil(n_f / PP_GT_CHUNK)] receives the
 * survivors per chunk of scene points and is read back by pp_gt_paste (same arguments, same stream).
 * pp_gt_paste: out f32[out_off_h[nb]][4], per frame (out_off_h: HOST CSR of out_n) the accepted objects in candidate order, each
 * point local + the candidate box's centre (one float32 addition each), then the surviving scene points in their order, bits
 * unchanged.  No row outside the frame's slot is written. */
int pp_gt_paste_count(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* cand, const int32_t* cand_idx,
                      const uint8_t* accept, const int32_t* cand_off_h, int nb, const int64_t* db_off, int64_t n_db, int64_t db_T,
                      int remove, int32_t* blk, int32_t* out_n, void* stream);
int pp_gt_paste(pp_ctx* ctx, const float* pts, const int32_t* pt_off_h, const float* cand, const int32_t* cand_idx, const uint8_t* accept,
                const int32_t* cand_off_h, int nb, const float* db_points, const int64_t* db_off, int64_t n_db, int64_t db_T, int remove,
                const int32_t* blk, const int32_t* out_off_h, float* out, void* stream);
/* device random mode: cand_idx i32[Gc], for frame f the classes in order, class c contributing k_h[f][c] (HOST i32[nb][num_classes],
 * 0 .. n_c) rows: class_off_h[c] + the first k values of the keyed Feistel bijection on [0, n_c) (the one pp_augment_points uses),
 * n_c = class_off_h[c+1] - class_off_h[c] (HOST i32[num_classes+1]), so no object is drawn twice.  The key is Philox4x32-10 of
 * (seed, counter (class, stream 16 | epoch << 8, sample_h[f])): a stream pp_augment_draw does not use; the draw depends on (seed,
 * epoch, sample index, class) only.  cand_off_h must equal the row sums of k_h. */
int pp_gt_draw(pp_ctx* ctx, uint64_t seed, uint32_t epoch, const int64_t* sample_h, const int32_t* class_off_h, int num_classes,
               const int32_t* k_h, const int32_t* cand_off_h, int nb, int32_t* cand_idx, void* stream);

/* ---- evaluation ----
 * pp_rotated_iou_eval replaces rotate_iou_gpu_eval (eval/iou.py:540-638): out[i,j] for box i and query j with
 * criterion -1: IoU, 0: inter / area(query), 1: inter / area(box), 2: intersection area -- the reference's kernel
 * hands the QUERY box to devRotateIoUEval first (:600-603).  Device pointers, boxes are (cx,cy,dx,dy,angle).
 * pp_eval_statistics / pp_eval_fused_statistics replace the numba host loops compute_statistics_jit and
 * fused_compute_statistics (eval/eval.py:62-119,182-216); HOST pointers, no GPU work.  overlaps is row-major
 * [det rows][gt columns] with `ov_ld` doubles per row; ignored_* are the reference's -1/0/1 codes.
 * thresholds_out must hold gt_size doubles; pr is [nthresh][4] and accumulated into (tp, fp, fn, unused). */
int pp_rotated_iou_eval(const float* boxes /*[n,5]*/, const float* qboxes /*[k,5]*/, float* out /*[n,k]*/, int n, int k, int criterion,
                        void* stream);
int pp_eval_statistics(const double* overlaps, int64_t ov_ld, int det_size, int gt_size, const int64_t* ignored_gt,
                       const int64_t* ignored_det, const float* dt_scores, double min_overlap, double thresh, int compute_fp,
                       int64_t* tp_fp_fn /*[3]*/, double* thresholds_out, int64_t* n_thresholds);
int pp_eval_fused_statistics(const double* overlaps, int64_t ov_ld, double* pr, const int64_t* gt_nums, const int64_t* dt_nums,
                             int n_frames, const int64_t* ignored_gts, const int64_t* ignored_dets, const float* dt_scores,
                             double min_overlap, const double* thresholds, int n_thresholds);

/* One (class, overlap threshold) cell of the AP table in one call: the loop nest of eval/eval.py:396-434 (per-frame
 * compute_statistics_jit at threshold 0, get_thresholds :42-59, fused_compute_statistics per part, precision / recall and
 * the running maximum).  parts_h[j]: row-major [detections of part j][ground truths of part j] overlaps; part_frames_h:
 * frames per part; *_nums_h per frame; ignored_* (-1/0/1 codes) and dt_scores concatenated in frame order.
 * precision_h / recall_h: n_sample_pts (41) doubles, zero behind the last threshold like the reference's np.zeros. */
int pp_eval_class_ap(const double* const* parts_h, const int64_t* part_frames_h, int n_parts, const int64_t* dt_nums_h,
                     const int64_t* gt_nums_h, int64_t n_frames, const int64_t* ignored_gt_h, const int64_t* ignored_dt_h,
                     const float* dt_scores_h, double min_overlap, int64_t num_valid_gt, int n_sample_pts, double* precision_h,
                     double* recall_h);

/* Measurement hooks for bench.py: between begin and end every launch of the dominant kernel
 * (conv3x3 stride 1 on the level-0 map, 3 launches per frame) is bracketed by hipEvents on the
 * launch stream.  pp_profile_end synchronises the events and reports the average duration (ms),
 * the number of launches seen and the algorithmic FLOPs of one launch (2*H*W*Cin*Cout*9). */
int pp_profile_begin(pp_ctx* ctx);
int pp_profile_end(pp_ctx* ctx, double* avg_ms_h, int32_t* launches_h, double* flops_per_launch_h);
/* executed MFMA flops / algorithmic (direct-convolution) flops of that layer's tiling (Winograd F(2x2,3x3): 4/9) */
double pp_dominant_executed_ratio(pp_ctx* ctx);
/* Per-stage GPU time of the fused path: between begin and end every pp_infer_batch pass records one event per stage
 * boundary on its stream (and so does a stand-alone pp_postprocess); end synchronises and sums the milliseconds
 * per stage into ms_h[12]: 0 voxelise, 1 anchor mask, 2 PFN + pillar map, 3 conv / deconv launches (+ statistics
 * finalisation), 4 norm_relu_stats, 5 head, 6 post-processing filter (mask, sigmoid, threshold, candidate gather),
 * 7 exact top-k + box decode, 8 NMS + direction flip / range mask / compaction (9-11 unused).
 * Meant for an untimed side pass of bench.py and for the drop-in classes' p1..p4 / stage timers. */
int pp_stage_profile_begin(pp_ctx* ctx);
int pp_stage_profile_end(pp_ctx* ctx, double* ms_h);
/* The network's launch plan as text, one line per conv / deconv / head layer in execution order:
 * "<index> kind=<0 conv3x3|1 deconv|2 head> cin= cout= stride= up= level= wino=<kernel family: 0 direct|1,4,6 Winograd|3 1x1 GEMM|5 16-bit conv> tiling=<name>".
 * Returns the text length (buf may be NULL to query). */
int pp_layer_tilings(pp_ctx* ctx, char* buf_h, int cap);
/* Test / inspection hook: the packed weight image of layer `layer` of the committed plan (0 .. 19 in pp_layer_tilings order), or the
 * sparse first convolution's own image of rpn.block1.0.weight (layer = -1), copied to DEVICE memory dst (cap bytes) on `stream`.  The
 * image's size comes back through bytes_h; dst may be NULL to query it.  What the in-place weight updates are compared by. */
int pp_weight_image(pp_ctx* ctx, int layer, void* dst, size_t cap, size_t* bytes_h, void* stream);
/* The autotuner's table (process-wide) as text, "layer signature<TAB>tiling" per line.  Rank 0 of a multi-GPU job
 * tunes, exports and broadcasts it; the other ranks import it BEFORE pp_commit_weights so all ranks run identical
 * kernels.  pp_tune_export returns the text length (buf may be NULL to query), pp_tune_import the lines taken. */
int pp_tune_export(char* buf_h, int cap);
int pp_tune_import(const char* text_h);
/* The tilings the tuner chooses from, by name, one per line and in menu order; stateless, no device needed.  which 0: the menu of a
 * layer, named the way the plan composes it -- kind (0 conv3x3, 1 upsampler, 2 head), stride (conv: 1 / 2), up (upsampler: 1 / 2 / 4),
 * cin, prec (0 .. 4 as pp_set_precision), head9 (the head has the reference's 9 anchors per location), first_conv (the strided conv of
 * level 0); which 1: the menu of the cls-only head pass; which 2: the four strip tilings of wino4 / wino6 (right, bottom of each).
 * rows > 0 keeps only the entries legal for a layer of `rows` GEMM rows (conv: cout, upsampler: cout up^2, head: 96) and cin input
 * channels on maps Hin x Win -> width Wout (the upsampler's Wout is its input width), by the rule the tuner itself applies; rows <= 0
 * returns the whole menu.  Returns the text length (buf_h may be NULL to query; at most cap - 1 characters are written), -1 for a
 * selector out of range. */
int pp_menu_names(int which, int kind, int stride, int up, int cin, int prec, int head9, int first_conv, int rows, int Hin, int Win, int Wout,
                  char* buf_h, int cap);
/* name of the tiling the autotuner chose for that dominant layer (static string owned by ctx) */
const char* pp_dominant_kernel(pp_ctx* ctx);
int pp_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PP_HIP_H */
