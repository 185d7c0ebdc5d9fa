/* odet.h -- C ABI of libodet_hip.so: the MI355X (gfx950) detection hot path.
 *
 * Drop-in boundary for the Faster-R-CNN / FPN inference hot path of
 * irvingzhang0512/tf_eager_object_detection.  The reference has no FFI of its own (it is
 * 100 % Python over TensorFlow ops); each entry point below replaces the TensorFlow work
 * behind one reference function, cited as file:line relative to the reference checkout.
 * The Python package tf_eager_object_detection_amd re-creates the reference's call surface
 * on top of these symbols with ctypes (see INTEGRATION.md for the binding).
 *
 * Conventions
 *  - extern "C", plain pointers + sizes, no C++/torch types.  All array pointers are DEVICE
 *    pointers (HBM) unless the parameter is documented "host".  The caller owns every
 *    buffer; the library allocates nothing.  Scratch memory is a caller-provided workspace
 *    sized by the matching *_workspace_bytes() query.
 *  - `stream` is a hipStream_t passed as void* (0 = null stream).  Calls only enqueue work;
 *    the few that must read a device-side count to decide how much more work to enqueue say
 *    so ("host-syncs on `stream`").
 *  - Boxes are float32 [x1,y1,x2,y2] rows; feature maps are NHWC float32 with batch = 1.
 *  - Return value: 0 = ok, negative = error (ODET_E_*); odet_last_error() gives the text for
 *    the calling thread.  Nothing throws across the ABI.
 *  - Arithmetic is float32 in the reference's operation order, no FMA contraction; exp/log
 *    are correctly rounded float32.  Ties in NMS / top-k: (score desc, index asc).
 */
#ifndef ODET_H_
#define ODET_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 100: round 4.  101: odet_fpn_step_t.ws_post_clean, the odet_*_x3 entry points (three bfloat16 limbs) with their split-K
 * workspace.  102: the odet_*_x2 entry points (two float16 limbs) and odet_split_f16x2; odet_bias_relu_maxpool keeps a NaN
 * in float32.  103: the two-limb launches report an out-of-range activation in a status word of their workspace
 * (odet_x2_status_offset); the tile-forcing diagnostics left this header and the shipped library (include/odet_diag.h, a
 * separate -DODET_DIAG build).  Added within 103: odet_preprocess_images (the eval loaders' input front end),
 * odet_eval_detect_topk, the odet_coco_* evaluation, the odet_voc_* evaluation and the fused training targets
 * (odet_anchor_target, odet_proposal_target) and the fused training losses with their gradients (odet_rpn_loss,
 * odet_rpn_loss_backward, odet_roi_loss) and odet_preprocess_train (the training input stage) and the training step
 * (odet_opt_step, odet_l2_loss, odet_opt_partials_bytes with the odet_opt_*_t records) and the float32 Dense backward
 * (odet_dense_dgrad_f32, odet_dense_wgrad_f32, odet_dense_grad_workspace_bytes), the 3x3 convolution's weight gradient
 * (odet_conv3x3_wgrad_f32_levels, odet_conv3x3_wgrad_workspace_bytes, odet_rpn_unpack_pair) and the RoI pooling backward
 * (odet_roi_pool_argmax, odet_roi_pool_backward) and the FPN top-down merge's backward (odet_fpn_topdown_backward_f32) and the
 * two elementwise launches of the ResNet bottleneck's backward (odet_stride_gather_f32, odet_block_input_grad_f32) and the VGG16
 * training graph's max-pooling and dropout backward (odet_relu_maxpool2_backward_f32, odet_dropout_f32, odet_dropout_backward_f32) and
 * the ResNet-C4 head's global average pooling (odet_global_avg_pool_f32, odet_global_avg_pool_backward_f32) and the
 * data-parallel gradient exchange (odet_bucket_pack_f32, odet_bucket_unpack_f32, odet_rank_mean_f32) and the FPN stem's
 * max-pooling backward (odet_relu_maxpool3_backward_f32) and the K-image step's accumulate launch
 * (odet_bucket_accumulate_f32) and the RoI pooling over a dense batch of images (odet_roi_pool_images,
 * odet_roi_pool_argmax_images, odet_roi_pool_backward_images, odet_roi_pool_backward_images_plan) and the FPN level
 * assignment over a dense batch of images (odet_assign_levels_images); no
 * existing struct or signature changed.  One documented order did: from
 * 4096 rows on, odet_dense_wgrad_f32 adds db in 256 running sums per column, not 4 (its own comment; below 4096 rows every bit is
 * as before). */
#define ODET_VERSION 103

#define ODET_OK 0
#define ODET_E_INVALID (-1)   /* bad argument (null pointer, negative size, unsupported shape) */
#define ODET_E_WORKSPACE (-2) /* workspace too small */
#define ODET_E_HIP (-3)       /* a HIP runtime call failed */
#define ODET_E_LIMIT (-4)     /* size exceeds a documented kernel limit */

typedef void* odet_stream_t;

int odet_version(void);
const char* odet_last_error(void);

/* ---- anchors ------------------------------------------------------------------------ */

/* utils/anchor_generator.py:46-60 generate_by_anchor_base_tf.
 * out[(y*fw+x)*A+a] = base[a] + (x*stride, y*stride, x*stride, y*stride).
 * anchor_base: device [A,4]; out: device [fh*fw*A,4]. */
int odet_anchors_shift(const float* anchor_base, int A, int feat_stride, int fh, int fw,
                       float* out, odet_stream_t stream);

#define ODET_MAX_LEVELS 8
#define ODET_MAX_ANCHORS_PER_CELL 32
/* utils/anchor_generator.py:137-178 make_anchors for ALL pyramid levels in one launch
 * (caller loop: model/fpn/base_fpn_model.py:163-186 _get_anchors).
 * Host arrays: fh/fw/stride [num_levels]; wh [num_levels*A*2] = per level, per anchor
 * (w, h) in float32 exactly as enum_scales/enum_ratios produce them (the Python layer
 * evaluates that A-element table with IEEE float32 ops).  out: device [sum fh*fw*A, 4],
 * levels concatenated in order, location-major / anchor-minor inside a level. */
int odet_anchors_fpn(int num_levels, int A, const int* fh, const int* fw, const int* stride,
                     const float* wh, float* out, odet_stream_t stream);

/* ---- box transforms ------------------------------------------------------------------ */

/* utils/bbox_transform.py:32-55 decode_bbox_with_mean_and_std.  means/stds: host [4].
 * If clip_h > 0 the result is also clipped to [0, clip_w-1] x [0, clip_h-1] as
 * utils/bbox_tf.py:70-74 does with min_value 0 (fusion used by region_proposal.py:59-63).
 * delta_stride: floats between consecutive delta rows (4 for a dense [n,4] array), >= 4.
 * deltas needs float alignment only: a row is read as one 16-byte load where the stride is
 * a multiple of 4 and the pointer is 16-byte aligned, as four floats otherwise. */
int odet_decode(const float* anchors, const float* deltas, int64_t delta_stride, int n,
                const float* means, const float* stds, int clip_h, int clip_w, float* out,
                odet_stream_t stream);

/* utils/bbox_transform.py:4-29 encode_bbox_with_mean_and_std. */
int odet_encode(const float* src, const float* dst, int n, const float* means, const float* stds,
                float* out, odet_stream_t stream);

/* utils/bbox_tf.py:59-78 bboxes_clip_filter with min_edge=None: clip only. */
int odet_clip(const float* boxes, int n, float min_value, int max_h, int max_w, float* out,
              odet_stream_t stream);

size_t odet_compact_workspace_bytes(int n);
/* utils/bbox_tf.py:59-84 bboxes_clip_filter with min_edge: clip, keep rows with both
 * (+1) edges >= min_edge, ascending index order.  out_boxes [n,4], out_idx int64 [n],
 * out_count device int32[1]. */
int odet_clip_filter(const float* boxes, int n, float min_value, int max_h, int max_w,
                     float min_edge, float* out_boxes, int64_t* out_idx, int32_t* out_count,
                     void* workspace, size_t workspace_bytes, odet_stream_t stream);

/* utils/bbox_tf.py:87-101 bboxes_range_filter: indices of boxes fully inside the image. */
int odet_range_filter(const float* boxes, int n, int max_h, int max_w, int64_t* out_idx,
                      int32_t* out_count, void* workspace, size_t workspace_bytes,
                      odet_stream_t stream);

/* model/prediction.py:136 tf.where(score > thr): ascending indices of values[i*stride] > thr. */
int odet_where_greater(const float* values, int64_t stride, int n, float thr, int64_t* out_idx,
                       int32_t* out_count, void* workspace, size_t workspace_bytes,
                       odet_stream_t stream);

/* utils/bbox_tf.py:37-56 pairwise_iou (+1 convention, 0 where intersection == 0).
 * out: device [n,m] row-major. */
int odet_pairwise_iou(const float* boxes1, int n, const float* boxes2, int m, float* out,
                      odet_stream_t stream);

/* rows gather: out[i,:] = src[idx[i],:] for i < count (count_dev overrides n when non-null).
 * idx_is_64 selects int64 / int32 indices.  row_floats floats per row. */
int odet_gather_rows(const float* src, const void* idx, int idx_is_64, int n,
                     const int32_t* count_dev, int row_floats, float* out, odet_stream_t stream);

/* ---- RPN score glue ------------------------------------------------------------------ */

#define ODET_RPN_LAYOUT_FPN 0   /* model/fpn/base_fpn_model.py:223,429: [n,2] (bg,fg) pairs */
#define ODET_RPN_LAYOUT_FRCNN 1 /* model/faster_rcnn/base_faster_rcnn_model.py:149-152:
                                   per location [A bg | A fg] */
/* fg probability = softmax(bg,fg)[1] with tf.nn.softmax arithmetic.  logits: [nloc, 2*A]
 * (FRCNN) or [n,2] with A ignored (FPN, nloc = n).  out: [nloc*A] resp. [n]. */
int odet_rpn_fg_softmax(const float* logits, int nloc, int A, int layout, float* out,
                        odet_stream_t stream);

/* ---- NMS / region proposal ----------------------------------------------------------- */

size_t odet_nms_workspace_bytes(int n, int max_output);
/* tf.image.non_max_suppression (NonMaxSuppressionV3, score_threshold=-inf) as called at
 * model/region_proposal.py:74-76 and model/prediction.py:146: exact greedy NMS over all n
 * boxes, IoU without +1, strict '>', stop at max_output.  out_idx int32 [max_output]
 * (original indices in keep order), out_boxes (nullable) [max_output,4] gathered rows,
 * out_count device int32[1].
 * Candidates are consumed in (score desc, index asc) order in chunks: chunk 0 = the best
 * ~1.5*max_output candidates (radix select, no full sort); if it does not reach max_output the
 * remaining candidates are fully sorted and consumed in chunks of 4096.  `blind_chunks` (>= 1)
 * chunks are enqueued unconditionally (the work of a chunk after completion is skipped on the
 * device).
 *  - out_done == NULL  (exact mode): if more chunks may be needed the call host-syncs on
 *    `stream` once per further chunk until the device reports completion.  Always exact.
 *  - out_done != NULL  (sync-free mode, graph-capturable): exactly blind_chunks chunks run;
 *    *out_done (device int32) = 1 when the result is complete, 0 when max_output was not
 *    reached within them; odet_nms / odet_region_proposal then hold the exact PREFIX found so far
 *    (out_count of it), the caller re-runs in exact mode.  The fused stages whose count feeds further
 *    kernels on the device (odet_fpn_proposals, odet_frcnn_proposals, the step descriptor) report an
 *    incomplete result as ZERO proposals (*out_count = 0, level counts 0, *out_done = 0): nothing
 *    downstream ever runs on a partial or stale RoI list -- an image that did not complete yields no
 *    detections and says so. */
int odet_nms(const float* boxes, const float* scores, int n, int max_output, float iou_threshold,
             int32_t* out_idx, float* out_boxes, int32_t* out_count, int blind_chunks,
             int32_t* out_done, void* workspace, size_t workspace_bytes, odet_stream_t stream);

size_t odet_region_proposal_workspace_bytes(int n, int max_output);
/* model/region_proposal.py:55-81 RegionProposal.call: decode (means/stds host [4]) -> clip
 * to the image -> NMS over ALL n anchors -> gather.  out_rois [max_output,4], out_idx
 * (nullable) int32 [max_output], out_count device int32[1]; blind_chunks / out_done as in
 * odet_nms. */
int odet_region_proposal(const float* deltas, const float* anchors, const float* scores, int n,
                         int image_h, int image_w, const float* means, const float* stds,
                         int max_output, float iou_threshold, float* out_rois, int32_t* out_idx,
                         int32_t* out_count, int blind_chunks, int32_t* out_done, void* workspace,
                         size_t workspace_bytes, odet_stream_t stream);

size_t odet_fpn_proposals_workspace_bytes(int n, int max_output);
/* The whole proposal stage of model/fpn/base_fpn_model.py BaseFPN.call in one entry point:
 * :220 _get_anchors (utils/anchor_generator.py:137-178, anchors are produced in registers and
 * never stored), :223 softmax(rpn_score)[:,1], :224 RegionProposal (model/region_proposal.py:
 * 55-81) and, when out_sorted_rois != NULL, :256 _assign_levels (:303-324) fused into the last
 * NMS launch.  rpn_logits [n,2] (bg,fg) as RpnHead emits them (:429), rpn_deltas [n,4], levels
 * concatenated in list order; fh/fw/stride/wh host arrays as in odet_anchors_fpn
 * (n = sum fh*fw*A).  Outputs as odet_region_proposal + odet_assign_levels.  out_order (nullable,
 * int32 [max_output], needs out_sorted_rois and max_output <= ODET_FUSED_ORDER_MAX_ROIS): the spatial
 * processing order of the level-sorted RoIs for odet_roi_pool_ordered (what odet_roi_order computes),
 * produced by the tail of the NMS walk instead of a launch of its own. */
#define ODET_FUSED_ORDER_MAX_ROIS 1024
int odet_fpn_proposals(const float* rpn_logits, const float* rpn_deltas, int num_levels, int A,
                       const int* fh, const int* fw, const int* stride, const float* wh,
                       int image_h, int image_w, const float* means, const float* stds,
                       int max_output, float iou_threshold, int min_level, int max_level,
                       float* out_rois, int32_t* out_idx, int32_t* out_count,
                       float* out_sorted_rois, int32_t* out_level, int64_t* out_perm,
                       int32_t* out_level_counts, int32_t* out_order, int blind_chunks,
                       int32_t* out_done, void* workspace, size_t workspace_bytes, odet_stream_t stream);

size_t odet_frcnn_proposals_workspace_bytes(int n, int max_output);
/* The proposal stage of model/faster_rcnn/base_faster_rcnn_model.py BaseFasterRcnn.call in one entry
 * point: :139-142 generate_by_anchor_base_tf (utils/anchor_generator.py:46-60, anchors produced in
 * registers), :149-152 fg probability from the [A bg | A fg] channel layout, :153 RegionProposal
 * (model/region_proposal.py:55-81).  rpn_logits [fh*fw, 2A], rpn_deltas [fh*fw*A, 4],
 * anchor_base host [A,4] float32 (generate_anchor_base cast to float32, :84).  n = fh*fw*A. */
int odet_frcnn_proposals(const float* rpn_logits, const float* rpn_deltas, const float* anchor_base,
                         int A, int feat_stride, int fh, int fw, int image_h, int image_w,
                         const float* means, const float* stds, int max_output,
                         float iou_threshold, float* out_rois, int32_t* out_idx,
                         int32_t* out_count, int blind_chunks, int32_t* out_done, void* workspace,
                         size_t workspace_bytes, odet_stream_t stream);

/* ---- FPN level assignment ------------------------------------------------------------ */

#define ODET_ASSIGN_MAX_ROIS 8192
/* model/fpn/base_fpn_model.py:303-324 _assign_levels.  rois [n,4] (count_dev overrides n
 * when non-null; n is then the capacity).  Outputs: out_rois [n,4] level-sorted (stable),
 * out_level int32 [n] (level - min_level of each SORTED row), out_perm int64 [n] (original
 * row of each sorted row), out_counts int32 [max_level-min_level+1]. */
int odet_assign_levels(const float* rois, int n, const int32_t* count_dev, int min_level,
                       int max_level, float* out_rois, int32_t* out_level, int64_t* out_perm,
                       int32_t* out_counts, odet_stream_t stream);

#define ODET_ASSIGN_MAX_BATCH 64     /* what one fused targets call produces */
/* odet_assign_levels for B images in dense tensors, ONE launch (workgroup b = image b): rois [B,n,4], count_dev int32 [B]
 * (nullable: n RoIs in every image) -> out_rois [B,n,4], out_level int32 [B,n], out_perm int64 [B,n] (rows counted INSIDE the
 * image), out_counts int32 [B, max_level-min_level+1].  With cnt_b = min(count_dev[b], n), image b's rows [0, cnt_b) of
 * out_rois / out_level / out_perm and out_counts[b, :] are what odet_assign_levels writes for image b alone, bit for bit;
 * rows >= cnt_b are not written; out_counts[b, :] is always written (zeros for an empty image).  No host read, no memset
 * (n == 0 apart: one hipMemsetAsync of the B*L counts), no atomics: graph-capturable.
 * Errors, before any HIP call: ODET_E_INVALID (null pointer, B < 1, n < 0, bad levels), ODET_E_LIMIT (B > ODET_ASSIGN_MAX_BATCH,
 * n > ODET_ASSIGN_MAX_ROIS). */
int odet_assign_levels_images(const float* rois, int B, int n, const int32_t* count_dev, int min_level,
                              int max_level, float* out_rois, int32_t* out_level, int64_t* out_perm,
                              int32_t* out_counts, odet_stream_t stream);

/* ---- RoI feature extraction ---------------------------------------------------------- */

#define ODET_ROI_NORM_STRIDE 0   /* model/roi_pooling.py:63-74: (roi/stride)/(dim-1) */
#define ODET_ROI_NORM_IMAGE 1    /* model/roi_pooling.py:25-35: roi/image_size (FPN) */
#define ODET_ROI_NORM_TP_ALIGN 2 /* model/roi_pooling.py:93-137,174-177: tensorpack RoIAlign */
#define ODET_ROI_NORM_TP_ALIGN_NOPAD 3 /* same with pad_border=False (roi_pooling.py:93,97) */
#define ODET_ROI_POOL_NONE 0     /* crop P x P            (roi_pooling.py:85-90) */
#define ODET_ROI_POOL_MAX2 1     /* crop 2P x 2P + 2x2 max (roi_pooling.py:36-42,75-84) */
#define ODET_ROI_POOL_AVG2 2     /* crop 2P x 2P + 2x2 avg (roi_pooling.py:149-154) */

typedef struct {
  const float* data; /* device NHWC [1,H,W,C] */
  int32_t H, W;
  float stride; /* used by NORM_STRIDE / NORM_TP_ALIGN */
} odet_level_t;

/* tf.image.crop_and_resize (bilinear, extrapolation 0) + optional 2x2 pool, fused, over up
 * to ODET_MAX_LEVELS feature maps in one launch.  levels: host array; roi_level: device
 * int32 [n] index into levels for each RoI (nullable = all 0); count_dev (nullable)
 * overrides n.  C % 4 == 0.  out [n,P,P,C]. */
int odet_roi_pool(const odet_level_t* levels, int num_levels, int C, const float* rois,
                  const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode,
                  int image_h, int image_w, int pool_size, int pool_mode, float* out,
                  odet_stream_t stream);

/* odet_roi_pool with HIP events attached to the dispatch itself (hipExtLaunchKernel start/stop
 * events, created with odet_prof_event_create): the kernel's own begin / end timestamps, for
 * bench.py's roofline figure.  odet_prof_event_elapsed_ms host-syncs on the stop event. */
int odet_roi_pool_timed(const odet_level_t* levels, int num_levels, int C, const float* rois,
                        const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode,
                        int image_h, int image_w, int pool_size, int pool_mode, float* out,
                        odet_stream_t stream, void* start_event, void* stop_event);
int odet_prof_event_create(void** ev);
/* Measurement infrastructure for bench.py's roofline object (no stage of the reference; csrc/calib.hip): a kernel
 * that only moves bytes -- reads read_bytes of src once (1 KB rows, XCD x reads the x-th eighth) and writes write_bytes
 * of dst with the RoI kernel's store instruction, interleaved at that byte ratio.  Timed with the optional events
 * (nullable), it is the time this box's memory system needs for the RoI launch's read : write mix. */
int odet_calib_stream_mix(const void* src, unsigned long long read_bytes, void* dst, unsigned long long write_bytes,
                          odet_stream_t stream, void* start_event, void* stop_event);
/* Counter calibration (measurement infrastructure): reads (an odd number of) 64 * bytes_per_lane-byte rows of src, `bytes`
 * in all, exactly once with 8 or 16 bytes per lane in a permuted row order -- a known byte count in the access shape of
 * the float16 / float32 RoI kernels, against which FETCH_SIZE's gfx950 factor is measured in the same profiler pass
 * (kernel names k_calib_read<8> / k_calib_read<16>).  Returns the rows read through *sink only in name (never written). */
int odet_calib_read_rows(const void* src, unsigned long long bytes, int bytes_per_lane, void* sink, odet_stream_t stream);
int odet_prof_event_destroy(void* ev);
int odet_prof_event_elapsed_ms(void* start, void* stop, float* ms);

/* Spatial processing order for odet_roi_pool_ordered: out_order int32 [n] = the RoI rows sorted by
 * (level, column strip of 1/8 of the image by the box centre's x, bin of 1/32 of the image by its y --
 * counted downwards on even strips and upwards on odd ones, a serpentine --, then y centre, x centre, row)
 * (padded rows >= count last).  Native addition (no reference counterpart): output row r still holds
 * RoI r, only the order in which workgroups pick RoIs changes, so that the chunk of RoIs one XCD processes
 * taps a window one strip wide of one pyramid level: a working set that slides through the XCD's L2 and
 * still fits when two or three launches share it.  The fused order of odet_fpn_proposals visits the same
 * (level, strip, bin) sequence, in arbitrary order inside a bin.  n <= 8192. */
int odet_roi_order(const float* rois, const int32_t* roi_level, int n, const int32_t* count_dev,
                   int image_h, int image_w, int32_t* out_order, odet_stream_t stream);
/* odet_roi_pool processing the RoIs in `order` (nullable = index order); start/stop events nullable
 * (see odet_roi_pool_timed). */
int odet_roi_pool_ordered(const odet_level_t* levels, int num_levels, int C, const float* rois,
                          const int32_t* roi_level, int n, const int32_t* count_dev,
                          const int32_t* order, int norm_mode, int image_h, int image_w,
                          int pool_size, int pool_mode, float* out, odet_stream_t stream,
                          void* start_event, void* stop_event);

/* odet_roi_pool_ordered for float16 feature maps (BASELINE config 5): levels[i].data points at NHWC
 * float16, out is float16 [n,P,P,C]; boxes stay float32, taps are widened to float32, lerped and pooled in
 * the same operation order, and rounded to nearest-even on the store.  Pooled (max / avg) un-padded modes
 * with pool_size <= 8. */
int odet_roi_pool_f16(const odet_level_t* levels, int num_levels, int C, const float* rois,
                      const int32_t* roi_level, int n, const int32_t* count_dev, const int32_t* order,
                      int norm_mode, int image_h, int image_w, int pool_size, int pool_mode, void* out,
                      odet_stream_t stream);
/* the same launch with HIP events attached to the dispatch (see odet_roi_pool_timed) */
int odet_roi_pool_f16_timed(const odet_level_t* levels, int num_levels, int C, const float* rois,
                            const int32_t* roi_level, int n, const int32_t* count_dev,
                            const int32_t* order, int norm_mode, int image_h, int image_w, int pool_size,
                            int pool_mode, void* out, odet_stream_t stream, void* start_event,
                            void* stop_event);

/* ---- detection post-processing ------------------------------------------------------- */

#define ODET_POSTOPS_MAX_ROIS 4096
#define ODET_POSTOPS_MAX_CANDIDATES 8192 /* (num_classes-1) * max_per_class */
size_t odet_post_ops_workspace_bytes(int num_classes, int max_per_class);
/* model/prediction.py:103-163 post_ops_prediction in ONE launch: a workgroup per class (filter, decode, clip,
 * sort, exact NMS); the last class workgroup of an image to finish merges the lists (concatenation, top-k) -- no
 * second launch, no host sync.  scores [R,Ccls] softmax, deltas [R,Ccls,4] (16-byte aligned), rois [R,4]
 * (count_dev overrides R).
 * Loops classes 1..num_classes-1 (num_classes <= Ccls).  means/stds host [4].
 * Outputs (capacity max_per_image): out_boxes [.,4], out_labels int32, out_scores in
 * (score desc, class asc, NMS order) order, out_count device int32[1]
 * (0 == the reference returns (None, None, None)). */
int odet_post_ops(const float* scores, const float* deltas, const float* rois, int R,
                  const int32_t* count_dev, int Ccls, int num_classes, int image_h, int image_w,
                  const float* means, const float* stds, int max_per_class, int max_per_image,
                  float nms_iou_threshold, float score_threshold, float min_edge,
                  float* out_boxes, int32_t* out_labels, float* out_scores, int32_t* out_count,
                  void* workspace, size_t workspace_bytes, odet_stream_t stream);

/* odet_post_ops that also writes the fixed-size detection record of odet_pack_detections
 * (out_record float32 [max_per_image*6 + 1]) from the same merge launch. */
int odet_post_ops_record(const float* scores, const float* deltas, const float* rois, int R,
                         const int32_t* count_dev, int Ccls, int num_classes, int image_h,
                         int image_w, const float* means, const float* stds, int max_per_class,
                         int max_per_image, float nms_iou_threshold, float score_threshold,
                         float min_edge, float* out_boxes, int32_t* out_labels, float* out_scores,
                         int32_t* out_count, float* out_record, void* workspace,
                         size_t workspace_bytes, odet_stream_t stream);

/* evaluation/pascal_eval_files_utils.py:76-106 (the mAP-producing per-image loop; scripts/eval_coco.py:117-164
 * has the same front end but a different per-image cap, see odet_eval_detect_topk) on the outputs of im_detect (model/fpn/base_fpn_model.py:364-390,
 * model/faster_rcnn/base_faster_rcnn_model.py:279-306): rois (resized-image pixels) are divided by
 * img_scale, then per class 1..num_classes-1: score > score_threshold -> decode -> clip to the RAW
 * image (raw_h, raw_w) with the min_size edge filter -> NMS(max_per_class, nms_iou_threshold); then
 * the per-image cap: when more than max_per_image detections survive, those with score >= the
 * max_per_image-th best score stay (ties all stay; max_per_image <= 0 disables the cap).
 * Outputs in the order of the reference's all_boxes lists (class ascending, NMS order inside a
 * class), capacity (num_classes-1)*max_per_class rows; out_count device int32[1].
 * Workspace: odet_post_ops_workspace_bytes. */
int odet_eval_detect(const float* scores, const float* deltas, const float* rois, int R,
                     const int32_t* count_dev, int Ccls, int num_classes, float img_scale,
                     float raw_h, float raw_w, const float* means, const float* stds,
                     int max_per_class, int max_per_image, float nms_iou_threshold,
                     float score_threshold, float min_size, float* out_boxes, int32_t* out_labels,
                     float* out_scores, int32_t* out_count, void* workspace,
                     size_t workspace_bytes, odet_stream_t stream);

/* scripts/eval_coco.py:117-164 (the COCO per-image loop): the front end of odet_eval_detect (rois / img_scale,
 * score > score_threshold, decode, clip to the raw image with the min_size filter, per-class NMS with max_per_class),
 * then the cap of :160, tf.nn.top_k(k = min(max_per_image, n)): exactly that many detections stay, ordered by (score
 * desc, concatenation position asc) -- the merge of odet_post_ops.  Ties at the k-th score are cut in position order
 * (odet_eval_detect keeps them all, the PASCAL rule).  Same arguments, capacity and workspace as odet_eval_detect;
 * out_count 0 when no class survives (the reference would raise at its tf.concat of an empty list). */
int odet_eval_detect_topk(const float* scores, const float* deltas, const float* rois, int R,
                          const int32_t* count_dev, int Ccls, int num_classes, float img_scale,
                          float raw_h, float raw_w, const float* means, const float* stds,
                          int max_per_class, int max_per_image, float nms_iou_threshold,
                          float score_threshold, float min_size, float* out_boxes, int32_t* out_labels,
                          float* out_scores, int32_t* out_count, void* workspace,
                          size_t workspace_bytes, odet_stream_t stream);

/* ---- COCO bbox evaluation (pycocotools COCOeval, iouType 'bbox', default Params) --------- */

/* scripts/eval_coco.py:65-73 eval_by_cocotools runs pycocotools' COCOeval.evaluate / accumulate over the result records.
 * Three launches restate it in float64; the host (evaluation/coco_eval.py) packs the ground truth and the results into
 * segments = (category, image) pairs that hold GT or detections, ordered (category asc, image id asc); inside a segment
 * GT keep annotation-file order and detections record order.  Boxes are xywh float64.  Parameters are fixed to
 * Params.setDetParams: 10 IoU thresholds, 4 area ranges, maxDets (1, 10, 100), 101 recall thresholds, useCats = 1. */
#define ODET_COCO_MAX_SEG_DETS 4096      /* detections of one segment before the maxDets[-1] = 100 truncation */
#define ODET_COCO_MAX_SEG_GT 1024        /* ground-truth boxes of one segment */
#define ODET_COCO_MAX_ENTRIES (1 << 24)  /* kept detections (at most 100 per segment) over all segments */
#define ODET_COCO_KEEP 100               /* maxDets[-1] */
#define ODET_COCO_T 10                   /* IoU thresholds */
#define ODET_COCO_A 4                    /* area ranges */
#define ODET_COCO_M 3                    /* maxDets */
#define ODET_COCO_R 101                  /* recall thresholds */

/* bytes of the workspace of odet_coco_order for num_entries kept detections */
size_t odet_coco_eval_workspace_bytes(int num_entries);

/* COCOeval.computeIoU (maskApi.c bbIou) + COCOeval.evaluateImg(maxDet = 100) for all 4 area ranges x 10 IoU
 * thresholds, one workgroup per segment.  Device CSR offsets int32 [S+1]: seg_gt_off, seg_dt_off and seg_entry_off
 * (entry_off[s+1] - entry_off[s] = min(detections, 100)).  gt_box [Ng,4], gt_area [Ng] (the annotation's area field),
 * gt_crowd uint8 [Ng] (ignore = iscrowd, as _prepare sets it), dt_box [Nd,4], dt_score [Nd].  Host: iou_thrs double[10],
 * area_rng double[8] (lo, hi pairs, inclusive).  max_seg_dets / max_seg_gt: the largest segment counts (they size the
 * LDS; a segment above them is skipped).  Outputs per kept detection e (segment order, then stable score desc):
 * out_score [E] double, out_matched / out_ignored uint64 [E] (bit a*10 + t: dtMatches != 0, dtIgnore), out_rank int32 [E]
 * (position in its segment); out_npig int32 [S,4] (GT with gtIgnore == 0 per area range).  Scores are ranked by an
 * order-keeping key with the index as tie-break, a total order on any values: -0.0 equals 0.0, and a NaN score ranks
 * after every number (where numpy's argsort of -score puts it), NaNs in input order.  (evaluation/coco_eval.py rejects
 * NaN before packing; a NaN box gives NaN IoUs, which never fault.)  Errors: ODET_E_LIMIT above the limits, before any
 * launch. */
int odet_coco_match(int num_segments, const int32_t* seg_gt_off, const int32_t* seg_dt_off,
                    const int32_t* seg_entry_off, const double* gt_box, const double* gt_area,
                    const uint8_t* gt_crowd, const double* dt_box, const double* dt_score,
                    const double* iou_thrs, const double* area_rng, int max_seg_dets, int max_seg_gt,
                    int num_entries, double* out_score, uint64_t* out_matched, uint64_t* out_ignored,
                    int32_t* out_rank, int32_t* out_npig, odet_stream_t stream);

/* COCOeval.accumulate's np.argsort(-dtScores, kind='mergesort') over each category's concatenation: the
 * kept detections sorted by (category asc, score desc, entry index asc) -- stable LSD radix passes over an order-keeping
 * 64-bit score key (-0.0 equals 0.0, NaN after every number; the key of odet_coco_match) and the category.
 * cat_entry_off: device int32 [K+1] (entries of category k are [off[k], off[k+1])).  out_order int32 [E]: entry indices
 * in sorted order.  Workspace: odet_coco_eval_workspace_bytes. */
int odet_coco_order(int num_entries, int num_cats, const int32_t* cat_entry_off, const double* entry_score,
                    int32_t* out_order, void* workspace, size_t workspace_bytes, odet_stream_t stream);

/* COCOeval.accumulate in float64, one workgroup per (IoU threshold, area range x maxDets, category):
 * cumulative TP / FP counts over the sorted entries with rank < maxDets[m] (ignored entries stay in the index space),
 * rc = tp / npig, pr = tp / ((fp + tp) + spacing(1)), its suffix maximum, searchsorted(rc, recThrs, 'left').
 * cat_seg_off: device int32 [K+1] (segments of category k), npig from odet_coco_match, rec_thrs: host double[101],
 * max_dets: host int[3].  Outputs (device float64): precision and scores [10,101,K,4,3], recall [10,K,4,3]; -1 where the
 * category has no segment or npig == 0. */
int odet_coco_accumulate(int num_cats, const int32_t* cat_seg_off, const int32_t* cat_entry_off,
                         const int32_t* npig, const int32_t* order, const double* entry_score,
                         const uint64_t* entry_matched, const uint64_t* entry_ignored,
                         const int32_t* entry_rank, const double* rec_thrs, const int* max_dets,
                         double* out_precision, double* out_recall, double* out_scores,
                         odet_stream_t stream);

/* ---- PASCAL VOC evaluation and the accuracy gate's paired bootstrap ---------------------- */

/* evaluation/detectron_pascal_evaluation_utils.py voc_eval (:86-222) / voc_ap (:54-83), which scripts/eval_pascal.py:74-96
 * runs once per class, in float64 and in the reference's operation order.  The host (evaluation/voc_eval_gpu.py) packs
 * ground truth and detections into segments = (class, image) pairs that hold either, ordered (class asc, image asc);
 * inside a segment ground truth keeps annotation order and detections the order of the caller's arrays.  Boxes are
 * x1 y1 x2 y2 float64 (inclusive pixels: the + 1 widths of :190-197).  An entry is a detection; entries of segment s are
 * [seg_dt_off[s], seg_dt_off[s+1]).  The score order of a class is odet_coco_order's (class asc, score desc, entry index
 * asc), which on these entries equals np.argsort(-confidence, kind='stable') over the class's detections in image order
 * (:169; the stable kind is what evaluation/pascal_eval.py uses, numpy's default leaves equal scores undefined). */
#define ODET_VOC_MAX_SEG_DETS 4096       /* detections of one segment */
#define ODET_VOC_MAX_SEG_GT 1024         /* ground-truth boxes of one segment */
#define ODET_VOC_MAX_ENTRIES (1 << 24)   /* detections over all segments (ODET_COCO_MAX_ENTRIES: the order is shared) */
#define ODET_VOC_R 11                    /* recall thresholds of the 11-point metric */
#define ODET_VOC_IGNORED 0               /* entry flags: matched a `difficult` box, neither tp nor fp (:204) */
#define ODET_VOC_TP 1                    /* :206 */
#define ODET_VOC_FP 2                    /* :209, :211 */
#define ODET_VOC_AP_07 0                 /* voc_ap(use_07_metric=True), :58-66 */
#define ODET_VOC_AP_AREA 1               /* voc_ap(use_07_metric=False), :67-82 */

/* bytes of the workspace of odet_voc_accumulate (num_resamples = 1, metric = ODET_VOC_AP_AREA) and odet_voc_bootstrap:
 * the terms of the area metric's sum, (num_entries + num_classes) doubles per resample; 0 for the 11-point metric */
size_t odet_voc_eval_workspace_bytes(int num_entries, int num_classes, int num_resamples, int metric);

/* :173-211 for all segments at once, one wave per segment.  A segment's detections are taken in (score desc, input
 * position asc) order -- the order in which the global walk of :177 meets this image's detections -- with the score key
 * of odet_coco_match (-0.0 equals 0.0, NaN last).  Per detection: overlaps (:186-199) with every ground-truth box of the
 * segment, ovmax / jmax = np.max / np.argmax (first maximum; a NaN overlap makes ovmax NaN, so the detection is a false
 * positive), ovmax > ovthresh strictly (:203), a `difficult` match is ODET_VOC_IGNORED and leaves the box free (:204),
 * the first match of a box ODET_VOC_TP (:205-207), a later one ODET_VOC_FP (:209), no ground truth ODET_VOC_FP (:211).
 * Device: seg_gt_off / seg_dt_off int32 [S+1], gt_box [num_gt,4], gt_difficult uint8 [num_gt], dt_box [E,4], dt_score
 * [E].  max_seg_dets / max_seg_gt: the largest segment counts (they size the LDS; a segment above them is skipped).
 * Outputs, per entry in its segment's sorted order: out_score double [E], out_flag uint8 [E]; per segment out_npos int32
 * [S] (boxes that are not difficult, :145).  Errors: ODET_E_LIMIT above the limits, before any launch. */
int odet_voc_match(int num_segments, const int32_t* seg_gt_off, const int32_t* seg_dt_off, const double* gt_box,
                   const uint8_t* gt_difficult, const double* dt_box, const double* dt_score, double ovthresh,
                   int max_seg_dets, int max_seg_gt, int num_gt, int num_entries, double* out_score,
                   uint8_t* out_flag, int32_t* out_npos, odet_stream_t stream);

/* :213-220 and voc_ap (:54-83), one workgroup per class over the entries in odet_coco_order's order: tp / fp = cumulative
 * counts (block prefix sums, a carry between chunks), rec = tp / npos (tp * 0 when npos == 0, as
 * evaluation/pascal_eval.py has it; the reference divides by zero there), prec = tp / max(tp + fp, eps); ap07: ap = ap +
 * p / 11. over rec_thrs (host double[11] = np.arange(0., 1.1, 0.1)), p = max(prec[rec >= t]) or 0; ap_area: the envelope
 * and np.sum((mrec[i+1] - mrec[i]) * mpre[i+1]) in numpy's own order of additions (add.reduce: pieces of 8192 elements,
 * each summed pairwise with eight running sums per block of up to 128), so that it equals the host value too.  Device: cls_seg_off / cls_entry_off int32 [K+1], seg_npos from odet_voc_match, order int32 [E],
 * entry_flag [E], entry_image int32 [E] (image index of every entry).  Outputs: out_rec / out_prec double [E] in sorted
 * order, out_ap07 / out_ap_area double [K], out_npos int64 [K], and the inputs of odet_voc_bootstrap: out_sorted_flag uint8
 * [E], out_sorted_image int32 [E] (flag and image of the entries in sorted order).  Workspace (the terms of the area
 * sum): odet_voc_eval_workspace_bytes(E, K, 1, ODET_VOC_AP_AREA). */
int odet_voc_accumulate(int num_classes, int num_segments, int num_entries, const int32_t* cls_seg_off,
                        const int32_t* cls_entry_off, const int32_t* seg_npos, const int32_t* order,
                        const uint8_t* entry_flag, const int32_t* entry_image, const double* rec_thrs,
                        double* out_rec, double* out_prec, double* out_ap07, double* out_ap_area, int64_t* out_npos,
                        uint8_t* out_sorted_flag, int32_t* out_sorted_image, void* workspace,
                        size_t workspace_bytes, odet_stream_t stream);

/* evaluation/precision_gate.py _map_weighted (the paired bootstrap over images of the float16 accuracy gate) for every
 * resample in one launch, grid = (resample, class): counts int32 [B, num_images] (device) says how often resample b drew
 * image i; npos = sum(counts * npos of the image), every entry weighs counts[b, its image], tp / fp = cumulative weighted
 * counts where every entry that is not ODET_VOC_TP is a false positive (_map_weighted's ~tp), rec, prec and the AP of
 * `metric` as in odet_voc_accumulate.  All sums are integers, so the results do not depend on their order.  seg_image:
 * int32 [S] image index of every segment.  Outputs: out_ap double [B, K] (0 where npos == 0: the host leaves such a class
 * out of the mean), out_npos int64 [B, K].  Workspace: odet_voc_eval_workspace_bytes(E, K, B, metric) (none for the
 * 11-point metric). */
int odet_voc_bootstrap(int num_resamples, int num_classes, int num_images, int num_segments, int num_entries,
                       const int32_t* cls_seg_off, const int32_t* cls_entry_off, const int32_t* seg_image,
                       const int32_t* seg_npos, const uint8_t* sorted_flag, const int32_t* sorted_image,
                       const int32_t* counts, const double* rec_thrs, int metric, double* out_ap, int64_t* out_npos,
                       void* workspace, size_t workspace_bytes, odet_stream_t stream);

/* ---- eval input front end ------------------------------------------------------------- */

#define ODET_PREP_VOC 0
#define ODET_PREP_COCO 1
#define ODET_PREP_CAFFE 0
#define ODET_PREP_TF 1
#define ODET_PREP_MAX_BATCH 64       /* the detectors' max_batch limit */
#define ODET_PREP_MAX_RAW_W 4096     /* raw pixels per row (two staged rows: 96 KB of LDS) */
#define ODET_PREP_MAX_RAW_H 65536
#define ODET_PREP_MAX_OUT 8192       /* output H and W */
/* The reference's eval preprocessing, decoded uint8 HWC images -> one NHWC batch out [B, H, W, 3] (float32, or float16
 * when f16 = 1: the float32 result rounded once to nearest even), in one launch; no host sync, no host->device copy.
 * Host arrays [B]: images (device pointers), raw_h, raw_w, row_pitch (bytes between rows, >= 3 * raw_w); means: host
 * double[3] in BGR order (may be NULL for preprocessing = ODET_PREP_TF).  out must be 16-byte aligned.  H x W is the
 * caller's (both loaders truncate scale * size; the two rules differ, see preprocess.py).
 *  pipeline ODET_PREP_VOC = dataset/eval_pascal_tf_dataset.py:32-52 (_map_from_cv2): BGR input; caffe:
 *    float32(float64(u) - means[c]) (:37, numpy promotes float32 -= float64[3]); tf: ((float32(u) / 255) * 2) - 1 (:39);
 *    cv2.resize INTER_LINEAR on float32 (:48; INTER_AREA when both axes shrink by exactly 2, as OpenCV switches);
 *    rgb = 1 flips the result to RGB (:50-51).
 *  pipeline ODET_PREP_COCO = dataset/utils/tf_dataset_utils.py:128-155 (preprocessing_eval_func): RGB input; caffe
 *    (:55-71): reversed to BGR, float32(u) - float32(means[c]); tf (:74-80): ((float32(u) * float32(1/255)) * 2) - 1, RGB;
 *    tf.image.resize_bilinear of TF 1.x (align_corners=False, the index math of odet_fpn_topdown_merge).  rgb must be 0.
 * B == 0 is a no-op.  Errors: ODET_E_INVALID (null pointer, bad size / mode, misaligned out), ODET_E_LIMIT (B > 64,
 * sizes above the limits above). */
int odet_preprocess_images(const void* const* images, const int* raw_h, const int* raw_w, const long long* row_pitch,
                           int B, int H, int W, int pipeline, int preprocessing, int rgb, const double* means, void* out,
                           int f16, odet_stream_t stream);

/* ---- training input front end (added within 103) -------------------------------------- */

#define ODET_PREP_MAX_BOXES 1024     /* ground-truth boxes per image (the fused targets' limit) */
/* The reference's TRAINING input stage for a batch: decoded uint8 RGB HWC images + normalised boxes -> exactly what
 * odet_anchor_target / odet_proposal_target take, in ONE launch (H row workgroups per image as odet_preprocess_images, plus
 * one workgroup per image for its boxes); no allocation, no host read.  The reference parts:
 *   image_argument_with_imgaug with the default iaa.Fliplr(0.5)   dataset/utils/tf_dataset_utils.py:10-52
 *   preprocessing_training_func                                   dataset/utils/tf_dataset_utils.py:55-80, 83-126
 *     (called from dataset/pascal_tf_dataset_generator.py:83-98 and dataset/coco_tf_dataset_generator.py:187-200)
 *   the column swap of train_one_epoch                            scripts/train.py:84-96
 * images, raw_h, raw_w, row_pitch, H, W, preprocessing, means, out, f16: as odet_preprocess_images with
 * pipeline = ODET_PREP_COCO (the same float32 rule, :109-117), whose limits and argument errors apply.
 *
 * Flip.  augment = 1 and flip == NULL: image b is mirrored iff w0 >> 31 == 1, w0 the first word of
 * philox((0, image_id, 5, 0), (seed low word, seed high word)), image_id = first_image_id + b (mod 2^32): stream 5 of the
 * sampling rule under "training targets" below, a function of (seed, image_id) alone.  flip (HOST int[B], each 0 or 1)
 * overrides the rule (tests, replaying a recorded epoch).  augment = 0 (the reference's argument=False): no flip, no
 * truncation.  The decision is taken on the HOST and travels in the kernel's parameters: the call captures into a graph,
 * and a replay repeats the flags of the capturing call.  flipped (HOST int[B], nullable) receives them.
 * Image.  A mirrored image is the raw uint8 image with its columns reversed (image[:, ::-1]), BEFORE normalisation and
 * resize: TF 1.x resize_bilinear is not mirror-symmetric, the other order gives other pixels.
 * Boxes.  boxes_yxyx: device float32 [sum G, 4] rows (ymin, xmin, ymax, xmax) in [0, 1] units of the raw h x w image, finite
 * (the reference's int() raises on anything else; here such a value is clamped to +-2^62 before the truncation); gt_offsets:
 * HOST int [B + 1], image b owns rows gt_offsets[b] .. gt_offsets[b + 1]; G = 0 is legal.  With augment = 1, EVERY image,
 * mirrored or not (:30-33, :47-52):
 *   iy1 = int(float64(ymin) * h), likewise ix1 (* w), iy2, ix2: a float64 product truncated toward zero (the reference's
 *     numpy promotes float32 scalar * int to float64: float32(0.7) * 10 truncates to 6, not to 7);
 *   ix1 > ix2 are swapped, likewise y (imgaug's BoundingBox constructor);
 *   mirrored: (ix1, ix2) -> (w - ix2, w - ix1) -- imgaug's x' = width - x on both corners, the rule of imgaug 0.2.8 and
 *     later.  UNPINNED: imgaug was not at hand when this was written, the rule is taken from its source as remembered; there
 *     is no switch for the older width - 1 - x;
 *   float64(i) / float64(size), clipped to [0, 1], rounded once to float32.
 * With augment = 0 the input values are taken as they are.  Then, in float32: y * float32(H - 1), x * float32(W - 1)
 * (:119-124), written x first: gt_boxes_xyxy device [sum G, 4] rows (xmin, ymin, xmax, ymax) (train.py:89-93).
 * gt_offsets_dev: device int32 [B + 1], written by the kernel from its parameters (no separate copy).  Labels need no
 * kernel (tf.to_int32, train.py:96).
 * B == 0 is a no-op.  Errors: those of odet_preprocess_images; ODET_E_INVALID for augment outside {0, 1}, flip given with
 * augment = 0 or holding anything but 0 / 1, offsets that do not start at 0 or that decrease, a null pointer;
 * ODET_E_LIMIT for an image with more than ODET_PREP_MAX_BOXES boxes (refused on the host: the offsets are host values). */
int odet_preprocess_train(const void* const* images, const int* raw_h, const int* raw_w, const long long* row_pitch,
                          int B, int H, int W, int preprocessing, const double* means,
                          const float* boxes_yxyx /* device [sum G,4] */, const int* gt_offsets /* HOST [B+1] */,
                          int augment, const int* flip /* HOST [B], nullable */, uint64_t seed, uint32_t first_image_id,
                          void* out, int f16, float* gt_boxes_xyxy /* device [sum G,4] */,
                          int32_t* gt_offsets_dev /* device [B+1] */, int* flipped /* HOST [B], out, nullable */,
                          odet_stream_t stream);

/* ---- FPN neck: top-down merge -------------------------------------- */

/* model/fpn/resnet_fpn.py:385-398 (ResnetFpnNeck.call): P_k = Add([resize_bilinear(P_{k+1},
 * size(C_k)) * 0.5, lateral(C_k) * 0.5]) with tf.image.resize_bilinear of TF 1.x
 * (align_corners=False: src = dst * in/out, lo = floor, hi = min(lo + 1, in - 1)) in one
 * launch.  NHWC: top [B,h,w,C], lateral and out [B,H,W,C]; f16 != 0: float16 maps (float32
 * arithmetic, one rounding at the end), C % 8 == 0; otherwise float32, C % 4 == 0. */
int odet_fpn_topdown_merge(const void* top, int h, int w, const void* lateral, int H, int W,
                           int B, int C, void* out, int f16, odet_stream_t stream);

/* The BACKWARD of that merge, float32 (added within 103): model/fpn/resnet_fpn.py:385-398 read in reverse -- the transpose
 * of up = resize_bilinear(top, (H, W)) as a gather per coarse pixel, with the other summands of the coarse map's gradient
 * folded in:
 *   d_top[b,Y,X,c] = out_scale * ( base[b,Y,X,c] + sub[b,Y/2,X/2,c] (only where Y and X are even) + S[b,Y,X,c] )
 * NHWC: fine [B,H,W,C] (the gradient with respect to `up`: the caller has applied the merge's 0.5), base and d_top
 * [B,h,w,C], sub [B,ceil(h/2),ceil(w/2),C] (the gradient of the stride-2 subsample p5[:, :, ::2, ::2], i.e. of P6).  fine,
 * base and sub are each nullable; an absent term is skipped, not added as a zero (without fine there is no S term and H, W
 * only have to be positive).  The terms are added left to right as written; the multiply by out_scale is one float32 multiply.
 * S, the sum of taps: for every fine pixel (y, x) in ascending y, then ascending x, with the forward's own float32
 * expressions ys = (float)h / (float)H, fy = (float)y * ys, y0 = floor(fy), y1 = min(y0 + 1, h - 1), yl = fy - y0 (likewise
 * x), the taps in the order TL (y0,x0), TR (y0,x1), BL (y1,x0), BR (y1,x1); each tap that lands on (Y, X) adds
 * (g * wy) * wx, g = fine[b,y,x,c], wy = 1 - yl (top row) or yl (bottom row), wx = 1 - xl (left) or xl (right): two float32
 * multiplies and a separate add, no FMA, onto an accumulator that starts at +0.  A clamped edge (y1 == y0 or x1 == x0)
 * gives two separate additions, in that order.  It is the order of a serial loop over (y, x) that accumulates into the
 * coarse map (TF's ResizeBilinearGrad on the CPU), restated in tests/neck_grad_np.py.  Taps of weight exactly zero are
 * skipped where that leaves the bits of finite data alone; non-finite gradients are outside the contract.
 * No atomics, no workspace, no allocation, no host read (graph-capturable); every element of d_top is written exactly once
 * (a coarse pixel no fine pixel taps -- a downscale -- gets S = +0); the result depends on the data and the shapes only.  Any
 * h, w, H, W combination the forward takes.  C % 4 == 0.  B == 0 is a no-op.
 * Errors, all before any HIP call: ODET_E_INVALID (null d_top; fine, base and sub all null; h, w, H or W <= 0; B < 0; C no
 * positive multiple of 4; a pointer not 16-byte aligned). */
int odet_fpn_topdown_backward_f32(const float* fine, int H, int W, const float* base, const float* sub, float out_scale,
                                  float* d_top, int h, int w, int B, int C, odet_stream_t stream);

/* ---- ResNet bottleneck backward: the two elementwise launches (added within 103) ------------------------------------------ */

/* The stride-s subsample of an NHWC float32 map, model/fpn/resnet_fpn.py:154-205 (Conv2D(1x1, strides=2, 'valid') on the first
 * block of conv3..conv5 reads every second pixel):
 *   out[b,i,j,c] = x[b, i*stride, j*stride, c],  x [B,H,W,C], out [B,Ho,Wo,C], Ho = (H-1)/stride + 1, Wo = (W-1)/stride + 1.
 * The forward convolution reads the map strided and never writes this; the Dense weight gradient of such a layer needs its input
 * as contiguous [rows, cin].  stride is 1 (a copy) or 2.  A copy of bits: no arithmetic.  No workspace, no host read
 * (graph-capturable); every element of out is written exactly once.  B == 0 is a no-op.
 * Errors, all before any HIP call: ODET_E_INVALID (a null pointer; H or W <= 0; B < 0; C no positive multiple of 4; a stride other
 * than 1 or 2; a pointer not 16-byte aligned). */
int odet_stride_gather_f32(const float* x, int B, int H, int W, int C, int stride, float* out, odet_stream_t stream);

/* The gradient with respect to a bottleneck block's INPUT (model/fpn/resnet_fpn.py:154-205 in reverse: Add([shortcut, x]) +
 * Activation('relu') at the block's end, the two branches that read the block's input at its start), dx [B,H,W,C] NHWC float32, in
 * one of two forms chosen by which pointers are null:
 *   identity shortcut (dy, y, d1 non-null [B,H,W,C]; d2 null; stride 1):
 *       dx[i] = (y[i] > 0 ? dy[i] : +0) + d1[i]
 *     y: the block's output (after the final ReLU), dy: its gradient -- the first term is the shortcut's gradient through that ReLU
 *     (strictly greater: y == +0 or -0 closes the gate) --, d1: the input gradient of the block's first convolution.
 *   convolutional shortcut (dy and y null; d1 and the nullable d2 [B,Ho,Wo,C], Ho = (H-1)/stride + 1, Wo likewise):
 *       dx[b,Y,X,c] = d1[b,Y/stride,X/stride,c] + d2[b,Y/stride,X/stride,c]   where Y % stride == 0 and X % stride == 0,
 *                     +0                                                      elsewhere
 *     the transpose of odet_stride_gather_f32 applied to the sum of the two branches' input gradients (first convolution, shortcut
 *     convolution); without d2 the one term is copied.
 * One float32 add per element (no FMA can arise), so the result is the NumPy statement's, bit for bit (tests/block_grad_np.py).
 * No atomics, no workspace, no host read (graph-capturable); every element of dx is written exactly once.  B == 0 is a no-op.
 * Errors, all before any HIP call: ODET_E_INVALID (null dx or d1; a null / non-null pattern that is neither form; H or W <= 0;
 * B < 0; C no positive multiple of 4; a stride other than 1 or 2; the identity form with stride 2; a pointer not 16-byte aligned). */
int odet_block_input_grad_f32(const float* dy, const float* y, const float* d1, const float* d2, float* dx, int B, int H, int W,
                              int C, int stride, odet_stream_t stream);

/* ---- VGG16 training graph: max-pooling and dropout backward (added within 103) ---------------------------------------------- */

/* The backward of odet_bias_relu_maxpool's float32 2x2 / stride-2 ceil-mode form -- MaxPooling2D((2,2), 2, 'same') after a ReLU
 * convolution, model/faster_rcnn/vgg16_faster_rcnn.py:307, 325 (block3_pool, block4_pool) -- as TF computes it: MaxPoolGrad, then
 * ReluGrad.  z [B,H,W,C] NHWC float32 is the convolution's raw output WITHOUT its bias (what the forward reads), bias [C],
 * dpool [B,OH,OW,C] with OH = (H+1)/2, OW = (W+1)/2, dz [B,H,W,C]:
 *   a = max(z + bias, 0)                         one float32 add, the sum the forward forms
 *   dz[b,y,x,c] = dpool[b,y>>1,x>>1,c]           if a[b,y,x,c] > 0 and (y,x) is the FIRST position of its window, in the row-major
 *                                                order (0,0),(0,1),(1,0),(1,1), that holds the window's maximum (strict '>' while
 *                                                scanning); a window whose maximum is 0 passes nothing
 *                 +0                             otherwise
 * Windows at an odd bottom or right edge hold only their taps inside the map (TF's 'same' rule pads at the end).  The windows
 * do not overlap: a gather, no atomics, no workspace, no host read (graph-capturable); every element of dz is written exactly
 * once.  Algorithmic bytes: 4 * (2 H W + OH OW) * C * B.  B == 0 is a no-op.
 * Errors, all before any HIP call: ODET_E_INVALID (a null pointer; H or W <= 0; B < 0; C no positive multiple of 4; a pointer not
 * 16-byte aligned). */
int odet_relu_maxpool2_backward_f32(const float* z, const float* bias, const float* dpool, float* dz, int B, int H, int W, int C,
                                    odet_stream_t stream);

/* tf.nn.dropout of TF r1.13 (model/faster_rcnn/vgg16_faster_rcnn.py:250-253: both dropouts of Vgg16RoiHead active in training,
 * keep_rate 0.5) on a flat float32 tensor of n elements, with the counter-based rule of "training targets" in place of TF's
 * generator.  Element e takes word e & 3 of philox((e >> 2, image_id, stream_id, 0), (seed low word, seed high word)) and
 *   u = bitcast<float>((word & 0x7fffff) | 0x3f800000) - 1        TF's Uint32ToFloat, in [0, 1)
 *   keep = floor(keep_prob + u)                                    a float32 add: 1 with probability keep_prob, else 0
 *   forward   y[e]  = (x[e] / keep_prob) * keep                    a float32 division, then the multiplication
 *   backward  dx[e] = (dy[e] * keep) / keep_prob                   the mask is recomputed from the same counters, never stored
 * keep_prob == 1 copies the input unchanged (TF returns it as it is).  Streams 0-5 belong to the samplers and the input stage; 6
 * is the dropout after fc1, 7 the one after fc2.  x == y (in place) is allowed.  Any n in [0, 2^34]; n == 0 is a no-op.  No
 * workspace, no host read (graph-capturable).
 * Errors, all before any HIP call: ODET_E_INVALID (n outside [0, 2^34]; keep_prob outside (0, 1]; a null pointer; a pointer not
 * 16-byte aligned). */
int odet_dropout_f32(const float* x, float* y, long long n, float keep_prob, uint64_t seed, uint32_t image_id, uint32_t stream_id,
                     odet_stream_t stream);
int odet_dropout_backward_f32(const float* dy, float* dx, long long n, float keep_prob, uint64_t seed, uint32_t image_id,
                              uint32_t stream_id, odet_stream_t stream);

/* ---- FPN stem training graph: the overlapping max-pooling's backward (added within 103) --------------------------------------- */

/* The backward of odet_bias_relu_maxpool's float32 3x3 / stride-2 / pad-1 floor-mode form -- conv1_relu, pool1_pad
 * (ZeroPadding2D(1)) and pool1_pool (MaxPooling2D(3, strides=2)) behind the trainable conv1_conv of the FPN extractor,
 * model/fpn/resnet_fpn.py:233-242 -- as TF computes it: MaxPoolGrad through the padding, then ReluGrad.  z [B,H,W,C] NHWC float32
 * is the convolution's raw output WITHOUT its bias (what the forward reads), bias [C], dpool [B,OH,OW,C] with OH = (H-1)/2 + 1,
 * OW = (W-1)/2 + 1, dz [B,H,W,C]:
 *   v = z + bias                                  one float32 add, the sum the forward forms; a = max(v, 0)
 *   window (p,q)                                  rows 2p-1 .. 2p+1, columns 2q-1 .. 2q+1, clipped to the map
 *   winner(p,q,c)                                 the FIRST tap of the window, in row-major order, that holds its maximum when
 *                                                 that maximum is > 0: scanning from +0 with a strict '>', so a window whose
 *                                                 maximum is 0 has no winner and a NaN tap never wins
 *   dz[b,i,j,c] = sum of dpool[b,p,q,c]           over the windows (p,q) whose winner is (i,j), in ascending (p,q) row-major
 *                                                 order, every add rounded to float32, started from the first term itself
 *                 +0                              where there is none
 * The padding taps are skipped.  In the reference a padding tap holds 0 and can win only a window whose maximum is 0; ReluGrad
 * zeroes that case (a = 0 at every real tap of such a window, and the padding has no gradient to keep), so skipping the taps and
 * passing the 0 through are the same function.  An odd row or column belongs to two window rows or columns: a pixel is in up to
 * four windows, and the order of its at most four terms is part of the contract (tests/stem_grad_np.py states it as a serial
 * loop; the result is that statement's, bit for bit).  No atomics, no arg-max tensor, no workspace, no host read
 * (graph-capturable); every element of dz is written exactly once.  Algorithmic bytes: 4 * (2 H W + OH OW) * C * B.
 * B == 0 is a no-op.
 * Errors, all before any HIP call: ODET_E_INVALID (a null pointer; H or W <= 0; B < 0; C no positive multiple of 4; a pointer not
 * 16-byte aligned; more than 2^31 - 1 workgroups of 6 window rows x (256 / min(C/4, 64) - 1) window columns x 256 channels). */
int odet_relu_maxpool3_backward_f32(const float* z, const float* bias, const float* dpool, float* dz, int B, int H, int W, int C,
                                    odet_stream_t stream);

/* ---- ResNet-C4 training graph: global average pooling, forward and backward (added within 103) ------------------------------ */

/* GlobalAveragePooling2D between the conv5 stack and the two Dense layers of the C4 RoI head,
 * model/faster_rcnn/resnet_faster_rcnn.py:167-168 (get_resnet_v1_roi_head: stack1(..., name='conv5'), then
 * layers.GlobalAveragePooling2D()), with a stated summation order.  x [rows, hw, channels] contiguous float32 -- an NHWC map [R,H,W,C] with hw = H * W --, out [rows, channels]:
 *   s = x[r,0,c];  s = s + x[r,p,c] for p = 1 .. hw-1 in that order      every add rounded to float32, started from the first pixel
 *   out[r,c] = s / (float)hw                                              itself (all pixels -0 give -0); one IEEE division
 * One lane per (row, 4 channels), the pixels walked serially with 16 loads in flight.  Algorithmic bytes: 4 * rows * (hw + 1) *
 * channels.  No atomics, no workspace, no host read (graph-capturable); every element of out is written exactly once; the result
 * is the NumPy statement's, bit for bit (tests/c4_grad_np.py).
 * Errors, all before any HIP call: ODET_E_INVALID (a null pointer; rows < 1; hw < 1; channels no positive multiple of 4; a pointer
 * not 16-byte aligned). */
int odet_global_avg_pool_f32(const float* x, int rows, int hw, int channels, float* out, odet_stream_t stream);

/* Its backward, TF's _MeanGrad (python/ops/math_grad.py: the gradient broadcast to the input's shape, then a true division by
 * the number of pooled elements): g [rows, channels], dx [rows, hw, channels],
 *   dx[r,p,c] = g[r,c] / (float)hw        for every p; one IEEE division per element
 * the transpose of the forward wherever the division is exact.  One lane per (row, 8 consecutive pixels, 4 channels): one
 * division of g per eight stores.  Same rules and errors as the forward; every element of dx is written exactly once. */
int odet_global_avg_pool_backward_f32(const float* g, int rows, int hw, int channels, float* dx, odet_stream_t stream);

/* Convolution epilogue of the dense path, in place on an NHWC activation x [npix, C]:
 * x = relu?((x + bias[C]) (+ residual[npix, C])) -- the frozen-BatchNormalization bias, the
 * bottleneck's Add([shortcut, x]) and Activation('relu') of model/fpn/resnet_fpn.py:154-205
 * (and the RpnHead's ReLU, base_fpn_model.py:393-434) in one pass.  residual may be NULL.
 * f16 != 0: float16 tensors (float32 arithmetic, one rounding), C % 8 == 0; else float32, C % 4 == 0. */
int odet_bias_act(void* x, const void* bias, const void* residual, long long npix, int C, int relu,
                  int f16, odet_stream_t stream);

/* Convolution epilogue + max-pooling in one pass (model/fpn/resnet_fpn.py:228-259 conv1 -> relu -> pool1;
 * model/faster_rcnn/vgg16_faster_rcnn.py:260-342 conv -> relu -> MaxPooling2D((2,2), 2, 'same')):
 * out[B, OH, OW, C] = maxpool_{kernel, stride, pad}(relu(x[B, H, W, C] + bias[C])), NHWC, x = the convolution
 * WITHOUT its bias.  Window taps outside the map are skipped (= zero padding after a ReLU, = TF 'same').
 * Bit-identical to the separate passes (bias and ReLU commute with the maximum).  f16: C % 8 == 0; else C % 4. */
int odet_bias_relu_maxpool(const void* x, const void* bias, void* out, int B, int H, int W, int C, int OH, int OW,
                           int kernel, int stride, int pad, int f16, odet_stream_t stream);

/* 3x3 stride-1 'same' convolution as an implicit GEMM on the matrix cores -- the RpnHead's convolution
 * (model/fpn/base_fpn_model.py:401-417, model/faster_rcnn/base_faster_rcnn_model.py:315-321): x NHWC float16
 * [batch,H,W,cin], w float16 [cout][3][3][cin] (= a channels_last torch weight), y NHWC float16 [batch,H,W,cout],
 * float32 accumulation; bias (nullable, float16 [cout]) and relu are applied before the one rounding.
 * cin % 64 == 0, cout % 64 == 0 (256-channel workgroup tiles; 128 / 64-channel tiles when cout is not a multiple of 256). */
int odet_conv3x3_f16(const void* x, const void* w, const void* bias, void* y, int batch, int H, int W,
                     int cin, int cout, int relu, odet_stream_t stream);
/* the same convolution (shared weights) over up to ODET_MAX_LEVELS maps in ONE launch -- the RpnHead over the pyramid
 * levels (base_fpn_model.py:188-200): the workgroups of the small levels fill the tail of the big ones'.  levels: host
 * array, x / y NHWC float16 [batch,H,W,cin] / [batch,H,W,cout]; list the big levels first. */
typedef struct {
  const void* x; void* y;
  int32_t H, W;
} odet_conv_level_t;
/* A stage's last convolution of VGG16 with its pooling (vgg16_faster_rcnn.py:260-342: Conv2D(3x3, 'same') + ReLU +
 * MaxPooling2D((2, 2), 2, padding='same')) in one launch: y [batch][ceil(H/2)][ceil(W/2)][cout] float16 -- the un-pooled map
 * is never written.  Same operand rules as odet_conv3x3_f16; max commutes with the rounding, so the result equals pooling
 * the rounded map. */
int odet_conv3x3_relu_pool2_f16(const void* x, const void* w, const void* bias, void* y, int batch, int H, int W,
                                int cin, int cout, odet_stream_t stream);
int odet_conv3x3_f16_levels(const odet_conv_level_t* levels, int num_levels, const void* w, const void* bias,
                            int batch, int cin, int cout, int relu, odet_stream_t stream);
/* The whole RpnHead (base_fpn_model.py:393-434, 188-200): the 3x3 convolution of every level as above, and in its
 * epilogue relu(conv + conv_b) (one float16 rounding) . w^T + b for the 2A score and 4A delta rows (w [6A][cout] float16,
 * b [6A] float16: rpn_score's rows, then rpn_bbox's), written as float32 into the concatenated arrays scores
 * [batch][N][2] / deltas [batch][N][4] (image strides in VALUES; the levels follow each other in the order given, H*W*A
 * anchors each).  levels[].y is not used: the cout-channel activation never goes to memory -- a workgroup walks the
 * channel tiles of its pixel slab and keeps the 32 float32 sums per pixel in registers (fixed order: deterministic; one
 * launch, no workspace).  cout = 256 or 512, 1 <= A <= 5. */
int odet_rpn_head_fused_f16(const odet_conv_level_t* levels, int num_levels, const void* conv_w, const void* conv_b,
                            const void* w, const void* b, int A, int batch, int cin, int cout, float* scores,
                            long long scores_image_stride, float* deltas, long long deltas_image_stride,
                            odet_stream_t stream);
/* A bottleneck block's 3x3 convolution AND its last 1x1 convolution in one launch (resnet_fpn.py:154-205 with the frozen
 * batch norms folded): y = relu( relu(conv3x3(x, w2) + b2) . w3^T + b3 + residual ), x NHWC float16 [batch,H,W,cin],
 * w2 [256][3][3][cin], b2 [256], w3 [n3][256], b3 [n3], residual (nullable) / y NHWC float16 [batch,H,W,n3]; the
 * 256-channel activation between the two is rounded to float16 once and never goes to memory.  cin % 64 == 0, the
 * 3x3 convolution has exactly 256 output channels (one workgroup holds them all), n3 % 64 == 0. */
int odet_conv3x3_conv1x1_f16(const void* x, const void* w2, const void* b2, const void* w3, const void* b3,
                             const void* residual, void* y, int batch, int H, int W, int cin, int n3, int relu,
                             odet_stream_t stream);
/* 1x1 convolutions and dense layers as the same LDS-staged GEMM on the matrix cores (the implicit-GEMM kernel with one
 * tap): y = relu?( x(:, ::stride, ::stride, :) . w^T + bias + residual ).  x NHWC float16 [batch,H,W,cin], w [cout][cin]
 * (a Conv2D 1x1 kernel, or a Dense kernel transposed), bias [cout] (nullable), residual (nullable) / y NHWC float16
 * [batch, ceil(H/stride), ceil(W/stride), cout].  Replaces, in the reference's ResNet-FPN (model/fpn/resnet_fpn.py): the
 * bottlenecks' first 1x1 convolution and their strided shortcut / first convolutions (:154-205; Conv2D(1x1, strides=2,
 * 'valid') reads every second pixel), the neck's P5 convolution (:339-384) and the RoI head's Dense layers (:292-336;
 * batch = 1, H = 1, W = rows).  cin % 64 == 0 and >= 128, cout % 64 == 0, stride 1 or 2.  The workgroup tile (256 / 128 /
 * 64 channels x 128..256 pixels) is picked per launch so that the workgroups fill whole rounds of the CUs. */
int odet_pointwise_f16(const void* x, const void* w, const void* bias, const void* residual, void* y, int batch,
                       int H, int W, int stride, int cin, int cout, int relu, odet_stream_t stream);
/* The end of a stage's FIRST bottleneck (resnet_fpn.py:154-205 with conv_shortcut: last 1x1 convolution + BN, convolutional
 * shortcut + BN on the block's input, Add, ReLU) as ONE contraction along the concatenated K:
 *   y = relu?( [x1 | x2(:, ::stride2, ::stride2, :)] . w^T + bias ),  w [cout][cin1 + cin2] = [w3 | w_shortcut], bias = b3 + b_sc.
 * x1 NHWC float16 [batch, ceil(H2/stride2), ceil(W2/stride2), cin1] (the block's 3x3 convolution output), x2 NHWC float16
 * [batch,H2,W2,cin2] (the block's input).  The shortcut map is never written or re-read.  cin1, cin2 % 64 == 0. */
int odet_pointwise_dual_f16(const void* x1, int cin1, const void* x2, int cin2, int H2, int W2, int stride2,
                            const void* w, const void* bias, void* y, int batch, int cout, int relu, odet_stream_t stream);
/* The network's LAST dense layer on the same kernel with float32 results: y[rows][cout] (float32) = relu?( x . w^T + bias ),
 * x [rows][cin] / w [cout][cin] float16, bias [cout] float32 (nullable) -- float32 accumulation and no rounding of the
 * result: the class logits and box regressions of the RoI head (resnet_fpn.py:327-336; a float16 logit near 10 is 0.008
 * coarse).  cout % 64 == 0: the caller pads the weight rows (Ccls + 4 Ccls -> 128) with zeros. */
int odet_dense_f16_out_f32(const void* x, const void* w, const float* bias, float* y, long long rows, int cin, int cout,
                           int relu, odet_stream_t stream);
/* A lateral 1x1 convolution of the FPN neck WITH the top-down merge in its epilogue (resnet_fpn.py:385-398):
 * y = 0.5 * resize_bilinear(top, (H, W)) + 0.5 * (x . w^T + bias), TF 1.x legacy resize (align_corners = False) in
 * float32 as odet_fpn_topdown_merge computes it, one rounding; top NHWC float16 [batch,th,tw,cout].  The lateral map
 * never goes to memory. */
int odet_lateral_merge_f16(const void* x, const void* w, const void* bias, const void* top, int th, int tw, void* y,
                           int batch, int H, int W, int cin, int cout, odet_stream_t stream);
/* The same with the 3x3 convolution's channel count as an argument: cmid = 64 (ResNet conv2), 128 (conv3) or 256 (conv4);
 * w2 [cmid][3][3][cin], b2 [cmid], w3 [n3][cmid].  odet_conv3x3_conv1x1_f16 = cmid 256. */
int odet_bottleneck_tail_f16(const void* x, const void* w2, const void* b2, const void* w3, const void* b3,
                             const void* residual, void* y, int batch, int H, int W, int cin, int cmid, int n3, int relu,
                             odet_stream_t stream);
/* The ResNet stem in one launch (resnet_fpn.py:262-289, resnet_faster_rcnn.py:31-60): ZeroPadding2D(3) -> Conv2D(64, 7x7,
 * stride 2, 'valid') + folded frozen BN -> ReLU -> ZeroPadding2D(1) -> MaxPooling2D(3x3, stride 2, 'valid'), from the
 * NHWC 3-channel image (float32: images_f16 = 0, or float16) to the NHWC float16 map [batch][PH][PW][64], PH =
 * ((H - 1) / 2 + 1 - 1) / 2 + 1.  The convolution runs on the matrix cores in float16 with float32 accumulation; neither
 * the padded image nor the convolution output go to memory.  packed_w: the weights repacked once by
 * odet_stem_pack_weights_f16 (from a float16 [64][3][7][7] tensor with the given element strides) into 64 x 7 x 32
 * float16. */
int odet_stem_pack_weights_f16(const void* w, long long stride_o, long long stride_c, long long stride_y,
                               long long stride_x, void* packed, odet_stream_t stream);
int odet_stem_conv7_pool3_f16(const void* images, int images_f16, const void* packed_w, const void* bias, void* out,
                              int batch, int H, int W, odet_stream_t stream);
/* VGG16's first convolution (vgg16_faster_rcnn.py:260-342: Conv2D(64, 3x3, padding 'same') + ReLU on the 3-channel image) in
 * one launch: NHWC image (float32: images_f16 = 0, or float16) -> NHWC float16 [batch][H][W][64], float16 products with
 * float32 accumulation on the matrix cores, + bias (+ ReLU), one rounding.  packed_w: the weights repacked once by
 * odet_conv3x3_rgb_pack_weights_f16 (from a float16 [64][3][3][3] tensor with the given element strides) into 4 x 2 x 64 x 8
 * float16. */
int odet_conv3x3_rgb_pack_weights_f16(const void* w, long long stride_o, long long stride_c, long long stride_y,
                                      long long stride_x, void* packed, odet_stream_t stream);
int odet_conv3x3_rgb_f16(const void* images, int images_f16, const void* packed_w, const void* bias, void* out,
                         int batch, int H, int W, int relu, odet_stream_t stream);
/* The float32 forms (csrc/conv_f32.hip): the detectors' PARITY mode computes in the reference's precision -- float32 x / w /
 * bias / y, exact-float32 matrix instructions (v_mfma_f32_16x16x4_f32: a chain of fmaf, no rounding the reference does
 * not have), the same tiling / staging / epilogues as the float16 entry points of the same names.  cin % 32 == 0,
 * cout % 64 == 0. */
int odet_conv3x3_f32(const void* x, const void* w, const void* bias, void* y, int batch, int H, int W,
                     int cin, int cout, int relu, odet_stream_t stream);
int odet_conv3x3_f32_levels(const odet_conv_level_t* levels, int num_levels, const void* w, const void* bias,
                            int batch, int cin, int cout, int relu, odet_stream_t stream);
/* 1x1 convolutions (stride 1 or 2) / dense layers (odet_pointwise_f16's float32 twin; cin >= 64 along K), the lateral
 * convolution with the top-down merge in its epilogue (bit-identical to odet_fpn_topdown_merge applied to the
 * convolution's float32 result) and a stage's first bottleneck's last convolution + convolutional shortcut as one
 * contraction (resnet_fpn.py:154-205, 292-336, 339-398). */
int odet_pointwise_f32(const void* x, const void* w, const void* bias, const void* residual, void* y, int batch,
                       int H, int W, int stride, int cin, int cout, int relu, odet_stream_t stream);
int odet_lateral_merge_f32(const void* x, const void* w, const void* bias, const void* top, int th, int tw, void* y,
                           int batch, int H, int W, int cin, int cout, odet_stream_t stream);
int odet_pointwise_dual_f32(const void* x1, int cin1, const void* x2, int cin2, int H2, int W2, int stride2,
                            const void* w, const void* bias, void* y, int batch, int cout, int relu, odet_stream_t stream);
/* The SPLIT-PRECISION float32 forms (csrc/conv_x3.hip): the same layers, the same float32 x / bias / y / residual / top in
 * memory and the same epilogues as the *_f32 entry points above, computed on the bfloat16 matrix instructions (16 x the
 * float32 MFMA rate): every float32 operand is the exact sum of three bfloat16 limbs (round to nearest even), a product
 * the six limb products down to 2^-16 of its size (the dropped ones are <= 2^-23 of it), float32 accumulation -- a float32
 * evaluation of the reference's float32 convolution (resnet_fpn.py:154-289, 339-407; base_fpn_model.py:393-434) within
 * float32 rounding of the float64 truth, like the fmaf chain of the *_f32 forms, not bit-identical to it.  `w3` = the
 * weight's limb planes, bfloat16 [3][cout][K] (K = taps * cin (+ cin2) in the order of the float32 weight), written ONCE per
 * weight tensor by odet_split_bf16x3 (n = cout * K float32 values -> planes [3][n]; n even).  cin (and cin2) a positive
 * multiple of 32 (the kernel's 128-byte K-steps), cout % 64 == 0.
 * `workspace` (nullable; odet_x3_workspace_bytes() bytes, 16-byte aligned, ZERO-FILLED ONCE by the caller and then only ever
 * handed to these entry points, one workspace per stream that runs them): with it a launch that would leave CUs idle (few
 * pixels, deep K: the small maps at batch 1 .. 8, the RoI head's dense layers) splits K over up to 8 workgroups per output
 * tile; the last one to finish adds the float32 parts in their fixed order (deterministic; exact on integer data) and runs the
 * epilogue.  Every launch leaves the workspace's ticket words zero again.  NULL: never split. */
size_t odet_x3_workspace_bytes(void);
int odet_split_bf16x3(const float* w, void* planes, long long n, odet_stream_t stream);
int odet_conv3x3_x3(const void* x, const void* w3, const void* bias, void* y, int batch, int H, int W,
                    int cin, int cout, int relu, void* workspace, size_t workspace_bytes, odet_stream_t stream);
int odet_conv3x3_x3_levels(const odet_conv_level_t* levels, int num_levels, const void* w3, const void* bias,
                           int batch, int cin, int cout, int relu, void* workspace, size_t workspace_bytes,
                           odet_stream_t stream);
int odet_pointwise_x3(const void* x, const void* w3, const void* bias, const void* residual, void* y, int batch,
                      int H, int W, int stride, int cin, int cout, int relu, void* workspace, size_t workspace_bytes,
                      odet_stream_t stream);
int odet_lateral_merge_x3(const void* x, const void* w3, const void* bias, const void* top, int th, int tw, void* y,
                          int batch, int H, int W, int cin, int cout, void* workspace, size_t workspace_bytes,
                          odet_stream_t stream);
int odet_pointwise_dual_x3(const void* x1, int cin1, const void* x2, int cin2, int H2, int W2, int stride2,
                           const void* w3, const void* bias, void* y, int batch, int cout, int relu,
                           void* workspace, size_t workspace_bytes, odet_stream_t stream);
/* The TWO-LIMB float16 forms of the same layers (csrc/conv_x3.hip, NL = 2): a float32 operand as h + l * 2^-11, h = f16(a),
 * l = f16((a - h) * 2^11) (round to nearest even: 11 + 11 bits and l's sign = 23 of float32's 24 bits, every operand to
 * within ONE float32 ulp), a product as h h + (h l + l h) * 2^-11 on v_mfma_f32_16x16x32_f16 (dropped: l l <= 2^-22 of it),
 * two float32 accumulators joined at the end: HALF the matrix work of the three-limb form; against float64 its error on the
 * detectors' layers is no larger than the exact-float32 form's (float32 accumulation dominates both) -- for data inside
 * float16's RANGE.  |activation| >= 65520 becomes an infinite limb: every product with it is infinite or NaN, so every sum it
 * enters is non-finite BEFORE bias / shortcut / ReLU whatever the weights' signs (never a wrong finite number), and the launch
 * REPORTS it: with a workspace, the epilogue ORs 1 into the uint32 RANGE STATUS word at byte odet_x2_status_offset() of the
 * workspace whenever a raw sum is not finite (sticky: launches only OR into it; the caller reads it after a chain of layers
 * and clears it -- it is part of the region the caller zero-fills once).  A ReLU (`v < 0 ? 0 : v` maps -inf to 0) can hide
 * the value downstream, never the flag.  Without a workspace a launch cannot report.  Activations below 2^-14
 * keep an absolute error <= 2^-36 instead of a relative one.  `w2` = float16 planes [2][cout][K] of w * 2^w_exp, written once
 * per weight tensor by odet_split_f16x2; the caller picks w_exp (|w_exp| <= 100) so that the largest |w| * 2^w_exp lies in
 * [512, 1024) -- every weight down to 2^-24 of the largest then keeps both limbs normal -- and passes the same w_exp to the
 * layer, which scales the sums back (a power of two: exact).  Everything else as the *_x3 entry points. */
int odet_split_f16x2(const float* w, void* planes, long long n, int w_exp, odet_stream_t stream);
size_t odet_x2_status_offset(void);
int odet_conv3x3_x2(const void* x, const void* w2, const void* bias, void* y, int batch, int H, int W,
                    int cin, int cout, int relu, int w_exp, void* workspace, size_t workspace_bytes, odet_stream_t stream);
int odet_conv3x3_x2_levels(const odet_conv_level_t* levels, int num_levels, const void* w2, const void* bias,
                           int batch, int cin, int cout, int relu, int w_exp, void* workspace, size_t workspace_bytes,
                           odet_stream_t stream);
int odet_pointwise_x2(const void* x, const void* w2, const void* bias, const void* residual, void* y, int batch,
                      int H, int W, int stride, int cin, int cout, int relu, int w_exp, void* workspace,
                      size_t workspace_bytes, odet_stream_t stream);
int odet_lateral_merge_x2(const void* x, const void* w2, const void* bias, const void* top, int th, int tw, void* y,
                          int batch, int H, int W, int cin, int cout, int w_exp, void* workspace, size_t workspace_bytes,
                          odet_stream_t stream);
int odet_pointwise_dual_x2(const void* x1, int cin1, const void* x2, int cin2, int H2, int W2, int stride2,
                           const void* w2, const void* bias, void* y, int batch, int cout, int relu, int w_exp,
                           void* workspace, size_t workspace_bytes, odet_stream_t stream);
/* The stem's patch matrix in float32 mode: row (image, yo, xo) = the zero-padded 7 x 7 x 3 window of conv1_pad +
 * Conv2D(64, 7x7, strides 2, 'valid') (resnet_fpn.py:262-289) in (dy, dx, channel) order, padded from 147 to 160 floats;
 * images NHWC float32 [batch,H,W,3] -> patches [batch * Ho * Wo][160], Ho = (H - 1) / 2 + 1.  The convolution is then
 * odet_pointwise_f32 with cin = 160 on it (weights [64][160] in the same order). */
int odet_stem_patches_f32(const float* images, float* patches, int batch, int H, int W, odet_stream_t stream);
/* The same for VGG16's first convolution (vgg16_faster_rcnn.py:260-342, Conv2D(64, 3x3, 'same') on the 3-channel image):
 * patches [batch][H][W][64] float32, row = the zero-padded 3 x 3 x 3 window in (dy, dx, channel) order, 27 values + zeros. */
int odet_rgb_patches3x3_f32(const float* images, float* patches, int batch, int H, int W, odet_stream_t stream);

/* 1x1 stride-1 convolution with its whole epilogue on the matrix cores (the third convolution
 * of a bottleneck block + Add([shortcut, x]) + Activation('relu'), model/fpn/resnet_fpn.py:154-205, frozen
 * BatchNormalization folded into w / bias): y[npix, cout] = relu?(x'[npix, cin] . w[cout, cin]^T + bias[cout]
 * (+ residual[npix, cout])), all float16 NHWC (w = the convolution's [cout, cin, 1, 1] weight), float32
 * accumulation, one rounding.  x' = x, or relu(x + in_bias[cin]) when in_bias != NULL (x is then the preceding
 * convolution WITHOUT its bias and ReLU: the block's 3x3 convolution; its epilogue pass disappears).
 * cin in {64, 128, 256, 512}, cout % 64 == 0, 16-byte aligned pointers; in_bias / residual may be NULL; y must not
 * alias x (it may alias residual). */
int odet_conv1x1_f16(const void* x, const void* in_bias, const void* w, const void* bias, const void* residual,
                     void* y, long long npix, int cin, int cout, int relu, odet_stream_t stream);

/* RPN head epilogue (model/fpn/base_fpn_model.py:188-200,427-432): one pyramid level's 1x1
 * convolution output level_out [B, pixels, ch] (NHWC, ch = 2A scores or 4A deltas, float32 or float16, WITHOUT
 * its bias) -> + bias[ch] -> float32 at out[b * out_image_stride + out_offset + ...]: the level's slice of the
 * concatenated [B, N, 2] / [B, N, 4] arrays the proposal stage reads (tf.reshape + tf.concat of the reference). */
int odet_rpn_pack(const void* level_out, const void* bias, long long pixels, int ch, int B, float* out,
                  long long out_image_stride, long long out_offset, int f16, odet_stream_t stream);

/* Same, for the RpnHead's two 1x1 convolutions run as ONE contraction (output channels = 2A scores then 4A
 * deltas, weights concatenated): level_out [B, pixels, 6A] + bias[6A] -> the level's slices of BOTH arrays
 * (scores [B, N, 2] at scores_offset values, deltas [B, N, 4] at deltas_offset values inside an image). */
int odet_rpn_pack_pair(const void* level_out, const void* bias, long long pixels, int A, int B, float* scores,
                       long long scores_image_stride, long long scores_offset, float* deltas,
                       long long deltas_image_stride, long long deltas_offset, int f16, odet_stream_t stream);

/* The whole RpnHead after its 3x3 convolution in one pass (base_fpn_model.py:393-434, 188-200):
 * conv_out [B, pixels, 512] = the 3x3 convolution WITHOUT its bias (float16 NHWC), conv_bias [512];
 * t = relu(conv_out + conv_bias); scores = t . w[0:2A]^T + bias[0:2A]; deltas = t . w[2A:6A]^T + bias[2A:6A]
 * (w [6A, 512] float16 = rpn_score's rows then rpn_bbox's, bias [6A] float16), written as float32 into the level's
 * slices of the concatenated [B, N, 2] / [B, N, 4] arrays (offsets / strides in VALUES, as odet_rpn_pack_pair).
 * Matrix cores, float32 accumulation; 1 <= A <= 4. */
int odet_rpn_head_tail_f16(const void* conv_out, const void* conv_bias, const void* w, const void* bias,
                           long long pixels, int A, int B, float* scores, long long scores_image_stride,
                           long long scores_offset, float* deltas, long long deltas_image_stride,
                           long long deltas_offset, odet_stream_t stream);

/* ---- multi-GPU detection records ------------------------------------------------------ */

/* Native addition (the reference has no multi-GPU path): packs the padded post-ops outputs of
 * one image into the fixed-size record exchanged by the image-parallel all-gather:
 * out_record float32 [max_det*6 + 1] = max_det rows (x1,y1,x2,y2,score,label), padded rows
 * zero with score -1, then the count.  capacity = rows available in boxes/labels/scores. */
int odet_pack_detections(const float* boxes, const int32_t* labels, const float* scores,
                         const int32_t* count_dev, int capacity, int max_det, float* out_record,
                         odet_stream_t stream);

/* ---- whole-step descriptor + native executor (throughput serving) ---------------------- */

/* One image through the FPN hot path as the reference's BaseFPN.call runs it
 * (model/fpn/base_fpn_model.py:208-276 minus the dense conv parts): every buffer is caller-owned
 * device memory, the struct is plain data.  odet_fpn_step_enqueue() issues the selected stages on
 * `stream` from the calling thread:
 *   ODET_STAGE_PROPOSALS = odet_fpn_proposals   (anchors, fg softmax, RegionProposal, _assign_levels; also the
 *                          processing order into roi_order when num_proposals <= ODET_FUSED_ORDER_MAX_ROIS)
 *   ODET_STAGE_ROI       = odet_roi_pool        (RoiPoolingCropAndResize2 over maps[0..num_maps); odet_roi_order
 *                          first when num_proposals > ODET_FUSED_ORDER_MAX_ROIS)
 *   ODET_STAGE_DETECT    = odet_post_ops_record (post_ops_prediction + detection record) */
#define ODET_STAGE_PROPOSALS 1
#define ODET_STAGE_ROI 2
#define ODET_STAGE_DETECT 4
#define ODET_STAGE_ALL 7

typedef struct {
  /* proposals */
  int32_t image_h, image_w;
  int32_t num_levels, A;                         /* RPN pyramid levels / anchors per cell */
  int32_t fh[ODET_MAX_LEVELS], fw[ODET_MAX_LEVELS], stride[ODET_MAX_LEVELS];
  float wh[ODET_MAX_LEVELS * ODET_MAX_ANCHORS_PER_CELL * 2];
  float rpn_means[4], rpn_stds[4];
  int32_t num_proposals;
  float rpn_nms_iou;
  int32_t min_level, max_level, blind_chunks;
  int32_t nms_first_chunk;   /* 0 = auto (~1.5 x num_proposals candidates); else candidates of the first NMS chunk,
                                <= 4096: a wider chunk lets heavy suppression (trained-like score clusters) finish
                                inside the one sync-free chunk of batched launches */
  /* roi */
  int32_t num_maps, channels, pool_size;
  int32_t maps_f16;          /* != 0: float16 feature maps and float16 roi_features (odet_roi_pool_f16) */
  odet_level_t maps[ODET_MAX_LEVELS];
  /* detect */
  int32_t ccls, num_classes, max_per_class, max_per_image;
  float roi_means[4], roi_stds[4];
  float nms_iou, score_threshold, min_edge;
  /* inputs (device) */
  const float* rpn_logits;   /* [n,2] */
  const float* rpn_deltas;   /* [n,4] */
  const float* cls_scores;   /* [num_proposals, ccls] */
  const float* cls_deltas;   /* [num_proposals, ccls, 4] */
  /* outputs / scratch (device, caller-owned) */
  float* rois; int32_t* roi_idx; int32_t* roi_count; int32_t* nms_done;
  float* sorted_rois; int32_t* roi_level; int64_t* roi_perm; int32_t* level_counts;
  void* roi_features;        /* [num_proposals, pool, pool, channels] float32 (float16 when maps_f16) */
  int32_t* roi_order;        /* nullable scratch int32 [num_proposals]: spatial processing order (odet_roi_order) */
  float* det_boxes; int32_t* det_labels; float* det_scores; int32_t* det_count; float* record;
  void* ws_rpn; size_t ws_rpn_bytes;
  void* ws_post; size_t ws_post_bytes;
  odet_stream_t stream;
  /* profiling (nullable): HIP events (odet_prof_event_create) attached to the RoI dispatch of this step -- in a
   * batch those of the first step bracket the one launch all its images share */
  void* roi_start_event; void* roi_stop_event;
  /* != 0: the caller promises that ws_rpn was zero-filled once after its allocation and has only ever been handed to
   * this library since: every call leaves the proposal stage's header clean again, so no launch / memset is spent on
   * zeroing it.  (ws_post has its own promise, ws_post_clean, since version 101.) */
  int32_t ws_rpn_clean;
  /* != 0: a single-level Faster R-CNN step (model/faster_rcnn/base_faster_rcnn_model.py:126-198 minus the dense
   * parts) instead of an FPN step: num_levels = num_maps = 1; fh[0] x fw[0] cells of stride[0] with A anchors each,
   * wh[0 .. 4A) = the anchor base (generate_anchor_base as float32 rows x1,y1,x2,y2); rpn_logits [fh*fw, 2A] in the
   * [A bg | A fg] layout; no level assignment (sorted_rois must alias rois; roi_level, roi_perm, level_counts NULL);
   * RoI crops normalised by maps[0].stride (ODET_ROI_NORM_STRIDE) with roi_pool_mode; min_edge = the stride. */
  int32_t single_level;
  int32_t roi_pool_mode;     /* single_level: ODET_ROI_POOL_MAX2 (VGG16) | ODET_ROI_POOL_NONE (ResNet C4); FPN: MAX2 */
  /* != 0: the same promise for ws_post (zero-filled once, only ever handed to this library): the post-processing
   * launch keeps a wrapping ticket counter at its end, which every COMPLETED call leaves at 0.  With 0 here the library
   * issues the 4-byte memset on the stream before the launch (the default; costs nothing at graph replay).  After a
   * failed call (an error from odet_exec_wait / a launch error) zero-fill ws_post again before promising this. */
  int32_t ws_post_clean;
} odet_fpn_step_t;

size_t odet_fpn_step_sizeof(void);
int odet_fpn_step_enqueue(const odet_fpn_step_t* step, int stages);
/* `count` (<= ODET_MAX_STEP_BATCH) images whose steps agree in every shape, parameter and the stream,
 * processed by the SAME kernel launches (one grid dimension = image): per-launch costs are paid once
 * per batch and the single-workgroup stages of the images run side by side.  Needs the sync-free NMS
 * mode (nms_done != NULL); blind_chunks >= 1 (chunk 1 comes from the same ranked selection in launches
 * shared by the batch, chunks 2.. per image on the full order).  An image whose NMS did not complete
 * inside its chunks reports zero proposals and nms_done = 0 (see odet_nms). */
#define ODET_MAX_STEP_BATCH 8
int odet_fpn_step_enqueue_batch(const odet_fpn_step_t* const* steps, int count, int stages);

/* Native executor: `num_workers` host threads, each draining its own FIFO of (step, stages) jobs by
 * calling odet_fpn_step_enqueue.  A HIP kernel launch costs ~3 us of host time and one image is ~11
 * launches, so one host thread saturates near 20k images/s; with one worker per stream the images of
 * different streams are enqueued in parallel (the reference has no counterpart: it is a
 * single-threaded Python loop).  A job only enqueues GPU work; completion is the stream's business.
 * The step structs must stay alive and unchanged until odet_exec_wait() has returned.  Work that
 * must be ordered after a job on the same stream from another thread (e.g. a torch op) has to be
 * issued after odet_exec_wait(). */
typedef struct odet_exec odet_exec_t;
odet_exec_t* odet_exec_create(int num_workers);
void odet_exec_destroy(odet_exec_t* ex);
int odet_exec_submit(odet_exec_t* ex, int worker, const odet_fpn_step_t* step, int stages);
int odet_exec_submit_batch(odet_exec_t* ex, int worker, const odet_fpn_step_t* const* steps, int count,
                           int stages);
/* blocks until every submitted job has been enqueued; returns the first error any job hit (0 = none;
 * text through odet_exec_last_error) and clears it */
int odet_exec_wait(odet_exec_t* ex);
const char* odet_exec_last_error(odet_exec_t* ex);

/* ---- training targets (added within 103) ---------------------------------------------------------------------------
 * model/anchor_target.py:49-107 and model/proposal_target.py:54-124 for a BATCH of images in a fixed number of launches on
 * `stream`: no IoU matrix in memory, no allocation, no host read (graph-capturable), every output bitwise reproducible and
 * independent of the batch an image sits in.
 *
 * Ground truth is packed: gt_boxes [sum G, 4], gt_offsets device int32 [batch+1] (image b owns rows
 * gt_offsets[b] .. gt_offsets[b+1]).  Limits: batch <= 64, total_num_samples <= 1024, max_pos_samples <= total_num_samples,
 * at most 2^20 anchors and 65536 RoIs per image (ODET_E_LIMIT / ODET_E_INVALID).  At most 1024 boxes per image: the offsets
 * live on the device, so the call cannot refuse on the host -- an image above the limit is reported ON THE DEVICE by a
 * `counts` row of -1 and gets fill values (labels -1, everything else 0, no sampled row) in every output.  An image with G = 0
 * (the reference cannot run it) is background only: row maximum 0, arg-maximum -1, targets 0.
 *
 * Sampling rule.  philox(ctr[4], key[2]) = Philox4x32-10.  Candidate i of image b owns
 *   key64(stream, image_id, i) = (w0 << 32) | w1  of  philox((i, image_id, stream, 0), (seed low word, seed high word)),
 * image_id = first_image_id + b.  "Keep k of the candidates" = the k candidates with the smallest (key64, i) pairs: a uniformly
 * random k-subset like the reference's shuffle-and-slice, and a function of (seed, image_id, i) alone.  Streams: 0 anchor
 * foreground, 1 anchor background, 2 RoI foreground, 3 RoI background; i = index into ALL anchors resp. the RoI's row.
 * With replacement (proposal_target.py:73-76): draw j picks bg_ascending[(uint64(w0) * n_bg) >> 32], w0 of
 * philox((j, image_id, 4, 0), seed).  Stream 5 is the flip decision of odet_preprocess_train (i = 0). */

size_t odet_anchor_target_workspace_bytes(int num_anchors, int batch, int total_num_samples);
/* anchors [num_anchors,4] shared by the batch (one image shape).  In the reference's order: inside = bboxes_range_filter;
 * IoU (the arithmetic of odet_pairwise_iou) over inside anchors only; row maximum and FIRST arg-maximum; column maximum per
 * box; labels -1, then 0 where max < neg, then 1 where IoU[a,g] == column maximum of any g (a box that meets no inside anchor
 * has maximum 0 and so marks every anchor with zero overlap: the reference's behaviour, kept), then 1 where max >= pos;
 * foreground kept to max_pos_samples, background to total_num_samples - kept foreground, by the sampling rule.
 * Outputs.  Dense, each nullable (null = not written): labels float32 [batch,N] in {-1,0,1}; targets [batch,N,4] =
 * odet_encode's arithmetic of (anchor, box[arg-maximum]) on EVERY inside anchor, 0 elsewhere; inside [batch,N,4] = 1 on
 * label 1; outside [batch,N,4] = float32(1) / float32(kept foreground + kept background) on labels >= 0.  Compact, required:
 * sample_idx int32 [batch,S] (S = total_num_samples: kept foreground anchors in ascending index order, then the background
 * ones, then -1), sample_targets [batch,S,4], counts int32 [batch,5] = inside anchors, foreground and background before
 * sampling, foreground and background kept.  For parity checks, nullable: labels_before_sampling int32 [batch,N] and
 * argmax int32 [batch,N], both -1 outside the image. */
int odet_anchor_target(const float* anchors, int num_anchors, const float* gt_boxes, const int32_t* gt_offsets,
                       int batch, int image_h, int image_w, float pos_iou_threshold, float neg_iou_threshold,
                       int total_num_samples, int max_pos_samples, const float* means, const float* stds,
                       uint64_t seed, uint32_t first_image_id, float* labels, float* targets, float* inside,
                       float* outside, int32_t* sample_idx, float* sample_targets, int32_t* counts,
                       int32_t* labels_before_sampling, int32_t* argmax, void* workspace, size_t workspace_bytes,
                       odet_stream_t stream);

size_t odet_proposal_target_workspace_bytes(int max_rois, int batch);
/* rois [batch,max_rois,4]; roi_counts (nullable) device int32 [batch]: valid rows per image.  gt_labels int32 [sum G].
 * Assignment (:55-63): row maximum, FIRST arg-maximum = gt_assignment, labels = gt_labels[gt_assignment]; foreground
 * max >= pos, background neg <= max < pos.  Keep max_pos_samples of the foreground, then want = S - kept foreground of the
 * background, with replacement when there are fewer.  Row order: foreground rows first, in ascending (key64, i) order when
 * they were sampled and in ascending row index when not; the same for the background; with-replacement picks in draw order.
 * Outputs, all of fixed shape (S = total_num_samples, C = num_classes): final_rois [batch,S,4]; final_labels int32 [batch,S]
 * (0 on background rows); targets, inside, outside float32 [batch,S,4C] (outside = 1 on written rows); keep int32 [batch,S]
 * = input row of each output row; gt_assignment int32 [batch,max_rois] (-1 on rows >= roi_counts or without ground truth);
 * counts int32 [batch,4] = foreground candidates, background candidates, foreground rows, rows written.
 * reference_row_labels != 0 keeps the reference's column choice (:96, :113): foreground row r writes into the class column
 * of INPUT RoI number r; 0 uses the sampled RoI's own class.  An image that wants background rows and has no candidate (the
 * reference fails there) gets its foreground rows, rows written < S, and zeros with keep = -1 behind them. */
int odet_proposal_target(const float* rois, const int32_t* roi_counts, int max_rois, const float* gt_boxes,
                         const int32_t* gt_labels, const int32_t* gt_offsets, int batch, int num_classes,
                         float pos_iou_threshold, float neg_iou_threshold, int total_num_samples,
                         int max_pos_samples, const float* means, const float* stds, int reference_row_labels,
                         uint64_t seed, uint32_t first_image_id, float* final_rois, int32_t* final_labels,
                         float* targets, float* inside, float* outside, int32_t* keep, int32_t* gt_assignment,
                         int32_t* counts, void* workspace, size_t workspace_bytes, odet_stream_t stream);

/* ---- training losses (added within 103) ----------------------------------------------------------------------------
 * The four losses of model/losses.py:4-28 as the caller models use them (fpn/base_fpn_model.py:278-301,
 * faster_rcnn/base_faster_rcnn_model.py:200-231), for a BATCH of images, from the outputs of odet_anchor_target /
 * odet_proposal_target and the raw float32 head outputs, with their gradients with respect to the head outputs.  One launch
 * per forward, no workspace, no allocation, no host read (graph-capturable), no float atomics; every output bitwise
 * reproducible and independent of the batch an image sits in.  Limits: batch <= 64, total_num_samples <= 1024
 * (ODET_E_LIMIT).
 *
 * Arithmetic.  Element operations are single float32 operations in the reference's order (no FMA contraction), exp / log are
 * correctly rounded.  sigma_2 = sigma * sigma, and 1 / sigma_2, sigma_2 / 2, 0.5 / sigma_2 are float32 operations.
 * A softmax row x[0..C): z_j = x_j - max, e_j = exp(z_j), s = e_0 + e_1 + ... , p_j = e_j / float32(s),
 * CE = log(float32(s)) - z_label.  A smooth-L1 element: d = inside * (pred - target), sign = |d| < 1 / sigma_2,
 * l = outside * (d * d * (sigma_2 / 2) * sign + (|d| - 0.5 / sigma_2) * (1 - sign)), gradient outside * inside * (sigma_2 * d
 * where sign, else +-1 with the sign of d).
 * Sums are accumulated in FLOAT64 in a fixed order and rounded to float32 once: the classes of a row in ascending order; the
 * 4 coordinates of an RPN row in ascending order; the 4C columns of a RoI row as 64 partial sums (partial l adds columns
 * l, l + 64, ... in ascending order) that are then added in ascending l; the rows of an image in ascending order. */

/* scores: `layout` (ODET_RPN_LAYOUT_*, anchors_per_location = A; N % A == 0 for the FRCNN layout) of 2N floats per image,
 * deltas [batch,N,4]; sample_idx [batch,S], sample_targets [batch,S,4], counts [batch,5] as odet_anchor_target wrote them
 * (S = total_num_samples).  n = counts[3] + counts[4]; rows r < counts[3] have label 1, rows counts[3] <= r < n label 0.
 * losses float32 [batch,2] = (cls, reg): cls = float32(sum of the rows' CE) / float32(max(n,1)); reg = float32(sum over the
 * label-1 rows and their 4 coordinates of l), with inside = 1 and outside = float32(1) / float32(n) (dim=[0,1]: a sum).
 * row_grad_scores [batch,S,2] = (p_j - [j == label]) / float32(n) and row_grad_deltas [batch,S,4] = the smooth-L1 gradient
 * (0 on label-0 rows): d loss / d (row of the head outputs) at upstream gradient 1.  Rows >= n are 0.  An image whose counts
 * row is -1 or whose n is 0 has losses 0 and gradients 0.  All pointers are required.
 * Counts and indices that odet_anchor_target never writes are clamped, not trusted: a negative counts[3] or counts[4] empties
 * the image; then counts[3] = min(counts[3], S) and n = min(counts[3] + counts[4], S).  A row r < n whose sample_idx lies
 * outside 0..N-1 adds nothing to either loss and has zero row gradients, but still counts in n (the divisor and outside);
 * odet_rpn_loss_backward skips every such index among all S entries and writes every other one (a row >= n with
 * upstream * 0, a zero that carries the upstream's sign). */
int odet_rpn_loss(const float* scores, const float* deltas, int num_anchors, int batch, int layout,
                  int anchors_per_location, const int32_t* sample_idx, const float* sample_targets, const int32_t* counts,
                  int total_num_samples, float sigma, float* losses, float* row_grad_scores, float* row_grad_deltas,
                  odet_stream_t stream);
/* The dense gradients: grad_scores in the SAME layout as the scores (2N floats per image) and grad_deltas [batch,N,4], each
 * nullable and 16-byte aligned: 0 everywhere except the rows of sample_idx, which hold upstream[b][0] * row_grad_scores resp.
 * upstream[b][1] * row_grad_deltas (upstream: device float32 [batch,2], the gradients arriving at (cls, reg)).  Two launches:
 * the zero fill, then the scatter (sample_idx holds no duplicates within an image). */
int odet_rpn_loss_backward(const int32_t* sample_idx, const float* row_grad_scores, const float* row_grad_deltas,
                           const float* upstream, int num_anchors, int batch, int layout, int anchors_per_location,
                           int total_num_samples, float* grad_scores, float* grad_deltas, odet_stream_t stream);
/* scores [batch,R,C], deltas [batch,R,4C] (R = num_rows <= 2048, C = num_classes <= 1024: ODET_E_LIMIT); final_labels
 * [batch,S], targets / inside / outside [batch,S,4C], counts [batch,4] as odet_proposal_target wrote them.  row_map
 * (nullable) int32 [batch,R]: head row r belongs to target row row_map[r] (the FPN caller's level-order permutation); null =
 * identity.  rows = counts[3].  A head row takes part when its target row m satisfies 0 <= m < rows (and its label lies in
 * 0..C-1); every other head row contributes nothing and gets gradient 0.
 * losses [batch,2] = (float32(sum over head rows of CE) / float32(max(rows,1)), float32(sum over head rows of the row's
 * smooth-L1 sum) / float32(max(rows,1))).  grad_scores [batch,R,C] = u_cls * ((p_j - [j == label]) / float32(rows)),
 * grad_deltas [batch,R,4C] = u_reg * (smooth-L1 gradient / float32(rows)), (u_cls, u_reg) = upstream[b] (device float32
 * [batch,2]) or (1, 1) when upstream is null.  losses, grad_scores and grad_deltas are each nullable.
 * rows is clamped to 0..S (a counts row of -1: nothing takes part).  A head row whose label is outside 0..C-1 (a stray -1 or
 * C) gets gradient 0 like a row without a target, and its target row still counts in rows.  With num_rows == 0 scores and
 * deltas may be NULL and the losses are 0. */
int odet_roi_loss(const float* scores, const float* deltas, int num_rows, int num_classes, int batch,
                  const int32_t* final_labels, const float* targets, const float* inside, const float* outside,
                  const int32_t* counts, int total_num_samples, const int32_t* row_map, float sigma,
                  const float* upstream, float* losses, float* grad_scores, float* grad_deltas, odet_stream_t stream);

/* ---- training step (added within 103) ------------------------------------------------------------------------------
 * The other end of train_one_epoch (scripts/train.py:22-50, 101-103) for the WHOLE variable list in one update launch plus
 * a one-workgroup finish launch: the L2 regulariser of every regularised kernel (keras regularizers.l2: tf.add_n(model.losses)),
 * the bias-gradient doubling of train_step, tf.train.piecewise_constant on the global step, and MomentumOptimizer /
 * AdamOptimizer.apply_gradients (TF r1.13 training_ops.cc ApplyMomentum / ApplyAdam).  No workspace beyond the caller's
 * partials buffer, no allocation, no host read (graph-capturable), no float atomics.  The update launch only reads the state
 * block; the finish launch, after it in stream order, is its only writer.
 *
 * Tables (DEVICE memory, built by the caller; the library cannot check their contents on the host, so the kernels skip what
 * does not fit: a chunk whose tensor index or offset is out of range, a float16 variable without a master, a tensor without
 * the slots its optimizer needs):
 *   tensors   odet_opt_tensor_t [num_tensors], one record per variable;
 *   grads     const void* [num_tensors], the gradient pointer column (float32, or float16 with ODET_OPT_GRAD_F16): a column of
 *             its own so that a step whose gradients moved re-uploads 8 bytes per variable.  A NULL entry means the gradient
 *             is None this step: the variable, its slots and its master are left untouched (its L2 loss is still computed);
 *   chunks    odet_opt_chunk_t [num_chunks]: chunk c covers elements offset .. min(offset + ODET_OPT_CHUNK, numel) of ONE
 *             tensor, offset a multiple of ODET_OPT_CHUNK; the chunks of tensor t are first_chunk .. first_chunk +
 *             ceil(numel / ODET_OPT_CHUNK) - 1 in ascending offset (a tensor of 0 elements has none);
 *   state     odet_opt_state_t: global_step (0 on the first step), the Adam beta powers (the caller initialises them to beta1,
 *             beta2) and the schedule.
 * Limits (ODET_E_LIMIT): num_tensors <= ODET_OPT_MAX_TENSORS, num_chunks <= ODET_OPT_MAX_CHUNKS, num_boundaries <=
 * ODET_OPT_MAX_BOUNDARIES.  A chunk goes through 16-byte loads and stores (8-byte for float16 arrays) when every array it
 * touches is 16-byte (8-byte) aligned, else element by element: any 4-byte (2-byte) aligned view works, with the same bits.
 *
 * Arithmetic.  Every operation below is ONE float32 operation, in this order, no FMA contraction; divide and sqrt are
 * correctly rounded.  w is the float32 variable, or the float32 master of a float16 variable.
 *   lr     = values[i], i = the number of boundaries strictly below global_step (piecewise_constant: x <= boundaries[0]
 *            still takes values[0]);
 *   g      = gradient (a float16 gradient is widened, exactly); if weight_decay != 0: g = g + weight_decay * (2 * w), w the
 *            pre-update value; then g = g * grad_scale;
 *   momentum (no Nesterov): a' = a * momentum + g;  w' = w - a' * lr;
 *   adam:  alpha = lr * sqrt(1 - beta2_power) / (1 - beta1_power), left to right;  m' = m + (g - m) * (1 - beta1);
 *          v' = v + (g * g - v) * (1 - beta2);  w' = w - (m' * alpha) / (sqrt(v') + epsilon);
 *   float16 variable: the master takes w', the variable takes w' rounded to nearest-even once;
 *   finish: global_step += 1; adam: beta1_power *= beta1, beta2_power *= beta2 (float32).
 * L2 loss of a tensor = float32(weight_decay * float32(S)) (0 when weight_decay == 0), S the FLOAT64 sum of the float32 squares
 * w * w of the PRE-update values in this order, a function of the tensor alone (not of its place in the table, the other
 * tensors, the grid or the alignment).  Cut the tensor into chunks of ODET_OPT_CHUNK = 4096 elements (the last one padded with
 * zeros).  In a chunk, element j belongs to lane (j / 4) % 256; a lane adds its 16 squares in ascending j (numpy:
 * sq.reshape(4, 256, 4).transpose(1, 0, 2).reshape(256, 16), cumsum along the last axis).  The 64 lane sums of each of the 4
 * waves (lanes 64 v .. 64 v + 63) are folded in halves: v = v[:32] + v[32:], then [:16] + [16:], ... down to one value; the
 * chunk sum is wave 0 + wave 1 + wave 2 + wave 3, left to right.  Over the chunks: 64 sums, sum l adding chunks l, l + 64, ...
 * in ascending order, then the same fold in halves of the 64.
 * total loss = the float32 left-to-right sum of the per-tensor losses in table order (tf.add_n). */
#define ODET_OPT_CHUNK 4096            /* elements per chunk */
#define ODET_OPT_MAX_TENSORS 4096
#define ODET_OPT_MAX_CHUNKS (1 << 24)  /* 2^36 elements */
#define ODET_OPT_MAX_BOUNDARIES 16
#define ODET_OPT_MOMENTUM 1
#define ODET_OPT_ADAM 2
#define ODET_OPT_VAR_F16 1             /* flags: var is float16 (master required) */
#define ODET_OPT_GRAD_F16 2            /* flags: the gradient is float16 */

typedef struct odet_opt_tensor_t {
  void* var;            /* float32, or float16 with ODET_OPT_VAR_F16 */
  float* slot0;         /* momentum: accum; adam: m */
  float* slot1;         /* adam: v; momentum: unused (NULL) */
  float* master;        /* float32 master of a float16 variable, else NULL */
  int64_t numel;
  float weight_decay;   /* 0 = unregularised */
  float grad_scale;     /* 1, or 2 for a bias under learning_rate_bias_double */
  int32_t flags;
  int32_t first_chunk;  /* index of the tensor's first chunk in the chunk table (and in the partials buffer) */
  int64_t reserved;     /* 0 */
} odet_opt_tensor_t;    /* 64 bytes */

typedef struct odet_opt_chunk_t {
  int64_t offset;       /* first element, a multiple of ODET_OPT_CHUNK */
  int32_t tensor;
  int32_t reserved;     /* 0 */
} odet_opt_chunk_t;     /* 16 bytes */

typedef struct odet_opt_state_t {
  int64_t global_step;
  float beta1_power, beta2_power;
  int64_t boundaries[ODET_OPT_MAX_BOUNDARIES];
  float values[ODET_OPT_MAX_BOUNDARIES + 1];
  float reserved;       /* 0 */
} odet_opt_state_t;     /* 216 bytes */

typedef struct odet_opt_config_t {   /* HOST */
  int32_t kind;         /* ODET_OPT_MOMENTUM / ODET_OPT_ADAM (odet_l2_loss ignores it) */
  int32_t num_tensors, num_chunks, num_boundaries;
  float momentum, beta1, beta2, epsilon;
} odet_opt_config_t;

/* bytes of the partials buffer (one float64 per chunk; 8-byte aligned); only the chunks of regularised tensors are used */
size_t odet_opt_partials_bytes(int num_chunks);
/* One training step.  cfg: HOST.  tensor_losses float32 [num_tensors] and total_loss float32 [1] are each nullable; with both
 * NULL no L2 sum is formed and partials may be NULL.  Errors, all before any GPU work: ODET_E_INVALID (null cfg / state /
 * table, unknown kind, a beta outside [0, 1), negative epsilon or count, L2 outputs without partials), ODET_E_LIMIT (above),
 * ODET_E_WORKSPACE (partials too small). */
int odet_opt_step(const odet_opt_config_t* cfg, const odet_opt_tensor_t* tensors, const void* const* grads,
                  const odet_opt_chunk_t* chunks, odet_opt_state_t* state, void* partials, size_t partials_bytes,
                  float* tensor_losses, float* total_loss, odet_stream_t stream);
/* The same L2 reduction with no update (the forward value of l2_loss): nothing but the two outputs and partials is written. */
int odet_l2_loss(const odet_opt_config_t* cfg, const odet_opt_tensor_t* tensors, const odet_opt_chunk_t* chunks, void* partials,
                 size_t partials_bytes, float* tensor_losses, float* total_loss, odet_stream_t stream);

/* ---- gradient exchange (added within 103) --------------------------------------------------------------------------
 * The byte moves and the arithmetic of data-parallel training, one image per rank (parallel.GradientExchange): the gradient
 * list goes into one contiguous float32 BUCKET in one launch, collectives that only move bytes hand rank r shard r of every
 * rank, and the sum over the ranks is formed here in ASCENDING RANK order -- so the exchanged gradient is a function of the data
 * alone, whatever the collective library's algorithm, channel count or topology.  All three: no allocation, no host read
 * (graph-capturable), no atomics, every output element written exactly once; errors are found on the host before any HIP call.
 *
 * Bucket layout.  The chunk table of the training step (odet_opt_chunk_t, ODET_OPT_CHUNK elements per chunk) built over the
 * PRESENT tensors in list order: chunk c of the table is elements c * ODET_OPT_CHUNK .. of the bucket and covers elements offset ..
 * min(offset + ODET_OPT_CHUNK, numel) of tensor `tensor`; a tensor of 0 elements, or an absent one (NULL in the pointer column),
 * has no chunk and no place.  bucket_chunks >= num_chunks is the bucket's size (a whole number of shards: world * shard_chunks).
 *   tensors   void* [num_tensors] (DEVICE): the pointer column, a table of its own so that tensors that moved cost an 8-byte
 *             re-upload each; float32, dense, 4-byte aligned;
 *   numels    int64 [num_tensors] (DEVICE);
 *   chunks    odet_opt_chunk_t [num_chunks] (DEVICE); a record that does not fit (tensor index or offset out of range, a NULL
 *             tensor) is treated as absent: pack writes +0.0f for it, unpack skips it.
 * odet_bucket_pack_f32 writes EVERY element of the bucket: the tensors' elements, +0.0f in the tail of a tensor's last chunk and
 * in the chunks num_chunks .. bucket_chunks - 1.  odet_bucket_unpack_f32 writes each present tensor's numel elements and
 * nothing else.  A chunk goes through 16-byte loads and stores when its tensor is 16-byte aligned, else element by element,
 * with the same bits; the bucket itself must be 16-byte aligned.
 * Errors: ODET_E_INVALID (a negative count, num_chunks > bucket_chunks, a null table that is needed, a null or misaligned
 * bucket), ODET_E_LIMIT (num_tensors > ODET_OPT_MAX_TENSORS, bucket_chunks > ODET_OPT_MAX_CHUNKS).
 *
 * odet_rank_mean_f32: parts float32 [world, n] -> out float32 [n].  s = parts[0][i]; s = s + parts[r][i] for r = 1 .. world - 1,
 * each ONE float32 add, in ascending r; average (0 / 1): out[i] = s / float32(world), one correctly rounded division (not a
 * multiplication by a reciprocal), else out[i] = s.  world == 1 returns the input's bits.  16-byte accesses where a row (and
 * out) is 16-byte aligned, else element by element, with the same bits; out must not overlap parts.
 * Errors: ODET_E_INVALID (world < 1, n < 0, average outside {0, 1}, a null pointer with n > 0, a pointer not 4-byte aligned),
 * ODET_E_LIMIT (world > ODET_RANK_MEAN_MAX_WORLD, n > ODET_OPT_MAX_CHUNKS * ODET_OPT_CHUNK).  n == 0 is a no-op. */
#define ODET_RANK_MEAN_MAX_WORLD 64
int odet_bucket_pack_f32(const void* const* tensors, const int64_t* numels, int num_tensors, const odet_opt_chunk_t* chunks,
                         int num_chunks, float* bucket, int64_t bucket_chunks, odet_stream_t stream);
int odet_bucket_unpack_f32(const float* bucket, int64_t bucket_chunks, void* const* tensors, const int64_t* numels,
                           int num_tensors, const odet_opt_chunk_t* chunks, int num_chunks, odet_stream_t stream);
int odet_rank_mean_f32(const float* parts, int world, int64_t n, int average, float* out, odet_stream_t stream);

/* odet_bucket_accumulate_f32: one image of a K-image training step (training.GradientAccumulator) in ONE launch over the whole
 * gradient list.  The tables, the layout, the "a record that does not fit is absent" rule and the alignment rules are those of
 * odet_bucket_pack_f32.  For every element e of a present tensor, g the tensor's element and b = bucket[e]:
 *   s = g when first, else s = b + g (ONE float32 add, no contraction);
 *   bucket[e] = s when divisor == 1.0f, else s / divisor (one correctly rounded IEEE division, not a multiplication by a
 *   reciprocal).
 * A window of K images is first = 1 on image 0, first = 0 after it, divisor = float32(K) on the last call (1.0f before): the
 * statement of odet_rank_mean_f32 -- the first image's bits, one add per image in ascending image order, one division at the end.
 * first = 1 writes EVERY element of the bucket as pack does (+0.0f in the tail of a tensor's last chunk, in absent records and in
 * the chunks num_chunks .. bucket_chunks - 1); first = 0 writes the present tensors' elements and nothing else.  Every element
 * that is written is written once; no atomics, no allocation, no host read (graph-capturable).  Per element 8 bytes are read and
 * 4 written (first: 4 and 4).
 * Errors, before any HIP call: ODET_E_INVALID (pack's conditions, first outside {0, 1}, a divisor that is not finite and > 0),
 * ODET_E_LIMIT (pack's limits). */
int odet_bucket_accumulate_f32(const void* const* tensors, const int64_t* numels, int num_tensors, const odet_opt_chunk_t* chunks,
                               int num_chunks, float* bucket, int64_t bucket_chunks, int first, float divisor, odet_stream_t stream);

/* ---- Dense backward, float32 (added within 103) --------------------------------------------------------------------
 * The gradients of a keras Dense layer y = relu?(x . w^T + b) (resnet_fpn.py:292-336, the FPN RoI head) on the exact-float32
 * matrix instruction of odet_pointwise_f32.  All tensors float32, row-major, in the forward's own layouts -- nothing is
 * transposed in memory: x [rows, cin], w [cout, cin], y / dy [rows, cout].  y_relu (nullable) is the layer's own forward
 * output: the operand is dz = y_relu > 0 ? dy : 0 (TF ReluGrad: strict '>', a select), formed while staging; no dz is written.
 *   odet_dense_dgrad_f32: dx [rows, cin] = dz . w (contraction along cout); x_relu (nullable, [rows, cin], the forward output of
 *     the layer below) keeps dx only where x_relu > 0, in the epilogue.
 *   odet_dense_wgrad_f32: dw [cout, cin] = dz^T . x (contraction along rows, any positive count); db (nullable) [cout] = the
 *     column sums of dz, from a second small launch.
 * Shapes (ODET_E_INVALID otherwise, as every error here before any GPU work): rows >= 1, cin a multiple of 32 and >= 64,
 * cout a multiple of 64; pointers 16-byte aligned (db: 4).  ODET_E_WORKSPACE: a workspace smaller than
 * odet_dense_grad_workspace_bytes(wgrad = 0 | 1, rows, cin, cout) -- 0 for most shapes; non-zero when the launch splits its
 * contraction (few output tiles, contraction >= 256), 16-byte aligned, contents arbitrary.
 * Order of sums: a function of the shape alone, no atomics -- an element adds its products in ascending k, four per matrix
 * instruction (each product and sum rounded to float32 once); a split launch leaves its parts (equal runs of whole 32-k steps)
 * in the workspace and adds them in ascending order; db adds the rows r = p, p + P, ... in ascending r for p = 0 .. P - 1, then
 * the P sums left to right, P = 4 below 4096 rows and 256 from there on.  Exact on integer data whose partial sums stay below 2^24.  No allocation, no host read
 * (graph-capturable after one eager call per device, which raises the kernels' LDS limit). */
size_t odet_dense_grad_workspace_bytes(int wgrad, int rows, int cin, int cout);
int odet_dense_dgrad_f32(const float* dy, const float* w, const float* y_relu, const float* x_relu, float* dx, int rows, int cin,
                         int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream);
int odet_dense_wgrad_f32(const float* dy, const float* x, const float* y_relu, float* dw, float* db, int rows, int cin, int cout,
                         void* workspace, size_t workspace_bytes, odet_stream_t stream);

/* ---- 3x3 convolution backward, float32 (added within 103) ----------------------------------------------------------
 * The weight gradient of odet_conv3x3_f32_levels (a 3x3 stride-1 'same' convolution with shared weights over up to
 * ODET_MAX_LEVELS maps: the RpnHead over the pyramid, base_fpn_model.py:393-434) on the exact-float32 matrix instruction:
 *   dw[co][ky][kx][ci] = sum over levels, images, rows, columns of dz[b,y,x,co] * x[b, y+ky-1, x+kx-1, ci]  (taps outside the
 *   map are zero);   db[co] (nullable) = the same sum of dz[b,y,x,co].
 * A level is {x [batch,H,W,cin], dy [batch,H,W,cout], y_relu (nullable, the forward output, as dy), H, W}: the forward's own
 * contiguous NHWC float32 tensors; dw [cout][3][3][cin] is its weight layout.  dz = y_relu > 0 ? dy : 0 (a select, strict '>')
 * formed while staging, dy itself for a level without y_relu.  Nothing is transposed, copied or written but dw, db and the
 * workspace.  (The input gradient needs no entry point: it is the forward convolution of dz with the flipped, transposed
 * weight w'[ci][ky][kx][co] = w[co][2-ky][2-kx][ci].)
 * Rules (ODET_E_INVALID before any GPU work): the forward's -- 1..ODET_MAX_LEVELS levels, batch >= 1, H, W >= 1,
 * cin % 32 == 0, cout % 64 == 0, fewer than 2^31 - 2^16 pixels in all; pointers 16-byte aligned (db: 4).  ODET_E_WORKSPACE: a
 * workspace smaller than odet_conv3x3_wgrad_workspace_bytes (same levels' H and W; their pointers are not read) --
 * parts * cout * 9 * cin * 4 bytes when the launch cuts its contraction into parts > 1, else 0; 16-byte aligned, contents
 * arbitrary.
 * Order of sums: a function of (num_levels, every H and W, batch, cin, cout) alone, no atomics, every element written once.
 * The pixels of all levels are numbered through (levels in the order given; image, row, column); an element adds its products
 * in ascending pixel order, four per matrix instruction, inside each of `parts` equal runs of whole 32-pixel steps (as many as
 * bring the launch to 512 workgroups, at most 16, each at least 64 pixels, none below 256 pixels), and a second launch adds the
 * parts in ascending order.  db adds the pixels r = p, p + P, ... in ascending r for p = 0 .. P - 1, then the P sums left to
 * right, P = 4 below 4096 pixels in all and 256 from there on.  Exact on integer data whose partial sums stay below 2^24.  No allocation, no host read (graph-capturable after one
 * eager call per device, which raises the kernels' LDS limit). */
typedef struct {
  const void* x; const void* dy; const void* y_relu;
  int32_t H, W;
} odet_conv_grad_level_t;
size_t odet_conv3x3_wgrad_workspace_bytes(const odet_conv_grad_level_t* levels, int num_levels, int batch, int cin, int cout);
int odet_conv3x3_wgrad_f32_levels(const odet_conv_grad_level_t* levels, int num_levels, float* dw, float* db, int batch, int cin,
                                  int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream);
/* ---- Split-precision backward (added within 103) ---------------------------------------------------------------------
 * The three gradient contractions above on the bfloat16 matrix instruction, in the arithmetic of odet_conv3x3_x3_levels: every
 * float32 operand (dz after its ReLU gate included) is split in the kernel into three bfloat16 limbs whose sum is the
 * operand exactly, a product is six limb products, each exact in float32, added in float32 accumulators (dropped: three limb
 * products below 2^-23 of the product).  Same tensors, layouts, argument rules, error codes and error texts (under the entry
 * point's own name) as odet_dense_dgrad_f32 / odet_dense_wgrad_f32 / odet_conv3x3_wgrad_f32_levels; the workspace is sized by
 * the form's OWN queries (its split rule differs: K / parts >= 128).  db is not part of the form: it is the same
 * ordered float32 sum, bit-equal to the exact entry points'.  Order of sums: a function of the shapes alone, no atomics --
 * bit-equal from call to call; a K-step's 32 k are added inside one matrix instruction per limb product (inner order
 * undocumented), K-steps ascending, parts in ascending order.  Exact on data whose limb products and partial sums are
 * representable (integers below 2^8 in magnitude with sums below 2^24, among others).
 * odet_*_x3_plan: the launch a shape gets -- the workgroup tile's edge (64 or 128) and the number of parts -- from the same
 * shape rules as the entry points (ODET_E_INVALID on a shape they refuse), without any device call. */
size_t odet_dense_grad_x3_workspace_bytes(int wgrad, int rows, int cin, int cout);
int odet_dense_grad_x3_plan(int wgrad, int rows, int cin, int cout, int* tile_edge, int* parts);
int odet_dense_dgrad_x3(const float* dy, const float* w, const float* y_relu, const float* x_relu, float* dx, int rows, int cin,
                        int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream);
int odet_dense_wgrad_x3(const float* dy, const float* x, const float* y_relu, float* dw, float* db, int rows, int cin, int cout,
                        void* workspace, size_t workspace_bytes, odet_stream_t stream);
size_t odet_conv3x3_wgrad_x3_workspace_bytes(const odet_conv_grad_level_t* levels, int num_levels, int batch, int cin, int cout);
int odet_conv3x3_wgrad_x3_plan(const odet_conv_grad_level_t* levels, int num_levels, int batch, int cin, int cout, int* tile_edge,
                               int* parts);
int odet_conv3x3_wgrad_x3_levels(const odet_conv_grad_level_t* levels, int num_levels, float* dw, float* db, int batch, int cin,
                                 int cout, void* workspace, size_t workspace_bytes, odet_stream_t stream);
/* The inverse of odet_rpn_pack_pair's index map, for the backward pass of the RpnHead's two 1x1 convolutions run as one
 * contraction: from d_scores [B,N,2] and d_deltas [B,N,4] (float32; image strides and the level's offsets in VALUES, as in
 * odet_rpn_pack_pair) the level's gradient level_grad [B * pixels, channels] of the PADDED pair output -- columns 0 .. 2A - 1
 * the score channels, 2A .. 6A - 1 the delta channels, 6A .. channels - 1 zeros (channels >= 6A).  Every element of level_grad
 * is written once; packing it again with a zero bias returns the inputs' slices. */
int odet_rpn_unpack_pair(const float* d_scores, long long scores_image_stride, long long scores_offset, const float* d_deltas,
                         long long deltas_image_stride, long long deltas_offset, long long pixels, int A, int B, int channels,
                         float* level_grad, odet_stream_t stream);

/* ---- RoI pooling backward, float32 (added within 103) --------------------------------------------------------------
 * The gradient of odet_roi_pool with respect to the float32 feature maps (TF r1.13 CropAndResizeGradImage and the max-pool
 * gradient), one image per call, any norm_mode x pool_mode the forward accepts; the boxes get no gradient.  crop = P
 * (POOL_NONE) or 2P; ty(r,i), tx(r,j) are the forward's own sample rows / columns (same normalisation, level clamp, count_dev
 * clamped to n, pad remap; an extrapolated sample never becomes an address).
 *   odet_roi_pool_argmax (POOL_MAX2): sel [n,P,P,C] uint8 -- which sample of each bin and channel the forward's max took: the
 *     first in the order (0,0),(0,1),(1,0),(1,1) that compares equal to the pooled value (the first-maximum rule of TF's and
 *     torch's max-pool gradients); 0..3 = 2*di+dj, 4 = none (an all-NaN bin; rows at or beyond the count).  levels = the maps.
 *   odet_roi_pool_backward: levels[i].data = dx of level i ([H,W,C] float32, written); dy [n,P,P,C]; sel required for
 *     POOL_MAX2, NULL otherwise.  Upstream per sample g = dy (NONE), dy * 0.25f (AVG2), dy for the selected sample only (MAX2).
 *     A sample inside the map adds wx * (wy * g) -- two float32 multiplies, a separate add, no FMA -- to up to four cells
 *     (wy = 1 - ty.lerp on ty.lo, ty.lerp on ty.hi; likewise wx); when lo == hi both are added.
 * Order of sums: dx[l][y][x][c] starts at +0.0f and receives its contributions in ascending (RoI r; sample row i; top before
 * bottom; sample column j; left before right), RoIs with r < count on level l only -- a function of the data's indices, no
 * atomics; bit-reproducible and restated on the CPU (tests/roi_grad_np.py).  Every element of every dx is written exactly once
 * (cells nothing taps: +0.0f); nothing is read from dx, no memset, no workspace.  dy rows at or beyond the count are ignored.
 * Errors, all before any HIP call: ODET_E_INVALID (null pointer, num_levels outside 1..ODET_MAX_LEVELS, C no multiple of 4,
 * unknown mode, sel against pool_mode, misaligned pointer: maps / dx / dy / rois 16 bytes, sel 4), ODET_E_LIMIT (n > 8192,
 * pool_size > 16, a level of 2 GiB or more).  n == 0: argmax is a no-op, backward writes zeros.  No allocation, no host read
 * (graph-capturable). */
int odet_roi_pool_argmax(const odet_level_t* levels, int num_levels, int C, const float* rois, const int32_t* roi_level, int n,
                         const int32_t* count_dev, int norm_mode, int image_h, int image_w, int pool_size, uint8_t* sel,
                         odet_stream_t stream);
int odet_roi_pool_backward(const odet_level_t* levels, int num_levels, int C, const float* rois, const int32_t* roi_level, int n,
                           const int32_t* count_dev, int norm_mode, int image_h, int image_w, int pool_size, int pool_mode,
                           const float* dy, const uint8_t* sel, odet_stream_t stream);

/* ---- RoI pooling over a batch of images, float32 (added within 103) -------------------------------------------------
 * B images in one call, dense and strided: levels[i].data = the base of a contiguous [B,H,W,C] tensor (the maps; for the
 * backward, dx); rois [B,n,4]; roi_level int32 [B,n] (nullable with one level); count_dev int32 [B] (nullable: every image has
 * n RoIs); out / dy float32 [B,n,P,P,C]; sel uint8 [B,n,P,P,C].  The images share the level shapes, n, P, the modes and the
 * image shape; image offsets are size_t, and the 2 GiB limit of a level holds per image.  Image b's out, sel and dx are, bit
 * for bit, what odet_roi_pool, odet_roi_pool_argmax and odet_roi_pool_backward give on image b alone (the order of sums
 * above, per image).
 *   odet_roi_pool_images: the forward's own batched launch, ODET_MAX_BATCH (8) images per launch -- ceil(B / 8) launches.
 *   odet_roi_pool_argmax_images: ONE launch, a wave per (image, RoI, output row); rows at or beyond count_dev[b] get 4.
 *   odet_roi_pool_backward_images: ONE launch of B x the single-image call's workgroups, the image the slowest index; a
 *     workgroup walks the RoIs of its own image only (r < count_dev[b]), so its serial depth does not grow with B.  Every
 *     element of every image's dx is written once, also where count_dev[b] == 0 (zeros).
 *   odet_roi_pool_backward_images_plan: host only, no device call -- the launch odet_roi_pool_backward_images makes for these
 *     shapes (levels[i].H / W; data and stride are not looked at): *grid = B * *tiles_per_image workgroups of one wave,
 *     tiles_per_image = the sum over levels of H * ceil(W / 32) * ceil(C / 256), level_start[num_levels] = the first workgroup
 *     of each level among an image's, *slices = ceil(C / 256), *lds_bytes = min(Wmax, 32) * min(C, 256) * 4 <= 32768.  The
 *     launcher sizes its launch with the same code.
 * Errors, all before any HIP call: those of the single-image entry points with the same rules (alignment: of the base
 * pointers; C % 4 == 0 keeps every image's offset 16-byte aligned; odet_roi_pool_images also wants out 16-byte aligned), and
 * ODET_E_INVALID for B < 1, ODET_E_LIMIT for B > 64 and for a grid of 2^31 workgroups or more.  n == 0: the forward and argmax
 * are no-ops, the backward writes zeros.  No allocation, no host read (graph-capturable). */
int odet_roi_pool_images(const odet_level_t* levels, int num_levels, int C, int B, const float* rois, const int32_t* roi_level,
                         int n, const int32_t* count_dev, int norm_mode, int image_h, int image_w, int pool_size, int pool_mode,
                         float* out, odet_stream_t stream);
int odet_roi_pool_argmax_images(const odet_level_t* levels, int num_levels, int C, int B, const float* rois,
                                const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode, int image_h, int image_w,
                                int pool_size, uint8_t* sel, odet_stream_t stream);
int odet_roi_pool_backward_images(const odet_level_t* levels, int num_levels, int C, int B, const float* rois,
                                  const int32_t* roi_level, int n, const int32_t* count_dev, int norm_mode, int image_h,
                                  int image_w, int pool_size, int pool_mode, const float* dy, const uint8_t* sel,
                                  odet_stream_t stream);
int odet_roi_pool_backward_images_plan(const odet_level_t* levels, int num_levels, int C, int B, int n, int pool_size, int* grid,
                                       int* tiles_per_image, int* level_start, int* slices, int* lds_bytes);

#ifdef __cplusplus
}
#endif
#endif /* ODET_H_ */
