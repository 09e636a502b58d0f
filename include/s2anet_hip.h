/* ============================================================================
 * s2anet_hip.h — C ABI of libs2anet_hip.so: the S2ANet dense-inference hot path
 * as hand-written HIP kernels for MI355X (gfx950, wave64).
 *
 * This is the drop-in boundary: every entry point replaces one
 * function of the reference's six pybind11 extension modules and takes plain
 * device pointers and sizes — no torch types.  All pointers are DEVICE pointers
 * unless a parameter is named host_*; every call is asynchronous on `stream`
 * (a hipStream_t passed as void*) unless documented otherwise.  Tensors are
 * dense row-major ("contiguous") like the reference requires
 * (models/utils.py:51-56, deform_conv_cuda.cpp:168-170).
 *
 * Return value: 0 on success, negative S2A_E* on error; s2a_last_error() gives
 * the message (thread-local).  The reference raises c10::Error -> RuntimeError
 * for the same conditions (deform_conv_cuda.cpp:62-150, nms_rotated_cuda.cu:80-82);
 * the Python host side maps S2A_E* back to RuntimeError.
 *
 * Workspaces: ops that need scratch take (workspace, workspace_bytes); query the
 * size with the matching *_workspace_bytes() (0: the sizes are ones the op refuses).
 * Exactly that many bytes suffice; their contents on entry are arbitrary (nothing
 * needs zeroing) and no result depends on them; nothing outside them is written;
 * fewer bytes, or a NULL workspace, return S2A_EWORKSPACE before the first launch
 * (tests/test_gpu_workspace_contract.py).  Nothing in this library calls
 * hipMalloc/hipFree/hipDeviceSynchronize on the hot path, so every launch
 * sequence is hipGraph-capturable; the only host synchronisations are the
 * explicitly documented `host_count` read-backs of the reference-shaped NMS calls.
 * ==========================================================================*/
#ifndef S2ANET_HIP_H_
#define S2ANET_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define S2A_OK 0
#define S2A_EINVAL (-1)      /* bad shape / argument (reference: TORCH_CHECK / AT_ERROR) */
#define S2A_EWORKSPACE (-2)  /* workspace too small */
#define S2A_EHIP (-3)        /* HIP runtime error (launch failure, ...) */
#define S2A_ENOTIMPL (-4)

#define S2A_DTYPE_F32 0
#define S2A_DTYPE_F16 1
#define S2A_DTYPE_F64 2 /* ARF forward / backward (AT_DISPATCH_FLOATING_TYPES, ActiveRotatingFilter_cuda.cu:104,149) and the generic
                           deformable convolution + its three backward kernels (deform_conv_cuda_kernel.cu:258,352,450) */

#define S2A_LAYOUT_NCHW 0 /* reference layout (contiguous NCHW) */
#define S2A_LAYOUT_NHWC 1 /* channels-last storage of the same logical tensor */

typedef void* s2a_stream_t; /* hipStream_t */

const char* s2a_last_error(void);
const char* s2a_version(void);

/* ---------------------------------------------------------------------------
 * Deterministic training mode: one process-wide atomic flag, off by default; the environment switch S2A_DETERMINISTIC
 * (anything but empty or "0") sets its initial value.  s2a_set_deterministic returns the previous value.  The flag is read
 * when a call is ISSUED: a captured graph keeps the mode it was captured in.  Off: nothing anywhere differs.  On:
 *   * the f16 fused input gradient of the deformable convolution (s2a_deform_conv_backward_typed / s2a_deform_conv_backward
 *     with S2A_DTYPE_F16, s2a_deform_conv_backward_input_f16) sums into 64-bit FIXED-POINT cells instead of f32 atomics:
 *     every contribution v enters as rint(v * 2^32) through one 64-bit integer atomic add, so the sum does not depend on the
 *     order the workgroups arrive in.  Quantum 2^-32 (below 1/256 of the smallest f16 subnormal; n contributions are off
 *     by at most n * 2^-33; the cell is then read as a double -- exact for |sum| < 2^21 -- and rounded once to f16, or
 *     added to the f32 gradInput in double and rounded to f32).  Finite range |v| < 2^20
 *     (sixteen times the f16 maximum); a cell cannot overflow below 2048 contributions of that magnitude (in general while
 *     the sum of |v| over a cell's contributions stays below 2^31).  A contribution that is NaN, infinite or at / beyond the
 *     range stays out of the integer sum and is recorded in a sticky class byte per cell: only +inf (or v >= 2^20) seen ->
 *     +inf, only -inf (or v <= -2^20) -> -inf, anything else -> NaN; a cell no such contribution reached is bit-equal to
 *     the same call without it.  Cells and class bytes (9 bytes per gradInput element instead of 4) come out of the
 *     workspace: the *_workspace_bytes queries of these entries answer for the mode that is on when they are called;
 *   * the f32 fused input gradient (s2a_deform_conv_backward_input_f32, the S2A_DTYPE_F32 forms with a grad_input) and
 *     s2a_deformable_col2im add floats straight into the caller's tensor and have no deterministic form: they return
 *     S2A_EINVAL with a message naming the mode, before any launch.  Weight-only calls are unaffected (no atomics).
 * Scope: bit-equal results from run to run on one device type (the weight gradients' split depends on the CU count). */
int s2a_set_deterministic(int on);
int s2a_get_deterministic(void);

/* ---------------------------------------------------------------------------
 * Rotated-box IoU.  Replaces  utils.box_iou_rotated.box_iou_rotated_cuda.box_iou_rotated
 * (utils/box_iou_rotated/src/box_iou_rotated.h:22-42, kernel box_iou_rotated_cuda.cu:14-101).
 * boxes1[N,5], boxes2[M,5] f32 (x_ctr,y_ctr,w,h,angle_rad) -> ious[N,M] f32.
 * Arithmetic follows the reference's __CUDACC__ branch of box_iou_rotated_utils.h
 * operation-for-operation (no FMA contraction).  N==0 or M==0 is a no-op.
 * ------------------------------------------------------------------------- */
size_t s2a_box_iou_rotated_workspace_bytes(int64_t n, int64_t m);
int s2a_box_iou_rotated(const float* boxes1, int64_t n, const float* boxes2, int64_t m,
                        float* ious, void* workspace, size_t workspace_bytes,
                        s2a_stream_t stream);

/* element-wise variant (pairs i<->i), used by tests and by the merge path */
int s2a_box_iou_rotated_pairs(const float* boxes1, const float* boxes2, int64_t n, float* ious,
                              s2a_stream_t stream);

/* polyiou.iou_poly (DOTA_devkit/polyiou/csrc/polyiou.cpp:108-128; SWIG module `polyiou`), element-wise
 * over n pairs of quadrilaterals: polys[n,8] f64 (x1,y1,...,x4,y4) -> ious[n] f64.  Double precision,
 * same operation order as the reference (bit-identical to it on the tested inputs). */
int s2a_polyiou_pairs(const double* polys1, const double* polys2, int64_t n, double* ious,
                      s2a_stream_t stream);

/* The search inside voc_eval (DOTA_devkit/dota_evaluation_task1.py:204-263): for every detection polygon
 * dets8[d] (8 doubles) of image det_image[d], the ground-truth polygon gts8[g], g in
 * [gt_offsets[img], gt_offsets[img+1]), with the largest iou_poly(GT, det) among those whose axis-aligned boxes
 * overlap it (:222-246) -> ovmax[d] (-inf when none) and argmax[d] (index into gts8, -1 when none; first maximum). */
int s2a_polyiou_match(const double* dets8, const int32_t* det_image, int64_t num_dets, const double* gts8,
                      const int64_t* gt_offsets, int64_t num_images, double* ovmax, int64_t* argmax,
                      s2a_stream_t stream);

/* Label assignment of the training side, fused: assign_labels(anchors[M,5], gt_boxes[N,5], imgs_size, pos_iou_thr,
 * neg_iou_thr, min_pos_iou_thr, gt_max_assign_all, filter_invalid_anchors, filter_invalid_ious)
 * (models/utils.py:33-147) -> assign_gt_ids[M] int64 (-2 ignore, -1 negative, >= 0 the gt index).  The
 * [M,N] IoU matrix of bbox_iou_rotated (utils/metrics.py:85-107) lives in the workspace only (same pipeline and
 * values as s2a_box_iou_rotated); three streaming passes over it replace the reference's tensor ops and its
 * Python loop over the gts.  Row arg-max ties: first index. */
size_t s2a_assign_labels_workspace_bytes(int64_t num_anchors, int64_t num_gts);
int s2a_assign_labels(const float* anchors, int64_t num_anchors, const float* gt_boxes, int64_t num_gts,
                      float img_h, float img_w, float pos_iou_thr, float neg_iou_thr, float min_pos_iou_thr,
                      int gt_max_assign_all, int filter_invalid_anchors, int filter_invalid_ious,
                      int64_t* assign_gt_ids, void* workspace, size_t workspace_bytes, s2a_stream_t stream);

/* The same assignment for a whole batch and several anchor sets in ONE fixed launch sequence, with the image sort of
 * the targets done on the device: no host read, no allocation, and a launch sequence and geometry that depend on the
 * host arguments only, so the call can be captured into a graph and replayed against new targets.
 *
 *   sets[num_sets]   1 to 4 anchor sets of num_anchors anchors each; batch_stride (floats between two images' anchors) is
 *                    0 for anchors shared by all images (the FAM grid anchors [A,5]) or >= 5 * A for per-image anchors
 *                    (the ODM refined anchors [B,A,5]: A * 5)
 *   targets          f32 [target_capacity,7] = (image, class, x, y, w, h, angle), px / rad, in ANY order.  The first
 *                    *num_targets rows take part (num_targets: device scalar; NULL = all rows); a row whose image index
 *                    (int64)targets[i,0] is outside [0, batch) is dropped, so such rows pad a static table
 *   sorted_targets   [target_capacity,7]: the rows that take part, stably sorted by image (bit-equal to
 *                    t[argsort(image, stable)]: rules 1 and 3 depend on the gt order); the rows behind them are zero.
 *                    Must not alias targets
 *   target_offsets   int64 [batch+1]: first sorted row of image b; [batch] = number of real rows
 *   assign_ids       int64 [num_sets, batch, num_anchors]: s2a_assign_labels of (set, image) against that image's gts, the
 *                    gt index counted within the image (what s2a_s2anet_loss_forward reads); an image without gts: valid
 *                    anchors -1, the others -2.  Needs min_pos_iou_thr >= 0 and pos_iou_thr > 0
 *   status           int64 [4]: [0] bit 0 = the pair list was too small (the ids are unspecified then, every write still
 *                    stays inside the outputs), bit 1 = a per-image limit was exceeded (reserved: this implementation
 *                    has none and never sets it); [1] = candidate pairs found, i.e. the pair_capacity a second call
 *                    needs; [2] = real target rows; [3] = 0
 *   pair_capacity    entries of the one pair list all (set, image) problems share (anchor-gt pairs that survive the circle
 *                    and separating-axis tests); num_sets * num_anchors * target_capacity can never overflow
 * workspace: s2a_assign_labels_batched_workspace_bytes of the same sizes (0 for sizes the call refuses), 16-byte aligned. */
typedef struct s2a_anchor_set {
  const float* anchors;
  int64_t batch_stride;
} s2a_anchor_set;
size_t s2a_assign_labels_batched_workspace_bytes(int64_t num_sets, int64_t batch, int64_t num_anchors,
                                                 int64_t target_capacity, int64_t pair_capacity);
int s2a_assign_labels_batched(const s2a_anchor_set* sets, int num_sets, int64_t batch, int64_t num_anchors,
                              const float* targets, int64_t target_capacity, const int64_t* num_targets, float img_h,
                              float img_w, float pos_iou_thr, float neg_iou_thr, float min_pos_iou_thr,
                              int gt_max_assign_all, int filter_invalid_anchors, int filter_invalid_ious,
                              int64_t* assign_ids, float* sorted_targets, int64_t* target_offsets, int64_t* status,
                              int64_t pair_capacity, void* workspace, size_t workspace_bytes, s2a_stream_t stream);

/* Chip-merge polygon NMS: py_cpu_nms_poly_fast(dets[n,9] f64 = 8 polygon coordinates + score, thresh)
 * (DOTA_devkit/ResultMerge_multi_process.py:62-123) entirely on the device.  keep[] (n int64) receives
 * the surviving original indices in descending-score order, *count_dev their number; host_count as in
 * s2a_nms_rotated.  Score ties: ascending index. */
size_t s2a_nms_poly_workspace_bytes(int64_t n);
int s2a_nms_poly(const double* dets9, int64_t n, double thresh, int64_t* keep, int64_t* count_dev,
                 int64_t* host_count, void* workspace, size_t workspace_bytes, s2a_stream_t stream);

/* ---------------------------------------------------------------------------
 * Rotated NMS.  Replaces
 *   utils.nms_rotated.nms_rotated_cuda.nms_rotated(dets[N,5], scores[N], thr) -> int64[K]
 *     (utils/nms_rotated/src/nms_rotated.h:21-41, nms_rotated_cuda.cu:14-133)
 *   utils.ml_nms_rotated.ml_nms_rotated_cuda.ml_nms_rotated(dets, scores, labels, thr)
 *     (utils/ml_nms_rotated/src/nms_rotated.h:23-44, nms_rotated_cuda.cu:14-137)
 * Semantics of the reference GPU op: sort by score descending, suppress j by a kept,
 * higher-scored i when iou(i,j) > thr (strict), IoU == 0 across different labels;
 * keep[] = indices into the ORIGINAL order, in descending-score order.
 * Ties in score are broken by ascending original index (the reference leaves them to
 * torch's unstable sort).
 *
 * Everything — sort, pair finding, exact IoU, greedy resolution, compaction — runs on the
 * device; the reference's N x N/64 mask and its device->host copy (cuda.cu:109) do not exist here:
 * suppressing pairs are kept as a list.  s2a_nms_rotated_workspace_bytes() sizes the lists for
 * dense inputs.  The two ops declared here take (n, n).  The segmented forms below accept a SMALLER one, down to
 * s2a_nms_rotated_workspace_bytes(n, 1) (they are not told the max_segment_rows a caller sized for, so that is the
 * bound they check): a call whose lists fill up finishes on a slower memory-free kernel with the same keep list.
 * Speed limit of the label handling (results are unaffected): inputs of more than 4 096 rows per label are ordered
 * spatially by an own counting sort whose tables hold at most 8 192 DISTINCT labels and 65 536 (label, cell) buckets;
 * beyond either the same memory-free kernel settles the call -- exact, but an order of magnitude slower (12 000 distinct
 * labels at n = 9 000 are tested for the keep list, tests/test_gpu_ops.py::test_nms_order_b_counting_sort_labels_of_any_kind).
 * The reference's use (utils/bbox_nms_rotated.py:47: labels = class ids, 15 for DOTA) is far inside the limit.
 * labels may be NULL (single class).  keep must hold n int64.  *count_dev (device
 * int64) receives K; if host_count != NULL the call synchronises the stream once and
 * stores K there (the reference call shape needs K on the host to size its result).
 * ------------------------------------------------------------------------- */
size_t s2a_nms_rotated_workspace_bytes(int64_t n, int64_t max_segment_rows);
int s2a_ml_nms_rotated(const float* dets, const float* scores, const float* labels, int64_t n,
                       float iou_threshold, int64_t* keep, int64_t* count_dev,
                       int64_t* host_count, void* workspace, size_t workspace_bytes,
                       s2a_stream_t stream);
int s2a_nms_rotated(const float* dets, const float* scores, int64_t n, float iou_threshold,
                    int64_t* keep, int64_t* count_dev, int64_t* host_count, void* workspace,
                    size_t workspace_bytes, s2a_stream_t stream);

/* Synchronous calls (host_count != NULL) of the two ops above on at most 16 384 rows are settled by ONE kernel launch when the
 * labels split the rows into at most 64 segments of at most 640 rows and at most 4 096 pairs survive the cull of a segment;
 * otherwise -- and always for host_count == NULL -- by the general multi-launch path (same keep list either way, tested).
 * Counters of the two outcomes since the library was loaded (diagnostic; tests assert that the small path really ran). */
int s2a_nms_small_stats(int64_t* taken, int64_t* fell_back);

/* The same two ops on float64 boxes.  The reference dispatches the NMS kernels on the dtype of `dets`
 * (AT_DISPATCH_FLOATING_TYPES_AND_HALF, utils/nms_rotated/src/nms_rotated_cuda.cu:95-100,
 * utils/ml_nms_rotated/src/nms_rotated_cuda.cu:100-105; AT_DISPATCH_FLOATING_TYPES in the CPU files): on double boxes it
 * evaluates single_box_iou_rotated<double>, and keep decisions next to the threshold differ from the float32 evaluation.
 * dets[n,5], scores[n], labels[n] (NULL: single class) float64; the threshold stays a float as in the reference's
 * signature.  A plain N x N/64 mask form (API completeness, not a hot path): n < 260 k.  Not HIP-graph capturable. */
size_t s2a_nms_rotated_f64_workspace_bytes(int64_t n);
int s2a_nms_rotated_f64(const double* dets, const double* scores, const double* labels, int64_t n,
                        float iou_threshold, int64_t* keep, int64_t* count_dev, int64_t* host_count,
                        void* workspace, size_t workspace_bytes, s2a_stream_t stream);

/* Batched form used by the detector (one call for a whole batch of images):
 * segment_ids[n] int32 in [0, num_segments) — NMS runs independently inside each
 * segment (segment = image*num_classes + label); a NEGATIVE segment id marks a padding row
 * that is ignored (never compared, never kept; lets callers use static-size buffers); group_ids[n] int32 in [0,num_groups)
 * (group = image) decides the output grouping: keep_flags[n] uint8 (1 = survives) and,
 * if keep != NULL, per-group lists keep[g*max_per_group + r] (int32 original index, score
 * descending, -1 padded) with group_counts[g] = min(K_g, max_per_group).
 * No host synchronisation. */
int s2a_nms_rotated_segmented(const float* dets, const float* scores, const int32_t* segment_ids,
                              const int32_t* group_ids, int64_t n, int32_t num_segments,
                              int32_t num_groups, float iou_threshold, uint8_t* keep_flags,
                              int32_t* keep, int32_t* group_counts, int32_t max_per_group,
                              void* workspace, size_t workspace_bytes, s2a_stream_t stream);

/* s2a_nms_rotated_segmented followed, in the same launch sequence, by the output assembly of
 * multiclass_nms_rotated (utils/bbox_nms_rotated.py:47-64: dets = cat([bboxes, scores[:, None]]), labels, sorted by
 * score, cut to max_per_img) for a whole batch — no host synchronisation, no stock tensor ops behind the NMS:
 *   wire[g][r*7 .. r*7+6] = x, y, w, h, angle, score, label (as float) of the r-th kept row of group g in
 *   descending-score order; rows behind the last kept one are 0,0,0,0,0,0,-1; wire[g][max_per_group*7] = the number
 *   of rows written = min(K_g, max_per_group).  wire is float32 [num_groups][max_per_group*7 + 1]: also the
 *   all-gather wire format of the data-parallel detector (one buffer per rank, s2anet_amd/gather.py).
 *   labels_out int32 [num_groups][max_per_group] (-1 padded) and counts_out int32 [num_groups]: optional copies.
 * row_labels[n] int32 = class of every row (out_cls of s2a_multiclass_candidates).
 * cand_found (device int64, may be NULL) = the untruncated candidate count of s2a_multiclass_candidates whose first
 * n rows these are.  Rows at or behind min(*cand_found, n) are PADDING by contract: they are never kept and (on every
 * internal path) never take part in a comparison, whatever their segment id -- a caller that passes a smaller count
 * than it filled rows cuts its own input.  overflow_out (device int64[2], may be NULL) receives [found, found - n clamped at 0] and
 * *dropped_total (device int64, may be NULL) is incremented by the second number (the reference never drops a
 * candidate, so a caller with a static row cap must be able to prove that nothing was cut). */
int s2a_nms_rotated_segmented_dets(const float* dets, const float* scores, const int32_t* segment_ids,
                                   const int32_t* group_ids, const int32_t* row_labels, int64_t n,
                                   int32_t num_segments, int32_t num_groups, float iou_threshold,
                                   int32_t max_per_group, float* wire, int32_t* labels_out,
                                   int32_t* counts_out, const int64_t* cand_found, int64_t* overflow_out,
                                   int64_t* dropped_total, void* workspace, size_t workspace_bytes,
                                   s2a_stream_t stream);

/* Candidate selection of multiclass_nms_rotated (utils/bbox_nms_rotated.py:29-42) for a whole
 * batch: every (box, class) pair with score > score_thr, in row-major (image, box, class) order,
 * compacted into `cap` slots (first `cap` in that order if there are more; *count_dev holds the
 * untruncated count).  boxes[batch*n,5], scores[batch*n*num_classes] f32.  Unused slots become
 * padding rows: out_seg = out_grp = out_cls = -1, score -1 (ignored by
 * s2a_nms_rotated_segmented).  out_seg = image*num_classes + class, out_grp = image. */
size_t s2a_multiclass_candidates_workspace_bytes(int64_t total_scores);
int s2a_multiclass_candidates(const float* boxes, const float* scores, int64_t batch, int64_t n,
                              int64_t num_classes, float score_thr, int64_t cap, float* out_boxes,
                              float* out_scores, int32_t* out_seg, int32_t* out_grp, int32_t* out_cls,
                              int64_t* count_dev, void* workspace, size_t workspace_bytes,
                              s2a_stream_t stream);

/* ---------------------------------------------------------------------------
 * ORN.  Replaces  models.orn.orn_cuda.arf_forward(weight[O,I,nOri,kH,kW], indices u8
 * [nOri,kH,kW,nRot]) -> [O*nRot, I*nOri, kH, kW]
 * (models/orn/src/vision.cpp:7-12, cuda/ActiveRotatingFilter_cuda.cu:20-46,79-119).
 * dtype F32 or F16 (element size only matters: the op is a permuting copy).
 * ------------------------------------------------------------------------- */
int s2a_arf_forward(const void* weight, const uint8_t* indices, int64_t n_out, int64_t n_in,
                    int n_orientation, int kh, int kw, int n_rotation, int dtype, void* output,
                    s2a_stream_t stream);

/* orn_cuda.arf_backward(indices, gradOutput[O*nRot, I*nOri, kH, kW]) -> gradInput[O,I,nOri,kH,kW]
 * (models/orn/src/vision.cpp:9, cuda/ActiveRotatingFilter_cuda.cu:49-76,122-162): sum over the nRot
 * rotated copies, ascending k.  float32 (the reference dispatches float/double only). */
int s2a_arf_backward(const uint8_t* indices, const void* grad_output, int64_t n_out, int64_t n_in,
                     int n_orientation, int kh, int kw, int n_rotation, int dtype, void* grad_input,
                     s2a_stream_t stream);

/* orn_cuda.rie_forward(feature[B,C,1,1], nOrientation) -> (mainDirection uint8[B,C/nOri], aligned[B,C,1,1]) and
 * orn_cuda.rie_backward(mainDirection, gradOutput[B,C,1,1], nOrientation) -> gradInput (models/orn/src/vision.cpp:10-11,
 * RotationInvariantEncoding.h:11-34, cuda/RotationInvariantEncoding_cuda.cu:20-84): main direction = first index of
 * the strict maximum of each group of nOri values, group rotated so that it comes first; backward rotates back.
 * float32.  Not used by the S2ANet model itself (exported by the module the model imports). */
int s2a_rie_forward(const void* feature, int64_t batch, int64_t channels, int n_orientation, int dtype,
                    uint8_t* main_direction, void* aligned, s2a_stream_t stream);
int s2a_rie_backward(const uint8_t* main_direction, const void* grad_output, int64_t batch, int64_t features,
                     int n_orientation, int dtype, void* grad_input, s2a_stream_t stream);

/* RotationInvariantPooling.forward (models/orn/functions/rotation_invariant_pooling.py:19-27):
 * x[B,C,H,W] -> out[B,C/nOri,H,W] = max over each group of nOri consecutive channels. */
int s2a_rot_inv_pool(const void* x, int64_t batch, int64_t channels, int64_t hw, int n_orientation,
                     int dtype, int layout, void* out, s2a_stream_t stream);
/* Its backward: grad_input[B,C,H,W] (every element written) = grad_output[B,C/nOri,H,W] at the maximal orientation of
 * each group of x (the lowest index on a tie, as torch.max(dim)), 0 elsewhere.  x, grad_output and grad_input share
 * dtype (f32 / f16) and layout (S2A_LAYOUT_NCHW / S2A_LAYOUT_NHWC). */
int s2a_rot_inv_pool_backward(const void* x, const void* grad_output, int64_t batch, int64_t channels, int64_t hw,
                              int n_orientation, int dtype, int layout, void* grad_input, s2a_stream_t stream);

/* ---------------------------------------------------------------------------
 * Deformable convolution v1 forward.  Replaces
 *   models.dcn.deform_conv_cuda.deform_conv_forward_cuda(input, weight, offset, output,
 *       columns, ones, kW, kH, dW, dH, padW, padH, dilationW, dilationH, group,
 *       deformable_group, im2col_step) -> int
 * (models/dcn/src/deform_conv_cuda.cpp:152-260; sampling kernel
 *  deform_conv_cuda_kernel.cu:83-114,189-242).  The reference's `columns` / `ones`
 * scratch tensors and im2col_step have no counterpart: sampling and the channel
 * contraction are fused (no columns buffer).  Argument order keeps the reference's
 * W-before-H convention.
 *   input  [B,C,H,W]                 dtype, `layout` storage
 *   weight [O, C/group, kH, kW]      dtype, contiguous
 *   offset [B, dg*2*kH*kW, Ho, Wo]   F32 (or dtype when offset_dtype says so), NCHW;
 *                                    channel 2t = dy, 2t+1 = dx of tap t (kernel.cu:221-222)
 *   output [B,O,Ho,Wo]               dtype, `layout` storage, caller-allocated
 * relu != 0 fuses AlignConv's ReLU (models/alignconv.py:97).
 *
 * NaN and the fused ReLU, for EVERY `relu` argument of this header (deform / align convolutions, s2a_bias_act_nhwc,
 * s2a_conv_nhwc_f16 and the pyramid, chain and tail launches built on it): the epilogue is max(v, 0) with the
 * hardware's rule, which returns 0 for a NaN; +-inf keep their class (relu(-inf) = 0).  That is the inference
 * contract.  A caller that needs torch's ReLU (NaN stays NaN), as training under a loss scale does, launches with
 * relu = 0 and applies the ReLU itself; s2anet_amd's autograd functions do exactly that.  The backward entries
 * (s2a_conv_backward_prep_f16) mask with out <= 0, so a gradient passes at a NaN output.
 * ------------------------------------------------------------------------- */
typedef struct s2a_dcn_params {
  int64_t batch, channels, height, width, out_channels;
  int kW, kH, dW, dH, padW, padH, dilationW, dilationH, group, deformable_group;
  int dtype;        /* S2A_DTYPE_* of input/weight/output */
  int offset_dtype; /* S2A_DTYPE_* of the offset tensor */
  int layout;       /* S2A_LAYOUT_* of input and output */
  int relu;
} s2a_dcn_params;

size_t s2a_deform_conv_workspace_bytes(const s2a_dcn_params* p);
int s2a_deform_conv_forward(const void* input, const void* weight, const void* offset,
                            void* output, const s2a_dcn_params* p, void* workspace,
                            size_t workspace_bytes, s2a_stream_t stream);

/* deform_conv_cuda.modulated_deform_conv_cuda_forward (models/dcn/src/deform_conv_cuda.cpp:491-570, kernel
 * deform_conv_cuda_kernel.cu:467-632; DCNv2): as s2a_deform_conv_forward with every sampled value multiplied by
 * mask[B, dg*kH*kW, Ho, Wo] and bias[O] (may be NULL) added after the contraction.  NCHW, any kernel size / stride /
 * padding / dilation / groups; offset and mask in the input's dtype.  One thread per output element (the S2ANet
 * model does not use this operator; it is exported by the module the model imports).  The backward is not built. */
int s2a_modulated_deform_conv_forward(const void* input, const void* weight, const void* bias, const void* offset,
                                      const void* mask, void* output, const s2a_dcn_params* p, s2a_stream_t stream);

/* AlignConv.get_offset (models/alignconv.py:30-87), batched: anchors[B,H*W,5] f32 (pixels,
 * radians) -> offset[B,2*k*k,H,W] f32 (k = 3). */
int s2a_align_offsets(const float* anchors, int64_t batch, int64_t height, int64_t width,
                      float stride, int ksize, float* offset, s2a_stream_t stream);

/* AlignConv.forward (models/alignconv.py:88-98) fully fused: refined anchors ->
 * sampling offsets (never materialised) -> bilinear sampling -> 3x3 contraction (MFMA)
 * -> ReLU.  x[B,C,H,W], anchors[B,H,W,5] f32, weight[O,C,3,3], out[B,O,H,W]. */
typedef struct s2a_align_params {
  int64_t batch, channels, height, width, out_channels;
  float stride;
  int dtype, layout, relu;
  int weight_packed; /* 1: `weight` is the output of s2a_dcn_pack_weight (cached by the caller at
                        inference, the weights do not change between forwards) */
} s2a_align_params;
size_t s2a_align_conv_workspace_bytes(const s2a_align_params* p);
/* weight[O,C,3,3] -> the layouts the fused kernels stream: stage-major [C/KC][9][O][KC]
 * (KC = 32 for f32, 64 for f16) and right behind it, for f16, a second copy in MFMA-fragment order; for f32, the filter split
 * into three bf16 planes, [C/16][9][plane][O][16] (hi + mid + lo = the f32 value exactly: the f32 forward runs on the 16-bit
 * matrix instruction, six plane products per f32 product -- the accuracy of f32 arithmetic for finite operands; an infinite
 * operand gives NaN where f32 arithmetic gives +-inf; S2A_DCN_F32=mfma32 selects the f32 instruction).
 * `packed` must hold s2a_dcn_packed_elems(O, C, dtype) elements (f16: 2 per weight, f32: 2.5 per weight). */
int64_t s2a_dcn_packed_elems(int64_t out_channels, int64_t channels, int dtype);
int s2a_dcn_pack_weight(const void* weight, int64_t out_channels, int64_t channels, int dtype,
                        void* packed, s2a_stream_t stream);
int s2a_align_conv_forward(const void* x, const float* anchors, const void* weight, void* out,
                           const s2a_align_params* p, void* workspace, size_t workspace_bytes,
                           s2a_stream_t stream);

/* ---------------------------------------------------------------------------
 * Head glue, batched and device-side.
 * s2a_delta2bbox_rotated: models/boxes.py:82-162 (is_encode_relative=True) + norm_angle
 *   (utils/general.py:925-929).  rois[n,5], deltas[n,5] f32 -> out[n,5].
 * s2a_fam_refine_anchors: gen_grid_anchors (models/anchors.py:75-126, 1 square anchor of
 *   side scale*stride per position) + fam_bbox_decode (models/head.py:27-52,
 *   wh_ratio_clip = 1e-6) straight from the NCHW/NHWC prediction map:
 *   bbox_pred[B,5,H,W] (dtype/layout) -> refined[B,H,W,5] f32.
 * ------------------------------------------------------------------------- */
/* level table of a pyramid-packed buffer (layout: see "Pyramid-packed head launches" below) */
typedef struct s2a_pyramid {
  int32_t n_levels;     /* 1..8 */
  int32_t height[8];
  int32_t width[8];
  float stride[8];      /* FPN stride of the level (AlignConv / anchor generation) */
} s2a_pyramid;

/* Candidate selection of get_bboxes for the whole batch on pyramid-packed predictions (models/head.py:684-717):
 * per level and image sigmoid -> max over classes -> top-k (max_per_level = 2000) only where H*W > k, levels
 * concatenated, final decode (wh_ratio_clip 16/1000).  cls[P,64] / reg[P,64] f16 (first num_classes / 5 columns),
 * anchors[P,5] f32 -> bboxes[B,n,5], scores[B,n,num_classes] f32 with n = s2a_pyramid_candidates_count; sel[B,n] int32
 * scratch receives the packed row of every candidate.  Ties at the k-th score: lowest positions first (the stock
 * top-k leaves them unspecified); candidates of a level come in position order.  Levels above 24576 positions that
 * need a top-k are refused (use the per-level path). */
int64_t s2a_pyramid_candidates_count(const s2a_pyramid* pyr, int64_t max_per_level);
int s2a_pyramid_candidates(const void* cls, const void* reg, const float* anchors, int64_t batch,
                           const s2a_pyramid* pyr, int num_classes, int64_t max_per_level, float wh_ratio_clip,
                           float* bboxes, float* scores, int32_t* sel, s2a_stream_t stream);

/* Output side (val.py:40-52): rotated_box_to_poly_single (utils/general.py:886-921) + cv2.boxPoints for a
 * whole batch: boxes rows (x,y,w,h,angle[,score...]) with row_stride floats -> polys[n,8] f32. */
int s2a_rbox_to_poly(const float* boxes, int64_t n, int64_t row_stride, float* polys, s2a_stream_t stream);
int s2a_delta2bbox_rotated(const float* rois, const float* deltas, int64_t n, float wh_ratio_clip,
                           float* out, s2a_stream_t stream);
int s2a_fam_refine_anchors(const void* bbox_pred, int64_t batch, int64_t height, int64_t width,
                           float stride, float anchor_scale, int dtype, int layout, float* refined,
                           s2a_stream_t stream);

/* ---- whole-scene detection: chips out of a device-resident scene, merged detections back (scene_ops.hip) ----
 *
 * Chip gather: replaces SplitSingle / saveimagepatches (DOTA_devkit/SplitOnlyImage_multi_process.py:39-49, :68-85).
 * scene uint8 [height,width,3] (HWC); origins int32 [n_chips,2] (left, up) on the device, any order, may reach past
 * the scene; chips uint8 [n_chips,subsize,subsize,3].  Pixels outside the scene are 0 (the np.zeros padding, :45-46).
 * One launch for all chips.  subsize % 16 == 0, chips 16-byte aligned, scene 4-byte aligned. */
int s2a_scene_gather_u8(const uint8_t* scene, int64_t height, int64_t width, const int32_t* origins, int64_t n_chips,
                        int32_t subsize, uint8_t* chips, s2a_stream_t stream);

/* Scene merge: replaces the text route val.py:40-52 -> mergesingle / poly2origpoly / nmsbynamedict
 * (DOTA_devkit/ResultMerge_multi_process.py:159-245) -> py_cpu_nms_poly_fast (:62-123), per class, for the chips of
 * one scene.  Input is the detector's padded output: dets f32 [n_chips,K,6] (x, y, w, h, theta, score; contiguous),
 * labels int32 [n_chips,K] (-1: no row), counts int32 [n_chips] (rows at or behind a chip's count are ignored),
 * origins int32 [n_chips,2] (left, up), rates f64 [n_chips] or NULL (= 1.0).  Per row: the float32 polygon of
 * rbox_to_poly widened to double, then (coordinate + origin) / rate in double (:178-185); rows are taken chip-major,
 * then in detection order; score ties: ascending row.  A row is kept iff no kept higher row OF ITS CLASS has
 * iou_poly > thresh (HBB prefilter :87-93).
 * Outputs (capacity n_chips*K rows each, all on the device): out_polys f64 [.,8], out_scores f64, out_labels int64,
 * out_src int64 (source row chip*K + k) -- compacted class-major, descending score inside a class; the rows behind
 * the kept total are cleared (0 / -1).  class_counts int64 [num_classes].  status int64 [4]: [0] != 0 <=> the
 * candidate pair list overflowed and THE OUTPUTS ARE NOT VALID, [1] candidate pairs found (run again with at least
 * that pair_capacity), [2] suppression edges, [3] real input rows.
 * pair_capacity <= 0: the default min(n(n-1)/2, max(32 n, 2^20)) + 1 with n = n_chips*K.  The workspace is
 * O(n + pair_capacity): no n x n / 64 mask.  No host synchronisation, no device-to-host copy, no memset node: the call
 * may be captured into a HIP graph. */
size_t s2a_scene_merge_workspace_bytes(int64_t n_rows, int64_t pair_capacity);
int s2a_scene_merge(const float* dets, const int32_t* labels, const int32_t* counts, const int32_t* origins,
                    const double* rates, int64_t n_chips, int64_t K, int32_t num_classes, double thresh,
                    int64_t pair_capacity, double* out_polys, double* out_scores, int64_t* out_labels,
                    int64_t* out_src, int64_t* class_counts, int64_t* status, void* workspace,
                    size_t workspace_bytes, s2a_stream_t stream);

/* ---- DOTA Task-1 evaluation of all classes on the device (eval_ops.hip) ----
 *
 * Replaces the loop of val.py:332-399: voc_eval (DOTA_devkit/dota_evaluation_task1.py:92-318) once per class, then the
 * max-F1 point of every curve (val.py:357-386).  Everything is on the device:
 *   detections    det_polys f64 [D,8], det_scores f64 [D], det_labels int32 [D], det_image int32 [D]
 *   ground truth  gt_polys f64 [G,8], gt_labels int32 [G], gt_image int32 [G], gt_difficult uint8 [G]
 * A row of either side is PADDING when its label is outside [0, num_classes) or its image is outside [0, num_images):
 * it is ignored and its polygon and score are never interpreted (NaN is harmless), so a static table or the detector's
 * -1 padded output is evaluated without compaction.
 * Order (:183 per class): class-major, descending score, equal scores (-0 == +0) by ascending input row.  Per detection
 * (:204-263): the first maximum of iou_poly(GT, det) over the ground truths of its class and image, in input order, that
 * pass the +1-pixel axis-aligned prefilter (:223-252) -- the values of s2a_polyiou_match.  TP/FP (:265-290) as a parallel
 * rule: a detection with ovmax > ovthresh whose ground truth is not a filtered difficult box QUALIFIES for it; of the
 * detections that qualify for one ground truth the first in the order is the TP, the others are FP; a match with a filtered
 * difficult box is neither; everything else is FP.  rec = tp / npos, prec = tp / max(tp + fp, eps) (:301-309), AP by the
 * 11-point rule (:62-70; thresholds11 = the 11 doubles of np.arange(0.0, 1.1, 0.1), a HOST array read during the call;
 * may be NULL when use_07_metric == 0) or the area rule (:72-88); f1 = 2 rec prec / (rec + prec + 1e-16), first maximum.
 * Outputs per class [num_classes]: ap, precision, recall, f1, conf (at the max-F1 point) f64; num_det_at_f1 (its index
 * + 1), npos (ground truths that count: all when is_filter_difficult == 0), ndet int64; valid uint8.
 *   - a class without detections reports zeros (:322) with num_det_at_f1 = 0;
 *   - a class with npos == 0 (the reference exits or divides by zero) reports zeros with valid = 0; otherwise valid = 1.
 * curves (may be NULL, and so may each member): one entry per position of the order, capacity D; entries behind the last
 * real detection are cleared (0, order / argmax -1).  order = source row, argmax = input ground-truth row or -1, ovmax =
 * -inf when no ground truth passed the prefilter, tp_cum / fp_cum / rec / prec = the class's curve, seg_start
 * [num_classes + 1] = first position of every class (last entry: number of real detections).
 * One fixed launch sequence: no host synchronisation, no device-to-host copy, no memset node -- the call may be captured
 * into a HIP graph.  Integer atomics only, every sum in a fixed order: two runs give the same bits.  Workspace
 * O(D + G + num_classes * num_images), no D x G array.  D, G < 2^31; num_classes <= 1024;
 * (num_classes + 1) * num_images < 2^31. */
typedef struct {
  int64_t* order;
  double* ovmax;
  int64_t* argmax;
  int64_t* tp_cum;
  int64_t* fp_cum;
  double* rec;
  double* prec;
  int64_t* seg_start;
} s2a_eval_curves;
size_t s2a_eval_task1_workspace_bytes(int64_t num_dets, int64_t num_gts, int32_t num_classes, int32_t num_images);
int s2a_eval_task1(const double* det_polys, const double* det_scores, const int32_t* det_labels, const int32_t* det_image,
                   int64_t num_dets, const double* gt_polys, const int32_t* gt_labels, const int32_t* gt_image,
                   const uint8_t* gt_difficult, int64_t num_gts, int32_t num_classes, int32_t num_images, double ovthresh,
                   int is_filter_difficult, int use_07_metric, const double* thresholds11, double* ap, double* precision,
                   double* recall, double* f1, double* conf, int64_t* num_det_at_f1, int64_t* npos, int64_t* ndet,
                   uint8_t* valid, const s2a_eval_curves* curves, void* workspace, size_t workspace_bytes,
                   s2a_stream_t stream);

/* Convolution epilogue for the conv layers of the head/carrier that MIOpen runs without fusion:
 * y[positions, channels] (channels-last storage) = act(y + bias[c] (+ residual)), in place.
 * Replaces the bias add / residual add / ReLU passes that follow every nn.Conv2d of
 * models/head.py:163-222 and models/backbone.py:37-83 (same arithmetic, one pass over HBM). */
int s2a_bias_act_nhwc(void* y, const void* bias, const void* residual, int64_t positions,
                      int64_t channels, int dtype, int relu, s2a_stream_t stream);
/* the same pass writing out[positions, channels] instead (out may equal y): lets the two library convolutions that
 * remain (FPN's stride-2 extra levels, models/neck.py:86-94) land in the pyramid-packed head buffer without a copy */
int s2a_bias_act_nhwc_to(const void* y, const void* bias, const void* residual, void* out, int64_t positions,
                         int64_t channels, int dtype, int relu, s2a_stream_t stream);

/* Regular convolutions, f16 channels-last, with bias / residual / ReLU fused — the conv towers of
 * S2ANetHead (models/head.py:163-222, nn.Conv2d + nn.ReLU pairs) and the 1x1 layers of the carrier,
 * on the same patch-staged MFMA structure as AlignConv.  ksize 3: pad 1, stride 1 or 2 (stride 2: O % 128 == 0).
 * ksize 1: pad 0, stride 1 or 2.  x[B,H,W,C] -> out[B,Ho,Wo,O] = relu?(conv(x) + bias (+ residual[B,Ho,Wo,O])).
 * The fused ReLU writes 0 for a NaN (see the note at s2a_dcn_params); relu = 0 hands every value on as it is.
 * weight_frag = s2a_conv_pack_weight_f16 of the [O,C,k,k] filter (O*C*k*k halfs, MFMA-fragment order);
 * bias[O] f16 or NULL; residual or NULL.  O must be a multiple of 64 (narrower heads: zero-pad the
 * filter), C a multiple of 64 or exactly 32 (then the filter given to s2a_conv_pack_weight_f16 is
 * zero-padded to 64 input channels). */
int s2a_conv_pack_weight_f16(const void* weight, int64_t out_channels, int64_t channels, int ksize,
                             void* packed, s2a_stream_t stream);
int s2a_conv_nhwc_f16(const void* x, const void* weight_frag, const void* bias, const void* residual,
                      void* out, int64_t batch, int64_t channels, int64_t height, int64_t width,
                      int64_t out_channels, int ksize, int stride, int relu, s2a_stream_t stream);
/* the k_conv_f16<TAPS, OG, PH, SD, TAIL, HT> that s2a_conv_nhwc_f16 would launch for these sizes now (the tile-shape
   switches are read from the environment as the call reads them) -> form[6].  No HIP call, no device needed.
   S2A_EINVAL with the entry point's own text for sizes it refuses (a call with a residual also refuses an output of
   2^31 bytes or more; the query takes no residual and answers as a call without one).  batch 0: the form of the sizes. */
int s2a_conv_nhwc_f16_form(int64_t batch, int64_t channels, int64_t height, int64_t width,
                           int64_t out_channels, int ksize, int stride, int32_t form[6]);

/* Training side of the regular convolutions above (FusedConv2d with own_grad; stride 1, ksize 3 / pad 1 or ksize 1 / pad 0,
 * C and O multiples of 64, every tensor under 2^31 bytes).  All three are fixed launch sequences without host reads, float
 * atomics or memset nodes: capturable, and bit-identical from call to call.
 * s2a_conv_pack_weight_train: the master filter [O,C,k,k] (contiguous, weight_dtype F32 or F16) -> two f16 filters in the
 *   order of s2a_conv_pack_weight_f16, in one launch: packed_fwd (the filter itself) and, unless NULL, packed_dgrad, the
 *   input-gradient filter w'[c,o,ky,kx] = w[o,c,k-1-ky,k-1-kx] (a [C,O,k,k] filter: s2a_conv_nhwc_f16 on the output gradient
 *   with it, channels = O, out_channels = C, gives the input gradient).
 * s2a_conv_backward_prep_f16: one pass over grad_out [positions, O] f16.  out (the forward's ReLU output, or NULL when no
 *   ReLU was applied): g = out <= 0 ? 0 : grad_out (torch's rule: the gradient passes at a NaN output), written to g unless
 *   g is NULL.  grad_bias [O] (grad_bias_dtype, or NULL): the
 *   per-channel sums of g (of grad_out without out), f32 partials per workgroup summed in workgroup order.  With neither g
 *   nor grad_bias nothing is launched.  workspace: only for grad_bias.
 * s2a_conv_backward_weight_f16: grad_weight[o,c,ky,kx] (grad_dtype, contiguous [O,C,k,k]) =
 *   sum over (b,y,x) of g[b,y,x,o] * x[b,y+ky-pad,x+kx-pad,c], zero padding, f32 accumulation; x [B,H,W,C], g [B,H,W,O] f16.
 *   Split over position slices into per-slice f32 partials that a second launch sums in slice order; the split depends on
 *   the shapes only. */
int s2a_conv_pack_weight_train(const void* weight, int weight_dtype, int64_t out_channels, int64_t channels, int ksize,
                               void* packed_fwd, void* packed_dgrad, s2a_stream_t stream);
size_t s2a_conv_backward_prep_f16_workspace_bytes(int64_t positions, int64_t out_channels);
int s2a_conv_backward_prep_f16(const void* grad_out, const void* out, void* g, void* grad_bias, int grad_bias_dtype,
                               int64_t positions, int64_t out_channels, void* workspace, size_t workspace_bytes,
                               s2a_stream_t stream);
size_t s2a_conv_backward_weight_f16_workspace_bytes(int64_t batch, int64_t channels, int64_t height, int64_t width,
                                                    int64_t out_channels, int ksize);
int s2a_conv_backward_weight_f16(const void* x, const void* g, void* grad_weight, int grad_dtype, int64_t batch,
                                 int64_t channels, int64_t height, int64_t width, int64_t out_channels, int ksize,
                                 void* workspace, size_t workspace_bytes, s2a_stream_t stream);

/* The same for the stride-2 layers (FusedConv2d with own_grad_strided): ksize 3 / pad 1 / stride 2 with O % 128 == 0 (the
 * forward's limit) or ksize 1 / pad 0 / stride 2; C and O multiples of 64; x [B,H,W,C], g [B,Ho,Wo,O] f16 with
 * Ho = (H-1)/2+1, Wo = (W-1)/2+1; every tensor under 2^31 bytes and 16-byte aligned.  The forward is s2a_conv_nhwc_f16 with
 * stride = 2, the filter pack and the prep pass (on [B*Ho*Wo, O]) are the ones above.  No workspace: every buffer these
 * entry points write is an argument with a stated size.  No host read, no float atomic, no memset node, a fixed summation
 * order: capturable and bit-identical from call to call.  Every check below is made before the first HIP call and
 * answers S2A_EINVAL with a message.
 * s2a_conv_backward_input_s2_f16: writes grad_input, f16 [B,H,W,C], all B*H*W*C elements and nothing else, from g and
 *   packed_dgrad (the input-gradient filter of s2a_conv_pack_weight_train, O*C*k*k halfs).  ksize 3: input pixel
 *   (2i+py, 2j+px) sums the taps of its parity class -- (0,0): w[1,1] g[i,j]; (0,1): w[1,0] g[i,j+1] + w[1,2] g[i,j];
 *   (1,0): w[0,1] g[i+1,j] + w[2,1] g[i,j]; (1,1): w[0,0] g[i+1,j+1] + w[0,2] g[i+1,j] + w[2,0] g[i,j+1] + w[2,2] g[i,j] --
 *   in this order over f32; a neighbour outside the map is neither loaded nor multiplied.  ksize 1:
 *   grad_input[b,2i,2j,:] = W^T g[b,i,j,:], every pixel with an odd row or column is +0.
 * s2a_conv_backward_weight_s2_slices: the number of position slices of the weight gradient, from the shapes only (the
 *   same answer for the same shapes); 0 for a problem the entry point refuses (and for batch 0).
 * s2a_conv_backward_weight_s2_f16: writes partial, f32 [slices][O][C*k*k], all slices*O*C*k*k elements and nothing else;
 *   partial[s] is in the gradient's own layout [O,C,k,k] and holds the exact f32 sums, in tile order, over the position
 *   tiles s, s + slices, ... (3x3: 4 x 16 output positions of one image; 1x1: 64 consecutive output positions) of
 *   g[b,oy,ox,o] * x[b,2oy+ky-pad,2ox+kx-pad,c]; a slice without a tile holds exact zeros.  slices must be the query's
 *   answer; anything else is refused with no buffer touched.
 * s2a_conv_backward_weight_s2_reduce: out[e] = partial[0][e] + partial[1][e] + ... + partial[slices-1][e] in this order
 *   over f32, e < count; out is count elements of out_dtype (F32, or F16 with one rounding). */
int s2a_conv_backward_input_s2_f16(const void* g, const void* packed_dgrad, void* grad_input, int64_t batch,
                                   int64_t channels, int64_t height, int64_t width, int64_t out_channels, int ksize,
                                   s2a_stream_t stream);
int s2a_conv_backward_weight_s2_slices(int64_t batch, int64_t channels, int64_t height, int64_t width,
                                       int64_t out_channels, int ksize);
int s2a_conv_backward_weight_s2_f16(const void* x, const void* g, void* partial, int slices, int64_t batch,
                                    int64_t channels, int64_t height, int64_t width, int64_t out_channels, int ksize,
                                    s2a_stream_t stream);
int s2a_conv_backward_weight_s2_reduce(const void* partial, int slices, int64_t count, void* out, int out_dtype,
                                       s2a_stream_t stream);

/* Training side of the deformable convolution: the three device functions the reference's
 * backward is composed of (models/dcn/src/deform_conv_cuda_kernel.cu): deformable_im2col (:244-276),
 * deformable_col2im (:332-370), deformable_col2im_coord (:431-464).  p->batch = the number of images of
 * the chunk (the reference's im2col_step / parallel_imgs); layouts as the reference: im [S,C,H,W],
 * offset [S, dg*2*kH*kW, Ho, Wo] (same dtype as im), columns [C*kH*kW, S*Ho*Wo]; NCHW only.
 * s2a_deformable_col2im ACCUMULATES into grad_im_acc [S,C,H,W] (float32 for float32 / float16 columns, float64 for
 * float64 columns; caller zeroes it, as deform_conv.py:88-90 does); s2a_deformable_col2im_coord overwrites grad_offset.
 * The GEMMs around them (deform_conv_cuda.cpp:323-324, :455-459 addmm_) are library GEMMs on the host side.
 * dtype S2A_DTYPE_F64 (the reference dispatches these kernels on double too: AT_DISPATCH_FLOATING_TYPES_AND_HALF,
 * deform_conv_cuda_kernel.cu:258,352,450): evaluated in double throughout -- s2a_deform_conv_forward takes it on its
 * generic NCHW kernel (offsets float64 as well), and torch.autograd.gradcheck ties backward to forward on it. */
int s2a_deformable_im2col(const void* im, const void* offset, void* columns, const s2a_dcn_params* p,
                          s2a_stream_t stream);
int s2a_deformable_col2im(const void* columns, const void* offset, void* grad_im_acc,
                          const s2a_dcn_params* p, s2a_stream_t stream);
int s2a_deformable_col2im_coord(const void* columns, const void* im, const void* offset, void* grad_offset,
                                const s2a_dcn_params* p, s2a_stream_t stream);

/* deform_conv_backward_input_cuda (models/dcn/src/deform_conv_cuda.cpp:262-374: gradInput and gradOffset) for f16 tensors
 * with the AlignConv geometry -- 3x3, stride 1, pad 1, dilation 1, one group, one deformable group, channels % 32 == 0,
 * out_channels % 16 == 0, out_channels <= 256 -- as ONE fused kernel per call: the column gradient W^T . gradOutput is
 * formed tile by tile on the matrix cores and consumed in LDS (offset gradient = contraction with the sampled corners,
 * input gradient = bilinear scatter into an LDS window, flushed with one atomic per touched cell); the reference's
 * `columns` [C*9, N] never exists.  All tensors NCHW f16 as the reference passes them; grad_input_f32 [S,C,H,W] is
 * ACCUMULATED (the caller zeroes it, deform_conv.py:88), grad_offset [S,18,H,W] f16 is overwritten. */
size_t s2a_deform_conv_backward_input_workspace_bytes(int64_t batch, int64_t channels, int64_t height, int64_t width,
                                                      int64_t out_channels);
int s2a_deform_conv_backward_input_f16(const void* input, const void* offset, const void* grad_output, const void* weight,
                                       float* grad_input_f32, void* grad_offset, int64_t batch, int64_t channels,
                                       int64_t height, int64_t width, int64_t out_channels, void* workspace,
                                       size_t workspace_bytes, s2a_stream_t stream);

/* The same entry for f32 tensors (same geometry limits), on the f32 matrix instruction: 4 x 8 position tiles, gradOutput
 * tile and column gradient in LDS, no `columns`.  grad_input [S,C,H,W] f32 is the caller's gradInput, ACCUMULATED in place
 * (deform_conv_cuda.cpp:334-340 adds into it through col2im's atomics); grad_offset [S,18,H,W] f32 is overwritten. */
size_t s2a_deform_conv_backward_input_f32_workspace_bytes(int64_t batch, int64_t channels, int64_t height, int64_t width,
                                                          int64_t out_channels);
int s2a_deform_conv_backward_input_f32(const float* input, const float* offset, const float* grad_output, const float* weight,
                                       float* grad_input, float* grad_offset, int64_t batch, int64_t channels,
                                       int64_t height, int64_t width, int64_t out_channels, void* workspace,
                                       size_t workspace_bytes, s2a_stream_t stream);

/* deform_conv_backward_parameters_cuda (models/dcn/src/deform_conv_cuda.cpp:376-489: gradWeight) for f16 tensors with the
 * AlignConv geometry (channels % 64 == 0, out_channels % 32 == 0, out_channels <= 256), fused: the sampled columns are
 * formed tile by tile in LDS (bilinear corners from an LDS patch, as the forward does) and contracted with gradOutput over
 * the POSITIONS on the matrix cores, both operands through gfx950's transposing LDS read; split-K over the position tiles:
 * every workgroup stores its partial block and one reduce kernel sums the slices in a fixed order into grad_weight_f32
 * [O,C,3,3] (ACCUMULATED, unscaled: the caller zeroes it and applies `scale`) -- no atomics, bit-identical from run to run. */
size_t s2a_deform_conv_backward_weight_workspace_bytes(int64_t batch, int64_t channels, int64_t height, int64_t width,
                                                       int64_t out_channels);
int s2a_deform_conv_backward_weight_f16(const void* input, const void* offset, const void* grad_output,
                                        float* grad_weight_f32, int64_t batch, int64_t channels, int64_t height,
                                        int64_t width, int64_t out_channels, void* workspace, size_t workspace_bytes,
                                        s2a_stream_t stream);

/* The same entry for f32 tensors (same geometry limits, 4 x 8 position tiles): grad_weight [O,C,3,3] f32 is the caller's
 * gradWeight, += scale * gradOutput x columns^T in place (deform_conv_cuda.cpp:455-459); deterministic as above.
 * Arithmetic: every f32 operand is split EXACTLY into three bf16 values (8 + 8 + 8 significand bits) and a product is the six
 * largest of the nine plane products, accumulated in f32 on the 16-bit matrix instruction -- the accuracy of f32 arithmetic
 * (|error| of a product <~ 3 * 2^-24 of it; the bilinear blend itself runs in f32), 2.7 x fewer matrix cycles than
 * v_mfma_f32_16x16x4_f32.  The environment switch S2A_BWD_F32_WEIGHT=mfma32 selects the kernel on the f32 instruction. */
size_t s2a_deform_conv_backward_weight_f32_workspace_bytes(int64_t batch, int64_t channels, int64_t height, int64_t width,
                                                           int64_t out_channels);
int s2a_deform_conv_backward_weight_f32(const float* input, const float* offset, const float* grad_output,
                                        float* grad_weight, float scale, int64_t batch, int64_t channels, int64_t height,
                                        int64_t width, int64_t out_channels, void* workspace, size_t workspace_bytes,
                                        s2a_stream_t stream);

/* Both gradients of the AlignConv-geometry deformable convolution in ONE call -- what DeformConvFunction.backward needs
 * (models/dcn/deform_conv.py:73-118 calls deform_conv_backward_input_cuda and deform_conv_backward_parameters_cuda on the same
 * tensors): the NHWC copies of input and gradOutput the fused kernels read are made once instead of twice.
 * dtype = S2A_DTYPE_F16 / S2A_DTYPE_F32: the type of input, offset, grad_output, weight [O,C,3,3] and grad_offset [S,18,H,W];
 * grad_input_f32 [S,C,H,W] (ACCUMULATED) and grad_weight_f32 [O,C,3,3] (+= scale * ...) are always f32.  Either may be NULL
 * to skip that gradient (grad_offset goes with grad_input).  Limits: channels % 64 == 0, out_channels % 32 == 0, <= 256. */
size_t s2a_deform_conv_backward_workspace_bytes(int dtype, int64_t batch, int64_t channels, int64_t height, int64_t width,
                                                int64_t out_channels);
int s2a_deform_conv_backward(int dtype, const void* input, const void* offset, const void* grad_output, const void* weight,
                             float* grad_input_f32, void* grad_offset, float* grad_weight_f32, float scale, int64_t batch,
                             int64_t channels, int64_t height, int64_t width, int64_t out_channels, void* workspace,
                             size_t workspace_bytes, s2a_stream_t stream);
/* The same call with gradInput as DeformConvFunction.backward owns it (deform_conv.py:88: zeros_like(input)): grad_input
 * [S,C,H,W] is a tensor of `dtype` and is OVERWRITTEN with the gradient (== the reference's accumulation into a zeroed
 * tensor) -- no f32 copy on the caller's side and no conversion pass behind the call.  The tiles' sums are accumulated in f32
 * (workspace, [S,H,W,C]: one pixel's 32 channels are one 128-byte atomic row) and rounded once.  Workspace:
 * s2a_deform_conv_backward_workspace_bytes. */
int s2a_deform_conv_backward_typed(int dtype, const void* input, const void* offset, const void* grad_output,
                                   const void* weight, void* grad_input, void* grad_offset, float* grad_weight_f32,
                                   float scale, int64_t batch, int64_t channels, int64_t height, int64_t width,
                                   int64_t out_channels, void* workspace, size_t workspace_bytes, s2a_stream_t stream);

/* A bottleneck's conv2 + conv3 in one launch (models/backbone.py:56-83 with the BatchNorms folded):
 *   out = relu(W3 . relu(conv3x3(x; W2) + b2) + b3 + residual)        x [B,H,W,64] -> out [B,H,W,256], f16 NHWC
 * The 64-map intermediate never leaves the workgroup (LDS); results are bit-identical to s2a_conv_nhwc_f16 (3x3,
 * ReLU) followed by s2a_conv_nhwc_f16 (1x1, residual, ReLU).  weight_frag / tail_weight_frag from
 * s2a_conv_pack_weight_f16 (ksize 3 / 1); residual may be NULL.  channels = mid_channels = 64, out_channels = 256.
 * chain_*: optionally the NEXT bottleneck's conv1 (1x1, 256 -> chain_channels = 64 or 128, + bias + ReLU) applied to
 * the finished output tile in the same launch: chain_out [B,H,W,chain_channels] = relu(Wc . out + bc), bit-identical
 * to a separate s2a_conv_nhwc_f16; all three pointers NULL = not computed. */
int s2a_conv3x3_tail1x1_f16(const void* x, const void* weight_frag, const void* bias, const void* tail_weight_frag,
                            const void* tail_bias, const void* residual, void* out, const void* chain_weight_frag,
                            const void* chain_bias, void* chain_out, int64_t chain_channels, int64_t batch, int64_t channels,
                            int64_t mid_channels, int64_t out_channels, int64_t height, int64_t width,
                            s2a_stream_t stream);

/* A bottleneck's conv3 and the NEXT bottleneck's conv1 in one launch (models/backbone.py:69-83 with the BatchNorms
 * folded: conv3 + bn3 + residual + relu, then the next block's conv1 + bn1 + relu):
 *   out       [B,H,W,O]  = relu(W . x + b + residual)        x [B,H,W,K], f16 NHWC, residual [B,H,W,O] or NULL
 *   chain_out [B,H,W,O3] = relu(Wc . out + bc)               computed from the finished rows inside the workgroup
 * Both results are bit-identical to the two s2a_conv_nhwc_f16 (1x1) launches; the block output is not read back.
 * weight_frag / chain_weight_frag from s2a_conv_pack_weight_f16 (ksize 1).  (channels, out_channels, chain_channels) =
 * (128, 512, 128), (128, 512, 256) or (256, 1024, 256); the chain filter, bias and output are required. */
int s2a_conv1x1_chain_f16(const void* x, const void* weight_frag, const void* bias, const void* residual, void* out,
                          const void* chain_weight_frag, const void* chain_bias, void* chain_out, int64_t chain_channels,
                          int64_t batch, int64_t channels, int64_t out_channels, int64_t height, int64_t width,
                          s2a_stream_t stream);

/* FPN top-down step in one launch (models/neck.py:67-79): out[B,H,W,O] = conv1x1(x[B,H,W,C]) + bias +
 * nearest-2x-upsample(coarse[B,H/2,W/2,O]); f16 channels-last, H and W even, C and O multiples of 64. */
int s2a_conv1x1_add_up2_f16(const void* x, const void* weight_frag, const void* bias, const void* coarse,
                            void* out, int64_t batch, int64_t channels, int64_t height, int64_t width,
                            int64_t out_channels, s2a_stream_t stream);
/* Its training side (FusedConv2d with own_grad_entry, s2anet_amd.fused.FusedConvUp2Function): the forward is the launch
 * above on the forward filter of s2a_conv_pack_weight_train; the input, weight and bias gradients are those of the 1x1
 * convolution (s2a_conv_nhwc_f16 on the input-gradient filter, s2a_conv_backward_weight_f16, s2a_conv_backward_prep_f16);
 * the gradient of coarse is s2a_sum_pool2x2_f16: g[B,H,W,O] f16 -> out[B,H/2,W/2,O] f16,
 *   out[b,i,j,o] = f16( ((g[b,2i,2j,o] + g[b,2i,2j+1,o]) + g[b,2i+1,2j,o]) + g[b,2i+1,2j+1,o] )   over f32, one rounding.
 * H and W even, O a multiple of 8, g under 2^31 bytes, both tensors 16-byte aligned; every element of out is written and
 * nothing else; checked before the first HIP call (S2A_EINVAL with a message). */
int s2a_sum_pool2x2_f16(const void* g, void* out, int64_t batch, int64_t height, int64_t width, int64_t channels,
                        s2a_stream_t stream);

/* Pyramid-packed head launches.  The conv towers, AlignConv and prediction heads of S2ANetHead share
 * their filters over the FPN levels (models/head.py:261-265 maps forward_single over the levels), so
 * one launch can serve all of them: the levels sit back to back in ONE channels-last buffer
 * [sum_l B*H_l*W_l, C], level l = [B,H_l,W_l,C] at pixel offset sum_{k<l} B*H_k*W_k (anchors
 * [.,5] f32 and outputs packed the same way).  A workgroup finds its level from its tile index.
 *   s2a_pyramid_pixels            -> total pixel rows of the packed buffer (or -1: bad table)
 *   s2a_conv3x3_pyramid_f16       = s2a_conv_nhwc_f16(ksize 3) on every level
 *   s2a_align_conv_pyramid_f16    = s2a_align_conv_forward (f16, NHWC, weight from s2a_dcn_pack_weight)
 *                                   on every level, stride[l] = the level's anchor stride
 *   s2a_fam_refine_anchors_pyramid = s2a_fam_refine_anchors on every level; pred rows have
 *                                   row_stride f16 columns of which the first 5 are the deltas */
int64_t s2a_pyramid_pixels(const s2a_pyramid* pyr, int64_t batch);
int s2a_conv3x3_pyramid_f16(const void* x, const void* weight_frag, const void* bias, const void* residual,
                            void* out, int64_t batch, int64_t channels, int64_t out_channels, int relu,
                            const s2a_pyramid* pyr, s2a_stream_t stream);
/* A conv tower's last 3x3 layer + the 1x1 prediction head that reads it (fam_reg_ls / fam_cls_ls -> fam_reg_head /
 * fam_cls_head, models/head.py:163-213, :296-306) in one launch: head_out[P,64] (columns 0..31 written; the head's
 * <= 32 maps first) = head(relu?(conv3x3(x) + bias)) + head_bias, computed from the staged f16 tile as the separate
 * layers would.  out may be NULL when nothing else reads the tower (then it is never written).  O must be 256;
 * head_weight_frag = s2a_conv_pack_weight_f16 of the zero-padded [64,256,1,1] filter, head_bias >= 32 f16. */
int s2a_conv3x3_head_pyramid_f16(const void* x, const void* weight_frag, const void* bias, void* out,
                                 const void* head_weight_frag, const void* head_bias, void* head_out,
                                 int64_t batch, int64_t channels, int64_t out_channels, int relu,
                                 const s2a_pyramid* pyr, s2a_stream_t stream);
/* The 3x3 prediction convs with at most 16 maps (odm_reg_head: 5, odm_cls_head: num_classes <= 16; models/head.py:214-222):
 * s2a_conv3x3_pyramid_f16 with out_channels = 64 on the same operands, but only the first 16 filter rows are multiplied
 * (the filter stays in LDS, persistent workgroups walk the tiles).  weight_frag = s2a_conv_pack_weight_f16 of the [64,C,3,3]
 * filter zero-padded from out_channels_used rows, bias = 64 f16 (zero beyond out_channels_used) or NULL, out[P,64]:
 * columns < out_channels_used have the bits of s2a_conv3x3_pyramid_f16, the others are written as +0.  channels a multiple
 * of 64, 1 <= out_channels_used <= 16.  S2A_CONV_NARROW=0 (and channels > 256: the filter no longer fits) sends the call to
 * s2a_conv3x3_pyramid_f16; S2A_CONV_NARROW_WGS=n caps the persistent grid. */
int s2a_conv3x3_narrow_pyramid_f16(const void* x, const void* weight_frag, const void* bias, void* out, int64_t batch,
                                   int64_t channels, int64_t out_channels_used, int relu, const s2a_pyramid* pyr,
                                   s2a_stream_t stream);
/* ORConv2d + RotationInvariantPooling in one launch (models/head.py:337-341): out[P,O] = conv3x3(x) + bias (no
 * activation) and pooled[P,O/8] = max over every run of 8 orientation channels of out, both pyramid-packed. */
int s2a_orconv_pool_pyramid_f16(const void* x, const void* weight_frag, const void* bias, void* out, void* pooled,
                                int64_t batch, int64_t channels, int64_t out_channels, const s2a_pyramid* pyr,
                                s2a_stream_t stream);
/* The same 3x3 / stride 1 / pad 1 convolution (bias, optional ReLU, optional orientation max-pool as
 * s2a_orconv_pool_pyramid_f16) in the Winograd F(2,3) minimal-filtering form along x: 6 C O multiply-adds per output
 * instead of 9 C O, f16 operands / f32 accumulation as the direct kernel (the reference leaves the algorithm to cuDNN,
 * models/head.py:163-222).  Results differ from s2a_conv3x3_pyramid_f16 by the rounding of the transformed operands
 * (one f16 rounding of d_i +- d_j and of the transformed filter): same tolerance against an f32 convolution.
 *   weight_wino = s2a_conv_wino_pack_weight_f16 of the [O,C,3,3] f16 filter (s2a_conv_wino_packed_elems halfs; O a
 *   multiple of 64, C a multiple of 32); pooled [P,O/8] or NULL; a one-level table serves a plain [B,H,W,C] tensor. */
int64_t s2a_conv_wino_packed_elems(int64_t out_channels, int64_t channels);
int s2a_conv_wino_pack_weight_f16(const void* weight, int64_t out_channels, int64_t channels, void* packed,
                                  s2a_stream_t stream);
int s2a_conv3x3_wino_pyramid_f16(const void* x, const void* weight_wino, const void* bias, void* out, void* pooled,
                                 int64_t batch, int64_t channels, int64_t out_channels, int relu,
                                 const s2a_pyramid* pyr, s2a_stream_t stream);
/* FP8 (OCP e4m3fn, one byte per value) form of the 256 -> 256 tower convolutions, on the block-scaled matrix instruction
 * v_mfma_scale_f32_16x16x128_f8f6f4 with every block scale 1.0.  Opt-in (s2anet_amd.fp8); nothing else calls these.
 *   s2a_quantize_e4m3        q[rows, channels] = e4m3_rne(clamp(f32(x[rows, channels] f16) * inv_scale, -448, 448)):
 *                            round to nearest even, subnormals kept, +-inf -> +-448, NaN -> NaN; channels % 16 == 0
 *   s2a_conv_pack_weight_fp8 the [O,C,3,3] filter given as e4m3 bytes -> the fragment order s2a_conv3x3_pyramid_fp8
 *                            reads (O*C*9 bytes; a permutation only: quantise the filter first); O % 64 == 0, C % 128 == 0
 *   s2a_conv3x3_pyramid_fp8  3x3 / stride 1 / pad 1 on every level of the pyramid-packed x_q[P,C] e4m3:
 *                            acc[o] = sum x_q * w_q in f32, v = fma(acc, scale[o], bias[o]) (scale = input scale * filter
 *                            scale of channel o, f32[O]; bias f32[O]), optional ReLU (NaN -> 0), then
 *                            out_e4m3 = 0: out[P,O] f16 = f16_rne(v)
 *                            out_e4m3 = 1: out[P,O] e4m3 = e4m3_rne(clamp(v * out_inv_scale, -448, 448)): the next fp8
 *                            layer's input without a quantise launch
 *                            C % 128 == 0, O % 64 == 0; anything else is refused before any launch. */
int s2a_quantize_e4m3(const void* x, void* q, int64_t rows, int64_t channels, float inv_scale, s2a_stream_t stream);
int s2a_conv_pack_weight_fp8(const void* weight_q, int64_t out_channels, int64_t channels, void* packed,
                             s2a_stream_t stream);
int s2a_conv3x3_pyramid_fp8(const void* x_q, const void* weight_frag, const float* scale, const float* bias, void* out,
                            int out_e4m3, float out_inv_scale, int64_t batch, int64_t channels, int64_t out_channels,
                            int relu, const s2a_pyramid* pyr, s2a_stream_t stream);
int s2a_align_conv_pyramid_f16(const void* x, const float* anchors, const void* weight_packed, void* out,
                               int64_t batch, int64_t channels, int64_t out_channels, int relu,
                               const s2a_pyramid* pyr, s2a_stream_t stream);
int s2a_fam_refine_anchors_pyramid(const void* pred, int64_t row_stride, int64_t batch, const s2a_pyramid* pyr,
                                   float anchor_scale, float* refined, s2a_stream_t stream);

/* Fused ResNet stem of the end-to-end config: uint8 image / divisor
 * (val.py:246-247) -> conv 7x7 / stride 2 / pad 3, 3 -> 64 maps + bias (BatchNorm folded) -> ReLU ->
 * max-pool 3x3 / stride 2 / pad 1 (models/backbone.py:112-117, :172-175) in one kernel.
 * image_u8[B,H,W,3] (channels-last uint8, W % 4 == 0) -> out[B,Hp,Wp,64] f16 with
 * Hc = (H-1)/2+1, Hp = (Hc-1)/2+1 (same for W).  weight_packed = s2a_stem_pack_weight_f16 of the
 * [64,3,7,7] f16 filter (s2a_stem_packed_elems() halfs); bias[64] f16 or NULL. */
int64_t s2a_stem_packed_elems(void);
int s2a_stem_pack_weight_f16(const void* weight, void* packed, s2a_stream_t stream);
int s2a_stem_u8_f16(const void* image_u8, const void* weight_packed, const void* bias, void* out,
                    int64_t batch, int64_t height, int64_t width, float divisor, s2a_stream_t stream);

/* Training side of the stem (FusedConv2d with own_grad_entry, s2anet_amd.fused.StemU8Function): forward from the uint8
 * batch, filter and bias gradient; the input is an image, so there is no input gradient.  Shapes and limits as
 * s2a_stem_u8_f16.  Fixed launch sequences without host reads, float atomics or memset nodes, and a fixed summation order:
 * capturable and bit-identical from call to call.  No workspace: every buffer written is an argument with a stated size.
 * Every check is made before the first HIP call and answers S2A_EINVAL with a message.
 * s2a_stem_u8_f16_train: s2a_stem_u8_f16 plus sel, uint8 [B,Hp,Wp,64] (8-byte aligned).  A separate instantiation of the
 *   kernel: the convolution, bias add and rounding are the inference kernel's, and for a finite filter and bias out has
 *   its bits.  The epilogue follows torch, not the inference contract (the note at s2a_dcn_params): a NaN pre-activation
 *   stays NaN through ReLU and pool, +inf stays +inf.  sel[b,py,px,o] = 3 dy + dx in 0 .. 8 names the tap of the
 *   3x3 / s2 / p1 window the pool took, conv pixel (2 py - 1 + dy, 2 px - 1 + dx), by ATen's rule: dy then dx, a later tap
 *   replaces the current one only if it is strictly greater or NaN; a tap outside the conv map is never taken.  Writes all
 *   B*Hp*Wp*64 elements of out and of sel and nothing else.
 * s2a_stem_backward_slices: the number of slices of the gradient, from the shapes only (the same answer for the same
 *   shapes); 0 for a problem the entry point refuses (and for batch 0).
 * s2a_stem_backward_f16: writes partial, f32 [slices][64*147 + 64], all of it and nothing else; partial[s] holds first the
 *   filter gradient in [64,3,7,7] order, then the 64 bias sums: the f32 sums, in tile order, over the tiles s, s + slices,
 *   ... (8 x 8 pooled outputs of one image, the forward's tiles; inside a tile in a fixed order) of
 *     gW[o,c,ky,kx] += m * grad_out[b,py,px,o] * lut(image[b, 2y+ky-3, 2x+kx-3, c]),   gB[o] += m * grad_out[b,py,px,o],
 *   (y, x) the conv pixel sel names, m = 0 where out <= 0 else 1 (the gradient passes at a NaN output, as in
 *   s2a_conv_backward_prep_f16), lut(u) = f16(u / divisor), the value the forward multiplied.  A term with m = 0 is selected
 *   away, not multiplied; a pixel outside the image is not loaded and enters as +0.  Every product is exact in f32 and no
 *   gradient is rounded before the sums.  A slice without a tile holds exact zeros.  slices must be the query's answer;
 *   anything else is refused with no buffer touched.  out, sel, grad_out ([B,Hp,Wp,64] f16 / uint8 / f16) and partial
 *   16-byte aligned.  s2a_conv_backward_weight_s2_reduce(partial, slices, 64*147 + 64, ...) sums the slices in slice order
 *   into the master dtype. */
int s2a_stem_u8_f16_train(const void* image_u8, const void* weight_packed, const void* bias, void* out, void* sel,
                          int64_t batch, int64_t height, int64_t width, float divisor, s2a_stream_t stream);
int s2a_stem_backward_slices(int64_t batch, int64_t height, int64_t width);
int s2a_stem_backward_f16(const void* image_u8, const void* out, const void* sel, const void* grad_out, void* partial,
                          int slices, int64_t batch, int64_t height, int64_t width, float divisor, s2a_stream_t stream);

/* ---------------------------------------------------------------------------
 * S2ANet training loss: compute_loss -> compute_loss_single_level of the reference (models/head.py:353-646) for BOTH
 * modules (0 = FAM, 1 = ODM), all levels and all images in one forward call, after the assignment
 * (s2a_assign_labels_batched: both modules and all images in one sync-free launch sequence, so assignment + loss can be
 * captured into one graph; or s2a_assign_labels, one call per image and module).
 *
 *   classification  focal BCE with logits (utils/loss.py:31-58): alpha factor t*alpha + (1-t)(1-alpha), modulating
 *                   factor (1 - p_t)^fl_gamma; positives: one-hot target on the gt's class, negatives: all-zero target,
 *                   ignored anchors (-2): nothing, zero gradient
 *   regression      positives only: smooth-L1 (beta = smooth_l1_beta) of the prediction against rboxes_encode(anchor, gt)
 *                   (models/boxes.py:166-221, relative encoding), summed over the 5 components
 *   weighting       level sums x fpn_balance; module sums / max(positives of the module over all levels and images,
 *                   batch); regression x reg_balance; both ODM terms x odm_balance
 *
 * Maps are dense NCHW: cls [B,num_classes,H,W], bbox [B,5,H,W], f32 or f16 each (computed in f32).  anchors: f32,
 * [H*W,5] shared by all images (anchor_batch_stride 0, the FAM grid anchors) or [B,H,W,5] (stride H*W*5, the ODM
 * refined anchors).  grad_cls / grad_bbox: f32 maps of the cls / bbox shapes that receive the gradient of the
 * UNNORMALISED, fpn_balance-weighted loss (every element written); s2a_s2anet_loss_backward scales them.
 * Both modules of a level must have the same H, W.  At most S2A_LOSS_MAX_LEVELS levels. */
#define S2A_LOSS_MAX_LEVELS 8

typedef struct s2a_loss_map {
  const void* cls;
  const void* bbox;
  const float* anchors;
  float* grad_cls;
  float* grad_bbox;
  int64_t anchor_batch_stride; /* floats between two images' anchors: 0 or H*W*5 */
  int32_t height, width;
  int32_t cls_dtype, bbox_dtype; /* S2A_DTYPE_F32 / S2A_DTYPE_F16 */
  float fpn_balance;
  int32_t reserved;
} s2a_loss_map;

typedef struct s2a_loss_params {
  int32_t batch, num_classes, n_levels, reserved;
  float fl_gamma, fl_alpha, smooth_l1_beta, reg_balance, odm_balance;
  s2a_loss_map map[2][S2A_LOSS_MAX_LEVELS]; /* [module][level] */
} s2a_loss_params;

/* assign_ids   int64 [2, B, A], A = sum of H*W over the levels (levels concatenated in order, row-major (y, x) within
 *              a level): -2 ignore, -1 negative, >= 0 index of the gt within its image (s2a_assign_labels);
 *              an index >= that image's gt count is treated as ignored
 * targets      f32 [G,7] = (image, class, x, y, w, h, angle), px / rad, sorted by image; NULL when G == 0
 * target_offsets int64 [B+1]: image b owns rows target_offsets[b] .. target_offsets[b+1]-1 (the gt of id k is row
 *              target_offsets[b] + k); a class outside [0, num_classes) gives an all-zero target
 * loss [1], items [4] (fam_cls, fam_reg, odm_cls, odm_reg) f32; norm [4] f32: the factors that turn the stored
 *              gradients into those of loss (FAM cls, FAM reg, ODM cls, ODM reg), read by the backward
 * Two launches, no host synchronisation, no atomics: the sums are reduced in a fixed order (bit-reproducible).
 * workspace: s2a_s2anet_loss_workspace_bytes(B, A). */
size_t s2a_s2anet_loss_workspace_bytes(int64_t batch, int64_t anchors_per_image);
int s2a_s2anet_loss_forward(const s2a_loss_params* params, const int64_t* assign_ids, const float* targets,
                            const int64_t* target_offsets, float* loss, float* items, float* norm, void* workspace,
                            size_t workspace_bytes, s2a_stream_t stream);

/* Backward of s2a_s2anet_loss_forward, one launch: dst[i] = src[i] * grad_loss[0] * norm[norm_index] for every map
 * (src: a grad_cls / grad_bbox map of the forward, dst: the gradient of the prediction in its dtype, numel elements).
 * norm_index: 0 FAM cls, 1 FAM bbox, 2 ODM cls, 3 ODM bbox.  grad_loss: device f32 [1] (the incoming gradient of
 * loss, e.g. a GradScaler scale).  At most 4 * S2A_LOSS_MAX_LEVELS maps. */
typedef struct s2a_loss_grad_map {
  const float* src;
  void* dst;
  int64_t numel;
  int32_t dtype;
  int32_t norm_index;
} s2a_loss_grad_map;
int s2a_s2anet_loss_backward(const s2a_loss_grad_map* maps, int n_maps, const float* grad_loss, const float* norm,
                             s2a_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training update: the end of the reference's iteration (train.py:358-373, utils/torch_utils.py:276-307) as one
 * capturable launch sequence -- GradScaler.unscale_, clip_grad_norm_, scaler.step(SGD with momentum / Nesterov and
 * parameter groups), scaler.update, zero_grad (to zero, not to None) and ModelEMA.update.
 *
 * All tensors are contiguous f32 and are described by two DEVICE tables that the caller builds once:
 *   tensors  one s2a_optim_tensor per tensor.  kind S2A_OPTIM_TRAINED: p, grad, momentum_buf are updated, ema too unless
 *            it is NULL; kind S2A_OPTIM_EMA_ONLY: ema follows p (a floating buffer or a frozen parameter), grad and
 *            momentum_buf are not read.  group indexes lr / hyper.
 *   chunks   int64 [n_chunks, 2] = (tensor, first element): chunk c covers elements [start, min(start +
 *            S2A_OPTIM_CHUNK, numel)) of its tensor; start is a multiple of S2A_OPTIM_CHUNK.  The chunks of the trained
 *            tensors come first (n_trained_chunks of them), in tensor order, so the norm is summed in a fixed order.
 * lr f32 [n_groups]; hyper f32 [n_groups, 4] = (momentum, weight_decay, nesterov != 0, reserved); both on the device.
 *
 * Launches (on `stream`, geometry from the host arguments only; no host read, allocation, memset node or float atomic):
 *   1  partials   per trained chunk: f32 sum of (grad / scale)^2, reduced per workgroup in a fixed order, and a flag from
 *                 a per-element isfinite test of grad.  Skipped when neither max_norm nor scaling is enabled.
 *   2  finalise   one workgroup: partials added in chunk order in double; total_norm = sqrt; clip = min(1, max_norm /
 *                 (total_norm + 1e-6)) (1 when max_norm <= 0; a NaN norm gives a NaN clip as torch's clamp does);
 *                 found_inf = OR of the flags; skip_update = (scaling enabled && found_inf) || *skip != 0; the scale
 *                 follows torch's _amp_update_scale_ on found_inf alone (x backoff and tracker 0, else ++tracker and
 *                 x growth when it reaches growth_interval and the product is finite); updates += 1 and
 *                 d = ema_decay * (1 - exp(-updates / ema_tau)) in double.
 *   3  apply      per element, skip_update == 0: g = grad / scale * clip; g += wd * p when wd != 0;
 *                 buf = momentum * buf + g; g = nesterov ? g + momentum * buf : buf; p -= lr * g.  skip_update == 1: p and
 *                 buf are not written.  Always: ema = d * ema + (1 - d) * p with the new p, and grad = 0.
 * scale f32 [1] and counters int32 [2] = (growth_tracker, updates) are device state, read and written; scale is neither
 * read nor written when scaling_enabled == 0.  skip: optional device flag, int32 (skip_elem_bytes 4) or int64 (8).
 * stats f32 [S2A_OPTIM_STATS] = (unscaled pre-clip gradient norm (0 when launch 1 is skipped), clip, found_inf,
 * skip_update, new scale, d, updates, growth_tracker).
 * Rows whose four pointers are all 16-byte aligned are walked with 16-byte accesses, others and tails element-wise.
 * workspace: s2a_train_update_workspace_bytes(n_trained_chunks), 16-byte aligned.  It need NOT be zeroed, on the first
 * call or any later one: launch 1 writes the partial and flag of every trained chunk and launch 2 every field of the control
 * block before anything reads them (the Python side's zeroed buffer is a habit, not a requirement). */
#define S2A_OPTIM_CHUNK 4096
#define S2A_OPTIM_STATS 8
#define S2A_OPTIM_TRAINED 0
#define S2A_OPTIM_EMA_ONLY 1

typedef struct s2a_optim_tensor {
  float* p;
  float* grad;
  float* momentum_buf;
  float* ema;
  int64_t numel;
  int32_t group;
  int32_t kind;
} s2a_optim_tensor;

typedef struct s2a_train_update_args {
  const s2a_optim_tensor* tensors; /* device */
  const int64_t* chunks;           /* device */
  int64_t n_tensors, n_chunks, n_trained_chunks;
  const float* lr;                 /* device */
  const float* hyper;              /* device */
  int32_t n_groups;
  int32_t scaling_enabled;
  float* scale;                    /* device */
  int32_t* counters;               /* device */
  const void* skip;                /* device or NULL */
  int32_t skip_elem_bytes;
  int32_t growth_interval;
  float max_norm;                  /* <= 0: no clipping */
  float growth_factor, backoff_factor;
  float reserved;
  double ema_decay, ema_tau;
  float* stats;                    /* device */
} s2a_train_update_args;

size_t s2a_train_update_workspace_bytes(int64_t n_trained_chunks);
int s2a_train_update(const s2a_train_update_args* args, void* workspace, size_t workspace_bytes, s2a_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training augmentation: the two augmentations the reference's S2ANet recipe enables (data/hyps/hyp.scratch.s2anet.yaml:
 * degrees 180, fliplr 0.5; flipud is built too, everything else in that file is 0) on a batch of square S x S chips and
 * its polygon labels (augment_ops.hip).  HSV jitter, mosaic, mixup, free-angle and scaled warps, non-square chips and
 * letterboxing are not built.
 *
 * params int32 [batch, 4] on the device = (rot, flipud, fliplr, 0) per image; rot 0..3 = the reference's angles 0, 90,
 * -180, -90 degrees.  s2a_augment_draw fills it; a caller may also write it.
 *
 * Image (utils/augmentations.py:93-175 with scale = shear = translate = perspective = 0, then np.flipud, np.fliplr of
 * utils/datasets_rotation.py:480-492).  The turn M = T R C is an integer pixel map about S / 2, not (S - 1) / 2:
 *   rot 1: x' = y, y' = S - x      rot 2: x' = S - x, y' = S - y      rot 3: x' = S - y, y' = x      rot 0: untouched
 * so one source row or column leaves the chip and the facing destination row or column takes the border value 114:
 * row 0 at rot 1, row 0 and column 0 at rot 2, column 0 at rot 3.  The flips are plain reversals after the turn (a border
 * line moves with them).  cv2.warpAffine is OpenCV and is restated from its definition for these integer maps.
 *
 * Labels: f32 [n_rows, 10] = (image, class, x1, y1 .. x4, y4) in pixels, rows in any order; an image outside [0, batch)
 * marks padding.  In float64: the points go through M; the row is dropped unless the centre of the minimum-area
 * rectangle of the points truncated towards zero lies in [0, S] x [0, S] (box_candidates_rotation_filter_center); flipud
 * is y <- S - y, fliplr x <- S - x (S, not S - 1: the reference's); the points are truncated again and their
 * minimum-area rectangle becomes (cx, cy, w, h, theta), w the long side and theta its direction atan2(dy, dx) in image
 * coordinates in [-pi/4, 3pi/4) (poly_to_rotated_box_np; what s2a_rbox_to_poly inverts).  Row g of targets f32
 * [n_rows, 7] = (image, class, cx, cy, w, h, theta); no compaction.  A padding row, a dropped row and a row whose
 * truncated points span no area get image = -1 and zeros (OpenCV gives the last kind a zero-area box that matches no
 * anchor: a deviation).  normalize != 0 divides cx, w by the width and cy, h by the height (xywhtheta2xywhtheta_n).
 * Coordinates beyond +-2^29 saturate.  cv2.minAreaRect is restated as the smallest of the edge-aligned bounding
 * rectangles of the convex hull.  status int64 [4] on the device = (rows that are not padding, kept, dropped by the
 * centre filter, dropped as degenerate).
 *
 * Draw: Philox4x32-10 with counter (image, 0, step_lo, step_hi) and key (seed_lo, seed_hi); rot = word 0 & 3 when
 * turn != 0, else 0; flipud = u1 < p_flipud, fliplr = u2 < p_fliplr with u = (word >> 8) * 2^-24 from words 1 and 2.
 * step and seed are int64 device scalars; the launch reads step and then adds 1 to it, so every replay of a captured
 * graph draws afresh.
 *
 * All three launch on `stream`, take no workspace, allocate nothing and read nothing back.  S2A_EINVAL before any HIP call
 * for: NULL pointers, sizes that are not positive, height != width, a width that is no multiple of 4 (images: below 8),
 * probabilities outside [0, 1], src and dst that overlap, misaligned buffers (images 4 bytes, params 16, step / seed /
 * status 8).  src and dst are uint8 channels-last [batch, height, width, 3]. */
int s2a_augment_draw(int64_t* step, const int64_t* seed, int64_t batch, int turn, float p_flipud, float p_fliplr,
                     int32_t* params, s2a_stream_t stream);
int s2a_augment_images_u8(const uint8_t* src, const int32_t* params, int64_t batch, int64_t height, int64_t width,
                          uint8_t* dst, s2a_stream_t stream);
int s2a_augment_labels(const float* labels, int64_t n_rows, const int32_t* params, int64_t batch, int64_t height,
                       int64_t width, int normalize, float* targets, int64_t* status, s2a_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Training-mode BatchNorm (bn_ops.hip; the slice plan and the moment merges are csrc/bn_plan.hpp).  Reference:
 * torch.nn.BatchNorm2d in training mode as used in models/backbone.py:54-83 (the bottleneck's bn1 / bn2 / bn3 and the
 * downsample's norm): batch statistics over (N, H, W), gamma / beta, running statistics moved by `momentum` with the
 * unbiased variance.
 *
 * All four passes work on an f16 channels-last activation seen as [positions, channels], positions = B H W >= 2,
 * channels % 64 == 0, under 2^31 bytes.  Each is one walk over memory with 16-byte accesses; a lane keeps its channel
 * octet, and lanes, then slices are combined in a fixed order: no float atomics, no memset node, no host read, grid and
 * slice count from (positions, channels) only -- capturable, and the same bits every run.
 *
 * s2a_bn_slices: the slice count of a problem (0 for a refused one).  `partial` is a caller's f32 buffer
 * [slices][2][channels] that the launch writes completely: per-slice (mean, M2) for the statistics, per-slice
 * (sum g, sum g xhat) for the backward.  There is no opaque workspace.
 *
 * s2a_bn_train_stats_f16: mean f32 [C] and invstd = 1 / sqrt(biased var + eps) f32 [C].  Lanes accumulate shifted sums in
 * f32, the merges (lanes, then slices) run in double: |mean| >> std costs no accuracy.  running_mean / running_var (both
 * or neither; f32 or f16 by running_dtype) are updated in place: (1 - momentum) r + momentum batch, the variance
 * unbiased by positions / (positions - 1).
 *
 * s2a_bn_train_apply_f16: out = relu?((x - mean) invstd weight + bias (+ residual)), one rounding to f16.  weight / bias
 * f32 or f16 (param_dtype).  The ReLU keeps a NaN (torch's), unlike the fused ReLU of the inference launches.
 *
 * s2a_bn_backward_reduce_f16: g = out <= 0 ? 0 : grad_out when `out` is given (a NaN output passes the gradient), else
 * g = grad_out.  With `partial`: grad_bias = sum g and grad_weight = sum g xhat (either may be NULL; param_dtype; from the
 * f32 slice sums added in a fixed order, one rounding) and coef f32 [2][C] = (sum g / P, sum g xhat / P).  With `g`: the
 * masked gradient is also written there (it is the residual's gradient); needs `out`.  partial == NULL: the mask alone.
 *
 * s2a_bn_backward_input_f16: grad_input = weight invstd (g - coef[0] - xhat coef[1]); with `out` given, `g` is grad_out
 * and the mask is applied again here.
 *
 * S2A_EINVAL before any HIP call: NULL or misaligned pointers (activations and partial 16 bytes, vectors 4), channels
 * that are no multiple of 64, positions < 2, 2^31 bytes or more, a slice count other than s2a_bn_slices answers. */
int s2a_bn_slices(int64_t positions, int64_t channels);
int s2a_bn_train_stats_f16(const void* x, int64_t positions, int64_t channels, double eps, double momentum, float* partial,
                           int slices, float* mean, float* invstd, void* running_mean, void* running_var, int running_dtype,
                           s2a_stream_t stream);
int s2a_bn_train_apply_f16(const void* x, const float* mean, const float* invstd, const void* weight, const void* bias,
                           int param_dtype, const void* residual, void* out, int64_t positions, int64_t channels, int relu,
                           s2a_stream_t stream);
int s2a_bn_backward_reduce_f16(const void* grad_out, const void* x, const void* out, const float* mean, const float* invstd,
                               void* g, float* partial, int slices, void* grad_weight, void* grad_bias, int param_dtype,
                               float* coef, int64_t positions, int64_t channels, s2a_stream_t stream);
int s2a_bn_backward_input_f16(const void* g, const void* x, const void* out, const float* mean, const float* invstd,
                              const void* weight, int param_dtype, const float* coef, void* grad_input, int64_t positions,
                              int64_t channels, s2a_stream_t stream);

/* 0 for a normal build; non-zero when an object was compiled with a measurement / ablation switch (-DS2A_MEASURE,
 * -DS2A_WABL=..., -DS2A_STAMP=1: such a build may skip work or print diagnostics).  Bits 0-7 (the former AlignConv
 * ablation mask) are no longer set by any object. */
int s2a_build_flags(void);

/* Diagnostic builds only (-DS2A_STAMP=1): per-workgroup s_memtime phase stamps of the AlignConv
 * kernel; returns S2A_ENOTIMPL in a normal build. */
int s2a_debug_read_stamps(unsigned long long* host_dst, int64_t count);

#ifdef __cplusplus
}
#endif
#endif /* S2ANET_HIP_H_ */
