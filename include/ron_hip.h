/*
 * ron_hip.h -- C ABI of libron_hip.so: the MI355X (gfx950) RON-320 inference hot path.
 *
 * The reference (HiKapok/RON_Tensorflow) is pure Python/TensorFlow-1 and has NO FFI of its
 * own; every entry point below replaces the reference *Python* interface quoted next to it
 * (file:line relative to the reference repository).  INTEGRATION.md shows the ctypes stub a
 * maintainer of the reference would add to call them.
 *
 * Conventions
 *   - Plain C: pointers, sizes, PODs.  No torch / TF types.  `stream` is a hipStream_t passed
 *     as void* (NULL = default stream).  All device pointers are HIP device pointers.
 *   - Every function returns 0 on success or a negative ron_status; the message is available
 *     through ron_last_error() (per thread when no context is involved).
 *   - Nothing here synchronises with the host unless stated; work is enqueued on `stream`.
 *   - Ownership: the caller owns every input/output buffer; a ron_ctx owns its weights,
 *     anchors and workspace.  One ron_ctx per device; calls on one ctx are not re-entrant.
 *     Everything a ctx owns - activations, split-K scratch, ron_detect's head buffers and
 *     post-processing workspace - is allocated by ron_create / ron_finalize_weights /
 *     ron_clone for max_batch: no entry point that enqueues work allocates or frees.
 *     The post-processing workspace of a ctx is cleaned by the kernels that use it, in
 *     stream order: the ron_detect calls of ONE ctx must all go to one stream, or be ordered
 *     by the caller (events); two batches in flight take two contexts (ron_clone).  A
 *     ron_detect that returns an error leaves the workspace to be re-zeroed by the next call.
 *   - Tensor layout: NHWC, row-major, fp32 at the boundary.  Boxes are (ymin, xmin, ymax, xmax)
 *     in normalised image coordinates.  Head tensors are ordered coarse -> fine
 *     (block7 5x5, block6 10x10, block5 20x20, block4 40x40), RONParams.feat_layers,
 *     nets/ron_vgg_320.py:101.
 */
#ifndef RON_HIP_H_
#define RON_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RON_MAX_LAYERS 8
#define RON_MAX_ANCHORS_PER_CELL 16
#define RON_MAX_GT 256             /* ground-truth boxes per image ron_bboxes_matching accepts */
#define RON_MAX_TOPK 512           /* rows a detection list can hold (np_methods top_k = 400) */
#define RON_MAX_CLASSES 128        /* RONParams.num_classes (background included) the entry points accept: VOC 21, COCO 81 / 91 */

typedef enum {
  RON_OK = 0,
  RON_ERR_INVALID = -1,      /* bad argument                                   */
  RON_ERR_HIP = -2,          /* a HIP runtime call failed                      */
  RON_ERR_STATE = -3,        /* call order (e.g. forward before finalize)      */
  RON_ERR_UNKNOWN_NAME = -4, /* unknown variable / end-point / network name    */
  RON_ERR_UNSUPPORTED = -5
} ron_status;

/* REDUCEDFC / FULL: RON-320 bodies (nets/ron_vgg_320.py:510-580 / :434-508); SSD512: nets/ssd_vgg_512.py:364-460 (512 x 512
 * inputs only); SSD300: nets/ssd_vgg_300.py:434-523 (300 x 300 inputs only: the maps are 300 / 150 / 75 / 38 / 19 / 10 / 5 / 3 / 1,
 * the 2x2 pools are SAME, i.e. ceil) */
typedef enum { RON_VARIANT_REDUCEDFC = 0, RON_VARIANT_FULL = 1, RON_VARIANT_SSD512 = 2, RON_VARIANT_SSD300 = 3 } ron_variant;
/* Arithmetic of the conv stack (activations + weights in HBM, what the MFMAs consume); accumulation is fp32 in all of them.
 *   F32   : v_mfma_f32_16x16x4_f32, exact fp32 products (parity mode, 157 TFLOP/s matrix peak)
 *   BF16  : v_mfma_f32_16x16x32_bf16 (benchmark mode of BASELINE config 2)
 *   F16   : v_mfma_f32_16x16x32_f16
 *   F16X3 : split precision -- every value is stored as two f16 planes hi = rnd(v), lo = rnd(v - hi) (22 mantissa bits,
 *           4 bytes per element: 32 hi followed by 32 lo per 128-byte channel chunk) and a product is three f16 MFMAs
 *           hi*hi + lo*hi + hi*lo into the fp32 accumulator (the dropped lo*lo term is 2^-22 relative); weights carry a
 *           per-layer power-of-two scale (undone in the epilogue) so that their lo plane stays a normal f16.  fp32-grade
 *           head tensors (detections within 1e-4 of the fp32 CPU reference) at a third of the f16 matrix peak.
 *           VALID ACTIVATION RANGE (activations carry no scale): 22 bits hold for 2^-3 <= |v| < 65504.  Above, a value
 *           saturates instead of overflowing: up to 131008 it is kept as 65504 + rest (f16 spacing of 32), beyond it clips;
 *           NaN stays NaN.  Below 2^-3 the lo plane is an f16 subnormal (the matrix core does not flush it): an ABSOLUTE error
 *           floor of 2^-25 per stored value, i.e. a tensor whose whole scale is 2^-10 keeps ~15 bits.  RON / SSD activations on
 *           unscaled mean-subtracted images are O(1) .. O(10^3).  tests/test_gpu_conv.py holds both regimes against float64. */
typedef enum { RON_DTYPE_F32 = 0, RON_DTYPE_BF16 = 1, RON_DTYPE_F16 = 2, RON_DTYPE_F16X3 = 3 } ron_dtype;

const char* ron_last_error(void);
/* ABI version of the library (bumped on any signature change). */
int ron_abi_version(void);
/* Host utility: CRC32C of a buffer (chain with `crc`, 0 first) -- the checksum of TensorFlow V2 checkpoint files
 * (tf.train.Saver(write_version=2), ron_net.py:395-398), used by ron_tensorflow_amd/checkpoint.py. */
uint32_t ron_crc32c(const void* data, uint64_t nbytes, uint32_t crc);

/* ------------------------------------------------------------------------------------------
 * Anchors.  Replaces ron_anchor_one_layer / ron_anchors_all_layers / RONNet.anchors
 * (nets/ron_vgg_320.py:285-333, :336-355, :162-171).  Pure host function, bit-exact with the
 * reference's numpy float32 arithmetic.
 *   y, x : [feat_h * feat_w]   (the reference returns them as [H, W, 1])
 *   h, w : [n_sizes * n_ratios], anchor a = i_ratio * n_sizes + j_size
 * ---------------------------------------------------------------------------------------- */
int ron_anchor_one_layer(int img_h, int img_w, int feat_h, int feat_w,
                         const double* sizes, int n_sizes,
                         const double* ratios, int n_ratios,
                         double step, double offset,
                         float* y, float* x, float* h, float* w);

/* SSD flavour: ssd_anchor_one_layer (nets/ssd_vgg_512.py:286-338); A = n_sizes + n_ratios anchors per cell:
 * [sizes[0] square, sqrt(sizes[0]*sizes[1]) square, sizes[0] at each ratio]. */
int ron_ssd_anchor_one_layer(int img_h, int img_w, int feat_h, int feat_w,
                             const double* sizes, int n_sizes,
                             const double* ratios, int n_ratios,
                             double step, double offset,
                             float* y, float* x, float* h, float* w);

/* ------------------------------------------------------------------------------------------
 * Head tensors of one batch (device pointers, fp32).  This is what RONNet.net() returns as
 * Python lists (nets/ron_vgg_320.py:136-154, :580) and what bboxes_decode / detected_bboxes /
 * np_methods.ssd_bboxes_select consume.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t num_layers;
  int32_t num_classes;                      /* C, background included (21)                  */
  int32_t feat_h[RON_MAX_LAYERS];
  int32_t feat_w[RON_MAX_LAYERS];
  int32_t num_anchors[RON_MAX_LAYERS];      /* A per cell (10)                              */
  const float* cls[RON_MAX_LAYERS];         /* [N,H,W,A,C]  logits or probabilities         */
  const float* obj[RON_MAX_LAYERS];         /* [N,H,W,A,2] logits | [N,H,W,A,1] prob | NULL */
  const float* loc[RON_MAX_LAYERS];         /* [N,H,W,A,4]  raw offsets or decoded boxes    */
  /* anchors (device): y, x [H*W]; h, w [A].  Needed only when loc holds raw offsets. */
  const float* anchor_y[RON_MAX_LAYERS];
  const float* anchor_x[RON_MAX_LAYERS];
  const float* anchor_h[RON_MAX_LAYERS];
  const float* anchor_w[RON_MAX_LAYERS];
} ron_heads;

/* flags for ron_post_cfg.input_flags */
#define RON_IN_CLS_IS_PROB 1u   /* cls holds softmax probabilities (RONNet.net()[0])          */
#define RON_IN_OBJ_IS_PROB 2u   /* obj holds P(object) [N,H,W,A,1] (RONNet.net()[2])          */
#define RON_IN_LOC_DECODED 4u   /* loc already holds decoded boxes (RONNet.bboxes_decode)     */
/* bits 30 and 31 of input_flags are reserved for the library: callers pass them as 0 */

typedef struct {
  float objectness_thres;   /* eval_ron_network.py:66-67,227-229 (0.03); ignored if obj NULL */
  float select_threshold;   /* np_methods.py:59 / eval_ron_network.py:64-65; 0 = the arg-max
                             * branch (np_methods.py:82-89): one candidate per anchor       */
  float nms_threshold;      /* np_methods.py:229                                             */
  int32_t top_k;            /* np_methods.py:137 (400); <= RON_MAX_TOPK                      */
  float bbox_img[4];        /* clip reference + resize box (notebook cell 8): [0,0,1,1]      */
  float prior_scaling[4];   /* np_methods.py:25: [0.1,0.1,0.2,0.2]                           */
  uint32_t input_flags;
} ron_post_cfg;

/* Fixed-capacity detection list per image; rows >= count[i] are zero. */
typedef struct {
  int32_t capacity;         /* rows per image, >= top_k                                      */
  int32_t* classes;         /* [N, capacity]                                                 */
  float* scores;            /* [N, capacity]                                                 */
  float* bboxes;            /* [N, capacity, 4]                                              */
  int32_t* anchor_index;    /* [N, capacity]  flat index into the concatenated anchor list   */
  int32_t* count;           /* [N]                                                           */
} ron_detections;

/* Bytes of device scratch ron_post_np needs for a batch of n images. */
int64_t ron_post_np_workspace_bytes(const ron_heads* heads, int n);

/*
 * np_methods pipeline on the device (one call per batch):
 *   [softmax + objectness gate]  nets/ron_vgg_320.py:572-576, eval_ron_network.py:227-229
 *   decode                        np_methods.py:23-53   (== ssd_common.py:448-474)
 *   select (score > thr, c >= 1)  np_methods.py:56-131
 *   clip to bbox_img              np_methods.py:153-164
 *   sort, keep top_k              np_methods.py:137-150 (order: score desc, position asc)
 *   greedy class-aware IoU NMS    np_methods.py:186-205, :229-242
 *   resize by bbox_img            np_methods.py:167-183
 * `out` receives the kept boxes; `sorted_out` (optional, may be NULL) the list after the
 * top_k cut and before NMS; `n_candidates` (optional) [N] the select count per image.
 */
int ron_post_np(const ron_heads* heads, int n, const ron_post_cfg* cfg,
                void* workspace, int64_t workspace_bytes,
                ron_detections* out, ron_detections* sorted_out, int32_t* n_candidates,
                void* stream);

/*
 * The last three steps alone, on explicit candidate lists (np_methods.bboxes_sort ->
 * bboxes_nms, np_methods.py:137-150, :229-242): classes [N, n_in] int32, scores [N, n_in],
 * bboxes [N, n_in, 4]; n_valid [N] (or NULL = n_in everywhere).  No clip / resize.
 * Scores may be any float: negative ones sort below positive ones, -0 ties with +0, NaN sorts
 * last (the order of np.argsort(-scores)); ties keep their input order.
 */
int ron_np_sort_nms(const int32_t* classes, const float* scores, const float* bboxes,
                    const int32_t* n_valid, int n, int n_in, int top_k, float nms_threshold,
                    void* workspace, int64_t workspace_bytes,
                    ron_detections* out, ron_detections* sorted_out, void* stream);
int64_t ron_np_sort_nms_workspace_bytes(int n, int n_in);

/* RONNet.bboxes_decode (nets/ron_vgg_320.py:188-195 -> ssd_common.py:448-498): one layer,
 * loc [N,H,W,A,4] raw -> out [N,H,W,A,4] (ymin,xmin,ymax,xmax). */
int ron_bboxes_decode_layer(const float* loc, int n, int feat_h, int feat_w, int num_anchors,
                            const float* anchor_y, const float* anchor_x,
                            const float* anchor_h, const float* anchor_w,
                            const float prior_scaling[4], float* out, void* stream);

/* slim.softmax over the last axis (nets/ron_vgg_320.py:572,574): x [rows, c] -> y [rows, c].
 * With pick >= 0 only channel `pick` is written: y [rows, 1] (objness_pred, :576). */
int ron_softmax_last(const float* x, int64_t rows, int c, int pick, float* y, void* stream);

/* RONNet.bboxes_filter_min (nets/ron_vgg_320.py:196-233) as an operator of its own: per list the rows with
 * w = xmax - xmin > minsize and h = ymax - ymin > minsize, in their order (tf.boolean_mask), zeros behind them
 * (tfe_tensors.pad_axis, tf_extended/tensors.py:59-86).
 *   scores [num_lists, rows], bboxes [num_lists, rows, 4] (ymin, xmin, ymax, xmax)  ->  out_scores [num_lists, out_rows],
 *   out_bboxes [num_lists, out_rows, 4] (out_rows >= rows; every row written), counts [num_lists] = rows that passed.
 * The reference returns max(count, top_k) rows of a list: the caller slices (ops.bboxes_filter_min).  (ron_post_tfe applies the
 * same filter inside detected_bboxes, ron_tfe_cfg.min_size.) */
int ron_bboxes_filter_min(const float* scores, const float* bboxes, int num_lists, int rows, float minsize,
                          float* out_scores, float* out_bboxes, int out_rows, int32_t* counts, void* stream);

/* Detection records for the multi-GPU exchange: one float32 tensor [n, capacity + 1, 7] per rank, rows
 * 0..capacity-1 = (class, score, ymin, xmin, ymax, xmax, anchor_index), zero padded past `count`; row `capacity` = the
 * count replicated.  The only thing that crosses xGMI: one RCCL all-gather of these. */
int ron_pack_records(const ron_detections* det, int n, float* records, void* stream);
/* ... and that all-gather (SURVEY.md 8e names ncclAllGather): every rank's `records` [n, capacity + 1, 7] into `gathered`
 * [world, n, capacity + 1, 7] on every rank, enqueued on `stream`.  nccl_comm: an ncclComm_t (rccl.h) the caller created with one
 * rank per GPU; RCCL is looked up at the first call (the host's own librccl, or one already loaded, or librccl.so.1) and is not a
 * link-time dependency of this library: RON_ERR_UNSUPPORTED when the process has none.  `records` may be the slice of `gathered`
 * that belongs to this rank (in place).  The reference has no inference data parallelism (eval_ron_network.py:93-94: batch 1, one
 * device); the Python host does the same exchange through torch.distributed (ron_tensorflow_amd/parallel.py). */
int ron_gather_records(const float* records, int n, int capacity, float* gathered, void* nccl_comm, void* stream);

/* ------------------------------------------------------------------------------------------
 * TF evaluation variant of the post-processing (what eval_ron_network.py:226-236 runs):
 *   tf_ssd_bboxes_select (ssd_common.py:504-589) -> tfe.bboxes_clip (bboxes.py:105-144)
 *   -> RONNet.bboxes_filter_min (ron_vgg_320.py:196-233) -> tfe.bboxes_sort (bboxes.py:60-101)
 *   -> tfe.bboxes_nms_batch (bboxes.py:173-234, :262-302).
 * Output: per class c = 1..C-1, keep_top_k rows, zero padded (tfe.pad_axis, tensors.py:59-86):
 *   scores [N, C-1, keep_top_k], bboxes [N, C-1, keep_top_k, 4].
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  float objectness_thres;
  float select_threshold;
  float nms_threshold;
  int32_t top_k;            /* select_top_k (200), <= RON_MAX_TOPK */
  int32_t keep_top_k;       /* 100 */
  int32_t nms_mode;         /* 0 = 'min' (bboxes.py:207-208), 1 = 'union' (:205-206) */
  int32_t clip;             /* clipping_bbox given? */
  float clipping_bbox[4];
  float min_size;           /* bboxes_filter_min minsize (0.03); < 0 disables (SSD) */
  float prior_scaling[4];
  uint32_t input_flags;
} ron_tfe_cfg;

int64_t ron_post_tfe_workspace_bytes(const ron_heads* heads, int n);
int ron_post_tfe(const ron_heads* heads, int n, const ron_tfe_cfg* cfg,
                 void* workspace, int64_t workspace_bytes,
                 float* scores, float* bboxes, void* stream);

/* ------------------------------------------------------------------------------------------
 * ron_eval.py variant of the post-processing (the reference's per-image harness, ron_eval.py:111-206, :369-392, :466-477):
 *   flaten_predict: score[c] = objectness * class probability, label = argmax over all classes, kept when label > 0 and
 *   objectness > objectness_thres -> tfe.bboxes_clip(bbox_img) -> filter_boxes (sides > min_size, centre inside the image)
 *   -> tf_bboxes_nms: score > select_threshold, all classes together, greedy in score order, at most keep_top_k kept,
 *   overlap 'union' (what main() passes) or 'min' -> tfe.bboxes_resize(bbox_img).
 *   nms_mode | 2: tf_bboxes_nms_by_class_v1 instead (ron_eval.py:282-366, the variant behind the commented call of :474): a kept
 *   box suppresses boxes of its own label only; the first keep_top_k kept rows in score order are returned.
 *   nms_mode | 4: tf_bboxes_nms_by_class (ron_eval.py:212-280, the other variant of that commented call): every score COLUMN
 *   (objectness * probability of class c, the background column included) is a list of its own - rows with score[c] >
 *   select_threshold, sorted by score[c], greedy with at most keep_top_k picks; a row some list kept is returned with the largest of
 *   its kept scores and that score's class (lowest class among equals), rows in the flattened anchor order (NOT score order), at most
 *   num_classes * keep_top_k of them: `out` needs that capacity, and the workspace ron_post_eval_workspace_bytes_mode() gives.
 * min_sizes: device [n], filter_boxes' min_size of every image (max(1e-4, 0.03 * sqrt(h * w / (320 * 320)))).
 * Output: ron_detections (classes = labels), capacity >= keep_top_k, kept rows in score order, zero padded.
 * The 1024 highest scores that pass the filters are the NMS candidates (the reference considers all of them; with its
 * thresholds, 0.95 / 0.6, a few dozen pass).
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  float objectness_thres;   /* 0.95 */
  float select_threshold;   /* 0.6  */
  float nms_threshold;      /* 0.4  */
  int32_t keep_top_k;       /* nms_topk = 20 */
  int32_t nms_mode;         /* 1 = 'union', 0 = 'min'; + 2 = by class (tf_bboxes_nms_by_class_v1); + 4 = tf_bboxes_nms_by_class */
  float bbox_img[4];
  float prior_scaling[4];
  uint32_t input_flags;
} ron_eval_cfg;
int64_t ron_post_eval_workspace_bytes(const ron_heads* heads, int n);                      /* nms_mode 0 .. 3 */
int64_t ron_post_eval_workspace_bytes_mode(const ron_heads* heads, int n, int nms_mode);   /* any nms_mode */
int ron_post_eval(const ron_heads* heads, int n, const float* min_sizes, const ron_eval_cfg* cfg,
                  void* workspace, int64_t workspace_bytes, ron_detections* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation preprocessing: preprocess_for_eval with Resize.WARP_RESIZE
 * (preprocessing/ssd_vgg_preprocessing.py:358-425, tf_image.py:269-282): uint8 RGB -> float, minus the channel means,
 * TF1 bilinear resize (align_corners=False, no half-pixel centres) to [out_h, out_w].
 *   packed  : the n images' HWC uint8 bytes back to back (device)
 *   offsets : [n] byte offset of image i in `packed` (device, int64)
 *   hw      : [n, 2] height, width of image i (device)
 *   means   : [3] host floats (123, 117, 104)
 *   out     : [n, out_h, out_w, 3] float32 (device) -- the `images` argument of ron_forward
 * ---------------------------------------------------------------------------------------- */
int ron_preprocess_eval(const uint8_t* packed, const int64_t* offsets, const int32_t* hw, int n,
                        int out_h, int out_w, const float* means, float* out, void* stream);
/* The other resize modes of preprocess_for_eval (CENTRAL_CROP: tf_image.resize_image_bboxes_with_crop_or_pad,
 * tf_image.py:141-254; PAD_AND_RESIZE: ssd_vgg_preprocessing.py:392-405) as one geometry table (device, int32 [n, 8]):
 *   {crop_y, crop_x, crop_h, crop_w, pad_y, pad_x, resized_h, resized_w}: the crop window of the whitened image is resized to
 *   resized_h x resized_w (TF1 bilinear) and placed at (pad_y, pad_x) of the output; the rest of the output is 0. */
int ron_preprocess_eval_geom(const uint8_t* packed, const int64_t* offsets, const int32_t* hw, const int32_t* geom, int n,
                             int out_h, int out_w, const float* means, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Evaluation bookkeeping: tfe.bboxes_matching_batch (tf_extended/bboxes.py:316-450) on the dense output of
 * ron_post_tfe.  List (i, c) holds class label c + 1 of image i:
 *   scores [N, L, K] (unused by the matching itself, kept for the reference's argument list), bboxes [N, L, K, 4],
 *   glabels [N, G] (0 = padding), gbboxes [N, G, 4], gdifficults [N, G] (non-zero = difficult), G <= RON_MAX_GT
 *   -> n_gbboxes [N, L] (non-difficult ground truth of the class), tp / fp [N, L, K] (0 / 1).
 * ---------------------------------------------------------------------------------------- */
int ron_bboxes_matching(const float* scores, const float* bboxes, int n, int num_lists, int k,
                        const int32_t* glabels, const float* gbboxes, const uint8_t* gdifficults, int g,
                        float matching_threshold, int32_t* n_gbboxes, uint8_t* tp, uint8_t* fp, void* stream);

/* ------------------------------------------------------------------------------------------
 * Label side: per-anchor targets, the loss, and the loss's gradient with respect to the head tensors (ron_losses_grad).  The
 * gradient stops at the head tensors: there is no backward pass through the conv stack.
 * ---------------------------------------------------------------------------------------- */
/* Per-anchor targets of one batch (device pointers, one per feature layer, coarse -> fine): what RONNet.bboxes_encode returns as
 * four Python lists (nets/ron_vgg_320.py:173-186) and RONNet.losses consumes. */
typedef struct {
  int64_t* gclasses[RON_MAX_LAYERS];        /* [N,H,W,A]    label of a positive, 0 negative, -1 ignored */
  float* glocalisations[RON_MAX_LAYERS];    /* [N,H,W,A,4]  (cx, cy, w, h) regression targets           */
  float* gscores[RON_MAX_LAYERS];           /* [N,H,W,A]    overlap with the matched box                */
  float* gbboxes[RON_MAX_LAYERS];           /* [N,H,W,A,4]  the anchors' corners (ymin,xmin,ymax,xmax)  */
} ron_targets;

/* RONNet.bboxes_encode (nets/ron_vgg_320.py:173-186) -> ssd_common.tf_ssd_bboxes_encode / tf_ssd_bboxes_encode_layer /
 * do_dual_max_match / iou_matrix (nets/ssd_common.py:337-414, :77-147, :49-75, :27-47), for a batch: the reference encodes one image
 * per call on the CPU in front of tf.train.batch (ron_net.py:277-304).
 *   anchors : shapes + anchor_y/x/h/w of every layer (what ron_heads_describe fills; cls / obj / loc are not read)
 *   glabels [N, G] int32 (0 = padding; the present rows are a prefix), gbboxes [N, G, 4], 1 <= G <= RON_MAX_GT (device)
 *   allowed_borders : [num_layers] host ints (RONParams.allowed_borders), prior_scaling : [4] host floats
 * An anchor whose best overlap is >= positive_threshold keeps its box (the reference's masks leave an overlap equal to the threshold
 * matched), one in [ignore_threshold, positive_threshold) is ignored (-1), the rest are negative; the best anchor of every box is
 * matched to it whatever its overlap (the lowest box wins an anchor several boxes claim).  An image without a present row (TF cannot
 * run it) gives all-negative targets.  The anchors' corners, the classes, scores and the centre targets are those of the reference's
 * float32 arithmetic bit for bit; the w / h targets go through logf.
 * workspace: ron_bboxes_encode_workspace_bytes(n, g) bytes of device scratch (one 64-bit key per box). */
int64_t ron_bboxes_encode_workspace_bytes(int n, int g);
int ron_bboxes_encode(const ron_heads* anchors, int n, const int32_t* glabels, const float* gbboxes, int g,
                      int img_h, int img_w, const int32_t* allowed_borders,
                      float positive_threshold, float ignore_threshold, const float prior_scaling[4],
                      void* workspace, int64_t workspace_bytes, ron_targets* out, void* stream);

/* RONNet.losses (nets/ron_vgg_320.py:258-279) -> ron_losses (:635-778) with custom_layers.modified_smooth_l1 (sigma 3,
 * nets/custom_layers.py:31-49), over the whole batch (the reference flattens layers, then images, into one list of rows).
 *   heads        : raw logits cls [N,H,W,A,C], obj [N,H,W,A,2], loc [N,H,W,A,4] (anchor_* are not read)
 *   objness_pred : per layer [N,H,W,A,1], P(object) (RONNet.net()[2])
 *   targets      : gclasses / glocalisations of ron_bboxes_encode (gscores / gbboxes are not read, as in the reference)
 *   rand_objness, rand_cls : one float in [0, 1) per row, in the flattened order (layer, image, row, column, anchor): the draws the
 *                  reference makes inside the graph (tf.random_uniform, :703, :735) are inputs here
 *   losses [4]   : cross_entropy_pos, cross_entropy_objectness, localization, their sum (device)
 *   counts [6]   : n_pos, n_neg, n_cls_pos, n_cls_neg, rows in the objectness set, rows in the class set (device, int32)
 * Deterministic: integer counts, float sums through per-workgroup partials added in a fixed order.
 * workspace: ron_losses_workspace_bytes(heads, n) bytes of device scratch. */
typedef struct {
  float objness_threshold;  /* 0.03 */
  float negative_ratio;     /* 3    */
  float alpha;              /* 1/3: weight of the objectness term */
  float beta;               /* 1/3: weight of the localisation term; the class term gets 1 - alpha - beta */
} ron_loss_cfg;
int64_t ron_losses_workspace_bytes(const ron_heads* heads, int n);
int ron_losses(const ron_heads* heads, const float* const* objness_pred, const ron_targets* targets, int n,
               const float* rand_objness, const float* rand_cls, const ron_loss_cfg* cfg,
               void* workspace, int64_t workspace_bytes, float* losses, int32_t* counts, void* stream);

/* ron_losses and, in the same call, d losses[0] / d cls, d losses[1] / d obj, d losses[2] / d loc.  Each term reads one head tensor,
 * so the three tensors are also the gradient of losses[3]; a caller scales each by its upstream scalar.  objness_pred enters through
 * comparisons only and has no gradient.  `losses` and `counts` are bit for bit what ron_losses writes (the same kernels run).
 *   class term   : a row of the class set with clipped label l gets (softmax(x)[k] - [k == l]) * s_cls, softmax(x)[k] =
 *                  expf(x[k] - max) / sum (the sum in index order), s_cls = (1 - alpha - beta) / n_cls_set when n_pos > 0, else 0;
 *                  a label equal to num_classes gives a NaN row, as it gives a NaN loss
 *   objectness   : the same over the objectness set with two logits and label (gclasses > 0), s_obj = alpha / n_objness_set
 *                  when n_pos > 0, else 0
 *   localisation : a row with gclasses > 0 and objness_pred > objness_threshold, d = pred - target per coordinate, gets
 *                  (9 * d) * s_loc when |d| < 1.0f / 9.0f, else copysignf(1, d) * s_loc; s_loc = beta / n_cls_pos when n_cls_pos > 0,
 *                  else 0
 * Every element of the three tensors is written (rows outside a set: +0), nothing has to be cleared; no floating-point atomics, two
 * calls give the same bytes; counts and scales stay on the device.  obj / d_obj rows are moved as 8-byte, loc / glocalisations /
 * d_loc rows as 16-byte accesses: the layer pointers must be aligned accordingly.
 * workspace: ron_losses_grad_workspace_bytes(heads, n) bytes of device scratch. */
typedef struct {                       /* device pointers, one per layer, same layouts as ron_heads' cls / obj / loc */
  float* d_cls[RON_MAX_LAYERS];        /* [N,H,W,A,C]  d losses[0] / d cls */
  float* d_obj[RON_MAX_LAYERS];        /* [N,H,W,A,2]  d losses[1] / d obj */
  float* d_loc[RON_MAX_LAYERS];        /* [N,H,W,A,4]  d losses[2] / d loc */
} ron_head_grads;
int64_t ron_losses_grad_workspace_bytes(const ron_heads* heads, int n);
int ron_losses_grad(const ron_heads* heads, const float* const* objness_pred, const ron_targets* targets, int n,
                    const float* rand_objness, const float* rand_cls, const ron_loss_cfg* cfg,
                    void* workspace, int64_t workspace_bytes,
                    float* losses, int32_t* counts, const ron_head_grads* grads, void* stream);

/* SSDNet.losses of the two SSD networks -> ssd_losses (nets/ssd_vgg_300.py:580-659, one hard-negative selection over the whole batch;
 * nets/ssd_vgg_512.py:516-607, one per feature layer) with custom_layers.abs_smooth (nets/custom_layers.py:51-63).  TensorFlow runs
 * neither where this library is built; the semantics below are the contract, the choices made where TF raises are marked (*).
 *   heads   : raw logits cls [N,H,W,A,C] and loc [N,H,W,A,4] (obj and anchor_* are not read)
 *   targets : gclasses, glocalisations, gscores of ron_bboxes_encode (gbboxes is not read)
 * Rows are flattened as in ron_losses (layer, image, row, column, anchor).  A segment is the whole batch (S = 1, BATCH) or one layer
 * (S = num_layers, LAYER); R is its row count, N the batch size.  Per row, with logits x, score s and class g:
 *   pos = s > match_threshold; cand = !pos && s > -0.5f; p0 = expf(x[0] - max) / sum (the sum in index order); v = cand ? p0 : 1.0f
 * Per segment, n_pos and n_cand counted as integers:
 *   BATCH  k = min((int)(negative_ratio * (float)n_pos) + N, n_cand)              (:630-632; the cast truncates)
 *   LAYER  k = min(max((int)(negative_ratio * (float)n_pos), R / 8, 4 * N), 1 + n_cand)   (:563-567)
 *   k = min(k, R) (*: top_k raises beyond R); t = the k-th smallest v over all R rows; mined = cand && v < t, strictly, so the k-th
 *   row and its ties are not mined; k == 0 (*: val[-1] raises) mines nothing
 * Terms: ce = sparse softmax cross-entropy (a label < 0 counts as 0, a label >= C gives NaN), sl1(d) = 0.5f*((|d|-1)*min(|d|,1)+|d|)
 *   BATCH  losses[0] = sum_pos ce(x, g) / N, losses[1] = sum_mined ce(x, 0) / N, losses[2] = alpha * (sum_pos sum_4 sl1(loc - gloc) / N)
 *   LAYER  per layer sum_pos ce / n_pos, sum_mined ce / n_mined, alpha * (sum_pos sum_4 sl1 / (4 n_pos)) (tf.losses.
 *          compute_weighted_loss: the sum by the number of non-zero weights), each 0 where its divisor is 0 and the last 0 when
 *          alpha == 0; the layers added in order
 *   losses[3] = (losses[0] + losses[1]) + losses[2]
 *   counts [4 * S] : per segment n_pos, n_cand, k, n_mined (device, int32)
 *   nvalues [rows] or NULL : every row's v
 * Deterministic: integer atomics only, float sums through per-workgroup double partials added in a fixed order; two calls give the
 * same bytes.  Non-finite logits give unspecified selections; the call stays memory safe and terminates.  loc / glocalisations rows
 * move as 16-byte accesses: the layer pointers must be aligned accordingly.
 * workspace: ron_ssd_losses_workspace_bytes(heads, n) bytes of device scratch, 16-byte aligned. */
enum { RON_SSD_MINING_BATCH = 0,   /* ssd_vgg_300.ssd_losses: one selection over the whole batch   */
       RON_SSD_MINING_LAYER = 1 }; /* ssd_vgg_512.ssd_losses: one selection per feature layer      */
typedef struct {
  int mining;
  float match_threshold;    /* 0.5 */
  float negative_ratio;     /* 3   */
  float alpha;              /* 1: weight of the localisation term */
} ron_ssd_loss_cfg;
int64_t ron_ssd_losses_workspace_bytes(const ron_heads* heads, int n);
int ron_ssd_losses(const ron_heads* heads, const ron_targets* targets, int n, const ron_ssd_loss_cfg* cfg,
                   void* workspace, int64_t workspace_bytes, float* losses, int32_t* counts, float* nvalues, void* stream);

/* ron_ssd_losses and, in the same call, d losses[0] + losses[1] / d cls and d losses[2] / d loc (grads->d_obj is not read).  t is a
 * constant with respect to the logits, as top_k's comparison is in TF.
 *   a pos row   : d_cls = (softmax(x) - onehot(g)) * s_pos (a label >= C: a NaN row), d_loc = clamp(loc - gloc, -1, 1) * s_loc
 *   a mined row : d_cls = (softmax(x) - onehot(0)) * s_neg
 *   s_pos, s_neg, s_loc : BATCH 1 / N, 1 / N, alpha / N; LAYER 1 / n_pos, 1 / n_mined, alpha / (4 n_pos), 0 where the term is 0
 * Every element of d_cls and d_loc is written (rows in no set: +0).  `losses` and `counts` are bit for bit those of ron_ssd_losses
 * (the same kernels run).  d_loc rows move as 16-byte accesses.
 * workspace: ron_ssd_losses_grad_workspace_bytes(heads, n) bytes of device scratch, 16-byte aligned. */
int64_t ron_ssd_losses_grad_workspace_bytes(const ron_heads* heads, int n);
int ron_ssd_losses_grad(const ron_heads* heads, const ron_targets* targets, int n, const ron_ssd_loss_cfg* cfg,
                        void* workspace, int64_t workspace_bytes, float* losses, int32_t* counts, float* nvalues,
                        const ron_head_grads* grads, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training preprocessing: ron_preprocess_for_train (preprocessing/ssd_vgg_preprocessing.py:297-356), the chain
 * preprocess_image(is_training=True) runs in front of RONNet.bboxes_encode (ron_net.py:249-306).  Its colour distortion is
 * computed and discarded (:343-348); what reaches the network is
 *   uint8 * (1/255) -> ssd_random_expand with probability 1/2 (tf_image.py:440-467) -> ssd_random_sample_patch (:310-438)
 *   -> random_flip_left_right (:284-308) -> TF1 bilinear resize -> * 255 -> minus the means.
 * TensorFlow's random streams cannot be reproduced: the draws are an input, RON_TRAIN_DRAWS uniform floats in [0, 1) per image
 * at fixed slots (a slot belongs to one decision whether or not that decision is reached):
 *   d[0]  expand unless d[0] < 0.5          d[1], d[2]  expand offsets x, y
 *   d[3]  min_iou = {0.4 .. 0.9}[min(int(d[3] * 6), 5)]       d[4]  flip iff d[4] < 0.5
 *   attempt (o, c) of the overlap loop (o < 10) and the centre loop (c < 10) owns the 12 slots from 5 + (o * 10 + c) * 12:
 *   try t = 0..4 of sample_width_height reads (u_w, u_h) at +2t, +2t+1, the roi position reads (u_x, u_y) at +10, +11.
 * A float draw is (u * (0.999f - 0.1f) + 0.1f) * size, an int draw in [0, m) is min((int)(u * (float)m), m - 1).
 * ---------------------------------------------------------------------------------------- */
#define RON_TRAIN_DRAWS 1205       /* 5 + 10 * 10 * 12 */
#define RON_TRAIN_GEOM 12          /* int32 columns of one geometry row */
/* Every random decision of a batch and its effect on the ground truth, without a host synchronisation (all pointers device):
 *   hw [N, 2], glabels [N, G] int32 (0 = padding; the present rows are a prefix), gbboxes [N, G, 4], 1 <= G <= RON_MAX_GT,
 *   draws [N, RON_TRAIN_DRAWS]
 *   geom [N, RON_TRAIN_GEOM] : {expanded, canvas_h, canvas_w, img_y, img_x, crop_y, crop_x, crop_h, crop_w, flip,
 *                               min_iou index, overlap iterations}: the image sits at (img_y, img_x) of a canvas_h x canvas_w
 *                               canvas (the image itself when not expanded); the crop window of the canvas is flipped or not
 *   glabels_out [N, G], gbboxes_out [N, G, 4] : the kept rows, transformed, at the front in their order, zeros behind
 *   counts [N] : kept rows
 * Padding rows take no part in any test.  All arithmetic is the reference's float32, one rounding per operation. */
int ron_train_geometry(const int32_t* hw, const int32_t* glabels, const float* gbboxes, int n, int g, const float* draws,
                       int32_t* geom, int32_t* glabels_out, float* gbboxes_out, int32_t* counts, void* stream);
/* The pixels for a geometry table: packed / offsets / hw / means as for the evaluation entry above, out [n, out_h, out_w, 3].
 * A canvas sample is (float)u8 * (1.0f / 255.0f) where the image lies and the fill elsewhere; the fill of channel c is
 * (float)((double)sum_c / (255.0 * h * w)) from exact integer channel sums, i.e. the correctly rounded mean colour
 * (tf.reduce_mean leaves the summation order open).  Bilinear over the flipped crop window, then * 255.0f, then - means[c].
 * workspace: that many bytes of device scratch (the channel sums), zeroed by the call itself. */
int64_t ron_preprocess_train_workspace_bytes(int n);
int ron_preprocess_train(const uint8_t* packed, const int64_t* offsets, const int32_t* hw, const int32_t* geom, int n,
                         int out_h, int out_w, const float* means, void* workspace, float* out, void* stream);

/* ------------------------------------------------------------------------------------------
 * Conv stack.  Replaces RONNet.net / ron_net / ron_net_reducedfc
 * (nets/ron_vgg_320.py:136-154, :434-508, :510-580) with slim semantics of ron_arg_scope
 * (:595-629).  Weights enter by TF variable name (SURVEY.md 8b "weight contract").
 * ---------------------------------------------------------------------------------------- */
typedef struct ron_ctx ron_ctx;

typedef struct {
  int32_t variant;          /* ron_variant: which body `net` builds                          */
  int32_t dtype;            /* ron_dtype: arithmetic type of the conv stack                  */
  int32_t img_h, img_w;     /* 320, 320                                                      */
  int32_t num_classes;      /* 21                                                            */
  int32_t max_batch;        /* workspace is sized for this many images per call              */
  int32_t device;           /* HIP device ordinal                                            */
  uint32_t flags;           /* RON_CFG_*                                                     */
} ron_config;
/* Do not materialise block1..block3 (conv1_2, conv2_2, conv3_3 at full resolution): their 2x2 max-pool is
 * fused into the conv epilogue.  ron_end_point_copy then fails for those names. */
#define RON_CFG_FUSE_POOLS 1u
/* Run the head branches of the three coarse scales (block7/6/5: small grids) on internal side streams beside the
 * main chain; ron_forward / ron_detect fork after each reference map and join before returning control to `stream`. */
#define RON_CFG_MULTI_STREAM 2u
/* With RON_CFG_FUSE_POOLS (bf16 / f16) conv1_1 + conv1_2 + pool1 run as ONE kernel that goes from the fp32 image to pool1
 * (neither 64-channel full-resolution map touches HBM).  This flag keeps them as separate launches (A/B tests). */
#define RON_CFG_NO_STEM2 4u
/* The small, mutually independent head convolutions of the coarse scales (block7 / block6 and the 1x1 / skinny ones of
 * block5) run as grouped launches, several convolutions per launch (33 head launches -> 16); this flag keeps one launch
 * per convolution (same results up to the order of the fp32 partial sums: the split of K differs; tests compare the two). */
#define RON_CFG_NO_GROUPS 8u
/* Small maps with large filters spend a good part of their MACs on the zero halo (fc6: 7x7 on 10 x 10, 31 %; conv6 of SSD-512;
 * the 3x3 heads of the 5 x 5 / 10 x 10 scales).  By default such launches order their GEMM rows by output row first (output row,
 * image, column) and every tile skips the filter rows that fall outside the image for all of its rows, walking the others from the
 * filter's centre row (only products with zeros go; the fp32 sums are taken in another order, so the last bit may differ).
 * This flag keeps the image-major order and the full K loop (tests compare the two). */
#define RON_CFG_NO_HALO_SKIP 16u
/* Which grouped plan the RON heads run: by default contexts with max_batch <= 12 launch the heads one launch per dependency
 * level (7 launches, the large convolutions grouped too: at such batches every launch is latency-bound); 13..23: mixed-width
 * level groups with the large layers on their own; >= 24: small convolutions packed into the partial rounds of 256 x 256-tile
 * launches (csrc/graph.cpp, plan_groups).  RON_CFG_LEVEL_GROUPS forces the level plan, RON_CFG_BATCH_GROUPS the plan max_batch
 * would select without the level rule (A/B tests; same results up to the order of the fp32 partial sums). */
#define RON_CFG_LEVEL_GROUPS 32u
#define RON_CFG_BATCH_GROUPS 64u
/* With RON_CFG_FUSE_POOLS a pool on an ODD map (SSD-300: conv3_3 75 x 75 -> pool3 38 x 38) is fused like the others: the last row /
 * column of windows then holds tile rows that are no pixel of the map.  This flag keeps such a pool a launch of its own (A/B tests:
 * tools/bench_ssd300.py --ab-pool3; same results bit for bit). */
#define RON_CFG_NO_ODD_POOL_FUSE 128u

int ron_create(ron_ctx** out, const ron_config* cfg);
int ron_destroy(ron_ctx* ctx);
/* A second execution slot over the weights of `src` (finalized): own activations, head buffers, scratch and streams,
 * so that several batches can be in flight on different streams (a serving loop keeps the GPU's 256 CUs busy across the
 * partial last round of workgroups every launch ends with).  Destroy the slots before the context that owns the weights. */
int ron_clone(ron_ctx* src, ron_ctx** out);

/* Number of variables the graph expects and the i-th name/shape ("ron_320_vgg/conv1/conv1_1/weights",
 * HWIO for conv, [kh,kw,Cout,Cin] for deconv, as TF stores them). */
int ron_num_variables(const ron_ctx* ctx);
int ron_variable_info(const ron_ctx* ctx, int i, const char** name, int64_t shape[4], int* ndim);
/* Host fp32 data for one variable (copied). */
int ron_load_weight(ron_ctx* ctx, const char* tf_name, const float* host_ptr,
                    const int64_t* shape, int ndim);
/* Fold BatchNorm (eps 1e-5), fuse parallel branches, repack to the kernel layout, cast, upload. */
int ron_finalize_weights(ron_ctx* ctx);

/* Filled by ron_forward: device fp32 tensors owned by the CALLER (ron_heads.cls/obj/loc must
 * point at writable buffers of the right size; anchor_* are filled in from the ctx). */
int ron_heads_describe(const ron_ctx* ctx, ron_heads* heads);   /* shapes + ctx anchor pointers */
int ron_forward(ron_ctx* ctx, const float* d_images, int n, ron_heads* d_out, void* stream);

/* Copy an end_point (nets/ron_vgg_320.py:455-483: block1..block7, plus every internal
 * activation by layer name) as dense fp32 NHWC into `d_out`; shape returned in nhwc. */
int ron_end_point_shape(const ron_ctx* ctx, const char* name, int n, int64_t nhwc[4]);
int ron_end_point_copy(ron_ctx* ctx, const char* name, int n, float* d_out, void* stream);

/* Fused: forward + np_methods post-processing, the graded path (config 2/3 of BASELINE.json). */
int ron_detect(ron_ctx* ctx, const float* d_images, int n, const ron_post_cfg* cfg,
               ron_detections* out, void* stream);

/* Fused: forward + TF-evaluation post-processing (what eval_ron_network.py:209-236 runs: net -> bboxes_decode -> objectness
 * gate -> detected_bboxes), one enqueue, the results of ron_forward followed by ron_post_tfe on raw heads bit for bit.
 *   scores [n, C-1, keep_top_k], bboxes [n, C-1, keep_top_k, 4]: device fp32, caller-owned, the layout ron_post_tfe writes.
 * cfg is checked as ron_post_tfe checks it, before anything is enqueued; cfg->input_flags is ignored (the context's raw heads go
 * in).  The objectness gate applies when the network has objectness heads (RON), not for SSD-512.  Runs in the post-processing
 * workspace ron_detect uses (no allocation); ron_detect and ron_detect_tfe may alternate on one context in any order and with
 * any n, on one stream as ron_detect's calls.  Its lists' counters clean themselves like ron_detect's; the first ron_detect_tfe
 * after a ron_detect zeroes them once (a memset of (C-1) ints per image of max_batch) because ron_detect's keys share their
 * bytes.  Profiling: the post stage is the last ron_profile_get index, as for ron_detect. */
int ron_detect_tfe(ron_ctx* ctx, const float* d_images, int n, const ron_tfe_cfg* cfg,
                   float* scores, float* bboxes, void* stream);

/* Algorithmic work of one image through the conv stack (2*MAC of conv + deconv). */
double ron_flops_per_image(const ron_ctx* ctx);

/* Per-launch timing with HIP events on the caller's stream (what bench.py's roofline uses; the reference's
 * only timing is wall-clock prints, eval_ron_network.py:353,363-366).  ron_profile_enable(ctx, n) makes the next n
 * ron_forward / ron_detect calls record one event per launch on the launch's stream (n = 0: off); ron_profile_get synchronises on the recorded events and
 * returns, for launch i (the last index is the post-processing stage of ron_detect), its name, whether it is
 * the implicit-GEMM conv kernel, its algorithmic FLOPs per image, the accumulated time and launch count, and its
 * algorithmic HBM bytes (activations in + out per image; packed weights once per launch).  A grouped launch (several small
 * head convolutions in one launch) is reported on its first member as "group[first+N]", the other members as "(name)" with
 * no work of their own.  *name points into the context and stays valid until ron_destroy. */
int ron_profile_enable(ron_ctx* ctx, int enable);
int ron_profile_num_ops(const ron_ctx* ctx);
/* Grouped launches in the plan of this context: RON-320 10 (max_batch >= 24), 7 (13..23), 6 (the level plan, <= 12 or
 * RON_CFG_LEVEL_GROUPS); SSD-512 5; SSD-300 4 (the heads of block8 .. block11, each with the next block's 1x1 where there is one);
 * 0 with RON_CFG_NO_GROUPS / RON_CFG_MULTI_STREAM. */
int ron_num_grouped_launches(const ron_ctx* ctx);
int ron_profile_get(ron_ctx* ctx, int i, const char** name, int* is_conv, double* flops_per_image,
                    double* total_ms, int* launches, double* act_bytes_per_image, double* weight_bytes);
int ron_profile_reset(ron_ctx* ctx);

/* ------------------------------------------------------------------------------------------
 * Single operators (used by the parity tests to pin each kernel against the oracle).
 * conv2d NHWC: x [n,h,w,cin] fp32 (device), w HWIO fp32 [kh,kw,cin,cout] and bias [cout] or NULL (HOST
 * pointers: they are packed on the host like ron_finalize_weights does), residual [n,ho,wo,cout] (device)
 * or NULL: y = act(conv + bias) ; if residual: y = relu(y + residual).  These two calls allocate scratch
 * and synchronise the stream (test / tooling use, not for graph capture).
 * `dtype` selects the arithmetic (operands rounded to bf16/f16, fp32 accumulate).
 * transpose != 0: slim.conv2d_transpose with kernel = stride (weights [kh,kw,cout,cin]).
 *
 * The envelope of ron_conv_desc, the same for every entry point that takes one (the kernels carry these fields in a few bits
 * each; a value beyond them is refused, never wrapped):
 *   kh, kw 1 .. 15; stride 1 .. 7; transposed kernel == stride 1 .. 7; dilation 1 .. 31; SAME padding (kh - 1) * dilation / 2 <= 63;
 *   relu, pool, transpose 0 or 1; n, h, w, cin, cout >= 1.
 * Filters are square (kh == kw); at stride 1 they are odd (an even filter's SAME padding is one pixel wider behind than in front,
 * which the shared halo cannot hold); a strided convolution has kernel == stride on a map that stride divides.  Anything else
 * is RON_ERR_INVALID with a message, before any allocation or launch.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n, h, w, cin, cout;
  int32_t kh, kw, stride, dilation;
  int32_t relu;
  int32_t transpose;
  int32_t dtype;            /* ron_dtype */
  int32_t tile_cfg;         /* -1 = by shape (what the graph does), else one of the ron_conv_num_tile_cfgs() selectable
                               configurations (csrc/conv_mfma.h kCfg*: 0-3 and 7 row-gather tiles, 4-6 halo-patch N tiles,
                               8 the resident-weight 3x3 kernel for 64-channel maps);
                               anything else, or one that does not cover this conv, is RON_ERR_INVALID             */
  int32_t in_cstride;       /* tooling: input laid out as a channel slice: elements per pixel (0 = cin) ...   */
  int32_t in_coff;          /* ... and first channel of the slice                                              */
  int32_t pool;             /* fuse a 2x2 stride-2 SAME max-pool into the epilogue: y is [n, ceil(h/2), ceil(w/2), cout] */
  int32_t splitk;           /* split-K factor: -1 = by grid size, 1 = off                                      */
  int32_t center_from;      /* > 0: output channels >= center_from have weights in the centre tap only (the caller's w is
                             * zero elsewhere): their column tiles run that tap's K steps alone.  0 = none              */
} ron_conv_desc;
int ron_conv2d_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias,
                    const float* residual, float* y, void* stream);
/* d->pool != 0 with the un-pooled map as a second output of the same launch (what the graph does for conv4_3 / conv5_3 under
 * RON_CFG_FUSE_POOLS): y_pooled [n, ceil(h/2), ceil(w/2), cout], y_full [n, h, w, cout].  Row-gather tiles only. */
int ron_conv2d_pool2_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias, float* y_pooled,
                          float* y_full, void* stream);
/* How ron_conv2d_nhwc would run `d`, without running it (tests, tools): out = {tile configuration (csrc/conv_mfma.h kCfg*),
 * split-K factor, tile order (0 = column tiles fastest inside an XCD's run, 1 = row tiles fastest, P >= 2 = panels of P column tiles
 * walked row by row), K order (1 = taps innermost)}.  Allocates and frees the operands like ron_conv2d_nhwc does. */
int ron_conv_plan(const ron_conv_desc* d, int32_t out[4]);
/* ... and the columns of the row-gather kernel's tile for the same launch: the width of the tile configuration (64 / 128 / 256), or 224
 * where a bf16 / f16 convolution of 193 .. 224 output channels runs the four-wave 256 x 256 configuration on its 256 x 224 form
 * (environment RON_IGEMM224=0, read per call by the single-operator entry points only - a test / sweep hook, the graph does not
 * read it: never); 0 for the halo-patch and resident-weight kernels. */
int ron_conv_plan_n_tile(const ron_conv_desc* d, int32_t* n_tile);
/* Tests / tooling: one or two plain stride-1 convolutions (db NULL: one), each over its own input, with the fp32 output of the
 * graph's head layers - the kernel's epilogue writes y [n,h,w,cout] (device, fp32) itself.  grouped = 0: launches of their own
 * (tile_cfg / splitk of each descriptor); grouped != 0: both as the members of ONE grouped launch of 256 x 256 tiles (what the
 * batch plan does with the class heads of the coarse scales; both padded widths must be multiples of 256 and tile_cfg -1 or 0,
 * else RON_ERR_INVALID; splitk of the descriptors when both are >= 1, else the group's own plan).  n_tiles (may be NULL): the
 * column-tile width each convolution ran on (64 / 128 / 256, or 224), one per convolution. */
int ron_conv2d_f32out_nhwc(const ron_conv_desc* da, const float* xa, const float* wa, const float* ba, float* ya,
                           const ron_conv_desc* db, const float* xb, const float* wb, const float* bb, float* yb,
                           int grouped, int32_t* n_tiles, void* stream);
/* Tests / tooling: the skinny heads of a scale as the batch plan launches them - two plain 3x3 convolutions of at most 64 output
 * channels over channel slices of ONE tensor x [n,h,w,in_cstride] (device fp32; both descriptors carry the same in_cstride > 0 and
 * their own in_coff), as one launch of the halo-patch pair kernel, fp32 outputs ya / yb [n,h,w,cout] (device).  bf16 / f16: a pair of
 * up to 32 and up to 48 output channels multiplies 32 + 48 columns instead of 64 + 64; full_width != 0 keeps 64 + 64.
 * columns (may be NULL): the columns each member multiplies. */
int ron_conv2d_patch_pair_nhwc(const ron_conv_desc* da, const ron_conv_desc* db, const float* x, const float* wa, const float* ba,
                               const float* wb, const float* bb, float* ya, float* yb, int full_width, int32_t* columns, void* stream);
/* Two fp32 head tensors from one convolution over a shared input - the class and the box convolution of an SSD feature layer
 * (nets/ssd_vgg_300.py:403-431), which the SSD-512 graph runs as one launch: w HWIO [kh,kw,cin,cout], its first `split_first`
 * output channels go to y_first [n,h,w,split_first], the other cout - split_first to y_second [n,h,w,cout - split_first]
 * (both fp32, device).  d: a plain stride-1 convolution (no transpose / pool); tile_cfg and splitk select the launch as in
 * ron_conv2d_nhwc. */
int ron_conv2d_heads_nhwc(const ron_conv_desc* d, int split_first, const float* x, const float* w, const float* bias,
                          float* y_first, float* y_second, void* stream);
/* slim.max_pool2d [2, 2] stride 2, padding SAME: y is [n, ceil(h/2), ceil(w/2), c]; the last window of an odd map holds one row /
 * column.  ron_conv2d_nhwc with `pool` produces the same map from the convolution's accumulators. */
int ron_maxpool2x2_nhwc(const float* x, int n, int h, int w, int c, int dtype, float* y, void* stream);
/* Tooling: time the conv kernel alone on random data (ms per launch, HIP events, default stream, synchronises). */
int ron_conv2d_bench(const ron_conv_desc* d, int warmup, int iters, float* ms_per_launch);
int ron_conv_num_tile_cfgs(void);
/* Tooling: workgroups of the fused stem kernel (conv1_1 + conv1_2 + pool1, bf16 / f16) that fit one CU of the current device, as the
 * runtime's occupancy query answers for the launch's block and LDS size.  ron_forward requires 2 and fails otherwise. */
int ron_stem2_workgroups_per_cu(int dtype, int32_t* per_cu);

/* ------------------------------------------------------------------------------------------
 * Convolution backward: the gradients of ONE stride-1 SAME convolution (every VGG body layer, fc6 / fc7, conv6 / conv7,
 * the stride-1 convolutions of the SSD extra blocks, every head).  Unlike the test operators above this is a real entry
 * point: it enqueues on `stream`, allocates nothing, never synchronises, honours the dry-run mode, and assumes nothing
 * about the workspace's contents (every halo and guard zero it relies on is written by the call).
 *
 * Operands are rounded to d->dtype (bf16 or fp16) and accumulated in fp32, like the forward:
 *   dz    = round(dy * (y > 0)) when d->relu (TF's ReluGrad: no gradient where y == 0), else round(dy)
 *   dx    = round(conv_SAME(dz, w')), w'[ky,kx,co,ci] = round(w)[kh-1-ky, kw-1-kx, ci, co], same dilation; delivered as
 *           storage-type values in fp32, as ron_conv2d_nhwc delivers y
 *   dw[ky,kx,ci,co] = sum over n, y, x of round(x)[n, y + ky*dil - pad, x + kx*dil - pad, ci] * dz[n,y,x,co]: an fp32 sum,
 *           not rounded further; terms outside the map are zero
 *   dbias[co] = sum of dz[..., co]: the rounded dz, in fp32
 * The sums run in a fixed order: the same inputs give the same bytes on every call.
 *
 * All pointers are DEVICE fp32, w included (weights live on the device in training): x [n,h,w,cin], w and dw HWIO
 * [kh,kw,cin,cout], y and dy [n,h,w,cout], dx [n,h,w,cin], dbias [cout].  y is read only when d->relu.  dx, dw, dbias may
 * each be NULL (not computed); every element of a non-NULL output is written.  x may be NULL when dw is, w when dx is.
 * x, y and dy must be 16-byte aligned (they are read 16 bytes at a time), the workspace 256-byte aligned.
 *
 * Accepted descriptors: stride 1, kh == kw in {1, 3} at dilation 1 .. 31 (the envelope of ron_conv_desc above: the data
 * gradient is a forward launch) or 7 x 7 at dilation 1 (fc6 of the `full` variant; 5 x 5 and a dilated 7 x 7 have no user and
 * are refused), dtype bf16 / fp16, cin a multiple of 64, any cout >= 1; relu 0 or 1; transpose, pool, center_from, in_cstride, in_coff = 0 and tile_cfg = -1.  d->splitk is the pixel-split
 * factor of the weight gradient: -1 = by shape, 1 = off, S = forced (capped at the number of 32-pixel steps and where the
 * fp32 partial sums of the slices would reach 2 GiB).  Anything else - a NULL y with relu set, a misaligned pointer and a
 * workspace that is too small included - is RON_ERR_INVALID with a message, before any HIP call.
 * Out of scope: the 3-channel stem (ron_conv2d_stem_backward_nhwc below), strided and transposed convolutions, pools (the 2x2 stride-2 ones have entry points of
 * their own below), fp32 and f16x3 arithmetic.
 * ron_conv2d_backward_workspace_bytes is host arithmetic only (it depends on d->splitk too); -1 + ron_last_error() on a
 * descriptor the call would refuse.
 * ---------------------------------------------------------------------------------------- */
int64_t ron_conv2d_backward_workspace_bytes(const ron_conv_desc* d);
int ron_conv2d_backward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* y, const float* dy,
                             float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution forward for training: ONE convolution from DEVICE weights, the forward that ron_conv2d_backward_nhwc,
 * ron_conv2d_stem_backward_nhwc and ron_conv2d_k2s2_backward_nhwc differentiate.  Its contract is that of
 * ron_conv2d_backward_nhwc: a real entry point that enqueues on `stream`, allocates nothing, never synchronises, honours the
 * dry-run mode and assumes nothing about the workspace's contents; every element of y is written.
 *
 * All pointers are DEVICE fp32, w and bias included (the optimizer changes them on the device every step; nothing is cached
 * between calls): x [n,h,w,cin], w HWIO [kh,kw,cin,cout] ([2,2,cout,cin] when d->transpose), bias [cout] or NULL, y
 * [n,ho,wo,cout] with (ho, wo) = (h, w) at stride 1, (h/2, w/2) for the strided and (2h, 2w) for the transposed form.  x and y
 * must be 16-byte aligned (the x of the 3-channel stem: 4-byte), w and bias 4-byte, the workspace 256-byte aligned.
 *
 * The arithmetic is ron_conv2d_nhwc's: operands rounded to d->dtype, fp32 accumulation, + fp32 bias, ReLU when d->relu, y
 * delivered as storage-type values in fp32.  It is the same launch on the same packed operands with the by-shape plan
 * (tile_cfg = -1, splitk = -1) - only the packing moved from the host to the stream - so for the same inputs y has the same
 * bytes as ron_conv2d_nhwc's.
 *
 * Accepted descriptors (dtype bf16 / fp16; relu 0 or 1; pool, center_from, in_cstride, in_coff = 0; tile_cfg = -1,
 * splitk = -1):
 *   - stride 1 SAME, kh == kw in {1, 3} at dilation 1 .. 31, or 7 x 7 at dilation 1; cin a multiple of 64, any cout >= 1;
 *   - the stem: cin 3, cout 64, 3 x 3, dilation 1, any width (with relu the stem kernel, without it im2col + one GEMM step:
 *     the routes of ron_conv2d_nhwc);
 *   - kh = kw = stride = 2, transpose 0: h and w even, cin a multiple of 64;
 *   - kh = kw = stride = 2, transpose 1: cin a multiple of 64, cout a multiple of 128.
 * There is no residual argument: a fused relu(y + residual) loses the mask of the inner ReLU that the backward needs, so the
 * join stays with the caller.  Out of scope: fp32 and f16x3 arithmetic, fused pools, channel slices, forced tile
 * configurations, the padded convolutions of the SSD extra blocks (ron_conv2d_nhwc runs those).
 * Anything else - a NULL x, w or y, a misaligned pointer, a workspace that is too small, a packed tensor that would reach
 * 2 GiB - is RON_ERR_INVALID with a message, before any HIP call.
 * ron_conv2d_forward_workspace_bytes is host arithmetic only; -1 + ron_last_error() on a descriptor the call would refuse.
 * ---------------------------------------------------------------------------------------- */
int64_t ron_conv2d_forward_workspace_bytes(const ron_conv_desc* d);
int ron_conv2d_forward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                            void* workspace, int64_t workspace_bytes, void* stream);
/* Tooling (tools/conv_forward_time.py): the same call restricted to some of its steps, so that each can be timed alone on a
 * workspace an earlier full call has filled: the pack of x, the packs of w and the bias, the convolution launch, the unpack
 * into y.  Same checks, same contract; RON_FWD_PART_ALL is ron_conv2d_forward_nhwc. */
enum { RON_FWD_PART_X = 1, RON_FWD_PART_W = 2, RON_FWD_PART_LAUNCH = 4, RON_FWD_PART_UNPACK = 8, RON_FWD_PART_ALL = 15 };
int ron_conv2d_forward_parts_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* bias, float* y,
                                  void* workspace, int64_t workspace_bytes, int parts, void* stream);

/* ------------------------------------------------------------------------------------------
 * Convolution chain: a SEQUENCE of layers - stride-1 SAME convolutions and 2x2 stride-2 SAME max-pools - forward in one call
 * and backward in one call: conv1_2 .. fc7 of both RON-320 variants, conv1_2 .. conv5_3 of the SSD networks.  Between the
 * layers, and between the two calls, activations and gradients stay storage-type (bf16 / fp16) halo tensors inside the
 * caller's workspace; fp32 dense NHWC appears only where data enters or leaves: x, y, the taps, dx, and the weights, biases
 * and their gradients.  The contract is that of ron_conv2d_forward_nhwc / ron_conv2d_backward_nhwc: both calls enqueue on
 * `stream`, allocate nothing, never synchronise, honour the dry-run mode; ron_conv_chain_forward assumes nothing about the
 * workspace's contents; everything refusable is RON_ERR_INVALID with a message, before any HIP call.
 *
 * The chain starts from a map [n,h,w,cin], cin a multiple of 64 (the stem's caller feeds its output as x and takes dx into
 * ron_conv2d_stem_backward_nhwc).  Layers:
 *   RON_CHAIN_CONV   k in {1, 3} at dilation 1 .. 31, or k = 7 at dilation 1; relu and has_bias 0 or 1; cout >= 1 on the last
 *                    layer, a multiple of 64 on a layer that feeds another one: what ron_conv2d_forward_nhwc and
 *                    ron_conv2d_backward_nhwc accept for a stride-1 convolution;
 *   RON_CHAIN_POOL2  the 2x2 stride-2 SAME max-pool, odd maps included (ron_maxpool2x2_nhwc, ron_maxpool2x2_backward_nhwc);
 *                    k, dilation, cout, relu, has_bias are ignored.
 * A convolution layer may be flagged `tap`: the forward also delivers its output as fp32 dense (taps[i]); the backward takes
 * an fp32 dense gradient for it (dtaps[i], NULL: none; dtaps itself may be NULL), and the gradient that enters the layer's ReLU
 * mask is float(the next layer's dx) + dtaps[i], added in fp32 before the one rounding - the sum autograd forms when the
 * operators are chained.  The last layer's output is always delivered (y) and dy is its gradient; a tap flag on it delivers
 * taps[i] as well and adds dtaps[i] to dy.  A pool layer cannot be tapped.
 *
 * Arithmetic: every convolution layer runs the launches ron_conv2d_forward_nhwc / ron_conv2d_backward_nhwc make for it on
 * its own (the same plan code, csrc/conv_train.h: views, by-shape tile and split, channel padding; only the base pointers
 * differ), the same weight packs and column sums, and the pools compare and route the same stored values.  y, every tap, dx,
 * every dw and every dbias therefore have the bytes that the per-operator entry points give when they are chained through
 * fp32, for any input.
 *
 * Pointer arrays (w, bias, taps, dtaps, dw, dbias) are HOST arrays of num_layers DEVICE pointers; entries of pool layers are
 * ignored.  w[i] is fp32 HWIO [k,k,cin_i,cout_i], packed on the stream at every call (nothing is cached: the optimizer
 * changes it every step); bias[i] is [cout_i], read when has_bias.  x [n,h,w,cin], y and dy the last layer's output shape
 * (ron_conv_chain_shape), taps[i] / dtaps[i] layer i's.  x, y, dy, dx, taps and dtaps entries must be 16-byte aligned, the
 * other pointers 4-byte, the workspace 256-byte.
 *
 * ron_conv_chain_backward reads the activations ron_conv_chain_forward left in the SAME workspace (same descriptor) and does not
 * destroy them: it may be called any number of times after one forward and gives the same bytes each time.  dx, any dw[i],
 * any dbias[i] (and the arrays dw, dbias themselves) may be NULL: not computed.  Launches whose results nobody asked for are
 * skipped: without dx the first layer's data gradient is not launched, and layers in front of the first requested gradient do
 * not run at all.  Every element of a non-NULL output is written.  w[i] of every convolution layer must be given to both calls.
 *
 * The workspace is 64-bit sized; each tensor inside it stays below 2 GiB (a larger one is refused).
 * ron_conv_chain_workspace_bytes is host arithmetic only; -1 + ron_last_error() on a descriptor the calls would refuse.
 * ron_conv_chain_shape: the output shape of `layer`.
 * Out of scope: the stem; the 3x3 stride-1 pool and the L2 normalisation; the 2x2 stride-2 convolutions; fp32 and f16x3
 * arithmetic; taps on pool layers.  Batch normalisation and the two-branch convolution: ron_head_chain_* below.
 * ---------------------------------------------------------------------------------------- */
enum { RON_CHAIN_CONV = 0, RON_CHAIN_POOL2 = 1 };
#define RON_CHAIN_MAX_LAYERS 32
typedef struct {
  int32_t kind;             /* RON_CHAIN_CONV / RON_CHAIN_POOL2 */
  int32_t k, dilation, cout, relu, has_bias;
  int32_t tap;
} ron_chain_layer;
typedef struct {
  int32_t n, h, w, cin;
  int32_t dtype;            /* ron_dtype: bf16 or fp16 */
  int32_t num_layers;
  ron_chain_layer layers[RON_CHAIN_MAX_LAYERS];
} ron_chain_desc;
int ron_conv_chain_shape(const ron_chain_desc* d, int layer, int64_t nhwc[4]);
int64_t ron_conv_chain_workspace_bytes(const ron_chain_desc* d);
int ron_conv_chain_forward(const ron_chain_desc* d, const float* x, const float* const* w, const float* const* bias,
                           float* const* taps, float* y, void* workspace, int64_t workspace_bytes, void* stream);
int ron_conv_chain_backward(const ron_chain_desc* d, const float* dy, const float* const* dtaps, const float* const* w,
                            float* dx, float* const* dw, float* const* dbias, void* workspace, int64_t workspace_bytes,
                            void* stream);

/* ------------------------------------------------------------------------------------------
 * Head chain: the convolution chain with two more layer kinds - training-mode batch normalisation and the two-branch
 * 3x3 | 1x1 convolution of pred_cls_module - so that every branch of a reverse_connection_module_with_pred
 * (nets/ron_vgg_320.py:378-432) is one chain: `_conv_left` (conv, BN), `_objectness` + `_objectness_score` (conv, BN, conv),
 * pred_cls_module (pair, BN, pair, BN, conv), reg_bbox_module (conv, BN, conv).  One planner and one runner serve both
 * families: ron_conv_chain_* is the case "no BN, no pair" of these entry points, with the same launches.  Everything the
 * convolution chain's contract says holds here (stream-ordered, no allocation, no synchronisation, dry run, refusals before
 * any HIP call, nothing assumed about the workspace's contents, the backward repeatable); RON_CHAIN_CONV and RON_CHAIN_POOL2
 * layers are the same.
 *
 *   RON_CHAIN_BN         batch normalisation of the previous layer's stored output with batch statistics over M = n h w, then
 *                        ReLU when `relu`: the contract of ron_batchnorm_train_nhwc / ron_batchnorm_backward_nhwc (its
 *                        geometry, shifted sums, Chan merges and fixed tree for this (M, c); rstd recomputed in the backward),
 *                        read and written as storage-type halo tensors.  The input already holds storage-type values, so
 *                        round(x) is the identity.  eps finite and >= 0, decay in [0, 1]; M at most 2^24.  moving_mean /
 *                        moving_var (both or neither) are updated in place by the forward.  mean and var stay in the workspace
 *                        for the backward and are also written to mean / var when those are not NULL.  May be the first layer,
 *                        the last one, follow a pool or another BN.  k, dilation, cout, cout2, has_bias are ignored.
 *   RON_CHAIN_CONV_PAIR  concat(conv3x3(x, w, bias), conv1x1(x, w2, bias2)) along the channels: cout channels of the 3x3
 *                        branch, then cout2 of the 1x1; both multiples of 64; relu and has_bias apply to both; k and dilation
 *                        are ignored.  Each branch runs the launches ron_conv2d_forward_nhwc / ron_conv2d_backward_nhwc make
 *                        for it on its own and writes its channel slice of one tensor.  The gradient of the pair's input is
 *                        float(dx of the 3x3) + float(dx of the 1x1) in fp32 - two terms, so the order does not matter -
 *                        which then enters the previous layer's mask and single rounding, or leaves as dx unrounded.
 * A chain that starts with a convolution or a pair needs cin a multiple of 64, as the convolution chain does; one that starts
 * with a batch normalisation or a pool a multiple of 8 (a convolution further on still asks for its 64).
 * Taps: convolution layers only.  A tap on a BN or pair layer is refused (not built), and so is a pair directly behind a
 * tapped layer (that gradient would be a sum of three terms whose order autograd does not fix).
 *
 * Bytes: y, taps, mean, var, the moving statistics, dx and every parameter gradient are those of the per-operator entry points
 * chained through fp32 (the pair: the two convolutions and a concatenation; BN: ron_batchnorm_*), for any input.
 *
 * Pointers travel as a HOST array of num_layers ron_head_chain_ptrs, one per layer; members a layer's kind does not use are
 * ignored.  The forward reads w, bias, w2, bias2, gamma, beta, updates moving_mean / moving_var and writes mean, var, tap;
 * the backward reads w, w2, gamma, dtap and writes dw, dbias, dw2, dbias2, dgamma, dbeta (each may be NULL: not computed; layers
 * in front of the first requested gradient do not run).  x, y, dy, dx, tap, dtap and every BN vector must be 16-byte
 * aligned, weights, biases and their gradients 4-byte, the workspace 256-byte.
 * ---------------------------------------------------------------------------------------- */
enum { RON_CHAIN_BN = 2, RON_CHAIN_CONV_PAIR = 3 };
typedef struct {
  int32_t kind;             /* RON_CHAIN_CONV / RON_CHAIN_POOL2 / RON_CHAIN_BN / RON_CHAIN_CONV_PAIR */
  int32_t k, dilation, cout, relu, has_bias;
  int32_t tap;
  int32_t cout2;            /* RON_CHAIN_CONV_PAIR: channels of the 1x1 branch */
  float eps, decay;         /* RON_CHAIN_BN */
} ron_head_chain_layer;
typedef struct {
  int32_t n, h, w, cin;
  int32_t dtype;            /* ron_dtype: bf16 or fp16 */
  int32_t num_layers;
  ron_head_chain_layer layers[RON_CHAIN_MAX_LAYERS];
} ron_head_chain_desc;
typedef struct {
  const float* w;           /* conv, pair (3x3 branch): HWIO */
  const float* bias;
  const float* w2;          /* pair: the 1x1 branch [1,1,cin,cout2] */
  const float* bias2;
  const float* gamma;       /* BN [c] */
  const float* beta;
  float* moving_mean;       /* BN [c], updated in place by the forward; both or neither */
  float* moving_var;
  float* mean;              /* out, forward: BN batch statistics [c] (NULL: kept in the workspace only) */
  float* var;
  float* tap;               /* out, forward: a tapped convolution's output */
  const float* dtap;        /* in, backward: its gradient (NULL: none) */
  float* dw;                /* out, backward */
  float* dbias;
  float* dw2;
  float* dbias2;
  float* dgamma;
  float* dbeta;
} ron_head_chain_ptrs;
int ron_head_chain_shape(const ron_head_chain_desc* d, int layer, int64_t nhwc[4]);
int64_t ron_head_chain_workspace_bytes(const ron_head_chain_desc* d);
int ron_head_chain_forward(const ron_head_chain_desc* d, const float* x, const ron_head_chain_ptrs* p, float* y, void* workspace,
                           int64_t workspace_bytes, void* stream);
int ron_head_chain_backward(const ron_head_chain_desc* d, const float* dy, const ron_head_chain_ptrs* p, float* dx, void* workspace,
                            int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the 3-channel stem convolution conv1_1 (3 -> 64 channels, 3x3, stride 1, SAME): its weight and bias
 * gradients, the two variables ron_conv2d_backward_nhwc cannot reach.  There is no gradient with respect to the image
 * (nothing takes one), hence no w and no dx.  A real entry point like the convolution backward: it enqueues on `stream`,
 * allocates nothing, never synchronises, honours the dry-run mode and assumes nothing about the workspace's contents.
 *
 * The semantics are those of ron_conv2d_backward_nhwc, restricted to dw and dbias:
 *   xs    = round(x) to d->dtype (what the forward's stem kernel multiplies)
 *   dz    = round(dy * (y > 0)) when d->relu (TF's ReluGrad: nothing where y == 0), else round(dy)
 *   dw[ky,kx,c,co] = sum over n, i, j of xs[n, i+ky-1, j+kx-1, c] * dz[n,i,j,co]: an fp32 sum, not rounded further; terms
 *           outside the map are zero; HWIO [3,3,3,64]
 *   dbias[co] = sum of dz[..., co]: the rounded dz, in fp32
 * The sums run in a fixed order (no float atomics): the same inputs give the same bytes on every call, for every split.
 *
 * All pointers are DEVICE fp32: x [n,h,w,3], y and dy [n,h,w,64], dw [3,3,3,64], dbias [64].  y and dy must be 16-byte
 * aligned (they are read 16 bytes at a time); x needs its natural 4-byte alignment only (a pixel is 12 bytes); the
 * workspace is 256-byte aligned.  y is read only when d->relu.  dw and dbias may each be NULL (not computed); every element
 * of a non-NULL output is written; with both NULL the call is accepted and enqueues nothing.  x may be NULL when dw is.
 *
 * Accepted descriptors: cin 3, cout 64, kh = kw = 3, stride 1, dilation 1 (the convolution the forward runs on its 3-channel
 * path); dtype bf16 / fp16; relu 0 or 1; transpose, pool, center_from, in_cstride, in_coff = 0 and tile_cfg = -1;
 * n, h, w >= 1 with n * h * w <= RON_STEM_BACKWARD_MAX_PIXELS: the kernel counts pixels, rounded up to its step of 32, in
 * 32-bit signed integers, and a larger tensor is refused, never wrapped.  d->splitk is the number of pixel slices: -1 = by
 * shape, 1 = off, S = forced (capped at the number of 32-pixel steps and where the fp32 partial sums of the slices would
 * reach 2 GiB).  Anything else - a NULL y with relu set, a misaligned y or dy and a workspace that is too small included -
 * is RON_ERR_INVALID with a message, before any HIP call.
 * ron_conv2d_stem_backward_workspace_bytes is host arithmetic only (it depends on d->splitk); -1 + ron_last_error() on a
 * descriptor the call would refuse.
 * ---------------------------------------------------------------------------------------- */
#define RON_STEM_BACKWARD_MAX_PIXELS 2147483616 /* 2^31 - 32 */
int64_t ron_conv2d_stem_backward_workspace_bytes(const ron_conv_desc* d);
int ron_conv2d_stem_backward_nhwc(const ron_conv_desc* d, const float* x, const float* y, const float* dy, float* dw,
                                  float* dbias, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the 2x2 stride-2 SAME max-pool (slim.max_pool2d [2, 2], pool1 .. pool5: nets/ron_vgg_320.py:456..475,
 * nets/ssd_vgg_300.py:450..462).  A real entry point like the convolution backward: it enqueues on `stream`, allocates
 * nothing, never synchronises, needs no workspace and honours the dry-run mode.
 *
 * x [n,h,w,c] is the pool's input, dy [n,ceil(h/2),ceil(w/2),c], dx [n,h,w,c]: device fp32, 16-byte aligned.  With
 * xs = round(x) to `dtype` (what ron_maxpool2x2_nhwc pools): dx[n,i,j,ch] = round(dy[n,i/2,j/2,ch]) if (i, j) is the FIRST
 * position of its window, in the order (0,0) (0,1) (1,0) (1,1), whose xs equals the window's maximum, else 0 (TensorFlow's
 * MaxPoolGrad).  The comparison is on the rounded values: inputs that agree after rounding are a tie, and so are -0.0 and
 * +0.0.  On an odd map the last window holds one row and / or one column; positions that do not exist are neither read nor
 * written.  A window that holds a NaN is outside the contract (the forward drops NaNs).
 * Every element of dx is written exactly once by a plain store (no atomics, no cleared buffer): the same inputs give the
 * same bytes.  Accepted: dtype bf16 / fp16, c a multiple of 8, n, h, w >= 1; anything else is RON_ERR_INVALID with a
 * message, before any HIP call.
 * ---------------------------------------------------------------------------------------- */
int ron_maxpool2x2_backward_nhwc(const float* x, const float* dy, int n, int h, int w, int c, int dtype, float* dx, void* stream);

/* ------------------------------------------------------------------------------------------
 * Backward of the two 2x2 stride-2 operators of the reverse connections: the strided convolution (block7_reverse_conv_left,
 * nets/ron_vgg_320.py:420) with d->transpose = 0 and the transposed convolution (the _deconv_right of the reverse connections,
 * nets/ron_vgg_320.py:424) with d->transpose = 1.  `d` is read as ron_conv2d_nhwc reads it - n, h, w are the dimensions of
 * the input x - with kh = kw = stride = 2 and dilation = 1:
 *   transpose = 0: x [n,h,w,cin], w and dw HWIO [2,2,cin,cout], y and dy [n,h/2,w/2,cout]; h and w even, cin a multiple of
 *                  64, any cout >= 1
 *   transpose = 1: x [n,h,w,cin], w and dw [2,2,cout,cin] (the forward's layout), y and dy [n,2h,2w,cout]; cin and cout
 *                  multiples of 64
 * Everything else is the contract of ron_conv2d_backward_nhwc: all pointers are DEVICE fp32, w included; operands are
 * rounded to d->dtype (bf16 or fp16) and accumulated in fp32; dz = round(dy * (y > 0)) when d->relu (y is this operator's own
 * output, so a branch of a reverse connection passes its own activation: see DESIGN.md 4.8), else round(dy); dx
 * [n,h,w,cin] is delivered as storage-type values in fp32; dw and dbias [cout] are unrounded fp32 sums in a fixed order (the
 * bias gradient of the transposed convolution adds its four taps in tap order); the same inputs give the same bytes.  dx,
 * dw, dbias may each be NULL; every element of a non-NULL output is written; x may be NULL when dw is, w when dx is.  The
 * call enqueues on `stream`, allocates nothing, never synchronises, honours the dry-run mode and assumes nothing about the
 * workspace's contents.  x, y and dy must be 16-byte aligned, the workspace 256-byte aligned.  pool, center_from,
 * in_cstride, in_coff = 0 and tile_cfg = -1; d->splitk is the pixel split of the weight gradient (-1 = by shape, 1 = off,
 * S = forced, capped as in ron_conv2d_backward_nhwc).  Anything else - a NULL y with relu set, a misaligned pointer, a
 * workspace that is too small, a packed tensor that would reach 2 GiB - is RON_ERR_INVALID with a message, before any HIP
 * call.  ron_conv2d_k2s2_backward_workspace_bytes is host arithmetic only; -1 + ron_last_error() on a refused descriptor.
 * ---------------------------------------------------------------------------------------- */
int64_t ron_conv2d_k2s2_backward_workspace_bytes(const ron_conv_desc* d);
int ron_conv2d_k2s2_backward_nhwc(const ron_conv_desc* d, const float* x, const float* w, const float* y, const float* dy,
                                  float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The SSD-only operators between pool1 and the SSD heads: pool5 (3x3 stride-1 max-pool), the block4 L2 normalisation and
 * the padded 3x3 convolutions of the extra blocks.  Each has a forward test operator where the library had none (they
 * allocate and synchronise, like ron_maxpool2x2_nhwc) and a backward that is a real entry point like the convolution
 * backward: it enqueues on `stream`, allocates nothing, never synchronises, honours the dry-run mode, assumes nothing about
 * the workspace's contents, writes every element of every non-NULL output by a plain store and uses no float atomics: the
 * same inputs give the same bytes.
 *
 * --- pool5: slim.max_pool2d [3, 3] stride 1 SAME (nets/ssd_vgg_300.py:472, nets/ssd_vgg_512.py:399) ---
 * ron_maxpool3x3s1_nhwc (test operator) runs the graph's own kernel on x [n,h,w,c] -> y [n,h,w,c], device fp32.  ONE
 * restriction: that kernel starts its maximum at 0 (its zero halo takes part), so it equals TensorFlow's pool for
 * NON-NEGATIVE inputs only - what pool5 sees behind conv5_3's ReLU.  c a multiple of 8 (bf16 / fp16).
 *
 * ron_maxpool3x3s1_backward_nhwc: x (the pool's input), dy and dx are [n,h,w,c] device fp32, 16-byte aligned; no workspace.
 *   xs = round(x) to `dtype`.  The window of output (oy, ox) holds the IN-BOUNDS positions of rows oy-1 .. oy+1 and columns
 *   ox-1 .. ox+1: padding does not take part - it is excluded, not a zero (so the backward is right for negative inputs
 *   too).  A window's gradient goes to the FIRST of its positions, in row-major order, whose xs equals the window's
 *   maximum: the running maximum starts at the window's first in-bounds position and a later position takes over only
 *   when it is greater (>), compared on the rounded values; ties after rounding are ties, and so are -0.0 and +0.0.
 *   dx[n,i,j,ch] = the fp32 sum of round(dy[n,oy,ox,ch]) over the up to nine windows that contain (i, j) and select it,
 *   added in row-major order of (oy, ox) starting from 0.f, rounded ONCE to the storage type and delivered as a
 *   storage-type value in fp32; a position no window selects gets 0.  A window that holds a NaN is outside the contract.
 *   This is torch-CPU's max_pool2d(3, 1, 1) backward in both memory formats and TensorFlow's MaxPoolGrad by the argument
 *   of the 2x2 pool above (parity with TensorFlow unpinned, as there).  The rule holds no multiplication: the result is
 *   reproducible bit for bit in numpy float32.
 *   Accepted: dtype bf16 / fp16, c a multiple of 8, n, h, w >= 1 with n h w c elements inside 64-bit indexing, 16-byte
 *   aligned non-NULL pointers; anything else is RON_ERR_INVALID with a message, before any HIP call.
 *
 * --- block4: custom_layers.l2_normalization(scaling=True) (nets/custom_layers.py:66-135, nets/ssd_vgg_300.py:413) ---
 * gamma is the variable .../L2Normalization/gamma: a DEVICE fp32 vector [c], never rounded.  Per pixel p, over channels:
 *   xs = round(x);  ss = sum_c xs^2 (fp32);  inv = 1 / sqrt(max(ss, 1e-12f));  y = round(xs * inv * gamma[c])
 * ron_l2norm_nhwc (test operator) runs the graph's kernel on x [n,h,w,c] -> y [n,h,w,c], device fp32.
 *
 * ron_l2norm_backward_nhwc: x, dy, dx [n,h,w,c]; gamma, dgamma [c]; all device fp32.  dx and dgamma may each be NULL.
 *   dz = round(dy) (there is no activation behind the normalisation);  u = xs * inv;  g = dz * gamma;  t = sum_c g u
 *   ss >= 1e-12f:  dx = round(inv * (g - u t))
 *   otherwise:     dx = round(inv * g)      the clamped branch: TF's maximum hands no gradient to ss there, so an all-zero
 *                                           post-ReLU pixel gets dy * gamma * 1e6
 *   dgamma[c] = sum_p dz[p,c] u[p,c]: an fp32 sum, not rounded further
 *   ss and t are fp32 sums in an order that is a function of the shape alone (a lane's channels in order, then a butterfly
 *   over the 64 lanes); so is dgamma: wave v of W = min(n h w, 2048) adds its pixels v, v + W, ... in that order into row
 *   v of a [W][c] table in the workspace, a second kernel adds eight contiguous runs of rows, each in row order, and then
 *   the runs in run order.  W does not depend on the device.
 *   Accepted: dtype bf16 / fp16, c a multiple of 8 and at most 2048 (a wave keeps its pixel in registers), n, h, w >= 1 with
 *   n h w c inside 64-bit indexing (the table has at most 2048 rows whatever the shape: it imposes no further limit),
 *   16-byte aligned tensors, x, gamma and dy non-NULL, a 256-byte aligned workspace of at least
 *   ron_l2norm_backward_workspace_bytes(...) bytes (host arithmetic only; -1 + ron_last_error() on a refused shape).
 *   Anything else is RON_ERR_INVALID with a message, before any HIP call.
 *
 * --- the 3x3 convolutions of the extra blocks ---
 * ron_conv2d_padded_backward_nhwc: `d` is read as everywhere - n, h, w are the dimensions of the input x - with
 * kh = kw = 3 and dilation = 1, and (d->stride, cpad) one of
 *   (2, 1)  custom_layers.pad2d(pad=(1, 1)) + 3x3 stride-2 VALID: block8 / block9 of SSD-300 (nets/ssd_vgg_300.py:488-495),
 *           block8 .. block11 of SSD-512 (nets/ssd_vgg_512.py:413-432)
 *   (1, 0)  plain 3x3 VALID, h, w >= 3: block10 / block11 of SSD-300 (nets/ssd_vgg_300.py:500, 505)
 * With ho = (h + 2 cpad - 3) / stride + 1 (wo likewise), y and dy are [n,ho,wo,cout]; x and dx [n,h,w,cin]; w and dw HWIO
 * [3,3,cin,cout]; dbias [cout].  Both forms are the stride-1 SAME convolution sampled at (o + stride oy, o + stride ox),
 * o = 1 - cpad, so their gradients are those of ron_conv2d_backward_nhwc for dz = round(dy * (y > 0)) (round(dy) without
 * relu; y is this operator's own [n,ho,wo,cout] output) scattered to those positions of a zero [n,h,w,cout] map: the same
 * sums with zero terms added.  Everything else - masks, roundings, NULL outputs, splitk, alignment, the 2 GiB caps of the
 * packed FULL-RESOLUTION tensors, the refusals - is the contract of ron_conv2d_backward_nhwc word for word.  At stride 2
 * this spends four times the MFMA work of a strided gather (on maps of 32 x 32 and smaller).
 * Block12 of SSD-512 (pad2d(1) + 4x4 VALID on a 2x2 map, nets/ssd_vgg_512.py:437-438) needs no entry point: only the
 * filter's inner 2x2 taps meet data, so it is ron_conv2d_k2s2_backward_nhwc with w[1:3, 1:3], and dw is zero in the twelve
 * outer taps.
 * ron_conv2d_padded_backward_workspace_bytes is host arithmetic only; -1 + ron_last_error() on what the call would refuse.
 * ---------------------------------------------------------------------------------------- */
int ron_maxpool3x3s1_nhwc(const float* x, int n, int h, int w, int c, int dtype, float* y, void* stream);
int ron_maxpool3x3s1_backward_nhwc(const float* x, const float* dy, int n, int h, int w, int c, int dtype, float* dx, void* stream);
int ron_l2norm_nhwc(const float* x, const float* gamma, int n, int h, int w, int c, int dtype, float* y, void* stream);
int64_t ron_l2norm_backward_workspace_bytes(int n, int h, int w, int c, int dtype);
int ron_l2norm_backward_nhwc(const float* x, const float* gamma, const float* dy, int n, int h, int w, int c, int dtype, float* dx,
                             float* dgamma, void* workspace, int64_t workspace_bytes, void* stream);
int64_t ron_conv2d_padded_backward_workspace_bytes(const ron_conv_desc* d, int cpad);
int ron_conv2d_padded_backward_nhwc(const ron_conv_desc* d, int cpad, const float* x, const float* w, const float* y, const float* dy,
                                    float* dx, float* dw, float* dbias, void* workspace, int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode batch normalisation (slim.batch_norm under ron_arg_scope(is_training=True), nets/ron_vgg_320.py:616-624:
 * fused=True, decay=0.997, epsilon=1e-5, scale=True; every _conv_left and _objectness, reg_bbox/Conv2d_0_3x3 and the two
 * inception concatenations of pred_cls_module), forward and backward.  Real entry points like the convolution backward: they
 * enqueue on `stream`, allocate nothing, never synchronise, honour the dry-run mode, assume nothing about the workspace's
 * contents and use no atomics; all sums run in a fixed order that depends only on the descriptor (the launch geometry is a
 * function of the shape alone), so the same inputs give the same bytes.
 *
 * All pointers are DEVICE fp32: x, y, dy, dx [n,h,w,c]; gamma, beta, mean, var, moving_mean, moving_var, dgamma, dbeta [c].
 * With M = n h w and xs = round(x) to d->dtype (bf16 / fp16: a convolution's output as this library stores it):
 *   forward   mean = sum(xs) / M;  var = sum((xs - mean)^2) / M (the BIASED variance: the one that normalises; never formed as
 *             E[x^2] - mean^2);  rstd = 1 / sqrt(var + eps);  y = round(act(gamma (xs - mean) rstd + beta)), delivered as
 *             storage-type values in fp32 as ron_conv2d_nhwc delivers y; act is ReLU when d->relu.  gamma, beta, the statistics
 *             and all arithmetic between the two roundings are fp32.  mean and var are outputs: the backward reads them and
 *             recomputes rstd with the same expression.
 *   moving    in place, both or neither (both NULL skips them): moving_mean = decay moving_mean + (1 - decay) mean and
 *             moving_var = decay moving_var + (1 - decay) var M / max(M - 1, 1): assign_moving_average(zero_debias=False) on the
 *             Bessel-corrected variance FusedBatchNorm returns, regrouped so that decay 0 gives the batch statistic and decay 1
 *             leaves the tensor unchanged bit for bit.
 *   backward  dz = round(dy (y > 0)) when d->relu (y is this operator's own output, read only then), else round(dy);
 *             xhat = (xs - mean) rstd;  dbeta = sum(dz), dgamma = sum(dz xhat): fp32 sums, not rounded further;
 *             dx = round(gamma rstd (dz - dbeta / M - xhat dgamma / M)), storage-type values in fp32: it goes straight into
 *             ron_conv2d_backward_nhwc (relu = 0) as its dy.  dx, dgamma, dbeta may each be NULL; every element of a non-NULL
 *             output is written by a plain store.
 * Accepted: dtype bf16 / fp16, c a multiple of 8, n, h, w >= 1, M <= 2^24 (the count stays exact in fp32), eps >= 0 and
 * finite, 0 <= decay <= 1, relu 0 / 1, every tensor pointer 16-byte aligned, the workspace 256-byte aligned and at least
 * ron_batchnorm_workspace_bytes(d) bytes (host arithmetic; one size serves both directions; -1 + ron_last_error() on a refused
 * descriptor).  Anything else - a NULL y with relu set, moving_mean without moving_var or the other way round - is
 * RON_ERR_INVALID with a message, before any HIP call.
 * ---------------------------------------------------------------------------------------- */
typedef struct {
  int32_t n, h, w, c;
  int32_t dtype; /* RON_DTYPE_BF16 or RON_DTYPE_F16 */
  int32_t relu;
  float eps;
  float decay;   /* of the moving statistics (the backward ignores it beyond the range check) */
} ron_bn_desc;
int64_t ron_batchnorm_workspace_bytes(const ron_bn_desc* d);
int ron_batchnorm_train_nhwc(const ron_bn_desc* d, const float* x, const float* gamma, const float* beta, float* y, float* mean,
                             float* var, float* moving_mean, float* moving_var, void* workspace, int64_t workspace_bytes,
                             void* stream);
int ron_batchnorm_backward_nhwc(const ron_bn_desc* d, const float* x, const float* y, const float* dy, const float* gamma,
                                const float* mean, const float* var, float* dx, float* dgamma, float* dbeta, void* workspace,
                                int64_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The training update: what ron_net.py:354-381 does with the gradients.  ron_optimizer_step applies ONE rule to a whole list
 * of variables - TensorFlow 1.x's dense apply kernels, the ones tf_utils.configure_optimizer instantiates (tf_utils.py:126-171;
 * the drivers' default is momentum, 0.9) - with the gradient of slim's l2_regularizer(weight_decay) folded into the gradient,
 * as optimizer.apply_gradients on tf.losses.get_total_loss() does (ron_arg_scope puts that regulariser on every conv /
 * conv_transpose `weights`, nets/ron_vgg_320.py:604-612).  A real entry point like the convolution backward and the batch
 * normalisation: it enqueues on `stream`, allocates nothing, never synchronises, honours the dry-run mode, assumes nothing
 * about the workspace's contents and uses no atomics; the same inputs give the same bytes.
 *
 * `t` is a HOST array of n entries whose pointers are DEVICE fp32 (var, grad, slot0, slot1: `count` elements each); the
 * pointers may differ from call to call (gradient buffers are the caller's).  The table reaches the kernel by value in the
 * kernel arguments (under 4 KiB per launch): no device-side table, no upload.  A list longer than one table is cut into
 * consecutive launches of the same kernel; the number of launches and the cut are a function of the counts alone.
 *
 * Everything is fp32, ONE rounded operation per arithmetic sign, in exactly the order written; 1 - decay, 1 - beta1 and
 * 1 - beta2 are formed once on the host in fp32; division and square root are the correctly rounded ones:
 *   g' = g + weight_decay * w    when the tensor's weight_decay != 0, else g' = g (the bits of g: nothing is multiplied by 0)
 *   RON_OPT_SGD       w = w - lr * g'
 *   RON_OPT_MOMENTUM  m = momentum * m + g';  w = w - lr * m                                  (slot0 = m; use_nesterov=False)
 *   RON_OPT_RMSPROP   ms = ms + (1 - decay) * (g' * g' - ms);  mom = momentum * mom + (lr * g') / sqrt(ms + epsilon);
 *                     w = w - mom                                                             (slot0 = ms, slot1 = mom)
 *   RON_OPT_ADAM      m = m + (1 - beta1) * (g' - m);  v = v + (1 - beta2) * (g' * g' - v);
 *                     w = w - (lr_t * m) / (sqrt(v) + epsilon)                                (slot0 = m, slot1 = v)
 *                     lr_t = lr * sqrt(1 - beta2^step) / (1 - beta1^step) in double on the host, rounded to fp32 once
 * weight_decay * w is the gradient of l2_regularizer(weight_decay)(w) = weight_decay * sum(w^2) / 2; a caller passes 0 for
 * biases, gamma and beta, as slim does.  The slots are the caller's, initial values included (TensorFlow: zeros; RMSProp's ms
 * ones): the call never initialises them.  Slots the rule does not need are ignored.
 *
 * reg_loss (DEVICE, one float; may be NULL) receives sum over tensors of (0.5f * weight_decay) * sum(w^2) of the weights
 * BEFORE the update - the regularisation part of the reference's total_loss - as an fp32 sum in a fixed order that depends on
 * the counts alone; tensors with weight_decay == 0 contribute nothing and are not read for it.  With reg_loss == NULL the
 * workspace is not touched and no reduction is launched.
 *
 * Accepted: n from 1 to 4096; count >= 1 (at most 2^40, and 2^22 work units per list); every tensor pointer the rule uses
 * non-NULL and 16-byte aligned (the counts are arbitrary: no access touches a byte outside [ptr, ptr + count), so packed
 * tensors may start 16 bytes behind a neighbour's last whole vector); weight_decay >= 0 and finite; learning_rate finite;
 * momentum, decay, beta1, beta2 in [0, 1], beta1 and beta2 below 1 for Adam; epsilon >= 0 and finite; step >= 1 for Adam
 * (ignored otherwise); with reg_loss the workspace 256-byte aligned and at least ron_optimizer_workspace_bytes(t, n) bytes
 * (host arithmetic on the counts; -1 + ron_last_error() when refused).  Refused as well: a var that appears twice in the list,
 * a var that equals its own grad or slot, an unknown rule.  Every refusal is RON_ERR_INVALID with a message of its own, before
 * any HIP call.  ron_optimizer_plan reports, for a list's counts, out[0] the launches of the update kernel, out[1] the work
 * units, out[2] the table entries per launch and out[3] the elements per work unit.
 * ---------------------------------------------------------------------------------------- */
typedef enum { RON_OPT_SGD = 0, RON_OPT_MOMENTUM = 1, RON_OPT_RMSPROP = 2, RON_OPT_ADAM = 3 } ron_opt_rule;
typedef struct {
  int32_t rule;      /* ron_opt_rule */
  float momentum;    /* momentum and rmsprop */
  float decay;       /* rmsprop */
  float beta1, beta2;
  float epsilon;     /* rmsprop and adam */
} ron_opt_cfg;
typedef struct {
  float* var;
  const float* grad;
  float* slot0;
  float* slot1;
  int64_t count;
  float weight_decay;
} ron_opt_tensor;
int ron_optimizer_plan(const ron_opt_tensor* t, int n, int64_t out[4]);
int64_t ron_optimizer_workspace_bytes(const ron_opt_tensor* t, int n);
int ron_optimizer_step(const ron_opt_cfg* cfg, const ron_opt_tensor* t, int n, float learning_rate, int64_t step, float* reg_loss,
                       void* workspace, int64_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* RON_HIP_H_ */
