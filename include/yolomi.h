/* yolomi — C-ABI of the MI355X-native YOLO11 inference path (gfx950 HIP kernels).
 *
 * The reference has no FFI: its hot path is pure Python delegating to Ultralytics
 * (/root/reference/core/model.py:118-133 `YOLO11Model.predict` → `self.model.predict(source, **kwargs)`;
 * /root/reference/core/model.py:253-291 `benchmark`).  This header is the boundary that replaces the
 * Ultralytics engine + ATen/torchvision kernels under that call: the Python facade
 * (`yolo-infer_amd/core/model.py`) binds it with ctypes; a C/C++ host can link it directly.
 *
 * Conventions: every function returns 0 (YM_OK) or a negative YM_E* code and never throws; the message of the
 * last failure on the calling thread is `ym_last_error()`.  The library owns weights, workspace and captured
 * graphs; the caller owns input/output device buffers.  One context per device; a context is not re-entrant;
 * distinct contexts may be used concurrently from different threads or processes.
 */
#ifndef YOLOMI_H
#define YOLOMI_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YM_OK 0
#define YM_EINVAL -1    /* bad argument (shape, pointer, size) */
#define YM_EBLOB -2     /* malformed model blob */
#define YM_EHIP -3      /* HIP runtime error */
#define YM_ENOMEM -4    /* device allocation failed */
#define YM_ESTATE -5    /* call order (e.g. infer before load) */

typedef struct ym_ctx ym_ctx;

/* What the caller expects the context to run (family / scale / task / dtype / max_B / S).  Capacity
 * fields are hints (0 = grow on demand); scale, task and dtype, when non-zero, are checked against every blob
 * ym_load_weights receives (YM_EBLOB on a mismatch) — the reference resolves them from the model name
 * (core/model.py:37-45, 106-107); here the packed plan carries them. */
typedef struct {
  int max_batch;
  int max_h;
  int max_w;
  int scale;  /* 0 = any, else 'n', 's', 'm', 'l' or 'x' */
  int task;   /* 0 = any, YM_TASK_DETECT, YM_TASK_SEGMENT, YM_TASK_POSE */
  int dtype;  /* 0 = any, YM_DTYPE_F16, YM_DTYPE_F32, YM_DTYPE_I8, YM_DTYPE_F8, YM_DTYPE_X3 */
  int reserved[2];
} ym_model_desc;

#define YM_TASK_DETECT 1
#define YM_TASK_SEGMENT 2
#define YM_TASK_POSE 3 /* Detect + keypoint branch; ym_infer rows carry the decoded keypoints (see ym_infer) */
#define YM_DTYPE_F16 1 /* fp16 storage, fp32 MFMA accumulation (throughput plan) */
#define YM_DTYPE_F32 2 /* exact-f32 MFMA (parity plan) */
#define YM_DTYPE_I8 3  /* PTQ int8 (torch.ao qconfig of optimization/quantization/quantizers.py:124-131) */
#define YM_DTYPE_F8 4  /* PTQ fp8 e4m3 (OCP) operands, fp32 accumulation */
#define YM_DTYPE_X3 5  /* fp32 storage, split-fp16 MFMA (x = hi + lo, three f16 MFMAs per K chunk): f16 tolerance plan */

/* An RCCL unique id (ncclUniqueId: 128 opaque bytes). */
typedef struct {
  char internal[128];
} ym_rccl_id;

/* Per-call predict arguments: the Ultralytics predict kwargs that reach the hot path
 * (conf, iou, classes, agnostic_nms, max_det; NMS constants max_nms=30000, max_wh=7680;
 * LoadTensor eps = finfo(input dtype).eps for the /255 rule). */
typedef struct {
  float conf;
  float max_wh;
  double iou;
  int max_det;
  int max_nms;
  int agnostic;
  float in_eps;
  int has_classes;
  uint32_t classes[4]; /* bit c set = keep class c (c < 128) */
  int use_graph;       /* 1: capture/replay a HIP graph per (shape, pointers, args); 0: eager launches */
  int lanes;           /* 1..4 image slices run as concurrent graph branches (0 = 1); conv tile tables are looked
                          up at the slice batch ceil(B / lanes) */
  int counts_after_dets; /* 1: the detection counts are also written, as B int32 words, right after the B x max_det
                            rows of d_dets (d_dets must hold B*max_det*(6+nm) + B floats): a caller that hands in
                            fresh rows per call gets that call's counts with them, and may read them later */
  const float* d_batch_max; /* NULL: LoadTensor's /255 rule reduces over d_input (the whole batch).  Else a device
                               pointer to ONE float, the max over the GLOBAL batch (batch-sharded multi-GPU: every
                               rank's ym_input_max, all-reduced MAX), read by the forward instead of its shard */
  int multi_label;  /* 1: validation mode, Ultralytics non_max_suppression(multi_label=True): every (anchor, class)
                       pair whose score exceeds conf is a candidate (not only the anchor's best class), the max_nms
                       best of them by (score, then lower anchor, then lower class) go through NMS.  Detect plans
                       only (YM_EINVAL for segment plans); a plan with one class takes the single-label path, as
                       upstream's `multi_label &= nc > 1`.  max_nms <= 32768 in this mode.  0: the predict path.
                       Any other value: YM_EINVAL.  (Carved out of reserved[4]: size and offsets are unchanged.) */
  int reserved[3];
} ym_infer_args;

/* Replaces `YOLO(model_path)` construction (core/model.py:100-116): create a context on `device`. */
int ym_create(int device, const ym_model_desc* desc, ym_ctx** out);

/* Load a model blob (plan + BN-folded packed weights, produced by yolomi.plan.pack_model) from host memory.
 * Replaces AutoBackend(fuse=True) weight preparation.  Copies to device; the host blob may be freed after. */
int ym_load_weights(ym_ctx* ctx, const void* blob, size_t bytes);
/* (blob dtypes: f16 and f32 plans, and int8 PTQ plans packed with calibrated quantisation parameters by
 *  yolomi.plan.pack_graph(..., dtype="i8", qparams=...) — the runtime of PostTrainingQuantizer.optimize,
 *  /root/reference/optimization/quantization/quantizers.py:48-91.) */

/* Multi-GPU initialisation (one process per GPU, batch-sharded): replaces the per-process
 * `YOLO(model_path)` load of core/model.py:100-116 on every rank by ONE load on `root` and an RCCL broadcast over
 * xGMI.  `comm` is an ncclComm_t of the RCCL library the process has loaded (e.g. from ym_rccl_comm_init).  On
 * `root` the context must hold weights (ym_load_weights); every other rank's context receives the root's blob and
 * loads it.  Collective: every rank of `comm` calls it.  Synchronous.  Every rank runs the same collectives whatever
 * fails locally (a root without weights, a staging allocation or a load failing on some rank) and all ranks then
 * return the same verdict, so no rank is left waiting inside RCCL. */
int ym_broadcast_weights(ym_ctx* ctx, void* comm, int root, void* stream);
/* The same broadcast with the ranks as `n` contexts of THIS process (SURVEY §4.4's fake backend: N "ranks" on one
 * GPU, the broadcast a device-to-device copy): ctxs[root] holds weights, every other context receives its blob
 * through the same per-rank staging / receive / ym_load_weights / verdict steps as ym_broadcast_weights' ranks.
 * Synchronous on `stream`.  Lets a one-GPU host (and the tests) run the receive path without RCCL. */
int ym_broadcast_weights_local(ym_ctx* const* ctxs, int n, int root, void* stream);
/* Minimal RCCL bootstrap for C hosts without their own communicator: rank 0 creates the id, the host ships the 128
 * bytes to the other ranks (any channel), every rank creates its communicator on `device`. */
int ym_rccl_get_unique_id(ym_rccl_id* id);
int ym_rccl_comm_init(int device, int nranks, const ym_rccl_id* id, int rank, void** comm);
int ym_rccl_comm_destroy(void* comm);

/* Replaces `YOLO11Model.predict(tensor)` (core/model.py:118-133) for tensor sources: asynchronous on `stream`
 * (a hipStream_t, NULL = default).  d_input: B×3×H×W fp32 NCHW device tensor (H, W multiples of 32).
 * d_dets: B×max_det×(6+nm) fp32 [x1,y1,x2,y2,conf,cls,(mask coeffs)], rows ordered by NMS keep order;
 * d_counts: B int32 kept counts.  d_dets / d_counts must be device pointers.  The forward of a (shape, input,
 * counts, args) key is captured once as a HIP graph; a later call with other d_dets rows replays it with its NMS
 * nodes re-pointed (no recapture, no copy), so a caller may hand in fresh output rows every call.
 * nm, the extras per row: 0 (detect), 32 mask coefficients (segment), or, for pose plans, K*ndim rounded up to a
 * multiple of 4 (COCO: 17*3 = 51 -> 52): [x1,y1,x2,y2,conf,cls, kpt_0 .. kpt_{K-1}, 0 pad] with kpt_k = (x, y[, v]) in
 * input pixels (Ultralytics Pose.kpts_decode: x = (raw*2 + grid_x)*stride, v = sigmoid(raw)); not clipped to the
 * image and not masked by visibility — scale_coords and the Keypoints view do that on the host side.
 * K and ndim: ym_kpt_shape. */
int ym_infer(ym_ctx* ctx, const float* d_input, int B, int H, int W, const ym_infer_args* args, float* d_dets,
             int* d_counts, void* stream);

/* LoadTensor statistics of a device batch: *d_max = max over the n fp32 elements of d_input (asynchronous on
 * `stream`).  Each rank of a batch-sharded run computes its shard's max, the ranks all-reduce it (MAX), and pass the
 * result as ym_infer_args.d_batch_max, so the /255 decision is the whole batch's, as in the reference. */
int ym_input_max(ym_ctx* ctx, const float* d_input, size_t n, float* d_max, void* stream);

/* PTQ calibration support (f32 plans only): one eager forward in which op i also writes its pre-activation output
 * to d_raw[i] (device pointer or NULL; fp32 row-major (pixels, channels): conv / depthwise ops their conv output, the
 * attention op its positional depthwise conv pe(v), ConvTranspose2d its (pixels, 4·C) GEMM output).  Feeds the
 * conv-output observers of the reference's PostTrainingQuantizer (optimization/quantization/quantizers.py:146-177).
 * Asynchronous on `stream`. */
int ym_calibrate(ym_ctx* ctx, const float* d_input, int B, int H, int W, const ym_infer_args* args, float* d_dets,
                 int* d_counts, float* const* d_raw, int n_ops, void* stream);

/* Eager run with a HIP event pair around every op: op_ms[i] = device time of op i (n_ops entries). */
int ym_profile(ym_ctx* ctx, const float* d_input, int B, int H, int W, const ym_infer_args* args, float* d_dets,
               int* d_counts, void* stream, float* op_ms, int n_ops);

/* Per-op device time without per-op markers: after one real forward, every conv / depthwise / SPPF / attention op
 * is captured as a graph of `reps` back-to-back launches on the real buffers and timed with one HIP event pair;
 * op_ms[i] = that time / reps (launch gaps included, as in the forward graph).  Ops that are not idempotent
 * (input statistics, decode, NMS) get -1.  Synchronous; leaves the activation buffers in an unspecified state. */
int ym_profile_replay(ym_ctx* ctx, const float* d_input, int B, int H, int W, const ym_infer_args* args,
                      float* d_dets, int* d_counts, void* stream, int reps, float* op_ms, int n_ops);

/* On-device autotuning of the conv tile configuration, per op, for input shape (B, H, W): every candidate is timed
 * as `reps` graph-captured back-to-back launches on this GPU (after one real forward so the buffers hold real
 * activations); the fastest is kept for this shape (one table per (B, H, W)).  Synchronous.  ym_get_op_cfg /
 * ym_set_op_cfg export / import the per-op choices for a shape (n_ops ints, -1 = built-in heuristic) so a tuned plan
 * can be cached and pinned; ym_get_op_cfg returns 1 (and all -1) when the shape has no table. */
int ym_tune(ym_ctx* ctx, const float* d_input, int B, int H, int W, const ym_infer_args* args, float* d_dets,
            int* d_counts, void* stream, int reps);
int ym_get_op_cfg(ym_ctx* ctx, int B, int H, int W, int* cfg, int n_ops);
int ym_set_op_cfg(ym_ctx* ctx, int B, int H, int W, const int* cfg, int n_ops);

/* Introspection for tests / bisecting: op count & names, and the device view of plan buffer `buf` as produced by
 * the last ym_infer/ym_profile (NHWC; elem_bytes 2 = fp16, 4 = fp32; for the anchor buffer H=1, W=A). */
int ym_num_ops(ym_ctx* ctx);
const char* ym_op_name(ym_ctx* ctx, int i);
int ym_num_buffers(ym_ctx* ctx);
int ym_buffer_info(ym_ctx* ctx, int buf, void** ptr, int* C, int* H, int* W, int* elem_bytes);

/* Copy the first `bytes` of plan buffer `buf` (as left by the last ym_infer/ym_profile) to `dst` (host or device
 * pointer); synchronous. */
int ym_read_buffer(ym_ctx* ctx, int buf, void* dst, size_t bytes);

/* Pose plans: keypoints per detection (K) and values per keypoint (ndim: 2 = x, y; 3 = x, y, visibility) of the loaded
 * model; both 0 for detect / segment plans. */
int ym_kpt_shape(ym_ctx* ctx, int* K, int* ndim);

/* Introspection for tests: copy the first `bytes` of a scratch region of the last forward to `dst`; synchronous.
 * YM_SCRATCH_KEYS: the candidate keys, per image `kstride` (the power of two >= A) uint64 words, score bits << 32 |
 * ~anchor, in no fixed order; YM_SCRATCH_COUNTS: the B candidate counts (int32); YM_SCRATCH_KPTS (pose plans): the
 * decoded keypoint rows (B, A, nm) fp32, written for the candidates' anchors only.
 * After a multi-label forward (ym_infer_args.multi_label = 1) YM_SCRATCH_COUNTS holds the per-image (anchor, class)
 * PAIR counts, before the max_nms cut, and YM_SCRATCH_KEYS the unused single-label keys. */
#define YM_SCRATCH_KEYS 0
#define YM_SCRATCH_COUNTS 1
#define YM_SCRATCH_KPTS 2
int ym_read_scratch(ym_ctx* ctx, int which, void* dst, size_t bytes);

/* Segment plans: instance masks of the detections of the last ym_infer (same B, H, W, stream order), i.e. Ultralytics
 * `ops.process_mask(proto, coef, boxes, (H, W), upsample=True)` per image.  d_dets: the ym_infer output rows;
 * d_offsets: B+1 device ints, offsets[b] = first mask of image b, offsets[B] = total (prefix of the kept counts);
 * d_masks: total x H x W bytes (1 = inside the instance); d_nonempty: total ints, 1 when the mask has any pixel
 * set (the predictor drops empty masks).  Asynchronous on `stream`. */
int ym_masks(ym_ctx* ctx, const float* d_dets, int B, int max_det, const int* d_offsets, int total, int H, int W,
             unsigned char* d_masks, int* d_nonempty, void* stream);

/* Segment plans, single-sync form of ym_masks: the masks of the first min(counts[b], cap) detections of every image,
 * taken from the DEVICE counts of the last ym_infer (d_counts, B ints), so the masks are enqueued right behind the
 * forward with no host round trip in between.  d_masks: B x cap x H x W bytes, slot (b, i) = detection i of image b
 * (unused slots are left unwritten); d_flags: B*cap + B ints = the non-empty flag of every slot (0 when unused),
 * then a copy of the B counts, so ONE device->host read of d_flags returns both.  The caller checks counts[b] <= cap
 * (else it calls ym_masks for that batch).  Same arithmetic as ym_masks.  Asynchronous on `stream`. */
int ym_masks_slots(ym_ctx* ctx, const float* d_dets, int B, int max_det, const int* d_counts, int cap, int H, int W,
                   unsigned char* d_masks, int* d_flags, void* stream);

/* Segment plans: native-resolution instance masks of the detections of the last ym_infer (same B, H, W, stream order),
 * i.e. Ultralytics `ops.process_mask_native(proto, coef, boxes, (h0, w0))` per image (predict's retina_masks=True):
 * the whole prototype-resolution mask, its letterbox window (scale_masks) resized bilinearly to the image's native
 * (h0, w0), cropped to the box there, > 0.  d_dets: rows [x1 y1 x2 y2 conf cls coef...] with the box ALREADY in native
 * pixels (scale_boxes), row i of image b at d_dets + (b * max_det + i) * det_stride floats (det_stride >= 6 + nm);
 * d_offsets: B+1 device ints as for ym_masks; shapes / d_shapes: the B x 2 native (h0, w0) on the host (validated here
 * and used to size the launch) and the same values on the device (what the kernel reads: the caller owns the upload,
 * so the call copies nothing and stays asynchronous); d_mask_offsets: B device int64, the first mask byte of image
 * b in d_masks; d_masks: packed bytes, image b's masks back to back, h0_b * w0_b bytes each (1 = inside the instance;
 * no alignment is required); d_nonempty: total ints, 1 when the mask has any pixel set.  YM_ESTATE on a non-segment plan
 * or when it does not follow ym_infer of the same (B, H, W); YM_EINVAL on a null pointer or a native size below 1 (or
 * above 2^30 pixels).  Asynchronous on `stream`. */
int ym_masks_native(ym_ctx* ctx, const float* d_dets, int det_stride, int B, int max_det, const int* d_offsets,
                    int total, int H, int W, const int* shapes, const int* d_shapes, const long long* d_mask_offsets,
                    unsigned char* d_masks, int* d_nonempty, void* stream);

/* Image sources: Ultralytics `LetterBox` + predictor preprocessing of ONE HWC uint8 image already
 * in device memory (d_src, rows row_bytes apart, 3 channels; bgr = 1 for cv2.imread order).  The image is resized to
 * uh x uw with OpenCV's 8-bit INTER_LINEAR fixed-point arithmetic (skipped when the size does not change), placed at
 * (top, left) of an Hn x Wn canvas filled with 114, converted to RGB planes and divided by 255 into d_dst (3 x Hn x Wn
 * fp32: one image of the batch ym_infer reads).  The geometry is the caller's (LetterBox arithmetic, see
 * yolomi/preprocess.py).  Asynchronous on `stream`.  Replaces the reference's cv2-based preprocessing under
 * YOLO11Model.predict(path | ndarray) (/root/reference/core/model.py:118-133, demos/detection_demo.py:87-93). */
int ym_letterbox(ym_ctx* ctx, const void* d_src, int h, int w, int row_bytes, int bgr, int uh, int uw, int top,
                 int left, float* d_dst, int Hn, int Wn, void* stream);

/* Test-time augmentation for detect plans (Ultralytics predict / val with augment=True, DetectionModel._predict_augment):
 * three passes at scales (1, 0.83, 0.67), the middle one mirrored along W, their decoded heads de-scaled, de-flipped,
 * clipped (_clip_augmented: pass 0 loses its last A0 / 21 anchors, pass 2 its first (A2 / 21) * 16) and concatenated in
 * pass order in front of ONE NMS.  A context holds one workspace shape, so the caller keeps one context per pass, all
 * loaded with the same blob, and issues on one stream:
 *   ym_tta_scale(pass 1), ym_tta_scale(pass 2)         the scaled inputs (pass 0 reads d_input itself)
 *   ym_tta_forward(ctx_p, pass p's input) for p = 0..2  the forward up to and including the anchor decode, no NMS
 *   ym_tta_nms(ctx_0, ctx_1, ctx_2, ...)                merge + NMS into d_dets / d_counts, as ym_infer writes them
 * Everything is asynchronous on `stream`; once the three shapes have been seen, a call allocates nothing and captures
 * no graph.
 *
 * ym_tta_shape: pass `pass` (0..2) of an H x W input is Hs x Ws, of which hc x wc = int(H s) x int(W s) is resized
 * content and the rest (right, bottom) pad.
 * ym_tta_scale: d_out (B x 3 x Hs x Ws fp32) = scale_img(flip ? x.flip(3) : x, s, gs = 32) of the NORMALISED batch:
 * LoadTensor's /255 rule (*d_max > 1 + in_eps, d_max = ym_input_max of the batch or the global batch max) is applied to
 * every tap, then torch's bilinear resize (align_corners = False), then the 0.447 pad.  pass is 1 or 2. */
int ym_tta_shape(int H, int W, int pass, int* Hs, int* Ws, int* hc, int* wc);
int ym_tta_scale(ym_ctx* ctx, const float* d_input, int B, int H, int W, int pass, const float* d_max, float in_eps,
                 float* d_out, void* stream);
/* ym_infer without its NMS stage (and without outputs): the context's decode scratch then holds this pass's boxes,
 * scores and classes for ym_tta_nms.  args as for ym_infer; multi_label is ignored here (ym_tta_nms takes it). */
int ym_tta_forward(ym_ctx* ctx, const float* d_input, int B, int H, int W, const ym_infer_args* args, void* stream);
/* Merge and NMS of the three passes' last ym_tta_forward (B images; pass p ran at ym_tta_shape(H, W, p)); H x W is the
 * full-size frame boxes are reported in and clipped to.  d_dets / d_counts and every field of args as for ym_infer
 * (multi_label = 1: the validator's multi-label NMS over the merged set); the merged scratch belongs to ctxs[0].
 * YM_EINVAL unless the three contexts hold the same detect plan. */
int ym_tta_nms(ym_ctx* const* ctxs, int B, int H, int W, const ym_infer_args* args, float* d_dets, int* d_counts,
               void* stream);
/* Introspection for tests: the B candidate counts of the last ym_tta_nms of `ctx` (merged anchors above conf, or the
 * (anchor, class) pairs before the max_nms cut after a multi-label call); synchronous. */
int ym_tta_counts(ym_ctx* ctx, int* dst, int B);

/* Feature embeddings (Ultralytics predict(source, embed=[layers]) / model.embed(source), BaseModel._predict_once's
 * embed branch): per image, the global average pool (adaptive_avg_pool2d(x, (1, 1))) of the named layers' outputs,
 * concatenated.  A layer's output is one or more channel views of plan buffers (yolomi.arch.GraphBuilder.layer_views:
 * a Concat layer is its inputs' views, an Upsample layer its source's), so the caller passes a view table; view i's C
 * means land in columns [sum of the earlier views' C, + C) of row b of d_out.
 * The forward (d_input, B, H, W, stream as for ym_infer; of args only in_eps, d_batch_max and use_graph are read) runs
 * up to and including the last op that stores a named buffer, then the pooling stage (csrc/ym_embed.hip) — nothing
 * else: no later op, no decode, no NMS, no detection rows or counts; it is captured and replayed like ym_infer's.
 * d_out: B rows of out_stride floats (out_stride >= the views' total C).  The mean is an fp32 tree sum over the pixels
 * (fixed order: results are bit-identical from call to call, eager or replayed) divided once by H_i * W_i.
 * YM_ESTATE before ym_load_weights.  YM_EINVAL: a null pointer; n_views outside 1..32; a view that names the input,
 * the anchor rows or no buffer, leaves its buffer, is not made of whole 8-channel groups, or whose buffer no op of
 * this plan stores (a conv fused into its successor); out_stride below the total C; an int8 / fp8 plan (their stored
 * codes would need each buffer's scale and zero point).  Asynchronous on `stream`. */
typedef struct {
  int buf;  /* plan buffer (ym_buffer_info ids) */
  int coff; /* first channel, a multiple of 8 */
  int C;    /* channels, a multiple of 8 */
  int reserved; /* 0 */
} ym_embed_view;
int ym_embed(ym_ctx* ctx, const float* d_input, int B, int H, int W, const ym_infer_args* args,
             const ym_embed_view* views, int n_views, float* d_out, long long out_stride, void* stream);

/* Object tracking (Ultralytics model.track(..., tracker="bytetrack.yaml"), trackers/byte_tracker.py BYTETracker.update):
 * a tracker holds the ByteTrack state of `streams` independent video streams in device memory; one ym_track_update
 * call advances stream b by the detections of image b of a batch, as ONE kernel launch behind the NMS
 * (csrc/ym_track.hip: fp64 XYAH Kalman filter, fp32 IoU, an optimal (not greedy) assignment), with no
 * host synchronisation.  Track ids count from 1 per stream.
 * ym_track_cfg: bytetrack.yaml's parameters; max_time_lost = track_buffer frames (frame rate 30).  capacity: track
 * slots per stream (tracked + lost + unconfirmed), 0 = YM_TRACK_CAPACITY; when every slot is taken, further
 * detections start no track and the stream's drop counter goes up.
 * ym_track_create: YM_EINVAL for a null pointer, streams outside 1..YM_TRACK_MAX_STREAMS, a threshold outside [0, 1],
 * track_buffer < 0 or capacity outside 0..YM_TRACK_CAPACITY.  The tracker lives on ctx's device and starts reset.
 * ym_track_reset: every stream back to frame 0, no tracks, next id 1, drops 0 (asynchronous on `stream`).
 * ym_track_update: d_dets = B x max_det rows of det_stride floats [x1,y1,x2,y2,conf,cls,extras] with d_counts[b] valid
 * rows per image (what ym_infer wrote; det_stride = 6 + nm).  d_tracks: B x max_det rows of det_stride + 1 floats
 * [x1,y1,x2,y2 (the filter's box), id, conf, cls, extras of the detection that fed the track]; d_idx: B x max_det
 * int32, that detection's row; d_track_counts: B int32 rows written per image.  Rows are in ascending id order; only
 * activated tracks matched in this frame appear.  An image whose count is 0 leaves its stream untouched (no frame is
 * counted) and writes count 0.  YM_EINVAL: a null pointer, B != streams, max_det outside 1..YM_TRACK_MAX_DET,
 * det_stride outside 6..YM_TRACK_MAX_STRIDE.  Asynchronous on `stream`; calls of one tracker must be stream-ordered.
 * ym_track_read_state: per stream YM_TRACK_STATE_WORDS ints [frame_id, next id, activated tracked tracks, lost
 * tracks, unconfirmed tracks, drops] after the last update, n_streams <= streams of them; synchronous. */
#define YM_TRACK_CAPACITY 512
#define YM_TRACK_MAX_DET 300
#define YM_TRACK_MAX_STRIDE 64
#define YM_TRACK_MAX_STREAMS 1024
#define YM_TRACK_STATE_WORDS 6
typedef struct ym_tracker ym_tracker;
typedef struct {
  double track_high_thresh; /* 0.25 */
  double track_low_thresh;  /* 0.1 */
  double new_track_thresh;  /* 0.25 */
  double match_thresh;      /* 0.8 */
  int track_buffer;         /* 30 */
  int fuse_score;           /* 1 */
  int capacity;             /* 0 = YM_TRACK_CAPACITY */
  int reserved;             /* 0 */
} ym_track_cfg;
int ym_track_create(ym_ctx* ctx, int streams, const ym_track_cfg* cfg, ym_tracker** out);
void ym_track_destroy(ym_tracker* trk);
int ym_track_reset(ym_tracker* trk, void* stream);
int ym_track_update(ym_tracker* trk, const float* d_dets, int det_stride, int B, int max_det, const int* d_counts,
                    float* d_tracks, int* d_idx, int* d_track_counts, void* stream);
int ym_track_read_state(ym_tracker* trk, int* state, int n_streams);

/* Annotated frames (Ultralytics Results.plot(): boxes, labels, masks, keypoints, skeletons, track ids), composited per
 * pixel on the device by two launches (csrc/ym_annot.hip; the drawing rules are this project's own, exact and integer:
 * DESIGN.md §17, csrc/ym_annot.h).  Works on any context, loaded or not: it reads rows, not activations.
 * d_frames: the B canvases, B x 3 x H x W fp32 (frames_are_f32_chw = 1: converted as trunc(clamp(x * 255, 0, 255)), no
 * channel flip) or B x H x W x 3 bytes; d_dets: B x max_det rows of args->det_stride floats, [x1 y1 x2 y2 conf cls
 * extras] or with args->tracked [x1 y1 x2 y2 id conf cls extras], the first d_counts[b] of image b valid (device counts:
 * no host value is needed); with args->K > 0 the first K * ndim extras are keypoints (x, y[, visibility]).
 * d_masks (may be null): packed mask planes of mask_h x mask_w bytes (non-zero = inside), instance i of image b at
 * d_masks + d_mask_offsets[b] + i * mask_h * mask_w for i < args->mask_cap (0: max_det); d_mask_geo (may be null: the
 * identity (H, W, 0, 0)): B x (uh, uw, top, left) int32, the window of the mask plane the canvas maps to.
 * d_names: args->nc x 24 bytes, class names (0-terminated when shorter); args->d_font: 95 glyphs x 11 row bytes
 * (yolomi/font6x11.py), column gx of a row in bit 5 - gx.  d_out: B x H x W x 3 bytes.
 * YM_EINVAL: a null pointer (frames, rows, counts, args, font, output; names with nc > 0; offsets with masks), B outside
 * 1..65535, a side outside 1..YM_ANNOT_MAX_SIDE, line_width outside 1..255, kpt_radius outside 0..255, K outside 0..32,
 * ndim not 2 | 3, det_stride below 6 + tracked + K * ndim, an unknown color_mode or switch bit.  Asynchronous on
 * `stream`.  The records of a call live in ONE scratch buffer per context: calls on the same context must be
 * stream-ordered (one stream, or the caller's own events between streams) — two calls in flight on different streams
 * would overwrite each other's records; contexts are independent, so concurrent streams take a context each.  The
 * scratch grows when B * max_det does, with hipDeviceSynchronize + hipFree + hipMalloc: a call that grows it must not
 * be made while a stream is capturing (make one call of the largest B * max_det first; later calls allocate nothing). */
#define YM_ANNOT_MAX_SIDE 8192
#define YM_ANNOT_BOXES 1     /* flags: off hides outline and label */
#define YM_ANNOT_LABELS 2    /* off hides the label */
#define YM_ANNOT_CONF 4      /* off drops the confidence from the label text */
#define YM_ANNOT_MASKS 8     /* off skips the mask blend */
#define YM_ANNOT_KPT_LINE 16 /* off hides the limbs */
#define YM_ANNOT_CLIP_KPTS 32 /* on: keypoints are clipped to [0, W] x [0, H] first, as predict()'s Results hold them */
#define YM_ANNOT_COLOR_CLASS 0
#define YM_ANNOT_COLOR_INSTANCE 1 /* by track id when tracked, else by row index */
typedef struct {
  int line_width; /* >= 1 (the caller applies upstream's default rule) */
  int kpt_radius; /* 5 */
  int flags;      /* YM_ANNOT_* switches */
  int color_mode; /* YM_ANNOT_COLOR_* */
  int tracked;    /* rows carry the id column */
  int det_stride; /* floats per row */
  int K, ndim;    /* keypoints per row (0: none), values per keypoint */
  int nc;         /* rows of d_names */
  int mask_cap;   /* mask planes per image (0: max_det) */
  const void* d_font;
  int reserved[2]; /* 0 */
} ym_annotate_args;
int ym_annotate(ym_ctx* ctx, const void* d_frames, int frames_are_f32_chw, int B, int H, int W, const float* d_dets,
                int max_det, const int* d_counts, const unsigned char* d_masks, const long long* d_mask_offsets,
                int mask_h, int mask_w, const int* d_mask_geo, const unsigned char* d_names, const ym_annotate_args* args,
                unsigned char* d_out, void* stream);

/* Instance polygons (Ultralytics Masks.xy: masks2segments' cv2.findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE) and
 * strategy "largest"), traced on the device (csrc/ym_contour.hip; the definition is this project's own):
 * per plane, the outer border of one top-level 8-connected component — the one with the most points after
 * compression, a tie going to the one that starts last in raster order — as (x, y) int32 pixel coordinates.  Works on
 * any context, loaded or not: it reads planes, not activations.
 * d_masks: n planes of H x W bytes (non-zero = inside), plane i at d_masks + i * plane_stride; the output of ym_masks,
 * ym_masks_slots, ym_masks_native or any other byte tensor, box-cropped or not.  d_offsets: n + 1 int64 words,
 * offsets[i] = the first point of plane i, offsets[n] = the points of all planes (a plane without foreground has
 * none).  d_points: cap_points x 2 int32, plane i's points at d_points + 2 * offsets[i], back to back, for every plane
 * with offsets[i + 1] <= cap_points; the points of the other planes are not written, so a caller that reads
 * offsets[n] > cap_points calls again with that capacity (d_points may be null with cap_points 0: a count-only call).
 * Reading a result is two device->host copies: the offsets, then offsets[n] points.
 * YM_EINVAL: a null pointer, n < 0, H or W below 1 (or H * W above 2^27), plane_stride < H * W, cap_points < 0; n = 0
 * is valid and writes offsets[0] = 0.  Asynchronous on `stream`.  Scratch: 16 bytes per plane, and for planes of more
 * than about 480k pixels (whose bit plane does not fit LDS) (H + 2) * (ceil(W / 32) + 2) * 4 bytes per plane more; ONE
 * buffer per context, grown like ym_annotate's (same rules: stream-ordered calls, no growth while capturing). */
int ym_mask_contours(ym_ctx* ctx, const unsigned char* d_masks, int n, int H, int W, long long plane_stride,
                     int* d_points, long long cap_points, long long* d_offsets, void* stream);

int ym_sync(ym_ctx* ctx);
const char* ym_last_error(void);
void ym_destroy(ym_ctx* ctx);
int ym_version(void);
/* Size of the conv tile-configuration catalogue of a plan dtype (ym_model_desc codes: 1 f16, 2 f32, 3 i8, 4 f8, 5 x3;
 * YM_EINVAL otherwise): the id space of the ym_get_op_cfg / ym_set_op_cfg tables, so a cached table is reused only
 * by a library with the same catalogue. */
int ym_num_conv_cfgs(int dtype);
/* Tests: whether the pinned configuration of each op (ym_set_op_cfg, ym_tune) was the kernel that ran in the last
 * forward this context launched eagerly or captured, which must have been a B x H x W one (else YM_ESTATE).
 * out: 2 * ym_num_ops ints.  out[2i]: 1 the kernel of op i's id ran, 0 the launcher fell back (the heuristic tile, the
 * first variant that takes the shape, or a fused pair's two convs), -1 op i is not a conv, is the stem, has no id
 * pinned, was not launched, or the plan is int8 / fp8 (not tracked).  For a fused pair whose id is a two-launch one
 * out[2i] and out[2i + 1] are those values of its first and second conv; out[2i + 1] is -1 otherwise. */
int ym_get_op_cfg_taken(ym_ctx* ctx, int B, int H, int W, int* out, int n);
/* Tests: which kernel instantiation the depthwise, SPPF and attention ops of that same last forward launched (set on
 * the host next to the launch actually issued; ym_get_op_cfg_taken and its values are untouched by it).  out:
 * ym_num_ops ints, -1 for every other op kind, an op not launched, and every op of an int8 / fp8 plan.  The storage
 * type (f16 / f32 / x3 pairs) is the plan's and not part of the code.
 *   YM_OP_DWCONV   0 dwconv3x3 (one pixel per thread), 1 dwconv3x3_row PXT 2, 2 dwconv3x3_row PXT 4 (f16 only),
 *                  3 dwconv3x3_strip PXT 2 RT 2, 4 dwconv3x3_strip PXT 4 RT 4,
 *                  5..8 dwconv3x3_lds tile 0..3 (8x16x4, 4x32x4, 8x32x2, 16x16x2: YM_DBG_DW_TILE)
 *   YM_OP_SPPF     0 sppf_pool separable (row then column maxima in LDS), 1 sppf_pool direct 2-D windows
 *   YM_OP_ATTN     0..3 attn_psa QB 4 / 8 / 16 / 32, 4..7 attn_psa_mfma NKT 8 / 16 / 26 / 32,
 *                  8..11 attn_psa_x3 NKT 8 / 16 / 26 / 32 (either KB: YM_DBG_ATTN_KB does not change the code),
 *                  12 attn_psa_flash<false> (f16), 13 attn_psa_flash<true> (x3)
 * ym_op_variant_count(kind): the number of distinct codes of an op kind (9, 2, 14), YM_EINVAL for another kind. */
#define YM_OP_DWCONV 1
#define YM_OP_SPPF 2
#define YM_OP_ATTN 3
#define YM_DWV_PIXEL 0
#define YM_DWV_ROW2 1
#define YM_DWV_ROW4 2
#define YM_DWV_STRIP2 3
#define YM_DWV_STRIP4 4
#define YM_DWV_LDS0 5
#define YM_DWV_COUNT 9
#define YM_SPPFV_SEP 0
#define YM_SPPFV_DIRECT 1
#define YM_SPPFV_COUNT 2
#define YM_ATTNV_SCALAR_QB4 0
#define YM_ATTNV_MFMA_NKT8 4
#define YM_ATTNV_X3_NKT8 8
#define YM_ATTNV_FLASH_F16 12
#define YM_ATTNV_FLASH_X3 13
#define YM_ATTNV_COUNT 14
int ym_get_op_variant(ym_ctx* ctx, int B, int H, int W, int* out, int n);
int ym_op_variant_count(int kind);

/* Process-wide debug switches for tests and A/B runs (not part of the reference interface; defaults 0), read when a
 * kernel is launched (so at graph capture for replayed forwards): YM_DBG_NMS (9 = the NMS kernel's per-box path
 * instead of the blocked one), YM_DBG_DW_MODE (depthwise variant: 0 LDS tiles, 1 rows, 2 column strips),
 * YM_DBG_DW_TILE (LDS tile shape 0..3), YM_DBG_CHAIN (1: the persistent two-conv chain kernel).
 * The environment variables YM_NMS_DBG, YM_DW_MODE, YM_DW_TILE, YM_CHAIN, YM_STEMFUSE, YM_ATTN_KB, YM_PAIRST and
 * YM_CONV_CFG (the last two: the value itself, stored + 1) set the initial values.  A forward graph
 * already captured keeps the kernels it was captured with.
 * Returns the previous value, or YM_EINVAL for an unknown key. */
#define YM_DBG_NMS 1
#define YM_DBG_DW_MODE 2
#define YM_DBG_DW_TILE 3
#define YM_DBG_CHAIN 4 /* 1: dependent x3 3x3 pairs on one LDS-DMA configuration as one persistent launch */
#define YM_DBG_CHAIN_LAUNCHES 5 /* chain kernels launched since it was last set (a counter) */
#define YM_DBG_STEMFUSE 6 /* 1: x3 stem + model.1 + model.2.cv1 as one launch (csrc/ym_stem_fused.hip); 0: three */
#define YM_DBG_ATTN_KB 7 /* 1: x3 attention loads K fragments 8 key tiles per round trip; 0: all tiles at once */
#define YM_DBG_PAIRST 8 /* x3 lane-pair epilogue store family mask + 1 (0: the default mask 21) */
#define YM_DBG_CONV_CFG 9 /* a forced conv tile configuration id + 1 for untuned ops (0: the heuristic) */
/* tests: 1 + the index of the last op an eager forward launches (0: a whole forward).  Every op of a stopped forward is
 * its own launch and no decode / NMS output is written, so a test can read a view that a later op overwrites.  Eager
 * only: while it is set, a call with args->use_graph returns YM_EINVAL (a stopped forward is never captured). */
#define YM_DBG_STOP 10
int ym_set_debug(int key, int value);

#ifdef __cplusplus
}
#endif
#endif /* YOLOMI_H */
