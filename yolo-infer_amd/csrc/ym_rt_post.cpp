// yolomi runtime, the stages beside a forward: letterbox and classify preprocessing in front of it; the mask stages, the
// annotator, contours and run-length encoding behind it.  None launches a plan op: each takes a context for its device,
// the prototypes its last forward left (the mask stages) or a scratch buffer of its own that grows on demand.
#include <algorithm>
#include <cstdlib>
#include "ym_runtime.h"
#include "ym_annot.h"
#include "ym_contour.h"
#include "ym_rle.h"

// The mask stages run behind a forward of the same (B, H, W), whose workspace still holds the prototypes: check that
// and point `a` (MaskArgs, MaskNativeArgs) at them.  `who` names the entry point in the message.
template <typename Args> static int mask_protos(ym_ctx* c, const char* who, int B, int H, int W, Args& a) {
  if (!c->d_arena || B > c->cB || H != c->cH || W != c->cW)
    return fail(YM_ESTATE, "%s must follow ym_infer of the same (B, H, W) (workspace %dx%dx%d)", who, c->cB, c->cH,
                c->cW);
  a.proto = reinterpret_cast<const float*>(c->bptr(c->proto_buf, 0));
  a.MH = c->buf_H(c->proto_buf); a.MW = c->buf_Wd(c->proto_buf); a.nm = c->nm;
  return YM_OK;
}

extern "C" {

int ym_letterbox(ym_ctx* c, const void* d_src, int h, int w, int row_bytes, int bgr, int uh, int uw, int top,
                 int left, float* d_dst, int Hn, int Wn, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_src || !d_dst || h < 1 || w < 1 || uh < 1 || uw < 1 || top < 0 || left < 0 || top + uh > Hn ||
      left + uw > Wn || row_bytes < 3 * w)
    return fail(YM_EINVAL, "bad ym_letterbox geometry (%dx%d -> %dx%d at (%d, %d) in %dx%d)", h, w, uh, uw, top, left,
                Hn, Wn);
  HIPCK(hipSetDevice(c->device));
  LetterboxArgs a{};
  a.src = static_cast<const unsigned char*>(d_src);
  a.h = h; a.w = w; a.row_bytes = row_bytes; a.bgr = bgr ? 1 : 0;
  a.uh = uh; a.uw = uw; a.top = top; a.left = left;
  a.scale_x = 1.0 / ((double)uw / w);  // cv2: scale_x = 1. / inv_scale_x, inv_scale_x = (double)dsize.width / ssize.width
  a.scale_y = 1.0 / ((double)uh / h);
  a.dst = d_dst; a.Hn = Hn; a.Wn = Wn;
  return launched(ym_launch_letterbox(a, static_cast<hipStream_t>(stream)), "letterbox launch");
}

int ym_letterbox_batch(ym_ctx* c, const ym_letterbox_desc* d_desc, const ym_letterbox_desc* h_desc, int B,
                       float* d_dst, int Hn, int Wn, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_desc || !h_desc || !d_dst) return fail(YM_EINVAL, "ym_letterbox_batch: null pointer");
  if (B < 1 || B > 65535) return fail(YM_EINVAL, "ym_letterbox_batch: B %d outside 1..65535", B);
  if (Hn < 1 || Wn < 4 || Wn % 4) return fail(YM_EINVAL, "ym_letterbox_batch: bad canvas %dx%d (Wn: a multiple of 4)", Hn, Wn);
  if (reinterpret_cast<uintptr_t>(d_dst) & 15) return fail(YM_EINVAL, "ym_letterbox_batch: d_dst not 16-byte aligned");
  for (int b = 0; b < B; ++b) {
    const ym_letterbox_desc& d = h_desc[b];
    if (!d.src || d.h < 1 || d.w < 1 || d.uh < 1 || d.uw < 1 || d.top < 0 || d.left < 0 ||
        (long long)d.top + d.uh > Hn || (long long)d.left + d.uw > Wn || d.row_bytes < 3 * (long long)d.w ||
        (d.bgr != 0 && d.bgr != 1))
      return fail(YM_EINVAL, "ym_letterbox_batch: frame %d: bad geometry (%dx%d, rows %d bytes -> %dx%d at (%d, %d) in "
                  "%dx%d, bgr %d)", b, d.h, d.w, d.row_bytes, d.uh, d.uw, d.top, d.left, Hn, Wn, d.bgr);
    if (d.scale_x != 1.0 / ((double)d.uw / d.w) || d.scale_y != 1.0 / ((double)d.uh / d.h))
      return fail(YM_EINVAL, "ym_letterbox_batch: frame %d: scales (%.17g, %.17g) are not 1 / (uw / w), 1 / (uh / h)", b,
                  d.scale_x, d.scale_y);
  }
  HIPCK(hipSetDevice(c->device));
  LetterboxBatchArgs a{};
  a.desc = d_desc; a.dst = d_dst; a.B = B; a.Hn = Hn; a.Wn = Wn;
  return launched(ym_launch_letterbox_batch(a, static_cast<hipStream_t>(stream)), "letterbox_batch launch");
}

// coef[6] of the NV12 entries → the kernels' Nv12Coef, refused when a converted channel's sum could leave int32
static int nv12_coef(const char* who, const int* coef, Nv12Coef& k) {
  if (!coef) return fail(YM_EINVAL, "%s: null coef", who);
  k = Nv12Coef{coef[0], coef[1], coef[2], coef[3], coef[4], coef[5]};
  const long long chroma = std::max({std::llabs((long long)k.cub), std::llabs((long long)k.cug) + std::llabs((long long)k.cvg),
                                     std::llabs((long long)k.cvr)});
  if (k.y_off < 0 || k.y_off > 255 || k.cy <= 0 || 255LL * k.cy + 128 * chroma + (1 << 19) >= (1LL << 31))
    return fail(YM_EINVAL, "%s: bad coefficients (y_off %d, CY %d, CUB %d, CUG %d, CVG %d, CVR %d)", who, k.y_off, k.cy,
                k.cub, k.cug, k.cvg, k.cvr);
  return YM_OK;
}

int ym_letterbox_nv12(ym_ctx* c, const ym_nv12_desc* d_desc, const ym_nv12_desc* h_desc, int B, const int coef[6],
                      float* d_dst, int Hn, int Wn, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_desc || !h_desc || !d_dst) return fail(YM_EINVAL, "ym_letterbox_nv12: null pointer");
  if (B < 1 || B > 65535) return fail(YM_EINVAL, "ym_letterbox_nv12: B %d outside 1..65535", B);
  if (Hn < 1 || Wn < 4 || Wn % 4) return fail(YM_EINVAL, "ym_letterbox_nv12: bad canvas %dx%d (Wn: a multiple of 4)", Hn, Wn);
  if (reinterpret_cast<uintptr_t>(d_dst) & 15) return fail(YM_EINVAL, "ym_letterbox_nv12: d_dst not 16-byte aligned");
  LetterboxNv12Args a{};
  if (int rc = nv12_coef("ym_letterbox_nv12", coef, a.coef)) return rc;
  for (int b = 0; b < B; ++b) {
    const ym_nv12_desc& d = h_desc[b];
    if (!d.y || !d.uv || d.h < 2 || d.w < 2 || (d.h & 1) || (d.w & 1) || d.y_pitch < d.w || d.uv_pitch < d.w ||
        d.uh < 1 || d.uw < 1 || d.top < 0 || d.left < 0 || (long long)d.top + d.uh > Hn || (long long)d.left + d.uw > Wn)
      return fail(YM_EINVAL, "ym_letterbox_nv12: frame %d: bad geometry (%dx%d (both even), pitches %d / %d -> %dx%d at "
                  "(%d, %d) in %dx%d)", b, d.h, d.w, d.y_pitch, d.uv_pitch, d.uh, d.uw, d.top, d.left, Hn, Wn);
    if (d.scale_x != 1.0 / ((double)d.uw / d.w) || d.scale_y != 1.0 / ((double)d.uh / d.h))
      return fail(YM_EINVAL, "ym_letterbox_nv12: frame %d: scales (%.17g, %.17g) are not 1 / (uw / w), 1 / (uh / h)", b,
                  d.scale_x, d.scale_y);
  }
  HIPCK(hipSetDevice(c->device));
  a.desc = d_desc; a.dst = d_dst; a.B = B; a.Hn = Hn; a.Wn = Wn;
  return launched(ym_launch_letterbox_nv12(a, static_cast<hipStream_t>(stream)), "letterbox_nv12 launch");
}

int ym_nv12_to_bgr(ym_ctx* c, const void* y, const void* uv, int h, int w, int y_pitch, int uv_pitch, const int coef[6],
                   void* d_bgr, int row_bytes, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!y || !uv || !d_bgr || h < 2 || w < 2 || (h & 1) || (w & 1) || h > 4 * 65535 || y_pitch < w || uv_pitch < w ||
      row_bytes < 3 * (long long)w)
    return fail(YM_EINVAL, "bad ym_nv12_to_bgr geometry (%dx%d (both even), pitches %d / %d, BGR rows %d bytes)", h, w,
                y_pitch, uv_pitch, row_bytes);
  Nv12ToBgrArgs a{};
  if (int rc = nv12_coef("ym_nv12_to_bgr", coef, a.coef)) return rc;
  HIPCK(hipSetDevice(c->device));
  a.y = static_cast<const unsigned char*>(y); a.uv = static_cast<const unsigned char*>(uv);
  a.h = h; a.w = w; a.y_pitch = y_pitch; a.uv_pitch = uv_pitch;
  a.bgr = static_cast<unsigned char*>(d_bgr); a.row_bytes = row_bytes;
  return launched(ym_launch_nv12_to_bgr(a, static_cast<hipStream_t>(stream)), "nv12_to_bgr launch");
}

int ym_classify_pre(ym_ctx* c, const void* d_images, const ym_cls_pre_desc* d_desc, const ym_cls_pre_desc* h_desc,
                    int B, int imgsz, float* d_dst, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_images || !d_desc || !h_desc || !d_dst) return fail(YM_EINVAL, "ym_classify_pre: null pointer");
  if (reinterpret_cast<uintptr_t>(d_images) & 15) return fail(YM_EINVAL, "ym_classify_pre: d_images not 16-byte aligned");
  if (B < 1 || B > 65535) return fail(YM_EINVAL, "ym_classify_pre: B %d outside 1..65535", B);
  if (imgsz < 32 || imgsz % 32) return fail(YM_EINVAL, "ym_classify_pre: imgsz %d is no positive multiple of 32", imgsz);
  ClsPreArgs a{};
  a.KH = a.KV = 3;
  for (int b = 0; b < B; ++b) {
    const ym_cls_pre_desc& d = h_desc[b];
    if (d.off < 0 || d.off % 16 || d.h < 1 || d.w < 1 || d.rh < 1 || d.rw < 1 || (d.bgr != 0 && d.bgr != 1))
      return fail(YM_EINVAL, "ym_classify_pre: image %d: bad descriptor (off %lld, %dx%d -> %dx%d, bgr %d)", b, d.off,
                  d.h, d.w, d.rh, d.rw, d.bgr);
    if (d.row_bytes < 3 * (long long)d.w)
      return fail(YM_EINVAL, "ym_classify_pre: image %d: row_bytes %d below 3 * w = %lld", b, d.row_bytes,
                  3 * (long long)d.w);
    if (d.top < 0 || d.left < 0 || (long long)d.top + imgsz > d.rh || (long long)d.left + imgsz > d.rw)
      return fail(YM_EINVAL, "ym_classify_pre: image %d: crop window %d at (%d, %d) outside %dx%d", b, imgsz, d.top,
                  d.left, d.rh, d.rw);
    if (d.h > (long long)kClsPreMaxScale * d.rh || d.w > (long long)kClsPreMaxScale * d.rw)
      return fail(YM_EINVAL, "ym_classify_pre: image %d: %dx%d -> %dx%d reduces by more than %d", b, d.h, d.w, d.rh,
                  d.rw, kClsPreMaxScale);
    a.KH = std::max(a.KH, ym_cls_pre_taps(d.w, d.rw));
    a.KV = std::max(a.KV, ym_cls_pre_taps(d.h, d.rh));
  }
  HIPCK(hipSetDevice(c->device));
  a.images = static_cast<const unsigned char*>(d_images);
  a.desc = d_desc; a.dst = d_dst; a.B = B; a.imgsz = imgsz;
  return launched(ym_launch_cls_pre(a, static_cast<hipStream_t>(stream)), "classify_pre launch");
}

static int launch_masks(ym_ctx* c, MaskArgs& a, int B, int H, int W, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (c->task != 1 || c->proto_buf < 0) return fail(YM_ESTATE, "ym_masks needs a segment plan");
  if (int rc = mask_protos(c, "ym_masks", B, H, W, a)) return rc;
  HIPCK(hipSetDevice(c->device));
  a.no = 6 + c->nm; a.B = B; a.H = H; a.W = W;
  if (a.total == 0) return YM_OK;
  if (!ym_masks_fused(a)) {  // the two-kernel path: (total, MH, MW) prototype-resolution scratch
    const size_t need = (size_t)a.total * a.MH * a.MW * sizeof(float);
    if (int rc = c->lowres.grow(need, "mask scratch hipMalloc(%zu)", need)) return rc;
    a.lowres = static_cast<float*>(c->lowres.p);
  }
  return launched(ym_launch_masks(a, static_cast<hipStream_t>(stream)), "mask kernels");
}

int ym_masks(ym_ctx* c, const float* d_dets, int B, int max_det, const int* d_offsets, int total, int H, int W,
             unsigned char* d_masks, int* d_nonempty, void* stream) {
  if (total < 0 || max_det < 1 || (total > 0 && (!d_dets || !d_offsets || !d_masks || !d_nonempty)))
    return fail(YM_EINVAL, "bad ym_masks arguments");
  MaskArgs a{};
  a.dets = d_dets; a.max_det = max_det; a.offsets = d_offsets; a.total = total;
  a.masks = d_masks; a.nonempty = d_nonempty;
  return launch_masks(c, a, B, H, W, stream);
}

int ym_masks_slots(ym_ctx* c, const float* d_dets, int B, int max_det, const int* d_counts, int cap, int H, int W,
                   unsigned char* d_masks, int* d_flags, void* stream) {
  if (B < 1 || cap < 1 || max_det < 1 || cap > max_det || !d_dets || !d_counts || !d_masks || !d_flags)
    return fail(YM_EINVAL, "bad ym_masks_slots arguments");
  MaskArgs a{};
  a.dets = d_dets; a.max_det = max_det; a.counts = d_counts; a.cap = cap; a.total = B * cap;
  a.masks = d_masks; a.nonempty = d_flags;
  return launch_masks(c, a, B, H, W, stream);
}

int ym_masks_native(ym_ctx* c, const float* d_dets, int det_stride, int B, int max_det, const int* d_offsets, int total,
                    int H, int W, const int* shapes, const int* d_shapes, const long long* d_mask_offsets,
                    unsigned char* d_masks, int* d_nonempty, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (B < 1 || total < 0 || max_det < 1 || !shapes || !d_dets || !d_offsets || !d_shapes || !d_mask_offsets ||
      (total > 0 && (!d_masks || !d_nonempty)))
    return fail(YM_EINVAL, "bad ym_masks_native arguments");
  long long max_bytes = 0;
  for (int b = 0; b < B; ++b) {
    const long long h0 = shapes[2 * b], w0 = shapes[2 * b + 1];
    if (h0 < 1 || w0 < 1 || h0 * w0 > (1ll << 30))
      return fail(YM_EINVAL, "ym_masks_native: native size %lld x %lld of image %d (1 x 1 .. 2^30 pixels)", h0, w0, b);
    max_bytes = std::max(max_bytes, h0 * w0);
  }
  if (c->task != 1 || c->proto_buf < 0) return fail(YM_ESTATE, "ym_masks_native needs a segment plan");
  if (det_stride < 6 + c->nm) return fail(YM_EINVAL, "ym_masks_native: row stride %d below %d", det_stride, 6 + c->nm);
  MaskNativeArgs a{};
  if (int rc = mask_protos(c, "ym_masks_native", B, H, W, a)) return rc;
  if (total == 0) return YM_OK;
  HIPCK(hipSetDevice(c->device));
  a.dets = d_dets; a.max_det = max_det; a.stride = det_stride;
  a.offsets = d_offsets; a.B = B; a.total = total;
  a.shapes = d_shapes; a.byte_off = d_mask_offsets; a.masks = d_masks; a.nonempty = d_nonempty;
  return launched(ym_launch_masks_native(a, max_bytes, static_cast<hipStream_t>(stream)), "native mask kernel");
}

// ---------------------------------------------------------------------------------- annotated frames
int ym_annotate(ym_ctx* c, const void* d_frames, int frames_are_f32_chw, int B, int H, int W, const float* d_dets,
                int max_det, const int* d_counts, const unsigned char* d_masks, const long long* d_mask_offsets,
                int mask_h, int mask_w, const int* d_mask_geo, const unsigned char* d_names, const ym_annotate_args* args,
                unsigned char* d_out, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_frames || !d_dets || !d_counts || !args || !d_out) return fail(YM_EINVAL, "ym_annotate: null pointer argument");
  if (!args->d_font) return fail(YM_EINVAL, "ym_annotate: no font table (ym_annotate_args.d_font)");
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > YM_ANNOT_MAX_SIDE || W > YM_ANNOT_MAX_SIDE)
    return fail(YM_EINVAL, "ym_annotate: batch %d of %d x %d frames (1..65535 of 1..%d a side)", B, H, W, YM_ANNOT_MAX_SIDE);
  if (max_det < 1 || max_det > (1 << 20)) return fail(YM_EINVAL, "ym_annotate: max_det %d", max_det);
  if (args->line_width < 1 || args->line_width > kAnnotMaxLw || args->kpt_radius < 0 || args->kpt_radius > kAnnotMaxLw)
    return fail(YM_EINVAL, "ym_annotate: line width %d (1..%d), keypoint radius %d (0..%d)", args->line_width, kAnnotMaxLw,
                args->kpt_radius, kAnnotMaxLw);
  if (args->K < 0 || args->K > kAnnotMaxK || (args->K > 0 && args->ndim != 2 && args->ndim != 3))
    return fail(YM_EINVAL, "ym_annotate: keypoint shape (%d, %d) (K 0..%d, ndim 2 | 3)", args->K, args->ndim, kAnnotMaxK);
  const int tracked = args->tracked ? 1 : 0;
  if (args->det_stride < 6 + tracked + args->K * (args->K ? args->ndim : 0) || args->det_stride > (1 << 16))
    return fail(YM_EINVAL, "ym_annotate: row stride %d below the %d values of a row with %d x %d keypoints",
                args->det_stride, 6 + tracked + args->K * args->ndim, args->K, args->ndim);
  if (args->color_mode != YM_ANNOT_COLOR_CLASS && args->color_mode != YM_ANNOT_COLOR_INSTANCE)
    return fail(YM_EINVAL, "ym_annotate: color_mode %d", args->color_mode);
  if (args->flags & ~(YM_ANNOT_BOXES | YM_ANNOT_LABELS | YM_ANNOT_CONF | YM_ANNOT_MASKS | YM_ANNOT_KPT_LINE | YM_ANNOT_CLIP_KPTS))
    return fail(YM_EINVAL, "ym_annotate: unknown switch bits 0x%x", args->flags);
  if (args->nc < 0 || (args->nc > 0 && !d_names)) return fail(YM_EINVAL, "ym_annotate: %d class names, null table", args->nc);
  if (d_masks && (!d_mask_offsets || mask_h < 1 || mask_w < 1 || mask_h > YM_ANNOT_MAX_SIDE || mask_w > YM_ANNOT_MAX_SIDE ||
                  args->mask_cap < 0))
    return fail(YM_EINVAL, "ym_annotate: masks of %d x %d bytes, offsets %p, cap %d", mask_h, mask_w,
                (const void*)d_mask_offsets, args->mask_cap);
  HIPCK(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t need = (size_t)B * max_det;  // (records)
  if (int rc = c->annot.grow(need * sizeof(AnnotRec), "ym_annotate: %zu records", need)) return rc;
  AnnotArgs a{};
  a.st.H = H; a.st.W = W; a.st.lw = args->line_width; a.st.radius = args->kpt_radius; a.st.flags = args->flags;
  a.st.by_instance = args->color_mode == YM_ANNOT_COLOR_INSTANCE; a.st.tracked = tracked;
  a.st.K = args->K; a.st.ndim = args->K ? args->ndim : 0; a.st.nc = args->nc;
  a.st.det_stride = args->det_stride; a.st.max_det = max_det;
  a.frames = d_frames; a.f32_chw = frames_are_f32_chw ? 1 : 0; a.B = B;
  a.dets = d_dets; a.counts = d_counts;
  a.masks = d_masks; a.mask_offsets = d_mask_offsets; a.mask_h = mask_h; a.mask_w = mask_w;
  a.mask_cap = args->mask_cap ? args->mask_cap : max_det; a.mask_geo = d_mask_geo;
  a.names = d_names; a.font = static_cast<const unsigned char*>(args->d_font);
  a.recs = static_cast<AnnotRec*>(c->annot.p); a.out = d_out;
  return launched(ym_launch_annotate(a, st), "annotate kernels");
}

// ---------------------------------------------------------------------------------- instance polygons
int ym_mask_contours(ym_ctx* c, const unsigned char* d_masks, int n, int H, int W, long long plane_stride, int* d_points,
                     long long cap_points, long long* d_offsets, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_offsets || (n > 0 && !d_masks) || (cap_points > 0 && !d_points))
    return fail(YM_EINVAL, "ym_mask_contours: null pointer argument");
  if (n < 0 || H < 1 || W < 1 || (long long)H * W > kContourMaxPixels || cap_points < 0)
    return fail(YM_EINVAL, "ym_mask_contours: %d planes of %d x %d (1 x 1 .. 2^27 pixels), capacity %lld", n, H, W, cap_points);
  if (plane_stride < (long long)H * W)
    return fail(YM_EINVAL, "ym_mask_contours: plane stride %lld below %d x %d", plane_stride, H, W);
  HIPCK(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long words = ym_ct_words(H, W);
  const bool in_lds = words <= kContourLdsWords;
  const size_t sel_bytes = ((size_t)n * sizeof(CtSel) + 255) & ~(size_t)255;
  const size_t need = sel_bytes + (in_lds ? 0 : (size_t)n * (size_t)words * sizeof(uint32_t));
  if (int rc = c->contour.grow(need, "ym_mask_contours: %zu scratch bytes", need)) return rc;
  char* const ws = static_cast<char*>(c->contour.p);
  return launched(ym_launch_contours(d_masks, plane_stride, n, H, W,
                                     in_lds ? nullptr : reinterpret_cast<uint32_t*>(ws + sel_bytes),
                                     reinterpret_cast<CtSel*>(ws), d_points, cap_points, d_offsets, st),
                  "contour kernels");
}

// ---------------------------------------------------------------------------------- run-length encoding
int ym_mask_rle(ym_ctx* c, const unsigned char* d_masks, int n, int H, int W, long long plane_stride, unsigned int* d_counts,
                long long cap_counts, unsigned char* d_bytes, long long cap_bytes, long long* d_run_offsets,
                long long* d_byte_offsets, long long* d_area, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_run_offsets || !d_byte_offsets || (n > 0 && (!d_masks || !d_area)) || (cap_counts > 0 && !d_counts) ||
      (cap_bytes > 0 && !d_bytes))
    return fail(YM_EINVAL, "ym_mask_rle: null pointer argument");
  if (n < 0 || H < 1 || W < 1 || (long long)H * W > kRleMaxPixels || cap_counts < 0 || cap_bytes < 0)
    return fail(YM_EINVAL, "ym_mask_rle: %d planes of %d x %d (1 x 1 .. 2^27 pixels), capacities %lld, %lld", n, H, W,
                cap_counts, cap_bytes);
  if (plane_stride < (long long)H * W)
    return fail(YM_EINVAL, "ym_mask_rle: plane stride %lld below %d x %d", plane_stride, H, W);
  const RleGeom g = ym_rle_geom(H, W);
  const long long strips = (long long)n * g.strips;
  if (strips > 0x7fffffffll) return fail(YM_EINVAL, "ym_mask_rle: %d planes of %d strips", n, g.strips);
  HIPCK(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const auto pad = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t agg_bytes = pad((size_t)strips * sizeof(RleAgg)), set_bytes = pad((size_t)strips * sizeof(int));
  const size_t total_bytes = pad((size_t)n * sizeof(RleAgg));
  const size_t need = 2 * agg_bytes + set_bytes + total_bytes + (size_t)strips * g.CS * g.JS * sizeof(uint32_t);
  if (int rc = c->rle.grow(need, "ym_mask_rle: %zu scratch bytes", need)) return rc;
  RleScratch ws;
  char* at = static_cast<char*>(c->rle.p);
  ws.own = reinterpret_cast<RleAgg*>(at);
  ws.prefix = reinterpret_cast<RleAgg*>(at += agg_bytes);
  ws.set = reinterpret_cast<int*>(at += agg_bytes);
  ws.total = reinterpret_cast<RleAgg*>(at += set_bytes);
  ws.words = reinterpret_cast<uint32_t*>(at += total_bytes);
  return launched(ym_launch_rle(d_masks, plane_stride, n, g, ws, cap_counts > 0 ? d_counts : nullptr, cap_counts,
                                cap_bytes > 0 ? d_bytes : nullptr, cap_bytes, d_run_offsets, d_byte_offsets, d_area, st),
                  "rle kernels");
}

}  // extern "C"
