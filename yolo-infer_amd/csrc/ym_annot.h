// Annotated frames (csrc/ym_annot.hip; driven by ym_annotate in ym_runtime.cpp): Results.plot()'s boxes, labels,
// masks, keypoints, skeletons and track ids, composited per pixel on the device.  DESIGN.md §17 states the rules.
//
// This header holds everything that decides a pixel and is shared by the kernels and a stand-alone host program
// (tests/annot_check.cpp includes only this file): the colour tables, the record a detection row is turned into
// (integer box, colours, label placement, label text with the confidence formatted here), the coverage predicates of
// every primitive, the mask geometry and the blend.  All geometry is exact integer arithmetic; the blend is fp32 with
// every operation rounded on its own.  No HIP includes.
#pragma once
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#define YM_HD __host__ __device__
#else
#define YM_HD
#endif

constexpr int kAnnotText = 48;       // label characters, at most: "id:-2147483648 " (15) + 24 + " 0.00" (5)
constexpr int kAnnotName = 24;       // bytes per class name in the device table (longer names are cut)
constexpr int kAnnotMaxK = 32;       // keypoints per instance, at most
constexpr int kAnnotMaxLw = 255;     // line width / keypoint radius, at most
constexpr int kAnnotGlyphW = 6, kAnnotGlyphH = 11, kAnnotGlyphs = 95;  // the font: ASCII 32..126, one byte per row
constexpr int kAnnotBoxClamp = 1 << 30;  // box corners are clamped here before truncation (no pixel can tell)
constexpr int kAnnotKptClamp = 1 << 20;  // a keypoint further out than this is not drawable (keeps the limb test in int64)

#ifndef YM_ANNOT_BOXES  // the switch bits of include/yolomi.h, restated for a program that includes only this header
#define YM_ANNOT_BOXES 1
#define YM_ANNOT_LABELS 2
#define YM_ANNOT_CONF 4
#define YM_ANNOT_MASKS 8
#define YM_ANNOT_KPT_LINE 16
#define YM_ANNOT_CLIP_KPTS 32
#endif

struct AnnotStyle {
  int H, W;          // canvas
  int lw, radius;    // line width, keypoint radius
  int flags;         // YM_ANNOT_*
  int by_instance;   // colour by track id (tracked rows) or row index instead of by class
  int tracked;       // rows are [x1 y1 x2 y2 id conf cls extras] instead of [x1 y1 x2 y2 conf cls extras]
  int K, ndim;       // keypoints per row (0: none) and values per keypoint (2 | 3)
  int nc;            // rows of the class-name table
  int det_stride, max_det;
};

// The part of a record the box pass reads (copied into LDS by the draw kernel).
struct AnnotBox {
  int X1, Y1, X2, Y2;    // the truncated corners
  int left, top, w, h;   // the label rectangle; w == 0: no label
  int s, len;            // glyph scale, characters
  unsigned col, txt;     // instance and text colour, canvas channel c in bits 8c..8c+7
  char text[kAnnotText];
};

struct AnnotRec {
  AnnotBox b;
  int box;               // 1: outline (and label) are drawn
  unsigned kmask;        // bit k: keypoint k is drawable
  int kb[4];             // x0, y0, x1, y1 around every keypoint primitive (x0 > x1: none)
  int kx[kAnnotMaxK], ky[kAnnotMaxK];
};

struct AnnotPrim {
  int ax, ay, bx, by;  // disc: centre a; limb: the segment a -> b
  unsigned col;
  int limb;
};

// ------------------------------------------------------------------------------------------------ colour tables
// Restated from Ultralytics 8.3.x utils/plotting.py (Colors) as remembered; stored as R, G, B and used as B, G, R.
YM_HD inline unsigned ym_annot_pack_rgb(unsigned r, unsigned g, unsigned b) { return b | (g << 8) | (r << 16); }

YM_HD inline unsigned ym_annot_palette(long long i) {
  const unsigned hex[20] = {0x042AFF, 0x0BDBEB, 0xF3F3F3, 0x00DFB7, 0x111F68, 0xFF6FDD, 0xFF444F, 0xCCED00, 0x00F344, 0xBD00FF,
                            0x00B4FF, 0xDD00BA, 0x00FFFF, 0x26C000, 0x01FFB3, 0x7D24FF, 0x7B0068, 0xFF1B6C, 0xFC6D2F, 0xA2FF0B};
  const unsigned h = hex[(int)(((i % 20) + 20) % 20)];
  return ym_annot_pack_rgb(h >> 16, (h >> 8) & 255u, h & 255u);
}

YM_HD inline unsigned ym_annot_pose_palette(int i) {
  const unsigned char p[20][3] = {{255, 128, 0},   {255, 153, 51},  {255, 178, 102}, {230, 230, 0},   {255, 153, 255},
                                  {153, 204, 255}, {255, 102, 255}, {255, 51, 255},  {102, 178, 255}, {51, 153, 255},
                                  {255, 153, 153}, {255, 102, 102}, {255, 51, 51},   {153, 255, 153}, {102, 255, 102},
                                  {51, 255, 51},   {0, 255, 0},     {0, 0, 255},     {255, 0, 0},     {255, 255, 255}};
  return ym_annot_pack_rgb(p[i][0], p[i][1], p[i][2]);
}

constexpr int kAnnotLimbs = 19;
YM_HD inline unsigned ym_annot_kpt_colour(int k) { return ym_annot_pose_palette(k < 5 ? 16 : k < 11 ? 0 : 9); }
YM_HD inline unsigned ym_annot_limb_colour(int l) {
  const unsigned char idx[kAnnotLimbs] = {9, 9, 9, 9, 7, 7, 7, 0, 0, 0, 0, 0, 16, 16, 16, 16, 16, 16, 16};
  return ym_annot_pose_palette(idx[l]);
}
YM_HD inline void ym_annot_limb_ends(int l, int& a, int& b) {  // 0-based keypoints of limb l
  const unsigned char sk[kAnnotLimbs][2] = {{16, 14}, {14, 12}, {17, 15}, {15, 13}, {12, 13}, {6, 12}, {7, 13}, {6, 7}, {6, 8}, {7, 9},
                                            {8, 10},  {9, 11},  {2, 3},   {1, 2},   {1, 3},   {2, 4},  {3, 5},  {4, 6}, {5, 7}};
  a = sk[l][0] - 1;
  b = sk[l][1] - 1;
}

// White, or the dark text colour on a light background.
YM_HD inline unsigned ym_annot_text_colour(unsigned col) {
  const unsigned B = col & 255u, G = (col >> 8) & 255u, R = (col >> 16) & 255u;
  const unsigned luma = (299u * R + 587u * G + 114u * B) / 1000u;
  return luma >= 160u ? (17u | (31u << 8) | (104u << 16)) : 0xFFFFFFu;
}

// ------------------------------------------------------------------------------------------------ numbers
// int(v) of a row value: false for NaN; clamped to +-lim first (so +-inf and huge values stay in int range).
YM_HD inline bool ym_annot_trunc(float v, int lim, int& out) {
  if (v != v) return false;
  const float l = (float)lim;
  out = v >= l ? lim : v <= -l ? -lim : (int)v;
  return true;
}

// The digits of Python's "%.2f" % float(v) for an fp32 v in [0, 10): the value is mantissa * 2^(e - 150) exactly, so
// mantissa * 100 is shifted and rounded half to even on the exact remainder.  Anything else, and a value that rounds
// up to 10.00, prints "?.??"; -0 prints as 0.
YM_HD inline int ym_annot_fmt2(float v, char* out) {
  out[1] = '.';
  out[0] = out[2] = out[3] = '?';
  if (!(v >= 0.f) || !(v < 10.f)) return 4;
  union { float f; uint32_t u; } cv;
  cv.f = v;
  const uint32_t ef = (cv.u >> 23) & 255u;
  const uint64_t mant = (cv.u & 0x7FFFFFu) | (ef ? 0x800000u : 0u);
  const int shift = 150 - (int)(ef ? ef : 1u);  // >= 20 below 10
  const uint64_t N = mant * 100u;              // < 2^31
  uint64_t q = 0;
  if (shift <= 62) {
    q = N >> shift;
    const uint64_t rem = N & ((1ull << shift) - 1), half = 1ull << (shift - 1);
    if (rem > half || (rem == half && (q & 1u))) ++q;
  }
  if (q > 999) return 4;
  out[0] = (char)('0' + (int)(q / 100));
  out[2] = (char)('0' + (int)((q / 10) % 10));
  out[3] = (char)('0' + (int)(q % 10));
  return 4;
}

YM_HD inline int ym_annot_put_int(long long v, char* out) {
  char tmp[24];
  int n = 0, len = 0;
  unsigned long long a = v < 0 ? 0ull - (unsigned long long)v : (unsigned long long)v;
  do {
    tmp[n++] = (char)('0' + (int)(a % 10));
    a /= 10;
  } while (a);
  if (v < 0) out[len++] = '-';
  while (n) out[len++] = tmp[--n];
  return len;
}

// ------------------------------------------------------------------------------------------------ coverage
YM_HD inline bool ym_annot_outline(int x, int y, int X1, int Y1, int X2, int Y2, int lw) {
  const int a = lw / 2, b = lw - a;
  if (x < X1 - a || x > X2 + a || y < Y1 - a || y > Y2 + a) return false;
  return !(x >= X1 + b && x <= X2 - b && y >= Y1 + b && y <= Y2 - b);
}

// Glyph bit (gx, gy) of character ch: font row bytes hold column gx in bit 5 - gx.
YM_HD inline bool ym_annot_glyph(const unsigned char* font, int ch, int gx, int gy) {
  if (ch < 32 || ch > 126) ch = '?';
  return (font[(ch - 32) * kAnnotGlyphH + gy] >> (kAnnotGlyphW - 1 - gx)) & 1;
}

// Label rectangle and text of a box at pixel (x, y): 0 not covered, 1 rectangle, 2 text.
YM_HD inline int ym_annot_label(const AnnotBox& b, int x, int y, const unsigned char* font) {
  if (b.w <= 0 || x < b.left || x >= b.left + b.w || y < b.top || y >= b.top + b.h) return 0;
  const int pad = b.s, tx = x - b.left - pad, ty = y - b.top - pad;
  if (tx < 0 || ty < 0) return 1;
  const int cx = tx / b.s, gy = ty / b.s, j = cx / kAnnotGlyphW;
  if (j >= b.len || gy >= kAnnotGlyphH) return 1;
  return ym_annot_glyph(font, (unsigned char)b.text[j], cx % kAnnotGlyphW, gy) ? 2 : 1;
}

// Text, rectangle, outline of one box, topmost first; false: the box does not cover the pixel.
YM_HD inline bool ym_annot_box_hit(const AnnotBox& b, int x, int y, int lw, const unsigned char* font, unsigned& col) {
  const int l = ym_annot_label(b, x, y, font);
  if (l) {
    col = l == 2 ? b.txt : b.col;
    return true;
  }
  if (!ym_annot_outline(x, y, b.X1, b.Y1, b.X2, b.Y2, lw)) return false;
  col = b.col;
  return true;
}

YM_HD inline bool ym_annot_disc(int x, int y, int cx, int cy, int r) {
  const long long dx = (long long)x - cx, dy = (long long)y - cy;
  return dx * dx + dy * dy <= (long long)r * r;
}

// Capsule of thickness t around the integer segment A -> B (|coordinates| <= kAnnotKptClamp, t <= kAnnotMaxLw).
YM_HD inline bool ym_annot_limb(int x, int y, int ax, int ay, int bx, int by, int t) {
  const long long t2 = (long long)t * t;
  const long long px = (long long)x - ax, py = (long long)y - ay, qx = (long long)x - bx, qy = (long long)y - by;
  if (4 * (px * px + py * py) <= t2 || 4 * (qx * qx + qy * qy) <= t2) return true;
  const long long ex = (long long)bx - ax, ey = (long long)by - ay, L2 = ex * ex + ey * ey;
  if (L2 <= 0) return false;
  const long long dot = px * ex + py * ey;
  if (dot < 0 || dot > L2) return false;
  long long cr = px * ey - py * ex;
  if (cr < 0) cr = -cr;
  if (cr > (1ll << 30)) return false;  // t2 * L2 < 2^60: far off the line, and 4 cr^2 stays below 2^63
  return 4 * cr * cr <= t2 * L2;
}

YM_HD inline bool ym_annot_prim_covers(const AnnotPrim& p, int x, int y, int radius, int t) {
  return p.limb ? ym_annot_limb(x, y, p.ax, p.ay, p.bx, p.by, t) : ym_annot_disc(x, y, p.ax, p.ay, radius);
}

// x0, y0, x1, y1 (inclusive) around a primitive.
YM_HD inline void ym_annot_prim_bbox(const AnnotPrim& p, int radius, int t, int bb[4]) {
  if (!p.limb) {
    bb[0] = p.ax - radius; bb[1] = p.ay - radius; bb[2] = p.ax + radius; bb[3] = p.ay + radius;
    return;
  }
  const int m = t / 2 + 1;
  bb[0] = (p.ax < p.bx ? p.ax : p.bx) - m; bb[1] = (p.ay < p.by ? p.ay : p.by) - m;
  bb[2] = (p.ax > p.bx ? p.ax : p.bx) + m; bb[3] = (p.ay > p.by ? p.ay : p.by) + m;
}

YM_HD inline int ym_annot_limb_thickness(int lw) { return (lw + 1) / 2; }

// Primitives of one instance in draw order: discs 0..K-1, then (K == 17) the 19 limbs.
YM_HD inline int ym_annot_nprims(int K) { return K == 17 ? K + kAnnotLimbs : K; }

// Primitive p of a record; false when it is not drawn.
YM_HD inline bool ym_annot_record_prim(const AnnotRec& r, int p, int K, bool kpt_line, AnnotPrim& out) {
  if (p < K) {
    if (!((r.kmask >> p) & 1u)) return false;
    out.ax = out.bx = r.kx[p];
    out.ay = out.by = r.ky[p];
    out.col = K == 17 ? ym_annot_kpt_colour(p) : ym_annot_palette(p);
    out.limb = 0;
    return true;
  }
  if (K != 17 || !kpt_line) return false;
  int a, b;
  ym_annot_limb_ends(p - K, a, b);
  if (!((r.kmask >> a) & 1u) || !((r.kmask >> b) & 1u)) return false;
  out.ax = r.kx[a]; out.ay = r.ky[a]; out.bx = r.kx[b]; out.by = r.ky[b];
  out.col = ym_annot_limb_colour(p - K);
  out.limb = 1;
  return true;
}

// Upstream's effective rule (Keypoints zeroes points below 0.5, Annotator.kpts skips zero and border coordinates),
// plus: finite and within kAnnotKptClamp.
// clip: x and y are first clipped to [0, W] and [0, H], as predict()'s Results hold them (ops.scale_coords' clip), so
// raw NMS rows draw what the Results built from them draw.
YM_HD inline bool ym_annot_kpt(const float* k, int ndim, int W, int H, bool clip, int& ix, int& iy) {
  float x = k[0], y = k[1];
  if (ndim == 3 && !(k[2] >= 0.5f)) return false;
  if (clip) {
    x = x < 0.f ? 0.f : x > (float)W ? (float)W : x;
    y = y < 0.f ? 0.f : y > (float)H ? (float)H : y;
  }
  const float lim = (float)kAnnotKptClamp;
  if (!(x >= -lim && x <= lim && y >= -lim && y <= lim)) return false;  // (NaN fails too)
  if (fmodf(x, (float)W) == 0.f || fmodf(y, (float)H) == 0.f) return false;
  ix = (int)x;
  iy = (int)y;
  return true;
}

// ------------------------------------------------------------------------------------------------ the record
// names: nc x kAnnotName bytes (0 ends a name), or null.
YM_HD inline void ym_annot_build(const float* row, int i, const AnnotStyle& st, const unsigned char* names, AnnotRec& r) {
  const int ccol = st.tracked ? 6 : 5, kcol = st.tracked ? 7 : 6;
  const float conf = row[ccol - 1];
  int cls = 0, id = 0;
  const bool cls_ok = ym_annot_trunc(row[ccol], kAnnotBoxClamp, cls);
  if (st.tracked) ym_annot_trunc(row[4], kAnnotBoxClamp, id);
  AnnotBox& b = r.b;
  b.col = ym_annot_palette(st.by_instance ? (st.tracked ? id : i) : cls);
  b.txt = ym_annot_text_colour(b.col);
  r.box = (st.flags & YM_ANNOT_BOXES) && ym_annot_trunc(row[0], kAnnotBoxClamp, b.X1) &&
          ym_annot_trunc(row[1], kAnnotBoxClamp, b.Y1) && ym_annot_trunc(row[2], kAnnotBoxClamp, b.X2) &&
          ym_annot_trunc(row[3], kAnnotBoxClamp, b.Y2);
  if (!r.box) b.X1 = b.Y1 = b.X2 = b.Y2 = 0;
  b.left = b.top = b.w = b.h = b.len = 0;
  b.s = st.lw / 2 > 1 ? st.lw / 2 : 1;
  for (int j = 0; j < kAnnotText; ++j) b.text[j] = 0;
  if (r.box && (st.flags & YM_ANNOT_LABELS)) {
    int len = 0;
    if (st.tracked) {
      b.text[len++] = 'i'; b.text[len++] = 'd'; b.text[len++] = ':';
      len += ym_annot_put_int(id, b.text + len);
      b.text[len++] = ' ';
    }
    const int len0 = len;
    if (names && cls_ok && cls >= 0 && cls < st.nc) {
      const unsigned char* nm = names + (size_t)cls * kAnnotName;
      for (int j = 0; j < kAnnotName && nm[j]; ++j) b.text[len++] = nm[j] >= 32 && nm[j] <= 126 ? (char)nm[j] : '?';
    }
    if (len == len0) b.text[len++] = '?';  // a class without a name
    if (st.flags & YM_ANNOT_CONF) {
      b.text[len++] = ' ';
      len += ym_annot_fmt2(conf, b.text + len);
    }
    b.len = len;
    const int pad = b.s, tw = kAnnotGlyphW * b.s * len, th = kAnnotGlyphH * b.s;
    b.w = tw + 2 * pad;
    b.h = th + 2 * pad;
    b.left = (long long)b.X1 + b.w > st.W ? (st.W - b.w > 0 ? st.W - b.w : 0) : b.X1;
    b.top = b.Y1 - b.h >= 0 ? b.Y1 - b.h : b.Y1;
  }
  r.kmask = 0;
  r.kb[0] = r.kb[1] = 1;
  r.kb[2] = r.kb[3] = 0;
  const int t = ym_annot_limb_thickness(st.lw);
  const int m = st.radius > t / 2 + 1 ? st.radius : t / 2 + 1;
  for (int k = 0; k < kAnnotMaxK; ++k) {
    int ix = 0, iy = 0;
    if (k < st.K && ym_annot_kpt(row + kcol + k * st.ndim, st.ndim, st.W, st.H, (st.flags & YM_ANNOT_CLIP_KPTS) != 0, ix, iy)) {
      if (!r.kmask) {
        r.kb[0] = ix - m; r.kb[1] = iy - m; r.kb[2] = ix + m; r.kb[3] = iy + m;
      } else {
        if (ix - m < r.kb[0]) r.kb[0] = ix - m;
        if (iy - m < r.kb[1]) r.kb[1] = iy - m;
        if (ix + m > r.kb[2]) r.kb[2] = ix + m;
        if (iy + m > r.kb[3]) r.kb[3] = iy + m;
      }
      r.kmask |= 1u << k;
    }
    r.kx[k] = ix;
    r.ky[k] = iy;
  }
}

// x0, y0, x1, y1 (inclusive) around the outline and the label of a box.
YM_HD inline void ym_annot_box_bbox(const AnnotBox& b, int lw, int bb[4]) {
  const int a = lw / 2;
  bb[0] = b.X1 - a; bb[1] = b.Y1 - a; bb[2] = b.X2 + a; bb[3] = b.Y2 + a;
  if (b.w > 0) {
    if (b.left < bb[0]) bb[0] = b.left;
    if (b.top < bb[1]) bb[1] = b.top;
    if (b.left + b.w - 1 > bb[2]) bb[2] = b.left + b.w - 1;
    if (b.top + b.h - 1 > bb[3]) bb[3] = b.top + b.h - 1;
  }
}

YM_HD inline bool ym_annot_touches(const int bb[4], int x0, int y0, int x1, int y1) {
  return bb[0] <= x1 && bb[2] >= x0 && bb[1] <= y1 && bb[3] >= y0;
}

// ------------------------------------------------------------------------------------------------ canvas, masks
// trunc(clamp(x * 255, 0, 255)) of a tensor source's value (NaN: 0), as Results.orig_img converts it.
YM_HD inline unsigned ym_annot_canvas(float x) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float v = __fmul_rn(x, 255.f);
#else
  const float v = x * 255.f;
#endif
  return !(v > 0.f) ? 0u : v >= 255.f ? 255u : (unsigned)v;
}

// The mask pixel behind canvas pixel (x, y); geo = (uh, uw, top, left).  false: outside the mask plane.
YM_HD inline bool ym_annot_mask_px(int x, int y, int H, int W, const int geo[4], int mh, int mw, int& my, int& mx) {
  const long long uh = geo[0], uw = geo[1];
  if (uh < 1 || uw < 1) return false;
  long long yy = ((2ll * y + 1) * uh) / (2ll * H), xx = ((2ll * x + 1) * uw) / (2ll * W);
  if (yy > uh - 1) yy = uh - 1;
  if (xx > uw - 1) xx = uw - 1;
  yy += geo[2];
  xx += geo[3];
  if (yy < 0 || yy >= mh || xx < 0 || xx >= mw) return false;
  my = (int)yy;
  mx = (int)xx;
  return true;
}

// One channel under k >= 1 covering masks whose largest colour value is cmax:
// trunc(clamp(((u / 255) * 0.5^k + (cmax / 255) * 0.5) * 255, 0, 255)), every operation rounded to fp32 on its own.
YM_HD inline unsigned ym_annot_blend(unsigned u, int k, unsigned cmax) {
  const float inv = k < 126 ? ldexpf(1.f, -k) : 0.f;
#if defined(__HIP_DEVICE_COMPILE__)
  const float a = __fmul_rn(__fdiv_rn((float)u, 255.f), inv);
  const float m = __fmul_rn(__fdiv_rn((float)cmax, 255.f), 0.5f);
  const float v = __fmul_rn(__fadd_rn(a, m), 255.f);
#else
  volatile float a = (float)u / 255.f;  // (volatile: no contraction into a fused multiply-add on the host either)
  a = a * inv;
  volatile float m = (float)cmax / 255.f;
  m = m * 0.5f;
  volatile float s = a + m;
  const float v = s * 255.f;
#endif
  return !(v > 0.f) ? 0u : v >= 255.f ? 255u : (unsigned)v;
}

// ------------------------------------------------------------------------------------------------ the launch
struct AnnotArgs {
  AnnotStyle st;
  const void* frames;  // B x 3 x H x W fp32 (f32_chw) or B x H x W x 3 bytes
  int f32_chw, B;
  const float* dets;   // B x max_det rows of det_stride floats
  const int* counts;   // B
  const unsigned char* masks;      // packed mask planes of mask_h x mask_w bytes, or null
  const long long* mask_offsets;   // B: the first mask byte of image b
  int mask_h, mask_w, mask_cap;    // instances i >= mask_cap have no mask
  const int* mask_geo;             // B x (uh, uw, top, left), or null: (H, W, 0, 0)
  const unsigned char* names;      // nc x kAnnotName bytes, or null
  const unsigned char* font;       // kAnnotGlyphs x kAnnotGlyphH row bytes
  AnnotRec* recs;                  // B x max_det records (scratch)
  unsigned char* out;              // B x H x W x 3
};

#if defined(__HIPCC__)
hipError_t ym_launch_annotate(const AnnotArgs& a, hipStream_t st);
#endif
