// Results.plot() on the device: two launches per batch, no atomics, no host round trip (rules: ym_annot.h).
//
//   annot_records  one thread per detection slot (b, i < counts[b]): the row -> an AnnotRec (integer box, colours, label
//                  placement, label text with the confidence formatted here, integer keypoints and their bounding box).
//   annot_draw     one workgroup per 64 x 16 pixel tile, thread = 4 adjacent pixels of one row.  A pixel's colour is that
//                  of the LAST primitive in draw order that covers it, so the tile walks the primitives topmost first
//                  and a pixel stops at its first hit:
//                    1. keypoint primitives, instances 0..n-1, each limb 18..0 then disc K-1..0: records are culled
//                       256 at a time by their keypoint bounding box into an ordered LDS list (ballot + prefix counts);
//                       that list is expanded 256 / P records at a time (P primitives per instance, one thread per
//                       primitive), culled against the tile into an ordered LDS primitive list; every pixel walks it;
//                    2. boxes 0..n-1 (text, label rectangle, outline): culled 128 at a time into LDS copies; walked;
//                    3. pixels still open: the mask blend over all n instances (their colours staged in LDS, 256 at a
//                       time), or the canvas value itself.
//                  Every list is rebuilt per chunk, so 300 instances x 36 primitives over one tile neither overflow LDS
//                  nor lose a primitive.  Stores: three dwords per thread where its 12 bytes are dword-aligned and
//                  inside the row (always, when W % 4 == 0), bytes otherwise.
#include <hip/hip_runtime.h>

#include "ym_annot.h"

namespace {

constexpr int kTileW = 64, kTileH = 16, kThreads = 256, kPx = 4;  // kThreads * kPx == kTileW * kTileH
constexpr int kBoxChunk = 128;
constexpr int kFontBytes = kAnnotGlyphs * kAnnotGlyphH;

__global__ __launch_bounds__(256) void annot_records(const AnnotArgs a) {
  const int slot = blockIdx.x * 256 + threadIdx.x;
  if (slot >= a.B * a.st.max_det) return;
  const int b = slot / a.st.max_det, i = slot - b * a.st.max_det;
  if (i >= a.counts[b]) return;
  AnnotRec r;
  ym_annot_build(a.dets + (size_t)slot * a.st.det_stride, i, a.st, a.names, r);
  a.recs[slot] = r;
}

// Ordered compaction over the workgroup: the rank of a set flag among the set flags, and their number.  Every thread
// of the workgroup calls it.
__device__ __forceinline__ int annot_rank(bool f, int tid, int* s_cnt, int& total) {
  const unsigned long long m = __ballot(f);
  const int lane = tid & 63, w = tid >> 6;
  const int pre = __popcll(m & ((1ull << lane) - 1ull));
  if (lane == 0) s_cnt[w] = __popcll(m);
  __syncthreads();
  int off = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < kThreads / 64; ++k) {
    const int c = s_cnt[k];
    off += k < w ? c : 0;
    total += c;
  }
  __syncthreads();
  return off + pre;
}

__global__ __launch_bounds__(kThreads) void annot_draw(const AnnotArgs a) {
  __shared__ unsigned char s_font[kFontBytes + 3];
  __shared__ AnnotBox s_box[kBoxChunk];
  __shared__ AnnotPrim s_prim[kThreads];
  __shared__ int s_rec[kThreads];
  __shared__ int s_cnt[kThreads / 64];
  __shared__ unsigned s_col[kThreads];

  const AnnotStyle& st = a.st;
  const int tid = threadIdx.x, b = blockIdx.z;
  const int tx0 = blockIdx.x * kTileW, ty0 = blockIdx.y * kTileH;
  const int tx1 = min(tx0 + kTileW, st.W) - 1, ty1 = min(ty0 + kTileH, st.H) - 1;
  const int y = ty0 + tid / (kTileW / kPx), x0 = tx0 + (tid % (kTileW / kPx)) * kPx;
  const bool row_ok = y < st.H;
  int n = a.counts[b];
  n = n < 0 ? 0 : n > st.max_det ? st.max_det : n;
  const AnnotRec* recs = a.recs + (size_t)b * st.max_det;
  for (int j = tid; j < kFontBytes; j += kThreads) s_font[j] = a.font[j];

  unsigned col[kPx];
  unsigned open = 0;  // bit e: pixel e is inside the canvas and no primitive has covered it yet
#pragma unroll
  for (int e = 0; e < kPx; ++e) {
    col[e] = 0;
    if (row_ok && x0 + e < st.W) open |= 1u << e;
  }
  __syncthreads();

  // ---- 1. keypoint primitives
  const int P = ym_annot_nprims(st.K);
  if (P > 0) {
    const int thick = ym_annot_limb_thickness(st.lw);
    const bool lines = (st.flags & YM_ANNOT_KPT_LINE) != 0;
    const int G = kThreads / P;  // records expanded per round (P <= 36)
    for (int c0 = 0; c0 < n; c0 += kThreads) {
      const int i = c0 + tid;
      bool f = false;
      if (i < n) {
        const AnnotRec& r = recs[i];
        f = r.kmask != 0 && ym_annot_touches(r.kb, tx0, ty0, tx1, ty1);
      }
      int m;
      const int pos = annot_rank(f, tid, s_cnt, m);
      if (f) s_rec[pos] = i;
      __syncthreads();
      for (int g0 = 0; g0 < m; g0 += G) {
        const int g = tid / P, p = P - 1 - tid % P;  // topmost first: record ascending, primitive descending
        AnnotPrim pr;
        bool pf = false;
        if (g < G && g0 + g < m && ym_annot_record_prim(recs[s_rec[g0 + g]], p, st.K, lines, pr)) {
          int bb[4];
          ym_annot_prim_bbox(pr, st.radius, thick, bb);
          pf = ym_annot_touches(bb, tx0, ty0, tx1, ty1);
        }
        int np;
        const int pp = annot_rank(pf, tid, s_cnt, np);
        if (pf) s_prim[pp] = pr;
        __syncthreads();
        if (open) {
          for (int j = 0; j < np; ++j) {
            const AnnotPrim q = s_prim[j];
#pragma unroll
            for (int e = 0; e < kPx; ++e)
              if (((open >> e) & 1u) && ym_annot_prim_covers(q, x0 + e, y, st.radius, thick)) {
                col[e] = q.col;
                open &= ~(1u << e);
              }
          }
        }
        __syncthreads();  // s_prim is rebuilt by the next round
      }
      __syncthreads();  // s_rec is rebuilt by the next chunk
    }
  }

  // ---- 2. boxes: text, label rectangle, outline
  if (st.flags & YM_ANNOT_BOXES) {
    for (int c0 = 0; c0 < n; c0 += kBoxChunk) {
      const int i = c0 + tid;
      bool f = false;
      if (tid < kBoxChunk && i < n && recs[i].box) {
        int bb[4];
        ym_annot_box_bbox(recs[i].b, st.lw, bb);
        f = ym_annot_touches(bb, tx0, ty0, tx1, ty1);
      }
      int m;
      const int pos = annot_rank(f, tid, s_cnt, m);
      if (f) s_box[pos] = recs[i].b;
      __syncthreads();
      if (open) {
        for (int j = 0; j < m; ++j) {
#pragma unroll
          for (int e = 0; e < kPx; ++e) {
            unsigned c;
            if (((open >> e) & 1u) && ym_annot_box_hit(s_box[j], x0 + e, y, st.lw, s_font, c)) {
              col[e] = c;
              open &= ~(1u << e);
            }
          }
        }
      }
      __syncthreads();
    }
  }

  // ---- 3. open pixels: the canvas value under the mask blend
  const size_t HW = (size_t)st.H * st.W;
  const bool blend = (st.flags & YM_ANNOT_MASKS) && a.masks && n > 0;  // (uniform over the workgroup)
  unsigned u[kPx][3];
  long long moff[kPx];  // the pixel's byte in mask plane 0 of this image; -1: no blend for this pixel
#pragma unroll
  for (int e = 0; e < kPx; ++e) {
    moff[e] = -1;
    u[e][0] = u[e][1] = u[e][2] = 0;
    if (!((open >> e) & 1u)) continue;
    const int x = x0 + e;
    if (a.f32_chw) {
      const float* f = static_cast<const float*>(a.frames) + (size_t)b * 3 * HW + (size_t)y * st.W + x;
      for (int c = 0; c < 3; ++c) u[e][c] = ym_annot_canvas(f[c * HW]);
    } else {
      const unsigned char* f = static_cast<const unsigned char*>(a.frames) + ((size_t)b * HW + (size_t)y * st.W + x) * 3;
      for (int c = 0; c < 3; ++c) u[e][c] = f[c];
    }
  }
  if (blend) {
    int geo[4] = {st.H, st.W, 0, 0};
    if (a.mask_geo)
      for (int k = 0; k < 4; ++k) geo[k] = a.mask_geo[4 * b + k];
    const size_t plane = (size_t)a.mask_h * a.mask_w;
    const int nm = n < a.mask_cap ? n : a.mask_cap;
    const unsigned char* mbase = a.masks + a.mask_offsets[b];
    int k[kPx];
    unsigned cm[kPx][3];
#pragma unroll
    for (int e = 0; e < kPx; ++e) {
      k[e] = 0;
      cm[e][0] = cm[e][1] = cm[e][2] = 0;
      int my, mx;
      if (((open >> e) & 1u) && ym_annot_mask_px(x0 + e, y, st.H, st.W, geo, a.mask_h, a.mask_w, my, mx))
        moff[e] = (long long)my * a.mask_w + mx;
    }
    // the instance colours go through LDS, kThreads at a time: one global read per instance and tile
    for (int c0 = 0; c0 < nm; c0 += kThreads) {
      if (c0 + tid < nm) s_col[tid] = recs[c0 + tid].b.col;
      __syncthreads();
      const int cnt = nm - c0 < kThreads ? nm - c0 : kThreads;
      for (int j = 0; j < cnt; ++j) {
        const unsigned c = s_col[j];
        const size_t po = (size_t)(c0 + j) * plane;
#pragma unroll
        for (int e = 0; e < kPx; ++e)
          if (moff[e] >= 0 && mbase[po + (size_t)moff[e]]) {
            ++k[e];
            cm[e][0] = max(cm[e][0], c & 255u);
            cm[e][1] = max(cm[e][1], (c >> 8) & 255u);
            cm[e][2] = max(cm[e][2], (c >> 16) & 255u);
          }
      }
      __syncthreads();  // s_col is rebuilt by the next chunk
    }
#pragma unroll
    for (int e = 0; e < kPx; ++e)
      if (k[e])
        for (int c = 0; c < 3; ++c) u[e][c] = ym_annot_blend(u[e][c], k[e], cm[e][c]);
  }
  if (!row_ok || x0 >= st.W) return;  // (no barrier below)
#pragma unroll
  for (int e = 0; e < kPx; ++e)
    if ((open >> e) & 1u) col[e] = u[e][0] | (u[e][1] << 8) | (u[e][2] << 16);

  // ---- store: 4 pixels = 12 bytes
  unsigned char* o = a.out + ((size_t)b * HW + (size_t)y * st.W + x0) * 3;
  if (x0 + kPx <= st.W && (reinterpret_cast<uintptr_t>(o) & 3u) == 0) {
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
    o4[0] = (col[0] & 0xFFFFFFu) | (col[1] << 24);
    o4[1] = ((col[1] >> 8) & 0xFFFFu) | (col[2] << 16);
    o4[2] = ((col[2] >> 16) & 0xFFu) | (col[3] << 8);
  } else {
    for (int e = 0; e < kPx && x0 + e < st.W; ++e) {
      o[3 * e] = (unsigned char)(col[e] & 255u);
      o[3 * e + 1] = (unsigned char)((col[e] >> 8) & 255u);
      o[3 * e + 2] = (unsigned char)((col[e] >> 16) & 255u);
    }
  }
}

}  // namespace

hipError_t ym_launch_annotate(const AnnotArgs& a, hipStream_t st) {
  const long slots = (long)a.B * a.st.max_det;
  hipLaunchKernelGGL(annot_records, dim3((unsigned)((slots + 255) / 256)), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid((a.st.W + kTileW - 1) / kTileW, (a.st.H + kTileH - 1) / kTileH, a.B);
  hipLaunchKernelGGL(annot_draw, grid, dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
