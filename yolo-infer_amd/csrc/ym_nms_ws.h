// The scratch of one NMS stage over nB images of A candidates each: where every region lies and how large it is.
// The forward's arena (ym_runtime.cpp ensure_workspace) and the merged test-time-augmentation scratch (ensure_tta)
// both lay their NMS block out through nms_scratch_append, so a region is sized in one place.  Plain C++, no HIP
// (tests/nms_ws_check.cpp builds it alone with a host compiler).
#pragma once
#include <cstddef>

constexpr int kMlCap = 32768;  // multi-label mode: selected keys per image (max_nms up to this; csrc/ym_nms_ml.hip)
constexpr size_t kMlHistBins = 1024;  // ... and the bins of its select histogram
constexpr size_t kMlStateBytes = 24;  // sizeof(MlState) (ym_common.h; ym_runtime.cpp asserts it)

// One region: image i's part starts `off + i * stride` bytes into the allocation (stride 0: the region is absent)
struct NmsRegion {
  size_t off = 0, stride = 0;
  size_t at(int img) const { return off + (size_t)img * stride; }
};

struct NmsScratch {
  NmsRegion boxes, scores, cls;   // decoded candidates: (nB, A) float4 / float / int
  NmsRegion keys, keys2, counts;  // (nB, kstride) sort keys, the presort's chunk-sorted copy, (nB) candidate counts
  NmsRegion sboxes, sareas, sup;  // the NMS kernel's own (nB, A) float4 / float / byte rows
  NmsRegion rows;                 // rows_per_anchor > 0: (nB, A, rows_per_anchor) fp32 merged class rows
  NmsRegion sel, sel2, hist, state, seln;  // ml: (nB, kMlCap) keys twice, (nB, 1024) bins, (nB) MlState, (nB) counts
  int A = 0, kstride = 0;  // kstride: the smallest power of two >= A
  bool ml = false;
  int rows_per_anchor = 0;
};

// Appends the regions behind byte `off`, each on a multiple of 256 bytes (as `off` is), and returns the first byte
// behind them.
inline size_t nms_scratch_append(NmsScratch& s, size_t off, int nB, int A, bool ml, int rows_per_anchor) {
  s = NmsScratch{};
  s.A = A;
  for (s.kstride = 1; s.kstride < A;) s.kstride <<= 1;
  s.ml = ml;
  s.rows_per_anchor = rows_per_anchor;
  auto put = [&](NmsRegion& r, size_t per_image) {
    r.off = off;
    r.stride = per_image;
    off = (off + (size_t)nB * per_image + 255) / 256 * 256;
  };
  const size_t a = (size_t)A, k = (size_t)s.kstride;
  put(s.boxes, a * 16); put(s.scores, a * 4); put(s.cls, a * 4);
  put(s.keys, k * 8);   put(s.keys2, k * 8);  put(s.counts, 4);
  put(s.sboxes, a * 16); put(s.sareas, a * 4); put(s.sup, a);
  if (rows_per_anchor > 0) put(s.rows, a * (size_t)rows_per_anchor * 4);
  if (ml) {
    put(s.sel, (size_t)kMlCap * 8); put(s.sel2, (size_t)kMlCap * 8);
    put(s.hist, kMlHistBins * 4);   put(s.state, kMlStateBytes);   put(s.seln, 4);
  }
  return off;
}
