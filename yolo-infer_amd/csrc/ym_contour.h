// Instance polygons behind the mask stages (csrc/ym_contour.hip; driven by ym_mask_contours in ym_runtime.cpp): per
// 0/1 byte plane, the outer border of one top-level 8-connected component, traced by Suzuki-Abe border following and
// compressed like OpenCV's CHAIN_APPROX_SIMPLE (the definition is DESIGN.md §18's; tests/contour_oracle.py is its
// sequential restatement).
//
// This header holds what the kernels and a stand-alone host program share (tests/contour_check.cpp includes only this
// file): the bit-plane layout, the 3 x 3 neighbourhood code, the state-successor function, the compression predicate,
// the candidate / validity / top-level rules that replace the sequential raster scan, and the selection key.
//
// Directions are as seen on screen, y down, numbered CLOCKWISE from west: 0 W, 1 NW, 2 N, 3 NE, 4 E, 5 SE, 6 S, 7 SW.
// A tracing state is (p, d): the current border pixel p and the direction d from p to the previous one.
//
// How the raster scan is replaced (every rule needs only the plane, so candidates are independent of each other):
//   candidate   a foreground pixel whose W, NW, N and NE neighbours are background: the raster-first pixel of every
//               component is one (so are other local raster minima: the second prong of a "U", a bump inside a hole)
//   valid       the cycle through (c, q(c)), q(c) the first foreground neighbour clockwise from W, never visits a pixel
//               raster-earlier than c.  Then c is the cycle's raster minimum and the cycle borders the background region
//               that holds c's west neighbour; were that region a hole, the hole's first pixel would have a border pixel
//               above it, earlier than c.  So the cycle is the outer border of c's component, started where the scan
//               would start it, and a component has exactly one valid candidate.
//   top-level   walk west from c along its row to the first foreground pixel p (none: the frame is reached).  p belongs
//               to another component D, and the background run between them joins c's surroundings to the cycle through
//               (p, the first foreground neighbour clockwise from E).  That cycle is D's outer border if and only if it
//               passes through (m, q(m)) for its raster minimum m with m a candidate; then D is a sibling of c's
//               component and the question repeats from m, strictly earlier in raster order.  Otherwise it is a hole
//               border of D: c's component lies in that hole.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YM_HD __host__ __device__
#else
#define YM_HD
#endif

constexpr int kContourThreads = 256;                // one workgroup per mask
constexpr int kContourLdsWords = 15360;             // bit planes up to this many words live in LDS (60 KiB)
constexpr long long kContourMaxPixels = 1ll << 27;  // per plane: chain lengths and raster indices stay in 31 bits

// The bit plane: H + 2 rows of wpr words, pixel (x, y) in bit x + 32 of row y + 1.  Row 0, row H + 1, the first word of
// every row and every bit from W on are zero: "outside the plane is background" needs no bounds check.
YM_HD inline int ym_ct_wpr(int W) { return (W + 31) / 32 + 2; }
YM_HD inline long long ym_ct_words(int H, int W) { return (long long)(H + 2) * ym_ct_wpr(W); }

struct CtPlane {
  const uint32_t* bits;
  int wpr, H, W;
};

// What the selection pass leaves per mask for the offsets and the write pass.
struct CtSel {
  uint32_t count;  // kept points of the chosen border; 0: no foreground
  int start;       // raster index of its start pixel
  int ymax;        // its last row (the write pass packs rows start_y - 1 .. ymax + 1 only)
  int reserved;
};

// One word of the bit plane from the byte plane: pixels 32 * (w - 1) .. + 31 of row py - 1 (non-zero = foreground).
YM_HD inline uint32_t ym_ct_pack_word(const unsigned char* src, int H, int W, int py, int w) {
  if (py < 1 || py > H || w < 1) return 0u;
  const int x0 = 32 * (w - 1);
  const unsigned char* row = src + (long long)(py - 1) * W;
  uint32_t v = 0u;
  for (int i = 0; i < 32; ++i)
    if (x0 + i < W && row[x0 + i]) v |= 1u << i;
  return v;
}

// The three bits x - 1, x, x + 1 of one row of the bit plane (row = bits + (y + 1) * wpr).
YM_HD inline uint32_t ym_ct_row3(const uint32_t* row, int x) {
  const int b = x + 31, w = b >> 5;
  const uint64_t v = (uint64_t)row[w] | ((uint64_t)row[w + 1] << 32);
  return (uint32_t)(v >> (b & 31)) & 7u;
}

// The eight neighbours of (x, y): bit d = the neighbour in direction d.
YM_HD inline uint32_t ym_ct_nb8(const CtPlane& p, int x, int y) {
  const uint32_t* mid = p.bits + (y + 1) * p.wpr;  // (word indices fit 31 bits: kContourMaxPixels)
  const uint32_t t = ym_ct_row3(mid - p.wpr, x), m = ym_ct_row3(mid, x), b = ym_ct_row3(mid + p.wpr, x);
  return (m & 1u) | (t & 1u) << 1 | (t & 2u) << 1 | (t & 4u) << 1 | (m & 4u) << 2 | (b & 4u) << 3 | (b & 2u) << 5 |
         (b & 1u) << 7;
}

YM_HD inline int ym_ct_dx(int d) { return (int)((0x1A90u >> (2 * d)) & 3u) - 1; }  // -1 -1 0 1 1 1 0 -1
YM_HD inline int ym_ct_dy(int d) { return (int)((0xA901u >> (2 * d)) & 3u) - 1; }  // 0 -1 -1 -1 0 1 1 1

// q(p): the first foreground neighbour clockwise starting at W (nb != 0).
YM_HD inline int ym_ct_first_from_w(uint32_t nb) { return __builtin_ctz(nb); }
// ... and starting at E: the state of p on the border with the background to its east.
YM_HD inline int ym_ct_first_from_e(uint32_t nb) { return (4 + __builtin_ctz(((nb | nb << 8) >> 4) & 0xffu)) & 7; }

// The state-successor function: from (p, d) the step goes to the first foreground neighbour of p met COUNTER-clockwise
// starting at the neighbour after d (d itself comes last: a pixel with one neighbour steps back).  Returns the step's
// direction s; the next state is (p + s, (s + 4) & 7).  nb != 0.
YM_HD inline int ym_ct_step(uint32_t nb, int d) {
  const uint32_t rot = ((nb | nb << 8) >> d) & 0xffu;  // bit j = direction d + j: want j = 7, 6, .., 1, then 0
  return (d + 31 - __builtin_clz(rot)) & 7;
}

// The compression predicate (CHAIN_APPROX_SIMPLE on the cyclic chain): a point stays when the step into it and the step
// out of it differ.  The chain's first point is entered by the step from q(s), direction (d0 + 4) & 7.
YM_HD inline bool ym_ct_keep(int step_in, int step_out) { return step_in != step_out; }

// The selection rule (strategy "largest"): most kept points, a tie to the start pixel that is last in raster order.
// 0 is below every border's key.
YM_HD inline uint64_t ym_ct_key(uint32_t count, int start) { return (uint64_t)count << 32 | (uint32_t)start; }

YM_HD inline bool ym_ct_before(int x, int y, int cx, int cy) { return y < cy || (y == cy && x < cx); }

// The candidates among pixels 32 * (w - 1) .. + 31 of row py - 1 (1 <= py <= H, 1 <= w <= wpr - 2), as a bit mask.
YM_HD inline uint32_t ym_ct_candidates(const CtPlane& p, int py, int w) {
  const uint32_t* row = p.bits + py * p.wpr;
  const uint32_t* up = row - p.wpr;
  const uint32_t cur = row[w], u = up[w];
  const uint32_t west = cur << 1 | row[w - 1] >> 31, nw = u << 1 | up[w - 1] >> 31, ne = u >> 1 | up[w + 1] << 31;
  return cur & ~west & ~u & ~nw & ~ne;
}

// The walk from candidate (cx, cy): false when the cycle meets a raster-earlier pixel (not this component's outer
// border).  count: kept points; ymax: the cycle's last row.  emit(x, y) is called for every kept point, in order.
template <class Emit>
YM_HD inline bool ym_ct_outer(const CtPlane& p, int cx, int cy, uint32_t& count, int& ymax, Emit emit) {
  uint32_t nb = ym_ct_nb8(p, cx, cy);
  count = 1;
  ymax = cy;
  if (!nb) {  // an isolated pixel: the border is the single point
    emit(cx, cy);
    return true;
  }
  const int d0 = ym_ct_first_from_w(nb);
  int x = cx, y = cy, d = d0, in = (d0 + 4) & 7;
  uint32_t kept = 0;
  for (int guard = 8 * p.H * p.W; guard >= 0; --guard) {  // every state at most once: a cycle (8 H W <= 2^30)
    const int s = ym_ct_step(nb, d);
    if (ym_ct_keep(in, s)) {
      emit(x, y);
      ++kept;
    }
    in = s;
    x += ym_ct_dx(s);
    y += ym_ct_dy(s);
    d = (s + 4) & 7;
    if (ym_ct_before(x, y, cx, cy)) return false;
    if (x == cx && y == cy && d == d0) {
      count = kept;
      return true;
    }
    ymax = y > ymax ? y : ymax;
    nb = ym_ct_nb8(p, x, y);
  }
  return false;
}

// The first foreground pixel west of (cx, cy) in its row, or -1.
YM_HD inline int ym_ct_west(const CtPlane& p, int cx, int cy) {
  const uint32_t* row = p.bits + (cy + 1) * p.wpr;
  const int b = cx + 31;  // the bit of pixel cx - 1
  uint32_t mask = (b & 31) == 31 ? ~0u : (1u << ((b & 31) + 1)) - 1u;
  for (int w = b >> 5; w >= 1; --w) {
    const uint32_t v = row[w] & mask;
    if (v) return 32 * (w - 1) + 31 - __builtin_clz(v);
    mask = ~0u;
  }
  return -1;
}

// Whether the component whose outer border starts at candidate (cx, cy) is top-level (the header comment's rule).
YM_HD inline bool ym_ct_top_level(const CtPlane& p, int cx, int cy) {
  for (;;) {
    const int px = ym_ct_west(p, cx, cy);
    if (px < 0) return true;
    uint32_t nb = ym_ct_nb8(p, px, cy);
    if (!nb) {  // an isolated pixel is its own outer border: a sibling
      cx = px;
      continue;
    }
    const int d0 = ym_ct_first_from_e(nb);
    int x = px, y = cy, d = d0, mx = px, my = cy;
    bool outer = false;
    bool closed = false;
    for (int guard = 8 * p.H * p.W; guard >= 0; --guard) {
      const bool less = ym_ct_before(x, y, mx, my);
      if (less || (x == mx && y == my)) {
        const bool st = (nb & 0xfu) == 0u && d == ym_ct_first_from_w(nb);
        outer = less ? st : (outer || st);
        mx = x;
        my = y;
      }
      const int s = ym_ct_step(nb, d);
      x += ym_ct_dx(s);
      y += ym_ct_dy(s);
      d = (s + 4) & 7;
      if (x == px && y == cy && d == d0) {
        closed = true;
        break;
      }
      nb = ym_ct_nb8(p, x, y);
    }
    if (!closed || !outer) return false;
    cx = mx;
    cy = my;
  }
}

// One candidate's key when it starts an outer border (valid), top-level or not; else 0.
YM_HD inline uint64_t ym_ct_valid_key(const CtPlane& p, int cx, int cy, int& ymax) {
  uint32_t count;
  if (!ym_ct_outer(p, cx, cy, count, ymax, [](int, int) {})) return 0;
  return ym_ct_key(count, cy * p.W + cx);
}

// One candidate, whole: its key when it starts the outer border of a top-level component and beats `best` (a key some
// top-level border already has: a border that cannot win skips the top-level question), else 0.
YM_HD inline uint64_t ym_ct_eval(const CtPlane& p, int cx, int cy, uint64_t best, int& ymax) {
  const uint64_t key = ym_ct_valid_key(p, cx, cy, ymax);
  if (key <= best || !ym_ct_top_level(p, cx, cy)) return 0;
  return key;
}

// The order the rules are applied in, per plane (the kernel spreads each loop over its lanes; tests/contour_check.cpp
// runs them as they stand):
//   1. every candidate: ym_ct_valid_key, the largest key K over the plane
//   2. K's border alone answers the top-level question; yes (nearly every real mask: the largest border is not inside
//      another component): it is the choice, and no other border was asked
//   3. no: every candidate again through ym_ct_eval with the running best
template <class ForEachCandidate>
YM_HD inline uint64_t ym_ct_select_serial(const CtPlane& p, ForEachCandidate each) {
  uint64_t top = 0;
  each([&](int x, int y) {
    int ymax;
    const uint64_t k = ym_ct_valid_key(p, x, y, ymax);
    top = k > top ? k : top;
  });
  if (!top) return 0;
  const int start = (int)(uint32_t)top;
  if (ym_ct_top_level(p, start % p.W, start / p.W)) return top;
  uint64_t best = 0;
  each([&](int x, int y) {
    int ymax;
    const uint64_t k = ym_ct_eval(p, x, y, best, ymax);
    best = k ? k : best;
  });
  return best;
}

#if defined(__HIPCC__)
// gbits: null when ym_ct_words(H, W) <= kContourLdsWords, else n planes of that many words (scratch); sel: n records.
hipError_t ym_launch_contours(const unsigned char* masks, long long plane_stride, int n, int H, int W, uint32_t* gbits,
                              CtSel* sel, int* points, long long cap, long long* offsets, hipStream_t st);
#endif
