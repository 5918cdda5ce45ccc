// COCO run-length encoding of mask planes (csrc/ym_rle.hip; driven by ym_mask_rle in ym_rt_post.cpp):
// pycocotools' rleEncode / rleToString.  Pixel (x, y) of an H x W plane has the column-major index x * H + y, a
// transition is an index whose pixel differs from the one before it (pixel -1 is 0), the counts are the distances
// between transitions (the last one reaches H * W), and count k is written to the string as count[k] - count[k - 2]
// (k > 2) in 5-bit groups.
//
// This header holds what the kernels and a stand-alone host program share (tests/rle_check.cpp includes only this
// file): how a plane is cut into strips of column bit words, the word-transition rule with its carry, the walk that
// turns words into transition positions, the summary of a range of transitions (RleAgg) with its associative join, and
// the byte-group encoder with its length.  The kernels run exactly these; there is no second definition.
//
// Bit words: 32 consecutive rows of one column per word, row 32 * j + r of column x in bit r of word (x, j); bits from
// row H on are zero.  A column has wpc = ceil(H / 32) words and the words of a plane are ordered column after column,
// which is the order of the column-major index.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define YM_HD __host__ __device__
#else
#define YM_HD
#endif

constexpr int kRleThreads = 256;                // one workgroup per strip
constexpr int kRleLdsWords = 13312;             // a strip's bit words live in LDS (52 KiB): 640 x 640 is one strip
constexpr long long kRleMaxPixels = 1ll << 27;  // per plane: positions and count differences stay in 29 bits

// How a plane is cut.  A strip is `cols` whole columns (nJ == 1) or, for a column taller than 32 * kRleLdsWords rows,
// a piece of one column (CS == 1, nJ pieces per column); either way its words are consecutive in the plane's order.
struct RleGeom {
  int H, W, wpc;
  int CS, JS;  // columns and words per column of a full strip
  int nJ, strips;
};

YM_HD inline RleGeom ym_rle_geom(int H, int W) {
  RleGeom g;
  g.H = H;
  g.W = W;
  g.wpc = (H + 31) / 32;
  if (g.wpc <= kRleLdsWords) {
    g.CS = kRleLdsWords / g.wpc;
    if (g.CS >= 4) g.CS &= ~3;  // strips start at a multiple of 4 columns: aligned 4-byte reads
    if (g.CS >= W) g.CS = W;
    g.JS = g.wpc;
    g.nJ = 1;
  } else {
    g.CS = 1;
    g.JS = kRleLdsWords;
    g.nJ = (g.wpc + g.JS - 1) / g.JS;
  }
  g.strips = ((W + g.CS - 1) / g.CS) * g.nJ;
  return g;
}

struct RleStrip {
  int x0, cols;  // columns x0 .. x0 + cols - 1
  int j0, rows;  // words j0 .. j0 + rows - 1 of each; word l of the strip is (x0 + l / rows, j0 + l % rows)
  int words;
};

YM_HD inline RleStrip ym_rle_strip(const RleGeom& g, int s) {
  RleStrip t;
  t.x0 = (s / g.nJ) * g.CS;
  t.cols = g.W - t.x0 < g.CS ? g.W - t.x0 : g.CS;
  t.j0 = (s % g.nJ) * g.JS;
  t.rows = g.wpc - t.j0 < g.JS ? g.wpc - t.j0 : g.JS;
  t.words = t.cols * t.rows;
  return t;
}

// The pixel before the strip's first one in column-major order, as a raster index into the byte plane (-1: none).
YM_HD inline long long ym_rle_strip_pred(const RleGeom& g, const RleStrip& s) {
  if (s.j0 > 0) return (long long)(32 * s.j0 - 1) * g.W + s.x0;
  if (s.x0 > 0) return (long long)(g.H - 1) * g.W + s.x0 - 1;
  return -1;
}

// The rows of a word that exist: the word starts at row y0.
YM_HD inline uint32_t ym_rle_valid(int H, int y0) { return H - y0 >= 32 ? 0xffffffffu : (1u << (H - y0)) - 1u; }

// The carry into a word from the word before it in the plane's order: its last row when that is the word above, else
// (the last word of the previous column) row H - 1.
YM_HD inline uint32_t ym_rle_carry(uint32_t prev, bool same_column, int H) {
  return (prev >> (same_column ? 31 : (H - 1) & 31)) & 1u;
}

// The word-transition rule: bit r is set when row r differs from the row before it.
YM_HD inline uint32_t ym_rle_transitions(uint32_t bits, uint32_t carry, uint32_t valid) {
  return (bits ^ ((bits << 1) | carry)) & valid;
}

// The transitions of words l0 .. l1 - 1 of a strip, in order: fn(position).  `bits`: the strip's words; `ext_carry`:
// the pixel before the strip (used by word 0 only).
template <class F>
YM_HD inline void ym_rle_walk(const uint32_t* bits, const RleGeom& g, const RleStrip& s, int l0, int l1, uint32_t ext_carry,
                              F&& fn) {
  if (l0 >= l1) return;
  int cx = l0 / s.rows, jj = l0 % s.rows;
  uint32_t prev = l0 ? bits[l0 - 1] : 0u;
  for (int l = l0; l < l1; ++l) {
    const uint32_t b = bits[l];
    const int y0 = 32 * (s.j0 + jj);
    const uint32_t carry = l ? ym_rle_carry(prev, jj != 0, g.H) : ext_carry;
    const int pos0 = (s.x0 + cx) * g.H + y0;
    for (uint32_t t = ym_rle_transitions(b, carry, ym_rle_valid(g.H, y0)); t; t &= t - 1u) fn(pos0 + __builtin_ctz(t));
    prev = b;
    if (++jj == s.rows) {
      jj = 0;
      ++cx;
    }
  }
}

// One count's bytes: 5 bits a group, bit 5 says another follows, + 48.  Returns the length (1 .. 6 for 29-bit values);
// out may be null.
YM_HD inline int ym_rle_group(int x, unsigned char* out) {
  int n = 0;
  bool more;
  do {
    int c = x & 0x1f;
    x >>= 5;
    more = (c & 0x10) ? x != -1 : x != 0;
    if (more) c |= 0x20;
    if (out) out[n] = (unsigned char)(c + 48);
    ++n;
  } while (more);
  return n;
}
YM_HD inline int ym_rle_group_len(int x) { return ym_rle_group(x, nullptr); }

// A range of consecutive transitions of one plane.  Joined left to right (ym_rle_join is associative) it becomes the
// plane's prefix: then `runs` is the rank of the next transition, tail holds the positions its count and its byte
// group need, and ym_rle_prefix_bytes is where its bytes start.
struct RleAgg {
  int runs;     // transitions in the range
  int bytes;    // group lengths of those with rank >= 3 in the range: the three before them lie in the range too
  int head[3];  // the positions of the first min(runs, 3): their groups wait for what comes before the range
  int tail[3];  // the positions of the last min(runs, 3), latest first; 0 where there is none (pixel -1 is at 0)
};

// Count and string value of a transition at p that follows the plane prefix a.
YM_HD inline int ym_rle_count(const RleAgg& a, int p) { return p - (a.runs ? a.tail[0] : 0); }
YM_HD inline int ym_rle_value(const RleAgg& a, int p) {
  const int c = ym_rle_count(a, p);
  return a.runs > 2 ? c - (a.tail[1] - a.tail[2]) : c;
}

YM_HD inline void ym_rle_advance(RleAgg& a, int p) {
  a.tail[2] = a.tail[1];
  a.tail[1] = a.tail[0];
  a.tail[0] = p;
  ++a.runs;
}

YM_HD inline void ym_rle_push(RleAgg& a, int p) {
  if (a.runs >= 3) a.bytes += ym_rle_group_len(ym_rle_value(a, p));
  else if (a.runs == 2) a.head[2] = p;  // (constant indices: the summary stays in registers)
  else if (a.runs == 1) a.head[1] = p;
  else a.head[0] = p;
  ym_rle_advance(a, p);
}

YM_HD inline RleAgg ym_rle_join(RleAgg a, const RleAgg& b) {
  const int nb = b.runs < 3 ? b.runs : 3;
  for (int i = 0; i < 3; ++i)
    if (i < nb) ym_rle_push(a, b.head[i]);
  if (b.runs >= 3) {
    a.tail[0] = b.tail[0];
    a.tail[1] = b.tail[1];
    a.tail[2] = b.tail[2];
  }
  a.runs += b.runs - nb;
  a.bytes += b.bytes;
  return a;
}

// The string bytes of a plane prefix: its first three counts are written as they are.
YM_HD inline int ym_rle_prefix_bytes(const RleAgg& a) {
  RleAgg e = {};
  int total = a.bytes;
  for (int i = 0; i < 3; ++i)
    if (i < a.runs) {
      total += ym_rle_group_len(ym_rle_value(e, a.head[i]));
      ym_rle_advance(e, a.head[i]);
    }
  return total;
}

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
// Scratch of one call (one buffer of the context): per (plane, strip) the strip's own summary, its plane prefix, its
// set pixels and g.CS * g.JS words (written for strips with transitions only); per plane the whole plane's summary.
struct RleScratch {
  RleAgg* own;
  RleAgg* prefix;
  int* set;
  RleAgg* total;
  uint32_t* words;
};
hipError_t ym_launch_rle(const unsigned char* masks, long long plane_stride, int n, const RleGeom& g, const RleScratch& ws,
                         uint32_t* counts, long long cap_counts, unsigned char* bytes, long long cap_bytes,
                         long long* run_offsets, long long* byte_offsets, long long* area, hipStream_t st);
#endif
