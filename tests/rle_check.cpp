// Stand-alone host program over csrc/ym_rle.h (nothing else of the project): the kernels' rules, run serially over
// planes built here.  Per plane: pack the column bit words strip by strip, walk every strip in pieces (as the lanes
// do), join the pieces' summaries in a tree (as the scans do), write counts and bytes from the joined prefixes (as the
// write pass does), and compare with a per-pixel loop (pycocotools' rleEncode / rleToString).  Prints "ok <planes>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../yolo-infer_amd/csrc/ym_rle.h"

typedef std::vector<unsigned char> Bytes;

static void reference(const Bytes& src, int H, int W, std::vector<uint32_t>& counts, Bytes& str) {
  unsigned char last = 0;
  uint32_t run = 0;
  for (int x = 0; x < W; ++x)
    for (int y = 0; y < H; ++y) {
      const unsigned char v = src[(size_t)y * W + x] ? 1 : 0;
      if (v != last) counts.push_back(run), run = 0, last = v;
      ++run;
    }
  counts.push_back(run);
  for (size_t k = 0; k < counts.size(); ++k) {
    long x = (long)counts[k] - (k > 2 ? (long)counts[k - 2] : 0);
    bool more = true;
    while (more) {
      long c = x & 0x1f;
      x >>= 5;
      more = (c & 0x10) ? x != -1 : x != 0;
      str.push_back((unsigned char)((more ? c | 0x20 : c) + 48));
    }
  }
}

static RleAgg tree(const std::vector<RleAgg>& v, size_t lo, size_t hi) {  // the join of v[lo .. hi), split in the middle
  return hi - lo == 1 ? v[lo] : ym_rle_join(tree(v, lo, lo + (hi - lo) / 2), tree(v, lo + (hi - lo) / 2, hi));
}

static bool check(const Bytes& src, int H, int W, int piece) {
  std::vector<uint32_t> ref_counts, counts;
  Bytes ref_str, str;
  reference(src, H, W, ref_counts, ref_str);
  const RleGeom g = ym_rle_geom(H, W);
  std::vector<std::vector<uint32_t>> bits(g.strips);
  std::vector<uint32_t> carry(g.strips);
  std::vector<int> strip_of, first;  // per piece: its strip and first word
  std::vector<RleAgg> aggs;
  for (int si = 0; si < g.strips; ++si) {
    const RleStrip s = ym_rle_strip(g, si);
    bits[si].assign(s.words, 0u);
    for (int l = 0; l < s.words; ++l)
      for (int r = 0; r < 32; ++r) {
        const int x = s.x0 + l / s.rows, y = 32 * (s.j0 + l % s.rows) + r;
        if (y < H && src[(size_t)y * W + x]) bits[si][l] |= 1u << r;
      }
    const long long pred = ym_rle_strip_pred(g, s);
    carry[si] = pred >= 0 && src[(size_t)pred] ? 1u : 0u;
    for (int l0 = 0; l0 < s.words; l0 += piece) {
      RleAgg a = {};
      ym_rle_walk(bits[si].data(), g, s, l0, std::min(l0 + piece, s.words), carry[si], [&](int p) { ym_rle_push(a, p); });
      strip_of.push_back(si), first.push_back(l0), aggs.push_back(a);
    }
  }
  const RleAgg all = tree(aggs, 0, aggs.size());
  counts.assign((size_t)all.runs + 1, 0xdeadbeefu);
  str.assign((size_t)ym_rle_prefix_bytes(all) + ym_rle_group_len(ym_rle_value(all, H * W)), 0);
  for (size_t i = 0; i < aggs.size(); ++i) {
    RleAgg e = i ? tree(aggs, 0, i) : RleAgg{};
    int at = ym_rle_prefix_bytes(e);
    const int si = strip_of[i];
    const RleStrip s = ym_rle_strip(g, si);
    ym_rle_walk(bits[si].data(), g, s, first[i], std::min(first[i] + piece, s.words), carry[si], [&](int p) {
      counts[e.runs] = (uint32_t)ym_rle_count(e, p);
      at += ym_rle_group(ym_rle_value(e, p), &str[at]);
      ym_rle_advance(e, p);
    });
  }
  counts[all.runs] = (uint32_t)ym_rle_count(all, H * W);
  ym_rle_group(ym_rle_value(all, H * W), &str[ym_rle_prefix_bytes(all)]);
  if (counts == ref_counts && str == ref_str) return true;
  std::fprintf(stderr, "plane %d x %d, pieces of %d words: %zu counts against %zu, %zu bytes against %zu\n", H, W, piece,
               counts.size(), ref_counts.size(), str.size(), ref_str.size());
  return false;
}

int main() {
  uint32_t seed = 12345u;
  const auto rnd = [&]() { return seed = seed * 1664525u + 1013904223u, seed >> 8; };
  int planes = 0;
  const auto run = [&](int H, int W, int mode, int piece) {
    Bytes src((size_t)H * W);
    const uint32_t dense = rnd() % 100, len = 1 + rnd() % (mode == 2 ? 40000 : 50);
    unsigned char v = 0;
    for (int x = 0; x < W; ++x)
      for (int y = 0; y < H; ++y) {
        if (mode == 0) v = rnd() % 100 < dense ? (unsigned char)(1 + rnd() % 255) : 0;  // noise
        else if (rnd() % len == 0) v = v ? 0 : 255;                                         // runs
        src[(size_t)y * W + x] = mode == 3 ? ((x + y) & 1) : mode == 4 ? 1 : mode == 5 ? 0 : v;
      }
    if (!check(src, H, W, piece)) std::exit(1);
    ++planes;
  };
  const int shapes[][2] = {{1, 1}, {1, 7}, {7, 1}, {3, 3}, {31, 5}, {32, 5}, {33, 5}, {65, 3}, {64, 64}, {5, 70}, {97, 33}};
  for (int i = 0; i < 6 * 11; ++i)
    for (int piece : {1, 2, 3, 7, 1000}) run(shapes[i / 6][0], shapes[i / 6][1], i % 6, piece);
  for (int mode : {0, 1, 2, 3}) run(40, 2 * (kRleLdsWords / 2) + 9, mode, 53);  // three strips of whole columns
  for (int mode : {1, 2, 4}) run(32 * kRleLdsWords + 77, 2, mode, 53);          // pieces of one tall column
  return std::printf("ok %d\n", planes) < 0;
}
