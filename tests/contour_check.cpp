// Stand-alone host program over csrc/ym_contour.h (nothing else of the project): the kernels' rules, run serially.
// stdin: per plane a line "H W" and H lines of W characters '0' / '1'.
//   contour_check select   per plane one line: k x0 y0 x1 y1 ...  — the chosen border's kept points
//   contour_check all      per plane one line: b, then per top-level border in raster order of the start pixels
//                          k x0 y0 ... — every valid candidate that answers the top-level question with yes
// The plane is packed word by word with ym_ct_pack_word, the candidates come from ym_ct_candidates, and they go through
// ym_ct_select_serial (select: the kernel's three steps, serially) or ym_ct_outer + ym_ct_top_level each (all).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../yolo-infer_amd/csrc/ym_contour.h"

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  const bool all = std::strcmp(argv[1], "all") == 0;
  if (!all && std::strcmp(argv[1], "select") != 0) return 2;
  int H, W;
  std::vector<char> line;
  while (std::scanf("%d %d", &H, &W) == 2) {
    if (H < 1 || W < 1 || (long long)H * W > kContourMaxPixels) return 3;
    std::vector<unsigned char> src((size_t)H * W);
    line.assign((size_t)W + 1, 0);
    for (int y = 0; y < H; ++y) {
      char fmt[32];
      std::snprintf(fmt, sizeof fmt, "%%%ds", W);
      if (std::scanf(fmt, line.data()) != 1 || (int)std::strlen(line.data()) != W) return 3;
      for (int x = 0; x < W; ++x) src[(size_t)y * W + x] = line[x] == '1' ? 1 : 0;
    }
    const int wpr = ym_ct_wpr(W);
    std::vector<uint32_t> bits((size_t)ym_ct_words(H, W));
    for (int py = 0; py < H + 2; ++py)
      for (int w = 0; w < wpr; ++w) bits[(size_t)py * wpr + w] = ym_ct_pack_word(src.data(), H, W, py, w);
    const CtPlane p{bits.data(), wpr, H, W};
    const auto each = [&](auto&& fn) {  // the candidates in raster order
      for (int py = 1; py <= H; ++py)
        for (int w = 1; w <= wpr - 2; ++w)
          for (uint32_t cand = ym_ct_candidates(p, py, w); cand; cand &= cand - 1u) fn(32 * (w - 1) + __builtin_ctz(cand), py - 1);
    };
    uint64_t best = 0;
    std::string out;
    int borders = 0;
    if (!all) best = ym_ct_select_serial(p, each);
    else
      each([&](int x, int y) {
        uint32_t count, seen = 0;
        int ymax;
        std::string pts;
        const bool ok = ym_ct_outer(p, x, y, count, ymax, [&](int px, int py2) {
          pts += " " + std::to_string(px) + " " + std::to_string(py2);
          ++seen;
        });
        if (!ok || !ym_ct_top_level(p, x, y)) return;
        if (seen != count) std::exit(4);
        ++borders;
        out += " " + std::to_string(count) + pts;
      });
    if (all) {
      std::printf("%d%s\n", borders, out.c_str());
      continue;
    }
    const uint32_t count = (uint32_t)(best >> 32);
    std::printf("%u", count);
    if (count) {
      const int start = (int)(uint32_t)best;
      uint32_t c2;
      int ymax;
      if (!ym_ct_outer(p, start % W, start / W, c2, ymax, [](int x, int y) { std::printf(" %d %d", x, y); })) return 4;
      if (c2 != count) return 4;
    }
    std::printf("\n");
  }
  return 0;
}
