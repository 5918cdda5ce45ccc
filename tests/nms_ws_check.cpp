// nms_ws_check NB A ML ROWS: lay out one NMS scratch (csrc/ym_nms_ws.h nms_scratch_append) behind two different
// starting offsets and check it: every region on a multiple of 256, inside the returned total, disjoint from every other,
// at least as large as what its kernel indexes, image i's part at off + i * (bytes per image), kstride the smallest
// power of two >= A.  Prints "OK TOTAL KSTRIDE" (TOTAL: bytes appended behind offset 0; exit 0) or the failed check
// (exit 1).  Host-only; tests/test_nms_ws_host.py builds it with the sanitizers, so the fill of every region inside
// an exact-size heap block fails too if a region leaves the block.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yolo-infer_amd/csrc/ym_nms_ws.h"

struct Want {
  const char* name;
  const NmsRegion* r;
  size_t per_image;  // bytes of one image its kernel indexes (0: the region must be absent)
};

static int check(int nB, int A, bool ml, int rows, size_t base, size_t* total) {
  NmsScratch s;
  const size_t end = nms_scratch_append(s, base, nB, A, ml, rows);
  size_t ks = 1;
  while (ks < (size_t)A) ks *= 2;
  if (s.A != A || (size_t)s.kstride != ks || s.ml != ml || s.rows_per_anchor != rows) {
    printf("A / kstride / ml / rows recorded as %d / %d / %d / %d\n", s.A, s.kstride, (int)s.ml, s.rows_per_anchor);
    return 1;
  }
  const size_t a = (size_t)A, mlb = ml ? 1 : 0;
  const Want want[] = {
      {"boxes", &s.boxes, a * 16},  {"scores", &s.scores, a * 4},  {"cls", &s.cls, a * 4},
      {"keys", &s.keys, ks * 8},    {"keys2", &s.keys2, ks * 8},   {"counts", &s.counts, 4},
      {"sboxes", &s.sboxes, a * 16}, {"sareas", &s.sareas, a * 4}, {"sup", &s.sup, a},
      {"rows", &s.rows, rows > 0 ? a * (size_t)rows * 4 : 0},
      {"sel", &s.sel, mlb * 32768 * 8},   {"sel2", &s.sel2, mlb * 32768 * 8}, {"hist", &s.hist, mlb * 1024 * 4},
      {"state", &s.state, mlb * 24},      {"seln", &s.seln, mlb * 4},
  };
  if (end < base || (end - base) % 256) {
    printf("end %zu behind base %zu is not a multiple of 256 further\n", end, base);
    return 1;
  }
  std::vector<unsigned char> block(end - base, 0);  // exact size: a fill past the end is a heap overflow
  for (const Want& w : want) {
    if (w.per_image == 0) {
      if (w.r->stride != 0) { printf("%s: present, but not asked for\n", w.name); return 1; }
      continue;
    }
    if (w.r->stride < w.per_image) { printf("%s: %zu bytes per image < %zu\n", w.name, w.r->stride, w.per_image); return 1; }
    if (w.r->off % 256 || w.r->off < base) { printf("%s: offset %zu\n", w.name, w.r->off); return 1; }
    for (int i = 0; i < nB; ++i) {
      if (w.r->at(i) != w.r->off + (size_t)i * w.r->stride) { printf("%s: at(%d)\n", w.name, i); return 1; }
      if (w.r->at(i) + w.per_image > end) { printf("%s: image %d ends behind the total %zu\n", w.name, i, end); return 1; }
      unsigned char* p = block.data() + (w.r->at(i) - base);
      for (size_t b = 0; b < w.per_image; ++b)
        if (p[b]++) { printf("%s: image %d overlaps another region\n", w.name, i); return 1; }
    }
  }
  *total = end - base;
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 5) {
    fprintf(stderr, "usage: nms_ws_check NB A ML ROWS\n");
    return 2;
  }
  const int nB = atoi(argv[1]), A = atoi(argv[2]), ml = atoi(argv[3]), rows = atoi(argv[4]);
  size_t t0 = 0, t1 = 0;
  if (check(nB, A, ml != 0, rows, 0, &t0) || check(nB, A, ml != 0, rows, 7 * 256, &t1)) return 1;
  if (t0 != t1) {
    printf("total %zu behind offset 0, %zu behind offset %d\n", t0, t1, 7 * 256);
    return 1;
  }
  size_t ks = 1;
  while (ks < (size_t)A) ks *= 2;
  printf("OK %zu %zu\n", t0, ks);
  return 0;
}
