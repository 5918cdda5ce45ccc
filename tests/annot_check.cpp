// Stand-alone host check of csrc/ym_annot.h (the only project header included): the functions the annotator kernels
// call, run on the CPU.  tests/test_plot_host.py builds it (with AddressSanitizer and UBSan where they link) and compares
// its output with tests/plot_oracle.py.
//   annot_check fmt <file>            fp32 values -> one "%.2f" rendering per line (ym_annot_fmt2)
//   annot_check render <scene> <out>  a scene file -> the H x W x 3 canvas bytes, painted in draw order (each primitive
//                                     over what is there; the kernel walks topmost-first instead)
//   annot_check count <kind> ...      covered pixels of one primitive on a 64 x 64 canvas (disc cx cy r | limb ax ay bx by t)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../yolo-infer_amd/csrc/ym_annot.h"

static std::vector<unsigned char> slurp(const char* path) {
  std::vector<unsigned char> v;
  FILE* f = std::fopen(path, "rb");
  if (!f) {
    std::fprintf(stderr, "cannot open %s\n", path);
    std::exit(2);
  }
  unsigned char buf[65536];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

struct Reader {
  const std::vector<unsigned char>& v;
  size_t at = 0;
  const unsigned char* take(size_t n) {
    if (at + n > v.size()) {
      std::fprintf(stderr, "scene file too short\n");
      std::exit(2);
    }
    const unsigned char* p = v.data() + at;
    at += n;
    return p;
  }
  std::vector<unsigned char> bytes(size_t n) {
    const unsigned char* p = take(n);
    return std::vector<unsigned char>(p, p + n);
  }
};

static void put(unsigned char* px, unsigned col) {
  px[0] = col & 255u;
  px[1] = (col >> 8) & 255u;
  px[2] = (col >> 16) & 255u;
}

static int render(const char* scene, const char* out_path) {
  const std::vector<unsigned char> file = slurp(scene);
  Reader rd{file};
  int hdr[21];
  std::memcpy(hdr, rd.take(sizeof hdr), sizeof hdr);
  AnnotStyle st{};
  st.H = hdr[0]; st.W = hdr[1]; st.lw = hdr[2]; st.radius = hdr[3]; st.flags = hdr[4]; st.by_instance = hdr[5];
  st.tracked = hdr[6]; st.K = hdr[7]; st.ndim = hdr[8]; st.nc = hdr[9]; st.det_stride = hdr[10];
  const int n = hdr[11], f32 = hdr[12], has_masks = hdr[13], mh = hdr[14], mw = hdr[15], mcap = hdr[16];
  const int geo[4] = {hdr[17], hdr[18], hdr[19], hdr[20]};
  st.max_det = n > 0 ? n : 1;
  const size_t HW = (size_t)st.H * st.W;
  const std::vector<unsigned char> font = rd.bytes((size_t)kAnnotGlyphs * kAnnotGlyphH);
  const std::vector<unsigned char> names = rd.bytes((size_t)st.nc * kAnnotName);
  std::vector<float> rows((size_t)n * st.det_stride);
  if (!rows.empty()) std::memcpy(rows.data(), rd.take(rows.size() * 4), rows.size() * 4);
  std::vector<float> ff;
  std::vector<unsigned char> fb;
  if (f32) {
    ff.resize(3 * HW);
    std::memcpy(ff.data(), rd.take(ff.size() * 4), ff.size() * 4);
  } else {
    fb = rd.bytes(3 * HW);
  }
  std::vector<unsigned char> masks;
  if (has_masks) masks = rd.bytes((size_t)mcap * mh * mw);

  std::vector<AnnotRec> recs(n);
  for (int i = 0; i < n; ++i) ym_annot_build(rows.data() + (size_t)i * st.det_stride, i, st, st.nc ? names.data() : nullptr, recs[i]);
  std::vector<unsigned char> img(3 * HW);
  const int thick = ym_annot_limb_thickness(st.lw), P = ym_annot_nprims(st.K);
  for (int y = 0; y < st.H; ++y)
    for (int x = 0; x < st.W; ++x) {
      unsigned u[3];
      for (int c = 0; c < 3; ++c) u[c] = f32 ? ym_annot_canvas(ff[c * HW + (size_t)y * st.W + x]) : fb[((size_t)y * st.W + x) * 3 + c];
      int my, mx;
      if ((st.flags & YM_ANNOT_MASKS) && has_masks && ym_annot_mask_px(x, y, st.H, st.W, geo, mh, mw, my, mx)) {
        int k = 0;
        unsigned cm[3] = {0, 0, 0};
        for (int i = 0; i < n && i < mcap; ++i)
          if (masks[((size_t)i * mh + my) * mw + mx]) {
            ++k;
            for (int c = 0; c < 3; ++c) {
              const unsigned v = (recs[i].b.col >> (8 * c)) & 255u;
              if (v > cm[c]) cm[c] = v;
            }
          }
        if (k)
          for (int c = 0; c < 3; ++c) u[c] = ym_annot_blend(u[c], k, cm[c]);
      }
      unsigned col = u[0] | (u[1] << 8) | (u[2] << 16);
      if (st.flags & YM_ANNOT_BOXES)
        for (int i = n - 1; i >= 0; --i) {
          unsigned c;
          if (recs[i].box && ym_annot_box_hit(recs[i].b, x, y, st.lw, font.data(), c)) col = c;
        }
      for (int i = n - 1; i >= 0; --i)
        for (int p = 0; p < P; ++p) {
          AnnotPrim pr;
          if (ym_annot_record_prim(recs[i], p, st.K, (st.flags & YM_ANNOT_KPT_LINE) != 0, pr) &&
              ym_annot_prim_covers(pr, x, y, st.radius, thick))
            col = pr.col;
        }
      put(&img[((size_t)y * st.W + x) * 3], col);
    }
  FILE* f = std::fopen(out_path, "wb");
  if (!f || std::fwrite(img.data(), 1, img.size(), f) != img.size()) {
    std::fprintf(stderr, "cannot write %s\n", out_path);
    return 2;
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 3 && !std::strcmp(argv[1], "fmt")) {
    const std::vector<unsigned char> file = slurp(argv[2]);
    for (size_t i = 0; i + 4 <= file.size(); i += 4) {
      float v;
      std::memcpy(&v, file.data() + i, 4);
      char s[8] = {0};
      s[ym_annot_fmt2(v, s)] = 0;
      std::puts(s);
    }
    return 0;
  }
  if (argc == 4 && !std::strcmp(argv[1], "render")) return render(argv[2], argv[3]);
  if (argc >= 3 && !std::strcmp(argv[1], "count")) {
    int a[5] = {0, 0, 0, 0, 0};
    for (int i = 3; i < argc && i < 8; ++i) a[i - 3] = std::atoi(argv[i]);
    const bool limb = !std::strcmp(argv[2], "limb");
    int cnt = 0;
    for (int y = 0; y < 64; ++y)
      for (int x = 0; x < 64; ++x)
        cnt += limb ? ym_annot_limb(x, y, a[0], a[1], a[2], a[3], a[4]) : ym_annot_disc(x, y, a[0], a[1], a[2]);
    std::printf("%d\n", cnt);
    return 0;
  }
  std::fprintf(stderr, "usage: annot_check fmt <file> | render <scene> <out> | count disc cx cy r | count limb ax ay bx by t\n");
  return 2;
}
