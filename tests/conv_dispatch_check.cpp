// Host check of the conv dispatch routine (yolo-infer_amd/csrc/ym_conv_catalog.h) with a recording stub for `launch`.
//
//   conv_dispatch_check trace    every (dtype, shape class, strict, stub policy, cfg) case: the ordered (family, local)
//                                calls, the returned code and `taken`, run-length coded over the cfg axis
//                                (tests/golden/conv_dispatch_trace.txt, recorded from the dispatch code this routine
//                                replaced)
//   conv_dispatch_check resolve  dtype dw cfg lines on stdin -> "family local" of ymc::resolve
//   conv_dispatch_check split    round trip of the split-pair helpers over all (a, b) in 0..255: prints "ok"
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "../yolo-infer_amd/csrc/ym_conv_catalog.h"

namespace {

struct Call {
  int family, local;
};
struct Result {
  std::vector<Call> calls;
  int code, taken;
};

// stub policies: what the recorded launch answers
enum Policy { P_ACCEPT, P_REFUSE, P_ONLY2, P_ERROR, P_COUNT };
const char* const kPolicy[P_COUNT] = {"accept", "refuse", "only2", "error"};
constexpr int kOtherError = 719;  // an error that is not InvalidValue

struct Recorder {
  Policy policy;
  std::vector<Call> calls;
  int operator()(int family, int local) {
    calls.push_back({family, local});
    switch (policy) {
      case P_ACCEPT: return 0;
      case P_REFUSE: return local < 0 ? 0 : 1;              // everything but the heuristics refuses
      case P_ONLY2: return (local < 0 || local == 2) ? 0 : 1;  // (the first-fit loops go on to index 2)
      default: return calls.size() == 1 ? kOtherError : 0;
    }
  }
};

struct Shape {
  const char* name;
  ymc::ConvShape s;
};
// {dw, nchw, k, s, src1, up0, pair, k2, kpad64, q8_ok}
const Shape kShapes[] = {
    {"1x1", {false, false, 1, 1, false, false, false, 0, true, true}},
    {"1x1-concat", {false, false, 1, 1, true, false, false, 0, true, true}},
    {"3x3", {false, false, 3, 1, false, false, false, 0, true, true}},
    {"3x3-up0", {false, false, 3, 1, false, true, false, 0, true, true}},
    {"pair-k2=1", {false, false, 1, 1, false, false, true, 1, true, true}},
    {"pair-k2=3", {false, false, 3, 1, false, false, true, 3, true, true}},
    {"dw", {true, false, 1, 1, false, false, false, 0, true, true}},
    {"kpad%64", {false, false, 1, 1, false, false, false, 0, false, false}},
    {"q8-unmet", {false, false, 1, 1, false, false, false, 0, true, false}},
};
struct Dtype {
  const char* name;
  int dt;
};
const Dtype kDtypes[] = {{"f16", YM_DT_F16}, {"f32", YM_DT_F32}, {"x3", YM_DT_X3}, {"int8", YM_DT_I8}, {"fp8", YM_DT_F8}};

// ---- the code under test
int num_cfgs(int dtype) { return ymc::num_cfgs(dtype); }
Result dispatch(int dtype, const Shape& sh, int cfg, bool strict, Policy policy) {
  Recorder rec{policy, {}};
  Result r;
  r.taken = -7;
  r.code = ymc::dispatch_conv(dtype, sh.s, cfg, strict, &r.taken, rec);
  r.calls = rec.calls;
  return r;
}
const char* family_name(int f) { return ymc::kFamilies[f].name; }

// ---- run-length output over the cfg axis: a call's local index either stays put over a run ("name[i]") or follows cfg
// ("name[i+]": i at the run's first cfg)
struct Run {
  int first, last;
  Result r0;
  std::vector<int> mode;  // per call: 0 unknown (a run of one), 1 fixed, 2 follows cfg
};
bool extend(Run& run, int cfg, const Result& r) {
  const Result& r0 = run.r0;
  if (r.code != r0.code || r.taken != r0.taken || r.calls.size() != r0.calls.size()) return false;
  const int d = cfg - run.first;
  std::vector<int> mode = run.mode;
  for (size_t i = 0; i < r.calls.size(); ++i) {
    if (r.calls[i].family != r0.calls[i].family) return false;
    const int m = r.calls[i].local == r0.calls[i].local ? 1 : (r.calls[i].local == r0.calls[i].local + d ? 2 : 0);
    if (!m || (mode[i] && mode[i] != m)) return false;
    mode[i] = m;
  }
  run.mode = mode;
  run.last = cfg;
  return true;
}
void print(const Run& run) {
  if (run.first == run.last) printf("  %d:", run.first);
  else printf("  %d..%d:", run.first, run.last);
  for (size_t i = 0; i < run.r0.calls.size(); ++i)
    printf(" %s[%d%s]", family_name(run.r0.calls[i].family), run.r0.calls[i].local, run.mode[i] == 2 ? "+" : "");
  printf(" -> %d taken %d\n", run.r0.code, run.r0.taken);
}

int trace() {
  for (const Dtype& dt : kDtypes)
    for (const Shape& sh : kShapes)
      for (int strict = 0; strict < 2; ++strict)
        for (int p = 0; p < P_COUNT; ++p) {
          printf("%s %s strict=%d %s\n", dt.name, sh.name, strict, kPolicy[p]);
          Run run{0, 0, {}, {}};
          bool open = false;
          for (int cfg = -1; cfg <= num_cfgs(dt.dt) + 2; ++cfg) {
            const Result r = dispatch(dt.dt, sh, cfg, strict != 0, (Policy)p);
            if (open && extend(run, cfg, r)) continue;
            if (open) print(run);
            run = Run{cfg, cfg, r, std::vector<int>(r.calls.size(), 0)};
            open = true;
          }
          print(run);
        }
  return 0;
}

int resolve() {
  int dtype, dw, cfg;
  while (scanf("%d %d %d", &dtype, &dw, &cfg) == 3) {
    const ymc::Slot s = ymc::resolve(dtype, dw != 0, cfg);
    printf("%s %d\n", s.family == ymc::F_NONE ? "none" : ymc::kFamilies[s.family].name, s.local);
  }
  return 0;
}

int split() {
  for (int a = 0; a < 256; ++a)
    for (int b = 0; b < 256; ++b) {
      const int c = ymc::split_encode(a, b);
      if (!ymc::is_split(c) || ymc::split_first(c) != a || ymc::split_second(c) != b) return printf("bad %d %d\n", a, b), 1;
      if (ymc::split_cfg(a) != (a == 255 ? -1 : a)) return printf("bad half %d\n", a), 1;
    }
  if (ymc::is_split(ymc::kSplitTag - 1) || ymc::is_split(ymc::split_encode(255, 255) + 1)) return printf("bad range\n"), 1;
  printf("ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 2 && !strcmp(argv[1], "trace")) return trace();
  if (argc == 2 && !strcmp(argv[1], "resolve")) return resolve();
  if (argc == 2 && !strcmp(argv[1], "split")) return split();
  fprintf(stderr, "usage: conv_dispatch_check trace|resolve|split\n");
  return 2;
}
