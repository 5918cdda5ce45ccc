// The conv-config catalogue: the kernel families behind a flat "conv config id", the one resolver from an id to
// (family, index inside the family), the split-pair encoding of a fused pair run as its two convs, and the one routine
// that decides which family a conv op is launched on (ym_launch_conv, csrc/ym_conv.hip).
//
// Host code with no HIP in it (tests/conv_dispatch_check.cpp builds it with a plain C++17 compiler).  The ids are frozen:
// committed tune tables (yolomi/tuned/*.json) and tests name them, so a new family is appended to its id space.
//
// Known warts, kept as they are (behaviour is frozen; each is a behavioural change of its own):
//  * an f32 plan given an `lds` id (12-16) launches the heuristic tile and returns success even under strict, with
//    `taken` left 0 (kAdmit: `silent`);
//  * f32 is offered the whole f16 id space (116 ids) although only `direct` applies;
//  * a depthwise-fused op is offered its dtype's full id count although only ids 0-7 exist for it;
//  * fp8 is offered the 35 conv_i8 / int8-streaming ids although only the one-K-chain conv_i8 tiles are admitted;
//  * the untuned Bottleneck fallback tries the 14 shared variants only, never the 2 x3-only ones;
//  * a single conv given a Bottleneck id (shared or x3-only), and a single x3 conv given a `halo` id, is refused:
//    InvalidValue under strict, the heuristic otherwise;
//  * strict with no id (cfg < 0) runs the heuristic of a single conv, but is refused for a fused pair or a
//    depthwise-fused op (`needs_pin`);
//  * a refused `direct` (or, f16, `lds`) id returns the refusal even when not strict; only x3 retries a refused `lds`
//    id on the heuristic tile (`terminal`);
//  * `taken` is not tracked (-1) for int8 / fp8 plans, except on the (never built) depthwise-fused ops of one.
#pragma once
#include "ym_plan.h"  // YM_DT_*

namespace ymc {

// The families, each with its name and count: the one place a count is written (each .hip that owns a family
// static_asserts its table against it).  lds, small, dma_x3 and bneck_x3 continue the table of the launcher they share.
#define YMC_FAMILIES(X)                                                                                             \
  X(F_DIRECT, "direct", 12)      /* csrc/ym_conv.hip conv_igemm tiles */                                            \
  X(F_LDS, "lds", 5)             /* csrc/ym_conv.hip conv_lds tiles (f16 / x3) */                                   \
  X(F_DMA, "dma", 30)            /* csrc/ym_conv_dma.hip (int8: its Q8 mode; x3 conv -> 1x1 pairs: the fused GEMM) */ \
  X(F_STREAM, "stream", 31)      /* csrc/ym_conv_stream.hip streaming kernels */                                    \
  X(F_SMALL, "small", 12)        /* csrc/ym_conv_stream.hip small-M kernels */                                      \
  X(F_HALO, "halo", 12)          /* csrc/ym_conv_halo.hip */                                                        \
  X(F_BNECK, "bneck", 14)        /* csrc/ym_conv_bneck.hip */                                                       \
  X(F_DMA_X3, "dma_x3", 9)       /* x3-only LDS-DMA configurations */                                               \
  X(F_BNECK_X3, "bneck_x3", 2)   /* x3-only Bottleneck variants */                                                  \
  X(F_I8, "conv_i8", 12)         /* csrc/ym_conv_i8.hip conv_i8 tiles */                                            \
  X(F_I8_STREAM, "i8_stream", 23) /* csrc/ym_conv_i8_stream.hip streaming and small-M kernels */                    \
  X(F_DWPW, "dwpw", 8)           /* csrc/ym_conv_dwpw.hip */
#define YMC_X(id, name, n) id,
enum Family : int { F_NONE = -1, YMC_FAMILIES(YMC_X) F_COUNT };
#undef YMC_X
struct FamilyInfo {
  const char* name;
  int count;
};
#define YMC_X(id, name, n) {name, n},
constexpr FamilyInfo kFamilies[F_COUNT] = {YMC_FAMILIES(YMC_X)};
#undef YMC_X
constexpr int count(Family f) { return kFamilies[f].count; }
// conv_i8 tiles with one K chain per output (WK = 1), the only ones an fp8 plan admits: bit i = tile i
constexpr unsigned kI8OneChain = 0x627;

// A family's index in its launcher's own table.
constexpr int table_index(Family f, int local) {
  const Family shared = f == F_LDS ? F_DIRECT : f == F_SMALL ? F_STREAM : f == F_DMA_X3 ? F_DMA : f == F_BNECK_X3 ? F_BNECK : F_NONE;
  return local < 0 || shared == F_NONE ? local : count(shared) + local;
}

// The id spaces, families in id order: [YM_DT_*], then the depthwise-fused ops' own (whatever the dtype).
struct Space {
  Family fam[9];
  int n;
};
constexpr Space kSpaces[6] = {{{F_DIRECT, F_LDS, F_DMA, F_STREAM, F_SMALL, F_HALO, F_BNECK}, 7},
                              {{F_DIRECT, F_LDS, F_DMA, F_STREAM, F_SMALL, F_HALO, F_BNECK}, 7},  // f32: f16's (wart)
                              {{F_I8, F_I8_STREAM, F_DMA}, 3},
                              {{F_I8, F_I8_STREAM}, 2},
                              {{F_DIRECT, F_LDS, F_DMA, F_STREAM, F_SMALL, F_HALO, F_BNECK, F_DMA_X3, F_BNECK_X3}, 9},
                              {{F_DWPW}, 1}};
struct Slot {
  Family family;  // F_NONE: cfg < 0 or past the space
  int local;
};
// The only place a base offset is computed.
constexpr Slot resolve(int dtype, bool dw, int cfg) {
  const Space& s = kSpaces[dw ? 5 : dtype];
  for (int i = 0, base = 0; i < s.n && cfg >= base; base += count(s.fam[i++]))
    if (cfg < base + count(s.fam[i])) return {s.fam[i], cfg - base};
  return {F_NONE, -1};
}
// ids a plan dtype is offered (the public ym_num_conv_cfgs; depthwise-fused ops are offered the same count: wart)
constexpr int num_cfgs(int dtype) {
  int n = 0;
  for (int i = 0; i < kSpaces[dtype].n; ++i) n += count(kSpaces[dtype].fam[i]);
  return n;
}

// A fused pair run as its two convs: op cfg = kSplitTag + 256 * cfg(first) + cfg(second), 8 bits per half, a half of
// kSplitHeuristic meaning "that conv's heuristic".
constexpr int kSplitTag = 1 << 20;
constexpr int kSplitHeuristic = 255;
constexpr int split_encode(int a, int b) { return kSplitTag + 256 * a + b; }
constexpr bool is_split(int cfg) { return cfg >= kSplitTag && cfg < kSplitTag + 256 * 256; }
constexpr int split_first(int cfg) { return (cfg - kSplitTag) >> 8; }
constexpr int split_second(int cfg) { return (cfg - kSplitTag) & 255; }
constexpr int split_cfg(int half) { return half == kSplitHeuristic ? -1 : half; }  // the half as a conv cfg
static_assert(num_cfgs(YM_DT_F16) <= 255 && num_cfgs(YM_DT_F32) <= 255 && num_cfgs(YM_DT_X3) <= 255 &&
                  num_cfgs(YM_DT_I8) <= 255 && num_cfgs(YM_DT_F8) <= 255,
              "the split-pair encoding holds 8 bits per half, and 255 is not an id");

// The shape facts dispatch reads (ym_launch_conv fills them from ConvArgs).
struct ConvShape {
  bool dw;      // depthwise-fused 1x1 (ConvArgs::dw_w)
  bool nchw;    // the stem's NCHW source: csrc/ym_stem.hip's, never a conv of this catalogue
  int k, s;
  bool src1, up0;
  bool pair;    // fused pair (ConvArgs::w2), second conv k2 x k2
  int k2;
  bool kpad64;  // Kpad % 64 == 0
  bool q8_ok;   // int8 / fp8 plans: the conv_i8 preconditions (ym_conv_i8_applies)
};
constexpr bool q8(int dtype) { return dtype == YM_DT_I8 || dtype == YM_DT_F8; }
// 1: 1x1 stride 1 (two sources, up-sampled first source; int8 / fp8: one plain source); 3: 3x3 on one plain source
constexpr int conv_kind(int dtype, const ConvShape& s) {
  if (s.nchw) return -1;
  if (s.k == 1 && s.s == 1 && !(q8(dtype) && (s.src1 || s.up0))) return 1;
  if (s.k == 3 && !s.src1 && !s.up0) return 3;
  return -1;
}

enum ShapeClass { SC_SINGLE, SC_PAIR1, SC_PAIR3, SC_DW, SC_COUNT };
constexpr ShapeClass shape_class(int dtype, const ConvShape& s) {
  if (s.dw) return SC_DW;
  if (!s.pair || q8(dtype)) return SC_SINGLE;  // (int8 / fp8 plans have no fused pairs)
  return s.k2 == 3 ? SC_PAIR3 : SC_PAIR1;      // (k2 is 1 or 3: conv_args; the `dma` pair launcher checks k2 == 1)
}

constexpr unsigned bit(Family f) { return 1u << f; }
struct Admit {
  unsigned pinned;    // families whose ids are launched on this shape class (0: the class has no kernel in this dtype)
  unsigned terminal;  // of those: a refusal is returned even when not strict (no fallback behind it)
  unsigned silent;    // ids neither launched nor refused: the fallback, under strict too
  Family fallback;    // first_fit 0: this family's heuristic (local index -1); n: every index of the n families from
  int first_fit;      //   this one on, in id order, until one is not refused
  bool needs_pin;     // strict without an id is refused
};
constexpr unsigned kStreams = bit(F_STREAM) | bit(F_SMALL);
constexpr unsigned kTiles = bit(F_DIRECT) | bit(F_LDS);
constexpr Admit kNoKernel = {0, 0, 0, F_NONE, 0, false};
constexpr Admit kPairF16 = {bit(F_BNECK) | kStreams, 0, 0, F_STREAM, 2, true};
constexpr Admit kDwpw = {bit(F_DWPW), 0, 0, F_DWPW, 0, true};
// [shape class][YM_DT_*: f16, f32, int8, fp8, x3]
constexpr Admit kAdmit[SC_COUNT][5] = {
    /* single */ {{kTiles | bit(F_DMA) | kStreams | bit(F_HALO), kTiles, 0, F_DIRECT, 0, false},
                  {bit(F_DIRECT), bit(F_DIRECT), bit(F_LDS), F_DIRECT, 0, false},
                  {bit(F_I8) | bit(F_I8_STREAM) | bit(F_DMA), bit(F_I8), 0, F_I8, 0, false},
                  {bit(F_I8), bit(F_I8), 0, F_I8, 0, false},  // (and of those the one-K-chain tiles only: kI8OneChain)
                  {kTiles | bit(F_DMA) | kStreams | bit(F_DMA_X3), bit(F_DIRECT), 0, F_DIRECT, 0, false}},
    /* -> 1x1 */ {kPairF16, kNoKernel, kNoKernel, kNoKernel, {bit(F_BNECK) | kStreams | bit(F_DMA), 0, 0, F_STREAM, 2, true}},
    /* -> 3x3 */ {{bit(F_BNECK), 0, 0, F_BNECK, 1, true}, kNoKernel, kNoKernel, kNoKernel,
                  {bit(F_BNECK) | bit(F_BNECK_X3), 0, 0, F_BNECK, 1, true}},
    /* dw+1x1 */ {kDwpw, kNoKernel, kNoKernel, kNoKernel, kDwpw}};

constexpr int kOk = 0, kRefused = 1;  // hipSuccess, hipErrorInvalidValue (csrc/ym_conv.hip asserts it)

// Launches one conv op: `launch(family, local)` runs the family's launcher on index `local` (-1: the family's
// heuristic) and returns its error code.  cfg < 0: no pinned id.  strict (the tuner): an id that does not apply is
// refused rather than replaced.  *taken (may be null): 1 when cfg's own kernel was launched, 0 when a pinned cfg fell
// back, -1 when there is no cfg or the plan is int8 / fp8.
template <typename Launch>
int dispatch_conv(int dtype, const ConvShape& s, int cfg, bool strict, int* taken, Launch&& launch) {
  if (dtype < YM_DT_F16 || dtype > YM_DT_X3) return kRefused;
  const bool tracked = cfg >= 0 && (s.dw || !q8(dtype));
  if (taken) *taken = tracked ? 0 : -1;
  if (!s.dw) {  // (a depthwise-fused op: every check is ym_launch_conv_dwpw's)
    if (conv_kind(dtype, s) < 0) return kRefused;
    if (q8(dtype) ? !s.q8_ok : !s.kpad64) return kRefused;
  }
  const Admit& adm = kAdmit[shape_class(dtype, s)][dtype];
  if (!adm.pinned) return kRefused;
  const Slot id = resolve(dtype, s.dw, cfg);
  unsigned fam = id.family == F_NONE ? 0 : bit(id.family);
  if (dtype == YM_DT_F8 && id.family == F_I8 && !(kI8OneChain >> id.local & 1)) fam = 0;  // one K chain per output
  if (fam & adm.pinned) {
    const int e = launch(id.family, id.local);
    if (e == kOk && tracked && taken) *taken = 1;
    if (e != kRefused || strict || (fam & adm.terminal)) return e;  // refused and not strict: the fallback
  } else if (strict && !(fam & adm.silent) && (cfg >= 0 || adm.needs_pin)) {
    return kRefused;
  }
  if (!adm.first_fit) return launch(adm.fallback, -1);
  for (int f = adm.fallback; f < adm.fallback + adm.first_fit; ++f) {
    for (int i = 0; i < count((Family)f); ++i) {
      const int e = launch((Family)f, i);
      if (e != kRefused) return e;
    }
  }
  return kRefused;
}

}  // namespace ymc
