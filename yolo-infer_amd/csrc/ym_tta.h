// Test-time augmentation (csrc/ym_tta.hip; driven by ym_tta_scale / ym_tta_forward / ym_tta_nms in ym_runtime.cpp):
// Ultralytics DetectionModel._predict_augment — three passes at scales (1, 0.83, 0.67), the middle one mirrored, their
// decoded heads de-scaled, de-flipped, clipped (_clip_augmented) and concatenated in front of ONE NMS.
#pragma once
#include "ym_common.h"

constexpr int kTtaPasses = 3;
constexpr double kTtaRatio[kTtaPasses] = {1.0, 0.83, 0.67};  // (de-scale divisors: their float32 values)
constexpr int kTtaFlip[kTtaPasses] = {0, 1, 0};              // 1: the W axis is mirrored
constexpr float kTtaPad = 0.447f;                            // scale_img's pad value
constexpr int kTtaGrid = 32;                                 // scale_img's gs

// Pass geometry (scale_img): content int(H s) x int(W s) in Python float arithmetic, padded right and bottom to
// ceil(H s / 32) * 32 x ceil(W s / 32) * 32; ratio 1 returns the input unchanged.
inline void ym_tta_pass_shape(int H, int W, int pass, int& Hs, int& Ws, int& hc, int& wc) {
  if (pass == 0) { Hs = hc = H; Ws = wc = W; return; }
  const double s = kTtaRatio[pass];
  hc = (int)(H * s);
  wc = (int)(W * s);
  Hs = (int)ceil(H * s / kTtaGrid) * kTtaGrid;
  Ws = (int)ceil(W * s / kTtaGrid) * kTtaGrid;
}

// One pass's scaled view of the caller's batch ...
struct TtaScaleArgs {
  const float* in; int B, H, W;  // (B, 3, H, W) fp32, as the caller handed it in (before LoadTensor's /255 rule)
  float* out; int Hs, Ws;        // (B, 3, Hs, Ws) fp32, normalised
  int hc, wc;                    // resized content; the rest of Hs x Ws holds kTtaPad
  int flip;
  const float* batch_max;        // one float: the batch max LoadTensor's rule reads
  float eps;
};

// ... and the merge of the three passes' decoded anchors into one candidate set in the NMS launchers' layout.
struct TtaPass {
  const float* anchors;                                      // (B, A, no_tot) fp32 head rows
  const float4* boxes; const float* scores; const int* cls;  // decode_anchors' outputs (B, A)
  int A, first, keep, base;  // anchors [first, first + keep) survive the clip as merged [base, base + keep)
  int lvl_W[4], lvl_off[4];
  float s; int flip;         // de-scale divisor, mirrored pass
};
struct TtaMergeArgs {
  TtaPass p[kTtaPasses];
  int no_tot, nc, reg_max, nl; float lvl_stride[4];
  float4* boxes; float* scores; int* cls;  // merged (B, Am)
  unsigned long long* keys; int* counts;   // single-label: candidate keys (B, kstride), counts (B), zeroed before
  float* rows;                             // multi-label: merged class-logit rows (B, Am, nc); null: single-label
  int Am, kstride, B;
  float conf; int has_classes; unsigned int classes[4];
  float img_w;                             // the full-size W the mirrored pass is flipped back in
  FDiv div_nc;                             // set by the launcher
};

hipError_t ym_launch_tta_scale(const TtaScaleArgs& a, hipStream_t st);
hipError_t ym_launch_tta_merge(const TtaMergeArgs& a, hipStream_t st);
