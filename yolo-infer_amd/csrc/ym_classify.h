// The Classify head (csrc/ym_classify.hip; the `classify` op of a yolo11-cls plan, driven by ym_classify in
// ym_runtime.cpp): Ultralytics Classify — Conv(c1, 1280, 1) -> AdaptiveAvgPool2d(1) -> Linear(1280, nc) -> softmax —
// and the top-5, as three launches behind layer 9.  The 1280-channel map is never stored.
#pragma once
#include "ym_common.h"

constexpr int kClsHidden = 1280;  // Classify's hidden width c_: fixed, not scaled by the model size
constexpr int kClsTopK = 5;       // classes reported per image: min(kClsTopK, nc)
constexpr int kClsThreads = 256;  // every launch: 4 waves
constexpr int kClsKC = 64;        // launch 1: logical K of one LDS stage
constexpr int kClsBN = 64;        // launch 1: output channels of a workgroup
constexpr int kClsBM = 64;        // launch 1: pixels of a workgroup pass (two 32-pixel MFMA tiles)
constexpr int kClsLinCT = 8;      // launch 2: classes of a workgroup (two per wave)
constexpr int kClsLinG = 8;       // launch 2: pooled vectors of an image group in LDS (40 KB)

struct ClsArgs {
  const void* x; int ctot, coff, C1, P;  // layer 9's view: image-major NHWC in the plan's storage, P pixels per image
  const void* w; const float* bias;      // head conv [kClsHidden][kpad] in the plan's operand format, folded-BN bias
  int kpad;                              // K pitch of a weight row in storage elements (x3: fp16 [hi | lo] pairs)
  float wsc;                             // x3: 2^-s of the weights packed as W * 2^s (1 otherwise)
  const void* lw; const float* lb;       // Linear [nc][kClsHidden] (fp32; f16 plans: fp16), fp32 bias
  int nc, B, k;                          // classes, images, min(kClsTopK, nc)
  float* pooled;                         // (B, kClsHidden) means
  float* logits;                         // (B, nc)
  float* probs; long ld;                 // (B, ld >= nc)
  int* topk; float* topk_conf;           // (B, k), best first
};

// The three launches on `st`; hipErrorInvalidValue for arguments the kernels do not take.
hipError_t ym_launch_classify(int dtype, const ClsArgs& a, hipStream_t st);
