// Feature embeddings (csrc/ym_embed.hip; driven by ym_embed in ym_runtime.cpp): Ultralytics _predict_once(embed=...) —
// adaptive_avg_pool2d(x, (1, 1)) of the named layers' outputs, concatenated per image.  The pooling stage reads the
// plan's own NHWC storage (fp32, fp16, or the x3 pair layout) behind a forward that stops at the last named layer.
#pragma once
#include "ym_common.h"

constexpr int kEmbedMaxViews = 32;  // layers 0..22 with the four Concat layers as two views each: 27
constexpr int kEmbedThreads = 256;
constexpr int kEmbedCG = 8;         // 8-channel groups per workgroup tile (64 channels)
constexpr int kEmbedPL = kEmbedThreads / kEmbedCG;  // 32 pixel lanes
constexpr int kEmbedIter = 16;      // pixels per thread, at most
constexpr int kEmbedChunk = kEmbedPL * kEmbedIter;  // 512 pixels per workgroup
constexpr int kEmbedFinL = 8;       // chunk lanes of the finishing kernel
constexpr int kEmbedFinC = kEmbedThreads / kEmbedFinL;  // 32 channels per finishing workgroup

enum { YM_EMB_F32 = 0, YM_EMB_F16 = 1, YM_EMB_X3 = 2 };

// One view: channels [coff, coff + C) of an image-major NHWC buffer of `pitch` channels and P pixels per image.
struct EmbedDesc {
  const void* ptr;
  int P, pitch, coff, C;
  int mode;   // YM_EMB_*: fp32 | fp16 | x3 pair chunks ([fp16 hi x8 | fp16 lo x8] per 8 channels)
  int col;    // first output column
  // set by the launcher
  int nch;    // pixel chunks per image: ceil(P / kEmbedChunk)
  int blk0;   // first workgroup of the pooling launch
  int fblk0;  // first workgroup of the finishing launch (views with nch > 1 only)
  int fblk_n;
  long poff;  // the view's chunk partials [B][nch][C] in `part`, in floats
};

struct EmbedArgs {
  EmbedDesc d[kEmbedMaxViews];
  int n, B;
  float* out;  // (B, ld) fp32: the means
  long ld;
  float* part;  // chunk partial sums of the views that span more than one chunk (ym_embed_part_floats)
};

// Floats of `part` a call needs (0 when every view fits one chunk); -1 for an invalid table.
long ym_embed_part_floats(const EmbedArgs& a);
// One pooling launch, plus one finishing launch when some view spans more than one chunk.
hipError_t ym_launch_embed(const EmbedArgs& a, hipStream_t st);
