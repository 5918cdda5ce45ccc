// OpenCV's INTER_LINEAR coefficient setup for one destination index (oracle/letterbox.py _axis), shared by the
// letterbox kernels: csrc/ym_letterbox.hip (one image, one thread per pixel) and csrc/ym_letterbox_batch.hip (a batch
// of frames, tiled).
#pragma once

__device__ __forceinline__ double opaque_d(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

// source index pair and 11-bit weights of destination index d (oracle/letterbox.py _axis)
__device__ __forceinline__ void axis(int d, int src, double scale, int& s0, int& s1, int& a0, int& a1, bool& edge) {
  float f = (float)(opaque_d((d + 0.5) * scale) - 0.5);  // (double) (d + .5)·scale − .5 in two roundings, to float
  int s = (int)floorf(f);
  f -= (float)s;
  edge = false;
  if (s < 0) { f = 0.f; s = 0; }
  if (s >= src - 1) { f = 0.f; s = src - 1; edge = true; }
  a0 = (int)rintf((1.f - f) * 2048.f);
  a1 = (int)rintf(f * 2048.f);
  s0 = s;
  s1 = s + 1 < src ? s + 1 : src - 1;
}
