// Instance polygons of mask planes (Masks.xy): three launches per call, one workgroup per mask in the
// first and the last.
//
//   select   pack the byte plane into a bit plane (LDS when it fits kContourLdsWords, else the context's scratch), find
//            the candidates word-parallel (32 pixels per thread and step), and let every thread take its candidates
//            through csrc/ym_contour.h's rules in ym_ct_select_serial's order: walk every candidate's cycle and keep
//            the largest key among the outer borders (an LDS atomic max); that border alone answers the top-level
//            question; only when it lies inside another component does every candidate go through the whole rule
//   offsets  one workgroup: the exclusive prefix sum of the n kept-point counts, n + 1 int64 words
//   emit     per mask whose points fit the caller's capacity: pack the rows the chosen border spans again (the scratch
//            copy is reused when the plane did not fit LDS) and walk it once more, one lane writing the kept points
//
// Why a walk and not pointer doubling: a step is three LDS reads and a dozen integer operations on a 3 x 3 code, the
// chosen border of a 640 x 640 instance mask is a few thousand steps, and the masks of a batch run side by side, two
// workgroups a CU.  The walks of one mask spread over the lanes by candidate; the raster scan, which is what a
// sequential tracer spends its time on, is the word-parallel part.  The cost that remains is quadratic only for planes
// of many nested or side-by-side components that all beat the running best, which the key test cuts short.
#include <hip/hip_runtime.h>

#include "ym_contour.h"

namespace {

struct CtArgs {
  const unsigned char* masks;
  long long plane_stride;
  int n, H, W;
  uint32_t* gbits;  // per mask ym_ct_words(H, W) words, or null: the bit plane fits LDS
  CtSel* sel;
  int* points;
  long long cap;
  long long* offsets;
};

// Rows py0 .. py1 of the bit plane (all of it: 0 .. H + 1).  16 aligned bytes at a time when the plane allows.
__device__ void pack_rows(uint32_t* bits, const unsigned char* src, int H, int W, int py0, int py1) {
  const int wpr = ym_ct_wpr(W);
  const bool vec = (W & 15) == 0 && (reinterpret_cast<uintptr_t>(src) & 15) == 0;
  const int total = (py1 - py0 + 1) * wpr;
  for (int i = threadIdx.x; i < total; i += kContourThreads) {
    const int py = py0 + i / wpr, w = i % wpr;
    uint32_t v = 0u;
    if (vec && py >= 1 && py <= H && w >= 1 && 32 * (w - 1) < W) {
      const unsigned char* at = src + (long long)(py - 1) * W + 32 * (w - 1);
      const int chunks = 32 * w <= W ? 2 : 1;  // W is a multiple of 16: a word holds 32 or 16 pixels
      for (int c = 0; c < chunks; ++c) {
        const uint4 q = *reinterpret_cast<const uint4*>(at + 16 * c);
        const uint32_t d[4] = {q.x, q.y, q.z, q.w};
        for (int k = 0; k < 4; ++k)
          for (int b = 0; b < 4; ++b)
            if ((d[k] >> (8 * b)) & 0xffu) v |= 1u << (16 * c + 4 * k + b);
      }
    } else {
      v = ym_ct_pack_word(src, H, W, py, w);
    }
    bits[(long long)py * wpr + w] = v;
  }
}

// One mask's selection over its bit plane.  Inlined once with the LDS array and once with the scratch plane, so each copy
// knows its address space (LDS reads, not flat ones, on the path every walk step takes).
__device__ __forceinline__ void select_mask(uint32_t* bits, const CtArgs& a, int m, unsigned long long* best, int* best_ymax) {
  const int tid = threadIdx.x;
  const int H = a.H, W = a.W, wpr = ym_ct_wpr(W);
  pack_rows(bits, a.masks + (long long)m * a.plane_stride, H, W, 0, H + 1);
  __syncthreads();
  const CtPlane p{bits, wpr, H, W};
  const int inner = wpr - 2, total = H * inner;
  uint64_t mine = 0;
  int mine_ymax = 0;
  // 1. the largest key over every border that is an outer one (ym_ct_select_serial's order, spread over the lanes)
  for (int i = tid; i < total; i += kContourThreads) {
    const int py = 1 + i / inner, w = 1 + i % inner;
    for (uint32_t cand = ym_ct_candidates(p, py, w); cand; cand &= cand - 1u) {
      int ymax;
      const uint64_t key = ym_ct_valid_key(p, 32 * (w - 1) + __builtin_ctz(cand), py - 1, ymax);
      if (key > mine) {
        mine = key;
        mine_ymax = ymax;
      }
    }
  }
  if (mine) atomicMax(best, (unsigned long long)mine);
  __syncthreads();
  // 2. its owner (keys are distinct: one thread) asks whether it is top-level
  if (mine != 0 && mine == *best) {
    const int start = (int)(uint32_t)mine;
    *best_ymax = ym_ct_top_level(p, start % W, start / W) ? mine_ymax : -1;
  }
  __syncthreads();
  if (*best == 0ull || *best_ymax >= 0) {
    if (tid == 0) {
      CtSel s{};
      s.count = (uint32_t)(*best >> 32);
      s.start = s.count ? (int)(uint32_t)*best : -1;
      s.ymax = *best_ymax;
      a.sel[m] = s;
    }
    return;
  }
  // 3. the largest border lies inside another component: every candidate, with the running best
  __syncthreads();
  if (tid == 0) *best = 0ull;
  __syncthreads();
  mine = 0;
  for (int i = tid; i < total; i += kContourThreads) {
    const int py = 1 + i / inner, w = 1 + i % inner;
    for (uint32_t cand = ym_ct_candidates(p, py, w); cand; cand &= cand - 1u) {
      int ymax;
      const uint64_t floor_key = *reinterpret_cast<volatile unsigned long long*>(best);
      const uint64_t key = ym_ct_eval(p, 32 * (w - 1) + __builtin_ctz(cand), py - 1, floor_key > mine ? floor_key : mine, ymax);
      if (key) {
        mine = key;
        mine_ymax = ymax;
        atomicMax(best, (unsigned long long)key);
      }
    }
  }
  __syncthreads();
  if (mine != 0 && mine == *best) *best_ymax = mine_ymax;  // keys are distinct: one thread
  __syncthreads();
  if (tid == 0) {
    CtSel s{};
    s.count = (uint32_t)(*best >> 32);
    s.start = s.count ? (int)(uint32_t)*best : -1;
    s.ymax = *best_ymax;
    a.sel[m] = s;
  }
}

__global__ __launch_bounds__(kContourThreads) void ct_select(const CtArgs a) {
  __shared__ uint32_t lds[kContourLdsWords];
  __shared__ unsigned long long best;
  __shared__ int best_ymax;
  const int m = blockIdx.x;
  if (threadIdx.x == 0) {
    best = 0ull;
    best_ymax = 0;
  }
  if (a.gbits)
    select_mask(a.gbits + (long long)m * ym_ct_words(a.H, a.W), a, m, &best, &best_ymax);
  else
    select_mask(lds, a, m, &best, &best_ymax);
}

constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kScanThreads) void ct_offsets(const CtArgs a) {
  __shared__ long long part[kScanThreads];
  __shared__ long long base;
  const int tid = threadIdx.x;
  if (tid == 0) {
    base = 0;
    a.offsets[0] = 0;
  }
  __syncthreads();
  for (int c = 0; c < a.n; c += kScanThreads) {
    const int i = c + tid;
    part[tid] = i < a.n ? (long long)a.sel[i].count : 0;
    __syncthreads();
    for (int off = 1; off < kScanThreads; off <<= 1) {
      const long long v = tid >= off ? part[tid - off] : 0;
      __syncthreads();
      part[tid] += v;
      __syncthreads();
    }
    if (i < a.n) a.offsets[i + 1] = base + part[tid];
    __syncthreads();
    if (tid == 0) base += part[kScanThreads - 1];
    __syncthreads();
  }
}

// The chosen border once more, one lane storing its kept points.
__device__ __forceinline__ void emit_mask(const uint32_t* bits, const CtArgs& a, const CtSel& s, long long at) {
  const CtPlane p{bits, ym_ct_wpr(a.W), a.H, a.W};
  int* out = a.points + 2 * at;
  const long long room = s.count;
  long long k = 0;
  uint32_t count;
  int ymax;
  ym_ct_outer(p, s.start % a.W, s.start / a.W, count, ymax, [&](int x, int y) {
    if (k < room) {  // (the same walk as ct_select's gives the same count: the bound only keeps a store in range)
      out[2 * k] = x;
      out[2 * k + 1] = y;
    }
    ++k;
  });
}

__global__ __launch_bounds__(kContourThreads) void ct_emit(const CtArgs a) {
  __shared__ uint32_t lds[kContourLdsWords];
  const int m = blockIdx.x;
  const CtSel s = a.sel[m];
  const long long at = a.offsets[m];
  if (s.count == 0 || at + (long long)s.count > a.cap) return;  // the caller sees offsets[n] > cap and calls again
  if (a.gbits) {
    if (threadIdx.x == 0) emit_mask(a.gbits + (long long)m * ym_ct_words(a.H, a.W), a, s, at);  // as ct_select left it
    return;
  }
  const int cy = s.start / a.W;
  pack_rows(lds, a.masks + (long long)m * a.plane_stride, a.H, a.W, cy, s.ymax + 2);  // pixel rows cy - 1 .. ymax + 1
  __syncthreads();
  if (threadIdx.x == 0) emit_mask(lds, a, s, at);
}

}  // namespace

// a.gbits: null when ym_ct_words(H, W) <= kContourLdsWords, else the scratch planes.
hipError_t ym_launch_contours(const unsigned char* masks, long long plane_stride, int n, int H, int W, uint32_t* gbits,
                              CtSel* sel, int* points, long long cap, long long* offsets, hipStream_t st) {
  CtArgs a{masks, plane_stride, n, H, W, gbits, sel, points, cap, offsets};
  if (n > 0) hipLaunchKernelGGL(ct_select, dim3(n), dim3(kContourThreads), 0, st, a);
  hipLaunchKernelGGL(ct_offsets, dim3(1), dim3(kScanThreads), 0, st, a);
  if (n > 0 && cap > 0) hipLaunchKernelGGL(ct_emit, dim3(n), dim3(kContourThreads), 0, st, a);
  return hipGetLastError();
}
