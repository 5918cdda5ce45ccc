// Anchor-free DFL decode and the candidate stage of NMS on gfx950 (Detect._inference).
#include <stdlib.h>

#include "ym_common.h"

namespace {

// ------------------------------------------------------------------------------------------------- decode
// Detect._inference + the candidate stage of non_max_suppression; 4 lanes per anchor (lane s: DFL side s and a
// quarter of the classes):
//   DFL softmax over reg_max bins → ltrb distances → dist2bbox(xywh) · stride → xywh2xyxy;
//   sigmoid class scores → (max, first argmax); candidate iff max > conf (and class in the filter).
// Candidates are appended to a per-image key list: key = score bits << 32 | ~anchor, so a descending sort gives
// score-descending order with ties broken by ascending anchor index (torchvision's stable sort).
// DIRECT (reg_max 16, nc 80: the YOLO11 heads): no LDS staging — lane s of an anchor loads its 16 DFL bins and its
// 20 class logits straight into registers (4 + 5 float4; the 4 lanes of an anchor cover its 576-byte row, so a wave's
// loads are 9.2 KB contiguous), no barrier before the math, and a small LDS footprint (more workgroups in flight).
// Same per-element arithmetic in the same order as the staged variant.
template <bool DIRECT>
__global__ __launch_bounds__(256) void decode_anchors(const DecodeArgs a) {
  float dist, best;
  int bi, b, ai, sub;
  long idx;
  bool valid;
  const long total = (long)a.B * a.A;
  const long a0 = blockIdx.x * 64L;
  if constexpr (DIRECT) {
    const long gidx = a0 + (threadIdx.x >> 2);
    sub = threadIdx.x & 3;
    valid = gidx < total;
    idx = valid ? gidx : 0;
    b = idx / a.A;
    ai = idx - (long)b * a.A;
    const f32x4* row = reinterpret_cast<const f32x4*>(a.anchors + idx * a.no_tot);
    f32x4 bv[4], cv[5];
#pragma unroll
    for (int i = 0; i < 4; ++i) bv[i] = row[4 * sub + i];
#pragma unroll
    for (int i = 0; i < 5; ++i) cv[i] = row[16 + 5 * sub + i];
    float mx = -INFINITY;
#pragma unroll
    for (int i = 0; i < 16; ++i) mx = fmaxf(mx, bv[i >> 2][i & 3]);
    float den = 0.f, num = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const float e = expf(bv[i >> 2][i & 3] - mx);
      den += e;
      num = fmaf(e, (float)i, num);
    }
    dist = num / den;
    float lmax = -INFINITY;
#pragma unroll
    for (int c = 0; c < 20; ++c) lmax = fmaxf(lmax, cv[c >> 2][c & 3]);
    const float lthr = lmax < 10.0f ? lmax - 0.5f : -INFINITY;
    best = -INFINITY;
    bi = 0x7FFFFFFF;
#pragma unroll
    for (int c = 0; c < 20; ++c) {
      const float l = cv[c >> 2][c & 3];
      if (!(l >= lthr)) continue;
      const float sc = ym_sigmoid(l);
      if (sc > best) { best = sc; bi = 20 * sub + c; }
    }
  } else {
    // the workgroup's 64 anchor rows are contiguous: stage them in LDS with coalesced 16-byte loads
    extern __shared__ float rows[];  // [64][no_tot + 1]
    const int nrow = total - a0 < 64 ? (int)(total - a0) : 64;
    // LDS rows are padded to an odd pitch (no_tot + 1 floats): the 16 anchors x 4 sides of a wave read 16-float
    // strided bins, which on a 144-float pitch fell into two banks (32-way conflicts)
    const int ldr = a.no_tot + 1;
    {  // every load in flight before the first LDS store (no_tot <= 192: at most 12 per thread)
      const f32x4* src = reinterpret_cast<const f32x4*>(a.anchors + a0 * a.no_tot);
      const int n4 = nrow * a.no_tot / 4, r4 = a.no_tot / 4;
      f32x4 v[12];
#pragma unroll
      for (int it = 0; it < 12; ++it) {
        const int i = threadIdx.x + 256 * it;
        if (i < n4) v[it] = src[i];
      }
#pragma unroll
      for (int it = 0; it < 12; ++it) {
        const int i = threadIdx.x + 256 * it;
        if (i < n4) {
          const int rr = i / r4, cc = 4 * (i - rr * r4);
          float* d = rows + rr * ldr + cc;
          d[0] = v[it][0]; d[1] = v[it][1]; d[2] = v[it][2]; d[3] = v[it][3];
        }
      }
    }
    __syncthreads();
    const long gidx = a0 + (threadIdx.x >> 2);
    sub = threadIdx.x & 3;
    valid = gidx < total;
    idx = valid ? gidx : 0;
    b = idx / a.A;
    ai = idx - (long)b * a.A;
    const float* row = rows + (valid ? (threadIdx.x >> 2) : 0) * ldr;
    {  // DFL: softmax over the bins, expectation of the bin index (one exp per bin, one division)
      const float* r = row + sub * a.reg_max;
      float mx = -INFINITY;
      for (int i = 0; i < a.reg_max; ++i) mx = fmaxf(mx, r[i]);
      float den = 0.f, num = 0.f;
      for (int i = 0; i < a.reg_max; ++i) {
        const float e = expf(r[i] - mx);
        den += e;
        num = fmaf(e, (float)i, num);
      }
      dist = num / den;
    }
    // class score = max sigmoid, first index on ties (torch max).  Sigmoid is monotonic, so only logits near the
    // quarter's max can reach its value: those within 0.5 of it while it is < 10 (there sigmoid' > 4e-5, so a logit
    // 0.5 lower is many ulps lower), every logit otherwise (saturation).
    const int q = (a.nc + 3) / 4;
    const float* cl = row + 4 * a.reg_max;
    const int c0 = sub * q, c1 = (sub + 1) * q < a.nc ? (sub + 1) * q : a.nc;
    float lmax = -INFINITY;
    for (int c = c0; c < c1; ++c) lmax = fmaxf(lmax, cl[c]);
    const float lthr = lmax < 10.0f ? lmax - 0.5f : -INFINITY;
    best = -INFINITY;
    bi = 0x7FFFFFFF;
    for (int c = c0; c < c1; ++c) {
      if (!(cl[c] >= lthr)) continue;
      const float sc = ym_sigmoid(cl[c]);
      if (sc > best) { best = sc; bi = c; }
    }
  }
#pragma unroll
  for (int o = 1; o < 4; o <<= 1) {
    const float ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  const int base = threadIdx.x & 60;
  const float d0 = __shfl(dist, base), d1 = __shfl(dist, base + 1), d2 = __shfl(dist, base + 2),
              d3 = __shfl(dist, base + 3);
  // candidates are appended per workgroup: LDS slots first, then ONE global atomic per (workgroup, image) — the 64
  // anchors of a workgroup span at most 5 images (A >= 21).  (Per-candidate atomics on the B per-image counters serialised:
  // thousands of same-address atomics at ~90 per µs.)
  __shared__ int wg_cnt[8], wg_base[8];
  if (threadIdx.x < 8) wg_cnt[threadIdx.x] = 0;
  __syncthreads();
  const int b_first = (int)(a0 / a.A);
  bool cand = false;
  int slot = 0;
  unsigned long long key = 0;
  if (sub == 0 && valid) {
    int l = 0;
    while (l + 1 < a.nl && ai >= a.lvl_off[l + 1]) ++l;
    const int p = ai - a.lvl_off[l];
    const float ax = (float)(p % a.lvl_W[l]) + 0.5f;
    const float ay = (float)(p / a.lvl_W[l]) + 0.5f;
    const float st = a.lvl_stride[l];
    const float x1 = ax - d0, y1 = ay - d1;
    const float x2 = ax + d2, y2 = ay + d3;
    const float cx = (x1 + x2) / 2.0f * st, cy = (y1 + y2) / 2.0f * st;
    const float w = (x2 - x1) * st, hh = (y2 - y1) * st;
    const float hw = w / 2.0f, hh2 = hh / 2.0f;
    a.boxes[idx] = make_float4(cx - hw, cy - hh2, cx + hw, cy + hh2);
    a.scores[idx] = best;
    a.cls[idx] = bi;
    cand = best > a.conf;
    if (cand && a.has_classes) cand = (a.classes[bi >> 5] >> (bi & 31)) & 1u;
    if (cand) {
      slot = atomicAdd(&wg_cnt[b - b_first], 1);
      key = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)ai);
  }
  }
  __syncthreads();
  if (threadIdx.x < 8 && wg_cnt[threadIdx.x] > 0)
    wg_base[threadIdx.x] = atomicAdd(&a.counts[b_first + threadIdx.x], wg_cnt[threadIdx.x]);
  __syncthreads();
  if (cand) a.keys[(size_t)b * a.kstride + wg_base[b - b_first] + slot] = key;
}

}  // namespace

// ------------------------------------------------------------------------------------------------- launchers
hipError_t ym_launch_decode(const DecodeArgs& a, hipStream_t st) {
  const long total = (long)a.B * a.A;
  if (a.no_tot % 4) return hipErrorInvalidValue;
  // YM_DECODE_STAGED=1 forces the general LDS-staged variant (tests: both variants agree bit for bit)
  static const bool staged = [] {
    const char* e = getenv("YM_DECODE_STAGED");
    return e && *e == '1';
  }();
  if (a.reg_max == 16 && a.nc == 80 && !staged) {
    hipLaunchKernelGGL(decode_anchors<true>, dim3((total + 63) / 64), dim3(256), 0, st, a);
    return hipGetLastError();
  }
  hipLaunchKernelGGL(decode_anchors<false>, dim3((total + 63) / 64), dim3(256), (size_t)64 * (a.no_tot + 1) * sizeof(float), st,
                     a);
  return hipGetLastError();
}
