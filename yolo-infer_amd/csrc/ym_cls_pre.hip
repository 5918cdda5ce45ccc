// Classify preprocessing: upstream's classify_transforms — torchvision Resize(imgsz) with Pillow's
// antialiased BILINEAR, CenterCrop(imgsz), ToTensor — for a whole batch of differently sized HWC uint8 images already
// on the device, as ONE launch that writes the (B, 3, imgsz, imgsz) fp32 batch ym_classify reads.  The arithmetic is
// Pillow's ImagingResample for 8 bits per channel, bit for bit: per axis a triangle filter widened by the scale factor,
// its weights formed in double, normalised, rounded to 22-bit fixed point; the horizontal pass first (into 8 bits),
// then the vertical pass, each `clip8((2^21 + sum k * v) >> 22)`, and a pass whose size does not change is not run.
//
// Work split: one workgroup of 256 threads per 32 x 32 output tile of one image (imgsz is a multiple of 32: no tails),
// grid (imgsz / 32, imgsz / 32, B).
//   1. The tile's 32 column and 32 row windows (first tap, tap count, weight sum) and then their fixed-point
//      coefficient tables are computed in fp64 straight into LDS: no table is built on the host.
//   2. The source rows the tile's vertical taps span are streamed in chunks of R rows.  A chunk's row segments (the
//      columns the tile's horizontal taps span) go global -> LDS with 16-byte loads, every source byte once per tile.
//   3. The horizontal pass runs out of the staged segments into an 8-bit (R, 32, 3) LDS tile: one thread per
//      (row, column), three channel sums, the coefficient read once for the three.
//   4. The vertical pass adds the chunk's rows into int32 register accumulators: a thread owns column x of rows
//      y, y + 8, y + 16, y + 24 (12 accumulators).  Nothing but the coefficient tables grows with the scale factor, and
//      those are bounded by the launcher (kClsPreMaxScale per axis).
//   5. clip8, BGR -> RGB, /255 and three plane stores, 128 contiguous bytes per row of the tile.
// LDS: 128 * (KH + KV) bytes of coefficients (KH, KV: the batch's largest tap counts, at most 129 each), 1 KiB of
// windows, a 3 KiB intermediate tile and a 24 KiB stage: 29 KiB at the usual scales, 60.3 KiB at the bound.
#include "ym_common.h"

#pragma clang fp contract(off)  // Pillow's doubles are separate multiplies and adds

namespace {

constexpr int kT = 32;                 // output tile edge
constexpr int kThreads = 256;
constexpr int kStageBytes = 24576;     // staged source row segments of one chunk
constexpr int kInterStride = kT * 3;   // one row of the 8-bit intermediate tile
constexpr int kMaxTaps = 2 * kClsPreMaxScale + 1;

__device__ __forceinline__ double opaque_d(double x) {
  asm volatile("" : "+v"(x));
  return x;
}

struct Axis {
  double scale, support, ss;  // in / out; max(scale, 1) (the bilinear filter's support is 1); 1 / support
  int in;
};

__device__ __forceinline__ Axis make_axis(int in, int out) {
  Axis a;
  a.in = in;
  a.scale = (double)in / (double)out;
  a.support = a.scale < 1.0 ? 1.0 : a.scale;
  a.ss = 1.0 / a.support;
  return a;
}

__device__ __forceinline__ double axis_center(const Axis& a, int xx) { return opaque_d((xx + 0.5) * a.scale); }

// precompute_coeffs' window of output index xx: first source index and tap count
__device__ __forceinline__ void axis_window(const Axis& a, double center, int& mn, int& n) {
  int lo = (int)(center - a.support + 0.5);
  int hi = (int)(center + a.support + 0.5);
  if (lo < 0) lo = 0;
  if (hi > a.in) hi = a.in;
  mn = lo;
  n = hi - lo;
}

// bilinear_filter((x + xmin - center + 0.5) * ss)
__device__ __forceinline__ double axis_weight(const Axis& a, double center, int mn, int x) {
  double t = opaque_d((x + mn - center + 0.5) * a.ss);
  if (t < 0.0) t = -t;
  return t < 1.0 ? 1.0 - t : 0.0;
}

__device__ __forceinline__ int clip8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

__global__ __launch_bounds__(kThreads) void cls_pre_u8(const ClsPreArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
  int* kh = reinterpret_cast<int*>(lds);  // (32, KH) horizontal coefficients, then (32, KV) vertical
  int* kv = kh + kT * a.KH;
  int* hmin = kv + kT * a.KV;             // windows: first tap and tap count of the tile's columns and rows
  int* hcnt = hmin + kT;
  int* vmin = hcnt + kT;
  int* vcnt = vmin + kT;
  double* hww = reinterpret_cast<double*>(vcnt + kT);  // weight sums
  double* vww = hww + kT;
  unsigned char* inter = reinterpret_cast<unsigned char*>(vww + kT);  // (<= 32, 32, 3) horizontally resized rows
  unsigned char* stage = inter + kT * kInterStride;                   // (R, sstride) staged source row segments

  const ym_cls_pre_desc d = a.desc[blockIdx.z];
  const int tid = threadIdx.x;
  const int X0 = d.left + blockIdx.x * kT, Y0 = d.top + blockIdx.y * kT;  // the tile in resized coordinates
  const bool hp = d.rw != d.w, vp = d.rh != d.h;
  const Axis ax = make_axis(d.w, d.rw), ay = make_axis(d.h, d.rh);

  // 1a. windows and weight sums: threads 0..31 the columns, 32..63 the rows.  A skipped pass reads source index = output
  // index, as one "tap" that the passes below copy instead of weighting.
  if (tid < 2 * kT) {
    const bool v = tid >= kT;
    const int i = tid & (kT - 1), o = (v ? Y0 : X0) + i;
    int mn = o, n = 1;
    double ww = 0.0;
    if (v ? vp : hp) {
      const Axis s = v ? ay : ax;
      const double c = axis_center(s, o);
      axis_window(s, c, mn, n);
      n = min(n, v ? a.KV : a.KH);  // (never binds: a window holds at most 2 * ceil(support) + 1 taps)
      for (int x = 0; x < n; ++x) ww += axis_weight(s, c, mn, x);
    }
    (v ? vmin : hmin)[i] = mn;
    (v ? vcnt : hcnt)[i] = n;
    (v ? vww : hww)[i] = ww;
  }
  __syncthreads();
  // 1b. the coefficients: w / ww in double, then normalize_coeffs_8bpc's rounding to 22 bits
  for (int idx = tid; idx < kT * (a.KH + a.KV); idx += kThreads) {
    const bool v = idx >= kT * a.KH;
    const int j = v ? idx - kT * a.KH : idx, K = v ? a.KV : a.KH;
    const int i = j / K, x = j - i * K;
    if (!(v ? vp : hp) || x >= (v ? vcnt : hcnt)[i]) continue;
    const Axis s = v ? ay : ax;
    const double c = axis_center(s, (v ? Y0 : X0) + i);
    double w = axis_weight(s, c, (v ? vmin : hmin)[i], x);
    const double ww = (v ? vww : hww)[i];
    if (ww != 0.0) w /= ww;
    (v ? kv : kh)[j] = w < 0.0 ? (int)(-0.5 + w * 4194304.0) : (int)(0.5 + w * 4194304.0);
  }
  __syncthreads();

  // windows are monotone in the output index: the tile's source span is first window's start .. last window's end
  const int sx_lo = hmin[0], sx_hi = hmin[kT - 1] + hcnt[kT - 1];
  const int r_lo = vmin[0], r_hi = vmin[kT - 1] + vcnt[kT - 1];
  const int seg = (sx_hi - sx_lo) * 3;        // bytes of one row segment
  const int sstride = (seg + 30) / 16 * 16;   // + up to 15 bytes in front (16-byte aligned loads), rounded up
  const int wpr = sstride / 16;               // 16-byte words per staged row
  const int R = min(kStageBytes / sstride, kT);
  if (R < 1) return;  // (the launcher's scale bound keeps a segment within the stage)
  const unsigned char* img = a.images + d.off;
  const unsigned char* img_end = img + (size_t)(d.h - 1) * d.row_bytes + (size_t)3 * d.w;
  const int x = tid & (kT - 1), yb = tid >> 5;
  int acc[4][3];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int c = 0; c < 3; ++c) acc[j][c] = vp ? 1 << 21 : 0;

  for (int c0 = r_lo; c0 < r_hi; c0 += R) {
    const int nr = min(R, r_hi - c0);
    // 2. stage: aligned 16-byte loads; the image starts 16-byte aligned, so a word never starts in front of it, and a
    // word that would cross the image's last byte is read byte by byte
    for (int i = tid; i < nr * wpr; i += kThreads) {
      const int rl = i / wpr, wd = i - rl * wpr;
      const unsigned char* p = img + (size_t)(c0 + rl) * d.row_bytes + (size_t)sx_lo * 3;
      const unsigned char* q = p - (reinterpret_cast<uintptr_t>(p) & 15) + wd * 16;
      if (q >= p + seg) continue;
      uint4 w4 = make_uint4(0, 0, 0, 0);
      if (q + 16 <= img_end) {
        w4 = *reinterpret_cast<const uint4*>(q);
      } else {
        unsigned int t[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b)
          if (q + b < img_end) t[b >> 2] |= (unsigned int)q[b] << (8 * (b & 3));
        w4 = make_uint4(t[0], t[1], t[2], t[3]);
      }
      *reinterpret_cast<uint4*>(stage + rl * sstride + wd * 16) = w4;
    }
    __syncthreads();
    // 3. horizontal pass: (row, column) per thread, three channel sums
    if (hp) {
      for (int i = tid; i < nr * kT; i += kThreads) {
        const int rl = i >> 5, c = i & (kT - 1);
        const size_t g = (size_t)(c0 + rl) * d.row_bytes + (size_t)sx_lo * 3;
        const int slack = (int)(reinterpret_cast<uintptr_t>(img + g) & 15);
        const unsigned char* s = stage + rl * sstride + slack + (hmin[c] - sx_lo) * 3;
        const int* k = kh + c * a.KH;
        const int n = hcnt[c];
        int s0 = 1 << 21, s1 = 1 << 21, s2 = 1 << 21;
        for (int t = 0; t < n; ++t) {
          const int kk = k[t];
          s0 += kk * s[3 * t];
          s1 += kk * s[3 * t + 1];
          s2 += kk * s[3 * t + 2];
        }
        unsigned char* o = inter + rl * kInterStride + c * 3;
        o[0] = (unsigned char)clip8(s0 >> 22);
        o[1] = (unsigned char)clip8(s1 >> 22);
        o[2] = (unsigned char)clip8(s2 >> 22);
      }
      __syncthreads();
    }
    // 4. vertical pass over the chunk's rows (a skipped vertical pass: the row itself)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int y = yb + 8 * j;
      const int lo = max(vmin[y], c0), hi = min(vmin[y] + vcnt[y], c0 + nr);
      for (int r = lo; r < hi; ++r) {
        const int rl = r - c0;
        const unsigned char* s;
        if (hp) {
          s = inter + rl * kInterStride + x * 3;
        } else {  // no horizontal pass: the staged segment starts at the tile's first column
          const size_t g = (size_t)r * d.row_bytes + (size_t)sx_lo * 3;
          s = stage + rl * sstride + (int)(reinterpret_cast<uintptr_t>(img + g) & 15) + x * 3;
        }
        const int kk = vp ? kv[y * a.KV + r - vmin[y]] : 1;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j][c] += kk * s[c];
      }
    }
    __syncthreads();
  }

  // 5. RGB planes (BGR sources flipped, as upstream's im[..., ::-1]), /255 as ToTensor
  const size_t plane = (size_t)a.imgsz * a.imgsz;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float* out = a.dst + (size_t)blockIdx.z * 3 * plane + (size_t)(blockIdx.y * kT + yb + 8 * j) * a.imgsz +
                 blockIdx.x * kT + x;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int v = d.bgr ? acc[j][2 - c] : acc[j][c];
      out[c * plane] = (float)(vp ? clip8(v >> 22) : v) / 255.f;
    }
  }
}

}  // namespace

int ym_cls_pre_taps(int in, int out) {
  const double scale = (double)in / (double)out;
  return 2 * (int)ceil(scale < 1.0 ? 1.0 : scale) + 1;
}

hipError_t ym_launch_cls_pre(const ClsPreArgs& a, hipStream_t st) {
  if (!a.images || !a.desc || !a.dst || (reinterpret_cast<uintptr_t>(a.images) & 15) || a.B < 1 || a.B > 65535 ||
      a.imgsz < kT || a.imgsz % kT || a.KH < 3 || a.KV < 3 || a.KH > kMaxTaps || a.KV > kMaxTaps)
    return hipErrorInvalidValue;
  const size_t lds = (size_t)kT * (a.KH + a.KV) * sizeof(int) + 4 * kT * sizeof(int) + 2 * kT * sizeof(double) +
                     kT * kInterStride + kStageBytes;
  hipLaunchKernelGGL(cls_pre_u8, dim3(a.imgsz / kT, a.imgsz / kT, a.B), dim3(kThreads), lds, st, a);
  return hipGetLastError();
}
