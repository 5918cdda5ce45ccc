// Frame-batch preprocessing: Ultralytics `LetterBox` + `BasePredictor.preprocess` for a whole batch of HWC
// uint8 frames that are already in device memory, as ONE launch that writes the fp32 NCHW batch ym_infer reads.  The
// arithmetic is letterbox_u8's (csrc/ym_letterbox.hip, oracle/letterbox.py) bit for bit: OpenCV's 8-bit INTER_LINEAR
// with 11-bit weights, horizontal sums S = p0·a0 + p1·a1, then (S0·b0 + S1·b1 + 2^21) >> 22, the 114 border, BGR→RGB
// and /255.  (The edge rule S = p0·2048 needs no case of its own here: at a clamped index axis() gives a0 = 2048,
// a1 = 0 and s1 = s0, so p0·a0 + p1·a1 is that value.)
//
// Work split: one workgroup of 256 threads per 64 x 16 output tile of one frame, grid (ceil(Wn / 64), ceil(Hn / 16), B);
// frame blockIdx.z's row of the descriptor table says where its pixels are and where its window lies in the canvas, so
// frames of different sizes share the launch.
//   0. A tile that misses the frame's window writes the border and touches no source byte; a tile of a frame that is
//      not resized (uh == h, uw == w) copies its pixels with no pass at all.
//   1. The first wave computes the tile's axis tables into LDS, once: per tile column (s0, s1, a0 | a1 << 16), per tile
//      row the same.  No pixel recomputes them; both index sequences are monotone, so the tile's source span is the
//      first entry's s0 .. the last entry's s1.
//   2. The vertical pass of 16 output rows reads at most 32 source rows, whatever the scale: the span itself when it has
//      at most 32 rows (upscales and reductions below 2), else the pair (s0, s1) of every output row.  Only these rows
//      are fetched.
//   3. Staging: the rows' byte span sx_lo·3 .. sx_hi·3 + 2 goes global → LDS with 16-byte loads, each row's first load
//      aligned down to 16 bytes (row_bytes and the base pointer are arbitrary; a word that would reach in front of the
//      frame's first byte or behind its last is read byte by byte instead).  The stage holds 16 KiB, so the rows go in
//      chunks of 16384 / pitch.  A span whose padded pitch exceeds 2 KiB (64 output columns reading more than ~670
//      source columns: a horizontal reduction beyond about 10) is not staged: its horizontal pass gathers its two
//      pixels per column from global memory, for the <= 32 needed rows only.
//   4. Horizontal pass, LDS → LDS: one thread per (needed row, tile column), three channel sums as int32 into
//      S[row][channel][column].
//   5. Vertical pass: a thread owns four consecutive pixels of one tile row; per channel two 16-byte LDS reads of S,
//      the rounding shift, the clamp, /255, and one 16-byte store per plane (Wn is a multiple of 4 and d_dst 16-byte
//      aligned: the launcher checks both).
// LDS: 24 KiB of S, the 16 KiB stage, 0.9 KiB of tables: 41 KiB, three workgroups per CU.
#include "ym_common.h"
#include "ym_letterbox_axis.h"

namespace {

constexpr int kTW = 64, kTH = 16;     // output tile
constexpr int kThreads = 256;         // = kTW / 4 * kTH: four pixels per thread
constexpr int kRows = 2 * kTH;        // source rows a tile's vertical pass can read
constexpr int kStageBytes = 16384;    // staged row segments of one chunk
constexpr int kMaxPitch = 2048;       // a wider row segment is gathered from global memory instead

// S[k][c][j] of row k's segment at p (its byte 0 = channel 0 of source column sx_lo), for tile column j
__device__ __forceinline__ void hsum(const unsigned char* p, int o0, int o1, int a0, int a1, int* s) {
#pragma unroll
  for (int c = 0; c < 3; ++c) s[c * kTW] = p[o0 + c] * a0 + p[o1 + c] * a1;
}

__device__ __forceinline__ void store4(float* out, size_t plane, const int (&v)[4][3], int bgr) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {  // RGB planes: BGR sources are flipped, as upstream's im[..., ::-1]
    const int s = bgr ? 2 - c : c;
    *reinterpret_cast<float4*>(out + c * plane) = make_float4((float)v[0][s] / 255.f, (float)v[1][s] / 255.f,
                                                              (float)v[2][s] / 255.f, (float)v[3][s] / 255.f);
  }
}

__global__ __launch_bounds__(kThreads) void letterbox_batch_u8(const LetterboxBatchArgs a) {
  __shared__ int xs0[kTW], xs1[kTW], xa[kTW], ys0[kTH], ys1[kTH], yb[kTH];
  __shared__ __attribute__((aligned(16))) int S[kRows * 3 * kTW];
  __shared__ __attribute__((aligned(16))) unsigned char stage[kStageBytes];

  const ym_letterbox_desc d = a.desc[blockIdx.z];
  const unsigned char* src = static_cast<const unsigned char*>(d.src);
  const int tid = threadIdx.x;
  const int x0 = blockIdx.x * kTW, y0 = blockIdx.y * kTH;
  // the tile columns [jlo, jhi] and rows [ilo, ihi] that lie in the frame's window
  const int jlo = max(d.left - x0, 0), jhi = min(min(d.left + d.uw, a.Wn) - x0, kTW) - 1;
  const int ilo = max(d.top - y0, 0), ihi = min(min(d.top + d.uh, a.Hn) - y0, kTH) - 1;
  const int tx = (tid & 15) * 4, ty = tid >> 4;  // this thread's four pixels: tile row ty, columns tx .. tx + 3
  const bool live = x0 + tx < a.Wn && y0 + ty < a.Hn;
  const bool rowin = ty >= ilo && ty <= ihi;
  const size_t plane = (size_t)a.Hn * a.Wn;
  float* out = a.dst + (size_t)blockIdx.z * 3 * plane + (size_t)(y0 + ty) * a.Wn + x0 + tx;
  int v[4][3];
#pragma unroll
  for (int k = 0; k < 4; ++k) v[k][0] = v[k][1] = v[k][2] = 114;

  if (jhi < jlo || ihi < ilo) {  // 0. all border
    if (live) store4(out, plane, v, 0);
    return;
  }
  if (d.uh == d.h && d.uw == d.w) {  // 0. not resized: the pixels themselves
    if (live && rowin) {
      const unsigned char* p = src + (size_t)(y0 + ty - d.top) * d.row_bytes + (ptrdiff_t)(x0 + tx - d.left) * 3;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (tx + k >= jlo && tx + k <= jhi) { v[k][0] = p[3 * k]; v[k][1] = p[3 * k + 1]; v[k][2] = p[3 * k + 2]; }
    }
    if (live) store4(out, plane, v, d.bgr);
    return;
  }

  // 1. axis tables, by the first wave
  if (tid < kTW) {
    int s0, s1, w0, w1;
    bool edge;
    if (tid >= jlo && tid <= jhi) {
      axis(x0 + tid - d.left, d.w, d.scale_x, s0, s1, w0, w1, edge);
      xs0[tid] = s0; xs1[tid] = s1; xa[tid] = w0 | (w1 << 16);
    }
    if (tid >= ilo && tid <= ihi) {
      axis(y0 + tid - d.top, d.h, d.scale_y, s0, s1, w0, w1, edge);
      ys0[tid] = s0; ys1[tid] = s1; yb[tid] = w0 | (w1 << 16);
    }
  }
  __syncthreads();

  // 2. the source rows the tile reads: slot k holds row sy_lo + k (dense), or output row ilo + k / 2's s0 / s1
  const int sx_lo = xs0[jlo], sx_hi = xs1[jhi], sy_lo = ys0[ilo], sy_hi = ys1[ihi];
  const bool dense = sy_hi - sy_lo < kRows;
  const int nrows = dense ? sy_hi - sy_lo + 1 : 2 * (ihi - ilo + 1);
  auto row_of = [&](int k) { return dense ? sy_lo + k : ((k & 1) ? ys1 : ys0)[ilo + (k >> 1)]; };
  const int seg = (sx_hi - sx_lo + 1) * 3;   // bytes of one row segment
  const int pitch = (seg + 30) / 16 * 16;    // + up to 15 bytes in front (aligned loads), rounded up
  const bool staged = pitch <= kMaxPitch;
  const int wpr = pitch / 16;
  const int R = staged ? min(kStageBytes / pitch, nrows) : nrows;
  const unsigned char* src_end = src + (size_t)(d.h - 1) * d.row_bytes + (size_t)3 * d.w;

  for (int k0 = 0; k0 < nrows; k0 += R) {
    const int nr = min(R, nrows - k0);
    if (staged) {  // 3. 16-byte loads of the chunk's row segments
      for (int i = tid; i < nr * wpr; i += kThreads) {
        const int rl = i / wpr, wd = i - rl * wpr;
        const unsigned char* p = src + (size_t)row_of(k0 + rl) * d.row_bytes + (size_t)sx_lo * 3;
        const unsigned char* q = p - (reinterpret_cast<uintptr_t>(p) & 15) + wd * 16;
        if (q >= p + seg) continue;
        uint4 w4;
        if (q >= src && q + 16 <= src_end) {
          w4 = *reinterpret_cast<const uint4*>(q);
        } else {
          unsigned int t[4] = {0, 0, 0, 0};
#pragma unroll
          for (int b = 0; b < 16; ++b)
            if (q + b >= src && q + b < src_end) t[b >> 2] |= (unsigned int)q[b] << (8 * (b & 3));
          w4 = make_uint4(t[0], t[1], t[2], t[3]);
        }
        *reinterpret_cast<uint4*>(stage + rl * pitch + wd * 16) = w4;
      }
      __syncthreads();
    }
    // 4. horizontal pass
    for (int i = tid; i < nr * kTW; i += kThreads) {
      const int rl = i >> 6, j = i & (kTW - 1);
      if (j < jlo || j > jhi) continue;
      const unsigned char* p = src + (size_t)row_of(k0 + rl) * d.row_bytes + (size_t)sx_lo * 3;
      const int o0 = (xs0[j] - sx_lo) * 3, o1 = (xs1[j] - sx_lo) * 3, w = xa[j];
      int* s = S + (k0 + rl) * 3 * kTW + j;
      if (staged)
        hsum(stage + rl * pitch + (int)(reinterpret_cast<uintptr_t>(p) & 15), o0, o1, w & 0xffff, w >> 16, s);
      else
        hsum(p, o0, o1, w & 0xffff, w >> 16, s);
    }
    __syncthreads();
  }

  // 5. vertical pass and the plane stores
  if (live && rowin) {
    const int k0 = dense ? ys0[ty] - sy_lo : 2 * (ty - ilo), k1 = dense ? ys1[ty] - sy_lo : 2 * (ty - ilo) + 1;
    const int b0 = yb[ty] & 0xffff, b1 = yb[ty] >> 16;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int4 u = *reinterpret_cast<const int4*>(S + (k0 * 3 + c) * kTW + tx);
      const int4 l = *reinterpret_cast<const int4*>(S + (k1 * 3 + c) * kTW + tx);
      const int s0[4] = {u.x, u.y, u.z, u.w}, s1[4] = {l.x, l.y, l.z, l.w};
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        if (tx + k < jlo || tx + k > jhi) continue;  // (a border column: S holds nothing there)
        const int t = (s0[k] * b0 + s1[k] * b1 + (1 << 21)) >> 22;
        v[k][c] = t < 0 ? 0 : (t > 255 ? 255 : t);
      }
    }
  }
  if (live) store4(out, plane, v, d.bgr);
}

}  // namespace

hipError_t ym_launch_letterbox_batch(const LetterboxBatchArgs& a, hipStream_t st) {
  if (!a.desc || !a.dst || (reinterpret_cast<uintptr_t>(a.dst) & 15) || a.B < 1 || a.B > 65535 || a.Hn < 1 ||
      a.Wn < 4 || a.Wn % 4)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(letterbox_batch_u8, dim3((a.Wn + kTW - 1) / kTW, (a.Hn + kTH - 1) / kTH, a.B), dim3(kThreads), 0,
                     st, a);
  return hipGetLastError();
}
