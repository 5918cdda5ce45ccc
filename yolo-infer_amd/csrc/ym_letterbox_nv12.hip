// NV12 frame batches: the decoder's own surfaces — a full-resolution Y plane and a half-resolution plane of
// interleaved U, V bytes, each with a pitch of its own — to the fp32 NCHW batch ym_infer reads, as ONE launch.  The bits
// are ym_letterbox_batch's (csrc/ym_letterbox_batch.hip, oracle/letterbox.py) for the frame converted to packed BGR by
//   yy = max(0, Y - y_off) * CY + 2^19,  B = u8((yy + CUB·(U-128)) >> 20),  G = u8((yy + CVG·(V-128) + CUG·(U-128)) >> 20),
//   R = u8((yy + CVR·(V-128)) >> 20)                        (int32, arithmetic shift; OpenCV's COLOR_YUV2BGR_NV12 form)
// with pixel (r, c) taking U, V from bytes 2·(c/2), 2·(c/2) + 1 of chroma row r/2.  The six integers are arguments: the
// kernel knows no standard.  Conversion precedes interpolation, so each tap is converted where it is used and no
// converted frame exists anywhere.
//
// Work split as §23's: one workgroup of 256 threads per 64 x 16 output tile of one frame, grid (ceil(Wn / 64),
// ceil(Hn / 16), B), frame blockIdx.z's descriptor row; axis tables by the first wave; at most 32 luma rows per tile (the
// row span when it has at most 32 rows, else each output row's pair).  What is this kernel's own:
//   * Two spans.  Luma columns sx_lo .. sx_hi need chroma bytes (sx_lo & ~1) .. (sx_hi | 1) (w is even, so the last one
//     is inside the row); luma row r needs chroma row r >> 1.  In the dense case a chunk of luma rows r_a .. r_b stages
//     chroma rows r_a >> 1 .. r_b >> 1 (at most nr / 2 + 1 of them) and luma slot k reads chroma slot
//     (r_k >> 1) - (r_a >> 1); with row pairs every luma slot stages the chroma row of its own.
//   * Stage: 14 KiB, luma rows first (R rows of pitch_y), chroma rows behind them (pitch_uv); each pitch is the segment
//     plus up to 15 bytes of alignment rounded up to 16, as §23's.  R is the largest row count whose two regions fit:
//     dense  R = 2·(14336 - pitch_uv) / (2·pitch_y + pitch_uv)   (R·pitch_y + (R/2 + 1)·pitch_uv <= 14336)
//     pairs  R = 14336 / (pitch_y + pitch_uv)
//     1080 x 1920 -> 640: 194 luma columns, both pitches 224 bytes, 32 row-pair slots: 14,336 bytes, one chunk.
//   * Gather rule: a tile whose pitch_y exceeds 1 KiB is not staged.  64 columns read 128 taps; beyond 1 KiB of segment
//     the 16-byte words outnumber the tap pairs, so staging would fetch words that hold no tap.  That is 64 output
//     columns over more than ~990 source columns: a horizontal reduction beyond about 15.5.  Such a tile reads its taps
//     from global memory, for the same <= 32 rows.  Below the rule R >= 6.
//   * Horizontal pass: one thread per (luma slot, tile column): two taps, each Y from the luma stage and U, V from the
//     chroma stage, converted to B, G, R, then the three int32 sums into S[slot][channel][column], channel order B, G, R.
//   * Vertical pass, rounding, clamp, the 114 border, RGB planes and /255.f: §23's.
// LDS: 24 KiB of S + the 14 KiB stage + 0.9 KiB of tables = 39,872 bytes: four workgroups per CU.
// Loads and stores are plain vector ones; nothing outside either plane is read (a 16-byte word that would start in front
// of a plane's first byte or end behind its last is read byte by byte).
#include "ym_common.h"
#include "ym_letterbox_axis.h"

namespace {

constexpr int kTW = 64, kTH = 16;     // output tile
constexpr int kThreads = 256;         // = kTW / 4 * kTH: four pixels per thread
constexpr int kRows = 2 * kTH;        // luma rows a tile's vertical pass can read
constexpr int kStageBytes = 14336;    // staged luma and chroma row segments of one chunk
constexpr int kMaxPitch = 1024;       // a wider luma segment is gathered from global memory instead

__device__ __forceinline__ int u8(int t) { return t < 0 ? 0 : (t > 255 ? 255 : t); }

// (B, G, R) of one pixel
__device__ __forceinline__ void to_bgr(int y, int u, int v, const Nv12Coef& k, int (&c)[3]) {
  const int yy = max(0, y - k.y_off) * k.cy + (1 << 19);
  u -= 128; v -= 128;
  c[0] = u8((yy + k.cub * u) >> 20);
  c[1] = u8((yy + k.cvg * v + k.cug * u) >> 20);
  c[2] = u8((yy + k.cvr * v) >> 20);
}

// Word wd of a staged row segment: the segment is p .. p + seg - 1 of a plane whose bytes are [lo, hi); the words are
// 16-byte aligned in global memory, word 0 the one that holds p.  dst: the row's slot in the stage.
__device__ __forceinline__ void stage_word(const unsigned char* p, int seg, int wd, const unsigned char* lo,
                                           const unsigned char* hi, unsigned char* dst) {
  const unsigned char* q = p - (reinterpret_cast<uintptr_t>(p) & 15) + wd * 16;
  if (q >= p + seg) return;
  uint4 w4;
  if (q >= lo && q + 16 <= hi) {
    w4 = *reinterpret_cast<const uint4*>(q);
  } else {
    unsigned int t[4] = {0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < 16; ++b)
      if (q + b >= lo && q + b < hi) t[b >> 2] |= (unsigned int)q[b] << (8 * (b & 3));
    w4 = make_uint4(t[0], t[1], t[2], t[3]);
  }
  *reinterpret_cast<uint4*>(dst + wd * 16) = w4;
}

__device__ __forceinline__ void store4(float* out, size_t plane, const int (&v)[4][3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c)  // RGB planes from (B, G, R)
    *reinterpret_cast<float4*>(out + c * plane) = make_float4((float)v[0][2 - c] / 255.f, (float)v[1][2 - c] / 255.f,
                                                              (float)v[2][2 - c] / 255.f, (float)v[3][2 - c] / 255.f);
}

__global__ __launch_bounds__(kThreads) void letterbox_nv12_u8(const LetterboxNv12Args a) {
  __shared__ int xs0[kTW], xs1[kTW], xa[kTW], ys0[kTH], ys1[kTH], yb[kTH];
  __shared__ __attribute__((aligned(16))) int S[kRows * 3 * kTW];
  __shared__ __attribute__((aligned(16))) unsigned char stage[kStageBytes];

  const ym_nv12_desc d = a.desc[blockIdx.z];
  const unsigned char* yp = static_cast<const unsigned char*>(d.y);
  const unsigned char* cp = static_cast<const unsigned char*>(d.uv);
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

  if (jhi < jlo || ihi < ilo) {  // all border: no source byte
    if (live) store4(out, plane, v);
    return;
  }
  if (d.uh == d.h && d.uw == d.w) {  // not resized: the converted pixels themselves
    if (live && rowin) {
      const int r = y0 + ty - d.top, c = x0 + tx - d.left;  // (c may be negative: only columns in the window are read)
      const unsigned char* py = yp + (size_t)r * d.y_pitch;
      const unsigned char* pc = cp + (size_t)(r >> 1) * d.uv_pitch;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (tx + k >= jlo && tx + k <= jhi) {
          const int cc = (c + k) & ~1;
          to_bgr(py[c + k], pc[cc], pc[cc + 1], a.coef, v[k]);
        }
    }
    if (live) store4(out, plane, v);
    return;
  }

  // axis tables, by the first wave
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

  // the luma rows the tile reads: slot k holds row sy_lo + k (dense), or output row ilo + k / 2's s0 / s1
  const int sx_lo = xs0[jlo], sx_hi = xs1[jhi], sy_lo = ys0[ilo], sy_hi = ys1[ihi];
  const bool dense = sy_hi - sy_lo < kRows;
  const int nrows = dense ? sy_hi - sy_lo + 1 : 2 * (ihi - ilo + 1);
  auto row_of = [&](int k) { return dense ? sy_lo + k : ((k & 1) ? ys1 : ys0)[ilo + (k >> 1)]; };
  const int ux_lo = sx_lo & ~1;                      // first chroma byte of a row segment
  const int seg_y = sx_hi - sx_lo + 1, seg_c = (sx_hi | 1) - ux_lo + 1;
  const int pitch_y = (seg_y + 30) / 16 * 16, pitch_c = (seg_c + 30) / 16 * 16;
  const bool staged = pitch_y <= kMaxPitch;
  const int wpr_y = pitch_y / 16, wpr_c = pitch_c / 16;
  const int fit = dense ? 2 * (kStageBytes - pitch_c) / (2 * pitch_y + pitch_c) : kStageBytes / (pitch_y + pitch_c);
  const int R = staged ? min(fit, nrows) : nrows;
  unsigned char* cstage = stage + (staged ? R * pitch_y : 0);
  const unsigned char* y_end = yp + (size_t)(d.h - 1) * d.y_pitch + d.w;
  const unsigned char* c_end = cp + (size_t)(d.h / 2 - 1) * d.uv_pitch + d.w;

  for (int k0 = 0; k0 < nrows; k0 += R) {
    const int nr = min(R, nrows - k0);
    const int c0 = row_of(k0) >> 1;                                 // dense: the chunk's first chroma row
    const int nc = dense ? (row_of(k0 + nr - 1) >> 1) - c0 + 1 : nr;  // chroma rows of the chunk
    if (staged) {
      for (int i = tid; i < nr * wpr_y + nc * wpr_c; i += kThreads) {
        if (i < nr * wpr_y) {
          const int rl = i / wpr_y;
          stage_word(yp + (size_t)row_of(k0 + rl) * d.y_pitch + sx_lo, seg_y, i - rl * wpr_y, yp, y_end,
                     stage + rl * pitch_y);
        } else {
          const int u = (i - nr * wpr_y) / wpr_c;
          const int cr = dense ? c0 + u : row_of(k0 + u) >> 1;
          stage_word(cp + (size_t)cr * d.uv_pitch + ux_lo, seg_c, i - nr * wpr_y - u * wpr_c, cp, c_end,
                     cstage + u * pitch_c);
        }
      }
      __syncthreads();
    }
    // horizontal pass: both taps converted, then the three sums
    for (int i = tid; i < nr * kTW; i += kThreads) {
      const int rl = i >> 6, j = i & (kTW - 1);
      if (j < jlo || j > jhi) continue;
      const int r = row_of(k0 + rl);
      const unsigned char* py = yp + (size_t)r * d.y_pitch + sx_lo;
      const unsigned char* pc = cp + (size_t)(r >> 1) * d.uv_pitch + ux_lo;
      if (staged) {
        py = stage + rl * pitch_y + (int)(reinterpret_cast<uintptr_t>(py) & 15);
        pc = cstage + (dense ? (r >> 1) - c0 : rl) * pitch_c + (int)(reinterpret_cast<uintptr_t>(pc) & 15);
      }
      const int t0 = xs0[j], t1 = xs1[j], w = xa[j];
      const int e0 = (t0 & ~1) - ux_lo, e1 = (t1 & ~1) - ux_lo;
      int p0[3], p1[3];
      to_bgr(py[t0 - sx_lo], pc[e0], pc[e0 + 1], a.coef, p0);
      to_bgr(py[t1 - sx_lo], pc[e1], pc[e1 + 1], a.coef, p1);
      int* s = S + (k0 + rl) * 3 * kTW + j;
#pragma unroll
      for (int c = 0; c < 3; ++c) s[c * kTW] = p0[c] * (w & 0xffff) + p1[c] * (w >> 16);
    }
    __syncthreads();
  }

  // vertical pass and the plane stores
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
        v[k][c] = u8((s0[k] * b0 + s1[k] * b1 + (1 << 21)) >> 22);
      }
    }
  }
  if (live) store4(out, plane, v);
}

// NV12 → packed (h, w, 3) uint8 BGR, for Results.orig_img / plot() / save(): a thread converts the two pixels that share
// one chroma pair; 64 pairs x 4 rows per workgroup.
__global__ __launch_bounds__(kThreads) void nv12_to_bgr_u8(const Nv12ToBgrArgs a) {
  const int c = (blockIdx.x * 64 + (threadIdx.x & 63)) * 2, r = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (c >= a.w || r >= a.h) return;
  const unsigned char* py = a.y + (size_t)r * a.y_pitch + c;
  const unsigned char* pc = a.uv + (size_t)(r >> 1) * a.uv_pitch + c;
  unsigned char* o = a.bgr + (size_t)r * a.row_bytes + (size_t)3 * c;
  const int u = pc[0], v = pc[1];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    int p[3];
    to_bgr(py[k], u, v, a.coef, p);
    o[3 * k] = (unsigned char)p[0]; o[3 * k + 1] = (unsigned char)p[1]; o[3 * k + 2] = (unsigned char)p[2];
  }
}

}  // namespace

hipError_t ym_launch_letterbox_nv12(const LetterboxNv12Args& a, hipStream_t st) {
  if (!a.desc || !a.dst || (reinterpret_cast<uintptr_t>(a.dst) & 15) || a.B < 1 || a.B > 65535 || a.Hn < 1 ||
      a.Wn < 4 || a.Wn % 4)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(letterbox_nv12_u8, dim3((a.Wn + kTW - 1) / kTW, (a.Hn + kTH - 1) / kTH, a.B), dim3(kThreads), 0,
                     st, a);
  return hipGetLastError();
}

hipError_t ym_launch_nv12_to_bgr(const Nv12ToBgrArgs& a, hipStream_t st) {
  if (!a.y || !a.uv || !a.bgr || a.h < 2 || a.w < 2 || (a.h & 1) || (a.w & 1) || a.h > 4 * 65535 || a.y_pitch < a.w ||
      a.uv_pitch < a.w || a.row_bytes < 3 * (long long)a.w)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(nv12_to_bgr_u8, dim3((a.w / 2 + 63) / 64, (a.h + 3) / 4), dim3(kThreads), 0, st, a);
  return hipGetLastError();
}
