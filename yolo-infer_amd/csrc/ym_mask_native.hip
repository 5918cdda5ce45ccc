// Native-resolution instance masks of the Segment head: Ultralytics `ops.process_mask_native(proto, coef, boxes, shape)`
// as the segmentation predictor calls it with retina_masks=True (reached from `YOLO11Model.predict(retina_masks=True)`),
// then the non-empty flag of the predictor's result construction.  Per detection of image b, native size (h0, w0):
//   1. m(y, x) = Σ_c coef[c] · proto[b](y, x, c) over the whole prototype plane (no crop at prototype resolution);
//   2. scale_masks: the window [top, bottom) x [left, right) of the plane that the letterboxed image occupies
//      (mask_window below, the rounding of yolomi/preprocess.py mask_window) is resized to (h0, w0), bilinear,
//      align_corners=False: source index (dst + 0.5)·in/out − 0.5 clamped at 0, neighbour clamped at in − 1, `in` the
//      WINDOW's size; the same formula up and down, no antialiasing;
//   3. crop_mask at native resolution on the box (already in native pixels): x1 ≤ x < x2, y1 ≤ y < y2 in fp32, i.e.
//      the integer range [ceil(x1), ceil(x2)) x [ceil(y1), ceil(y2)); then > 0 → one byte per pixel.
// The crop comes after the resize here (process_mask crops first), so the two paths differ along the box edge and
// mask_upsample16 cannot serve this one.
//
// Layout: image b's n_b masks lie back to back at byte_off[b] of one packed buffer, each h0_b·w0_b bytes, so neither a
// mask nor its rows need be 16-byte aligned.  A workgroup owns CHUNK consecutive bytes of one mask, counted from the
// 16-byte boundary at or below the mask's first byte, so every thread's 16-byte run is aligned in memory whatever the
// mask's address: full runs are one 16-byte store, the runs cut by the mask's first or last byte are byte stores.
// Both evaluate a pixel with the same function.  Only box pixels are evaluated; the rest is stored as zero.  The
// prototype-resolution values a workgroup's box pixels can reach (their bilinear taps: a sub-rectangle of the window)
// are computed into LDS once (mask_lowres's fmaf chain over c) and never touch global memory; where that rectangle
// exceeds the LDS tile (a strong down-scale, where most window pixels are no tap of any output pixel anyway) every
// pixel computes its own four taps from the prototypes instead.
#include "ym_common.h"

namespace {

constexpr int NTILE = 6144;          // LDS tile, floats (24 KB)
constexpr int NRPT = 8;              // 16-byte runs per thread
constexpr int CHUNK = 256 * NRPT * 16;  // mask bytes per workgroup

// scale_masks' window of an (mh, mw) plane for a native (h0, w0) image, in Python's double arithmetic (rint: round
// half to even, as Python's round()).  A window that rounds to nothing is widened to one row / column.
__device__ __forceinline__ void mask_window(int mh, int mw, int h0, int w0, int& top, int& bottom, int& left,
                                            int& right) {
  const double gy = (double)mh / (double)h0, gx = (double)mw / (double)w0;
  const double gain = gy < gx ? gy : gx;
  const double px = ((double)mw - (double)w0 * gain) / 2.0, py = ((double)mh - (double)h0 * gain) / 2.0;
  top = (int)rint(py - 0.1); left = (int)rint(px - 0.1);
  bottom = mh - (int)rint(py + 0.1); right = mw - (int)rint(px + 0.1);
  top = min(max(top, 0), mh - 1); left = min(max(left, 0), mw - 1);
  bottom = min(max(bottom, top + 1), mh); right = min(max(right, left + 1), mw);
}

__device__ __forceinline__ float proto_dot(const float* px, const float* coef, int nm) {
  const f32x4* pr = reinterpret_cast<const f32x4*>(px);
  float v = 0.f;
#pragma unroll 8
  for (int c4 = 0; c4 < nm / 4; ++c4) {
    const f32x4 q = pr[c4];
    v = fmaf(coef[4 * c4], q[0], v);
    v = fmaf(coef[4 * c4 + 1], q[1], v);
    v = fmaf(coef[4 * c4 + 2], q[2], v);
    v = fmaf(coef[4 * c4 + 3], q[3], v);
  }
  return v;
}

// torch's source index (dst + 0.5)·scale − 0.5, each operation rounded on its own (no fused multiply-add), so the tile
// bounds and the pixels that read the tile agree to the bit
__device__ __forceinline__ float src_index(int o, float r) {
  return __fsub_rn(__fmul_rn((float)o + 0.5f, r), 0.5f);
}

// ceil of a box edge as crop_mask's integer bound, clamped to [0, n] (a NaN edge gives 0)
__device__ __forceinline__ int edge(float v, int n) { return (int)fminf(fmaxf(ceilf(v), 0.f), (float)n); }

__global__ __launch_bounds__(256) void mask_native(const MaskNativeArgs a) {
  __shared__ float tile[NTILE];
  __shared__ float coef[64];
  const int d = blockIdx.y;
  // image of mask d: the number of k in [1, B) with offsets[k] <= d, 64 offsets per load round (one dependent load
  // instead of up to B in a row at the head of every workgroup's chain)
  int b = 0;
  for (int k0 = 1; k0 < a.B; k0 += 64) {
    const int k = k0 + (int)(threadIdx.x & 63);
    b += __popcll(__ballot(k < a.B && a.offsets[k] <= d));
  }
  const int h0 = a.shapes[2 * b], w0 = a.shapes[2 * b + 1];
  const int n = h0 * w0;  // bytes of this mask
  unsigned char* const mask = a.masks + (size_t)a.byte_off[b] + (size_t)(d - a.offsets[b]) * (size_t)n;
  const int mis = (int)(reinterpret_cast<size_t>(mask) & 15);
  // this workgroup's bytes [lo, hi) of the mask; v = p + mis counts from the 16-byte boundary below the mask
  const long long v0 = (long long)blockIdx.x * CHUNK;
  if (v0 - mis >= n) return;  // uniform per workgroup
  const int lo = (int)max(0ll, v0 - mis), hi = (int)min((long long)n, v0 + CHUNK - mis);
  const float* row = a.dets + ((size_t)b * a.max_det + (d - a.offsets[b])) * a.stride;
  if (threadIdx.x < a.nm) coef[threadIdx.x] = row[6 + threadIdx.x];
  // crop_mask's integer ranges at native resolution
  const int cx0 = edge(row[0], w0), cx1 = edge(row[2], w0), cy0 = edge(row[1], h0), cy1 = edge(row[3], h0);
  int top, bottom, left, right;
  mask_window(a.MH, a.MW, h0, w0, top, bottom, left, right);
  const int wh = bottom - top, ww = right - left;
  const float ry = (float)wh / (float)h0, rx = (float)ww / (float)w0;
  auto src = [](int o, float r) { const float f = src_index(o, r); return f < 0.f ? 0 : (int)f; };
  // box rows among this workgroup's output rows, and the window rectangle their taps lie in
  const int ra = max(lo / w0, cy0), rb = min((hi - 1) / w0, cy1 - 1);
  const bool hit = ra <= rb && cx0 < cx1;
  int ya = 0, xa = 0, th = 0, tw = 0;
  if (hit) {
    ya = min(src(ra, ry), wh - 1); xa = min(src(cx0, rx), ww - 1);
    th = min(src(rb, ry) + 1, wh - 1) - ya + 1;
    tw = min(src(cx1 - 1, rx) + 1, ww - 1) - xa + 1;
  }
  const bool staged = hit && th * tw <= NTILE;
  const float* plane = a.proto + ((size_t)b * a.MH * a.MW + (size_t)top * a.MW + left) * a.nm;  // the window's origin
  __syncthreads();
  if (staged) {
    for (int i = threadIdx.x; i < th * tw; i += 256) {
      const int y = ya + i / tw, x = xa + (i - (i / tw) * tw);
      tile[i] = proto_dot(plane + ((size_t)y * a.MW + x) * a.nm, coef, a.nm);
    }
    __syncthreads();
  }
  // a pixel's row part (the two source rows and their weight) and the pixel itself: the four taps from the tile, or
  // computed here.  Every store path below evaluates a pixel through these two.
  struct Row { int y0, y1; float ly; };
  auto row_of = [&](int oy) -> Row {
    float fy = src_index(oy, ry);
    fy = fy < 0.f ? 0.f : fy;
    const int y0 = min((int)fy, wh - 1);
    return Row{y0, y0 < wh - 1 ? y0 + 1 : y0, fy - (float)y0};
  };
  auto pixel = [&](const Row& r, int ox) -> bool {
    float fx = src_index(ox, rx);
    fx = fx < 0.f ? 0.f : fx;
    const int x0 = min((int)fx, ww - 1), x1 = x0 < ww - 1 ? x0 + 1 : x0;
    const float ly = r.ly, lx = fx - (float)x0;
    float m00, m01, m10, m11;
    if (staged) {
      const float* t0 = tile + (r.y0 - ya) * tw - xa;
      const float* t1 = tile + (r.y1 - ya) * tw - xa;
      m00 = t0[x0]; m01 = t0[x1]; m10 = t1[x0]; m11 = t1[x1];
    } else {
      const float* p0 = plane + (size_t)r.y0 * a.MW * a.nm;
      const float* p1 = plane + (size_t)r.y1 * a.MW * a.nm;
      m00 = proto_dot(p0 + (size_t)x0 * a.nm, coef, a.nm); m01 = proto_dot(p0 + (size_t)x1 * a.nm, coef, a.nm);
      m10 = proto_dot(p1 + (size_t)x0 * a.nm, coef, a.nm); m11 = proto_dot(p1 + (size_t)x1 * a.nm, coef, a.nm);
    }
    const float v = (1.f - ly) * ((1.f - lx) * m00 + lx * m01) + ly * ((1.f - lx) * m10 + lx * m11);
    return v > 0.f;
  };
  bool on = false;
#pragma unroll 1
  for (int r = 0; r < NRPT; ++r) {
    const int p0 = (int)(v0 + 16 * (256 * r + (int)threadIdx.x) - mis);  // first byte of the run (may be < 0)
    if (p0 >= hi) break;
    if (p0 + 16 <= lo) continue;
    unsigned w[4] = {0u, 0u, 0u, 0u};  // the run's 16 bytes
    const int pa = max(p0, lo), pb = min(p0 + 16, hi);  // the run's bytes inside the mask
    const bool whole = pb - pa == 16;
    if (hit) {
      int oy = pa / w0, ox = pa - oy * w0;
      if (whole && staged && ox + 16 <= w0) {  // the usual run, inside one row: the row part once, 16 unrolled pixels
        if (oy >= ra && oy <= rb && ox < cx1 && ox + 16 > cx0) {
          const Row rw = row_of(oy);
#pragma unroll
          for (int i = 0; i < 16; ++i)
            if (ox + i >= cx0 && ox + i < cx1 && pixel(rw, ox + i)) w[i >> 2] |= 1u << (8 * (i & 3));
        }
      } else if (whole && staged && w0 >= 16) {  // a row's last nA pixels, then the next row's first 16 - nA
        const int nA = w0 - ox;
        const bool inA = oy >= ra && oy <= rb, inB = oy + 1 >= ra && oy + 1 <= rb;
        if ((inA && ox < cx1) || (inB && cx0 < 16 - nA)) {
          const Row rA = row_of(oy), rB = row_of(oy + 1);
#pragma unroll
          for (int i = 0; i < 16; ++i) {
            const bool sec = i >= nA;
            const int x = sec ? i - nA : ox + i;
            const Row rw = sec ? rB : rA;
            if ((sec ? inB : inA) && x >= cx0 && x < cx1 && pixel(rw, x)) w[i >> 2] |= 1u << (8 * (i & 3));
          }
        }
      } else {  // a run cut by the mask's ends, narrower rows than a run, or computing its own taps: pixel by pixel
        unsigned long long w0_7 = 0ull, w8_15 = 0ull;
#pragma unroll 1
        for (int p = pa; p < pb; ++p) {
          if (oy >= ra && oy <= rb && ox >= cx0 && ox < cx1 && pixel(row_of(oy), ox)) {
            const int i = p - p0;
            const unsigned long long bit = 1ull << (8 * (i & 7));
            w0_7 |= i < 8 ? bit : 0ull;
            w8_15 |= i < 8 ? 0ull : bit;
          }
          if (++ox == w0) { ox = 0; ++oy; }
        }
        w[0] = (unsigned)w0_7; w[1] = (unsigned)(w0_7 >> 32); w[2] = (unsigned)w8_15; w[3] = (unsigned)(w8_15 >> 32);
      }
      on = on || (w[0] | w[1] | w[2] | w[3]) != 0u;
    }
    if (whole) {  // mask + p0 is 16-byte aligned by the choice of v
      typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
      *reinterpret_cast<u32x4*>(mask + p0) = u32x4{w[0], w[1], w[2], w[3]};
    } else {  // cut by the mask's first or last byte
      const unsigned long long w0_7 = w[0] | (unsigned long long)w[1] << 32, w8_15 = w[2] | (unsigned long long)w[3] << 32;
      for (int p = pa; p < pb; ++p) {
        const int i = p - p0;
        mask[p] = (unsigned char)(((i < 8 ? w0_7 : w8_15) >> (8 * (i & 7))) & 1ull);
      }
    }
  }
  const unsigned long long bal = __ballot(on);
  if (bal && (threadIdx.x & 63) == __builtin_ctzll(bal)) a.nonempty[d] = 1;
}

}  // namespace

hipError_t ym_launch_masks_native(const MaskNativeArgs& a, long long max_bytes, hipStream_t st) {
  if (a.total <= 0) return hipSuccess;
  if (a.nm > 64 || a.nm % 4 || max_bytes < 1) return hipErrorInvalidValue;
  (void)hipMemsetAsync(a.nonempty, 0, (size_t)a.total * sizeof(int), st);
  const long long gx = (max_bytes + 15 + CHUNK - 1) / CHUNK;  // + 15: a mask may start up to 15 bytes into its first run
  if (gx > 0x7fffffffll || a.total > 65535) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mask_native, dim3((unsigned)gx, a.total), dim3(256), 0, st, a);
  return hipGetLastError();
}
