// Test-time augmentation for detect plans: Ultralytics DetectionModel._predict_augment (predict / val with augment=True).
//   tta_scale: one pass's input — scale_img(x.flip(3) if flip else x, s, gs=32) of the NORMALISED batch: torch's
//     bilinear resize (align_corners=False, size given) to int(H s) x int(W s), padded right / bottom with 0.447 to
//     the next multiples of 32.  LoadTensor's /255 rule is applied to every tap first (upstream divides, then
//     scales), so the pass's own forward sees values <= 1 and leaves them alone.  Arithmetic as torch's CPU kernel
//     evaluates it: scale = (float)in / out, src = fma(scale, dst + 0.5, -0.5) clamped at 0, i0 = (int)src,
//     i1 = i0 + (i0 < in - 1), l = src - i0, out = fma(1 - ly, fma(1 - lx, a, lx b), ly fma(1 - lx, c, lx d)).
//   tta_merge: after the three forwards have run decode_anchors, the merged candidate set: per merged anchor (the
//     concatenation of the passes' anchors that survive _clip_augmented, in pass order) its box — _descale_pred on
//     xywh: / s in fp32, cx = W - cx for the mirrored pass, then xywh2xyxy — score, class, candidate key
//     (score bits << 32 | ~merged anchor) and, for the multi-label NMS, its class-logit row.  decode_anchors stores
//     xyxy, from which cx and w do not come back bit for bit, so a scaled pass's box is decoded again from its raw DFL
//     bins with decode_anchors' own arithmetic; pass 0 (s = 1) keeps decode_anchors' box.
#include "ym_tta.h"

namespace {

// source index pair and weight of destination index d (torch area_pixel_compute_source_index + guard_index_and_lambda)
__device__ __forceinline__ void tta_axis(int d, int in, float scale, int& i0, int& i1, float& l) {
  float src = fmaf(scale, (float)d + 0.5f, -0.5f);
  src = src < 0.f ? 0.f : src;
  i0 = (int)src;
  i0 = i0 < in - 1 ? i0 : in - 1;
  i1 = i0 + (i0 < in - 1 ? 1 : 0);
  l = fminf(fmaxf(src - (float)i0, 0.f), 1.f);
}

// 4 consecutive output pixels of a row per thread (Ws % 32 == 0): one 16-byte store
__global__ __launch_bounds__(256) void tta_scale(const TtaScaleArgs a) {
  const int q = a.Ws >> 2;
  const long i = blockIdx.x * 256L + threadIdx.x;
  if (i >= (long)a.B * 3 * a.Hs * q) return;
  const int xq = (int)(i % q);
  const long r = i / q;
  const int oy = (int)(r % a.Hs);
  const long pl = r / a.Hs;  // image * 3 + channel
  const bool div = *a.batch_max > 1.0f + a.eps;
  const float* src = a.in + (size_t)pl * a.H * a.W;
  float o[4];
  int y0 = 0, y1 = 0;
  float ly = 0.f;
  if (oy < a.hc) tta_axis(oy, a.H, (float)a.H / (float)a.hc, y0, y1, ly);
  const float sx = (float)a.W / (float)a.wc;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int ox = 4 * xq + e;
    if (oy >= a.hc || ox >= a.wc) {
      o[e] = kTtaPad;
      continue;
    }
    int x0, x1;
    float lx;
    tta_axis(ox, a.W, sx, x0, x1, lx);
    if (a.flip) { x0 = a.W - 1 - x0; x1 = a.W - 1 - x1; }
    float ta = src[(size_t)y0 * a.W + x0], tb = src[(size_t)y0 * a.W + x1];
    float tc = src[(size_t)y1 * a.W + x0], td = src[(size_t)y1 * a.W + x1];
    if (div) { ta = ta / 255.0f; tb = tb / 255.0f; tc = tc / 255.0f; td = td / 255.0f; }
    const float wx0 = 1.0f - lx, wy0 = 1.0f - ly;
    const float top = fmaf(wx0, ta, ym_opaque(lx * tb));
    const float bot = fmaf(wx0, tc, ym_opaque(lx * td));
    o[e] = fmaf(wy0, top, ym_opaque(ly * bot));
  }
  float4* dst = reinterpret_cast<float4*>(a.out + ((size_t)pl * a.Hs + oy) * a.Ws) + xq;
  *dst = make_float4(o[0], o[1], o[2], o[3]);
}

// merged anchor m -> its pass and that pass's anchor index (m < Am)
__device__ __forceinline__ int tta_pass_of(const TtaMergeArgs& a, int m, int& ai) {
  const int p = m >= a.p[2].base ? 2 : (m >= a.p[1].base ? 1 : 0);
  ai = m - a.p[p].base + a.p[p].first;
  return p;
}

constexpr int MG_T = 256;  // merged anchors per workgroup (one image per workgroup row)

__global__ __launch_bounds__(MG_T) void tta_merge(const TtaMergeArgs a) {
  __shared__ int wg_cnt, wg_base;
  const int b = blockIdx.y, tid = threadIdx.x;
  const int m0 = blockIdx.x * MG_T, m = m0 + tid;
  const bool ml = a.rows != nullptr;
  if (tid == 0) wg_cnt = 0;
  __syncthreads();
  bool cand = false;
  int slot = 0;
  unsigned long long key = 0ull;
  if (m < a.Am) {
    int ai;
    const int pi = tta_pass_of(a, m, ai);
    const TtaPass& P = a.p[pi];
    const size_t src = (size_t)b * P.A + ai, dst = (size_t)b * a.Am + m;
    const float best = P.scores[src];
    const int bi = P.cls[src];
    a.scores[dst] = best;
    a.cls[dst] = bi;
    cand = best > a.conf;
    if (cand && a.has_classes) cand = (unsigned)bi < 128u && ((a.classes[bi >> 5] >> (bi & 31)) & 1u);
    if (ml || cand) {  // (the NMS kernels read the boxes of candidates only; multi-label: of any anchor)
      float4 bx = P.boxes[src];
      if (pi != 0) {
        // the DFL expectation per side, as decode_anchors computes it
        const float* row = P.anchors + src * a.no_tot;
        float d[4];
        for (int sd = 0; sd < 4; ++sd) {
          const float* r = row + sd * a.reg_max;
          float mx = -INFINITY;
          for (int i = 0; i < a.reg_max; ++i) mx = fmaxf(mx, r[i]);
          float den = 0.f, num = 0.f;
          for (int i = 0; i < a.reg_max; ++i) {
            const float e = expf(r[i] - mx);
            den += e;
            num = fmaf(e, (float)i, num);
          }
          d[sd] = num / den;
        }
        int l = 0;
        while (l + 1 < a.nl && ai >= P.lvl_off[l + 1]) ++l;
        const int p = ai - P.lvl_off[l];
        const float ax = (float)(p % P.lvl_W[l]) + 0.5f;
        const float ay = (float)(p / P.lvl_W[l]) + 0.5f;
        const float st = a.lvl_stride[l];
        const float x1 = ax - d[0], y1 = ay - d[1];
        const float x2 = ax + d[2], y2 = ay + d[3];
        float cx = (x1 + x2) / 2.0f * st, cy = (y1 + y2) / 2.0f * st;
        float w = (x2 - x1) * st, hh = (y2 - y1) * st;
        // _descale_pred: y[:, :4] /= s in fp32, then cx = W - cx for the mirrored pass; xywh2xyxy after
        cx = __fdiv_rn(cx, P.s); cy = __fdiv_rn(cy, P.s); w = __fdiv_rn(w, P.s); hh = __fdiv_rn(hh, P.s);
        if (P.flip) cx = __fsub_rn(a.img_w, cx);
        const float hw = w / 2.0f, hh2 = hh / 2.0f;
        bx = make_float4(cx - hw, cy - hh2, cx + hw, cy + hh2);
      }
      a.boxes[dst] = bx;
    }
    if (cand && !ml) {
      slot = atomicAdd(&wg_cnt, 1);
      key = ((unsigned long long)__float_as_uint(best) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)m);
    }
  }
  if (ml) {  // the workgroup's class-logit rows: consecutive threads copy consecutive floats
    const int nrow = a.Am - m0 < MG_T ? a.Am - m0 : MG_T;
    const int coff = 4 * a.reg_max;
    float* out = a.rows + ((size_t)b * a.Am + m0) * a.nc;
    for (int e = tid; e < nrow * a.nc; e += MG_T) {
      const int j = ym_div(e, a.div_nc), c = e - j * a.nc;
      int ai;
      const TtaPass& P = a.p[tta_pass_of(a, m0 + j, ai)];
      out[e] = P.anchors[((size_t)b * P.A + ai) * a.no_tot + coff + c];
    }
    return;  // (uniform; ym_launch_nms_ml counts its own candidates)
  }
  __syncthreads();
  if (tid == 0 && wg_cnt > 0) wg_base = atomicAdd(&a.counts[b], wg_cnt);
  __syncthreads();
  if (cand) {
    const int at = wg_base + slot;  // < Am <= kstride: every merged anchor is appended at most once
    if (at >= 0 && at < a.kstride) a.keys[(size_t)b * a.kstride + at] = key;
  }
}

}  // namespace

hipError_t ym_launch_tta_scale(const TtaScaleArgs& a, hipStream_t st) {
  if (!a.in || !a.out || !a.batch_max || a.B < 1 || a.H < 1 || a.W < 1 || a.hc < 1 || a.wc < 1 || a.hc > a.Hs ||
      a.wc > a.Ws || a.Ws % 4)
    return hipErrorInvalidValue;
  const long n = (long)a.B * 3 * a.Hs * (a.Ws >> 2);
  hipLaunchKernelGGL(tta_scale, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
  return hipGetLastError();
}

hipError_t ym_launch_tta_merge(const TtaMergeArgs& a0, hipStream_t st) {
  TtaMergeArgs a = a0;
  int at = 0;
  for (int i = 0; i < kTtaPasses; ++i) {  // the kept ranges tile [0, Am) in pass order, inside each pass's anchors
    const TtaPass& P = a.p[i];
    if (!P.anchors || !P.boxes || !P.scores || !P.cls || P.first < 0 || P.keep < 1 || P.first + P.keep > P.A ||
        P.base != at || !(P.s > 0.f))
      return hipErrorInvalidValue;
    at += P.keep;
  }
  if (at != a.Am || a.kstride < a.Am || a.B < 1 || a.nc < 1 || a.reg_max < 1 || a.nl < 1 || a.nl > 4 ||
      a.no_tot < 4 * a.reg_max + a.nc || !a.boxes || !a.scores || !a.cls || (!a.rows && (!a.keys || !a.counts)))
    return hipErrorInvalidValue;
  a.div_nc = ym_fdiv(a.nc);
  hipLaunchKernelGGL(tta_merge, dim3((a.Am + MG_T - 1) / MG_T, a.B), dim3(MG_T), 0, st, a);
  return hipGetLastError();
}
