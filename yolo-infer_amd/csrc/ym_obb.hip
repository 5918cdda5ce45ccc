// Oriented bounding boxes on gfx950 (Ultralytics OBB head, 8.3.x rules restated in DESIGN.md): the rotated decode
// (dist2rbox), the candidate stage, and non_max_suppression(rotated=True) = nms_rotated: a Fast-NMS on ProbIoU.
//
//   obb_decode       4 lanes per anchor, decode_anchors' split and arithmetic order for the DFL distances and the class
//                    scan (so scores equal a detect plan's bit for bit), plus theta = (sigmoid(z) - 0.25) pi, the
//                    rotated centre, and the covariance terms (A, B, C) of the box — the NMS never calls sin / cos.
//   obb_sort_gather  one workgroup per image: the candidate keys sorted by bitonic_sort_desc (ym_common.h; presorted
//                    by ym_launch_nms_presort at low conf, as for nms_image), then candidate i of the score order is
//                    gathered into one 32-byte ObbEntry with its class offset applied.
//   obb_nms_flags    Fast-NMS has no sequential dependency: keep[j] = no i < j with probiou(i, j) >= iou, whether i
//                    itself survives or not.  Grid (blocks of 256 sorted candidates j, image); a workgroup streams the
//                    tiles of earlier candidates i = 0 .. its own block through LDS, double buffered (one barrier per
//                    tile, the next tile's global loads in flight during the pair arithmetic); each thread owns one j
//                    and folds the comparison over the tile, reading entry i as an LDS broadcast (all lanes the same
//                    address).  The workgroup stops streaming once every wave's ballot says its j are all suppressed;
//                    the diagonal tile masks i < j.  One keep byte per candidate; no atomics, no data-dependent order.
//   obb_rows         one workgroup per image: ballot + prefix sum of the keep bytes in score order; the first max_det
//                    keepers become rows [cx, cy, w, h, conf, cls, theta].
//
// Plain fp32: the pair function is a transcendental chain (log, exp, sqrt, two divisions) over five sums, not a GEMM,
// so matrix instructions have nothing to multiply.  The >= comparison is made in one place, probiou_ge.
#include "ym_nms_scan.h"

namespace {

constexpr int OBB_T = 256;  // candidates j per flags workgroup = entries per LDS tile
constexpr float kObbEps = 1e-7f;

// probiou(i, j) >= thr, batch_probiou's formula.  det = sA sB - sC² loses its leading digits for thin boxes near 45°
// (both products ~a'²/4, the difference ~a' b'), so the two products' rounding errors are added back (fmaf residuals);
// sqrt(max(A B - C², 0)) of one box is w h / 12 exactly, carried as S.
__device__ __forceinline__ bool probiou_ge(const float4 i0, const float2 i1, const float4 j0, const float2 j1,
                                           double thr) {
  const float sA = i0.z + j0.z, sB = i0.w + j0.w, sC = i1.x + j1.x;
  const float p = __fmul_rn(sA, sB), q = __fmul_rn(sC, sC);
  const float det = __fadd_rn(__fsub_rn(p, q), __fsub_rn(fmaf(sA, sB, -p), fmaf(sC, sC, -q)));
  const float den = det + kObbEps;
  const float dx = i0.x - j0.x, dy = i0.y - j0.y;
  const float t1 = 0.25f * (sA * dy * dy + sB * dx * dx) / den;
  const float t2 = -0.5f * (sC * dx * dy) / den;  // (x2 - x1)(y1 - y2) = -dx dy
  const float t3 = 0.5f * logf(det / (4.0f * i1.y * j1.y + kObbEps) + kObbEps);
  const float bd = fminf(fmaxf(t1 + t2 + t3, kObbEps), 100.0f);
  const float hd = sqrtf(-expm1f(-bd) + kObbEps);
  return (double)(1.0f - hd) >= thr;
}

// ------------------------------------------------------------------------------------------------- decode
__global__ __launch_bounds__(256) void obb_decode(const ObbArgs a) {
  // the workgroup's 64 anchor rows are contiguous: staged in LDS with coalesced 16-byte loads (odd pitch: the 16
  // anchors x 4 sides of a wave read 16-float strided bins)
  extern __shared__ float rows[];  // [64][no_tot + 1]
  const long total = (long)a.B * a.A;
  const long a0 = blockIdx.x * 64L;
  const int nrow = total - a0 < 64 ? (int)(total - a0) : 64;
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
  const int sub = threadIdx.x & 3;
  const bool valid = gidx < total;
  const long idx = valid ? gidx : 0;
  const int b = idx / a.A;
  const int ai = idx - (long)b * a.A;
  const float* row = rows + (valid ? (threadIdx.x >> 2) : 0) * ldr;
  float dist;
  {  // DFL: softmax over the bins, expectation of the bin index (decode_anchors' order)
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
  // class score = max sigmoid, first index on ties; only logits within 0.5 of the quarter's max can reach its value
  const int q = (a.nc + 3) / 4;
  const float* cl = row + 4 * a.reg_max;
  const int c0 = sub * q, c1 = (sub + 1) * q < a.nc ? (sub + 1) * q : a.nc;
  float lmax = -INFINITY;
  for (int c = c0; c < c1; ++c) lmax = fmaxf(lmax, cl[c]);
  const float lthr = lmax < 10.0f ? lmax - 0.5f : -INFINITY;
  float best = -INFINITY;
  int bi = 0x7FFFFFFF;
  for (int c = c0; c < c1; ++c) {
    if (!(cl[c] >= lthr)) continue;
    const float sc = ym_sigmoid(cl[c]);
    if (sc > best) { best = sc; bi = c; }
  }
#pragma unroll
  for (int o = 1; o < 4; o <<= 1) {
    const float ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi < bi)) { best = ob; bi = oi; }
  }
  const int base = threadIdx.x & 60;
  const float dl = __shfl(dist, base), dt = __shfl(dist, base + 1), dr = __shfl(dist, base + 2),
              db = __shfl(dist, base + 3);
  // candidates are appended per workgroup: LDS slots, then one global atomic per (workgroup, image)
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
    // dist2rbox: the ltrb midpoint offset rotated by theta about the anchor point
    const float th = (ym_sigmoid(row[a.ang_off]) - 0.25f) * 3.14159265358979323846f;
    float sn, cs;
    sincosf(th, &sn, &cs);
    const float xf = (dr - dl) / 2.0f, yf = (db - dt) / 2.0f;
    const float cx = (xf * cs - yf * sn + ax) * st, cy = (xf * sn + yf * cs + ay) * st;
    const float w = (dl + dr) * st, h = (dt + db) * st;
    const float va = w * w / 12.0f, vb = h * h / 12.0f;
    a.boxes[idx] = make_float4(cx, cy, w, h);
    a.cov[idx] = make_float4(th, va * cs * cs + vb * sn * sn, va * sn * sn + vb * cs * cs, (va - vb) * cs * sn);
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

// ------------------------------------------------------------------------------------------------- sort + gather
__global__ __launch_bounds__(NMS_T) void obb_sort_gather(const ObbArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned long long arena[NMS_SORT];
  const int b = blockIdx.x, tid = threadIdx.x;
  unsigned long long* gk = a.keys + (size_t)b * a.kstride;
  int n = a.counts[b];
  if (n > a.A) n = a.A;
  // the presort kernels take exactly the images with NMS_BM < n <= NMS_SORT (ym_nms.hip); every other image is sorted
  // here: in LDS, or (n above NMS_SORT) in place in its key row, whose stride is a power of two >= A
  const bool sorted = a.presort && n > NMS_BM && n <= NMS_SORT;
  const unsigned long long* k = sorted ? gk : nms_sort_keys(gk, arena, NMS_SORT, n, tid);
  const int ne = n < a.max_nms ? n : a.max_nms;
  const size_t ib = (size_t)b * a.A;
  for (int i = tid; i < ne; i += NMS_T) {
    unsigned anc = nms_key_index(k[i]);
    if (anc >= (unsigned)a.A) anc = 0;  // (not a key obb_decode wrote: never read out of bounds)
    const float4 v = a.boxes[ib + anc], c = a.cov[ib + anc];
    const int cl = a.cls[ib + anc];
    ObbEntry e;
    e.x = a.agnostic ? v.x : __fadd_rn(v.x, __fmul_rn((float)cl, a.max_wh));
    e.y = v.y; e.A = c.y; e.B = c.z; e.C = c.w; e.S = v.z * v.w / 12.0f;
    e.cls = cl; e.anc = anc;
    a.sorted[ib + i] = e;
  }
  if (tid == 0) a.nsel[b] = ne;
}

// ------------------------------------------------------------------------------------------------- Fast-NMS flags
__global__ __launch_bounds__(OBB_T) void obb_nms_flags(const ObbArgs a) {
  __shared__ float4 tile[2][2 * OBB_T];  // two buffers of 256 entries (8 KB each)
  __shared__ int alive[2][OBB_T / 64];
  const int b = blockIdx.y, jb = blockIdx.x, tid = threadIdx.x;
  const int ne = a.nsel[b] < a.A ? a.nsel[b] : a.A;
  if (jb * OBB_T >= ne) return;  // (uniform)
  const float4* src = reinterpret_cast<const float4*>(a.sorted + (size_t)b * a.A);
  const int j = jb * OBB_T + tid;
  const bool live = j < ne;
  float4 j0 = make_float4(0.f, 0.f, 0.f, 0.f), j1 = j0;
  if (live) { j0 = src[2 * j]; j1 = src[2 * j + 1]; }
  const int cj = __float_as_int(j1.z);
  // different classes are cls * max_wh apart in x and cannot overlap: nms_image's class filter, under its condition
  const bool cf = nms_class_filter(a.agnostic, a.iou, a.max_wh, a.img_w, a.img_h);
  bool sup = false;
  float4 p0 = j0, p1 = j0;
  if (tid < ne) { p0 = src[2 * tid]; p1 = src[2 * tid + 1]; }  // tile 0
  for (int t = 0; t <= jb; ++t) {
    float4* cur = tile[t & 1];
    cur[2 * tid] = p0;
    cur[2 * tid + 1] = p1;
    const unsigned long long al = __ballot(live && !sup);
    if ((tid & 63) == 0) alive[t & 1][tid >> 6] = al != 0ull;
    __syncthreads();  // the only barrier per tile: buffer t & 1 is rewritten two tiles on, behind the next barrier
    int any = 0;
#pragma unroll
    for (int w = 0; w < OBB_T / 64; ++w) any |= alive[t & 1][w];
    if (!any) break;  // (uniform: every thread reads the same flags)
    if (t < jb) {     // the next tile's loads fly during this tile's arithmetic
      const int i = (t + 1) * OBB_T + tid;
      if (i < ne) { p0 = src[2 * i]; p1 = src[2 * i + 1]; }
    }
    if (al == 0ull) continue;  // (wave-uniform) this wave's j are all decided; it only keeps feeding tiles
    const int base = t * OBB_T;
    int lim = ne - base < OBB_T ? ne - base : OBB_T;
    if (t == jb && lim > (tid | 63)) lim = tid | 63;  // diagonal tile: i < j, and the wave's largest j is base + tid | 63
    for (int i = 0; i < lim; ++i) {
      const float4 i0 = cur[2 * i], i1 = cur[2 * i + 1];  // LDS broadcast
      if (base + i < j && live && !sup && (!cf || __float_as_int(i1.z) == cj))
        sup = probiou_ge(i0, make_float2(i1.x, i1.y), j0, make_float2(j1.x, j1.y), a.iou);
    }
  }
  if (live) a.keep[(size_t)b * a.A + j] = sup ? 0 : 1;
}

// ------------------------------------------------------------------------------------------------- rows
__global__ __launch_bounds__(NMS_T) void obb_rows(const ObbArgs a) {
  __shared__ int wsum[NMS_T / 64];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int ne = a.nsel[b] < a.A ? a.nsel[b] : a.A;
  const size_t ib = (size_t)b * a.A;
  float* out = a.dets + (size_t)b * a.max_det * 7;
  int kept = 0;  // uniform
  for (int j0 = 0; j0 < ne && kept < a.max_det; j0 += NMS_T) {
    const int j = j0 + tid;
    const bool k = j < ne && a.keep[ib + j] != 0;
    const unsigned long long bal = __ballot(k);
    if (lane == 0) wsum[wv] = __popcll(bal);
    __syncthreads();
    int off = kept, tot = 0;
#pragma unroll
    for (int w = 0; w < NMS_T / 64; ++w) {
      const int v = wsum[w];
      off += w < wv ? v : 0;
      tot += v;
    }
    const int pos = off + __popcll(bal & ((1ull << lane) - 1ull));
    if (k && pos < a.max_det) {
      const size_t anc = ib + a.sorted[ib + j].anc;
      const float4 v = a.boxes[anc];
      float* r = out + (size_t)pos * 7;
      r[0] = v.x; r[1] = v.y; r[2] = v.z; r[3] = v.w;
      r[4] = a.scores[anc];
      r[5] = (float)a.cls[anc];
      r[6] = a.cov[anc].x;
    }
    kept += tot;
    __syncthreads();  // wsum is rewritten by the next chunk
  }
  if (tid == 0) {
    const int n = kept < a.max_det ? kept : a.max_det;
    a.out_counts[b] = n;
    if (a.counts2) a.counts2[b] = n;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------- launchers
hipError_t ym_launch_obb_decode(const ObbArgs& a, hipStream_t st) {
  if (a.B < 1 || a.A < 21 || a.no_tot % 4 || a.no_tot > 192 || a.reg_max < 1 || a.nc < 1 || a.nl < 1 || a.nl > 4 ||
      4 * a.reg_max + a.nc > a.no_tot || a.ang_off < 0 || a.ang_off >= a.no_tot || a.kstride < a.A)
    return hipErrorInvalidValue;  // (A >= 21: a workgroup's 64 anchors span at most 5 images, 8 counter slots)
  const long total = (long)a.B * a.A;
  hipLaunchKernelGGL(obb_decode, dim3((total + 63) / 64), dim3(256), (size_t)64 * (a.no_tot + 1) * sizeof(float), st, a);
  return hipGetLastError();
}

hipError_t ym_launch_obb_nms(const ObbArgs& a, hipStream_t st) {
  if (a.B < 1 || a.A < 1 || a.kstride < a.A || a.max_det < 1 || a.max_nms < 1) return hipErrorInvalidValue;
  if (a.presort) {  // the keys sorted over several workgroups per image, as ahead of nms_image
    NmsArgs n{};
    n.keys = a.keys; n.keys2 = a.keys2; n.counts = a.counts; n.kstride = a.kstride; n.A = a.A; n.B = a.B;
    const hipError_t e = ym_launch_nms_presort(n, st);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(obb_sort_gather, dim3(a.B), dim3(NMS_T), 0, st, a);
  const int jmax = a.A < a.max_nms ? a.A : a.max_nms;
  hipLaunchKernelGGL(obb_nms_flags, dim3((jmax + OBB_T - 1) / OBB_T, a.B), dim3(OBB_T), 0, st, a);
  hipLaunchKernelGGL(obb_rows, dim3(a.B), dim3(NMS_T), 0, st, a);
  return hipGetLastError();
}
