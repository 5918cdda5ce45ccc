// Single-label class-offset greedy NMS on gfx950 (torchvision's result), one workgroup per image, and the
// multi-workgroup presort of its keys.  The multi-label path: csrc/ym_nms_ml.hip.  The steps the two share (the
// one-wave word scan, the blocked greedy scan, the box / row / count helpers): csrc/ym_nms_scan.h.
#include "ym_nms_scan.h"

namespace {

// ------------------------------------------------------------------------------------------------- NMS
// Per image, one 1024-thread workgroup: bitonic sort of the candidate keys, then greedy suppression exactly as
// torchvision's CPU nms: boxes offset by cls·max_wh (0 if agnostic), areas and IoU in fp32 on the offset boxes,
// suppress iff IoU > iou (compared in double), keep <= max_det, clip to the image.  Up to NMS_LDS candidates
// everything (keys, boxes, areas, flags) lives in LDS, so the serial scan costs LDS latency per candidate;
// larger candidate sets fall back to the same algorithm on global scratch.
constexpr int NMS_LDS = 4096;
// (NMS_BM = 512, ym_common.h) bit-matrix path: 512 x 8 words of 64 bits (32 KB) behind the first 512 boxes
// blocked path (NMS_BM < n, up to NMS_BLK_MAX candidates after max_nms, e.g. the validator's conf 0.001 at 640²: up to
// A = 8,400): the keys sorted in LDS, then nms_blocked_scan (ym_nms_scan.h) over them, with its class filter when
// also nc <= NMS_NC.
// (NMS_SORT = 16384, ym_common.h: keys sorted in LDS, 128 KB, the whole LDS arena)
constexpr int NMS_KEEP = 512;    // kept boxes held in LDS: max_det up to this on the blocked path
// the scan's block / kept-list regions and the block's anchor indices (u64 units) sit at the end of the arena, behind
// the sorted keys they leave in place
constexpr int NR_BB = 0, NR_BA = NR_BB + 2 * NMS_BLK, NR_BAI = NR_BA + NMS_BLK / 2, NR_BSUP = NR_BAI + NMS_BLK / 2,
              NR_BCLS = NR_BSUP + NMS_BLK / 2, NR_BMASK = NR_BCLS + NMS_BLK / 2, NR_CCM = NR_BMASK + NMS_BLK * NMS_W,
              NR_KB = NR_CCM + NMS_W * NMS_NC, NR_KA = NR_KB + 2 * NMS_KEEP, NR_KNEXT = NR_KA + NMS_KEEP / 2,
              NR_KHEAD = NR_KNEXT + NMS_KEEP / 2, NMS_REG = NR_KHEAD + NMS_NC / 2;
constexpr int NMS_BLK_MAX = NMS_SORT - NMS_REG;  // candidates (after max_nms) the blocked path takes: 12,224

// one output row [x1 y1 x2 y2 conf cls coef_0 .. coef_nm-1]: box clipped to the image; a Segment head's nm mask
// coefficients are fetched as float4s all issued before the first store (a scalar load-store loop waited one memory
// latency per coefficient)
__device__ __forceinline__ void write_det(const NmsArgs& a, float* r, size_t anc) {
  const float4 v = a.boxes[anc];
  const float sc = a.scores[anc];
  const int cl = a.cls[anc];
  if (a.nm > 0 && a.nm <= 64 && (a.nm & 3) == 0 && ((a.no_tot | a.mask_off) & 3) == 0) {
    const float4* src = reinterpret_cast<const float4*>(a.anchors + anc * a.no_tot + a.mask_off);
    float4 c[16];
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (4 * i < a.nm) c[i] = src[i];
#pragma unroll
    for (int i = 0; i < 16; ++i)
      if (4 * i < a.nm) {
        r[6 + 4 * i] = c[i].x;
        r[7 + 4 * i] = c[i].y;
        r[8 + 4 * i] = c[i].z;
        r[9 + 4 * i] = c[i].w;
      }
  } else {
    for (int m = 0; m < a.nm; ++m) r[6 + m] = a.anchors[anc * a.no_tot + a.mask_off + m];
  }
  nms_write_row6(r, v, sc, (float)cl, a.img_w, a.img_h);
}

// candidate i of the score order (ym_nms_scan.h, nms_blocked_scan's source): the anchor of sorted key i.  Class and
// score are the anchor's; the block keeps its anchor indices (4 bytes per candidate) for the rows.
struct AnchorSrc {
  const NmsArgs& a;
  const unsigned long long* keys;  // the sorted keys, in LDS
  int* bai;                        // [NMS_BLK] anchor indices of the block
  size_t ib;                       // the image's first anchor
  float* out;
  int rowlen;
  __device__ __forceinline__ void cand(int i, int t, float4& box, int& cls) const {
    const unsigned ai = nms_key_index(keys[i]);
    box = a.boxes[ib + ai];
    cls = a.cls[ib + ai];
    bai[t] = (int)ai;
  }
  __device__ __forceinline__ void write_row(int t, int idx) const {
    write_det(a, out + (size_t)idx * rowlen, ib + (size_t)bai[t]);
  }
};

__global__ __launch_bounds__(NMS_T) void nms_image(const NmsArgs a) {
  // one LDS arena (128 KB), carved per path: keys [NMS_LDS], boxes [NMS_LDS], areas [NMS_LDS], flags [NMS_LDS] for the
  // paths up to NMS_LDS candidates; the sort buffer, then the block / kept-list regions for the blocked path
  __shared__ __attribute__((aligned(16))) unsigned long long arena[NMS_SORT];
  unsigned long long* sk = arena;
  float4* sbx = reinterpret_cast<float4*>(arena + NMS_LDS);
  float* sar = reinterpret_cast<float*>(arena + 3 * NMS_LDS);
  unsigned char* ssup = reinterpret_cast<unsigned char*>(arena + 3 * NMS_LDS + NMS_LDS / 2);
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  if (a.dbg == 6) return;
  unsigned long long* gk = a.keys + (size_t)b * a.kstride;
  // the first NMS_BM keys are loaded before the count is known (the key rows hold kstride >= A entries): the count
  // and the keys are ONE memory round trip instead of two dependent ones; entries past the count are ignored
  const unsigned long long kpre = tid < NMS_BM && tid < a.kstride ? gk[tid] : 0ull;
  int n = a.counts[b];
  if (n > a.A) n = a.A;
  if (a.dbg == 7) return;
  const size_t ib = (size_t)b * a.A;
  const int rowlen = 6 + a.nm;
  float* out = a.dets + (size_t)b * a.max_det * rowlen;
  if (n <= 64) {
    // common case at predict thresholds: one wave, everything in registers, no barriers.
    // lane i holds candidate i; bitonic sort by key across lanes, then the greedy scan with shuffles.
    if (tid >= 64) return;
    const int lane = tid;
    unsigned long long key = lane < n ? kpre : 0ull;
#pragma unroll
    for (int size = 2; size <= 64; size <<= 1) {
#pragma unroll
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        const unsigned long long other = __shfl_xor(key, stride);
        const bool desc = (lane & size) == 0 || size == 64;
        const bool lower = (lane & stride) == 0;
        const bool keep_max = lower == desc;
        key = keep_max ? (key > other ? key : other) : (key < other ? key : other);
      }
    }
    const int ne = n < a.max_nms ? n : a.max_nms;
    const unsigned ai = nms_key_index(key);
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    float ar = 0.f;
    if (lane < ne) {
      const NmsBox o = nms_offset_box(a.boxes[ib + ai], a.cls[ib + ai], a.agnostic, a.max_wh);
      bx = o.b;
      ar = o.area;
    }
    int sup = lane >= ne;
    int keep = 0, kept = 0;
    // candidate i is wave-uniform: v_readlane (a VALU -> SGPR move) instead of ds_bpermute round trips
    auto rl = [](float v, int i) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), i)); };
    for (int i = 0; i < ne && kept < a.max_det; ++i) {
      if (__builtin_amdgcn_readlane(sup, i)) continue;
      ++kept;
      if (lane == i) keep = 1;
      const float4 bi = make_float4(rl(bx.x, i), rl(bx.y, i), rl(bx.z, i), rl(bx.w, i));
      const float ai_area = rl(ar, i);
      if (lane > i && !sup && iou_gt(bi, ai_area, bx, ar, a.iou)) sup = 1;
    }
    const unsigned long long km = __ballot(keep);
    if (keep) {
      const int pos = __popcll(km & ((1ull << lane) - 1ull));
      write_det(a, out + (size_t)pos * rowlen, ib + ai);
    }
    if (lane == 0) nms_store_count(a.out_counts, a.counts2, b, kept);
    return;
  }
  if (n <= NMS_BM) {
    // 64 < n <= 512: rank sort (one barrier), the IoU > iou bit matrix computed by all 1024 threads, then ONE
    // wave scans it greedily (torchvision's loop: keep i unless a kept earlier box suppressed it) — no barrier
    // per kept box.  Keys are unique (anchor index in the low word), so the ranks are a permutation.
    unsigned long long* sorted = sk + NMS_BM;
    unsigned long long* mask = reinterpret_cast<unsigned long long*>(sbx + NMS_BM);  // [ne][W]
    unsigned long long ki = 0;
    if (tid < n) sk[tid] = ki = kpre;
    if (tid == n) sk[n] = 0ull;  // pad to an even count (keys are > 0: the score bits of a candidate are)
    __syncthreads();
    if (a.dbg == 1) return;
    if (tid < n) {
      int r = 0;
      const int n2 = (n + 1) >> 1;
#pragma unroll 4
      for (int j = 0; j < n2; ++j) {  // 16-byte LDS reads, two keys each
        const unsigned long long k0 = sk[2 * j], k1 = sk[2 * j + 1];
        r += (k0 > ki) + (k1 > ki);
      }
      sorted[r] = ki;
    }
    __syncthreads();
    if (a.dbg == 2) return;
    const int ne = n < a.max_nms ? n : a.max_nms;
    const int W = (ne + 63) >> 6;
    if (tid < ne) {
      const unsigned ai = nms_key_index(sorted[tid]);
      const NmsBox o = nms_offset_box(a.boxes[ib + ai], a.cls[ib + ai], a.agnostic, a.max_wh);
      sbx[tid] = o.b;
      sar[tid] = o.area;
    }
    __syncthreads();
    if (a.dbg == 3) return;
    {  // one IoU per lane: wave item (i, w) has lane l test box j = 64 w + l against row i; the ballot IS word w
      const int wv = tid >> 6, ln = tid & 63;
      for (int pq = wv; pq < ne * W; pq += NMS_T / 64) {
        const int i = pq / W, w = pq - i * W;
        const int j = 64 * w + ln;
        const bool s = 64 * w + 63 > i && j > i && j < ne && iou_gt(sbx[i], sar[i], sbx[j], sar[j], a.iou);
        const unsigned long long bits = __ballot(s);
        if (ln == 0) mask[pq] = bits;
      }
    }
    __syncthreads();
    if (a.dbg == 4) return;
    __shared__ int keep_bm[NMS_BM], kept_bm;
    if (tid < 64) {
      // greedy scan, 64 rows per word (nms_scan_word, ym_nms_scan.h); the removed words live in LDS, and a word's
      // kept rows are written in parallel, then OR their later mask words into the later removed words
      const int lane = tid, cap = a.max_det;
      __shared__ unsigned long long rem_w[NMS_BM / 64];
      if (lane < W) rem_w[lane] = 0ull;
      int kept = 0;
      for (int k = 0; k < W && kept < cap; ++k) {
        const int row = 64 * k + lane;
        const int jn = ne - 64 * k < 64 ? ne - 64 * k : 64;
        const int q0 = kept;
        const unsigned long long keepbits = nms_scan_word(row < ne ? mask[row * W + k] : 0ull, rem_w[k], jn, cap, kept);
        const bool mine = (keepbits >> lane) & 1ull;
        if (mine) keep_bm[q0 + nms_keep_slot(keepbits, lane)] = row;
        for (int w = k + 1; w < W; ++w) nms_or_word(mine ? mask[row * W + w] : 0ull, &rem_w[w], lane);
      }
      if (lane == 0) kept_bm = kept;
    }
    __syncthreads();
    if (a.dbg == 5) return;
    const int kept = kept_bm;
    for (int q = tid; q < kept; q += NMS_T)
      write_det(a, out + (size_t)q * rowlen, ib + nms_key_index(sorted[keep_bm[q]]));
    if (tid == 0) nms_store_count(a.out_counts, a.counts2, b, kept);
    return;
  }
  if (n <= NMS_SORT && (n < a.max_nms ? n : a.max_nms) <= NMS_BLK_MAX && a.max_det <= NMS_KEEP && a.dbg != 9) {
    // the blocked path (YM_NMS_DBG=9: off, for the A/B test against the one-box-per-barrier path below)
    int n2 = 1;
    while (n2 < n) n2 <<= 1;
    if (a.dbg == 12) return;  // timing only: the kernel up to the blocked path
    for (int i = tid; i < n2; i += NMS_T) arena[i] = i < n ? gk[i] : 0ull;
    __syncthreads();
    if (a.dbg == 11) return;  // timing only: + the key loads
    // keys sorted ahead of this kernel by several workgroups per image (nms_presort_*, the validator's low conf)
    if (!(a.presorted && n > NMS_BM && n <= NMS_SORT)) bitonic_sort_desc(arena, n2, tid);
    if (a.dbg == 10) return;  // timing only: + the sort
    const int ne = n < a.max_nms ? n : a.max_nms;  // the sorted keys stay in arena[0, ne); the regions follow them
    unsigned long long* reg = arena + NMS_BLK_MAX;
    __shared__ int blk_keep[NMS_BLK], blk_kept;
    __shared__ unsigned long long blk_rem[NMS_W];
    NmsBlockLds L;
    L.bb = reinterpret_cast<float4*>(reg + NR_BB);
    L.ba = reinterpret_cast<float*>(reg + NR_BA);
    L.bsup = reinterpret_cast<unsigned*>(reg + NR_BSUP);
    L.bcls = reinterpret_cast<int*>(reg + NR_BCLS);
    L.bmask = reg + NR_BMASK;
    L.ccm = reg + NR_CCM;
    L.kb = reinterpret_cast<float4*>(reg + NR_KB);  // [NMS_KEEP], as ka and knext
    L.ka = reinterpret_cast<float*>(reg + NR_KA);
    L.knext = reinterpret_cast<int*>(reg + NR_KNEXT);
    L.khead = reinterpret_cast<int*>(reg + NR_KHEAD);
    L.blk_keep = blk_keep;
    L.blk_kept = &blk_kept;
    L.blk_rem = blk_rem;
    const bool cf = a.nc <= NMS_NC && nms_class_filter(a.agnostic, a.iou, a.max_wh, a.img_w, a.img_h);
    const AnchorSrc src{a, arena, reinterpret_cast<int*>(reg + NR_BAI), ib, out, rowlen};
    const int kept = nms_blocked_scan(a, L, ne, a.max_det /* <= NMS_KEEP */, cf, tid, src);
    if (tid == 0) nms_store_count(a.out_counts, a.counts2, b, kept);
    return;
  }
  // the per-box path: keys sorted in LDS up to NMS_LDS of them (after padding), else in place in their global row
  unsigned long long* k = nms_sort_keys(gk, sk, NMS_LDS, n, tid);
  const bool lds = k == sk;
  if (n > a.max_nms) n = a.max_nms;
  float4* bx = lds ? sbx : a.sboxes + (size_t)b * a.A;
  float* ar = lds ? sar : a.sareas + (size_t)b * a.A;
  unsigned char* sup = lds ? ssup : a.sup + (size_t)b * a.A;
  for (int i = tid; i < n; i += NMS_T) {
    const unsigned ai = nms_key_index(k[i]);
    const NmsBox o = nms_offset_box(a.boxes[ib + ai], a.cls[ib + ai], a.agnostic, a.max_wh);
    bx[i] = o.b;
    ar[i] = o.area;
    sup[i] = 0;
  }
  __syncthreads();
  // greedy scan: only LDS traffic inside the loop (a global store here would make every barrier drain vmcnt);
  // the kept sorted positions are recorded and written out in parallel afterwards
  __shared__ int keep_pos[1024];
  const int cap = a.max_det < 1024 ? a.max_det : 1024;
  int kept = 0;
  for (int i = 0; i < n && kept < cap; ++i) {
    if (sup[i]) continue;  // written before the last barrier; uniform across the workgroup
    const float4 bi = bx[i];
    const float ai_area = ar[i];
    if (tid == 0) keep_pos[kept] = i;
    ++kept;
    for (int j = i + 1 + tid; j < n; j += NMS_T)
      if (!sup[j] && iou_gt(bi, ai_area, bx[j], ar[j], a.iou)) sup[j] = 1;
    __syncthreads();
  }
  __syncthreads();
  for (int q = tid; q < kept; q += NMS_T)
    write_det(a, out + (size_t)q * rowlen, ib + nms_key_index(k[keep_pos[q]]));
  if (tid == 0) nms_store_count(a.out_counts, a.counts2, b, kept);
}

}  // namespace

// ------------------------------------------------------------------------------------------------- launchers
hipError_t ym_launch_nms(const NmsArgs& a0, hipStream_t st) {
  NmsArgs a = a0;
  a.dbg = ym_debug_get(YM_DBG_NMS);  // (a test switches the blocked path off between eager runs)
  hipLaunchKernelGGL(nms_image, dim3(a.B), dim3(NMS_T), 0, st, a);
  return hipGetLastError();
}

const void* ym_nms_kernel() { return reinterpret_cast<const void*>(&nms_image); }

// ---- multi-workgroup presort of the NMS keys (verdict r5 item 6: at the validator's conf 0.001 the blocked path's
// one-workgroup sort of up to 16,384 keys took ~130 of nms_image's ~254 us, profiles/r05ad_nms_sort_probe.txt).
// Phase 1: NMS_SORT / PS_CH workgroups per image each sort one 2,048-key chunk in LDS (descending; padding keys 0,
// a real key is never 0: its score bits are those of a positive float) into keys2.  Phase 2: each workgroup stages
// all of its image's sorted chunks in LDS (<= 128 KB) and gives each key of its own chunk its final position —
// its index in its chunk plus, per other chunk, the number of larger keys there (a binary search; keys are unique,
// the anchor index is in their low bits) — and writes it back to keys.  Both phases exit at once for an image with
// <= NMS_BM or > NMS_SORT candidates, where nms_image keeps its own sort (NmsArgs::presorted is checked alike).
constexpr int PS_CH = 2048;
constexpr int PS_NCH = NMS_SORT / PS_CH;

__global__ __launch_bounds__(NMS_T) void nms_presort_chunks(const NmsArgs a) {
  __shared__ unsigned long long k[PS_CH];
  const int b = blockIdx.x / PS_NCH, c = blockIdx.x % PS_NCH, tid = threadIdx.x;
  int n = a.counts[b];
  if (n > a.A) n = a.A;
  if (n <= NMS_BM || n > NMS_SORT || c * PS_CH >= n) return;
  const unsigned long long* gk = a.keys + (size_t)b * a.kstride + c * PS_CH;
  const int m = n - c * PS_CH;
  for (int i = tid; i < PS_CH; i += NMS_T) k[i] = i < m ? gk[i] : 0ull;
  __syncthreads();
  bitonic_sort_desc(k, PS_CH, tid);
  unsigned long long* out = a.keys2 + (size_t)b * a.kstride + c * PS_CH;
  for (int i = tid; i < PS_CH; i += NMS_T) out[i] = k[i];
}

__global__ __launch_bounds__(NMS_T) void nms_presort_merge(const NmsArgs a) {
  __shared__ unsigned long long s[NMS_SORT];
  const int b = blockIdx.x / PS_NCH, c = blockIdx.x % PS_NCH, tid = threadIdx.x;
  int n = a.counts[b];
  if (n > a.A) n = a.A;
  if (n <= NMS_BM || n > NMS_SORT || c * PS_CH >= n) return;
  const int nc = (n + PS_CH - 1) / PS_CH;
  const unsigned long long* src = a.keys2 + (size_t)b * a.kstride;
  for (int i = tid; i < nc * PS_CH; i += NMS_T) s[i] = src[i];
  __syncthreads();
  unsigned long long* gk = a.keys + (size_t)b * a.kstride;
  for (int j = tid; j < PS_CH; j += NMS_T) {
    const unsigned long long key = s[c * PS_CH + j];
    if (key == 0ull) continue;  // chunk padding
    int rank = j;
    for (int c2 = 0; c2 < nc; ++c2) {
      if (c2 == c) continue;
      const unsigned long long* q = s + c2 * PS_CH;
      int lo = 0, hi = PS_CH;  // the first index whose key is smaller (descending order)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (q[mid] > key) lo = mid + 1;
        else hi = mid;
      }
      rank += lo;
    }
    gk[rank] = key;
  }
}

hipError_t ym_launch_nms_presort(const NmsArgs& a, hipStream_t st) {
  if (!a.keys2 || a.kstride < NMS_SORT) return hipErrorInvalidValue;
  hipLaunchKernelGGL(nms_presort_chunks, dim3(a.B * PS_NCH), dim3(NMS_T), 0, st, a);
  hipLaunchKernelGGL(nms_presort_merge, dim3(a.B * PS_NCH), dim3(NMS_T), 0, st, a);
  return hipGetLastError();
}
