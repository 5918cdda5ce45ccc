// Single-label class-offset greedy NMS on gfx950 (torchvision's result), one workgroup per image, and the
// multi-workgroup presort of its keys.  The multi-label path: csrc/ym_nms_ml.hip.
#include "ym_common.h"

namespace {

// ------------------------------------------------------------------------------------------------- NMS
// Per image, one 1024-thread workgroup: bitonic sort of the candidate keys, then greedy suppression exactly as
// torchvision's CPU nms: boxes offset by cls·max_wh (0 if agnostic), areas and IoU in fp32 on the offset boxes,
// suppress iff IoU > iou (compared in double), keep <= max_det, clip to the image.  Up to NMS_LDS candidates
// everything (keys, boxes, areas, flags) lives in LDS, so the serial scan costs LDS latency per candidate;
// larger candidate sets fall back to the same algorithm on global scratch.
constexpr int NMS_LDS = 4096;
constexpr int NMS_BM = 512;  // bit-matrix path: 512 x 8 words of 64 bits (32 KB) behind the first 512 boxes
// blocked path (NMS_BM < n, up to NMS_BLK_MAX candidates after max_nms, e.g. the validator's conf 0.001 at 640²: up to
// A = 8,400): the keys sorted in LDS, then the greedy scan in blocks of NMS_BLK candidates in score order — a block's
// candidates are first tested against every box kept by earlier blocks (the kept list in LDS), the survivors'
// intra-block IoU bit matrix is built by all waves, and one wave scans it in order (as the bit-matrix path).
// Candidate j is kept iff no kept i < j has IoU > iou: torchvision's greedy result, with a few barriers per block
// instead of one per kept box.  Class filter (not agnostic, iou >= 0, max_wh above the boxes' coordinate range, nc <=
// NMS_NC): boxes of different classes are offset cls * max_wh apart and cannot intersect (IoU 0, never > iou), so a
// candidate is tested only against kept boxes of its class (per-class lists) and a bit-matrix word only where the
// word holds a box of row i's class (per-word class masks).
constexpr int NMS_SORT = 16384;  // keys sorted in LDS (128 KB: the whole LDS arena)
constexpr int NMS_BLK = 256;     // candidates per block (bit matrix 256 x 4 words)
constexpr int NMS_KEEP = 512;    // kept boxes held in LDS: max_det up to this on the blocked path
constexpr int NMS_NC = 128;      // classes of the class filter
constexpr int NMS_W = NMS_BLK / 64;
// the block / kept-list regions (u64 units) sit at the end of the arena, behind the sorted keys they leave in place
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
  r[0] = fminf(fmaxf(v.x, 0.f), a.img_w);
  r[1] = fminf(fmaxf(v.y, 0.f), a.img_h);
  r[2] = fminf(fmaxf(v.z, 0.f), a.img_w);
  r[3] = fminf(fmaxf(v.w, 0.f), a.img_h);
  r[4] = sc;
  r[5] = (float)cl;
}

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
    const unsigned ai = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
    float4 bx = make_float4(0.f, 0.f, 0.f, 0.f);
    float ar = 0.f;
    if (lane < ne) {
      const float4 v = a.boxes[ib + ai];
      const float off = a.agnostic ? 0.0f : (float)a.cls[ib + ai] * a.max_wh;
      bx = make_float4(v.x + off, v.y + off, v.z + off, v.w + off);
      ar = __fmul_rn(__fsub_rn(bx.z, bx.x), __fsub_rn(bx.w, bx.y));
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
    if (lane == 0) {
      a.out_counts[b] = kept;
      if (a.counts2) a.counts2[b] = kept;
    }
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
      const unsigned ai = 0xFFFFFFFFu - (unsigned)(sorted[tid] & 0xFFFFFFFFull);
      const float4 v = a.boxes[ib + ai];
      const float off = a.agnostic ? 0.0f : (float)a.cls[ib + ai] * a.max_wh;
      const float4 o = make_float4(v.x + off, v.y + off, v.z + off, v.w + off);
      sbx[tid] = o;
      sar[tid] = __fmul_rn(__fsub_rn(o.z, o.x), __fsub_rn(o.w, o.y));
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
      // greedy scan, 64 candidates per block: lane w holds removed-word w.  Within block k the decisions are a
      // wave-uniform chain on scalar registers: rem (the block's removed bits) and each row's own diagonal word are
      // read into SGPRs (readfirstlane / readlane), so a row costs a few scalar instructions, no exec-mask branch;
      // the block's kept rows are then written in parallel and OR-reduced across the wave into the later words.
      const int lane = tid, cap = a.max_det;
      // the removed words live in LDS: a kept row ORs its later mask words in with ds_or_b64 (one LDS atomic per
      // word, no cross-lane reduction)
      __shared__ unsigned long long rem_w[NMS_BM / 64];
      if (lane < W) rem_w[lane] = 0ull;
      int kept = 0;
      for (int k = 0; k < W && kept < cap; ++k) {
        const int row = 64 * k + lane;
        const unsigned long long diag = row < ne ? mask[row * W + k] : 0ull;
        const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
        const unsigned long long remv = rem_w[k];
        unsigned long long remk =
            ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(remv >> 32)) << 32) |
            (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)remv);
        const int jn = ne - 64 * k < 64 ? ne - 64 * k : 64;
        // visit only the rows that are kept: the next one is the lowest bit of the block's not-yet-removed rows
        // (a row's diagonal word only has bits above the row, so rows below it are final)
        unsigned long long keepbits = 0;
        int kk = kept;
        unsigned long long avail = ~remk & (jn == 64 ? ~0ull : ((1ull << jn) - 1ull));
        while (avail && kk < cap) {
          const int j = __builtin_ctzll(avail);
          keepbits |= 1ull << j;
          ++kk;
          remk |= ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, j) << 32) |
                  (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, j);
          avail &= ~remk & ~((2ull << j) - 1ull);
        }
        const bool mine = (keepbits >> lane) & 1ull;
        if (mine) keep_bm[kept + __popcll(keepbits & ((1ull << lane) - 1ull))] = row;
        // the block's kept rows OR their later mask words into the removed words: an OR across the wave (shuffles),
        // one LDS write per word (per-lane LDS atomics on one address serialised, ~35 per block)
        for (int w = k + 1; w < W; ++w) {
          const unsigned long long v = mine ? mask[row * W + w] : 0ull;
          unsigned vlo = (unsigned)v, vhi = (unsigned)(v >> 32);
#pragma unroll
          for (int o = 32; o > 0; o >>= 1) {
            vlo |= (unsigned)__shfl_xor((int)vlo, o);
            vhi |= (unsigned)__shfl_xor((int)vhi, o);
          }
          if (lane == 0) rem_w[w] |= ((unsigned long long)vhi << 32) | vlo;
        }
        kept = kk;
      }
      if (lane == 0) kept_bm = kept;
    }
    __syncthreads();
    if (a.dbg == 5) return;
    const int kept = kept_bm;
    for (int q = tid; q < kept; q += NMS_T) {
      const unsigned ai = 0xFFFFFFFFu - (unsigned)(sorted[keep_bm[q]] & 0xFFFFFFFFull);
      write_det(a, out + (size_t)q * rowlen, ib + ai);
    }
    if (tid == 0) {
      a.out_counts[b] = kept;
      if (a.counts2) a.counts2[b] = kept;
    }
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
    constexpr int W = NMS_W;
    unsigned long long* reg = arena + NMS_BLK_MAX;
    float4* bb = reinterpret_cast<float4*>(reg + NR_BB);          // [NMS_BLK] class-offset boxes
    float* ba = reinterpret_cast<float*>(reg + NR_BA);            // [NMS_BLK] areas
    int* bai = reinterpret_cast<int*>(reg + NR_BAI);              // [NMS_BLK] anchor indices
    unsigned* bsup = reinterpret_cast<unsigned*>(reg + NR_BSUP);  // [NMS_BLK] removed flags
    int* bcls = reinterpret_cast<int*>(reg + NR_BCLS);            // [NMS_BLK] the class list each joins
    unsigned long long* bmask = reg + NR_BMASK;                   // [NMS_BLK][W]
    unsigned long long* ccm = reg + NR_CCM;                       // [W][NMS_NC] lanes of word w holding class c
    float4* kb = reinterpret_cast<float4*>(reg + NR_KB);          // [NMS_KEEP] kept boxes
    float* ka = reinterpret_cast<float*>(reg + NR_KA);            // [NMS_KEEP] their areas
    int* knext = reinterpret_cast<int*>(reg + NR_KNEXT);          // [NMS_KEEP] per-class kept lists
    int* khead = reinterpret_cast<int*>(reg + NR_KHEAD);          // [NMS_NC]
    __shared__ int blk_keep[NMS_BLK], blk_kept;
    __shared__ unsigned long long blk_rem[W];
    // class filter: exact when the class offsets separate every pair of boxes (decoded coordinates lie within
    // +-reg_max * stride of the image: the 2,048 margin covers 16 bins x 64 px)
    const bool cf = !a.agnostic && a.iou >= 0.0 && a.nc <= NMS_NC &&
                    (double)a.max_wh >= (double)a.img_w + (double)a.img_h + 2048.0;
    const int cap = a.max_det;  // <= NMS_KEEP
    for (int i = tid; i < W * NMS_NC; i += NMS_T) ccm[i] = 0ull;
    if (tid < NMS_NC) khead[tid] = -1;
    __syncthreads();
    int kept = 0;  // uniform: every thread reads blk_kept after the block's barrier
    for (int b0 = 0; b0 < ne && kept < cap; b0 += NMS_BLK) {
      const int nb = ne - b0 < NMS_BLK ? ne - b0 : NMS_BLK;
      if (tid < nb) {
        const unsigned ai = 0xFFFFFFFFu - (unsigned)(arena[b0 + tid] & 0xFFFFFFFFull);
        const float4 v = a.boxes[ib + ai];
        const int cl = a.cls[ib + ai];
        const float off = a.agnostic ? 0.0f : (float)cl * a.max_wh;
        const float4 o = make_float4(v.x + off, v.y + off, v.z + off, v.w + off);
        bb[tid] = o;
        ba[tid] = __fmul_rn(__fsub_rn(o.z, o.x), __fsub_rn(o.w, o.y));
        bai[tid] = (int)ai;
        const int c = cf ? cl : 0;
        bcls[tid] = c;
        if (cf) atomicOr(&ccm[(tid >> 6) * NMS_NC + c], 1ull << (tid & 63));
      }
      if (tid < NMS_BLK) bsup[tid] = tid >= nb;
      __syncthreads();
      if (tid < nb) {  // suppression by the boxes kept in earlier blocks (of this candidate's class)
        bool sj = false;
        for (int q = khead[bcls[tid]]; q >= 0 && !sj; q = knext[q]) sj = iou_gt(kb[q], ka[q], bb[tid], ba[tid], a.iou);
        if (sj) bsup[tid] = 1u;
      }
      __syncthreads();
      {  // the survivors' bit matrix: wave item (i, w) tests row i against boxes 64 w .. 64 w + 63 (ballot = word w);
         // a word without a box of row i's class (or past i) is zero without a test
        const int wv = tid >> 6, ln = tid & 63;
        for (int pq = wv; pq < nb * W; pq += NMS_T / 64) {
          const int i = pq / W, w = pq - i * W;
          const int j = 64 * w + ln;
          const int lo = i + 1 - 64 * w;  // lanes >= lo lie past row i
          const unsigned long long past = lo <= 0 ? ~0ull : (lo >= 64 ? 0ull : ~0ull << lo);
          const int hiw = nb - 64 * w;    // lanes < hiw lie inside the block
          const unsigned long long in = hiw >= 64 ? ~0ull : (hiw <= 0 ? 0ull : ((1ull << hiw) - 1ull));
          const unsigned long long cand = (cf ? ccm[w * NMS_NC + bcls[i]] : ~0ull) & past & in;
          unsigned long long bits = 0ull;
          if (!bsup[i] && cand) {  // (uniform)
            const bool sij = ((cand >> ln) & 1ull) && !bsup[j] && iou_gt(bb[i], ba[i], bb[j], ba[j], a.iou);
            bits = __ballot(sij);
          }
          if (ln == 0) bmask[pq] = bits;
        }
      }
      __syncthreads();
      if (tid < 64) {  // one wave: the block's greedy scan (the bit-matrix path's), removed words seeded by bsup
        const int lane = tid;
#pragma unroll
        for (int w = 0; w < W; ++w) {
          const unsigned long long r = __ballot(bsup[64 * w + lane] != 0u);
          if (lane == 0) blk_rem[w] = r;
        }
        int kk = kept;
        for (int k2 = 0; k2 < W && kk < cap; ++k2) {
          const int jn = nb - 64 * k2 < 64 ? nb - 64 * k2 : 64;
          if (jn <= 0) break;
          const int row = 64 * k2 + lane;
          const unsigned long long diag = row < nb ? bmask[row * W + k2] : 0ull;
          const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
          const unsigned long long remv = blk_rem[k2];
          unsigned long long remk =
              ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(remv >> 32)) << 32) |
              (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)remv);
          unsigned long long keepbits = 0;
          const int q0 = kk - kept;
          unsigned long long avail = ~remk & (jn == 64 ? ~0ull : ((1ull << jn) - 1ull));
          while (avail && kk < cap) {
            const int j = __builtin_ctzll(avail);
            keepbits |= 1ull << j;
            ++kk;
            remk |= ((unsigned long long)(unsigned)__builtin_amdgcn_readlane(dhi, j) << 32) |
                    (unsigned long long)(unsigned)__builtin_amdgcn_readlane(dlo, j);
            avail &= ~remk & ~((2ull << j) - 1ull);
          }
          const bool mine = (keepbits >> lane) & 1ull;
          if (mine) blk_keep[q0 + __popcll(keepbits & ((1ull << lane) - 1ull))] = row;
          for (int w = k2 + 1; w < W; ++w) {
            const unsigned long long v = mine ? bmask[row * W + w] : 0ull;
            unsigned vlo = (unsigned)v, vhi = (unsigned)(v >> 32);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
              vlo |= (unsigned)__shfl_xor((int)vlo, o);
              vhi |= (unsigned)__shfl_xor((int)vhi, o);
            }
            if (lane == 0) blk_rem[w] |= ((unsigned long long)vhi << 32) | vlo;
          }
        }
        if (lane == 0) blk_kept = kk;
      } else if (cf) {  // the other waves clear the class masks for the next block
        for (int i = tid - 64; i < W * NMS_NC; i += NMS_T - 64) ccm[i] = 0ull;
      }
      __syncthreads();
      const int kept2 = blk_kept;
      for (int q = tid; q < kept2 - kept; q += NMS_T) {  // the block's kept boxes join their class lists; rows written
        const int r = blk_keep[q], idx = kept + q;
        kb[idx] = bb[r];
        ka[idx] = ba[r];
        knext[idx] = atomicExch(&khead[bcls[r]], idx);
        write_det(a, out + (size_t)idx * rowlen, ib + (size_t)bai[r]);
      }
      kept = kept2;
      __syncthreads();  // the kept lists are complete before the next block reads them; the block regions are free
    }
    if (tid == 0) {
      a.out_counts[b] = kept;
      if (a.counts2) a.counts2[b] = kept;
    }
    return;
  }
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  const bool lds = n2 <= NMS_LDS;
  unsigned long long* k = lds ? sk : gk;
  if (lds) {
    for (int i = tid; i < n2; i += NMS_T) sk[i] = i < n ? gk[i] : 0ull;
  } else {
    for (int i = n + tid; i < n2; i += NMS_T) gk[i] = 0ull;  // keys have a power-of-two stride >= A
  }
  __syncthreads();
  if (n > 1) bitonic_sort_desc(k, n2, tid);
  if (n > a.max_nms) n = a.max_nms;
  float4* bx = lds ? sbx : a.sboxes + (size_t)b * a.A;
  float* ar = lds ? sar : a.sareas + (size_t)b * a.A;
  unsigned char* sup = lds ? ssup : a.sup + (size_t)b * a.A;
  for (int i = tid; i < n; i += NMS_T) {
    const unsigned ai = 0xFFFFFFFFu - (unsigned)(k[i] & 0xFFFFFFFFull);
    const float4 v = a.boxes[ib + ai];
    const float off = a.agnostic ? 0.0f : (float)a.cls[ib + ai] * a.max_wh;
    const float4 o = make_float4(v.x + off, v.y + off, v.z + off, v.w + off);
    bx[i] = o;
    ar[i] = __fmul_rn(__fsub_rn(o.z, o.x), __fsub_rn(o.w, o.y));
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
  for (int q = tid; q < kept; q += NMS_T) {
    const int i = keep_pos[q];
    const unsigned ai = 0xFFFFFFFFu - (unsigned)(k[i] & 0xFFFFFFFFull);
    write_det(a, out + (size_t)q * rowlen, ib + ai);
  }
  if (tid == 0) {
    a.out_counts[b] = kept;
    if (a.counts2) a.counts2[b] = kept;
  }
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
