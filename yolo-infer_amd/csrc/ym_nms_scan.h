// Device code shared by the NMS kernels (csrc/ym_nms.hip nms_image, csrc/ym_nms_ml.hip nms_ml_image, csrc/ym_obb.hip):
// the small steps every path repeats, the one-wave greedy scan of a 64-row bit-matrix word, and the blocked greedy
// scan.  Inlined device functions only: no kernels, no launchers, no symbols.
#pragma once
#include "ym_common.h"

// ------------------------------------------------------------------------------------------------- small steps
// the index in a candidate key's low word (stored complemented, so equal scores sort by ascending index): the anchor,
// or the multi-label pair anchor * 128 + cls
__device__ __forceinline__ unsigned nms_key_index(unsigned long long key) {
  return 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
}

// a box as the greedy scan compares it: offset by cls * max_wh (0 if agnostic), its area from the offset corners
struct NmsBox {
  float4 b;
  float area;
};
__device__ __forceinline__ NmsBox nms_offset_box(const float4 v, int cl, int agnostic, float max_wh) {
  const float off = agnostic ? 0.0f : (float)cl * max_wh;
  NmsBox o;
  o.b = make_float4(v.x + off, v.y + off, v.z + off, v.w + off);
  o.area = __fmul_rn(__fsub_rn(o.b.z, o.b.x), __fsub_rn(o.b.w, o.b.y));
  return o;
}

// the first six floats of an output row: the box clipped to the image, the score, the class
__device__ __forceinline__ void nms_write_row6(float* r, const float4 v, float score, float cls, float img_w,
                                               float img_h) {
  r[0] = fminf(fmaxf(v.x, 0.f), img_w);
  r[1] = fminf(fmaxf(v.y, 0.f), img_h);
  r[2] = fminf(fmaxf(v.z, 0.f), img_w);
  r[3] = fminf(fmaxf(v.w, 0.f), img_h);
  r[4] = score;
  r[5] = cls;
}

// image b's row count (one thread calls this)
__device__ __forceinline__ void nms_store_count(int* out_counts, int* counts2, int b, int kept) {
  out_counts[b] = kept;
  if (counts2) counts2[b] = kept;
}

// class filter: boxes of different classes are offset cls * max_wh apart and cannot intersect, so a candidate need
// only be compared within its class.  Exact when the offsets separate every pair of boxes: decoded coordinates lie
// within +-reg_max * stride of the image, and the 2,048 margin covers 16 bins x 64 px.
__device__ __forceinline__ bool nms_class_filter(int agnostic, double iou, float max_wh, float img_w, float img_h) {
  return !agnostic && iou >= 0.0 && (double)max_wh >= (double)img_w + (double)img_h + 2048.0;
}

// The n keys of row gk sorted descending, whole workgroup: in `lds` when the count padded to a power of two fits its
// lds_cap entries, else in place in the row (whose stride is a power of two >= n).  Padding keys are 0, below every
// real key.  Returns where the sorted keys are.
__device__ __forceinline__ unsigned long long* nms_sort_keys(unsigned long long* gk, unsigned long long* lds,
                                                             int lds_cap, int n, int tid) {
  int n2 = 1;
  while (n2 < n) n2 <<= 1;
  unsigned long long* k = n2 <= lds_cap ? lds : gk;
  if (k == lds) {
    for (int i = tid; i < n2; i += NMS_T) lds[i] = i < n ? gk[i] : 0ull;
  } else {
    for (int i = n + tid; i < n2; i += NMS_T) gk[i] = 0ull;
  }
  __syncthreads();
  if (n > 1) bitonic_sort_desc(k, n2, tid);
  return k;
}

// ------------------------------------------------------------------------------------------------- the word scan
// One wave decides 64 consecutive rows of a greedy bit matrix (row i's word holds the later rows that i suppresses).
// Lane l passes row l's diagonal word `diag` (bits above l only) and the word's removed bits so far `remv` (the same
// value in every lane); jn rows are real.  The decisions are a wave-uniform chain on scalar registers: the removed
// bits and each visited row's diagonal word are read into SGPRs (readfirstlane / readlane), so a row costs a few
// scalar instructions and no exec-mask branch.  Only the kept rows are visited: the next one is the lowest bit not
// yet removed (rows below a kept row are final, its word only has bits above it).  Returns the kept rows' bits and
// advances `kept`, which never passes cap.
__device__ __forceinline__ unsigned long long nms_scan_word(unsigned long long diag, unsigned long long remv, int jn,
                                                            int cap, int& kept) {
  const unsigned dlo = (unsigned)diag, dhi = (unsigned)(diag >> 32);
  unsigned long long remk =
      ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)(remv >> 32)) << 32) |
      (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((unsigned)remv);
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
  kept = kk;
  return keepbits;
}

// the slot of a kept row among its word's kept rows
__device__ __forceinline__ int nms_keep_slot(unsigned long long keepbits, int lane) {
  return __popcll(keepbits & ((1ull << lane) - 1ull));
}

// The kept rows' later word v (0 from a row that is not kept) ORed across the wave into *rem: shuffles, then one LDS
// write per word (per-lane LDS atomics on one address serialised, ~35 per word).
__device__ __forceinline__ void nms_or_word(unsigned long long v, unsigned long long* rem, int lane) {
  unsigned vlo = (unsigned)v, vhi = (unsigned)(v >> 32);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    vlo |= (unsigned)__shfl_xor((int)vlo, o);
    vhi |= (unsigned)__shfl_xor((int)vhi, o);
  }
  if (lane == 0) *rem |= ((unsigned long long)vhi << 32) | vlo;
}

// ------------------------------------------------------------------------------------------------- the blocked scan
// Greedy NMS over ne candidates in score order, in blocks of NMS_BLK: a block's candidates are first tested against
// every box kept by earlier blocks (the kept lists in LDS), the survivors' intra-block IoU bit matrix is built by all
// waves, and one wave scans it in order with nms_scan_word.  Candidate j is kept iff no kept i < j has IoU > iou:
// torchvision's greedy result, with a few barriers per block instead of one per kept box.  With the class filter
// (cf) a candidate is tested only against kept boxes of its class (per-class lists) and a bit-matrix word only where
// the word holds a box of row i's class (per-word class masks); without it every candidate joins list 0.
constexpr int NMS_BLK = 256;  // candidates per block (bit matrix 256 x 4 words)
constexpr int NMS_W = NMS_BLK / 64;
constexpr int NMS_NC = 128;   // classes of the class filter

struct NmsBlockLds {                    // the scan's LDS regions; a kernel places them
  float4* bb;                           // [NMS_BLK] class-offset boxes of the block
  float* ba;                            // [NMS_BLK] areas
  unsigned* bsup;                       // [NMS_BLK] removed flags
  int* bcls;                            // [NMS_BLK] the class list each joins
  unsigned long long* bmask;            // [NMS_BLK][NMS_W]
  unsigned long long* ccm;              // [NMS_W][NMS_NC] lanes of word w holding class c
  float4* kb;                           // [cap] kept boxes
  float* ka;                            // [cap] their areas
  int* knext;                           // [cap] per-class kept lists
  int* khead;                           // [NMS_NC]
  int* blk_keep;                        // [NMS_BLK] the block's kept rows
  int* blk_kept;                        // [1]
  unsigned long long* blk_rem;          // [NMS_W] removed words
};

// Src is the kernel's candidate source, passed by value:
//   void cand(int i, int t, float4& box, int& cls) const   candidate i of the score order, held in block slot t: its
//                                                          decoded box and class; keeps what write_row will need
//   void write_row(int t, int idx) const                   output row idx from the candidate in block slot t
// Whole workgroup (NMS_T threads); cap <= the kept regions' size.  Returns the number of rows written.
template <class Src>
__device__ __forceinline__ int nms_blocked_scan(const NmsArgs& a, const NmsBlockLds& L, int ne, int cap, bool cf,
                                                int tid, const Src src) {
  constexpr int W = NMS_W;
  for (int i = tid; i < W * NMS_NC; i += NMS_T) L.ccm[i] = 0ull;
  if (tid < NMS_NC) L.khead[tid] = -1;
  __syncthreads();
  int kept = 0;  // uniform: every thread reads blk_kept after the block's barrier
  for (int b0 = 0; b0 < ne && kept < cap; b0 += NMS_BLK) {
    const int nb = ne - b0 < NMS_BLK ? ne - b0 : NMS_BLK;
    if (tid < nb) {
      float4 v;
      int cl;
      src.cand(b0 + tid, tid, v, cl);
      const NmsBox o = nms_offset_box(v, cl, a.agnostic, a.max_wh);
      L.bb[tid] = o.b;
      L.ba[tid] = o.area;
      const int c = cf ? cl : 0;
      L.bcls[tid] = c;
      if (cf) atomicOr(&L.ccm[(tid >> 6) * NMS_NC + c], 1ull << (tid & 63));
    }
    if (tid < NMS_BLK) L.bsup[tid] = tid >= nb;
    __syncthreads();
    if (tid < nb) {  // suppression by the boxes kept in earlier blocks (of this candidate's class list)
      bool sj = false;
      for (int q = L.khead[L.bcls[tid]]; q >= 0 && !sj; q = L.knext[q])
        sj = iou_gt(L.kb[q], L.ka[q], L.bb[tid], L.ba[tid], a.iou);
      if (sj) L.bsup[tid] = 1u;
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
        const unsigned long long cand = (cf ? L.ccm[w * NMS_NC + L.bcls[i]] : ~0ull) & past & in;
        unsigned long long bits = 0ull;
        if (!L.bsup[i] && cand) {  // (uniform)
          const bool sij =
              ((cand >> ln) & 1ull) && !L.bsup[j] && iou_gt(L.bb[i], L.ba[i], L.bb[j], L.ba[j], a.iou);
          bits = __ballot(sij);
        }
        if (ln == 0) L.bmask[pq] = bits;
      }
    }
    __syncthreads();
    if (tid < 64) {  // one wave: the block's greedy scan, removed words seeded by bsup
      const int lane = tid;
#pragma unroll
      for (int w = 0; w < W; ++w) {
        const unsigned long long r = __ballot(L.bsup[64 * w + lane] != 0u);
        if (lane == 0) L.blk_rem[w] = r;
      }
      int kk = kept;
      for (int k2 = 0; k2 < W && kk < cap; ++k2) {
        const int jn = nb - 64 * k2 < 64 ? nb - 64 * k2 : 64;
        if (jn <= 0) break;
        const int row = 64 * k2 + lane;
        const int q0 = kk - kept;
        const unsigned long long keepbits =
            nms_scan_word(row < nb ? L.bmask[row * W + k2] : 0ull, L.blk_rem[k2], jn, cap, kk);
        const bool mine = (keepbits >> lane) & 1ull;
        if (mine) L.blk_keep[q0 + nms_keep_slot(keepbits, lane)] = row;
        for (int w = k2 + 1; w < W; ++w) nms_or_word(mine ? L.bmask[row * W + w] : 0ull, &L.blk_rem[w], lane);
      }
      if (lane == 0) *L.blk_kept = kk;
    } else if (cf) {  // the other waves clear the class masks for the next block
      for (int i = tid - 64; i < W * NMS_NC; i += NMS_T - 64) L.ccm[i] = 0ull;
    }
    __syncthreads();
    const int kept2 = *L.blk_kept;  // <= cap; kept2 - kept <= nb
    for (int q = tid; q < kept2 - kept; q += NMS_T) {  // the block's kept boxes join their class lists; rows written
      const int r = L.blk_keep[q], idx = kept + q;
      L.kb[idx] = L.bb[r];
      L.ka[idx] = L.ba[r];
      L.knext[idx] = atomicExch(&L.khead[L.bcls[r]], idx);
      src.write_row(r, idx);
    }
    kept = kept2;
    __syncthreads();  // the kept lists are complete before the next block reads them; the block regions are free
  }
  return kept;
}
