// Multi-label candidate stage, top-max_nms selection, key sort and NMS: Ultralytics non_max_suppression(...,
// multi_label=True), the validator's post-processing (ym_infer_args.multi_label).  Per image:
//   i, j = where(cls_scores > conf)            every (anchor, class) pair above conf is a candidate
//   keep the max_nms best by (score desc, anchor asc, class asc); greedy NMS on box + cls * max_wh; <= max_det rows.
// The pair count reaches A * nc (672,000 at 640²), so no (B, A * nc) key array exists.  The candidates are never
// materialised before the cut:
//   1. ml_hist / ml_pick, up to 6 levels: an exact radix select of the max_nms-th largest key.  A key is
//      score bits << 32 | ~(anchor * 128 + cls); its 60 significant bits (a score in [0, 1] has bits < 2^30, the pair
//      index is < 2^30) are taken 10 at a time, most significant first.  A level histograms the digit of the pairs
//      that match the digits chosen so far (1024 bins per image) and picks the bin that holds the cut.  An image is
//      done as soon as the cut falls on a bin boundary (its whole bin is taken) — with distinct scores after 2 or 3
//      levels; the index levels only run out when many equal scores straddle the cut.  Keys are unique, so after the
//      last level the cut is one key: the selection is exact for any input.
//   2. ml_compact: the pairs whose key is >= the cut are appended to the image's `sel` row (`cap` keys).  The row
//      holds exactly min(n, max_nms) keys by construction; every slot is still compared with `cap` before the store.
//      Appends race, but the keys are unique and sorted next, so the output does not depend on their order.
//   3. ml_sort_chunks / ml_sort_merge: 2,048-key chunks sorted in LDS, then every key ranked against the other chunks
//      (the scheme of nms_presort_* in csrc/ym_nms.hip; 32,768 keys do not fit in LDS at once, so the other chunks
//      pass through it one at a time).
//   4. nms_ml_image: nms_image's blocked greedy scan (blocks of 256 candidates in score order against the kept list,
//      an intra-block bit matrix, one wave scanning it) with the class and the score taken from the key, the sorted
//      keys read from global memory and up to 1,024 kept boxes.  Same arithmetic: iou_gt (csrc/ym_common.h), offset
//      cls * max_wh added in fp32, rows clipped as write_det does.
// Every pass recomputes the scores from the fp32 anchor buffer with decode_anchors' ym_sigmoid on the same logit, so a
// pair that is also its anchor's single-label candidate has the bit-identical score; boxes are decode_anchors' own.
#include "ym_common.h"

namespace {

constexpr int ML_T = 256;             // threads of a candidate-stage workgroup
constexpr int ML_EPT = 16;            // (anchor, class) elements per thread
constexpr int ML_EPB = ML_T * ML_EPT;  // elements per workgroup (4,096: also the LDS staging rows of ml_compact)
constexpr int ML_BINS = 1024;         // 10-bit digits
constexpr int ML_LEVELS = 6;          // 60 key bits
constexpr int ML_CH = 2048;           // keys per sort chunk
constexpr int ML_MAXCH = 16;          // sort chunks per image (cap <= 32,768 keys)

// the 60 significant bits of a pair's key: score bits (30) above the complemented pair index (30)
__device__ __forceinline__ unsigned long long ml_value(float score, unsigned idx) {
  return ((unsigned long long)(__float_as_uint(score) & 0x3FFFFFFFu) << 30) |
         (unsigned long long)((0xFFFFFFFFu - idx) & 0x3FFFFFFFu);
}

// element e of image b: its score and pair index, and whether it is a candidate at all
struct MlElem {
  bool cand;
  float score;
  unsigned idx;
};
__device__ __forceinline__ MlElem ml_elem(const MlArgs& a, int b, int e) {
  MlElem r;
  const int ai = ym_div(e, a.div_nc), c = e - ai * a.nc;
  const float l = a.anchors[((size_t)b * a.A + ai) * a.no_tot + a.cls_off + c];
  r.score = ym_sigmoid(l);
  r.idx = (unsigned)ai * 128u + (unsigned)c;
  r.cand = r.score > a.conf;
  if (r.cand && a.has_classes) {
    const unsigned w = c < 64 ? (c < 32 ? a.classes[0] : a.classes[1]) : (c < 96 ? a.classes[2] : a.classes[3]);
    r.cand = (w >> (c & 31)) & 1u;
  }
  return r;
}

// counts, histogram and selection state of this launch's images start from zero (decode_anchors has counted its
// single-label candidates into `counts`; in this mode the words hold the pair counts)
__global__ __launch_bounds__(NMS_T) void ml_init(const MlArgs a) {
  const int b = blockIdx.x, tid = threadIdx.x;
  for (int i = tid; i < ML_BINS; i += NMS_T) a.hist[(size_t)b * ML_BINS + i] = 0u;
  if (tid == 0) {
    a.counts[b] = 0;
    a.seln[b] = 0;
    MlState s;
    s.thr = 0ull; s.need = 0; s.done = 0; s.selcnt = 0; s.pad = 0;
    a.state[b] = s;
  }
}

__global__ __launch_bounds__(ML_T) void ml_hist(const MlArgs a, int level) {
  __shared__ unsigned lh[ML_BINS];
  __shared__ int lcnt;
  const int b = blockIdx.y, tid = threadIdx.x;
  const MlState st = a.state[b];
  if (st.done) return;  // (uniform: one image per workgroup)
  for (int i = tid; i < ML_BINS; i += ML_T) lh[i] = 0u;
  if (tid == 0) lcnt = 0;
  __syncthreads();
  const int total = a.A * a.nc;
  const int e0 = blockIdx.x * ML_EPB;
  const int pshift = 60 - 10 * level, dshift = 50 - 10 * level;
  int mine = 0;
#pragma unroll 4
  for (int it = 0; it < ML_EPT; ++it) {
    const int e = e0 + it * ML_T + tid;
    if (e >= total) break;
    const MlElem el = ml_elem(a, b, e);
    if (!el.cand) continue;
    ++mine;
    const unsigned long long v = ml_value(el.score, el.idx);
    if (level > 0 && (v >> pshift) != (st.thr >> pshift)) continue;
    atomicAdd(&lh[(unsigned)(v >> dshift) & (ML_BINS - 1)], 1u);
  }
  if (level == 0 && mine) atomicAdd(&lcnt, mine);
  __syncthreads();
  for (int i = tid; i < ML_BINS; i += ML_T)
    if (lh[i]) atomicAdd(&a.hist[(size_t)b * ML_BINS + i], lh[i]);
  if (level == 0 && tid == 0 && lcnt) atomicAdd(&a.counts[b], lcnt);
}

// one workgroup per image, thread t = bin t: the bin that holds the cut, i.e. S(t) < need <= S(t) + h(t) with S(t) the
// number of keys in the bins above t
__global__ __launch_bounds__(ML_BINS) void ml_pick(const MlArgs a, int level) {
  __shared__ unsigned s[ML_BINS];
  const int b = blockIdx.x, tid = threadIdx.x;
  const MlState st = a.state[b];
  if (st.done) return;
  const unsigned h = a.hist[(size_t)b * ML_BINS + tid];
  a.hist[(size_t)b * ML_BINS + tid] = 0u;  // the next level starts from zero
  const int n = a.counts[b];
  if (level == 0 && n <= a.max_nms) {  // no cut: every candidate is taken (thr 0)
    if (tid == 0) {
      MlState o = st;
      o.thr = 0ull; o.need = 0; o.done = 1;
      a.state[b] = o;
    }
    return;
  }
  const unsigned need = level == 0 ? (unsigned)a.max_nms : (unsigned)st.need;
  // inclusive suffix sums (Hillis-Steele over the reversed index)
  s[tid] = h;
  __syncthreads();
  for (int o = 1; o < ML_BINS; o <<= 1) {
    const unsigned add = tid + o < ML_BINS ? s[tid + o] : 0u;
    __syncthreads();
    s[tid] += add;
    __syncthreads();
  }
  const unsigned incl = s[tid], above = incl - h;
  if (above < need && need <= incl) {  // exactly one bin
    MlState o = st;
    o.thr = st.thr | ((unsigned long long)tid << (50 - 10 * level));
    o.need = (int)(need - above);
    // the whole bin is taken (always so at the last level: its bins are single keys): the cut is the bin's lower edge
    o.done = (need == incl || level == ML_LEVELS - 1) ? 1 : 0;
    a.state[b] = o;
  }
  if (tid == 0 && s[0] < need) {  // fewer matching keys than asked for (cannot follow from ml_hist's counts): take them all
    MlState o = st;
    o.done = 1;
    a.state[b] = o;
  }
}

__global__ __launch_bounds__(ML_T) void ml_compact(const MlArgs a) {
  __shared__ unsigned long long stage[ML_EPB];
  __shared__ int lcnt, gbase;
  const int b = blockIdx.y, tid = threadIdx.x;
  const unsigned long long thr = a.state[b].thr;
  if (tid == 0) lcnt = 0;
  __syncthreads();
  const int total = a.A * a.nc;
  const int e0 = blockIdx.x * ML_EPB;
#pragma unroll 4
  for (int it = 0; it < ML_EPT; ++it) {
    const int e = e0 + it * ML_T + tid;
    if (e >= total) break;
    const MlElem el = ml_elem(a, b, e);
    if (!el.cand || ml_value(el.score, el.idx) < thr) continue;
    const int slot = atomicAdd(&lcnt, 1);
    if (slot < ML_EPB)  // (a workgroup has ML_EPB elements)
      stage[slot] = ((unsigned long long)__float_as_uint(el.score) << 32) | (unsigned long long)(0xFFFFFFFFu - el.idx);
  }
  __syncthreads();
  const int cnt = lcnt < ML_EPB ? lcnt : ML_EPB;
  if (tid == 0 && cnt) gbase = atomicAdd(&a.state[b].selcnt, cnt);
  __syncthreads();
  if (!cnt) return;
  unsigned long long* sel = a.sel + (size_t)b * a.cap;
  for (int i = tid; i < cnt; i += ML_T) {
    const int slot = gbase + i;
    if (slot >= 0 && slot < a.cap) sel[slot] = stage[i];
  }
}

// keys selected for image b (what ml_compact stored)
__device__ __forceinline__ int ml_selected(const MlArgs& a, int b) {
  int m = a.state[b].selcnt;
  if (m > a.max_nms) m = a.max_nms;
  if (m > a.cap) m = a.cap;
  return m < 0 ? 0 : m;
}

__global__ __launch_bounds__(NMS_T) void ml_sort_chunks(const MlArgs a) {
  __shared__ unsigned long long k[ML_CH];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int m = ml_selected(a, b);
  if (c == 0 && tid == 0) a.seln[b] = m;
  if (c * ML_CH >= m) return;
  const unsigned long long* src = a.sel + (size_t)b * a.cap + c * ML_CH;
  const int mc = m - c * ML_CH;
  for (int i = tid; i < ML_CH; i += NMS_T) k[i] = i < mc ? src[i] : 0ull;  // padding 0: below every real key
  __syncthreads();
  bitonic_sort_desc(k, ML_CH, tid);
  unsigned long long* out = a.sel2 + (size_t)b * a.cap + c * ML_CH;  // (cap is a multiple of ML_CH)
  for (int i = tid; i < ML_CH; i += NMS_T) out[i] = k[i];
}

// Every key's final position: its index in its own chunk plus, per other chunk, the number of larger keys there (a
// binary search; descending order, keys unique, padding 0).  The other chunks pass through LDS one at a time, double
// buffered: a chunk's 16 KB arrive as one coalesced read per workgroup while the previous chunk is searched.  (Searching
// them in place in L2 — ~150 scattered 8-byte reads per key — took 112 us for 8 x 30,000 keys)
__global__ __launch_bounds__(NMS_T) void ml_sort_merge(const MlArgs a) {
  static_assert(ML_CH == 2 * NMS_T, "two keys per thread");
  __shared__ unsigned long long buf[2][ML_CH];
  const int b = blockIdx.y, c = blockIdx.x, tid = threadIdx.x;
  const int m = ml_selected(a, b);
  if (c * ML_CH >= m) return;  // (uniform)
  int nch = (m + ML_CH - 1) / ML_CH;
  if (nch > ML_MAXCH) nch = ML_MAXCH;
  const unsigned long long* src = a.sel2 + (size_t)b * a.cap;  // chunks 0 .. nch - 1 are written in full
  unsigned long long* dst = a.sel + (size_t)b * a.cap;
  const unsigned long long k0 = src[c * ML_CH + tid], k1 = src[c * ML_CH + tid + NMS_T];
  int r0 = tid, r1 = tid + NMS_T;
  int cur = c == 0 ? 1 : 0, pb = 0;
  unsigned long long p0 = 0ull, p1 = 0ull;
  if (cur < nch) {
    p0 = src[cur * ML_CH + tid];
    p1 = src[cur * ML_CH + tid + NMS_T];
  }
  while (cur < nch) {  // (uniform)
    buf[pb][tid] = p0;
    buf[pb][tid + NMS_T] = p1;
    int nxt = cur + 1;
    if (nxt == c) ++nxt;
    if (nxt < nch) {  // in flight while this chunk is searched
      p0 = src[nxt * ML_CH + tid];
      p1 = src[nxt * ML_CH + tid + NMS_T];
    }
    __syncthreads();  // buf[pb] complete; the other buffer's readers passed the previous barrier
    const unsigned long long* q = buf[pb];
    int lo0 = 0, hi0 = ML_CH, lo1 = 0, hi1 = ML_CH;  // the first index whose key is smaller
#pragma unroll 1
    for (int it = 0; it < 12; ++it) {  // 2^11 keys: both intervals are empty after 12 halvings
      const int m0 = (lo0 + hi0) >> 1, m1 = (lo1 + hi1) >> 1;
      const unsigned long long v0 = q[m0 < ML_CH ? m0 : ML_CH - 1], v1 = q[m1 < ML_CH ? m1 : ML_CH - 1];
      if (lo0 < hi0) {
        if (v0 > k0) lo0 = m0 + 1;
        else hi0 = m0;
      }
      if (lo1 < hi1) {
        if (v1 > k1) lo1 = m1 + 1;
        else hi1 = m1;
      }
    }
    r0 += lo0;
    r1 += lo1;
    cur = nxt;
    pb ^= 1;
  }
  // (the ranks of the m unique keys are a permutation of [0, m); padding keys are dropped)
  if (k0 != 0ull && r0 < m) dst[r0] = k0;
  if (k1 != 0ull && r1 < m) dst[r1] = k1;
}

// ------------------------------------------------------------------------------------------------- NMS
constexpr int MB_BLK = 256;    // candidates per block
constexpr int MB_KEEP = 1024;  // kept boxes in LDS: max_det up to this
constexpr int MB_NC = 128;     // classes of the class filter (and of the key's class field)
constexpr int MB_W = MB_BLK / 64;

// NmsArgs as nms_image takes them, except: keys = the sorted selected keys (kstride per image), counts = their
// number per image; scores / cls are unused (both come from the key); nm = 0.
__global__ __launch_bounds__(NMS_T) void nms_ml_image(const NmsArgs a) {
  __shared__ float4 bb[MB_BLK];                    // class-offset boxes of the block
  __shared__ float ba[MB_BLK];                     // areas
  __shared__ unsigned long long bkey[MB_BLK];      // keys
  __shared__ unsigned bsup[MB_BLK];                // removed flags
  __shared__ int bcls[MB_BLK];                     // the class list each joins
  __shared__ unsigned long long bmask[MB_BLK * MB_W];
  __shared__ unsigned long long ccm[MB_W * MB_NC];  // lanes of word w holding class c
  __shared__ float4 kb[MB_KEEP];                   // kept boxes
  __shared__ float ka[MB_KEEP];
  __shared__ int knext[MB_KEEP];                   // per-class kept lists
  __shared__ int khead[MB_NC];
  __shared__ int blk_keep[MB_BLK], blk_kept;
  __shared__ unsigned long long blk_rem[MB_W];
  constexpr int W = MB_W;
  const int b = blockIdx.x, tid = threadIdx.x;
  int ne = a.counts[b];
  if (ne > a.max_nms) ne = a.max_nms;
  if (ne > a.kstride) ne = a.kstride;
  if (ne < 0) ne = 0;
  const unsigned long long* gk = a.keys + (size_t)b * a.kstride;
  const size_t ib = (size_t)b * a.A;
  float* out = a.dets + (size_t)b * a.max_det * 6;
  // class filter: as nms_image's (exact when the class offsets separate every pair of boxes); otherwise every
  // candidate joins list 0 and is tested against every kept box
  const bool cf = !a.agnostic && a.iou >= 0.0 && (double)a.max_wh >= (double)a.img_w + (double)a.img_h + 2048.0;
  const int cap = a.max_det < MB_KEEP ? a.max_det : MB_KEEP;
  for (int i = tid; i < W * MB_NC; i += NMS_T) ccm[i] = 0ull;
  if (tid < MB_NC) khead[tid] = -1;
  __syncthreads();
  int kept = 0;  // uniform: every thread reads blk_kept after the block's barrier
  for (int b0 = 0; b0 < ne && kept < cap; b0 += MB_BLK) {
    const int nb = ne - b0 < MB_BLK ? ne - b0 : MB_BLK;
    if (tid < nb) {
      const unsigned long long key = gk[b0 + tid];
      const unsigned idx = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
      unsigned ai = idx >> 7;
      if (ai >= (unsigned)a.A) ai = 0;  // (a selected key always names an anchor of the image)
      const int cl = (int)(idx & 127u);
      const float4 v = a.boxes[ib + ai];
      const float off = a.agnostic ? 0.0f : (float)cl * a.max_wh;
      const float4 o = make_float4(v.x + off, v.y + off, v.z + off, v.w + off);
      bb[tid] = o;
      ba[tid] = __fmul_rn(__fsub_rn(o.z, o.x), __fsub_rn(o.w, o.y));
      bkey[tid] = key;
      const int c = cf ? cl : 0;
      bcls[tid] = c;
      if (cf) atomicOr(&ccm[(tid >> 6) * MB_NC + c], 1ull << (tid & 63));
    }
    if (tid < MB_BLK) bsup[tid] = tid >= nb;
    __syncthreads();
    if (tid < nb) {  // suppression by the boxes kept in earlier blocks (of this candidate's class list)
      bool sj = false;
      for (int q = khead[bcls[tid]]; q >= 0 && !sj; q = knext[q]) sj = iou_gt(kb[q], ka[q], bb[tid], ba[tid], a.iou);
      if (sj) bsup[tid] = 1u;
    }
    __syncthreads();
    {  // the survivors' bit matrix: wave item (i, w) tests row i against boxes 64 w .. 64 w + 63 (ballot = word w)
      const int wv = tid >> 6, ln = tid & 63;
      for (int pq = wv; pq < nb * W; pq += NMS_T / 64) {
        const int i = pq / W, w = pq - i * W;
        const int j = 64 * w + ln;
        const int lo = i + 1 - 64 * w;  // lanes >= lo lie past row i
        const unsigned long long past = lo <= 0 ? ~0ull : (lo >= 64 ? 0ull : ~0ull << lo);
        const int hiw = nb - 64 * w;    // lanes < hiw lie inside the block
        const unsigned long long in = hiw >= 64 ? ~0ull : (hiw <= 0 ? 0ull : ((1ull << hiw) - 1ull));
        const unsigned long long cand = (cf ? ccm[w * MB_NC + bcls[i]] : ~0ull) & past & in;
        unsigned long long bits = 0ull;
        if (!bsup[i] && cand) {  // (uniform)
          const bool sij = ((cand >> ln) & 1ull) && !bsup[j] && iou_gt(bb[i], ba[i], bb[j], ba[j], a.iou);
          bits = __ballot(sij);
        }
        if (ln == 0) bmask[pq] = bits;
      }
    }
    __syncthreads();
    if (tid < 64) {  // one wave: the block's greedy scan, removed words seeded by bsup
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
      for (int i = tid - 64; i < W * MB_NC; i += NMS_T - 64) ccm[i] = 0ull;
    }
    __syncthreads();
    const int kept2 = blk_kept;  // <= cap <= MB_KEEP; kept2 - kept <= nb <= MB_BLK
    for (int q = tid; q < kept2 - kept; q += NMS_T) {  // the block's kept boxes join their class lists; rows written
      const int r = blk_keep[q], idx = kept + q;
      kb[idx] = bb[r];
      ka[idx] = ba[r];
      knext[idx] = atomicExch(&khead[bcls[r]], idx);
      // the row, clipped as write_det does; score and class from the key
      const unsigned long long key = bkey[r];
      const unsigned pidx = 0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFull);
      unsigned ai = pidx >> 7;
      if (ai >= (unsigned)a.A) ai = 0;
      const float4 v = a.boxes[ib + ai];
      float* o = out + (size_t)idx * 6;
      o[0] = fminf(fmaxf(v.x, 0.f), a.img_w);
      o[1] = fminf(fmaxf(v.y, 0.f), a.img_h);
      o[2] = fminf(fmaxf(v.z, 0.f), a.img_w);
      o[3] = fminf(fmaxf(v.w, 0.f), a.img_h);
      o[4] = __uint_as_float((unsigned)(key >> 32));
      o[5] = (float)(pidx & 127u);
    }
    kept = kept2;
    __syncthreads();  // the kept lists are complete before the next block reads them; the block regions are free
  }
  if (tid == 0) {
    a.out_counts[b] = kept;
    if (a.counts2) a.counts2[b] = kept;
  }
}

}  // namespace

const void* ym_nms_ml_kernel() { return reinterpret_cast<const void*>(&nms_ml_image); }

// stop_after (YM_DBG_NMS 21 / 22, timing only): 21 = the candidate stage and the selection, 22 = + the sort
hipError_t ym_launch_nms_ml(const MlArgs& m0, const NmsArgs& n, hipStream_t st) {
  MlArgs m = m0;
  if (m.nc < 2 || m.nc > MB_NC || m.B < 1 || m.A < 1 || m.max_nms < 1 || m.cap < ML_CH || m.cap % ML_CH || m.cap > ML_MAXCH * ML_CH ||
      m.max_nms > m.cap || (long)m.A * 128 >= (1L << 30) || n.nm != 0 || n.max_det > MB_KEEP || n.kstride != m.cap)
    return hipErrorInvalidValue;
  m.div_nc = ym_fdiv(m.nc);
  const int dbg = ym_debug_get(YM_DBG_NMS);
  const dim3 ge(((long)m.A * m.nc + ML_EPB - 1) / ML_EPB, m.B);
  hipLaunchKernelGGL(ml_init, dim3(m.B), dim3(NMS_T), 0, st, m);
  for (int level = 0; level < ML_LEVELS; ++level) {
    hipLaunchKernelGGL(ml_hist, ge, dim3(ML_T), 0, st, m, level);
    hipLaunchKernelGGL(ml_pick, dim3(m.B), dim3(ML_BINS), 0, st, m, level);
  }
  hipLaunchKernelGGL(ml_compact, ge, dim3(ML_T), 0, st, m);
  if (dbg == 21) return hipGetLastError();
  const dim3 gs(m.cap / ML_CH, m.B);
  hipLaunchKernelGGL(ml_sort_chunks, gs, dim3(NMS_T), 0, st, m);
  hipLaunchKernelGGL(ml_sort_merge, gs, dim3(NMS_T), 0, st, m);
  if (dbg == 22) return hipGetLastError();
  hipLaunchKernelGGL(nms_ml_image, dim3(m.B), dim3(NMS_T), 0, st, n);
  return hipGetLastError();
}
