// COCO run-length encoding of mask planes (Masks.rle): four launches per call.
//
//   strips   one workgroup per (plane, strip).  The strip's bytes are read along rows, a lane taking 4 columns (one
//            aligned 4-byte read a row; 1 column when the plane does not allow it) over the 32 rows of a word, so a wave
//            reads 256 consecutive bytes of a row, and leaves column bit words in LDS.  Every lane then walks a
//            contiguous piece of the strip's words (ym_rle_walk: transitions = bits ^ (bits << 1 | carry), positions by
//            count-trailing-zeros) into an RleAgg, the pieces are joined by a scan in LDS, and the strip's summary, its
//            set pixels and (only when it has transitions) its words go to the scratch.
//   join     one workgroup per plane: the exclusive scan of the strip summaries with ym_rle_join, the plane's summary
//            and its area.
//   offsets  one workgroup: the two int64 prefix sums over the planes (runs, string bytes), and each plane's last
//            count (the run that reaches H * W), which no transition starts.
//   write    one workgroup per (plane, strip), gone at once for a strip without transitions or a plane that does not
//            fit: the words come back from the scratch (1 / 8 of the plane; of the bytes only the one pixel before the
//            strip is read again), the same walk and scan give every lane the plane prefix before its piece (rank of
//            its first run, where its bytes start, the three positions before it), and the lane writes its counts
//            and byte groups.
//
// Order is fixed by the scans alone: no atomic places anything (the area is an integer sum).
#include <hip/hip_runtime.h>

#include "ym_rle.h"

namespace {

struct RleArgs {
  const unsigned char* masks;
  long long plane_stride;
  int n;
  RleGeom g;
  RleScratch ws;
  uint32_t* counts;
  long long cap_counts;
  unsigned char* bytes;
  long long cap_bytes;
  long long* run_offsets;
  long long* byte_offsets;
  long long* area;
};

// The inclusive scan of one RleAgg per lane, in place in LDS; returns the lane's exclusive value.
__device__ RleAgg scan_aggs(RleAgg* sc, const RleAgg& mine) {
  const int tid = threadIdx.x;
  sc[tid] = mine;
  __syncthreads();
  for (int off = 1; off < kRleThreads; off <<= 1) {
    RleAgg left = {};
    if (tid >= off) left = sc[tid - off];
    __syncthreads();
    if (tid >= off) sc[tid] = ym_rle_join(left, sc[tid]);
    __syncthreads();
  }
  RleAgg before = {};
  if (tid > 0) before = sc[tid - 1];
  return before;
}

// The lane's piece of `total` items: contiguous, of an odd length (LDS banks).
__device__ void piece(int total, int& l0, int& l1) {
  const int per = ((total + kRleThreads - 1) / kRleThreads) | 1;
  l0 = min((int)threadIdx.x * per, total);
  l1 = min(l0 + per, total);
}

// Byte plane -> column bit words of one strip.  V columns a lane.
template <int V>
__device__ void pack_strip(uint32_t* bits, const unsigned char* plane, const RleGeom& g, const RleStrip& s) {
  const int groups = (s.cols + V - 1) / V, items = groups * s.rows;
  for (int it = threadIdx.x; it < items; it += kRleThreads) {
    const int jj = it / groups, cx = (it % groups) * V;
    const int y0 = 32 * (s.j0 + jj), rows = min(32, g.H - y0);
    const unsigned char* at = plane + (long long)y0 * g.W + s.x0 + cx;
    uint32_t w[V] = {};
#pragma unroll 8
    for (int r = 0; r < rows; ++r) {
      if (V == 4) {
        const uint32_t q = *reinterpret_cast<const uint32_t*>(at + (long long)r * g.W);
#pragma unroll
        for (int c = 0; c < 4; ++c) w[c] |= ((q >> (8 * c)) & 0xffu ? 1u : 0u) << r;
      } else {
        w[0] |= (at[(long long)r * g.W] ? 1u : 0u) << r;
      }
    }
#pragma unroll
    for (int c = 0; c < V; ++c)
      if (cx + c < s.cols) bits[(cx + c) * s.rows + jj] = w[c];
  }
}

// The pixel before the strip: one byte of the plane, read by lane 0 alone (the walk uses it for word 0 only).
__device__ uint32_t strip_carry(const unsigned char* plane, const RleGeom& g, const RleStrip& s) {
  const long long at = ym_rle_strip_pred(g, s);
  return threadIdx.x == 0 && at >= 0 && plane[at] ? 1u : 0u;
}

__global__ __launch_bounds__(kRleThreads) void rle_strips(const RleArgs a) {
  __shared__ uint32_t bits[kRleLdsWords];
  __shared__ RleAgg sc[kRleThreads];
  __shared__ int set;
  const RleGeom g = a.g;
  const long long flat = blockIdx.x;
  const int m = (int)(flat / g.strips);
  const RleStrip s = ym_rle_strip(g, (int)(flat % g.strips));
  const unsigned char* plane = a.masks + (long long)m * a.plane_stride;
  if (threadIdx.x == 0) set = 0;
  // (a 4-byte read needs the plane, its rows and the strip's first column aligned, and whole groups of 4 columns)
  const bool vec = ((reinterpret_cast<uintptr_t>(plane) | (uintptr_t)g.W | (uintptr_t)s.x0 | (uintptr_t)s.cols) & 3) == 0;
  if (vec) pack_strip<4>(bits, plane, g, s);
  else pack_strip<1>(bits, plane, g, s);
  __syncthreads();
  int l0, l1;
  piece(s.words, l0, l1);
  RleAgg mine = {};
  ym_rle_walk(bits, g, s, l0, l1, strip_carry(plane, g, s), [&](int p) { ym_rle_push(mine, p); });
  int ones = 0;
  for (int l = l0; l < l1; ++l) ones += __popc(bits[l]);
  if (ones) atomicAdd(&set, ones);
  scan_aggs(sc, mine);
  const RleAgg all = sc[kRleThreads - 1];
  if (threadIdx.x == 0) {
    a.ws.own[flat] = all;
    a.ws.set[flat] = set;
  }
  if (all.runs == 0) return;
  uint32_t* out = a.ws.words + flat * ((long long)g.CS * g.JS);
  for (int l = threadIdx.x; l < s.words; l += kRleThreads) out[l] = bits[l];
}

__global__ __launch_bounds__(kRleThreads) void rle_join(const RleArgs a) {
  __shared__ RleAgg sc[kRleThreads];
  __shared__ int set;
  const int m = blockIdx.x, S = a.g.strips;
  const RleAgg* own = a.ws.own + (long long)m * S;
  RleAgg* prefix = a.ws.prefix + (long long)m * S;
  if (threadIdx.x == 0) set = 0;
  __syncthreads();
  int s0, s1;
  piece(S, s0, s1);
  RleAgg mine = {};
  int ones = 0;
  for (int s = s0; s < s1; ++s) {
    mine = ym_rle_join(mine, own[s]);
    ones += a.ws.set[(long long)m * S + s];
  }
  if (ones) atomicAdd(&set, ones);
  RleAgg run = scan_aggs(sc, mine);
  for (int s = s0; s < s1; ++s) {
    prefix[s] = run;
    run = ym_rle_join(run, own[s]);
  }
  if (threadIdx.x == 0) {
    a.ws.total[m] = sc[kRleThreads - 1];
    a.area[m] = set;
  }
}

constexpr int kRleScanThreads = 1024;

__global__ __launch_bounds__(kRleScanThreads) void rle_offsets(const RleArgs a) {
  __shared__ long long runs[kRleScanThreads], bytes[kRleScanThreads];
  __shared__ long long base_runs, base_bytes;
  const int tid = threadIdx.x, hw = a.g.H * a.g.W;
  if (tid == 0) {
    base_runs = base_bytes = 0;
    a.run_offsets[0] = a.byte_offsets[0] = 0;
  }
  __syncthreads();
  for (int c = 0; c < a.n; c += kRleScanThreads) {
    const int i = c + tid;
    RleAgg t = {};
    int before = 0;  // the string bytes of plane i's counts but the last
    long long r = 0, b = 0;
    if (i < a.n) {
      t = a.ws.total[i];
      before = ym_rle_prefix_bytes(t);
      r = t.runs + 1;
      b = before + ym_rle_group_len(ym_rle_value(t, hw));
    }
    runs[tid] = r;
    bytes[tid] = b;
    __syncthreads();
    for (int off = 1; off < kRleScanThreads; off <<= 1) {
      const long long vr = tid >= off ? runs[tid - off] : 0, vb = tid >= off ? bytes[tid - off] : 0;
      __syncthreads();
      runs[tid] += vr;
      bytes[tid] += vb;
      __syncthreads();
    }
    if (i < a.n) {
      const long long r1 = base_runs + runs[tid], b1 = base_bytes + bytes[tid];
      a.run_offsets[i + 1] = r1;
      a.byte_offsets[i + 1] = b1;
      if (a.counts && r1 <= a.cap_counts) a.counts[r1 - 1] = (uint32_t)ym_rle_count(t, hw);
      if (a.bytes && b1 <= a.cap_bytes) ym_rle_group(ym_rle_value(t, hw), a.bytes + (b1 - b) + before);
    }
    __syncthreads();
    if (tid == 0) {
      base_runs += runs[kRleScanThreads - 1];
      base_bytes += bytes[kRleScanThreads - 1];
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(kRleThreads) void rle_write(const RleArgs a) {
  __shared__ uint32_t bits[kRleLdsWords];
  __shared__ RleAgg sc[kRleThreads];
  const RleGeom g = a.g;
  const long long flat = blockIdx.x;
  const int m = (int)(flat / g.strips);
  if (a.ws.own[flat].runs == 0) return;  // nothing starts here: the strip is not read again
  uint32_t* counts = a.counts && a.run_offsets[m + 1] <= a.cap_counts ? a.counts + a.run_offsets[m] : nullptr;
  unsigned char* bytes = a.bytes && a.byte_offsets[m + 1] <= a.cap_bytes ? a.bytes + a.byte_offsets[m] : nullptr;
  if (!counts && !bytes) return;  // the caller sees the totals above its capacities and calls again
  const RleStrip s = ym_rle_strip(g, (int)(flat % g.strips));
  const uint32_t* in = a.ws.words + flat * ((long long)g.CS * g.JS);
  for (int l = threadIdx.x; l < s.words; l += kRleThreads) bits[l] = in[l];
  __syncthreads();
  const uint32_t carry = strip_carry(a.masks + (long long)m * a.plane_stride, g, s);
  int l0, l1;
  piece(s.words, l0, l1);
  RleAgg mine = {};
  ym_rle_walk(bits, g, s, l0, l1, carry, [&](int p) { ym_rle_push(mine, p); });
  RleAgg e = ym_rle_join(a.ws.prefix[flat], scan_aggs(sc, mine));
  if (mine.runs == 0) return;
  int at = ym_rle_prefix_bytes(e);
  ym_rle_walk(bits, g, s, l0, l1, carry, [&](int p) {
    if (counts) counts[e.runs] = (uint32_t)ym_rle_count(e, p);
    const int x = ym_rle_value(e, p);
    at += ym_rle_group(x, bytes ? bytes + at : nullptr);
    ym_rle_advance(e, p);
  });
}

}  // namespace

hipError_t ym_launch_rle(const unsigned char* masks, long long plane_stride, int n, const RleGeom& g, const RleScratch& ws,
                         uint32_t* counts, long long cap_counts, unsigned char* bytes, long long cap_bytes,
                         long long* run_offsets, long long* byte_offsets, long long* area, hipStream_t st) {
  const RleArgs a{masks, plane_stride, n, g, ws, counts, cap_counts, bytes, cap_bytes, run_offsets, byte_offsets, area};
  const unsigned blocks = (unsigned)((long long)n * g.strips);
  if (n > 0) {
    hipLaunchKernelGGL(rle_strips, dim3(blocks), dim3(kRleThreads), 0, st, a);
    hipLaunchKernelGGL(rle_join, dim3(n), dim3(kRleThreads), 0, st, a);
  }
  hipLaunchKernelGGL(rle_offsets, dim3(1), dim3(kRleScanThreads), 0, st, a);
  if (n > 0 && (cap_counts > 0 || cap_bytes > 0)) hipLaunchKernelGGL(rle_write, dim3(blocks), dim3(kRleThreads), 0, st, a);
  return hipGetLastError();
}
