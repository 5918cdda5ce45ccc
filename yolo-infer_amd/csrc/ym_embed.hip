// Feature embeddings: global average pooling of plan buffers, all requested views of a call in one launch (plus one
// finishing launch when a view spans more than one pixel chunk).  Layer 22 at 640² is 400 pixels per image: the stage
// is bound by launch and load latency, not bandwidth, so there is no launch per layer.
//
// The reduction is a tree with a fixed shape and order (no floating-point atomics), so a result is bit-identical from
// call to call and between eager launches and graph replays:
//   embed_pool    a workgroup owns (view, image, chunk of kEmbedChunk = 512 pixels, tile of 64 channels); thread
//                 (cg = tid & 7, pl = tid >> 3) adds the pixels pl, pl + 32, ... of its 8 channels: <= kEmbedIter = 16
//                 additions; the 8 pixel lanes of a wave fold by 3 xor-shuffles; the 4 waves' partials meet in LDS as
//                 (w0 + w1) + (w2 + w3): 2 additions.  A view of one chunk is divided and stored here.
//   embed_finish  per (view, image, 32 channels): chunk lane j = tid >> 5 adds the partials of chunks j, j + 8, ...:
//                 ceil(nch / 8) additions; the 8 lanes meet in LDS as a 3-level tree.
// Longest chain of dependent fp32 additions for one output over P pixels, nch = ceil(P / 512):
//   k(P) = min(16, ceil(min(P, 512) / 32)) + 3 + 2                      nch == 1
//   k(P) = 16 + 3 + 2 + ceil(nch / 8) + 3                                nch > 1
// (6 at P = 1, 18 at P = 400, 31 at P = 25,600, 49 at P = 102,400).  The mean is that sum divided by (float)P: one
// correctly rounded fp32 division (P < 2^24 is exact in fp32).  An x3 value is float(hi) + float(lo), as
// Engine.read_buffer forms it.
#include "ym_embed.h"

namespace {

template <typename T>
__device__ __forceinline__ void embed_accumulate(const EmbedDesc& d, int b, int p0, int p1, int pl, int c, float* acc) {
  const T* base = static_cast<const T*>(d.ptr) + ((size_t)b * d.P) * d.pitch + d.coff + c;
#pragma unroll 4
  for (int p = p0 + pl; p < p1; p += kEmbedPL) {
    const typename Vec8<T>::type v = Vec8<T>::load(base + (size_t)p * d.pitch);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += (float)v[e];
  }
}

__global__ __launch_bounds__(kEmbedThreads) void embed_pool(const EmbedArgs a) {
  __shared__ float red[kEmbedThreads / YM_WAVE][kEmbedCG * 8];
  const int blk = blockIdx.x, tid = threadIdx.x;
  int v = 0;
  while (v + 1 < a.n && blk >= a.d[v + 1].blk0) ++v;  // (uniform; at most kEmbedMaxViews steps)
  const EmbedDesc& d = a.d[v];
  const int ntile = (d.C + 63) >> 6;
  int r = blk - d.blk0;
  const int tile = r % ntile;
  r /= ntile;
  const int chunk = r % d.nch, b = r / d.nch;
  const int cg = tid & (kEmbedCG - 1), pl = tid >> 3;
  const int c = tile * 64 + cg * 8;
  const int p0 = chunk * kEmbedChunk;
  const int p1 = p0 + kEmbedChunk < d.P ? p0 + kEmbedChunk : d.P;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (b < a.B && c < d.C) {  // (C % 8 == 0: a channel group is inside the view or outside it)
    if (d.mode == YM_EMB_F16) embed_accumulate<f16>(d, b, p0, p1, pl, c, acc);
    else if (d.mode == YM_EMB_X3) embed_accumulate<P2>(d, b, p0, p1, pl, c, acc);
    else embed_accumulate<float>(d, b, p0, p1, pl, c, acc);
  }
  // the wave's 8 pixel lanes (lane bits 3..5)
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    acc[e] += __shfl_xor(acc[e], 8);
    acc[e] += __shfl_xor(acc[e], 16);
    acc[e] += __shfl_xor(acc[e], 32);
  }
  const int lane = tid & (YM_WAVE - 1), wave = tid >> 6;
  if (lane < kEmbedCG) {
#pragma unroll
    for (int e = 0; e < 8; ++e) red[wave][lane * 8 + e] = acc[e];
  }
  __syncthreads();
  if (tid < 64) {
    const float s = (red[0][tid] + red[1][tid]) + (red[2][tid] + red[3][tid]);
    const int co = tile * 64 + tid;
    if (b < a.B && co < d.C) {
      if (d.nch == 1) a.out[(size_t)b * a.ld + d.col + co] = __fdiv_rn(s, (float)d.P);
      else a.part[d.poff + ((size_t)b * d.nch + chunk) * d.C + co] = s;
    }
  }
}

__global__ __launch_bounds__(kEmbedThreads) void embed_finish(const EmbedArgs a) {
  __shared__ float red[kEmbedFinL][kEmbedFinC];
  const int blk = blockIdx.x, tid = threadIdx.x;
  int v = 0;
  while (v + 1 < a.n && blk >= a.d[v].fblk0 + a.d[v].fblk_n) ++v;  // (views of one chunk have no workgroup here)
  const EmbedDesc& d = a.d[v];
  const int ntile = (d.C + kEmbedFinC - 1) / kEmbedFinC;
  const int r = blk - d.fblk0;
  const int tile = r % ntile, b = r / ntile;
  const int o = tid & (kEmbedFinC - 1), j = tid >> 5;
  const int co = tile * kEmbedFinC + o;
  const bool ok = r >= 0 && r < d.fblk_n && b < a.B && co < d.C;
  float acc = 0.f;
  if (ok) {
    const float* p = a.part + d.poff + (size_t)b * d.nch * d.C + co;
    for (int ch = j; ch < d.nch; ch += kEmbedFinL) acc += p[(size_t)ch * d.C];
  }
  red[j][o] = acc;
  __syncthreads();
  if (tid < kEmbedFinC && ok) {
    const float s = ((red[0][o] + red[1][o]) + (red[2][o] + red[3][o])) + ((red[4][o] + red[5][o]) + (red[6][o] + red[7][o]));
    a.out[(size_t)b * a.ld + d.col + co] = __fdiv_rn(s, (float)d.P);
  }
}

// the launch geometry of a validated table: chunk counts, workgroup ranges, partial offsets; false: invalid table
bool embed_layout(EmbedArgs& a, long& blocks, long& fblocks, long& part) {
  if (a.n < 1 || a.n > kEmbedMaxViews || a.B < 1 || a.ld < 1) return false;
  blocks = fblocks = part = 0;
  for (int i = 0; i < a.n; ++i) {
    EmbedDesc& d = a.d[i];
    if (!d.ptr || d.P < 1 || d.P >= (1 << 24) || d.C < 8 || d.C % 8 || d.coff < 0 || d.coff % 8 || d.pitch % 8 ||
        d.coff + d.C > d.pitch || d.col < 0 || (long)d.col + d.C > a.ld || d.mode < YM_EMB_F32 || d.mode > YM_EMB_X3)
      return false;
    d.nch = (d.P + kEmbedChunk - 1) / kEmbedChunk;
    d.blk0 = (int)blocks;
    blocks += (long)a.B * d.nch * ((d.C + 63) / 64);
    d.fblk0 = (int)fblocks;
    d.fblk_n = 0;
    d.poff = part;
    if (d.nch > 1) {
      d.fblk_n = a.B * ((d.C + kEmbedFinC - 1) / kEmbedFinC);
      fblocks += d.fblk_n;
      part += (long)a.B * d.nch * d.C;
    }
    if (blocks > (1L << 30) || fblocks > (1L << 30)) return false;
  }
  return true;
}

}  // namespace

long ym_embed_part_floats(const EmbedArgs& a0) {
  EmbedArgs a = a0;
  long blocks, fblocks, part;
  return embed_layout(a, blocks, fblocks, part) ? part : -1;
}

hipError_t ym_launch_embed(const EmbedArgs& a0, hipStream_t st) {
  EmbedArgs a = a0;
  long blocks, fblocks, part;
  if (!a.out || !embed_layout(a, blocks, fblocks, part) || (part > 0 && !a.part)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(embed_pool, dim3((unsigned)blocks), dim3(kEmbedThreads), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || fblocks == 0) return e;
  hipLaunchKernelGGL(embed_finish, dim3((unsigned)fblocks), dim3(kEmbedThreads), 0, st, a);
  return hipGetLastError();
}
