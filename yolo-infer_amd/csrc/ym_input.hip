// The forward's first kernel on gfx950: the input statistics (LoadTensor's /255 rule) with the per-forward counter
// reset, and the profiling spin kernel.
#include "ym_common.h"

namespace {

// ------------------------------------------------------------------------------------------------- input stats
// LoadTensor._single_check: `if im.max() > 1 + finfo(dtype).eps: im = im.float() / 255` over the WHOLE batch.
// ctl[0] holds max as an order-preserving int (ym_input_max reads the YM_CTL_SLOTS slots).
// The division itself happens in the stem conv's loader (csrc/ym_stem.hip), which reads the NCHW batch.
//
// input_stats: the forward's first kernel, one launch.  Every block zeroes its share of the per-image candidate
// counts and the split-K tile counters (csrc/ym_conv_dma.hip; self-resetting, cleared here as a guard against an
// aborted forward), reduces a contiguous chunk of the batch to its max and stores it write-through (sc1) into its
// partial slot; after its `vmcnt(0)` one lane takes an agent-scope ticket, and the block whose ticket is last
// reduces the partials (sc1 loads: the hand-off of MI355X_MICROARCH §inter-workgroup visibility, first table row),
// writes the slots and resets the ticket.  The ticket is two-level: block b counts on group ticket b % 16 and the
// last block of each group on the top ticket — same-address agent-scope atomics serialise at ~10 ns each, so one
// ticket for 1,024 blocks cost ~10 us of the kernel's ~28 (tools/probe_input_stats.hip, profiles/r06j_input_stats.txt:
// 27.9 -> 20.3 us in isolation, 17.9 with no ticket at all).  No per-forward init kernel, no same-address atomicMax storm.  The ticket
// starts at zero (ensure_workspace zeroes the arena it lives in), and a launch can only stop part-way through a device
// fault, which ends the context: a stale ticket cannot carry into a later forward.
// batch_max non-null (multi-GPU shard): the slots take the given global max, x is not read.
constexpr int kStatsBlocks = 1024;  // partial slots (ym_runtime.cpp reserves them behind the ctl slots)
constexpr int kStatsU = 10;         // float4 loads in flight per lane and round
__global__ __launch_bounds__(256) void input_stats(const float* __restrict__ x, long n, float* ctl, int* counts, int B,
                                                   int* cnt, int cnt_len, const float* batch_max) {
  const int tid = threadIdx.x;
  const long gt = blockIdx.x * 256L + tid, gstride = (long)gridDim.x * 256;
  for (long b = gt; b < B; b += gstride) counts[b] = 0;
  int4* c4 = reinterpret_cast<int4*>(cnt);
  for (long i = gt; i < cnt_len / 4; i += gstride) c4[i] = make_int4(0, 0, 0, 0);
  int* slots = reinterpret_cast<int*>(ctl);
  if (batch_max) {
    if (blockIdx.x == 0 && tid < YM_CTL_SLOTS) slots[tid * YM_CTL_STRIDE] = tid == 0 ? f2ord(*batch_max) : f2ord(-INFINITY);
    return;
  }
  int* part = slots + YM_CTL_SLOTS * YM_CTL_STRIDE + 64;  // [kStatsBlocks], after the ticket's 256-byte line
  int* ticket = slots + YM_CTL_SLOTS * YM_CTL_STRIDE;
  int* gticket = part + kStatsBlocks;                     // [YM_STATS_GROUPS][32]
  // contiguous chunk of whole float4s per block; every round issues kStatsU 16-byte loads per lane at once, the
  // indices past the chunk clamped onto its last float4 (a duplicate cannot change a max), so there is no
  // predicated or remainder load: at B = 8, 640² (2400 float4 per block) the whole chunk is ONE round trip
  const long n4 = n >> 2;
  const long per = (n4 + gridDim.x - 1) / gridDim.x;
  const long lo = blockIdx.x * per, hi = lo + per < n4 ? lo + per : n4;
  const f32x4* x4 = reinterpret_cast<const f32x4*>(x);
  float m = -INFINITY;
  for (long i = lo + tid; lo < hi && i - tid < hi; i += kStatsU * 256) {
    f32x4 v[kStatsU];
#pragma unroll
    for (int u = 0; u < kStatsU; ++u) {
      const long j = i + u * 256;
      v[u] = x4[j < hi ? j : hi - 1];  // (plain loads: the stem reads the batch next)
    }
#pragma unroll
    for (int u = 0; u < kStatsU; ++u) m = fmaxf(m, fmaxf(fmaxf(v[u][0], v[u][1]), fmaxf(v[u][2], v[u][3])));
  }
  if (blockIdx.x == 0)
    for (long j = (n4 << 2) + tid; j < n; j += 256) m = fmaxf(m, x[j]);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
  __shared__ float wm[4];
  __shared__ int last;
  if ((tid & 63) == 0) wm[tid >> 6] = m;
  __syncthreads();
  if (tid == 0) {
    m = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    // the sc1 hand-off (cdna_hip_programming.md Guideline 16, MI355X_MICROARCH.md § visibility, the counter row):
    // the partial is stored write-through (an agent-scope relaxed store is sc1) and drained before the agent-scope
    // ticket; the last block reads every partial with sc1 loads (agent-scope relaxed loads), so neither side needs a
    // fence instruction.  (An acquire-release ticket puts an L2 write-back in every one of the 1,024 blocks: the
    // kernel went 21.8 -> 52.8 us per call under rocprofv3: profiles/r04d_s_b8_x3_summary.json vs r05c.)
    __hip_atomic_store(part + blockIdx.x, f2ord(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int g = blockIdx.x % YM_STATS_GROUPS, ng = ((int)gridDim.x - g + YM_STATS_GROUPS - 1) / YM_STATS_GROUPS;
    const int t = __hip_atomic_fetch_add(gticket + 32 * g, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    int l = 0;
    if (t == ng - 1) {  // the group's last block: its count is complete, so every partial of the group is stored
      __hip_atomic_store(gticket + 32 * g, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const int u = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      l = u == min((int)gridDim.x, YM_STATS_GROUPS) - 1;
    }
    last = l;
  }
  __syncthreads();
  if (!last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");  // no instruction: keeps the sc1 loads below the ticket
  int r = f2ord(-INFINITY);
  for (int b = tid; b < (int)gridDim.x; b += 256)
    r = max(r, __hip_atomic_load(part + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) r = max(r, __shfl_xor(r, o));
  __shared__ int wr[4];
  if ((tid & 63) == 0) wr[tid >> 6] = r;
  __syncthreads();
  if (tid < YM_CTL_SLOTS)
    slots[tid * YM_CTL_STRIDE] = tid == 0 ? max(max(wr[0], wr[1]), max(wr[2], wr[3])) : f2ord(-INFINITY);
  if (tid == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ void ctl_to_max(const float* ctl, float* out) {
  if (threadIdx.x == 0) *out = ym_input_max(ctl);
}

// ------------------------------------------------------------------------------------------------- profiling aid
// One wave parks for `ticks` of the constant 100 MHz wall clock.  ym_profile queues it ahead of the per-op event
// pairs so the host enqueues the whole forward while the GPU waits: the events then time device work only, not host
// launch latency.  Always terminates (bounded by the clock, not by memory state).
__global__ void spin_wait(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}

}  // namespace

// ------------------------------------------------------------------------------------------------- launchers
hipError_t ym_launch_spin(int usec, hipStream_t st) {
  if (usec < 0) usec = 0;
  if (usec > 200000) usec = 200000;
  hipLaunchKernelGGL(spin_wait, dim3(1), dim3(64), 0, st, (long long)usec * 100);
  return hipGetLastError();
}

hipError_t ym_launch_prep(int dtype, const PrepArgs& a, int* counts, int B, hipStream_t st) {
  (void)dtype;
  // one launch: counters cleared, batch max reduced (or the given global max taken) — input_stats above
  const long n = (long)a.B * a.C * a.H * a.W;
  long blocks = a.batch_max ? 64 : (n / 4 + 2047) / 2048;  // >= 8 float4 per lane
  if (blocks > kStatsBlocks) blocks = kStatsBlocks;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(input_stats, dim3(blocks), dim3(256), 0, st, a.in, n, a.ctl, counts, B, a.cnt, a.cnt_len,
                     a.batch_max);
  return hipGetLastError();
}

hipError_t ym_launch_input_max(const float* x, long n, float* ctl, float* out, hipStream_t st) {
  long blocks = (n / 4 + 2047) / 2048;
  if (blocks > kStatsBlocks) blocks = kStatsBlocks;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(input_stats, dim3(blocks), dim3(256), 0, st, x, n, ctl, nullptr, 0, nullptr, 0, nullptr);
  hipLaunchKernelGGL(ctl_to_max, dim3(1), dim3(64), 0, st, ctl, out);
  return hipGetLastError();
}
