// C2PSA attention (+ the fused positional depthwise conv) on gfx950: a scalar kernel for any plan and shape, three MFMA
// kernels for the f16 / x3 plans, and the launcher that takes one by
// csrc/ym_op_select.h's rule.  int8 / fp8 plans: csrc/ym_conv_i8.hip.
#include <stdlib.h>

#include <type_traits>

#include "ym_common.h"
#include "ym_op_select.h"

namespace {

// ------------------------------------------------------------------------------------------------- attention
// C2PSA Attention, one workgroup = (image, head, QB queries):
//   1. S = (Q·Kᵀ)·kd^-½ for all N keys into LDS (each thread holds one key row in registers, Q is broadcast);
//   2. row softmax in LDS (max-subtracted exp, divide by the sum — as torch.softmax);
//   3. O = P·V: thread = (head dim d, group of QB/4 queries), V rows read coalesced (128 B per key);
//   4. + pe(v): depthwise 3x3 + folded BN on v (the `+ self.pe(v.reshape(B,C,H,W))` term), store.
constexpr int AKD = 32, AHD = 64;

// one element of an activation tensor (x3 pair storage: hi + lo of its chunk)
template <typename T> __device__ __forceinline__ float ld1(const T* p) {
  if constexpr (std::is_same<T, P2>::value) return ym_p2_get(p);
  else return (float)*p;
}
template <typename T> __device__ __forceinline__ void st1(T* p, float v) {
  if constexpr (std::is_same<T, P2>::value) ym_p2_set(p, v);
  else *p = (T)v;
}

template <typename T, int QB>
__global__ __launch_bounds__(256) void attn_psa(const AttnArgs a) {
  extern __shared__ float S[];  // [QB][N], then Q [QB][AKD]
  const int N = a.N;
  float* Qs = S + (size_t)QB * N;
  const int nqb = (N + QB - 1) / QB;
  const int vb = ym_xcd_block(blockIdx.x, gridDim.x);  // the query blocks of one (image, head) on one XCD
  const int qb = vb % nqb;
  const int bh = vb / nqb;
  const int h = bh % a.nh;
  const int b = bh / a.nh;
  const int tid = threadIdx.x;
  const int per = 2 * a.kd + a.hd;
  const T* qkv = static_cast<const T*>(a.qkv);
  const size_t img = (size_t)b * a.q_P;
  const int hq = a.q_coff + h * per;
  for (int i = tid; i < QB * AKD; i += 256) {
    const int r = i / AKD, c = i % AKD;
    const int n = qb * QB + r;
    Qs[i] = (n < N && c < a.kd) ? ld1(qkv + (img + n) * a.q_ctot + hq + c) : 0.f;
  }
  __syncthreads();
  // 1. scores
  for (int key = tid; key < N; key += 256) {
    float k[AKD];
    const T* kp = qkv + (img + key) * a.q_ctot + hq + a.kd;
#pragma unroll
    for (int c8 = 0; c8 < AKD / 8; ++c8) {
      const typename Vec8<T>::type v = Vec8<T>::load(kp + c8 * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) k[c8 * 8 + e] = (c8 * 8 + e < a.kd) ? (float)v[e] : 0.f;
    }
#pragma unroll 4
    for (int q = 0; q < QB; ++q) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < AKD; ++c) s = fmaf(Qs[q * AKD + c], k[c], s);
      S[q * N + key] = s * a.scale;
    }
  }
  __syncthreads();
  // 2. softmax: 256/QB threads per row
  {
    constexpr int TPR = 256 / QB;
    const int q = tid / TPR, sub = tid % TPR;
    float* row = S + (size_t)q * N;
    float m = -INFINITY;
    for (int j = sub; j < N; j += TPR) m = fmaxf(m, row[j]);
#pragma unroll
    for (int o = TPR / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
    float sum = 0.f;
    for (int j = sub; j < N; j += TPR) {
      const float e = expf(row[j] - m);
      row[j] = e;
      sum += e;
    }
#pragma unroll
    for (int o = TPR / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    for (int j = sub; j < N; j += TPR) row[j] = row[j] / sum;
  }
  __syncthreads();
  // 3. O = P·V
  constexpr int QPG = QB / 4;
  const int d = tid & 63, qg = tid >> 6;
  float o[QPG];
#pragma unroll
  for (int i = 0; i < QPG; ++i) o[i] = 0.f;
  const T* vp = qkv + img * a.q_ctot + hq + 2 * a.kd + d;
  float* Vs = Qs + QB * AKD;  // [64 keys][AHD] chunk of V, staged with 16-byte loads
  for (int k0 = 0; k0 < N; k0 += 64) {
    __syncthreads();
    {
      const int kk = tid >> 2, part = tid & 3;  // 64 keys x 4 quarters of 16 dims
      const int key = k0 + kk;
#pragma unroll
      for (int h8 = 0; h8 < 2; ++h8) {
        const int d0 = part * 16 + h8 * 8;
        typename Vec8<T>::type v = Vec8<T>::zero();
        if (key < N && d0 < a.hd) v = Vec8<T>::load(qkv + (img + key) * a.q_ctot + hq + 2 * a.kd + d0);
#pragma unroll
        for (int e = 0; e < 8; ++e) Vs[kk * AHD + d0 + e] = (float)v[e];
      }
    }
    __syncthreads();
    const int kn = N - k0 < 64 ? N - k0 : 64;
    for (int kj = 0; kj < kn; ++kj) {
      const float v = Vs[kj * AHD + d];
#pragma unroll
      for (int i = 0; i < QPG; ++i) o[i] = fmaf(S[(qg + 4 * i) * N + k0 + kj], v, o[i]);
    }
  }
  // 4. + pe(v), store
  if (d >= a.hd) return;
  const int ch = h * a.hd + d;
  T* dst = static_cast<T*>(a.dst);
#pragma unroll
  for (int i = 0; i < QPG; ++i) {
    const int n = qb * QB + qg + 4 * i;
    if (n >= N) continue;
    const int y = n / a.W, x = n - (n / a.W) * a.W;
    float pe = a.pe_b[ch];
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = y + ky - 1;
      if ((unsigned)iy >= (unsigned)a.H) continue;
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = x + kx - 1;
        if ((unsigned)ix >= (unsigned)a.W) continue;
        pe = fmaf(ld1(vp + (size_t)(iy * a.W + ix) * a.q_ctot), a.pe_w[(ky * 3 + kx) * a.C + ch], pe);
      }
    }
    st1(dst + ((size_t)b * a.d_P + n) * a.d_ctot + a.d_coff + ch, o[i] + pe);
    if (a.raw) a.raw[((size_t)b * N + n) * a.C + ch] = pe;  // f32 calibration run: pe(v) before the add
  }
}

// f16 plans, kd = 32 / hd = 64 (every YOLO11 scale) and N <= 512 tokens (inputs up to 724 px): the same Attention on
// MFMA.  One workgroup = (image, head, 64 queries), one wave = 16 queries:
//   1. K [N][32] and V^T [64][N] of the whole (image, head) are staged in LDS with every load in flight at once
//      (K rows padded to 80 bytes, V^T rows to 16 NKT + 4 halves: the fragment reads below spread over the banks);
//   2. S^T = K·Q^T: one v_mfma_f32_16x16x32_f16 per 16 keys (K = kd = 32), A = K rows from LDS, B = the wave's 16
//      query rows (one 16-byte load); the lane holds S^T[key 16t + 4(l>>4) + r][query l&15], all N keys in registers;
//   3. softmax over keys: in-lane over the tiles, then across the 4 lane groups (fp32, max-subtracted, v_exp_f32
//      on log2-scaled scores);
//   4. O^T = V^T·P^T, K = 32 keys per MFMA in the lane-group order of step 2 (slot j of group g is key
//      32s + 4g + j, or 32s + 16 + 4g + j - 4), so P comes straight from the softmax registers (rounded to fp16)
//      and V^T as two 8-byte LDS reads; a lane ends with 4 consecutive channels of one query: 8-byte NHWC stores;
//   5. + pe(v) (depthwise 3x3 + folded BN) from the staged V^T and LDS taps, store.
typedef _Float16 h8v __attribute__((ext_vector_type(8)));

// ---- steps the three MFMA kernels below share.  Each is used wherever every instantiation's assembly stays the same
// as with the step written out; the rest (img / hq and the lane's part of the coordinates, the score tile,
// attn_psa_mfma's sum, attn_psa_flash's MFMA chain, the + pe(v) epilogue) changes the schedule when factored, and is
// spelled out in the kernels.
// query block qb of head h of image b
struct AttnBlock { int qb, h, b; };
__device__ __forceinline__ AttnBlock attn_block(const AttnArgs& a) {
  const int nqb = (a.N + 63) / 64;
  const int vb = ym_xcd_block(blockIdx.x, gridDim.x);  // the query blocks of one (image, head) on one XCD
  const int bh = vb / nqb;
  return AttnBlock{vb % nqb, bh % a.nh, bh / a.nh};
}
// the max of a query's scores: in-lane over the tiles, then over the 4 lane groups that hold its keys
template <int NKT>
__device__ __forceinline__ float attn_row_max(const float (&s)[NKT][4]) {
  float m = -INFINITY;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) m = fmaxf(m, s[t][r]);
  m = fmaxf(m, __shfl_xor(m, 16));
  return fmaxf(m, __shfl_xor(m, 32));
}
// a query's sum over the lane groups
__device__ __forceinline__ float attn_group_sum(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}
// 8 keys of one V^T row as an MFMA operand: the lane group's 4 keys of two consecutive key tiles (two 8-byte LDS reads)
__device__ __forceinline__ h8v attn_vt_frag(const f16* vr) {
  const f16x4 lo = *reinterpret_cast<const f16x4*>(vr), hi = *reinterpret_cast<const f16x4*>(vr + 16);
  return h8v{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// this head's positional-conv taps [9][64] and bias [64] into LDS
__device__ __forceinline__ void attn_fill_pw(float* pw, const AttnArgs& a, int h, int tid) {
  for (int i = tid; i < 640; i += 256)
    pw[i] = i < 576 ? a.pe_w[(i >> 6) * a.C + h * 64 + (i & 63)] : a.pe_b[h * 64 + i - 576];
}
// one PV step: o += V^T fragment (row vh_row; X3: and its lo plane's vl_row) x P fragment, the split product in the
// order lo·hi, hi·lo, hi·hi (X3 false: pl and vl_row are unused)
template <bool X3>
__device__ __forceinline__ void attn_pv_step(f32x4& o, const f16* vh_row, const f16* vl_row, const h8v& ph,
                                             const h8v& pl) {
  const h8v vh = attn_vt_frag(vh_row);
  if constexpr (X3) {
    const h8v vl = attn_vt_frag(vl_row);
    o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o, 0, 0, 0);
    o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o, 0, 0, 0);
  }
  o = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o, 0, 0, 0);
}
// slot j of a P fragment from the fp32 weight p (X3: split hi / lo)
template <bool X3>
__device__ __forceinline__ void attn_split_p(h8v& ph, h8v& pl, int j, float p) {
  ph[j] = (f16)p;
  if constexpr (X3) pl[j] = (f16)(p - (float)ph[j]);
}

template <int NKT>  // key tiles of 16 (even): N <= 16 NKT
__global__ __launch_bounds__(256) void attn_psa_mfma(const AttnArgs a) {
  // LDS: V^T [64][LDV] f16, K [16 NKT][LDK] f16, pe weights [9][64] + bias [64] f32
  extern __shared__ __attribute__((aligned(16))) f16 vt[];
  constexpr int LDV = 16 * NKT + 4;
  // 96-byte K rows (6 16-byte slots): the 16-row x 4-chunk fragment reads hit distinct slots in each of ds_read_b128's
  // non-contiguous lane groups (MI355X_MICROARCH §LDS); 80-byte rows were 2-way there
  constexpr int LDK = 48;
  f16* kl = vt + 64 * LDV;
  float* pw = reinterpret_cast<float*>(kl + 16 * NKT * LDK);
  const int N = a.N;
  const auto [qb, h, b] = attn_block(a);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const f16* qkv = static_cast<const f16*>(a.qkv);
  const size_t img = (size_t)b * a.q_P;
  const int hq = a.q_coff + h * 128;  // per head: q 32, k 32, v 64 channels
  // 1. K and V^T of the (image, head) into LDS (keys >= N zero), this head's positional-conv taps and bias
  attn_fill_pw(pw, a, h, tid);
  {  // all loads in flight before the first LDS store (one memory latency, not NIT): 12 chunks of 8 per key
    constexpr int NIT = (16 * NKT * 12 + 255) / 256;
    f16x8 v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 256 * it, key = i / 12, ch = i - key * 12;
      v[it] = key < N ? Vec8<f16>::load(qkv + (img + key) * a.q_ctot + hq + 32 + 8 * ch) : Vec8<f16>::zero();
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 256 * it, key = i / 12, ch = i - key * 12;
      if (key >= 16 * NKT) break;
      if (ch < 4) {
        *reinterpret_cast<f16x8*>(kl + key * LDK + 8 * ch) = v[it];
      } else {
        const int d0 = 8 * (ch - 4);
#pragma unroll
        for (int e = 0; e < 8; ++e) vt[(d0 + e) * LDV + key] = v[it][e];
      }
    }
  }
  const int q = qb * 64 + wave * 16 + c;
  h8v qf = Vec8<f16>::zero();
  if (q < N) qf = Vec8<f16>::load(qkv + (img + q) * a.q_ctot + hq + 8 * g);
  __syncthreads();
  // 2. scores, in log2 units (scale·log2 e folded in: softmax by exp2)
  const float sl2 = a.scale * 1.4426950408889634f;
  float s[NKT][4];
#pragma unroll
  for (int t = 0; t < NKT; ++t) {
    const h8v kf = *reinterpret_cast<const h8v*>(kl + (16 * t + c) * LDK + 8 * g);
    const f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) s[t][r] = 16 * t + 4 * g + r < N ? d[r] * sl2 : -INFINITY;
  }
  // 3. softmax over the keys of query l&15
  const float m = attn_row_max<NKT>(s);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[t][r] = __builtin_amdgcn_exp2f(s[t][r] - m);  // v_exp_f32 (~1 ulp; P is rounded to fp16 below)
      sum += s[t][r];
    }
  sum += __shfl_xor(sum, 16);  // (attn_group_sum here changes this kernel's schedule)
  sum += __shfl_xor(sum, 32);
  const float rs = 1.0f / sum;
  // 4. O^T = V^T P^T
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < NKT / 2; ++ks) {
    h8v pf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      attn_split_p<false>(pf, pf, r, s[2 * ks][r] * rs);
      attn_split_p<false>(pf, pf, 4 + r, s[2 * ks + 1][r] * rs);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const f16* vr = vt + (16 * dt + c) * LDV + 32 * ks + 4 * g;
      attn_pv_step<false>(o[dt], vr, vr, pf, pf);
    }
  }
  // 5. + pe(v), store: lane = channels 16dt + 4g .. +3 of query q
  if (q >= N) return;
  const int y = q / a.W, x = q - (q / a.W) * a.W;
  f16* dst = static_cast<f16*>(a.dst) + ((size_t)b * a.d_P + q) * a.d_ctot + a.d_coff + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const int d0 = 16 * dt + 4 * g;
    float pe[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pe[r] = pw[576 + d0 + r];
#pragma unroll
    for (int t = 0; t < 9; ++t) {  // taps in (ky, kx) order; out-of-image taps skipped, as the zero-padded conv
      const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
      if ((unsigned)iy >= (unsigned)a.H || (unsigned)ix >= (unsigned)a.W) continue;
      const int nb = iy * a.W + ix;
      const f32x4 w = *reinterpret_cast<const f32x4*>(pw + 64 * t + d0);
#pragma unroll
      for (int r = 0; r < 4; ++r) pe[r] = fmaf((float)vt[(d0 + r) * LDV + nb], w[r], pe[r]);
    }
    f16x4 out;
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = (f16)(o[dt][r] + pe[r]);
    *reinterpret_cast<f16x4*>(dst + d0) = out;
  }
}

// x3 plans, kd = 32 / hd = 64, N <= 512 tokens: attn_psa_mfma's structure on the pair layout, every product split
// (hi·hi + lo·hi + hi·lo on v_mfma_f32_16x16x32_f16, fp32 accumulation).  V^T of the (image, head) is staged in LDS
// as hi and lo planes (the two planes of K as well would not fit beside them), K fragments stream from global
// (32 bytes = the [hi | lo] pair of one key chunk per lane and key tile; L2-resident), P is split in registers.
template <int NKT, int KB>
__global__ __launch_bounds__(256) void attn_psa_x3(const AttnArgs a) {
  extern __shared__ __attribute__((aligned(16))) f16 vt[];  // [2][64][LDV]: V^T hi, lo; then pe weights + bias f32
  constexpr int LDV = 16 * NKT + 4;
  f16* vtl = vt + 64 * LDV;
  float* pw = reinterpret_cast<float*>(vtl + 64 * LDV);
  const int N = a.N;
  const auto [qb, h, b] = attn_block(a);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const P2* qkv = static_cast<const P2*>(a.qkv);
  const size_t img = (size_t)b * a.q_P;
  const int hq = a.q_coff + h * 128;  // per head: q 32, k 32, v 64 logical channels
  attn_fill_pw(pw, a, h, tid);
  // 1. V^T hi / lo planes (keys >= N zero): 8 chunks of 8 v channels per key.  Every chunk load is in flight
  // before the first LDS store (one memory latency, not NIT of them: the loop form waited for each load in turn)
  {
    constexpr int NIT = 16 * NKT * 8 / 256;
    static_assert(16 * NKT * 8 % 256 == 0, "V chunks divide over the threads");
    HL v[NIT];
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 256 * it, key = i >> 3, ch = i & 7;
      // (an unconditional load of a clamped key, zeroed below: a load under a condition is waited for on the spot)
      v[it] = ym_load_hl(qkv + (img + (key < N ? key : N - 1)) * a.q_ctot + hq + 64 + 8 * ch);
    }
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
      const int i = tid + 256 * it, key = i >> 3, ch = i & 7;
      const bool ok = key < N;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        vt[(8 * ch + e) * LDV + key] = ok ? v[it].hi[e] : (f16)0;
        vtl[(8 * ch + e) * LDV + key] = ok ? v[it].lo[e] : (f16)0;
      }
    }
  }
  const int q = qb * 64 + wave * 16 + c;
  // (queries past N: a clamped row; their outputs are never stored)
  const HL qf = ym_load_hl(qkv + (img + (q < N ? q : N - 1)) * a.q_ctot + hq + 8 * g);
  // 2. scores S^T = K·Q^T (log2 units): lane (g, c) supplies key 16t + c, logical chunk g of K.  The K fragments
  // of KB key tiles are loaded together (unconditional loads of clamped keys: rows past N only feed scores that are
  // masked to -inf), then their MFMAs run: NKT / KB memory round trips instead of one per tile (KB = NKT: one; the
  // kernel runs one wave per SIMD, so the registers are there)
  const float sl2 = a.scale * 1.4426950408889634f;
  float s[NKT][4];
#pragma unroll
  for (int t0 = 0; t0 < NKT; t0 += KB) {
    HL kf[KB];
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      const int key = 16 * (t0 + u) + c;
      if (t0 + u < NKT) kf[u] = ym_load_hl(qkv + (img + (key < N ? key : N - 1)) * a.q_ctot + hq + 32 + 8 * g);
    }
#pragma unroll
    for (int u = 0; u < KB; ++u) {
      const int t = t0 + u;
      if (t >= NKT) break;
      f32x4 d = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[u].lo, qf.hi, f32x4{0.f, 0.f, 0.f, 0.f}, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[u].hi, qf.lo, d, 0, 0, 0);
      d = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[u].hi, qf.hi, d, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) s[t][r] = 16 * t + 4 * g + r < N ? d[r] * sl2 : -INFINITY;
    }
  }
  __syncthreads();
  // 3. softmax over the keys of query l&15 (fp32, exact exp2)
  const float m = attn_row_max<NKT>(s);
  float sum = 0.f;
#pragma unroll
  for (int t = 0; t < NKT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      s[t][r] = exp2f(s[t][r] - m);
      sum += s[t][r];
    }
  sum = attn_group_sum(sum);
  const float rs = 1.0f / sum;
  // 4. O^T = V^T P^T, K = 32 keys per MFMA in the lane-group order of step 2 (as attn_psa_mfma), P split hi / lo
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int ks = 0; ks < NKT / 2; ++ks) {
    h8v ph, pl;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      attn_split_p<true>(ph, pl, r, s[2 * ks][r] * rs);
      attn_split_p<true>(ph, pl, 4 + r, s[2 * ks + 1][r] * rs);
    }
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const int row = (16 * dt + c) * LDV + 32 * ks + 4 * g;
      attn_pv_step<true>(o[dt], vt + row, vtl + row, ph, pl);
    }
  }
  // 5. + pe(v) (v = hi + lo from LDS), store in the pair layout: lane = channels 16dt + 4g .. +3 of query q
  if (q >= N) return;
  const int y = q / a.W, x = q - (q / a.W) * a.W;
  P2* dst = static_cast<P2*>(a.dst) + ((size_t)b * a.d_P + q) * a.d_ctot + a.d_coff + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const int d0 = 16 * dt + 4 * g;
    float pe[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pe[r] = pw[576 + d0 + r];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
      if ((unsigned)iy >= (unsigned)a.H || (unsigned)ix >= (unsigned)a.W) continue;
      const int nb = iy * a.W + ix;
      const f32x4 w = *reinterpret_cast<const f32x4*>(pw + 64 * t + d0);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        pe[r] = fmaf((float)vt[(d0 + r) * LDV + nb] + (float)vtl[(d0 + r) * LDV + nb], w[r], pe[r]);
    }
    float out[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = o[dt][r] + pe[r];
    ym_p2_store4(dst + d0, out);
  }
}

// Any N (the 1280² input: 1600 tokens, core/validator.py:188): the MFMA attention with the keys in blocks of 256
// and an online softmax (running max / sum per query, O rescaled when the max grows), so neither the scores nor
// V^T of the whole (image, head) need to fit: per block, V^T (f16, or hi / lo planes for x3) is staged in LDS, K
// fragments stream from global; pe(v) reads its 3x3 taps from global.  X3: every product split as in attn_psa_x3.
template <bool X3>
__global__ __launch_bounds__(256) void attn_psa_flash(const AttnArgs a) {
  constexpr int KB = 256, NKT = KB / 16, LDV = KB + 4;
  typedef typename std::conditional<X3, P2, f16>::type T;
  extern __shared__ __attribute__((aligned(16))) f16 vt[];  // [X3 ? 2 : 1][64][LDV]
  f16* vtl = vt + 64 * LDV;
  const int N = a.N;
  const auto [qb, h, b] = attn_block(a);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, c = lane & 15;
  const T* qkv = static_cast<const T*>(a.qkv);
  const size_t img = (size_t)b * a.q_P;
  const int hq = a.q_coff + h * 128;  // per head: q 32, k 32, v 64 channels
  auto frag = [&](const T* p) -> HL {  // 8 channels of one token (hi and, for x3, lo)
    if constexpr (X3) return ym_load_hl(p);
    else return HL{Vec8<f16>::load(p), Vec8<f16>::zero()};
  };
  const int q = qb * 64 + wave * 16 + c;
  HL qf{Vec8<f16>::zero(), Vec8<f16>::zero()};
  if (q < N) qf = frag(qkv + (img + q) * a.q_ctot + hq + 8 * g);
  const float sl2 = a.scale * 1.4426950408889634f;
  float m = -INFINITY, l = 0.f;  // running max (log2 units) and this lane's partial sum of its query's weights
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += KB) {
    __syncthreads();  // every wave is done with the previous block's V^T
    for (int i = tid; i < KB * 8; i += 256) {
      const int key = i >> 3, ch = i & 7;
      HL v{Vec8<f16>::zero(), Vec8<f16>::zero()};
      if (k0 + key < N) v = frag(qkv + (img + k0 + key) * a.q_ctot + hq + 64 + 8 * ch);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        vt[(8 * ch + e) * LDV + key] = v.hi[e];
        if constexpr (X3) vtl[(8 * ch + e) * LDV + key] = v.lo[e];
      }
    }
    float s[NKT][4];
#pragma unroll
    for (int t = 0; t < NKT; ++t) {
      const int key = k0 + 16 * t + c;
      HL kf{Vec8<f16>::zero(), Vec8<f16>::zero()};
      if (key < N) kf = frag(qkv + (img + key) * a.q_ctot + hq + 32 + 8 * g);
      f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (X3) {
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf.lo, qf.hi, d, 0, 0, 0);
        d = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf.hi, qf.lo, d, 0, 0, 0);
      }
      d = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf.hi, qf.hi, d, 0, 0, 0);
#pragma unroll
      for (int r = 0; r < 4; ++r) s[t][r] = k0 + 16 * t + 4 * g + r < N ? d[r] * sl2 : -INFINITY;
    }
    const float mb = attn_row_max<NKT>(s);
    const float mn = fmaxf(m, mb);
    const float sc = exp2f(m - mn);  // 0 on the first block (m = -inf)
    m = mn;
    l *= sc;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] *= sc;
#pragma unroll
    for (int t = 0; t < NKT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[t][r] = exp2f(s[t][r] - mn);
        l += s[t][r];
      }
    __syncthreads();  // this block's V^T is staged
#pragma unroll
    for (int ks = 0; ks < NKT / 2; ++ks) {
      h8v ph, pl;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        attn_split_p<X3>(ph, pl, r, s[2 * ks][r]);
        attn_split_p<X3>(ph, pl, 4 + r, s[2 * ks + 1][r]);
      }
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        const int row = (16 * dt + c) * LDV + 32 * ks + 4 * g;
        const h8v vh = attn_vt_frag(vt + row);  // (attn_pv_step here changes attn_psa_flash<true>'s schedule)
        if constexpr (X3) {
          const h8v vl = attn_vt_frag(vtl + row);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph, o[dt], 0, 0, 0);
          o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl, o[dt], 0, 0, 0);
        }
        o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph, o[dt], 0, 0, 0);
      }
    }
  }
  l = attn_group_sum(l);
  const float rs = 1.0f / l;
  if (q >= N) return;
  const int y = q / a.W, x = q - (q / a.W) * a.W;
  T* dst = static_cast<T*>(a.dst) + ((size_t)b * a.d_P + q) * a.d_ctot + a.d_coff + h * 64;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    const int d0 = 16 * dt + 4 * g;
    float pe[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) pe[r] = a.pe_b[h * 64 + d0 + r];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
      if ((unsigned)iy >= (unsigned)a.H || (unsigned)ix >= (unsigned)a.W) continue;
      const T* vp = qkv + (img + iy * a.W + ix) * a.q_ctot + hq + 64 + d0;
      float v[4];
      if constexpr (X3) {
        ym_p2_load4(vp, v);
      } else {
        const f16x4 hv = *reinterpret_cast<const f16x4*>(vp);
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = (float)hv[r];
      }
      const f32x4 w = *reinterpret_cast<const f32x4*>(a.pe_w + t * a.C + h * 64 + d0);
#pragma unroll
      for (int r = 0; r < 4; ++r) pe[r] = fmaf(v[r], w[r], pe[r]);
    }
    float out[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) out[r] = o[dt][r] * rs + pe[r];
    if constexpr (X3) {
      ym_p2_store4(dst + d0, out);
    } else {
      *reinterpret_cast<f16x4*>(dst + d0) = f16x4{(f16)out[0], (f16)out[1], (f16)out[2], (f16)out[3]};
    }
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------- launchers
hipError_t ym_launch_attn(int dtype, const AttnArgs& a, hipStream_t st, int* variant) {
  if (ym_dt_q8(dtype)) return ym_launch_attn_i8(a, st, dtype == YM_DT_F8);
  // YM_ATTN_FLASH_OFF=1 (tests): N > 512 tokens on the scalar kernel
  static const bool flash_off = [] { const char* e = getenv("YM_ATTN_FLASH_OFF"); return e && *e == '1'; }();
  const int code = ym_select_attn(dtype, a.N, a.B, a.nh, a.kd, a.hd, a.raw != nullptr, a.q_ctot, a.q_coff, a.d_ctot,
                                  a.d_coff, flash_off);
  if (code < 0) return hipErrorInvalidValue;
  static_assert(AKD == YM_ATTN_KD && AHD == YM_ATTN_HD, "the rule sizes the scalar kernel's LDS");
  const dim3 g64(a.B * a.nh * ((a.N + 63) / 64));  // the MFMA kernels: 64 queries per workgroup
  const size_t pw_bytes = 640 * sizeof(float);
  auto scalar = [&](auto qb) {
    constexpr int QB = decltype(qb)::value;
    ym_with_type(dtype, [&](auto t) {
      hipLaunchKernelGGL((attn_psa<typename decltype(t)::type, QB>), dim3(a.B * a.nh * ((a.N + QB - 1) / QB)), dim3(256),
                         ym_attn_scalar_lds(QB, a.N), st, a);
    });
  };
  auto mfma = [&](auto nkt) {
    constexpr int NKT = decltype(nkt)::value;
    const size_t lds = ((size_t)64 * (16 * NKT + 4) + (size_t)16 * NKT * 48) * sizeof(f16) + pw_bytes;
    hipLaunchKernelGGL((attn_psa_mfma<NKT>), g64, dim3(256), lds, st, a);
  };
  auto x3 = [&](auto nkt) {
    constexpr int NKT = decltype(nkt)::value;
    const size_t lds = (size_t)2 * 64 * (16 * NKT + 4) * sizeof(f16) + pw_bytes;
    // K fragments of every key tile in flight at once (up to 26 tiles); YM_DBG_ATTN_KB = 1: 8 tiles per round trip
    constexpr int KBALL = NKT <= 26 ? NKT : 16;
    if (ym_debug_get(YM_DBG_ATTN_KB) == 1) hipLaunchKernelGGL((attn_psa_x3<NKT, 8>), g64, dim3(256), lds, st, a);
    else hipLaunchKernelGGL((attn_psa_x3<NKT, KBALL>), g64, dim3(256), lds, st, a);
  };
  const size_t flash_lds = (size_t)64 * (256 + 4) * sizeof(f16);  // one V^T plane of a key block
  typedef std::integral_constant<int, 4> i4;
  typedef std::integral_constant<int, 8> i8t;
  typedef std::integral_constant<int, 16> i16;
  typedef std::integral_constant<int, 26> i26;
  typedef std::integral_constant<int, 32> i32;
  switch (code) {
    case YM_ATTNV_SCALAR_QB4: scalar(i4()); break;
    case YM_ATTNV_SCALAR_QB4 + 1: scalar(i8t()); break;
    case YM_ATTNV_SCALAR_QB4 + 2: scalar(i16()); break;
    case YM_ATTNV_SCALAR_QB4 + 3: scalar(i32()); break;
    case YM_ATTNV_MFMA_NKT8: mfma(i8t()); break;
    case YM_ATTNV_MFMA_NKT8 + 1: mfma(i16()); break;
    case YM_ATTNV_MFMA_NKT8 + 2: mfma(i26()); break;
    case YM_ATTNV_MFMA_NKT8 + 3: mfma(i32()); break;
    case YM_ATTNV_X3_NKT8: x3(i8t()); break;
    case YM_ATTNV_X3_NKT8 + 1: x3(i16()); break;
    case YM_ATTNV_X3_NKT8 + 2: x3(i26()); break;
    case YM_ATTNV_X3_NKT8 + 3: x3(i32()); break;
    case YM_ATTNV_FLASH_F16: hipLaunchKernelGGL(attn_psa_flash<false>, g64, dim3(256), flash_lds, st, a); break;
    case YM_ATTNV_FLASH_X3: hipLaunchKernelGGL(attn_psa_flash<true>, g64, dim3(256), 2 * flash_lds, st, a); break;
    default: return hipErrorInvalidValue;
  }
  if (variant) *variant = code;
  return hipGetLastError();
}
