// The Classify head of a yolo11-cls plan on gfx950: conv 1x1 -> SiLU -> global mean, Linear, softmax + top-k, as three
// launches behind layer 9.  Every intermediate and output value is fp32; there are no floating-point atomics and every
// reduction is a tree of fixed shape and order, so a result is bit-identical from call to call and between eager
// launches and graph replays.
//
//   cls_pool      (launch 1) the conv as a GEMM per image, D[n][m] = sum_k W[n][k] X[k][m] with n = head channel (MFMA
//                 rows), m = pixel (MFMA columns), K = c1, on v_mfma_f32_32x32x16_f16 (f16 plans: one per 16 K; x3
//                 plans: three on the stored hi / lo split, lo.hi, hi.lo, hi.hi as the conv kernels order them, the
//                 weight scale undone by ym_x3_pre) or v_mfma_f32_32x32x2_f32 (f32 plans).  A workgroup owns (image, 64
//                 channels) and walks the image's pixels 64 at a time; wave (wn = w & 1, wp = w >> 1) holds the 32 x 32
//                 tile of channels 32 wn.. and pixels 32 wp.. of the pass.  K streams through LDS in stages of 64: the
//                 64 weight rows and the 64 pixel rows of a stage, rows padded by 8 elements (x3: an fp16 hi and an fp16
//                 lo plane each) — 18 KB (f16) or 36 KB (x3, f32) whatever c1 is.  The epilogue adds the bias, applies
//                 the plan's SiLU, zeroes the columns beyond the image's P pixels (SiLU(bias) of a padded column is not
//                 zero), folds the 32 pixel lanes by 5 xor-shuffles and adds the result to the wave's running sums;
//                 the two pixel waves meet in LDS, and the sum is divided once by (float)P (__fdiv_rn).  The
//                 1280-channel map never leaves the registers.
//   cls_linear    (launch 2) logits[b][j] = bias[j] + sum_k W[j][k] pooled[b][k]: bound by reading W.  A workgroup owns
//                 8 classes, a wave two of them: lane l keeps W[j][4 l + 256 i + e] (i < 5, e < 4; 16-byte loads) in
//                 registers and serves every image from that one read, the pooled vectors staged through LDS in groups
//                 of 8 images (40 KB).  Per image a lane runs 20 fmaf, the 64 lanes fold by 6 xor-shuffles, the bias is
//                 added last.
//   cls_softmax   (launch 3) one workgroup per image: the row max (NaN ignored), e = expf(x - max) summed per thread
//                 over classes t, t + 256, ..., the 64 lanes by 6 xor-shuffles, the 4 waves as (w0 + w1) + (w2 + w3);
//                 probs = __fdiv_rn(e, sum) (a correctly rounded division, not a reciprocal).  Then k = min(5, nc) rounds
//                 of an arg-max over the keys (prob bits << 32 | ~class): descending probability, equal probabilities
//                 to the lower class, a NaN probability as key value 0 so it never wins.  topk_conf is read back from
//                 the stored probs.
//
// Longest chain of dependent fp32 additions of each reduction (an fmaf counts as one):
//   pixels of one channel, P pixels:    k_pool(P) = 5 + ceil(ceil(P / 32) / 2) + 1     (7 at P = 1 and 49, 13 at 400)
//   the 1280 terms of one logit:        k_lin     = 20 + 6 + 1 = 27
//   the nc terms of the softmax sum:    k_sm(nc)  = ceil(nc / 256) + 6 + 2             (12 at nc = 1000, 9 at nc <= 256)
#include <type_traits>

#include "ym_classify.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

namespace {

constexpr int kPitch = kClsKC + 8;  // LDS row pitch in elements: rows 16-byte aligned, fragment reads spread over banks

// Storage type T of the plan (f16, P2 pair layout, float): LDS element, planes per operand, global bytes per logical K
template <typename T> struct Stage {
  typedef f16 elem;
  static constexpr int planes = 1;
};
template <> struct Stage<P2> {
  typedef f16 elem;
  static constexpr int planes = 2;
};
template <> struct Stage<float> {
  typedef float elem;
  static constexpr int planes = 1;
};

// 64 rows x one K stage, global -> LDS with 16-byte loads; a row beyond `nrows` is zeros.  row(r): the row's first byte.
template <typename T, typename RowF>
__device__ __forceinline__ void stage_rows(typename Stage<T>::elem (*s)[64][kPitch], int nrows, size_t koff, RowF row) {
  typedef typename Stage<T>::elem E;
  constexpr int NV = kClsKC * (int)sizeof(T) / 16;  // 16-byte vectors of a row's stage: 8 (f16) or 16
#pragma unroll
  for (int v = threadIdx.x; v < 64 * NV; v += kClsThreads) {
    const int r = v / NV, j = v - r * NV;
    uint4 d = uint4{0u, 0u, 0u, 0u};
    if (r < nrows) d = *reinterpret_cast<const uint4*>(row(r) + koff + (size_t)j * 16);
    E* dst;
    if constexpr (std::is_same<T, P2>::value) dst = &s[j & 1][r][(j >> 1) * 8];  // [hi x8 | lo x8] -> the two planes
    else dst = &s[0][r][j * (16 / (int)sizeof(E))];
    *reinterpret_cast<uint4*>(dst) = d;
  }
}

template <typename T>
__device__ __forceinline__ void mma_stage(const typename Stage<T>::elem (*sw)[64][kPitch],
                                          const typename Stage<T>::elem (*sx)[64][kPitch], int wrow, int xrow, int h,
                                          f32x16& acc) {
#pragma unroll
  for (int ks = 0; ks < kClsKC / 16; ++ks) {
    const int k = ks * 16 + 8 * h;  // lane half h holds K 8h .. 8h + 7 of the 16-deep step, on both operands
    if constexpr (std::is_same<T, float>::value) {
      const f32x8 a = Vec8<float>::load(&sw[0][wrow][k]), b = Vec8<float>::load(&sx[0][xrow][k]);
#pragma unroll
      for (int s = 0; s < 8; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s], b[s], acc, 0, 0, 0);
    } else if constexpr (std::is_same<T, P2>::value) {
      const HL a{Vec8<f16>::load(&sw[0][wrow][k]), Vec8<f16>::load(&sw[1][wrow][k])};
      const HL b{Vec8<f16>::load(&sx[0][xrow][k]), Vec8<f16>::load(&sx[1][xrow][k])};
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.lo, b.hi, acc, 0, 0, 0);  // the small cross terms first
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.hi, b.lo, acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(a.hi, b.hi, acc, 0, 0, 0);
    } else {
      acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(Vec8<f16>::load(&sw[0][wrow][k]), Vec8<f16>::load(&sx[0][xrow][k]),
                                                   acc, 0, 0, 0);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kClsThreads) void cls_pool(const ClsArgs a) {
  typedef typename Stage<T>::elem E;
  constexpr int NP = Stage<T>::planes;
  constexpr size_t WB = std::is_same<T, float>::value ? 4 : 2;  // bytes of a weight storage element
  __shared__ __attribute__((aligned(16))) E sw[NP][64][kPitch];
  __shared__ __attribute__((aligned(16))) E sx[NP][64][kPitch];
  __shared__ float red[2][kClsBN];
  const int tiles_n = (kClsHidden + kClsBN - 1) / kClsBN;
  const int b = blockIdx.x / tiles_n, tn = blockIdx.x - b * tiles_n;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wn = wave & 1, wp = wave >> 1, l32 = lane & 31, h = lane >> 5;
  const int n0 = tn * kClsBN;
  const int wrows = kClsHidden - n0 < kClsBN ? kClsHidden - n0 : kClsBN;
  const char* wbase = static_cast<const char*>(a.w) + (size_t)n0 * a.kpad * WB;
  const char* xbase = static_cast<const char*>(a.x) + ((size_t)b * a.P * a.ctot + a.coff) * sizeof(T);
  const size_t wpitch = (size_t)a.kpad * WB, xpitch = (size_t)a.ctot * sizeof(T);
  const int nkc = a.C1 / kClsKC;

  // this lane's 16 channels: n0 + 32 wn + 8 q + 4 h + e (accumulator register 4 q + e), of pixel column l32
  float bias[16];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int n = n0 + wn * 32 + 8 * q + 4 * h;
    const f32x4 b4 = n < kClsHidden ? *reinterpret_cast<const f32x4*>(a.bias + n) : f32x4{0, 0, 0, 0};
#pragma unroll
    for (int e = 0; e < 4; ++e) bias[4 * q + e] = b4[e];
  }
  float csum[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) csum[r] = 0.f;

  for (int p0 = 0; p0 < a.P; p0 += kClsBM) {
    const int xrows = a.P - p0 < kClsBM ? a.P - p0 : kClsBM;
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    for (int kc = 0; kc < nkc; ++kc) {
      const size_t koff = (size_t)kc * kClsKC * sizeof(T);  // (a pair row stores 4 bytes per logical K as P2 does)
      __syncthreads();  // the previous stage's fragment reads
      stage_rows<T>(sw, wrows, koff, [&](int r) { return wbase + (size_t)r * wpitch; });
      stage_rows<T>(sx, xrows, koff, [&](int r) { return xbase + (size_t)(p0 + r) * xpitch; });
      __syncthreads();
      mma_stage<T>(sw, sx, wn * 32 + l32, wp * 32 + l32, h, acc);
    }
    const bool pix_ok = p0 + wp * 32 + l32 < a.P;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      float x, v;
      if constexpr (std::is_same<T, P2>::value) {
        x = ym_x3_pre(acc[r], a.wsc, bias[r]);
        v = ym_silu_x3(x);
      } else if constexpr (std::is_same<T, f16>::value) {
        x = acc[r] + bias[r];
        v = ym_silu_fast(x);
      } else {
        x = acc[r] + bias[r];
        v = ym_silu(x);
      }
      v = pix_ok ? v : 0.f;  // after the activation: a padded column holds SiLU(bias)
      v += __shfl_xor(v, 1);
      v += __shfl_xor(v, 2);
      v += __shfl_xor(v, 4);
      v += __shfl_xor(v, 8);
      v += __shfl_xor(v, 16);
      csum[r] += v;
    }
  }
  if (l32 == 0) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[wp][wn * 32 + 8 * (r >> 2) + 4 * h + (r & 3)] = csum[r];
  }
  __syncthreads();
  if (threadIdx.x < kClsBN && n0 + (int)threadIdx.x < kClsHidden)
    a.pooled[(size_t)b * kClsHidden + n0 + threadIdx.x] =
        __fdiv_rn(red[0][threadIdx.x] + red[1][threadIdx.x], (float)a.P);
}

template <typename WT>
__global__ __launch_bounds__(kClsThreads) void cls_linear(const ClsArgs a) {
  constexpr int NI = kClsHidden / 256;  // 16-byte vectors of a row per lane
  static_assert(kClsHidden % 256 == 0, "a wave covers a weight row in whole 4-element vectors");
  __shared__ __attribute__((aligned(16))) float sp[kClsLinG][kClsHidden];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = blockIdx.x * kClsLinCT + wave * 2;
  f32x4 w[2][NI];
#pragma unroll
  for (int c = 0; c < 2; ++c)
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      w[c][i] = f32x4{0, 0, 0, 0};
      if (j0 + c < a.nc) {
        const WT* p = static_cast<const WT*>(a.lw) + (size_t)(j0 + c) * kClsHidden + 4 * lane + 256 * i;
        if constexpr (std::is_same<WT, float>::value) {
          w[c][i] = *reinterpret_cast<const f32x4*>(p);
        } else {
          const f16x4 v = *reinterpret_cast<const f16x4*>(p);
          w[c][i] = f32x4{(float)v[0], (float)v[1], (float)v[2], (float)v[3]};
        }
      }
    }
  for (int g0 = 0; g0 < a.B; g0 += kClsLinG) {
    const int ng = a.B - g0 < kClsLinG ? a.B - g0 : kClsLinG;
    __syncthreads();  // the previous group's reads
    const f32x4* src = reinterpret_cast<const f32x4*>(a.pooled + (size_t)g0 * kClsHidden);
    for (int v = threadIdx.x; v < ng * (kClsHidden / 4); v += kClsThreads) reinterpret_cast<f32x4*>(&sp[0][0])[v] = src[v];
    __syncthreads();
    for (int g = 0; g < ng; ++g) {
      float acc[2] = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < NI; ++i) {
        const f32x4 x = *reinterpret_cast<const f32x4*>(&sp[g][4 * lane + 256 * i]);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          acc[0] = fmaf(w[0][i][e], x[e], acc[0]);
          acc[1] = fmaf(w[1][i][e], x[e], acc[1]);
        }
      }
#pragma unroll
      for (int c = 0; c < 2; ++c) {
#pragma unroll
        for (int o = 1; o < YM_WAVE; o <<= 1) acc[c] += __shfl_xor(acc[c], o);
        if (lane == 0 && j0 + c < a.nc) a.logits[(size_t)(g0 + g) * a.nc + j0 + c] = acc[c] + a.lb[j0 + c];
      }
    }
  }
}

__global__ __launch_bounds__(kClsThreads) void cls_softmax(const ClsArgs a) {
  __shared__ float sf[kClsThreads / YM_WAVE];
  __shared__ unsigned long long sk[kClsThreads / YM_WAVE];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const float* x = a.logits + (size_t)b * a.nc;
  float* p = a.probs + (size_t)b * a.ld;
  float m = -INFINITY;
  for (int j = tid; j < a.nc; j += kClsThreads) m = fmaxf(m, x[j]);  // (fmaxf drops a NaN operand)
#pragma unroll
  for (int o = 1; o < YM_WAVE; o <<= 1) m = fmaxf(m, __shfl_xor(m, o));
  if (lane == 0) sf[wave] = m;
  __syncthreads();
  m = fmaxf(fmaxf(sf[0], sf[1]), fmaxf(sf[2], sf[3]));
  __syncthreads();
  float s = 0.f;
  for (int j = tid; j < a.nc; j += kClsThreads) {
    const float e = expf(x[j] - m);
    p[j] = e;
    s += e;
  }
#pragma unroll
  for (int o = 1; o < YM_WAVE; o <<= 1) s += __shfl_xor(s, o);
  if (lane == 0) sf[wave] = s;
  __syncthreads();
  s = (sf[0] + sf[1]) + (sf[2] + sf[3]);
  for (int j = tid; j < a.nc; j += kClsThreads) p[j] = __fdiv_rn(p[j], s);  // (each thread its own elements)
  __syncthreads();
  // top-k: round r takes the largest key below round r - 1's.  Keys are unique (the class is part of them) and above 0
  unsigned long long prev = ~0ull;
  for (int r = 0; r < a.k; ++r) {
    unsigned long long best = 0;
    for (int j = tid; j < a.nc; j += kClsThreads) {
      const float v = p[j];
      const unsigned bits = v == v ? __float_as_uint(v) : 0u;  // probabilities are >= 0: their bits order as they do
      const unsigned long long key = ((unsigned long long)bits << 32) | (0xFFFFFFFFu - (unsigned)j);
      if (key < prev && key > best) best = key;
    }
#pragma unroll
    for (int o = 1; o < YM_WAVE; o <<= 1) {
      const unsigned long long t = __shfl_xor(best, o);
      best = t > best ? t : best;
    }
    if (lane == 0) sk[wave] = best;
    __syncthreads();
    best = sk[0];
#pragma unroll
    for (int w = 1; w < kClsThreads / YM_WAVE; ++w) best = sk[w] > best ? sk[w] : best;
    __syncthreads();
    if (tid == 0) {
      const int idx = (int)(0xFFFFFFFFu - (unsigned)(best & 0xFFFFFFFFull));
      a.topk[(size_t)b * a.k + r] = idx;
      a.topk_conf[(size_t)b * a.k + r] = p[idx];
    }
    prev = best;
  }
}

}  // namespace

hipError_t ym_launch_classify(int dtype, const ClsArgs& a, hipStream_t st) {
  const int xs = dtype == YM_DT_X3 ? 2 : 1;  // storage elements per logical K of a weight row
  if (dtype != YM_DT_F16 && !ym_dt_f32s(dtype)) return hipErrorInvalidValue;
  if (!a.x || !a.w || !a.bias || !a.lw || !a.lb || !a.pooled || !a.logits || !a.probs || !a.topk || !a.topk_conf)
    return hipErrorInvalidValue;
  if (a.B < 1 || a.P < 1 || a.P >= (1 << 24) || a.C1 < kClsKC || a.C1 % kClsKC || a.coff < 0 || a.coff % 8 || a.ctot % 8 ||
      a.coff + a.C1 > a.ctot || a.kpad < xs * a.C1 || a.kpad % 8 || a.nc < 1 || a.ld < a.nc ||
      a.k != (a.nc < kClsTopK ? a.nc : kClsTopK) || (long)a.B * (kClsHidden / kClsBN) > (1L << 30))
    return hipErrorInvalidValue;
  const dim3 grid1((unsigned)(a.B * ((kClsHidden + kClsBN - 1) / kClsBN))), block(kClsThreads);
  ym_with_type(dtype, [&](auto t) {
    typedef typename decltype(t)::type T;
    hipLaunchKernelGGL(cls_pool<T>, grid1, block, 0, st, a);
  });
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const dim3 grid2((unsigned)((a.nc + kClsLinCT - 1) / kClsLinCT));
  if (dtype == YM_DT_F16) hipLaunchKernelGGL(cls_linear<f16>, grid2, block, 0, st, a);
  else hipLaunchKernelGGL(cls_linear<float>, grid2, block, 0, st, a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(cls_softmax, dim3((unsigned)a.B), block, 0, st, a);
  return hipGetLastError();
}
