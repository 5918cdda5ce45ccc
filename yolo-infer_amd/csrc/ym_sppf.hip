// The fused SPPF max-pool pyramid on gfx950 (every plan dtype) and its launcher.
#include "ym_common.h"
#include "ym_op_select.h"

namespace {

// ------------------------------------------------------------------------------------------------- SPPF pools
// y1 = max5(y0), y2 = max5(y1) = max9(y0), y3 = max13(y0) (stride 1, -inf padding: the cascade is exactly the
// wider window).  Separable: row maxima of radius 2/4/6 in one pass over the 13-wide row window, then column
// maxima.  One workgroup = one image x 8 channels; pixels move as 16-byte vectors and stay in LDS in the storage
// type (max is exact in any precision).
template <typename V>
__device__ __forceinline__ V vmax(V x, V y) { return __builtin_elementwise_max(x, y); }  // v_pk_max_f16 for fp16

// fp8 e4m3 codes (sign-magnitude bytes) are max-pooled as order keys: key = sign ? -magnitude : magnitude, an int8
// whose order is the values' order (both zeros -> 0, stored back as +0: the same value)
template <typename V>
__device__ __forceinline__ V f8_key(V v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = (v[e] & 0x80) ? (signed char)(-(v[e] & 0x7F)) : v[e];
  return v;
}
template <typename V>
__device__ __forceinline__ V f8_unkey(V v) {
#pragma unroll
  for (int e = 0; e < 8; ++e) v[e] = v[e] < 0 ? (signed char)(0x80 | -v[e]) : v[e];
  return v;
}

template <typename T, bool F8 = false>
__global__ __launch_bounds__(256) void sppf_pool(const PoolArgs a) {
  typedef typename Vec8<T>::type V;
  auto ld = [&](const T* p) { V v = Vec8<T>::load(p); if constexpr (F8) v = f8_key(v); return v; };
  auto st = [&](T* p, V v) { if constexpr (F8) v = f8_unkey(v); Vec8<T>::store(p, v); };
  extern __shared__ __attribute__((aligned(16))) unsigned char smraw[];
  V* in = reinterpret_cast<V*>(smraw);  // [HW]
  const int HW = a.H * a.W;
  V* hr = in + HW;                      // [3][HW] row maxima, radius 2, 4, 6
  const int ng = a.C / 8;
  const int vb = ym_xcd_block(blockIdx.x, gridDim.x);  // an image's channel groups share cache lines: one XCD
  const int b = vb / ng;
  const int c0 = (vb % ng) * 8;
  T* buf = static_cast<T*>(a.buf);
  {  // all loads in flight before the first LDS store (HW <= 1024 on the separable path's maps)
    V v[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int p = threadIdx.x + 256 * it;
      if (p < HW) v[it] = ld(buf + (size_t)(b * a.P + p) * a.ctot + a.coff + c0);
    }
#pragma unroll
    for (int it = 0; it < 4; ++it) {
      const int p = threadIdx.x + 256 * it;
      if (p < HW) in[p] = v[it];
    }
    for (int p = threadIdx.x + 1024; p < HW; p += 256)
      in[p] = ld(buf + (size_t)(b * a.P + p) * a.ctot + a.coff + c0);
  }
  __syncthreads();
  if (!a.sep) {  // LDS holds only the input image (large maps in f32): direct 2-D windows
    for (int it = threadIdx.x; it < 3 * HW; it += 256) {
      const int j = it / HW, p = it - (it / HW) * HW;
      const int r = 2 * (j + 1);
      const int y = p / a.W, x = p - (p / a.W) * a.W;
      V m = in[p];
      for (int yy = y - r < 0 ? 0 : y - r; yy <= y + r && yy < a.H; ++yy)
        for (int xx = x - r < 0 ? 0 : x - r; xx <= x + r && xx < a.W; ++xx) m = vmax(m, in[yy * a.W + xx]);
      st(buf + (size_t)(b * a.P + p) * a.ctot + a.coff + (j + 1) * a.C + c0, m);
    }
    return;
  }
  for (int p = threadIdx.x; p < HW; p += 256) {
    const int y = p / a.W, x = p - (p / a.W) * a.W;
    V m2 = in[p], m4 = m2, m6 = m2;
    for (int dx = -6; dx <= 6; ++dx) {
      const int xx = x + dx;
      if (dx == 0 || (unsigned)xx >= (unsigned)a.W) continue;
      const V v = in[y * a.W + xx];
      const int ad = dx < 0 ? -dx : dx;
      m6 = vmax(m6, v);
      if (ad <= 4) m4 = vmax(m4, v);
      if (ad <= 2) m2 = vmax(m2, v);
    }
    hr[p] = m2;
    hr[HW + p] = m4;
    hr[2 * HW + p] = m6;
  }
  __syncthreads();
  for (int it = threadIdx.x; it < 3 * HW; it += 256) {
    const int j = it / HW, p = it - (it / HW) * HW;
    const int r = 2 * (j + 1);
    const int y = p / a.W, x = p - (p / a.W) * a.W;
    const V* h = hr + (size_t)j * HW;
    V m = h[p];
    for (int dy = -r; dy <= r; ++dy) {
      const int yy = y + dy;
      if (dy == 0 || (unsigned)yy >= (unsigned)a.H) continue;
      m = vmax(m, h[yy * a.W + x]);
    }
    st(buf + (size_t)(b * a.P + p) * a.ctot + a.coff + (j + 1) * a.C + c0, m);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------- launchers
hipError_t ym_launch_sppf(int dtype, const PoolArgs& a, hipStream_t st, int* variant) {
  const int code = ym_select_sppf(dtype, a.H, a.W, a.C);
  if (code < 0) return hipErrorInvalidValue;
  PoolArgs b = a;
  b.sep = code == YM_SPPFV_SEP;
  const size_t lds = (b.sep ? 4 : 1) * ym_sppf_image_bytes(dtype, a.H, a.W);  // the input (+ 3 row-max images)
  const dim3 g(a.B * (a.C / 8));
  if (dtype == YM_DT_F16) hipLaunchKernelGGL(sppf_pool<f16>, g, dim3(256), lds, st, b);
  else if (dtype == YM_DT_I8) hipLaunchKernelGGL(sppf_pool<i8>, g, dim3(256), lds, st, b);  // max on q - 128: exact
  else if (dtype == YM_DT_F8) hipLaunchKernelGGL((sppf_pool<i8, true>), g, dim3(256), lds, st, b);
  else if (dtype == YM_DT_X3) hipLaunchKernelGGL(sppf_pool<P2>, g, dim3(256), lds, st, b);  // max of hi + lo values
  else hipLaunchKernelGGL(sppf_pool<float>, g, dim3(256), lds, st, b);
  if (variant && !ym_dt_q8(dtype)) *variant = code;
  return hipGetLastError();
}
