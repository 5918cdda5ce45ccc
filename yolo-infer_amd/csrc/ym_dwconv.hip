// Depthwise 3x3 conv (Detect cv3 DWConv) on gfx950, bandwidth-bound: four kernel families with bit-identical results
// and the launcher that takes one by csrc/ym_op_select.h's rule.  int8 / fp8 plans: csrc/ym_conv_i8.hip.
#include <stdlib.h>

#include <type_traits>

#include "ym_common.h"
#include "ym_op_select.h"

namespace {

// ------------------------------------------------------------------------------------------------- depthwise 3x3
// DWConv(c, c, 3) = Conv(g=c): 3x3, stride 1, pad 1, BN folded, SiLU.  One thread = 8 channels of one pixel.
// Every load a thread needs (9 taps x 16 B of activations, 9 x 2 float4 of weights + 2 of bias, the weights L1/L2-
// resident) is independent and issued up front: one memory latency per thread, no LDS staging loop (a strided
// staging loop of 10·C floats was ~10 dependent global round trips for C = 512).
template <typename T>
__global__ __launch_bounds__(256) void dwconv3x3(const DwArgs a) {
  const int C8 = a.C >> 3;
  // 32-bit index math (checked < 2^31 on the host); each XCD owns one contiguous run of blocks (shared tap rows)
  const int idx = ym_xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;
  const int total = a.B * a.H * a.W * C8;
  if (idx >= total) return;
  const int pix = idx / C8;
  const int cg = idx - pix * C8;
  const int HW = a.H * a.W;
  const int b = pix / HW;
  const int p = pix - b * HW;
  const int y = p / a.W, x = p - (p / a.W) * a.W;
  const int c0 = cg * 8;
  const T* src = static_cast<const T*>(a.src);
  typename Vec8<T>::type v[9];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
    v[t] = ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
               ? Vec8<T>::load(src + (size_t)(b * a.s_P + iy * a.W + ix) * a.s_ctot + a.s_coff + c0)
               : Vec8<T>::zero();
  }
  f32x4 w[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    w[t][0] = *reinterpret_cast<const f32x4*>(a.w + t * a.C + c0);
    w[t][1] = *reinterpret_cast<const f32x4*>(a.w + t * a.C + c0 + 4);
  }
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.bias + c0), b1 = *reinterpret_cast<const f32x4*>(a.bias + c0 + 4);
  float acc[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = fmaf((float)v[t][e], w[t][e >> 2][e & 3], acc[e]);
  typename Vec8<T>::type o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {  // f16 plans: the fp16 rounding hides the fast SiLU's ~1 ulp (fp32)
    const float sv = sizeof(T) == 2 ? ym_silu_fast(acc[e]) : (std::is_same<T, P2>::value ? ym_silu_x3(acc[e]) : ym_silu(acc[e]));
    o[e] = (typename Vec8<T>::elem)(a.act ? sv : acc[e]);
  }
  Vec8<T>::store(static_cast<T*>(a.dst) + (size_t)(b * a.d_P + p) * a.d_ctot + a.d_coff + c0, o);
  if (a.raw) {  // f32 calibration run: the pre-activation output
#pragma unroll
    for (int e = 0; e < 8; ++e) a.raw[(size_t)pix * a.C + c0 + e] = acc[e];
  }
}

// Row variant: one thread = 8 channels of PXT consecutive pixels of one row (W % PXT == 0).  The 3 x (PXT + 2)
// activation window and the 9 x 8 weights are loaded once for PXT outputs: (3 (PXT + 2) + 20) vector loads per
// PXT pixels instead of 29 per pixel — the single-pixel kernel is bound by load-instruction issue, not bytes.
// Same fmaf order per output as dwconv3x3 (bias, then taps 0..8): bit-identical results.
template <typename T, int PXT>
__global__ __launch_bounds__(256) void dwconv3x3_row(const DwArgs a) {
  const int C8 = a.C >> 3;
  const int Wq = a.W / PXT;
  const int idx = ym_xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;  // contiguous run per XCD
  const int total = a.B * a.H * Wq * C8;
  if (idx >= total) return;
  const int q = idx / C8;
  const int cg = idx - q * C8;
  const int row = q / Wq;  // b * H + y
  const int x0 = (q - row * Wq) * PXT;
  const int b = row / a.H, y = row - b * a.H;
  const int c0 = cg * 8;
  const T* src = static_cast<const T*>(a.src) + (size_t)b * a.s_P * a.s_ctot + a.s_coff + c0;
  typename Vec8<T>::type v[3][PXT + 2];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const int iy = y + r - 1;
#pragma unroll
    for (int cc = 0; cc < PXT + 2; ++cc) {
      const int ix = x0 + cc - 1;
      v[r][cc] = ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                     ? Vec8<T>::load(src + (size_t)(iy * a.W + ix) * a.s_ctot)
                     : Vec8<T>::zero();
    }
  }
  f32x4 w[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    w[t][0] = *reinterpret_cast<const f32x4*>(a.w + t * a.C + c0);
    w[t][1] = *reinterpret_cast<const f32x4*>(a.w + t * a.C + c0 + 4);
  }
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.bias + c0), b1 = *reinterpret_cast<const f32x4*>(a.bias + c0 + 4);
#pragma unroll
  for (int px = 0; px < PXT; ++px) {
    float acc[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf((float)v[t / 3][px + t % 3][e], w[t][e >> 2][e & 3], acc[e]);
    typename Vec8<T>::type o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sv = sizeof(T) == 2 ? ym_silu_fast(acc[e]) : (std::is_same<T, P2>::value ? ym_silu_x3(acc[e]) : ym_silu(acc[e]));
      o[e] = (typename Vec8<T>::elem)(a.act ? sv : acc[e]);
    }
    const int p = y * a.W + x0 + px;
    Vec8<T>::store(static_cast<T*>(a.dst) + (size_t)(b * a.d_P + p) * a.d_ctot + a.d_coff + c0, o);
    if (a.raw) {
#pragma unroll
      for (int e = 0; e < 8; ++e) a.raw[((size_t)b * a.H * a.W + p) * a.C + c0 + e] = acc[e];
    }
  }
}

// Column-strip variant: one thread = 8 channels of PXT consecutive pixels in RT consecutive rows.  The 3-row window
// rolls down the strip: each new output row loads one input row of PXT + 2 pixels, so (RT + 2)(PXT + 2) vector loads
// serve RT·PXT outputs (PXT 4, RT 4: 2.25 loads per output against 4.5 for the row variant).  Same fmaf order per
// output as dwconv3x3 (bias, then taps 0..8): bit-identical results.
template <typename T, int PXT, int RT>
__global__ __launch_bounds__(256) void dwconv3x3_strip(const DwArgs a) {
  const int C8 = a.C >> 3;
  const int Wq = a.W / PXT, Hq = (a.H + RT - 1) / RT;
  const int idx = ym_xcd_block(blockIdx.x, gridDim.x) * blockDim.x + threadIdx.x;  // contiguous run per XCD
  const int total = a.B * Hq * Wq * C8;
  if (idx >= total) return;
  const int q = idx / C8;
  const int cg = idx - q * C8;
  const int rb = q / Wq;  // b * Hq + row block
  const int x0 = (q - rb * Wq) * PXT;
  const int b = rb / Hq, y0 = (rb - b * Hq) * RT;
  const int c0 = cg * 8;
  const T* src = static_cast<const T*>(a.src) + (size_t)b * a.s_P * a.s_ctot + a.s_coff + c0;
  typedef typename Vec8<T>::type V;
  auto load_row = [&](V* r, int iy) {
#pragma unroll
    for (int cc = 0; cc < PXT + 2; ++cc) {
      const int ix = x0 + cc - 1;
      r[cc] = ((unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W)
                  ? Vec8<T>::load(src + (size_t)(iy * a.W + ix) * a.s_ctot)
                  : Vec8<T>::zero();
    }
  };
  f32x4 w[9][2];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    w[t][0] = *reinterpret_cast<const f32x4*>(a.w + t * a.C + c0);
    w[t][1] = *reinterpret_cast<const f32x4*>(a.w + t * a.C + c0 + 4);
  }
  const f32x4 b0 = *reinterpret_cast<const f32x4*>(a.bias + c0), b1 = *reinterpret_cast<const f32x4*>(a.bias + c0 + 4);
  V v[3][PXT + 2];  // v[(y - y0 + 1 + r) % 3] holds input row y + r - 1 while output row y is computed
  load_row(v[0], y0 - 1);
  load_row(v[1], y0);
#pragma unroll
  for (int j = 0; j < RT; ++j) {
    const int y = y0 + j;
    if (y >= a.H) break;
    load_row(v[(j + 2) % 3], y + 1);
#pragma unroll
    for (int px = 0; px < PXT; ++px) {
      float acc[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = fmaf((float)v[(j + t / 3) % 3][px + t % 3][e], w[t][e >> 2][e & 3], acc[e]);
      V o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float sv = sizeof(T) == 2 ? ym_silu_fast(acc[e]) : (std::is_same<T, P2>::value ? ym_silu_x3(acc[e]) : ym_silu(acc[e]));
        o[e] = (typename Vec8<T>::elem)(a.act ? sv : acc[e]);
      }
      const int p = y * a.W + x0 + px;
      Vec8<T>::store(static_cast<T*>(a.dst) + (size_t)(b * a.d_P + p) * a.d_ctot + a.d_coff + c0, o);
      if (a.raw) {
#pragma unroll
        for (int e = 0; e < 8; ++e) a.raw[((size_t)b * a.H * a.W + p) * a.C + c0 + e] = acc[e];
      }
    }
  }
}

// LDS-tile variant: a workgroup owns TH x TW output pixels x CG 8-channel chunks of one image.  Phase 1: the
// (TH + 2) x (TW + 2) input window of those chunks (zeros outside the map) and the tile's weights / bias go into LDS,
// every global load of the workgroup issued before the barrier — one memory round trip per workgroup, each input
// chunk fetched ~(TH+2)(TW+2)/(TH·TW) times instead of the 9 (one-pixel) or 3(PXT+2)/PXT (row variant) per output.
// Phase 2: each thread computes its outputs from LDS in the fmaf order of dwconv3x3 (bias, then taps 0..8):
// bit-identical results.  LDS holds the values as the other variants compute with them (fp16, or fp32 = hi + lo).
template <typename T, int TH, int TW, int CG>
__global__ __launch_bounds__(256) void dwconv3x3_lds(const DwArgs a) {
  typedef typename std::conditional<sizeof(T) == 2, f16x8, f32x8>::type LV;  // one chunk as the kernel computes it
  constexpr int IH = TH + 2, IW = TW + 2;
  __shared__ LV xin[IH * IW * CG];
  __shared__ f32x8 wl[10 * CG];  // taps 0..8, then the bias
  const int C8 = a.C >> 3;
  const int ntx = (a.W + TW - 1) / TW, nty = (a.H + TH - 1) / TH, ncg = (C8 + CG - 1) / CG;
  int vb = ym_xcd_block(blockIdx.x, gridDim.x);  // neighbouring tiles (shared halo rows) on one XCD
  const int cgi = vb % ncg; vb /= ncg;
  const int tx = vb % ntx; vb /= ntx;
  const int ty = vb % nty;
  const int b = vb / nty;
  const int x0 = tx * TW, y0 = ty * TH, c0 = cgi * CG;  // c0: first chunk
  const T* src = static_cast<const T*>(a.src) + (size_t)b * a.s_P * a.s_ctot + a.s_coff;
  constexpr int NIN = IH * IW * CG;
  constexpr int PER = (NIN + 255) / 256;
  LV v[PER];
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int i = threadIdx.x + 256 * u;
    const int c = i % CG, q = i / CG;
    const int iy = y0 - 1 + q / IW, ix = x0 - 1 + q % IW;
    LV z;
#pragma unroll
    for (int e = 0; e < 8; ++e) z[e] = 0;
    if (i < NIN && c0 + c < C8 && (unsigned)iy < (unsigned)a.H && (unsigned)ix < (unsigned)a.W) {
      const auto t = Vec8<T>::load(src + (size_t)(iy * a.W + ix) * a.s_ctot + 8 * (c0 + c));
#pragma unroll
      for (int e = 0; e < 8; ++e) z[e] = t[e];
    }
    v[u] = z;
  }
  if (threadIdx.x < 10 * CG) {
    const int t = threadIdx.x / CG, c = threadIdx.x % CG;
    f32x8 w8;
#pragma unroll
    for (int e = 0; e < 8; ++e) w8[e] = 0.f;
    if (c0 + c < C8) {
      const float* p = t < 9 ? a.w + t * a.C + 8 * (c0 + c) : a.bias + 8 * (c0 + c);
      const f32x4 lo4 = *reinterpret_cast<const f32x4*>(p), hi4 = *reinterpret_cast<const f32x4*>(p + 4);
      w8 = f32x8{lo4[0], lo4[1], lo4[2], lo4[3], hi4[0], hi4[1], hi4[2], hi4[3]};
    }
    wl[threadIdx.x] = w8;
  }
#pragma unroll
  for (int u = 0; u < PER; ++u) {
    const int i = threadIdx.x + 256 * u;
    if (i < NIN) xin[i] = v[u];
  }
  __syncthreads();
  constexpr int NOUT = TH * TW * CG;
  T* dst = static_cast<T*>(a.dst);
#pragma unroll
  for (int u = 0; u < (NOUT + 255) / 256; ++u) {
    const int i = threadIdx.x + 256 * u;
    const int c = i % CG, q = i / CG;
    const int oy = q / TW, ox = q % TW;
    const int y = y0 + oy, x = x0 + ox;
    if (i >= NOUT || y >= a.H || x >= a.W || c0 + c >= C8) continue;
    const f32x8 bv = wl[9 * CG + c];
    float acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = bv[e];
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const LV xv = xin[((oy + t / 3) * IW + ox + t % 3) * CG + c];
      const f32x8 wv = wl[t * CG + c];
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] = fmaf((float)xv[e], wv[e], acc[e]);
    }
    typename Vec8<T>::type o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float sv = sizeof(T) == 2 ? ym_silu_fast(acc[e]) : (std::is_same<T, P2>::value ? ym_silu_x3(acc[e]) : ym_silu(acc[e]));
      o[e] = (typename Vec8<T>::elem)(a.act ? sv : acc[e]);
    }
    Vec8<T>::store(dst + (size_t)(b * a.d_P + y * a.W + x) * a.d_ctot + a.d_coff + 8 * (c0 + c), o);
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------- launchers
hipError_t ym_launch_dwconv(int dtype, const DwArgs& a, hipStream_t st, int* variant) {
  if (ym_dt_q8(dtype)) return ym_launch_dwconv_i8(a, st, dtype == YM_DT_F8);
  // YM_DW_PXT / YM_DW_RT force the row variants' pixels and the strip variants' rows per thread (read once);
  // YM_DBG_DW_MODE / YM_DBG_DW_TILE (A/B and tests) are read at every launch, i.e. at graph capture
  static const int env_pxt = [] { const char* e = getenv("YM_DW_PXT"); return e ? atoi(e) : 0; }();
  static const int env_rt = [] { const char* e = getenv("YM_DW_RT"); return e ? atoi(e) : 0; }();
  const int code = ym_select_dwconv(dtype, a.B, a.H, a.W, a.C, a.raw != nullptr, ym_debug_get(YM_DBG_DW_MODE),
                                    ym_debug_get(YM_DBG_DW_TILE), env_pxt, env_rt);
  if (code < 0) return hipErrorInvalidValue;
  // workgroups of 256 threads, a thread owning pxt pixels in each of rt rows
  auto grid = [&](int pxt, int rt) { return dim3((ym_dw_threads(a.B, a.H, a.W, a.C, pxt, rt) + 255) / 256); };
  return ym_with_type(dtype, [&](auto t) -> hipError_t {
    typedef typename decltype(t)::type T;
    auto lds = [&](auto th, auto tw, auto cg) -> hipError_t {  // LDS tiles of TH x TW pixels x CG chunks
      constexpr int TH = decltype(th)::value, TW = decltype(tw)::value, CG = decltype(cg)::value;
      const long tiles = (long)a.B * ((a.H + TH - 1) / TH) * ((a.W + TW - 1) / TW) * ((a.C / 8 + CG - 1) / CG);
      if (tiles >= 0x7FFFFFFFL) return hipErrorInvalidValue;
      hipLaunchKernelGGL((dwconv3x3_lds<T, TH, TW, CG>), dim3(tiles), dim3(256), 0, st, a);
      return hipSuccess;
    };
    typedef std::integral_constant<int, 2> i2;
    typedef std::integral_constant<int, 4> i4;
    typedef std::integral_constant<int, 8> i8t;
    typedef std::integral_constant<int, 16> i16;
    typedef std::integral_constant<int, 32> i32;
    hipError_t e = hipSuccess;
    switch (code) {
      case YM_DWV_PIXEL: hipLaunchKernelGGL(dwconv3x3<T>, grid(1, 1), dim3(256), 0, st, a); break;
      case YM_DWV_ROW2: hipLaunchKernelGGL((dwconv3x3_row<T, 2>), grid(2, 1), dim3(256), 0, st, a); break;
      case YM_DWV_ROW4:  // f16 only (the rule)
        if constexpr (std::is_same<T, f16>::value) hipLaunchKernelGGL((dwconv3x3_row<T, 4>), grid(4, 1), dim3(256), 0, st, a);
        else e = hipErrorInvalidValue;
        break;
      case YM_DWV_STRIP2: hipLaunchKernelGGL((dwconv3x3_strip<T, 2, 2>), grid(2, 2), dim3(256), 0, st, a); break;
      case YM_DWV_STRIP4: hipLaunchKernelGGL((dwconv3x3_strip<T, 4, 4>), grid(4, 4), dim3(256), 0, st, a); break;
      case YM_DWV_LDS0: e = lds(i8t(), i16(), i4()); break;
      case YM_DWV_LDS0 + 1: e = lds(i4(), i32(), i4()); break;
      case YM_DWV_LDS0 + 2: e = lds(i8t(), i32(), i2()); break;
      case YM_DWV_LDS0 + 3: e = lds(i16(), i16(), i2()); break;
      default: e = hipErrorInvalidValue;
    }
    if (e != hipSuccess) return e;
    if (variant) *variant = code;
    return hipGetLastError();
  });
}
