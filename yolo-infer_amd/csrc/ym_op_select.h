// Launch rules of the attention, depthwise 3x3 and SPPF ops: which instantiation a launcher takes, as pure functions
// of the launch's shape and switches.  Each returns the variant code of include/yolomi.h (YM_ATTNV_* / YM_DWV_* /
// YM_SPPFV_*), or -1 when the op refuses the shape (the launcher's hipErrorInvalidValue).  Host only, plain C++:
// tests/op_select_check.cpp builds it with the host compiler; the launchers (csrc/ym_attn.hip, ym_dwconv.hip,
// ym_sppf.hip) switch on the code.  int8 / fp8 plans have launchers of their own (csrc/ym_conv_i8.hip), except SPPF.
#pragma once
#include "ym_plan.h"

// ---- C2PSA attention (kd, hd: key and head dims; flash_off: YM_ATTN_FLASH_OFF=1, tests)
constexpr int YM_ATTN_KD = 32, YM_ATTN_HD = 64;    // the dims every kernel is laid out for (smaller ones: scalar only)
constexpr int YM_ATTN_NKT[4] = {8, 16, 26, 32};    // key tiles of 16 of the MFMA kernels' instantiations: N <= 512
constexpr int YM_ATTN_QB[4] = {4, 8, 16, 32};      // queries per workgroup of the scalar kernel's
constexpr size_t YM_ATTN_LDS_BUDGET = 150 * 1024;  // of the scalar kernel

// dynamic LDS of the scalar kernel: scores [qb][N], Q [qb][kd], a 64-key chunk of V, all fp32
inline size_t ym_attn_scalar_lds(int qb, int N) {
  return ((size_t)qb * N + (size_t)qb * YM_ATTN_KD + 64 * YM_ATTN_HD) * sizeof(float);
}

inline int ym_select_attn(int dtype, int N, int B, int nh, int kd, int hd, bool raw, int q_ctot, int q_coff, int d_ctot,
                          int d_coff, bool flash_off) {
  // the MFMA kernels: f16 and x3 plans at the YOLO11 head layout (per head q 32, k 32, v 64 channels), 16-byte
  // loads and 8-byte stores aligned, no calibration output
  const bool mfma = (dtype == YM_DT_F16 || dtype == YM_DT_X3) && kd == 32 && hd == 64 && !raw && nh * 128 <= q_ctot &&
                    d_ctot % 4 == 0 && d_coff % 4 == 0 && q_ctot % 8 == 0 && q_coff % 8 == 0;
  if (mfma) {
    const bool x3 = dtype == YM_DT_X3;
    const int nkt = (N + 15) / 16;
    for (int i = 0; i < 4; ++i)
      if (nkt <= YM_ATTN_NKT[i]) return (x3 ? YM_ATTNV_X3_NKT8 : YM_ATTNV_MFMA_NKT8) + i;
    // N > 512 tokens (inputs above 724 px): keys in blocks, online softmax
    if (!flash_off) return x3 ? YM_ATTNV_FLASH_X3 : YM_ATTNV_FLASH_F16;
  }
  if (kd > YM_ATTN_KD || hd > YM_ATTN_HD) return -1;
  // the scalar kernel.  Fewer queries per workgroup = more workgroups: with one wave per SIMD nothing hides this
  // kernel's latencies, so the largest block that still leaves 512 workgroups (16: or whose half does not fit)
  const auto fits = [&](int i) { return ym_attn_scalar_lds(YM_ATTN_QB[i], N) <= YM_ATTN_LDS_BUDGET; };
  const auto wgs = [&](int i) { return (long)B * nh * ((N + YM_ATTN_QB[i] - 1) / YM_ATTN_QB[i]); };
  if (fits(3) && wgs(3) >= 512) return YM_ATTNV_SCALAR_QB4 + 3;
  if (fits(2) && (wgs(2) >= 512 || !fits(1))) return YM_ATTNV_SCALAR_QB4 + 2;
  if (fits(1)) return YM_ATTNV_SCALAR_QB4 + 1;
  if (fits(0)) return YM_ATTNV_SCALAR_QB4;
  return -1;  // N > ~9,600 tokens (input > 3136 px): not supported
}

// ---- depthwise 3x3.  mode: YM_DBG_DW_MODE (0 = LDS tiles (default), 1 = row / one-pixel variants, 2 = column strips),
// tile: YM_DBG_DW_TILE, env_pxt / env_rt: YM_DW_PXT / YM_DW_RT (0: unset).  A thread owns 8 channels of its pixels.
inline long ym_dw_threads(int B, int H, int W, int C, int pxt = 1, int rt = 1) {
  return (long)B * ((H + rt - 1) / rt) * (W / pxt) * (C / 8);
}

inline int ym_select_dwconv(int dtype, int B, int H, int W, int C, bool raw, int mode, int tile, int env_pxt,
                            int env_rt) {
  const long total = ym_dw_threads(B, H, W, C);
  if (total >= 0x7FFFFFFFL - 256) return -1;  // the kernels index in 32 bits
  if (C % 8) return -1;
  // (the calibration output is written by the row / one-pixel variants only)
  if (mode == 0 && !raw) return YM_DWV_LDS0 + (tile >= 1 && tile <= 3 ? tile : 0);
  if (mode == 2 && !raw) {
    // pixels per thread by the row width; rows per thread where the grid keeps >= 256 workgroups
    const int px = (W % 4 == 0) ? 4 : (W % 2 == 0 ? 2 : 0);
    const auto blocks = [&](int p, int rt) { return (ym_dw_threads(B, H, W, C, p, rt) + 255) / 256; };
    int rt = env_rt;
    if (!rt && px) rt = blocks(px, 4) >= 256 ? 4 : (blocks(px, 2) >= 256 ? 2 : 0);
    if (px == 4 && rt == 4) return YM_DWV_STRIP4;
    if (px && rt == 2) return YM_DWV_STRIP2;
  }
  // pixels per thread: 4 where that still leaves >= 128 workgroups (measured best at 80²/160²), else 2 (20²/40²)
  const int pxt = env_pxt ? env_pxt : (total / 4 >= 128 * 256 ? 4 : 2);
  if (dtype == YM_DT_F16 && pxt == 4 && W % 4 == 0) return YM_DWV_ROW4;
  if (pxt >= 2 && W % 2 == 0) return YM_DWV_ROW2;
  return YM_DWV_PIXEL;
}

// ---- SPPF pools: one image x 8 channels per workgroup, in LDS in the storage type
inline size_t ym_sppf_image_bytes(int dtype, int H, int W) {
  return (size_t)H * W * 8 * (dtype == YM_DT_F16 ? 2 : (ym_dt_q8(dtype) ? 1 : 4));
}

inline int ym_select_sppf(int dtype, int H, int W, int C) {
  const size_t img = ym_sppf_image_bytes(dtype, H, W);
  const bool sep = 4 * img <= 128 * 1024;  // input + 3 row-max images
  if (C % 8 || (sep ? 4 * img : img) > 160 * 1024) return -1;
  return sep ? YM_SPPFV_SEP : YM_SPPFV_DIRECT;
}
