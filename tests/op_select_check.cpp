// Host check of the launch rules of the attention, depthwise and SPPF ops (yolo-infer_amd/csrc/ym_op_select.h).
//
//   op_select_check trace   the selected variant code (-1: refused) over the grid below
//                           (tests/golden/op_select_trace.txt, recorded from the three launchers these rules were
//                           written out of, their kernel launches replaced by a recorder)
//   op_select_check attn <flash_off> | dw <env_pxt> <env_rt> | sppf
//                           one section of the trace: the part that one set of the once-per-process switches
//                           (YM_ATTN_FLASH_OFF, YM_DW_PXT, YM_DW_RT) decides
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../yolo-infer_amd/csrc/ym_op_select.h"

namespace {

int attn_code(int dtype, int N, int B, int nh, int kd, int hd, bool raw, int q_ctot, int q_coff, int d_ctot, int d_coff,
              bool flash_off) {
  return ym_select_attn(dtype, N, B, nh, kd, hd, raw, q_ctot, q_coff, d_ctot, d_coff, flash_off);
}
int dw_code(int dtype, int B, int H, int W, int C, bool raw, int mode, int tile, int env_pxt, int env_rt) {
  return ym_select_dwconv(dtype, B, H, W, C, raw, mode, tile, env_pxt, env_rt);
}
int sppf_code(int dtype, int H, int W, int C) { return ym_select_sppf(dtype, H, W, C); }

// ---- the grid (everything below is shared with the recording program)
const int kDt[3] = {YM_DT_F16, YM_DT_X3, YM_DT_F32};
const char* const kDtName[3] = {"f16", "x3", "f32"};

// one line per (dtype, case, B x nh): the code at every N
void attn_section(bool flash_off) {
  const int Ns[16] = {13, 15, 128, 129, 256, 257, 416, 417, 512, 513, 1136, 1137, 2115, 4256, 4257, 9700};
  const int Bnh[5][2] = {{1, 1}, {1, 2}, {4, 2}, {15, 4}, {128, 4}};  // B * nh = 1, 2, 8, 60, 512
  struct Case {
    const char* name;
    int kd, raw, d_coff;
  };
  const Case cases[4] = {{"plain", 32, 0, 0}, {"raw", 32, 1, 0}, {"d_coff=2", 32, 0, 2}, {"kd=16", 16, 0, 0}};
  printf("attn flash_off=%d N:", (int)flash_off);
  for (int N : Ns) printf(" %d", N);
  printf("\n");
  for (int d = 0; d < 3; ++d)
    for (const Case& c : cases)
      for (const auto& bn : Bnh) {
        const int B = bn[0], nh = bn[1];
        printf(" %s %s B=%d nh=%d:", kDtName[d], c.name, B, nh);
        // the C2PSA layout: qkv holds nh * (2 kd + hd) channels, the output nh * hd
        for (int N : Ns)
          printf(" %d", attn_code(kDt[d], N, B, nh, c.kd, 64, c.raw != 0, nh * (2 * c.kd + 64), 0, nh * 64, c.d_coff,
                                  flash_off));
        printf("\n");
      }
}

// one line per (map, raw, mode, tile): per dtype the code at every (C, B)
void dw_section(int env_pxt, int env_rt) {
  const int maps[8][2] = {{1, 13}, {3, 5},   {3, 6},   {20, 20},
                          {20, 22}, {80, 80}, {80, 82}, {160, 160}};  // W odd, W % 4 == 2, W % 4 == 0
  const int Cs[4] = {8, 64, 512, 12}, Bs[3] = {1, 8, 11};
  printf("dw pxt=%d rt=%d (C, B):", env_pxt, env_rt);
  for (int C : Cs)
    for (int B : Bs) printf(" (%d, %d)", C, B);
  printf("\n");
  for (const auto& m : maps)
    for (int raw = 0; raw < 2; ++raw)
      for (int mode = 0; mode < 3; ++mode)
        for (int tile = 0; tile < 4; ++tile) {
          printf(" %dx%d raw=%d mode=%d tile=%d:", m[0], m[1], raw, mode, tile);
          for (int d = 0; d < 3; ++d) {
            printf(" %s", kDtName[d]);
            for (int C : Cs)
              for (int B : Bs) printf(" %d", dw_code(kDt[d], B, m[0], m[1], C, raw != 0, mode, tile, env_pxt, env_rt));
          }
          printf("\n");
        }
}

// maps on both sides of 4 * image <= 128 KiB (separable) and image <= 160 KiB (direct), per element size
void sppf_section() {
  const int dts[5] = {YM_DT_F16, YM_DT_X3, YM_DT_F32, YM_DT_I8, YM_DT_F8};
  const char* const names[5] = {"f16", "x3", "f32", "int8", "fp8"};
  const int maps[16][2] = {{20, 20},  {32, 32},  {25, 41},   {64, 32},  {41, 50},   {64, 64},   {17, 241},  {80, 64},
                           {3, 1707}, {128, 80}, {7, 1463}, {160, 128}, {3, 6827}, {160, 160}, {1, 20480}, {1, 20481}};
  printf("sppf HxW:");
  for (const auto& m : maps) printf(" %dx%d", m[0], m[1]);
  printf("\n");
  for (int d = 0; d < 5; ++d)
    for (int C : {64, 12}) {
      printf(" %s C=%d:", names[d], C);
      for (const auto& m : maps) printf(" %d", sppf_code(dts[d], m[0], m[1], C));
      printf("\n");
    }
}

const int kEnv[5][2] = {{0, 0}, {2, 0}, {4, 0}, {0, 2}, {0, 4}};  // (YM_DW_PXT, YM_DW_RT): unset (0) or forced

}  // namespace

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "";
  if (!strcmp(mode, "attn") && argc == 3) {
    attn_section(atoi(argv[2]) != 0);
  } else if (!strcmp(mode, "dw") && argc == 4) {
    dw_section(atoi(argv[2]), atoi(argv[3]));
  } else if (!strcmp(mode, "sppf")) {
    sppf_section();
  } else if (!strcmp(mode, "trace")) {
    attn_section(false);
    attn_section(true);
    for (const auto& e : kEnv) dw_section(e[0], e[1]);
    sppf_section();
  } else {
    fprintf(stderr, "usage: op_select_check trace | attn <flash_off> | dw <env_pxt> <env_rt> | sppf\n");
    return 2;
  }
  return 0;
}
