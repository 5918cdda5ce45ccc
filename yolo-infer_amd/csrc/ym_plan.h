// The plan blob: the one binary a model reaches the runtime in (packed by yolomi/plan.py, loaded by ym_load_weights).
// Host-only and HIP-free: this header and ym_plan.cpp compile with any C++17 compiler.
//
// Layout (int32 little-endian):
//   PlanHeader[32] | buffers[nbuf][8] | OpRec[nop][32] | names[nop][48 bytes] | pad to 256 | weights[wbytes]
// A buffer record is (channels, stride f of its map relative to the input (0: the anchor rows), fp32 flag, 5 x 0).
// Every offset in a record counts bytes from the start of the weight section.  yolomi/plan.py names the slots with
// the member names below (HDR_FIELDS / OP_FIELDS; tests/test_plan_format.py compares them).
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../include/yolomi.h"

// Activation storage precision of a plan: f16 (MFMA 32x32x16 f16), f32 (exact-f32 MFMA 32x32x2, parity mode),
// i8 (PTQ int8: activations stored as q - 128 in int8, weights int8, MFMA 32x32x32 i8 with int32 accumulation), or
// x3 (fp32 storage, every conv GEMM as three f16 MFMAs on split operands: x = hi + lo with hi = fp16(x),
// lo = fp16(x - hi); x·w ≈ hi·w_hi + lo·w_hi + hi·w_lo, fp32 accumulation — ~2^-21 relative, the f16 MFMA rate / 3).
enum { YM_DT_F16 = 0, YM_DT_F32 = 1, YM_DT_I8 = 2, YM_DT_F8 = 3, YM_DT_X3 = 4 };
// plans whose activations are stored fp32 (the exact-f32 parity plan and the split-f16 plan share every non-GEMM kernel)
inline bool ym_dt_f32s(int dt) { return dt == YM_DT_F32 || dt == YM_DT_X3; }
// one-byte quantized plans (int8 affine / fp8 e4m3): same graph, storage and kernels (csrc/ym_quant.h Q8)
inline bool ym_dt_q8(int dt) { return dt == YM_DT_I8 || dt == YM_DT_F8; }

constexpr int32_t kPlanMagic = 0x4C504D59;  // 'YMPL'
constexpr int kBufRec = 8, kNameLen = 48;   // int32 words per buffer record, bytes per op name
constexpr size_t kQRecBytes = 1088;         // sizeof(QRec) (ym_common.h)
constexpr int kTaskPose = 2;
constexpr int kMaxLevels = 3;  // the header has three stride slots

enum OpKind { OP_INPUT = 1, OP_CONV = 2, OP_DW = 3, OP_SPPF = 4, OP_ATTN = 5, OP_DECODE = 6, OP_NMS = 7, OP_REQ = 8 };

struct PlanHeader {
  // -- header fields begin
  int32_t magic;       // kPlanMagic
  int32_t version;     // 1
  int32_t dtype;       // YM_DT_*
  int32_t task;        // 0 detect, 1 segment, 2 pose
  int32_t nc;          // classes
  int32_t nm;          // extras NMS carries per row (segment: 32 mask coefficients; pose: K * ndim padded to 4)
  int32_t reg_max;
  int32_t nl;          // head levels, <= kMaxLevels
  int32_t stride0;
  int32_t stride1;
  int32_t stride2;
  int32_t nbuf;
  int32_t nop;
  int32_t wbytes_lo;   // size of the weight section
  int32_t wbytes_hi;
  int32_t input_buf;
  int32_t anchor_buf;
  int32_t proto_buf;   // segment plans (-1 otherwise)
  int32_t no;          // offset of the nm extras in the anchor row
  int32_t scale;       // 'n', 's', ... (checked against ym_model_desc.scale; 0: unknown)
  int32_t kpt_k;       // pose plans: keypoints ...
  int32_t kpt_ndim;    // ... values of each (2 | 3) ...
  int32_t kpt_off;     // ... offset of the raw keypoints in the anchor row (= no) ...
  int32_t cls_pad;     // ... and class channels of the anchor row (nc padded to 4); all four 0 in other plans
  int32_t rsv24;
  int32_t rsv25;
  int32_t rsv26;
  int32_t rsv27;
  int32_t rsv28;
  int32_t rsv29;
  int32_t rsv30;
  int32_t rsv31;
  // -- header fields end
  int stride(int l) const { return l == 0 ? stride0 : l == 1 ? stride1 : stride2; }
  size_t wbytes() const { return (size_t)(uint32_t)wbytes_lo | ((size_t)(uint32_t)wbytes_hi << 32); }
};
static_assert(sizeof(PlanHeader) == 128, "32 int32 slots");

// One op.  The members are named for the conv record; other kinds reuse some slots under another meaning, read
// through the accessors below.  Input, decode and NMS ops have no operands besides the header's buffers.
struct OpRec {
  // -- op fields begin
  int32_t kind;       // OpKind
  int32_t k;          // kernel size
  int32_t s;          // stride
  int32_t cin;        // c0 + c1 (depthwise, SPPF, attention, requant: their channels C)
  int32_t n;          // output channels (attention: heads)
  int32_t act;        // SiLU flag (attention: key dim per head)
  int32_t src0;       // first source buffer, ...
  int32_t src0_coff;  // ... its channel offset (SPPF: of y0 in dst) ...
  int32_t c0;         // ... and channels
  int32_t up0;        // src0 read 2x nearest-upsampled (attention: value dim per head; requant: upsample)
  int32_t src1;       // concat tail (-1: none)
  int32_t src1_coff;
  int32_t c1;
  int32_t dst;        // destination buffer (SPPF: the buffer pooled in place)
  int32_t dst_coff;
  int32_t level;      // head level whose anchor rows the conv writes (-1: a plain map)
  int32_t shuffle;    // ConvTranspose2d 2x2 as a 1x1 GEMM with a pixel-shuffle epilogue
  int32_t res;        // residual buffer (-1: none)
  int32_t res_coff;
  int32_t w_off;      // weights [n][kpad] (depthwise, attention pe: [9][C])
  int32_t b_off;      // fp32 bias
  int32_t kpad;       // K pitch of a weight row in storage elements (attention: the fp32 bits of its scale)
  int32_t q_off;      // one-byte plans: QRec (x3 plans: exponent s of the weights stored as W·2^s)
  int32_t sasw_off;   // one-byte plans: fp32 s_in·s_w per output channel (x3 plans: W2's exponent)
  int32_t biasi_off;  // one-byte plans: int32 bias (f16 / x3 plans: 1 + offset of a fused depthwise's [9][C] ‖ [C]; 0: none)
  int32_t w2_off;     // fused successor conv (f16 / x3 plans; k2 == 0: none): W2 [n2][kpad2], ...
  int32_t b2_off;     // ... its bias, ...
  int32_t n2;
  int32_t act2;
  int32_t kpad2;
  int32_t k2;         // ... kernel size (1: streaming pair, 3: Bottleneck kernel) ...
  int32_t mid;        // ... and the intermediate buffer, used when the pair runs as two launches
  // -- op fields end
  int attn_nh() const { return n; }
  int attn_kd() const { return act; }
  int attn_hd() const { return up0; }
  float attn_scale() const { float f; memcpy(&f, &kpad, 4); return f; }
  int req_up() const { return up0; }
  int sppf_buf() const { return dst; }
  int sppf_coff() const { return src0_coff; }
  int x3_wexp() const { return q_off; }
  int x3_wexp2() const { return sasw_off; }
  bool has_fused_dw() const { return biasi_off > 0; }  // (float plans)
  int32_t fused_dw_off() const { return biasi_off - 1; }
};
static_assert(sizeof(OpRec) == 128, "32 int32 slots");

struct BufDesc {
  int C, f, f32;
};

struct Op : OpRec {
  char name[kNameLen];
};

struct Plan {
  PlanHeader h;
  std::vector<BufDesc> bufs;
  std::vector<Op> ops;
  size_t woff = 0, wbytes = 0;  // the weight section: blob + woff, wbytes long
};

// Parse and validate a blob: header, ym_model_desc expectations (`want` may be null: any), buffer ids and channel
// views [coff, coff + C) of every op inside their buffers, every weight / bias / quantisation record inside the
// weight section.  The kernels index device memory with these values, so a malformed blob must fail here, never
// inside a launch.  YM_OK, or YM_EBLOB with the message in `err` (`out` is then unspecified).
int ym_plan_parse(const void* blob, size_t bytes, const ym_model_desc* want, Plan& out, std::string& err);

// The plan buffers an op record names: the ones it reads into out[] (their count is returned) and the one it
// writes (-1: none).
int op_reads(const OpRec& o, int out[3]);
int op_writes(const OpRec& o);

// Bytes per element of a conv weight row.  (x3 plans: 2-byte pair-chunk rows, except the stem's fp32 rows.)
inline size_t weight_elem_bytes(int dtype, bool is_stem) {
  if (dtype == YM_DT_F32 || (is_stem && dtype == YM_DT_X3)) return 4;
  return (dtype == YM_DT_F16 || dtype == YM_DT_X3) ? 2 : 1;
}

const char* ym_task_name(int task);
