// Plan blob parsing and validation (ym_plan.h).  Host-only: no HIP header.
#include "ym_plan.h"

#include <cstdarg>
#include <cstdio>

namespace {

int bad(std::string& err, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  err = buf;
  return YM_EBLOB;
}

// Structural check of the op records against the buffers and the weight section.
int validate_ops(const Plan& p, std::string& err) {
  const int nbuf = (int)p.bufs.size(), dtype = p.h.dtype;
  const size_t wbytes = p.wbytes;
  for (int i = 0; i < nbuf; ++i)
    if (p.bufs[i].C <= 0 || p.bufs[i].C > (1 << 16) || p.bufs[i].f < 0 || p.bufs[i].f > 64)
      return bad(err, "buffer %d: bad geometry (C %d, f %d)", i, p.bufs[i].C, p.bufs[i].f);
  // (x3 plans: kpad counts the fp16 [hi | lo] storage K of the pair-chunk weight rows; their fp32 stem rows are
  // checked again where they are read)
  const size_t esz = weight_elem_bytes(dtype, false);
  for (const Op& o : p.ops) {
    auto buf_ok = [&](int b, bool opt) { return (opt && b == -1) || (b >= 0 && b < nbuf); };
    auto w_ok = [&](int32_t off, size_t n) { return (size_t)(uint32_t)off + n <= wbytes; };
    // a channel view [coff, coff + C) of buffer b (b == -1: absent, when optional)
    auto view_ok = [&](int b, int coff, long C, bool opt) {
      if (opt && b == -1) return true;
      return buf_ok(b, false) && coff >= 0 && C > 0 && coff + C <= p.bufs[b].C;
    };
    bool ok = true;
    switch (o.kind) {
      case OP_INPUT: case OP_DECODE: case OP_NMS: break;  // no operands besides the header's input/anchor buffers
      case OP_CONV: {
        const int N = o.n, Kpad = o.kpad;
        const int Nout = o.k2 ? o.n2 : N;            // the channels the launch writes (a fused pair: its second conv's)
        const int Cd = o.shuffle ? Nout / 4 : Nout;  // pixel shuffle (ConvTranspose2d 2x2): N/4 channels per pixel
        const int C1 = o.src1 >= 0 ? o.c1 : 0;
        ok = N > 0 && Kpad > 0 && Kpad <= (1 << 16) && o.cin == (long)o.c0 + C1 &&
             view_ok(o.src0, o.src0_coff, o.c0, false) && view_ok(o.src1, o.src1_coff, o.c1, true) &&
             view_ok(o.dst, o.dst_coff, Cd, false) && view_ok(o.res, o.res_coff, Nout, true) &&
             (o.src0 != p.h.input_buf || (o.src0_coff == 0 && o.src1 == -1)) &&
             w_ok(o.w_off, (size_t)N * Kpad * esz) && w_ok(o.b_off, (size_t)N * 4);
        if (ok && ym_dt_q8(dtype))
          ok = w_ok(o.q_off, kQRecBytes) && w_ok(o.sasw_off, (size_t)N * 4) && w_ok(o.biasi_off, (size_t)N * 4);
        else if (ok && o.has_fused_dw())
          ok = w_ok(o.fused_dw_off(), (size_t)10 * o.cin * 4);  // fused depthwise weights + bias
        if (ok && o.k2)
          ok = o.n2 > 0 && o.kpad2 > 0 && o.kpad2 <= (1 << 16) && buf_ok(o.mid, false) &&
               w_ok(o.w2_off, (size_t)o.n2 * o.kpad2 * 2) && w_ok(o.b2_off, (size_t)o.n2 * 4);
        break;
      }
      case OP_DW: case OP_ATTN: {
        const long C = o.cin, nh = o.attn_nh();
        // attention: the (q, k, v) channels of every head after q_coff; the output slice is C wide
        // (64-bit: the three factors are any int32 until the view checks have bounded them)
        const long Cin = o.kind == OP_ATTN ? (nh > 0 && nh <= C ? nh * (2L * o.attn_kd() + o.attn_hd()) : 0) : C;
        ok = C > 0 && view_ok(o.src0, o.src0_coff, Cin, false) && view_ok(o.dst, o.dst_coff, C, false) &&
             (o.kind == OP_DW || (nh > 0 && nh * o.attn_hd() == C)) &&
             w_ok(o.w_off, (size_t)9 * C * (ym_dt_q8(dtype) ? 1 : 4)) && w_ok(o.b_off, (size_t)C * 4);
        if (ok && ym_dt_q8(dtype)) ok = w_ok(o.q_off, kQRecBytes) && w_ok(o.sasw_off, (size_t)C * 4);
        break;
      }
      case OP_SPPF:  // y0 and the 3 pooled slices
        ok = o.cin > 0 && view_ok(o.sppf_buf(), o.sppf_coff(), 4L * o.cin, false);
        break;
      case OP_REQ:
        ok = o.cin > 0 && view_ok(o.src0, o.src0_coff, o.cin, false) && view_ok(o.dst, o.dst_coff, o.cin, false) &&
             w_ok(o.q_off, kQRecBytes);
        break;
      default: return bad(err, "op %s: unknown op kind %d", o.name, o.kind);
    }
    if (!ok) return bad(err, "op %s: buffer id, channel view or weight range out of bounds", o.name);
  }
  return YM_OK;
}

}  // namespace

const char* ym_task_name(int t) { return t == 0 ? "detect" : t == 1 ? "segment" : t == kTaskPose ? "pose" : "unknown"; }

int op_reads(const OpRec& o, int out[3]) {
  int n = 0;
  switch (o.kind) {
    case OP_CONV:
      out[n++] = o.src0;
      if (o.src1 >= 0) out[n++] = o.src1;
      if (o.res >= 0) out[n++] = o.res;
      break;
    case OP_DW: case OP_ATTN: case OP_REQ: out[n++] = o.src0; break;
    case OP_SPPF: out[n++] = o.sppf_buf(); break;
    default: break;
  }
  return n;
}

int op_writes(const OpRec& o) {
  switch (o.kind) {
    case OP_CONV: case OP_DW: case OP_ATTN: case OP_REQ: case OP_SPPF: return o.dst;
    default: return -1;
  }
}

int ym_plan_parse(const void* blob, size_t bytes, const ym_model_desc* want, Plan& out, std::string& err) {
  const char* base = static_cast<const char*>(blob);
  PlanHeader& h = out.h;
  if (bytes >= sizeof(h)) memcpy(&h, base, sizeof(h));
  if (bytes < sizeof(h) || h.magic != kPlanMagic || h.version != 1) return bad(err, "bad blob magic/version");
  const int nbuf = h.nbuf, nop = h.nop;
  if (nbuf < 1 || nbuf > 4096 || nop < 1 || nop > 4096) return bad(err, "bad buffer/op counts (%d, %d)", nbuf, nop);
  const size_t wbytes = h.wbytes();
  const size_t off_bufs = sizeof(PlanHeader), off_ops = off_bufs + (size_t)nbuf * kBufRec * 4;
  const size_t off_names = off_ops + (size_t)nop * sizeof(OpRec);
  const size_t woff = (off_names + (size_t)nop * kNameLen + 255) / 256 * 256;
  if (wbytes > bytes || bytes < woff + wbytes) return bad(err, "blob truncated (%zu < %zu)", bytes, woff + wbytes);
  const int dtype = h.dtype, task = h.task, nm = h.nm;
  if (dtype != YM_DT_F16 && !ym_dt_f32s(dtype) && !ym_dt_q8(dtype)) return bad(err, "unknown dtype %d", dtype);
  if (h.nl < 1 || h.nl > kMaxLevels) return bad(err, "bad level count");
  if (h.nc < 1 || h.nc > 128 || nm < 0 || nm > 64 || h.reg_max < 1 || h.reg_max > 64)
    return bad(err, "bad head geometry (nc %d, nm %d, reg_max %d)", h.nc, nm, h.reg_max);
  for (int l = 0; l < h.nl; ++l)
    if (h.stride(l) < 1 || h.stride(l) > 64) return bad(err, "bad stride %d", h.stride(l));
  if (task < 0 || task > kTaskPose) return bad(err, "unknown task %d (detect 0, segment 1, pose 2)", task);
  if (want) {  // what the creator of the context expects (0 = any)
    if (want->task && want->task != task + 1)
      return bad(err, "blob task %s, context created for %s", ym_task_name(task), ym_task_name(want->task - 1));
    if (want->dtype && want->dtype != dtype + 1)
      return bad(err, "blob dtype %d, context created for %d", dtype + 1, want->dtype);
    if (want->scale && h.scale && want->scale != h.scale)
      return bad(err, "blob scale '%c', context created for '%c'", (char)h.scale, (char)want->scale);
  }
  if (h.input_buf < 0 || h.input_buf >= nbuf || h.anchor_buf < 0 || h.anchor_buf >= nbuf)
    return bad(err, "bad input/anchor buffer ids");
  if (task == 1 && (h.proto_buf < 0 || h.proto_buf >= nbuf)) return bad(err, "segment plan without proto buffer");
  out.bufs.resize(nbuf);
  for (int i = 0; i < nbuf; ++i) {
    int32_t rec[3];
    memcpy(rec, base + off_bufs + (size_t)i * kBufRec * 4, sizeof(rec));
    out.bufs[i] = BufDesc{rec[0], rec[1], rec[2]};
  }
  if (task == kTaskPose) {  // the keypoint slice [kpt_off, kpt_off + nm) of the anchor row; nm = K * ndim padded to 4
    const int arow = out.bufs[h.anchor_buf].C;
    if (h.kpt_k < 1 || (h.kpt_ndim != 2 && h.kpt_ndim != 3) || nm < (long)h.kpt_k * h.kpt_ndim || (nm & 3) ||
        h.kpt_off < 0 || (h.kpt_off & 3) || (arow & 3) || (long)h.kpt_off + nm > arow || h.no != h.kpt_off)
      return bad(err, "bad pose head geometry (K %d, ndim %d, nm %d, offset %d, row %d)", h.kpt_k, h.kpt_ndim, nm,
                 h.kpt_off, arow);
  }
  out.ops.resize(nop);
  for (int i = 0; i < nop; ++i) {
    Op& o = out.ops[i];
    OpRec rec;
    memcpy(&rec, base + off_ops + (size_t)i * sizeof(OpRec), sizeof(OpRec));
    static_cast<OpRec&>(o) = rec;
    memcpy(o.name, base + off_names + (size_t)i * kNameLen, kNameLen);
    o.name[kNameLen - 1] = 0;
  }
  out.woff = woff;
  out.wbytes = wbytes;
  return validate_ops(out, err);
}
