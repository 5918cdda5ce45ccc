// yolomi runtime: model-blob parsing, device weight/workspace arena, per-op launch, HIP-graph cache, C-ABI.
//
// This is the native replacement for the Ultralytics predictor loop that `YOLO11Model.predict` delegates to
// (/root/reference/core/model.py:118-133): per batch it replays ONE captured HIP graph of the whole forward
// (input /255 rule → 80+ fused conv launches → attention → decode → NMS), so the Python host issues one call.
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <string>

#include "ym_runtime.h"
#include "ym_embed.h"
#include "ym_tta.h"

// process-wide debug switches (ym_set_debug; include/yolomi.h YM_DBG_*): set from the environment once, then only by
// the setter — a launch reads an atomic instead of calling getenv (getenv per launch is not thread-safe
// against setenv and costs time on every eager forward)
namespace {
constexpr int kDbgKeys = YM_DBG_STOP + 1;  // include/yolomi.h YM_DBG_* keys 1..10
std::atomic<int>* dbg_slots() {
  static std::atomic<int> v[kDbgKeys] = {};
  static const bool init = [] {
    const char* names[kDbgKeys] = {nullptr,       "YM_NMS_DBG", "YM_DW_MODE", "YM_DW_TILE", "YM_CHAIN",
                                   nullptr,       "YM_STEMFUSE", "YM_ATTN_KB", "YM_PAIRST", "YM_CONV_CFG",
                                   nullptr};  // (YM_DBG_STOP: set by a test only, never from the environment)
    for (int k = 1; k < kDbgKeys; ++k) {
      if (!names[k]) continue;
      const char* e = getenv(names[k]);
      // these two hold value + 1 (0: unset — the pair-store default mask, no forced tile configuration)
      v[k].store(e && *e ? atoi(e) + (k == YM_DBG_PAIRST || k == YM_DBG_CONV_CFG ? 1 : 0) : 0);
    }
    return true;
  }();
  (void)init;
  return v;
}
}  // namespace

int ym_debug_get(int key) { return key > 0 && key < kDbgKeys ? dbg_slots()[key].load(std::memory_order_relaxed) : 0; }
int ym_debug_set(int key, int value) {
  if (key <= 0 || key >= kDbgKeys) return -1;
  return dbg_slots()[key].exchange(value);
}
void ym_debug_add(int key, int d) {
  if (key > 0 && key < kDbgKeys) dbg_slots()[key].fetch_add(d);
}

namespace {

thread_local std::string g_err;

// YM_SEGV_TRACE=1: on SIGSEGV / SIGBUS print the native backtrace (library + offset per frame) to stderr, then hand
// the signal to the handler installed before ours (Python's faulthandler under pytest, which prints the Python
// stack), so a host crash inside the runtime leaves a trace that names the frame.
struct sigaction g_prev_sig[2];
void segv_trace(int sig, siginfo_t* si, void* uc) {
  static const char msg[] = "[yolomi] fatal signal, native backtrace:\n";
  void* fr[64];
  const int n = backtrace(fr, 64);
  if (write(2, msg, sizeof msg - 1) < 0) {}
  backtrace_symbols_fd(fr, n, 2);
  const struct sigaction& p = g_prev_sig[sig == SIGBUS];
  if ((p.sa_flags & SA_SIGINFO) && p.sa_sigaction) return p.sa_sigaction(sig, si, uc);
  if (!(p.sa_flags & SA_SIGINFO) && p.sa_handler != SIG_DFL && p.sa_handler != SIG_IGN) return p.sa_handler(sig);
  signal(sig, SIG_DFL);
  raise(sig);
}
__attribute__((constructor)) void install_segv_trace() {
  const char* e = getenv("YM_SEGV_TRACE");
  if (!e || !*e || *e == '0') return;
  void* warm[2];
  (void)backtrace(warm, 2);  // loads the unwinder now, not inside the handler
  struct sigaction sa;
  memset(&sa, 0, sizeof(sa));
  sa.sa_sigaction = segv_trace;
  sa.sa_flags = SA_SIGINFO | SA_ONSTACK;
  sigemptyset(&sa.sa_mask);
  sigaction(SIGSEGV, &sa, &g_prev_sig[0]);
  sigaction(SIGBUS, &sa, &g_prev_sig[1]);
}

}  // namespace

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

static_assert(sizeof(MlState) == kMlStateBytes, "ym_nms_ws.h sizes the multi-label state rows");

// The device under DevBuf (ym_devbuf.h)
int ym_dev_alloc(void** p, size_t bytes, const char* what, size_t n) {
  const hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) return YM_OK;
  return fail(YM_ENOMEM, (std::string(what) + ": %s").c_str(), n, hipGetErrorString(e));  // (what: one %zu, for n)
}
int ym_dev_free(void* p) { HIPCK(hipFree(p)); return YM_OK; }
int ym_dev_sync() { HIPCK(hipDeviceSynchronize()); return YM_OK; }

// The NMS kernel nodes of a captured forward and their arguments (false when none is found: the caller keys the
// graph on the output pointer instead)
static bool find_nms_nodes(GraphEntry& ge) {
  size_t nn = 0;
  if (hipGraphGetNodes(ge.graph, nullptr, &nn) != hipSuccess || nn == 0) return false;
  std::vector<hipGraphNode_t> nodes(nn);
  if (hipGraphGetNodes(ge.graph, nodes.data(), &nn) != hipSuccess) return false;
  for (hipGraphNode_t n : nodes) {
    hipGraphNodeType t;
    if (hipGraphNodeGetType(n, &t) != hipSuccess || t != hipGraphNodeTypeKernel) continue;
    hipKernelNodeParams p{};
    if (hipGraphKernelNodeGetParams(n, &p) != hipSuccess || (p.func != ym_nms_kernel() && p.func != ym_nms_ml_kernel()))
      continue;  // (both NMS kernels take one NmsArgs)
    if (!p.kernelParams || !p.kernelParams[0]) return false;
    ge.nms_nodes.push_back(n);
    ge.nms_args.push_back(*static_cast<const NmsArgs*>(p.kernelParams[0]));
  }
  if (ge.nms_nodes.empty()) return false;
  for (const NmsArgs& a : ge.nms_args)  // every node writes inside the captured rows
    if (a.dets < ge.dets) {
      ge.nms_nodes.clear();
      ge.nms_args.clear();
      return false;
    }
  return true;
}

static int repoint_dets(GraphEntry& ge, float* d_dets) {
  for (size_t j = 0; j < ge.nms_nodes.size(); ++j) {
    NmsArgs na = ge.nms_args[j];
    na.dets = d_dets + (na.dets - ge.dets);
    if (na.counts2)  // the counts behind the rows move with them
      na.counts2 = reinterpret_cast<int*>(reinterpret_cast<char*>(na.counts2) +
                                          (reinterpret_cast<char*>(d_dets) - reinterpret_cast<char*>(ge.dets)));
    hipKernelNodeParams p{};
    HIPCK(hipGraphKernelNodeGetParams(ge.nms_nodes[j], &p));
    void* args[] = {&na};
    p.kernelParams = args;
    p.extra = nullptr;
    HIPCK(hipGraphExecKernelNodeSetParams(ge.exec, ge.nms_nodes[j], &p));
    ge.nms_args[j] = na;
  }
  ge.dets = d_dets;
  return YM_OK;
}

void retire_graph(GraphEntry& g) {
  if (g.done) {
    (void)hipEventSynchronize(g.done);
    (void)hipEventDestroy(g.done);
    g.done = nullptr;
  }
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g.exec = nullptr;
  g.graph = nullptr;
}

int ensure_workspace(ym_ctx* c, int B, int H, int W) {
  if (c->d_arena && B <= c->cB && H == c->cH && W == c->cW && (!c->ml_want || c->nms.ml)) return YM_OK;
  const int nB = (H == c->cH && W == c->cW && B < c->cB) ? c->cB : B;
  c->clear_graphs();
  if (c->d_arena) {
    HIPCK(hipDeviceSynchronize());  // eager forwards on any stream may still read or write the old arena
    HIPCK(hipFree(c->d_arena));
    c->d_arena = nullptr;
  }
  c->cB = nB;
  c->cH = H;
  c->cW = W;
  c->A = 0;
  for (int l = 0; l < c->nl; ++l) {
    c->lvl_off[l] = c->A;
    c->lvl_W[l] = W / c->strides[l];
    c->A += (H / c->strides[l]) * (W / c->strides[l]);
  }
  size_t off = 0;
  c->buf_off.assign(c->bufs.size(), 0);
  for (size_t b = 0; b < c->bufs.size(); ++b) {
    c->buf_off[b] = off;
    if ((int)b == c->input_buf) continue;  // the stem conv reads the caller's NCHW fp32 batch directly
    off = align_up(off + (size_t)nB * c->buf_P((int)b) * c->bufs[b].C * c->elem((int)b), 256);
  }
  off = nms_scratch_append(c->nms, off, nB, c->A, c->ml_want, 0);
  c->off_ctl = off;    off = align_up(off + YM_CTL_BYTES, 256);
  // split-K workspace of the LDS-DMA conv kernels: fp32 partial tiles + per-tile arrival counters
  c->slab_bytes = std::min<size_t>(std::max<size_t>(32u << 20, (size_t)nB << 22), 1u << 30);
  c->off_slab = off;   off = align_up(off + kMaxLanes * c->slab_bytes, 256);  // one slab region per lane
  c->off_cnt = off;    off = align_up(off + (size_t)kMaxLanes * kSplitCounters * 4, 256);
  c->off_chain = off;  off = align_up(off + (size_t)kChainCtl * 4, 256);  // persistent chain kernel's counters
  c->off_kpts = off;  // pose plans: decoded keypoints (B, A, nm) fp32, the rows NMS takes its extras from
  if (c->task == kTaskPose) off = align_up(off + (size_t)nB * c->A * c->nm * 4, 256);
  c->off_cls = off;
  if (c->task == kTaskClassify) off = align_up(off + c->cls_bytes(nB), 256);
  if (c->task == kTaskObb) {
    const size_t na = (size_t)nB * c->A;
    c->off_obb_cov = off;     off = align_up(off + na * sizeof(float4), 256);
    c->off_obb_sorted = off;  off = align_up(off + na * sizeof(ObbEntry), 256);
    c->off_obb_keep = off;    off = align_up(off + na, 256);
    c->off_obb_nsel = off;    off = align_up(off + (size_t)nB * 4, 256);
  }
  c->arena_bytes = off;
  hipError_t e = hipMalloc(&c->d_arena, off);
  if (e != hipSuccess) {
    c->d_arena = nullptr;
    c->cB = 0;
    return fail(YM_ENOMEM, "workspace hipMalloc(%zu) failed: %s", off, hipGetErrorString(e));
  }
  HIPCK(hipMemset(c->d_arena, 0, off));
  return YM_OK;
}

// Kernel arguments of a conv op for batch B at the current workspace shape.
static int conv_args(ym_ctx* c, const Launch& L, const Op& op, int B, const float* d_in, float in_eps, ConvArgs& a,
                     int& out_f32) {
  a = ConvArgs{};
  a.wsc = a.wsc2 = 1.0f;
  const int pst = ym_debug_get(YM_DBG_PAIRST);  // (value + 1; 0: the default family mask 21)
  a.pst = pst ? pst - 1 : 21;
  const int k = op.k, s = op.s, cin = op.cin, cout = op.n;
  const int b0 = op.src0, b1 = op.src1, bd = op.dst, br = op.res;
  const int up0 = op.up0;
  a.src0 = c->bptr(b0, L.img0); a.s0_ctot = c->bufs[b0].C; a.s0_coff = op.src0_coff; a.C0 = op.c0;
  if (b0 == c->input_buf) {  // stem: NCHW fp32 source, LoadTensor /255 decided on device from ctl[0]
    a.src0 = nullptr;
    a.nchw = d_in;
    a.ctl = reinterpret_cast<const float*>(c->d_arena + c->off_ctl);
    a.eps = in_eps;
    a.wstem = reinterpret_cast<const float*>(c->d_weights + c->off_wstem);
  }
  a.s0_W = c->buf_Wd(b0); a.s0_P = c->buf_P(b0); a.up0 = up0;
  a.Hin = c->buf_H(b0) * (up0 ? 2 : 1);
  a.Win = c->buf_Wd(b0) * (up0 ? 2 : 1);
  if (b1 >= 0) {
    a.src1 = c->bptr(b1, L.img0); a.s1_ctot = c->bufs[b1].C; a.s1_coff = op.src1_coff; a.C1 = op.c1;
    a.s1_P = c->buf_P(b1);
    if (c->buf_H(b1) != a.Hin || c->buf_Wd(b1) != a.Win)
      return fail(YM_EBLOB, "op %s: concat sources disagree in shape", op.name);
  }
  a.k = k; a.s = s; a.pad = k / 2;
  a.Ho = (a.Hin + 2 * a.pad - k) / s + 1;
  a.Wo = (a.Win + 2 * a.pad - k) / s + 1;
  if (cin % 8 || (a.C0 + a.C1) != cin) return fail(YM_EBLOB, "op %s: cin %d not a multiple of 8", op.name, cin);
  a.Cin8 = cin / 8;
  if (ym_dt_q8(c->dtype)) {  // int8 / fp8 plans: K chunks of 16 channels (the stem keeps its 8-padded taps)
    if (b0 != c->input_buf) {
      if (cin % 16) return fail(YM_EBLOB, "op %s: int8 cin %d not a multiple of 16", op.name, cin);
      a.Cin8 = cin / 16;
    }
    a.q = c->wptr<QRec>(op.q_off);
    a.sasw = c->wptr<float>(op.sasw_off);
    a.biasi = c->wptr<int>(op.biasi_off);
    const size_t oi = (size_t)(&op - c->ops.data());
    if (oi < c->off_wtap.size() && c->off_wtap[oi])
      a.wtap = reinterpret_cast<const int*>(c->d_weights + c->off_wtap0 + (c->off_wtap[oi] - 1));
  }
  if (c->dtype == YM_DT_X3 && b0 != c->input_buf) {  // pair layout: fp16 storage chunks per tap double
    a.x3 = 1;
    a.Cin8 = 2 * (cin / 8);
    // the packed weights are W·2^s (and W2·2^s2): yolomi/plan.py
    const int ws = op.x3_wexp(), ws2 = op.x3_wexp2();
    if (ws < -64 || ws > 64 || ws2 < -64 || ws2 > 64)
      return fail(YM_EBLOB, "op %s: bad x3 weight scale exponents %d / %d", op.name, ws, ws2);
    a.wsc = ldexpf(1.0f, -ws);
    a.wsc2 = ldexpf(1.0f, -ws2);
  }
  a.Kc = k * k * a.Cin8;
  a.Kpad = op.kpad;
  a.N = cout;
  a.w = c->wptr<char>(op.w_off);
  a.bias = c->wptr<float>(op.b_off);
  a.act = op.act;
  if (op.k2) {  // fused pair (yolomi/arch.py fuse_pairs): a following 1x1 conv, output in dst/res
    if (c->dtype != YM_DT_F16 && c->dtype != YM_DT_X3)
      return fail(YM_EBLOB, "op %s: fused conv pairs are f16 / x3 only", op.name);
    a.w2 = c->wptr<char>(op.w2_off);
    a.bias2 = c->wptr<float>(op.b2_off);
    a.N2 = op.n2; a.act2 = op.act2; a.Kpad2 = op.kpad2; a.k2 = op.k2;
    const int mid = op.mid;
    if ((a.k2 != 1 && a.k2 != 3) || a.N2 <= 0 || a.Kpad2 < a.k2 * a.k2 * cout * (a.x3 ? 2 : 1) || mid < 0 ||
        mid >= (int)c->bufs.size() || cout % 8 || c->buf_H(mid) != a.Ho || c->buf_Wd(mid) != a.Wo ||
        c->bufs[mid].C != cout || c->bufs[mid].f32)
      return fail(YM_EBLOB, "op %s: bad fused-pair geometry", op.name);
  }
  if (op.has_fused_dw() && !ym_dt_q8(c->dtype)) {  // fused depthwise (yolomi/arch.py fuse_dw): [9][C] weights ‖ [C] bias
    if ((c->dtype != YM_DT_F16 && c->dtype != YM_DT_X3) || k != 1 || s != 1 || b1 >= 0 || up0 || op.k2)
      return fail(YM_EBLOB, "op %s: a fused depthwise needs a single-source 1x1 conv of an f16 / x3 plan", op.name);
    a.dw_w = c->wptr<float>(op.fused_dw_off());
    a.dw_b = a.dw_w + 9 * (size_t)cin;
    a.dw_act = 1;
  }
  a.shuffle = op.shuffle;
  a.npr = a.shuffle ? cout / 4 : cout;
  a.dst = c->bptr(bd, L.img0); a.d_ctot = c->bufs[bd].C; a.d_coff = op.dst_coff; a.d_P = c->buf_P(bd);
  const int lvl = op.level;
  if (lvl >= 0) {
    a.d_pixoff = c->lvl_off[lvl];
    a.d_W = a.Wo;
    if (a.Wo != c->lvl_W[lvl]) return fail(YM_EBLOB, "op %s: head level width mismatch", op.name);
  } else {
    a.d_pixoff = 0;
    a.d_W = c->buf_Wd(bd);
    const int expect = a.shuffle ? 2 : 1;
    if (c->buf_H(bd) != expect * a.Ho || c->buf_Wd(bd) != expect * a.Wo)
      return fail(YM_EBLOB, "op %s: output %dx%d does not match dst buffer %dx%d", op.name, a.Ho, a.Wo,
                  c->buf_H(bd), c->buf_Wd(bd));
  }
  if (br >= 0) { a.res = c->bptr(br, L.img0); a.r_ctot = c->bufs[br].C; a.r_coff = op.res_coff; a.r_P = c->buf_P(br); }
  a.M = B * a.Ho * a.Wo;
  a.fd_hw = ym_fdiv(a.Ho * a.Wo);
  a.fd_w = ym_fdiv(a.Wo);
  out_f32 = c->bufs[bd].f32 && c->dtype != YM_DT_F32;  // (x3: fp32 head rows, pair-layout activations)
  a.raw = c->raw_of(L, op);
  // operand extents in storage elements (the LDS-DMA buffer descriptors): fp16 halves of the x3 pairs
  const long xs = a.x3 ? 2 : 1;
  a.s0_elems = (b0 == c->input_buf) ? 0 : xs * c->cB * c->buf_P(b0) * c->bufs[b0].C;
  a.s1_elems = b1 >= 0 ? xs * c->cB * c->buf_P(b1) * c->bufs[b1].C : 0;
  a.slab = reinterpret_cast<float*>(c->d_arena + c->off_slab + (size_t)L.lane * c->slab_bytes);
  a.slab_cap = (long)c->slab_bytes;
  a.cnt = reinterpret_cast<int*>(c->d_arena + c->off_cnt) + (size_t)L.lane * kSplitCounters;
  a.cnt_cap = kSplitCounters;
  static const int pf_max = [] { const char* e = getenv("YM_DMA_PF"); return e ? atoi(e) : 0; }();
  a.pf = a.M <= pf_max;
  return YM_OK;
}

// A fused pair (ConvArgs::w2) run as its two convs: A writes the intermediate buffer (the record's `mid`), B reads it.
// The tuner picks this when the two tuned single launches beat every fused variant (op cfg ymc::split_encode).
static void split_args(ym_ctx* c, const Launch& L, const Op& op, const ConvArgs& a, ConvArgs& A, ConvArgs& Bc) {
  const int mid = op.mid;
  A = a;
  A.w2 = nullptr; A.bias2 = nullptr; A.res = nullptr;
  A.dst = c->bptr(mid, L.img0); A.d_ctot = c->bufs[mid].C; A.d_coff = 0; A.d_P = c->buf_P(mid); A.d_pixoff = 0;
  A.d_W = c->buf_Wd(mid);
  Bc = a;
  Bc.w2 = nullptr; Bc.bias2 = nullptr;
  Bc.src0 = c->bptr(mid, L.img0); Bc.s0_ctot = c->bufs[mid].C; Bc.s0_coff = 0; Bc.C0 = a.N; Bc.s0_W = c->buf_Wd(mid);
  Bc.s0_P = c->buf_P(mid); Bc.up0 = 0;
  Bc.src1 = nullptr; Bc.C1 = 0; Bc.s1_elems = 0;
  Bc.Hin = a.Ho; Bc.Win = a.Wo; Bc.k = a.k2; Bc.s = 1; Bc.pad = a.k2 / 2;
  const int xs = a.x3 ? 2 : 1;  // x3: fp16 storage chunks of the pair layout
  Bc.Cin8 = xs * a.N / 8; Bc.Kc = a.k2 * a.k2 * Bc.Cin8; Bc.Kpad = a.Kpad2; Bc.N = a.N2; Bc.npr = a.N2;
  Bc.w = a.w2; Bc.bias = a.bias2; Bc.act = a.act2; Bc.wsc = a.wsc2;
  Bc.s0_elems = (long)xs * c->cB * c->buf_P(mid) * c->bufs[mid].C;
}

// taken[2]: ym_launch_conv's `taken` of the fused launch, or of the two convs of a split cfg (a "heuristic" half:
// -1); a fused cfg that fell back to the split pair is {0, -1}
static hipError_t launch_fused(ym_ctx* c, const Launch& L, const Op& op, const ConvArgs& a, int out_f32, int cfg,
                               hipStream_t st, int* taken) {
  const bool tagged = ymc::is_split(cfg);
  if (!tagged) {
    const hipError_t e = ym_launch_conv(c->dtype, out_f32, a, cfg, st, false, &taken[0]);
    if (e != hipErrorInvalidValue) return e;
    // no fused kernel takes this shape (e.g. a map width the Bottleneck kernel does not tile): the two convs with
    cfg = ymc::split_encode(ymc::kSplitHeuristic, ymc::kSplitHeuristic);  // their heuristic tiles
  }
  ConvArgs A, Bc;
  split_args(c, L, op, a, A, Bc);
  int* const ta = tagged ? &taken[0] : nullptr;  // (a fallback from the fused cfg keeps that launch's {0, -1})
  int* const tb = tagged ? &taken[1] : nullptr;
  const hipError_t e = ym_launch_conv(c->dtype, 0, A, ymc::split_cfg(ymc::split_first(cfg)), st, false, ta);
  if (e != hipSuccess) return e;
  return ym_launch_conv(c->dtype, out_f32, Bc, ymc::split_cfg(ymc::split_second(cfg)), st, false, tb);
}

hipError_t launch_nms_stage(const NmsView& v, const NmsSource& src, const ym_infer_args* args, int B, int nc, int nm,
                            int H, int W, float* dets, int* out_counts, int* counts2, hipStream_t st) {
  NmsArgs a{};
  a.anchors = src.extras; a.no_tot = src.extras_ld; a.mask_off = src.mask_off;
  a.boxes = v.boxes; a.scores = v.scores; a.cls = v.cls; a.keys = v.keys; a.counts = v.counts;
  a.sboxes = v.sboxes; a.sareas = v.sareas; a.sup = v.sup;
  a.dets = dets; a.out_counts = out_counts; a.counts2 = counts2;
  a.A = v.A; a.kstride = v.kstride; a.nm = nm; a.max_det = args->max_det; a.max_nms = args->max_nms;
  a.agnostic = args->agnostic; a.B = B; a.nc = nc;
  a.max_wh = args->max_wh; a.img_h = (float)H; a.img_w = (float)W;
  a.iou = args->iou;
  if (args->multi_label && nc > 1) {
    // every (anchor, class) pair above conf: candidates, the max_nms best, their sort and the NMS in
    // csrc/ym_nms_ml.hip (the boxes are written; the single-label keys go unused)
    MlArgs m{};
    m.anchors = src.cls; m.no_tot = src.cls_ld; m.cls_off = src.cls_off;
    m.A = v.A; m.nc = nc; m.B = B;
    set_filter(m, args);
    m.max_nms = args->max_nms; m.cap = kMlCap;
    m.counts = v.counts; m.hist = v.hist; m.state = v.state; m.sel = v.sel; m.sel2 = v.sel2; m.seln = v.seln;
    a.keys = m.sel; a.kstride = kMlCap; a.counts = m.seln;
    a.scores = nullptr; a.cls = nullptr;
    return ym_launch_nms_ml(m, a, st);
  }
  // low conf (the validator's 0.001): thousands of candidates per image; sort their keys over several
  // workgroups per image first (conf is part of the graph key: the predict default 0.25 never launches these)
  if (args->conf < kPresortConf && v.kstride >= 16384) {
    a.keys2 = v.keys2;
    a.presorted = 1;
    const hipError_t e = ym_launch_nms_presort(a, st);
    if (e != hipSuccess) return e;
  }
  return ym_launch_nms(a, st);
}

// The OBB stage's arguments over B images from image img0 on: `rows` their (B, A, no_tot) head rows
static ObbArgs obb_args(ym_ctx* c, const float* rows, int img0, int B, const ym_infer_args* args, float* dets,
                        int* out_counts, int* counts2) {
  const NmsView v = nms_view(c->d_arena, c->nms, img0);
  ObbArgs a{};
  a.anchors = rows; a.no_tot = c->bufs[c->anchor_buf].C; a.ang_off = c->no;
  a.boxes = v.boxes; a.scores = v.scores; a.cls = v.cls; a.keys = v.keys; a.keys2 = v.keys2; a.counts = v.counts;
  const size_t i0 = (size_t)img0 * c->A;
  a.cov = reinterpret_cast<float4*>(c->d_arena + c->off_obb_cov) + i0;
  a.sorted = reinterpret_cast<ObbEntry*>(c->d_arena + c->off_obb_sorted) + i0;
  a.keep = reinterpret_cast<unsigned char*>(c->d_arena + c->off_obb_keep) + i0;
  a.nsel = reinterpret_cast<int*>(c->d_arena + c->off_obb_nsel) + img0;
  a.dets = dets; a.out_counts = out_counts; a.counts2 = counts2;
  a.A = v.A; a.kstride = v.kstride; a.nc = c->nc; a.reg_max = c->reg_max; a.B = B;
  set_levels(a, c);
  set_filter(a, args);
  a.max_det = args->max_det; a.max_nms = args->max_nms; a.agnostic = args->agnostic;
  a.presort = args->conf < kPresortConf && v.kstride >= NMS_SORT;  // as launch_nms_stage
  a.max_wh = args->max_wh; a.img_h = (float)c->cH; a.img_w = (float)c->cW; a.iou = args->iou;
  return a;
}

static int launch_op(ym_ctx* c, const Launch& L, const Op& op, int B, const float* d_in, const ym_infer_args* args,
                     float* d_dets, int* d_counts, hipStream_t st) {
  const int dt = c->dtype;
  hipError_t e = hipSuccess;
  switch (op.kind) {
    case OP_INPUT: {
      PrepArgs a{};
      a.in = d_in;
      a.out = c->bptr(c->input_buf, L.img0);
      a.ctl = reinterpret_cast<float*>(c->d_arena + c->off_ctl);
      a.B = B; a.C = 3; a.H = c->cH; a.W = c->cW;
      a.eps = args->in_eps;
      a.batch_max = args->d_batch_max;
      a.cnt = reinterpret_cast<int*>(c->d_arena + c->off_cnt);
      a.cnt_len = kMaxLanes * kSplitCounters;
      // (ym_embed runs no decode: the previous forward's candidate counts stay as they are)
      e = ym_launch_prep(dt, a, nms_view(c->d_arena, c->nms, 0).counts, L.stop >= 0 ? 0 : B, st);
      break;
    }
    case OP_CONV: {
      ConvArgs a{};
      int out_f32 = 0;
      const int rc = conv_args(c, L, op, B, d_in, args->in_eps, a, out_f32);
      if (rc) return rc;
      const size_t oi = (size_t)(&op - c->ops.data());
      const int cfg = c->op_cfg((long)oi, B);
      int tk[2] = {-1, -1};
      e = a.nchw ? ym_launch_stem(dt, a, st)
                 : (a.w2 ? launch_fused(c, L, op, a, out_f32, cfg, st, tk)
                         : ym_launch_conv(dt, out_f32, a, cfg, st, false, &tk[0]));
      if (c->taken.size() == 2 * c->ops.size()) { c->taken[2 * oi] = tk[0]; c->taken[2 * oi + 1] = tk[1]; }
      break;
    }
    case OP_DW: {
      DwArgs a{};
      const int bs = op.src0, bd = op.dst;
      a.src = c->bptr(bs, L.img0); a.s_ctot = c->bufs[bs].C; a.s_coff = op.src0_coff; a.s_P = c->buf_P(bs);
      a.dst = c->bptr(bd, L.img0); a.d_ctot = c->bufs[bd].C; a.d_coff = op.dst_coff; a.d_P = c->buf_P(bd);
      a.w = c->wptr<float>(op.w_off);
      a.bias = c->wptr<float>(op.b_off);
      a.C = op.cin; a.act = op.act; a.H = c->buf_H(bs); a.W = c->buf_Wd(bs); a.B = B;
      if (ym_dt_q8(dt)) {
        a.w = nullptr;
        a.wq = c->wptr<i8>(op.w_off);
        a.q = c->wptr<QRec>(op.q_off);
        a.sasw = c->wptr<float>(op.sasw_off);
      }
      a.raw = c->raw_of(L, op);
      e = ym_launch_dwconv(dt, a, st, c->variant_of(op));
      break;
    }
    case OP_SPPF: {
      PoolArgs a{};
      const int bb = op.sppf_buf();
      a.buf = c->bptr(bb, L.img0); a.ctot = c->bufs[bb].C; a.coff = op.sppf_coff(); a.P = c->buf_P(bb);
      a.C = op.cin; a.H = c->buf_H(bb); a.W = c->buf_Wd(bb); a.B = B;
      e = ym_launch_sppf(dt, a, st, c->variant_of(op));
      break;
    }
    case OP_ATTN: {
      AttnArgs a{};
      const int bq = op.src0, bd = op.dst;
      a.qkv = c->bptr(bq, L.img0); a.q_ctot = c->bufs[bq].C; a.q_coff = op.src0_coff; a.q_P = c->buf_P(bq);
      a.dst = c->bptr(bd, L.img0); a.d_ctot = c->bufs[bd].C; a.d_coff = op.dst_coff; a.d_P = c->buf_P(bd);
      a.pe_w = c->wptr<float>(op.w_off);
      a.pe_b = c->wptr<float>(op.b_off);
      a.C = op.cin; a.nh = op.attn_nh(); a.kd = op.attn_kd(); a.hd = op.attn_hd();
      a.H = c->buf_H(bq); a.W = c->buf_Wd(bq); a.N = a.H * a.W; a.B = B;
      a.scale = op.attn_scale();
      if (ym_dt_q8(dt)) {
        a.pe_w = nullptr;
        a.pe_wq = c->wptr<i8>(op.w_off);
        a.q = c->wptr<QRec>(op.q_off);
        a.pe_sasw = c->wptr<float>(op.sasw_off);
      }
      a.raw = c->raw_of(L, op);
      e = ym_launch_attn(dt, a, st, c->variant_of(op));
      break;
    }
    case OP_REQ: {
      if (!ym_dt_q8(dt)) return fail(YM_EBLOB, "op %s: requant in a non-quantized plan", op.name);
      ReqArgs a{};
      const int bs = op.src0, bd = op.dst;
      a.src = static_cast<const i8*>(c->bptr(bs, L.img0)); a.s_ctot = c->bufs[bs].C; a.s_coff = op.src0_coff;
      a.s_P = c->buf_P(bs); a.s_W = c->buf_Wd(bs); a.up = op.req_up();
      a.dst = static_cast<i8*>(c->bptr(bd, L.img0)); a.d_ctot = c->bufs[bd].C; a.d_coff = op.dst_coff;
      a.d_P = c->buf_P(bd); a.d_W = c->buf_Wd(bd);
      a.C = op.cin; a.H = c->buf_H(bd); a.W = c->buf_Wd(bd); a.B = B;
      if (c->buf_H(bs) * (a.up ? 2 : 1) != a.H || a.s_W * (a.up ? 2 : 1) != a.W)
        return fail(YM_EBLOB, "op %s: requant source/destination shapes disagree", op.name);
      a.q = c->wptr<QRec>(op.q_off);
      e = ym_launch_requant(a, st, dt == YM_DT_F8);
      break;
    }
    case OP_DECODE: {
      if (c->task == kTaskObb) {  // the rotated decode (csrc/ym_obb.hip); the rows and counts come with OP_NMS
        e = ym_launch_obb_decode(obb_args(c, reinterpret_cast<const float*>(c->bptr(c->anchor_buf, L.img0)), L.img0, B,
                                          args, nullptr, nullptr, nullptr), st);
        break;
      }
      const NmsView v = nms_view(c->d_arena, c->nms, L.img0);
      DecodeArgs a{};
      a.anchors = reinterpret_cast<const float*>(c->bptr(c->anchor_buf, L.img0));
      a.no_tot = c->bufs[c->anchor_buf].C;
      a.boxes = v.boxes; a.scores = v.scores; a.cls = v.cls; a.keys = v.keys; a.counts = v.counts;
      a.A = v.A; a.kstride = v.kstride; a.nc = c->nc; a.reg_max = c->reg_max; a.B = B;
      set_levels(a, c);
      set_filter(a, args);
      e = ym_launch_decode(a, st);
      break;
    }
    case OP_NMS: {
      if (L.skip_nms) break;
      const NmsView v = nms_view(c->d_arena, c->nms, L.img0);
      const float* rows = reinterpret_cast<const float*>(c->bptr(c->anchor_buf, L.img0));
      const int no_tot = c->bufs[c->anchor_buf].C;
      NmsSource src{rows, no_tot, c->no, rows, no_tot, 4 * c->reg_max};
      // counts_after_dets: this lane's images' words behind the WHOLE batch's rows (d_dets is the lane's)
      const int left = L.B - L.img0, cad = args->counts_after_dets;
      if (c->task == kTaskObb) {  // sort -> Fast-NMS keep flags -> rows, in place of the greedy NMS
        int* c2 = cad ? counts_behind(d_dets, left, args->max_det, 7, L.img0) : nullptr;
        e = ym_launch_obb_nms(obb_args(c, rows, L.img0, B, args, d_dets, d_counts, c2), st);
        break;
      }
      if (c->task == kTaskPose) {
        // Pose: decode the candidates' keypoints (behind decode_anchors, before any NMS kernel) into their own
        // (B, A, nm) rows and let NMS carry its nm extras from there; the raw head rows stay as the convs wrote them
        KptArgs k{};
        k.anchors = rows; k.no_tot = no_tot; k.kpt_off = c->kpt_off;
        k.keys = v.keys; k.counts = v.counts;
        k.out = reinterpret_cast<float*>(c->d_arena + c->off_kpts) + (size_t)L.img0 * c->A * c->nm;
        k.nk_pad = c->nm; k.A = v.A; k.kstride = v.kstride; k.K = c->kpt_K; k.ndim = c->kpt_ndim; k.B = B;
        set_levels(k, c);
        e = ym_launch_kpts(k, st);
        if (e != hipSuccess) break;
        src.extras = k.out; src.extras_ld = c->nm; src.mask_off = 0;
      }
      int* counts2 = cad ? counts_behind(d_dets, left, args->max_det, 6 + c->nm, L.img0) : nullptr;
      e = launch_nms_stage(v, src, args, B, c->nc, c->nm, c->cH, c->cW, d_dets, d_counts, counts2, st);
      break;
    }
    case OP_CLASSIFY: {
      ClsArgs a{};
      const int bs = op.src0;
      a.x = c->bptr(bs, L.img0); a.ctot = c->bufs[bs].C; a.coff = op.src0_coff; a.C1 = op.c0; a.P = c->buf_P(bs);
      a.w = c->wptr<char>(op.w_off); a.bias = c->wptr<float>(op.b_off); a.kpad = op.kpad;
      a.wsc = dt == YM_DT_X3 ? ldexpf(1.0f, -op.x3_wexp()) : 1.0f;
      a.lw = c->wptr<char>(op.w2_off); a.lb = c->wptr<float>(op.b2_off);
      a.nc = c->nc; a.B = B; a.k = c->nc < kClsTopK ? c->nc : kClsTopK;
      // the scratch rows of the whole batch (cB images), this launch's images from img0 on
      float* f = reinterpret_cast<float*>(c->d_arena + c->off_cls);
      const size_t nB = (size_t)c->cB, i0 = (size_t)L.img0, nc = (size_t)c->nc;
      a.pooled = f + i0 * kClsHidden;
      f += nB * kClsHidden;
      a.logits = L.cls.logits ? L.cls.logits + i0 * nc : f + i0 * nc;
      f += nB * nc;
      a.probs = L.cls.probs ? L.cls.probs + i0 * L.cls.ld : f + i0 * nc;
      a.ld = L.cls.probs ? (long)L.cls.ld : (long)nc;
      f += nB * nc;
      a.topk = L.cls.topk ? L.cls.topk + i0 * a.k : reinterpret_cast<int*>(f) + i0 * a.k;
      f += nB * kClsTopK;
      a.topk_conf = L.cls.topk_conf ? L.cls.topk_conf + i0 * a.k : f + i0 * a.k;
      e = ym_launch_classify(dt, a, st);
      break;
    }
    default:
      return fail(YM_EBLOB, "unknown op kind %d", op.kind);
  }
  if (e != hipSuccess) return fail(YM_EHIP, "launch of op %s failed: %s", op.name, hipGetErrorString(e));
  return YM_OK;
}

int check_ctx(const ym_ctx* c, const char* who, int task, const char* want) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!c->loaded) return fail(YM_ESTATE, "%s before ym_load_weights", who);
  if (want && c->task != task)
    return fail(YM_EINVAL, "%s: the loaded plan is a %s plan, not %s plan", who, ym_task_name(c->task), want);
  return YM_OK;
}

int check_shape(int B, int H, int W, const char* who) {
  if (B < 1 || H < 32 || W < 32 || H % 32 || W % 32)
    return fail(YM_EINVAL, "%sinput shape (%d,3,%d,%d): H and W must be positive multiples of 32", who, B, H, W);
  return YM_OK;
}

int check_nms_args(const ym_infer_args* args, int nc, int task) {
  if (args->max_det < 1 || args->max_nms < 1) return fail(YM_EINVAL, "max_det/max_nms must be >= 1");
  if (args->max_det > 1024) return fail(YM_EINVAL, "max_det %d > 1024 is not supported", args->max_det);
  if (args->counts_after_dets != 0 && args->counts_after_dets != 1) return fail(YM_EINVAL, "counts_after_dets is 0 or 1");
  if (args->multi_label != 0 && args->multi_label != 1) return fail(YM_EINVAL, "multi_label is 0 or 1");
  // (nc == 1: the single-label path, as upstream's multi_label &= nc > 1; obb plans refuse it whatever nc is)
  if (args->multi_label && (task == kTaskObb || (nc > 1 && task != 0)))
    return fail(YM_EINVAL, "multi_label: %s plans are not supported (validation mode is for detect plans)",
                ym_task_name(task));
  if (args->multi_label && nc > 1) {
    if (nc > 128) return fail(YM_EINVAL, "multi_label: nc %d > 128 is not supported", nc);
    if (args->max_nms > kMlCap) return fail(YM_EINVAL, "multi_label: max_nms %d > %d is not supported", args->max_nms, kMlCap);
  }
  return YM_OK;
}

static int check_call(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
                      int* d_counts) {
  if (int rc = check_ctx(c, "ym_infer")) return rc;
  if (!d_in || !d_dets || !d_counts || !args) return fail(YM_EINVAL, "null pointer argument");
  if (int rc = check_shape(B, H, W, "")) return rc;
  if (int rc = check_nms_args(args, c->nc, c->task)) return rc;
  if (args->multi_label && c->nc > 1) c->ml_want = true;
  return YM_OK;
}

int begin_launch(ym_ctx* c, int B, int H, int W, hipStream_t st, Launch& L) {
  HIPCK(hipSetDevice(c->device));
  if (int rc = ensure_workspace(c, B, H, W)) return rc;
  L = Launch{};
  L.B = B;
  return c->order_after_last(st);
}

// `reps` calls of launch(stream) captured on the private stream as one graph, replayed on `st`: once warm, then
// `timed` times between two events (device-bound even for tiny kernels).  Returns a HIP failure as YM_EHIP; else
// launch_rc is the first non-zero result of `launch` (nothing was replayed) or 0 with the timed replays' total in ms.
// Graph, exec and events are destroyed on every path.
template <typename F>
static int time_captured(ym_ctx* c, hipStream_t st, int reps, int timed, F&& launch, int& launch_rc, float& ms) {
  hipGraph_t g = nullptr;
  hipGraphExec_t ge = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  launch_rc = 0;
  hipError_t e = hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeRelaxed);
  if (e == hipSuccess) {
    for (int r = 0; r < reps && launch_rc == 0; ++r) launch_rc = launch(c->cap_stream);
    e = hipStreamEndCapture(c->cap_stream, &g);  // (always: the capture must not stay open)
  }
  if (e == hipSuccess && launch_rc == 0) {
    e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
    if (e == hipSuccess) e = hipEventCreate(&e0);
    if (e == hipSuccess) e = hipEventCreate(&e1);
    if (e == hipSuccess) e = hipGraphLaunch(ge, st);  // warm
    if (e == hipSuccess) e = hipEventRecord(e0, st);
    for (int r = 0; r < timed && e == hipSuccess; ++r) e = hipGraphLaunch(ge, st);
    if (e == hipSuccess) e = hipEventRecord(e1, st);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  }
  if (e1) (void)hipEventDestroy(e1);
  if (e0) (void)hipEventDestroy(e0);
  if (ge) (void)hipGraphExecDestroy(ge);
  if (g) (void)hipGraphDestroy(g);
  if (launch_rc != 0) return YM_OK;  // (the caller skips or reports it)
  return e == hipSuccess ? YM_OK : fail(YM_EHIP, "timed graph replay: %s", hipGetErrorString(e));
}

extern "C" {

int ym_version(void) { return 1; }
int ym_num_conv_cfgs(int dtype) {  // public dtype codes (ym_model_desc): 1 f16, 2 f32, 3 i8, 4 f8, 5 x3
  if (dtype < 1 || dtype > 5) return YM_EINVAL;
  static const int dt[6] = {0, YM_DT_F16, YM_DT_F32, YM_DT_I8, YM_DT_F8, YM_DT_X3};
  return ymc::num_cfgs(dt[dtype]);
}

const char* ym_last_error(void) { return g_err.c_str(); }
int ym_set_debug(int key, int value) {
  if (key < YM_DBG_NMS || key > YM_DBG_STOP) return fail(YM_EINVAL, "unknown debug key %d", key);
  return ym_debug_set(key, value);
}

int ym_create(int device, const ym_model_desc* desc, ym_ctx** out) {
  if (!out) return fail(YM_EINVAL, "null out");
  int n = 0;
  HIPCK(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(YM_EINVAL, "device %d out of range (%d devices)", device, n);
  HIPCK(hipSetDevice(device));
  ym_ctx* c = new ym_ctx();
  c->device = device;
  if (desc) c->desc = *desc;
  hipError_t e = hipStreamCreateWithFlags(&c->cap_stream, hipStreamNonBlocking);
  for (int l = 1; l < kMaxLanes && e == hipSuccess; ++l) e = hipStreamCreateWithFlags(&c->lane_streams[l], hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&c->fork_ev, hipEventDisableTiming);
  if (e == hipSuccess) e = hipMalloc(&c->d_misc, kMiscBytes);
  if (e == hipSuccess) e = hipMemset(c->d_misc, 0, kMiscBytes);
  for (int l = 1; l < kMaxLanes && e == hipSuccess; ++l) e = hipEventCreateWithFlags(&c->join_ev[l], hipEventDisableTiming);
  if (e != hipSuccess) {
    delete c;
    return fail(YM_EHIP, "hipStreamCreate/hipEventCreate: %s", hipGetErrorString(e));
  }
  *out = c;
  return YM_OK;
}

// Static branch schedule (one-lane forwards): op i depends on every earlier op that writes a buffer it reads
// (buffer granularity; the planner never rewrites a buffer region within a forward, so RAW is the only hazard).
// Ops go in program order onto up to kMaxLanes streams: an op continues the stream of its latest dependency when
// that dependency is the stream's tail, else opens an unused stream, else joins the stream whose tail is oldest.
// Cross-stream dependencies become event waits (skipped when already implied by an earlier wait).  The Detect-head
// chains of P3/P4 then run beside the neck's latency-bound 40x40/20x20 layers.
static void build_schedule(ym_ctx* c) {
  const int nop = (int)c->ops.size(), nbuf = (int)c->bufs.size();
  const int P_DEC = nbuf, P_OUT = nbuf + 1;  // pseudo buffers: decode scratch, detections
  auto rw = [&](const Op& o, std::vector<int>& rd, std::vector<int>& wr) {
    int b[3];
    rd.assign(b, b + op_reads(o, b));
    wr.clear();
    if (op_writes(o) >= 0) wr.push_back(op_writes(o));
    switch (o.kind) {  // the header's buffers and the pseudo ones
      case OP_INPUT: wr.push_back(c->input_buf); break;
      case OP_DECODE: rd.push_back(c->anchor_buf); wr.push_back(P_DEC); break;
      case OP_NMS: rd.push_back(P_DEC); rd.push_back(c->anchor_buf); wr.push_back(P_OUT); break;
      default: break;
    }
  };
  const int S = kMaxLanes;
  c->br_of.assign(nop, 0);
  c->br_wait.assign(nop, {});
  c->br_rec.assign(nop, 0);
  std::vector<std::vector<int>> writers(nbuf + 2);
  std::vector<int> tail(S, -1);
  std::vector<std::vector<int>> known(S, std::vector<int>(S, -1));  // known[s][t]: ops of stream t done before s
  std::vector<std::vector<int>> snap(nop);                          // known vector of an op's stream after it
  std::vector<int> rd, wr;
  int used = 1;
  // YM_BRANCHES=1..4; default 4 streams for f16 detect plans, serial otherwise.  tools/branch_ab.sh on MI355X (one
  // box, bench.py device img/s, serial -> 4 streams): yolo11s f16 B=8 8.06k -> 8.51k, yolo11n f16 12.1k -> 13.0k (the
  // Detect-head chains of one level overlap the neck's 20x20 / 40x40 layers, whose launches leave most CUs idle), but
  // yolo11s-seg f16 B=4 4.35k -> 3.84k, yolo11n int8 8.62k -> 7.39k and fp8 9.25k -> 7.87k (their head / requant /
  // float-island kernels contend with the neck instead of filling idle CUs).  Round 3, x3 detect plans: yolo11s B=8
  // 4.47k -> 4.68k predict img/s, yolo11n device 6.88k -> 7.31k: on by default too.
  const char* env = getenv("YM_BRANCHES");
  const int def = (c->dtype == YM_DT_F16 || c->dtype == YM_DT_X3) && c->task == 0 ? S : 1;
  const int maxs = env && *env ? (atoi(env) < 1 ? 1 : (atoi(env) > S ? S : atoi(env))) : def;
  // YM_SCHED=crit: continue the stream of the dependency expected to finish LAST (a per-op time estimate at
  // 640², B = 8: ~6 us per launch plus MACs at ~40 TMAC/s), instead of the latest dependency in program order — a
  // join then waits on the other streams' earlier producers, and the slowest chain flows straight into its consumer
  // without a cross-queue wait (the kernel trace shows ~10 us idle at such joins, e.g. before decode)
  const char* sched = getenv("YM_SCHED");
  const bool crit = sched && !strcmp(sched, "crit");
  std::vector<double> fin(nop, 0.0), sfin(S, 0.0);
  auto est_us = [&](const Op& o) {
    double macs = 0;
    if (o.kind == OP_CONV) {
      const int f = c->bufs[o.dst].f > 0 ? c->bufs[o.dst].f : 8;  // output stride (head rows: level stride unknown)
      const double px = 8.0 * (640.0 / f) * (640.0 / f);
      macs = px * o.k * o.k * (double)o.cin * o.n * (o.k2 ? 2 : 1);
    }
    return 6.0 + macs / 40e6;
  };
  for (int i = 0; i < nop; ++i) {
    rw(c->ops[i], rd, wr);
    std::vector<int> deps;  // (every buffer id of a loaded plan is in range: ym_plan_parse)
    for (int b : rd) deps.insert(deps.end(), writers[b].begin(), writers[b].end());
    int jmax = -1;
    for (int j : deps) jmax = j > jmax ? j : jmax;
    int s = -1;
    if (crit) {  // the stream tail among the dependencies with the latest estimated finish
      double best = -1;
      for (int j : deps)
        if (tail[c->br_of[j]] == j && fin[j] > best) { best = fin[j]; s = c->br_of[j]; }
    }
    if (s < 0 && jmax >= 0 && tail[c->br_of[jmax]] == jmax) s = c->br_of[jmax];
    if (s < 0 && jmax >= 0 && used < maxs) s = used++;
    if (s < 0) {  // the stream whose tail is oldest
      s = 0;
      for (int t = 1; t < used; ++t) if (tail[t] < tail[s]) s = t;
    }
    if (i == 0) s = 0;
    for (int j : deps) {
      const int t = c->br_of[j];
      if (t == s || known[s][t] >= j) continue;
      c->br_wait[i].push_back(j);
      c->br_rec[j] = 1;
      known[s][t] = j;
      for (int u = 0; u < S; ++u) if (snap[j][u] > known[s][u]) known[s][u] = snap[j][u];
    }
    double start = sfin[s];
    for (int j : deps) start = fin[j] > start ? fin[j] : start;
    fin[i] = sfin[s] = start + est_us(c->ops[i]);
    c->br_of[i] = s;
    tail[s] = i;
    known[s][s] = i;
    snap[i] = known[s];
    for (int b : wr) writers[b].push_back(i);
  }
  c->nbr = used;
}

// OCP e4m3 (gfx950 fp8) code -> value: the fp8 plan's stem weights, re-laid out as fp32 (exact)
static float e4m3_value(uint8_t b) {
  const int e = (b >> 3) & 15, m = b & 7;
  const float v = e == 0 ? ldexpf((float)m, -9) : ((e == 15 && m == 7) ? NAN : ldexpf((float)(8 + m), e - 10));
  return (b & 0x80) ? -v : v;
}

int ym_load_weights(ym_ctx* c, const void* blob, size_t bytes) {
  if (!c || !blob) return fail(YM_EINVAL, "null argument");
  HIPCK(hipSetDevice(c->device));
  // the blob is parsed and validated into `plan`; the context changes only once the whole blob checks out
  Plan plan;
  std::string err;
  if (int rc = ym_plan_parse(blob, bytes, &c->desc, plan, err)) return fail(rc, "%s", err.c_str());
  const PlanHeader& h = plan.h;
  const int dtype = h.dtype;
  const bool pose = h.task == kTaskPose;
  const size_t woff = plan.woff, wbytes = plan.wbytes;
  if (h.task == kTaskClassify) {  // exactly one head, behind every other op; its x3 weight exponent in ldexpf's range
    int heads = 0;
    for (const Op& o : plan.ops) heads += o.kind == OP_CLASSIFY;
    const Op& last = plan.ops.back();
    if (heads != 1 || last.kind != OP_CLASSIFY || (dtype == YM_DT_X3 && (last.x3_wexp() < -64 || last.x3_wexp() > 64)))
      return fail(YM_EBLOB, "classify plan: one classify op, the last, with |x3 exponent| <= 64");
  }
  // commit: a reload drops the previous plan's workspace, graphs and per-shape tile tables (they index its ops and
  // buffers); the weights are replaced below
  c->loaded = false;
  c->clear_graphs();
  if (c->d_arena || c->d_weights) HIPCK(hipDeviceSynchronize());  // no launch may still use the old plan's memory
  if (c->d_arena) HIPCK(hipFree(c->d_arena));
  c->d_arena = nullptr;
  c->arena_bytes = 0;
  c->cB = c->cH = c->cW = 0;
  c->buf_off.clear();
  c->cfgs.clear();
  c->dtype = dtype;
  c->task = h.task; c->nc = h.nc; c->nm = h.nm; c->reg_max = h.reg_max; c->nl = h.nl;
  for (int l = 0; l < h.nl; ++l) c->strides[l] = h.stride(l);
  c->input_buf = h.input_buf; c->anchor_buf = h.anchor_buf; c->proto_buf = h.proto_buf; c->no = h.no;
  c->kpt_K = pose ? h.kpt_k : 0; c->kpt_ndim = pose ? h.kpt_ndim : 0;
  c->kpt_off = pose ? h.kpt_off : 0;
  c->bufs = std::move(plan.bufs);
  c->ops = std::move(plan.ops);
  c->cls_op = -1;
  for (size_t i = 0; i < c->ops.size(); ++i)
    if (c->ops[i].kind == OP_CLASSIFY) c->cls_op = (int)i;
  c->blob_host.assign(static_cast<const char*>(blob), static_cast<const char*>(blob) + bytes);  // ym_broadcast_weights
  build_schedule(c);
  while (c->op_ev.size() < c->ops.size()) {
    hipEvent_t ev;
    HIPCK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    c->op_ev.push_back(ev);
  }
  c->clear_graphs();
  if (c->d_weights) HIPCK(hipFree(c->d_weights));
  c->d_weights = nullptr;
  // The stem conv's weights, re-laid out on the host as fp32 [27][N] (tap-major: (ky, kx, c), N contiguous) so the
  // stem kernel reads them with wave-uniform (scalar) loads; the blob packs them as [N][Kpad] GEMM rows with the
  // 3 input channels padded to 8 per tap.  int8 plans keep the integer weight values, fp8 plans the e4m3 values
  // (both exact in fp32).
  std::vector<float> wstem;
  for (const Op& o : c->ops) {
    if (o.kind != OP_CONV || o.src0 != c->input_buf) continue;
    const int N = o.n, Kpad = o.kpad;
    if (o.k != 3 || o.cin != 8 || Kpad < 72) return fail(YM_EBLOB, "op %s: unexpected stem geometry", o.name);
    const char* w = static_cast<const char*>(blob) + woff + (size_t)(uint32_t)o.w_off;
    if ((size_t)(uint32_t)o.w_off + (size_t)N * Kpad * weight_elem_bytes(dtype, true) > wbytes)
      return fail(YM_EBLOB, "stem weights out of range");
    wstem.assign((size_t)27 * N, 0.f);
    for (int n = 0; n < N; ++n)
      for (int t = 0; t < 27; ++t) {
        const size_t i = (size_t)n * Kpad + (t / 3) * 8 + t % 3;
        float v;
        if (ym_dt_f32s(c->dtype)) memcpy(&v, w + 4 * i, 4);
        else if (c->dtype == YM_DT_F16) { _Float16 h16; memcpy(&h16, w + 2 * i, 2); v = (float)h16; }
        else if (c->dtype == YM_DT_F8) v = e4m3_value(reinterpret_cast<const uint8_t*>(w)[i]);
        else v = (float)reinterpret_cast<const int8_t*>(w)[i];
        wstem[(size_t)t * N + n] = v;
      }
    break;
  }
  // int8 plans: per 3x3 conv the [9][N] int32 tap sums of its weights (ConvArgs::wtap: the LDS-DMA kernels' padding
  // correction), behind the stem weights
  std::vector<int32_t> wtap;
  c->off_wtap.assign(c->ops.size(), 0);
  if (dtype == YM_DT_I8) {
    for (size_t i = 0; i < c->ops.size(); ++i) {
      const Op& o = c->ops[i];
      if (o.kind != OP_CONV || o.src0 == c->input_buf || o.k != 3) continue;
      const int N = o.n, Kpad = o.kpad, cs = (o.cin + 15) / 16 * 16;
      if (9 * cs > Kpad || (size_t)(uint32_t)o.w_off + (size_t)N * Kpad * weight_elem_bytes(dtype, false) > wbytes) continue;
      const int8_t* w = reinterpret_cast<const int8_t*>(static_cast<const char*>(blob) + woff + (size_t)(uint32_t)o.w_off);
      c->off_wtap[i] = wtap.size() * 4 + 1;  // + 1: 0 means none (relative to off_wtap0, 4-byte units * 4)
      for (int t = 0; t < 9; ++t)
        for (int n = 0; n < N; ++n) {
          int32_t sum = 0;
          for (int k = 0; k < cs; ++k) sum += w[(size_t)n * Kpad + t * cs + k];
          wtap.push_back(sum);
        }
    }
  }
  c->off_wstem = align_up(wbytes, 256);
  c->off_wtap0 = align_up(c->off_wstem + wstem.size() * sizeof(float), 256);
  const size_t dbytes = c->off_wtap0 + wtap.size() * sizeof(int32_t);
  hipError_t e = hipMalloc(&c->d_weights, dbytes ? dbytes : 256);
  if (e != hipSuccess) return fail(YM_ENOMEM, "weights hipMalloc(%zu): %s", dbytes, hipGetErrorString(e));
  HIPCK(hipMemcpy(c->d_weights, static_cast<const char*>(blob) + woff, wbytes, hipMemcpyHostToDevice));
  if (!wstem.empty())
    HIPCK(hipMemcpy(c->d_weights + c->off_wstem, wstem.data(), wstem.size() * sizeof(float), hipMemcpyHostToDevice));
  if (!wtap.empty())
    HIPCK(hipMemcpy(c->d_weights + c->off_wtap0, wtap.data(), wtap.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  c->wbytes = wbytes;
  c->loaded = true;
  return YM_OK;
}

// Lane split of a B-image batch: L = clamp(args->lanes, 1, kMaxLanes) slices of ceil(B / L) images (0 = 1 lane).
static void lane_split(const ym_infer_args* args, int B, int& L, int& Bl) {
  L = args->lanes < 1 ? 1 : (args->lanes > kMaxLanes ? kMaxLanes : args->lanes);
  if (L > B) L = B;
  Bl = (B + L - 1) / L;
  L = (B + Bl - 1) / Bl;
}

// YM_DBG_CHAIN = 1 (ym_set_debug, or YM_CHAIN=1 in the environment; verdict r5 item 1): op i and op i+1 as ONE persistent launch (csrc/ym_conv_dma.hip
// conv_dma_chain) where both are x3 3x3 convs on the same LDS-DMA configuration, op i+1 reads op i's output and waits
// for nothing else, and both run on the main stream (one chain kernel in flight at a time).  Returns 1 when launched.
static int try_chain(ym_ctx* c, const Launch& L, size_t i, int B, const float* d_in, const ym_infer_args* args,
                     hipStream_t st, int& rc) {
  rc = YM_OK;
  if (ym_debug_get(YM_DBG_CHAIN) != 1 || c->dtype != YM_DT_X3 || i + 1 >= c->ops.size() || L.lane != 0) return 0;
  const Op &o0 = c->ops[i], &o1 = c->ops[i + 1];
  if (o0.kind != OP_CONV || o1.kind != OP_CONV || o0.k2 || o1.k2) return 0;
  if (c->nbr > 1 && (c->br_of[i] != 0 || c->br_of[i + 1] != 0 || !c->br_wait[i + 1].empty())) return 0;
  const int cf0 = c->op_cfg((long)i, B), cf1 = c->op_cfg((long)i + 1, B);
  const int dma = cf0 - 17;  // LDS-DMA ids follow the 17 first-generation configurations (csrc/ym_conv.hip)
  if (cf0 != cf1 || (dma != 8 && dma != 13 && dma != 26)) return 0;
  ConvArgs a0{}, a1{};
  int f0 = 0, f1 = 0;
  const float eps = args->in_eps;
  if ((rc = conv_args(c, L, o0, B, d_in, eps, a0, f0)) || (rc = conv_args(c, L, o1, B, d_in, eps, a1, f1))) return 1;
  if (f0 || f1 || a0.nchw) return 0;
  const hipError_t e = ym_launch_conv_dma_chain(a0, a1, dma, reinterpret_cast<int*>(c->d_arena + c->off_chain),
                                                kChainCtl, st);
  if (e == hipErrorInvalidValue) return 0;  // shapes the chain kernel does not take: two launches
  if (e != hipSuccess) rc = fail(YM_EHIP, "chain launch of %s + %s: %s", o0.name, o1.name, hipGetErrorString(e));
  else ym_debug_add(YM_DBG_CHAIN_LAUNCHES, 1);
  return 1;
}

// YM_DBG_STEMFUSE = 1 (verdict r5 item 5): the x3 stem (op i) and the fused 3x3 s2 -> 1x1 pair that
// reads its output (op i + 1: model.1 -> model.2.cv1) as ONE launch (csrc/ym_stem_fused.hip): the stem's output is
// never stored.  Only where nothing else reads that output and op i + 1 waits for nothing else.  Returns 1 when
// launched.
static int try_stem_fuse(ym_ctx* c, const Launch& L, size_t i, int B, const float* d_in, const ym_infer_args* args,
                         hipStream_t st, int& rc) {
  rc = YM_OK;
  if (ym_debug_get(YM_DBG_STEMFUSE) != 1 || c->dtype != YM_DT_X3 || i + 1 >= c->ops.size()) return 0;
  const Op &o0 = c->ops[i], &o1 = c->ops[i + 1];
  if (o0.kind != OP_CONV || o1.kind != OP_CONV || o0.src0 != c->input_buf || !o1.k2 || o1.src0 != o0.dst) return 0;
  if (c->nbr > 1 && (c->br_of[i] != c->br_of[i + 1] || !c->br_wait[i + 1].empty())) return 0;
  for (size_t j = 0; j < c->ops.size(); ++j) {  // the stem's output: op i + 1 must be its only reader
    if (j == i + 1) continue;
    int rd[3];
    const int n = op_reads(c->ops[j], rd);
    if (std::find(rd, rd + n, o0.dst) != rd + n) return 0;
  }
  ConvArgs a0{}, a1{};
  int f0 = 0, f1 = 0;
  const float eps = args->in_eps;
  if ((rc = conv_args(c, L, o0, B, d_in, eps, a0, f0)) || (rc = conv_args(c, L, o1, B, d_in, eps, a1, f1))) return 1;
  if (f0 || f1) return 0;
  const hipError_t e = ym_launch_stem_down_x3(a0, a1, st);
  if (e == hipErrorInvalidValue) return 0;
  if (e != hipSuccess) rc = fail(YM_EHIP, "fused stem launch of %s + %s: %s", o0.name, o1.name, hipGetErrorString(e));
  return 1;
}

// The pooling stage's descriptor table for B images of an H x W input: the context's validated views (ym_embed) at
// their places in the arena (`with_ptrs`; without: the geometry only, to size the partials before the arena exists).
static void embed_args(const ym_ctx* c, int B, int H, int W, bool with_ptrs, EmbedArgs& a) {
  a = EmbedArgs{};
  a.n = (int)c->embed_views.size();
  a.B = B;
  a.out = c->embed_out;
  a.ld = (long)c->embed_ld;
  a.part = static_cast<float*>(c->embed.p);
  int col = 0;
  for (int i = 0; i < a.n; ++i) {
    const ym_embed_view& v = c->embed_views[i];
    const BufDesc& bd = c->bufs[v.buf];
    EmbedDesc& d = a.d[i];
    d.ptr = with_ptrs ? c->d_arena + c->buf_off[v.buf] : reinterpret_cast<const void*>(c);  // (any non-null)
    d.P = (H / bd.f) * (W / bd.f);
    d.pitch = bd.C;
    d.coff = v.coff;
    d.C = v.C;
    d.mode = (bd.f32 || c->dtype == YM_DT_F32) ? YM_EMB_F32 : (c->dtype == YM_DT_X3 ? YM_EMB_X3 : YM_EMB_F16);
    d.col = col;
    col += v.C;
  }
}

static int launch_embed(ym_ctx* c, int B, hipStream_t st) {
  EmbedArgs a;
  embed_args(c, B, c->cH, c->cW, true, a);
  const long need = ym_embed_part_floats(a);
  if (need < 0 || (size_t)need * sizeof(float) > c->embed.bytes) return fail(YM_EINVAL, "ym_embed: bad view table");
  return launched(ym_launch_embed(a, st), "embed pooling launch");
}

// One step of a forward's op loop: op i alone, or (`pair_ok`) ops i and i + 1 as one launch where the fused stem or the
// chain kernel takes them.  Returns the ops consumed (1 or 2); rc: the step's status.
static int launch_step(ym_ctx* c, const Launch& L, size_t i, bool pair_ok, int B, const float* d_in,
                       const ym_infer_args* args, float* d_dets, int* d_counts, hipStream_t st, int& rc) {
  if (pair_ok && (try_stem_fuse(c, L, i, B, d_in, args, st, rc) || try_chain(c, L, i, B, d_in, args, st, rc))) return 2;
  rc = launch_op(c, L, c->ops[i], B, d_in, args, d_dets, d_counts, st);
  return 1;
}

// Launch one forward of call.B images: the input statistics over the WHOLE batch (LoadTensor's /255 rule is a
// batch-wide max), then every other op per lane on its image slice.  With fork/join events the lanes are parallel
// graph branches when `st` is capturing; eagerly (no capture) they run on the lane streams concurrently as well.
static int launch_forward(ym_ctx* c, const Launch& call, const float* d_in, const ym_infer_args* args, float* d_dets,
                          int* d_counts, hipStream_t st) {
  const int B = call.B;
  int L, Bl, rc = YM_OK;
  lane_split(args, B, L, Bl);
  // ym_embed: ops [0, nops) only, every op its own launch (a two-op launch could run past the stop, and the fused
  // stem never stores model.0's output), then the pooling stage
  const bool embed = call.stop >= 0;
  const size_t nops = embed ? (size_t)call.stop + 1 : c->ops.size();
  if (L == 1 && c->nbr > 1) {  // one lane: the branch schedule (build_schedule)
    hipStream_t bs[kMaxLanes] = {st};
    bool opened[kMaxLanes] = {};  // streams that took an op (a whole forward: all nbr; a truncated one maybe fewer)
    for (int s = 1; s < kMaxLanes; ++s) bs[s] = c->lane_streams[s];
    for (size_t i = 0; i < nops;) {
      const int s = c->br_of[i];
      opened[s] = true;
      for (int j : c->br_wait[i]) HIPCK(hipStreamWaitEvent(bs[s], c->op_ev[j], 0));
      Launch l = call;
      l.lane = s;  // split-K slab / counter region of this stream
      const int n = launch_step(c, l, i, !embed, B, d_in, args, d_dets, d_counts, bs[s], rc);
      if (rc) return rc;
      for (const size_t end = i + n; i < end; ++i)  // (both ops of a two-op launch)
        if (c->br_rec[i]) HIPCK(hipEventRecord(c->op_ev[i], bs[s]));
    }
    for (int s = 1; s < c->nbr; ++s) {  // every branch that was opened joins back into the caller's stream
      if (!opened[s]) continue;
      HIPCK(hipEventRecord(c->join_ev[s], bs[s]));
      HIPCK(hipStreamWaitEvent(st, c->join_ev[s], 0));
    }
    return embed && call.pool ? launch_embed(c, B, st) : YM_OK;  // (the pooling stage reads behind the join)
  }
  size_t o = 0;
  for (o = 0; o < nops && c->ops[o].kind == OP_INPUT; ++o)
    if ((rc = launch_op(c, call, c->ops[o], B, d_in, args, d_dets, d_counts, st))) return rc;
  if (L > 1) HIPCK(hipEventRecord(c->fork_ev, st));
  const size_t in_img = (size_t)3 * c->cH * c->cW, det_img = (size_t)args->max_det * (6 + c->nm);
  for (int ln = 0; ln < L; ++ln) {
    hipStream_t ls = ln == 0 ? st : c->lane_streams[ln];
    if (ln > 0) HIPCK(hipStreamWaitEvent(ls, c->fork_ev, 0));
    Launch l = call;
    l.lane = ln;
    l.img0 = ln * Bl;
    const int nb = B - l.img0 < Bl ? B - l.img0 : Bl;
    for (size_t i = o; i < nops;) {
      i += launch_step(c, l, i, L == 1 && !embed, nb, d_in + l.img0 * in_img, args, d_dets + l.img0 * det_img,
                       d_counts + l.img0, ls, rc);
      if (rc) return rc;
    }
    if (ln > 0) {
      HIPCK(hipEventRecord(c->join_ev[ln], ls));
      HIPCK(hipStreamWaitEvent(st, c->join_ev[ln], 0));
    }
  }
  return embed && call.pool ? launch_embed(c, B, st) : YM_OK;  // (ym_embed runs one lane: everything above is on `st`)
}

// ym_infer, (skip_nms) ym_tta_forward and (stop >= 0) ym_embed
static int infer_impl(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
                      int* d_counts, void* stream, bool skip_nms, int stop, const ClsOut* cls = nullptr) {
  int rc = check_call(c, d_in, B, H, W, args, d_dets, d_counts);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Launch L;
  if ((rc = begin_launch(c, B, H, W, st, L))) return rc;
  L.skip_nms = skip_nms; L.stop = stop;
  if (cls) L.cls = *cls;
  // YM_DBG_STOP (tests): an eager forward that ends behind op value - 1, every op its own launch as ym_embed's
  // truncated forward but with no pooling stage.  Never captured: a stopped forward must not be cached as, or
  // replayed for, a whole one
  if (const int dbg_stop = ym_debug_get(YM_DBG_STOP); dbg_stop > 0 && stop < 0) {
    if (args->use_graph) return fail(YM_EINVAL, "YM_DBG_STOP is set: eager forwards only (use_graph = 0)");
    if (dbg_stop > (int)c->ops.size()) return fail(YM_EINVAL, "YM_DBG_STOP: op %d of %zu", dbg_stop - 1, c->ops.size());
    L.stop = dbg_stop - 1;
    L.pool = false;
  }
  c->taken.assign(2 * c->ops.size(), -1);
  c->variant.assign(c->ops.size(), -1);
  c->tkB = B; c->tkH = H; c->tkW = W;
  if (!args->use_graph) {
    if ((rc = launch_forward(c, L, d_in, args, d_dets, d_counts, st))) return rc;
    return c->mark_last(st);
  }
  GraphKey key;
  memset(&key, 0, sizeof(key));
  key.B = B; key.H = H; key.W = W; key.in = d_in; key.dets = nullptr; key.counts = d_counts; key.args = *args;
  key.skip_nms = L.skip_nms ? 1 : 0;
  key.cls = L.cls;
  const bool embed = L.stop >= 0;
  if (embed) {
    key.embed_stop = L.stop + 1;
    key.embed_n = (int)c->embed_views.size();
    key.embed_out = c->embed_out;
    key.embed_ld = c->embed_ld;
  }
  auto same_views = [&](const GraphEntry& g) {
    return !embed || (g.embed_views.size() == c->embed_views.size() &&
                      memcmp(g.embed_views.data(), c->embed_views.data(), g.embed_views.size() * sizeof(ym_embed_view)) == 0);
  };
  GraphKey key_d = key;  // the key of a graph whose NMS nodes could not be re-pointed
  key_d.dets = d_dets;
  for (auto& g : c->graphs) {
    if ((g.key == key || g.key == key_d) && same_views(g)) {
      // re-pointable: new rows through the NMS nodes' parameters.  A launch already queued keeps the parameters it
      // was launched with (hipGraphExecKernelNodeSetParams changes later launches only:
      // tests/test_gpu_kernels.py test_repointed_graph_rows_with_no_sync_between_calls), so no wait here — an
      // asynchronous predict() loop enqueues the next forward while the previous one runs
      if (g.key == key && g.dets != d_dets && (rc = repoint_dets(g, d_dets))) return rc;
      return c->launch_graph(g, st);
    }
  }
  if (c->graphs.size() >= kMaxGraphs) {  // evict the oldest capture once its last replay has drained
    c->retire(c->graphs.front());
    c->graphs.erase(c->graphs.begin());
  }
  // capture on the private stream (lane streams join through the fork event), replay on the caller's stream
  HIPCK(hipStreamBeginCapture(c->cap_stream, hipStreamCaptureModeRelaxed));
  if ((rc = launch_forward(c, L, d_in, args, d_dets, d_counts, c->cap_stream))) {
    hipGraph_t g = nullptr;
    (void)hipStreamEndCapture(c->cap_stream, &g);
    if (g) (void)hipGraphDestroy(g);
    return rc;
  }
  GraphEntry ge;
  HIPCK(hipStreamEndCapture(c->cap_stream, &ge.graph));
  hipError_t e = hipGraphInstantiate(&ge.exec, ge.graph, nullptr, nullptr, 0);
  if (e == hipSuccess) e = hipEventCreateWithFlags(&ge.done, hipEventDisableTiming);
  if (e != hipSuccess) {
    retire_graph(ge);
    return fail(YM_EHIP, "graph instantiate: %s", hipGetErrorString(e));
  }
  ge.dets = d_dets;
  if (embed) ge.embed_views = c->embed_views;
  static const bool no_repoint = [] { const char* v = getenv("YM_GRAPH_REPOINT"); return v && *v == '0'; }();
  ge.key = (!no_repoint && find_nms_nodes(ge)) ? key : key_d;
  c->graphs.push_back(ge);
  return c->launch_graph(c->graphs.back(), st);
}

int ym_infer(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
             int* d_counts, void* stream) {
  if (c && c->loaded && c->task == kTaskClassify)
    return fail(YM_EINVAL, "ym_infer: a classify plan has no detections (ym_classify runs it)");
  return infer_impl(c, d_in, B, H, W, args, d_dets, d_counts, stream, false, -1);
}

// ---------------------------------------------------------------------------------- oriented boxes
int ym_obb_nms(ym_ctx* c, const float* d_rows, int B, int H, int W, const ym_infer_args* args, float* d_dets,
               int* d_counts, void* stream) {
  if (int rc = check_ctx(c, "ym_obb_nms", kTaskObb, "an obb")) return rc;
  if (!d_rows || !args || !d_dets || !d_counts) return fail(YM_EINVAL, "null pointer argument");
  if (int rc = check_shape(B, H, W, "ym_obb_nms: ")) return rc;
  if (int rc = check_nms_args(args, c->nc, c->task)) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Launch L;
  if (int rc = begin_launch(c, B, H, W, st, L)) return rc;
  // the candidate counts start at 0 (the forward's input op clears them; this entry point is never captured)
  HIPCK(hipMemsetAsync(nms_view(c->d_arena, c->nms, 0).counts, 0, (size_t)B * 4, st));
  int* c2 = args->counts_after_dets ? counts_behind(d_dets, B, args->max_det, 7, 0) : nullptr;
  const ObbArgs a = obb_args(c, d_rows, 0, B, args, d_dets, d_counts, c2);
  if (int rc = launched(ym_launch_obb_decode(a, st), "ym_obb_nms launch")) return rc;
  if (int rc = launched(ym_launch_obb_nms(a, st), "ym_obb_nms launch")) return rc;
  return c->mark_last(st);
}

// ---------------------------------------------------------------------------------- classification
int ym_classify(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_probs, int ld,
                float* d_logits, int* d_topk, float* d_topk_conf, void* stream) {
  if (int rc = check_ctx(c, "ym_classify", kTaskClassify, "a classify")) return rc;
  if (!d_in || !args || !d_probs || !d_topk || !d_topk_conf) return fail(YM_EINVAL, "null pointer argument");
  if (ld < c->nc) return fail(YM_EINVAL, "ym_classify: row stride %d below the %d classes", ld, c->nc);
  const ym_infer_args fa = forward_only_args(args);  // (no detection output is written)
  const ClsOut out{d_probs, ld, d_logits, d_topk, d_topk_conf};
  return infer_impl(c, d_in, B, H, W, &fa, no_dets(c), reinterpret_cast<int*>(no_dets(c)), stream, false, -1, &out);
}

// ---------------------------------------------------------------------------------- test-time augmentation
int ym_tta_shape(int H, int W, int pass, int* Hs, int* Ws, int* hc, int* wc) {
  if (int rc = check_shape(1, H, W, "ym_tta_shape: ")) return rc;
  if (pass < 0 || pass >= kTtaPasses) return fail(YM_EINVAL, "ym_tta_shape: pass is 0..%d", kTtaPasses - 1);
  int v[4], *const out[4] = {Hs, Ws, hc, wc};
  ym_tta_pass_shape(H, W, pass, v[0], v[1], v[2], v[3]);
  for (int i = 0; i < 4; ++i)
    if (out[i]) *out[i] = v[i];
  return YM_OK;
}

int ym_tta_scale(ym_ctx* c, const float* d_in, int B, int H, int W, int pass, const float* d_max, float in_eps,
                 float* d_out, void* stream) {
  if (!c || !d_in || !d_max || !d_out) return fail(YM_EINVAL, "null argument");
  if (int rc = check_shape(B, H, W, "ym_tta_scale: ")) return rc;
  if (pass < 1 || pass >= kTtaPasses) return fail(YM_EINVAL, "ym_tta_scale: pass %d (1 or 2)", pass);
  HIPCK(hipSetDevice(c->device));
  TtaScaleArgs a{};
  a.in = d_in; a.B = B; a.H = H; a.W = W; a.out = d_out;
  ym_tta_pass_shape(H, W, pass, a.Hs, a.Ws, a.hc, a.wc);
  a.flip = kTtaFlip[pass]; a.batch_max = d_max; a.eps = in_eps;
  return launched(ym_launch_tta_scale(a, static_cast<hipStream_t>(stream)), "tta scale launch");
}

int ym_tta_forward(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, void* stream) {
  if (!c || !args) return fail(YM_EINVAL, "null argument");
  if (c->loaded && c->task != 0)
    return fail(YM_EINVAL, "test-time augmentation: %s plans are not supported (detect plans only)", ym_task_name(c->task));
  ym_infer_args fa = *args;  // one capture serves the single- and the multi-label NMS that follows
  fa.multi_label = 0;
  fa.counts_after_dets = 0;
  // (the NMS stage is the only reader of the outputs: any device words do, they are never written)
  return infer_impl(c, d_in, B, H, W, &fa, no_dets(c), reinterpret_cast<int*>(no_dets(c)), stream, true, -1);
}

// ---------------------------------------------------------------------------------- feature embeddings
int ym_embed(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, const ym_embed_view* views,
             int n_views, float* d_out, long long out_stride, void* stream) {
  if (int rc = check_ctx(c, "ym_embed")) return rc;
  if (!d_in || !args || !views || !d_out) return fail(YM_EINVAL, "null pointer argument");
  if (c->task == kTaskObb) return fail(YM_EINVAL, "ym_embed: obb plans are not supported");
  if (ym_dt_q8(c->dtype))
    return fail(YM_EINVAL, "ym_embed: the quantized plans are not supported (their stored codes need each buffer's "
                           "scale and zero point); use an x3, f16 or f32 plan");
  if (int rc = check_shape(B, H, W, "")) return rc;
  if (n_views < 1 || n_views > kEmbedMaxViews)
    return fail(YM_EINVAL, "ym_embed: %d views (1..%d)", n_views, kEmbedMaxViews);
  long long cols = 0;
  std::vector<char> want(c->bufs.size(), 0);
  for (int i = 0; i < n_views; ++i) {
    const ym_embed_view& v = views[i];
    if (v.buf < 0 || v.buf >= (int)c->bufs.size() || v.buf == c->input_buf || c->bufs[v.buf].f < 1)
      return fail(YM_EINVAL, "ym_embed: view %d names buffer %d, which is not a feature map of this plan", i, v.buf);
    if (v.coff < 0 || v.C < 8 || v.coff % 8 || v.C % 8 || (long long)v.coff + v.C > c->bufs[v.buf].C)
      return fail(YM_EINVAL, "ym_embed: view %d, channels [%d, %d + %d) of buffer %d (%d channels): outside the buffer "
                             "or not in groups of 8", i, v.coff, v.coff, v.C, v.buf, c->bufs[v.buf].C);
    want[v.buf] = 1;
    cols += v.C;
  }
  if (out_stride < cols)
    return fail(YM_EINVAL, "ym_embed: row stride %lld below the %lld pooled channels", out_stride, cols);
  // the forward runs up to and including the last op that writes a requested buffer
  int stop = -1;
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const int w = op_writes(c->ops[i]);
    if (w >= 0 && w < (int)want.size() && want[w]) {
      want[w] = 2;
      stop = (int)i;
    }
  }
  for (size_t b = 0; b < want.size(); ++b)
    if (want[b] == 1) return fail(YM_EINVAL, "ym_embed: no op of this plan stores buffer %zu", b);
  HIPCK(hipSetDevice(c->device));
  c->embed_views.assign(views, views + n_views);
  c->embed_out = d_out;
  c->embed_ld = out_stride;
  EmbedArgs ea;
  embed_args(c, B, H, W, false, ea);
  const long need = ym_embed_part_floats(ea);
  if (need < 0) return fail(YM_EINVAL, "ym_embed: bad view table");
  const size_t part_bytes = (size_t)need * sizeof(float);
  if (part_bytes > c->embed.bytes) c->clear_graphs();  // the chunk partials grow: no captured pooling stage may keep the old ones
  if (int rc = c->embed.grow(part_bytes, "embed partials hipMalloc(%zu floats)", (size_t)need)) return rc;
  const ym_infer_args fa = forward_only_args(args);  // (the truncated forward; no output is written)
  return infer_impl(c, d_in, B, H, W, &fa, no_dets(c), reinterpret_cast<int*>(no_dets(c)), stream, false, stop);
}

// the merged scratch of ctxs[0] for B images of an H x W frame: Am merged anchors, multi-label regions on demand
static int ensure_tta(ym_ctx* c, int B, int H, int W, int Am, bool ml) {
  ym_ctx::TtaWs& t = c->tta;
  if (t.d && B <= t.B && H == t.H && W == t.W && Am == t.ws.A && c->nc == t.nc && (!ml || t.ws.ml)) return YM_OK;
  if (t.d) {
    HIPCK(hipDeviceSynchronize());  // an earlier merge / NMS on any stream may still use the old scratch
    HIPCK(hipFree(t.d));
    t.d = nullptr;
  }
  const int nB = (H == t.H && W == t.W && Am == t.ws.A && B < t.B) ? t.B : B;
  ml = ml || (t.ws.ml && H == t.H && W == t.W);
  t.B = 0;
  t.H = H; t.W = W; t.nc = c->nc;
  const size_t bytes = nms_scratch_append(t.ws, 0, nB, Am, ml, ml ? c->nc : 0);
  const hipError_t e = hipMalloc(&t.d, bytes);
  if (e != hipSuccess) {
    t.d = nullptr;
    return fail(YM_ENOMEM, "tta scratch hipMalloc(%zu) failed: %s", bytes, hipGetErrorString(e));
  }
  HIPCK(hipMemset(t.d, 0, bytes));
  t.B = nB;
  return YM_OK;
}

int ym_tta_nms(ym_ctx* const* ctxs, int B, int H, int W, const ym_infer_args* args, float* d_dets, int* d_counts,
               void* stream) {
  if (!ctxs || !args || !d_dets || !d_counts) return fail(YM_EINVAL, "null pointer argument");
  if (int rc = check_shape(B, H, W, "")) return rc;
  ym_ctx* c = ctxs[0];
  for (int p = 0; p < kTtaPasses; ++p) {
    ym_ctx* q = ctxs[p];
    if (!q) return fail(YM_EINVAL, "null context for pass %d", p);
    if (!q->loaded) return fail(YM_ESTATE, "ym_tta_nms before ym_load_weights (pass %d)", p);
    for (int r = 0; r < p; ++r)
      if (ctxs[r] == q) return fail(YM_EINVAL, "passes %d and %d share a context: every pass needs its own workspace", r, p);
    if (q->task != 0)
      return fail(YM_EINVAL, "test-time augmentation: %s plans are not supported (detect plans only)", ym_task_name(q->task));
    if (q->device != c->device || q->dtype != c->dtype || q->nc != c->nc || q->reg_max != c->reg_max || q->nl != c->nl ||
        q->no != c->no || q->nm != 0 || memcmp(q->strides, c->strides, sizeof(c->strides)) ||
        q->bufs[q->anchor_buf].C != c->bufs[c->anchor_buf].C)
      return fail(YM_EINVAL, "pass %d's context does not hold the plan of pass 0", p);
    int Hs, Ws, hc, wc;
    ym_tta_pass_shape(H, W, p, Hs, Ws, hc, wc);
    if (!q->d_arena || q->cB < B || q->cH != Hs || q->cW != Ws)
      return fail(YM_ESTATE, "pass %d: ym_tta_nms must follow ym_tta_forward of (%d,3,%d,%d) (workspace %dx%dx%d)", p, B, Hs,
                  Ws, q->cB, q->cH, q->cW);
  }
  if (int rc = check_nms_args(args, c->nc, c->task)) return rc;
  const bool ml = args->multi_label && c->nc > 1;
  HIPCK(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  // _clip_augmented (g = 21 = 1 + 4 + 16 grid points per stride-32 cell): pass 0 without its last A / 21 anchors,
  // the last pass without its first (A / 21) * 16
  TtaMergeArgs m{};
  int Am = 0;
  for (int p = 0; p < kTtaPasses; ++p) {
    ym_ctx* q = ctxs[p];
    TtaPass& P = m.p[p];
    P.A = q->A;
    P.first = p == kTtaPasses - 1 ? (q->A / 21) * 16 : 0;
    P.keep = p == 0 ? q->A - q->A / 21 : q->A - P.first;
    P.base = Am;
    Am += P.keep;
    P.anchors = reinterpret_cast<const float*>(q->d_arena + q->buf_off[q->anchor_buf]);
    const NmsView qv = nms_view(q->d_arena, q->nms, 0);
    P.boxes = qv.boxes; P.scores = qv.scores; P.cls = qv.cls;
    for (int l = 0; l < q->nl; ++l) { P.lvl_W[l] = q->lvl_W[l]; P.lvl_off[l] = q->lvl_off[l]; }
    P.s = (float)kTtaRatio[p];
    P.flip = kTtaFlip[p];
  }
  if (int rc = ensure_tta(c, B, H, W, Am, ml)) return rc;
  const NmsView v = nms_view(c->tta.d, c->tta.ws, 0);
  if (int rc = c->order_after_last(st)) return rc;  // (the scratch's previous user: ctxs[0]'s last call)
  m.no_tot = c->bufs[c->anchor_buf].C; m.nc = c->nc; m.reg_max = c->reg_max; m.nl = c->nl;
  for (int l = 0; l < c->nl; ++l) m.lvl_stride[l] = (float)c->strides[l];
  m.boxes = v.boxes; m.scores = v.scores; m.cls = v.cls; m.keys = v.keys; m.counts = v.counts;
  m.rows = ml ? v.rows : nullptr;
  m.Am = Am; m.kstride = v.kstride; m.B = B;
  set_filter(m, args);
  m.img_w = (float)W;
  if (!ml) HIPCK(hipMemsetAsync(m.counts, 0, (size_t)B * 4, st));
  if (int rc = launched(ym_launch_tta_merge(m, st), "tta merge launch")) return rc;
  // no extras (detect plans: nm = 0); multi-label thresholds the merged class rows
  const NmsSource src{nullptr, 0, 0, m.rows, c->nc, 0};
  int* counts2 = args->counts_after_dets ? counts_behind(d_dets, B, args->max_det, 6, 0) : nullptr;
  const hipError_t e = launch_nms_stage(v, src, args, B, c->nc, 0, H, W, d_dets, d_counts, counts2, st);
  if (int rc = launched(e, "tta NMS launch")) return rc;
  // the merge read every pass's arena: a later forward of any of them on another stream waits for this call
  for (int p = 0; p < kTtaPasses; ++p)
    if (int rc = ctxs[p]->mark_last(st)) return rc;
  return YM_OK;
}

int ym_tta_counts(ym_ctx* c, int* dst, int B) {
  if (!c || !dst || B < 1) return fail(YM_EINVAL, "bad ym_tta_counts arguments");
  if (!c->tta.d || B > c->tta.B) return fail(YM_ESTATE, "no merged scratch for %d images yet (run ym_tta_nms first)", B);
  return read_back(c->device, dst, c->tta.d + c->tta.ws.counts.off, (size_t)B * 4);
}

int ym_input_max(ym_ctx* c, const float* d_in, size_t n, float* d_max, void* stream) {
  if (!c || !d_in || !d_max || n == 0) return fail(YM_EINVAL, "bad ym_input_max arguments");
  HIPCK(hipSetDevice(c->device));
  return launched(ym_launch_input_max(d_in, (long)n, reinterpret_cast<float*>(c->d_misc + kMiscStats), d_max,
                                      static_cast<hipStream_t>(stream)), "input max");
}

int ym_calibrate(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
                 int* d_counts, float* const* d_raw, int n_ops, void* stream) {
  int rc = check_call(c, d_in, B, H, W, args, d_dets, d_counts);
  if (rc) return rc;
  if (c->dtype != YM_DT_F32) return fail(YM_ESTATE, "ym_calibrate needs an f32 (parity) plan");
  if (!d_raw || n_ops != (int)c->ops.size()) return fail(YM_EINVAL, "d_raw must hold %zu entries", c->ops.size());
  hipStream_t st = static_cast<hipStream_t>(stream);
  Launch L;
  if ((rc = begin_launch(c, B, H, W, st, L))) return rc;
  ym_infer_args one = *args;
  one.lanes = 1;
  L.calib_raw = d_raw;
  if ((rc = launch_forward(c, L, d_in, &one, d_dets, d_counts, st))) return rc;
  return c->mark_last(st);  // (a later forward on another stream waits for this one on the shared arena)
}

int ym_profile(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
               int* d_counts, void* stream, float* op_ms, int n_ops) {
  int rc = check_call(c, d_in, B, H, W, args, d_dets, d_counts);
  if (rc) return rc;
  if (!op_ms || n_ops < (int)c->ops.size()) return fail(YM_EINVAL, "op_ms must hold %zu entries", c->ops.size());
  hipStream_t st = static_cast<hipStream_t>(stream);
  Launch L;
  if ((rc = begin_launch(c, B, H, W, st, L))) return rc;
  const size_t ne = c->ops.size() + 1;
  while (c->prof_events.size() < ne) {
    hipEvent_t e;
    HIPCK(hipEventCreate(&e));
    c->prof_events.push_back(e);
  }
  // park the stream first so the host has queued every op + event before the GPU reaches them: the event pairs
  // then bracket device execution only (an eager host launch takes longer than most of these kernels)
  HIPCK(ym_launch_spin(20 * (int)c->ops.size() + 2000, st));
  HIPCK(hipEventRecord(c->prof_events[0], st));
  for (size_t i = 0; i < c->ops.size(); ++i) {
    if ((rc = launch_op(c, L, c->ops[i], B, d_in, args, d_dets, d_counts, st))) return rc;
    HIPCK(hipEventRecord(c->prof_events[i + 1], st));
  }
  HIPCK(hipEventSynchronize(c->prof_events[ne - 1]));
  for (size_t i = 0; i < c->ops.size(); ++i)
    HIPCK(hipEventElapsedTime(&op_ms[i], c->prof_events[i], c->prof_events[i + 1]));
  return YM_OK;
}

int ym_profile_replay(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
                      int* d_counts, void* stream, int reps, float* op_ms, int n_ops) {
  int rc = check_call(c, d_in, B, H, W, args, d_dets, d_counts);
  if (rc) return rc;
  if (!op_ms || n_ops < (int)c->ops.size()) return fail(YM_EINVAL, "op_ms must hold %zu entries", c->ops.size());
  if (reps < 1) reps = 20;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Launch L;
  if ((rc = begin_launch(c, B, H, W, st, L))) return rc;
  // one real forward so every buffer holds this input's activations (and the /255 flag is set)
  for (const Op& op : c->ops)
    if ((rc = launch_op(c, L, op, B, d_in, args, d_dets, d_counts, st))) return rc;
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op& op = c->ops[i];
    const int k = op.kind;
    op_ms[i] = -1.f;
    // input (resets counters), decode (appends candidates) and NMS (consumes them) are not idempotent: skipped
    if (k != OP_CONV && k != OP_DW && k != OP_SPPF && k != OP_ATTN && k != OP_CLASSIFY) continue;
    int lrc = YM_OK;
    float ms = 0.f;
    auto launch = [&](hipStream_t s) { return launch_op(c, L, op, B, d_in, args, d_dets, d_counts, s); };
    if ((rc = time_captured(c, st, reps, 1, launch, lrc, ms))) return rc;
    if (lrc != YM_OK) return lrc;
    op_ms[i] = ms / reps;
  }
  return YM_OK;
}

int ym_tune(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
            int* d_counts, void* stream, int reps) {
  int rc = check_call(c, d_in, B, H, W, args, d_dets, d_counts);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Launch L;
  if ((rc = begin_launch(c, B, H, W, st, L))) return rc;
  if (reps < 1) reps = 8;
  // one real forward first so every buffer a candidate reads holds this model's activations
  c->drop_cfg(B, H, W);
  for (const Op& op : c->ops)
    if ((rc = launch_op(c, L, op, B, d_in, args, d_dets, d_counts, st))) return rc;
  HIPCK(hipStreamSynchronize(st));
  std::vector<int> best(c->ops.size(), -1);
  const int ncfg = ymc::num_cfgs(c->dtype);
  const char* tl = getenv("YM_TUNE_LOG");  // per-candidate timings to stderr (tools/)
  const bool tune_log = tl && *tl && *tl != '0';
  for (size_t i = 0; i < c->ops.size(); ++i) {
    const Op& op = c->ops[i];
    if (op.kind != OP_CONV) continue;
    ConvArgs a;
    int out_f32 = 0;
    if ((rc = conv_args(c, L, op, B, d_in, args->in_eps, a, out_f32))) return rc;
    if (a.nchw) continue;  // the stem has its own kernel (csrc/ym_stem.hip)
    // best config of one conv launch (bcf, its time bt; -1: none launched): `reps` back-to-back launches of each
    // candidate, replayed twice between the events
    auto tune_one = [&](const ConvArgs& ca, int of32, int& bcf, float& bt) -> int {
      bt = 1e30f;
      bcf = -1;
      for (int cf = 0; cf < ncfg; ++cf) {
        int lrc = 0;
        float ms = 0.f;
        auto launch = [&](hipStream_t s) { return (int)ym_launch_conv(c->dtype, of32, ca, cf, s, true); };
        if (int trc = time_captured(c, st, reps, 2, launch, lrc, ms)) return trc;
        if (lrc != 0) continue;  // this configuration does not take the shape
        if (tune_log) fprintf(stderr, "[ym_tune] %s cfg %d: %.2f us\n", op.name, cf, ms * 1e3f / (2 * reps));
        if (ms < bt) { bt = ms; bcf = cf; }
      }
      return YM_OK;
    };
    int cf = -1;
    float tf = 0.f;
    if ((rc = tune_one(a, out_f32, cf, tf))) return rc;
    best[i] = cf;
    if (a.w2) {  // fused pair: also the two convs as separate tuned launches
      ConvArgs A, Bc;
      split_args(c, L, op, a, A, Bc);
      int ca = -1, cb = -1;
      float ta = 0.f, tb = 0.f;
      if ((rc = tune_one(A, 0, ca, ta)) || (rc = tune_one(Bc, out_f32, cb, tb))) return rc;
      if (ca >= 0 && cb >= 0 && ta + tb < tf) best[i] = ymc::split_encode(ca, cb);
    }
  }
  c->clear_graphs();
  c->put_cfg(B, H, W, best);
  return YM_OK;
}

int ym_get_op_cfg(ym_ctx* c, int B, int H, int W, int* cfg, int n) {
  if (!c || !cfg || n < (int)c->ops.size()) return fail(YM_EINVAL, "cfg array must hold %zu entries", c ? c->ops.size() : 0);
  const std::vector<int>* v = c->find_cfg(B, H, W);
  for (size_t i = 0; i < c->ops.size(); ++i) cfg[i] = (v && i < v->size()) ? (*v)[i] : -1;
  return v ? YM_OK : 1;
}

int ym_set_op_cfg(ym_ctx* c, int B, int H, int W, const int* cfg, int n) {
  if (!c || !cfg || n != (int)c->ops.size()) return fail(YM_EINVAL, "cfg array must hold %zu entries", c ? c->ops.size() : 0);
  const int ncfg = ymc::num_cfgs(c->dtype);
  for (int i = 0; i < n; ++i) {
    if (ymc::is_split(cfg[i]) && c->ops[i].kind == OP_CONV && c->ops[i].k2 && ymc::split_first(cfg[i]) < ncfg &&
        ymc::split_second(cfg[i]) < ncfg)
      continue;  // a fused pair run as two launches
    if (cfg[i] >= ncfg) return fail(YM_EINVAL, "cfg[%d] = %d out of range", i, cfg[i]);
  }
  c->put_cfg(B, H, W, std::vector<int>(cfg, cfg + n));
  c->clear_graphs();
  return YM_OK;
}

int ym_get_op_cfg_taken(ym_ctx* c, int B, int H, int W, int* out, int n) {
  if (!c || !out || n < 2 * (int)c->ops.size())
    return fail(YM_EINVAL, "taken array must hold %zu entries", c ? 2 * c->ops.size() : 0);
  if (c->taken.size() != 2 * c->ops.size() || B != c->tkB || H != c->tkH || W != c->tkW)
    return fail(YM_ESTATE, "ym_get_op_cfg_taken: the last forward was not a %d x %d x %d one", B, H, W);
  for (size_t i = 0; i < c->taken.size(); ++i) out[i] = c->taken[i];
  return YM_OK;
}

int ym_get_op_variant(ym_ctx* c, int B, int H, int W, int* out, int n) {
  if (!c || !out || n < (int)c->ops.size()) return fail(YM_EINVAL, "variant array must hold %zu entries", c ? c->ops.size() : 0);
  if (c->variant.size() != c->ops.size() || B != c->tkB || H != c->tkH || W != c->tkW)
    return fail(YM_ESTATE, "ym_get_op_variant: the last forward was not a %d x %d x %d one", B, H, W);
  for (size_t i = 0; i < c->variant.size(); ++i) out[i] = c->variant[i];
  return YM_OK;
}

int ym_op_variant_count(int kind) {
  switch (kind) {
    case YM_OP_DWCONV: return YM_DWV_COUNT;
    case YM_OP_SPPF: return YM_SPPFV_COUNT;
    case YM_OP_ATTN: return YM_ATTNV_COUNT;
    default: return fail(YM_EINVAL, "ym_op_variant_count: kind %d", kind);
  }
}

int ym_num_ops(ym_ctx* c) { return c ? (int)c->ops.size() : fail(YM_EINVAL, "null context"); }

const char* ym_op_name(ym_ctx* c, int i) {
  if (!c || i < 0 || i >= (int)c->ops.size()) return "";
  return c->ops[i].name;
}

int ym_num_buffers(ym_ctx* c) { return c ? (int)c->bufs.size() : fail(YM_EINVAL, "null context"); }

int ym_buffer_info(ym_ctx* c, int b, void** ptr, int* C, int* H, int* W, int* elem_bytes) {
  if (!c || b < 0 || b >= (int)c->bufs.size()) return fail(YM_EINVAL, "bad buffer id");
  if (!c->d_arena) return fail(YM_ESTATE, "no workspace yet (run ym_infer first)");
  if (ptr) *ptr = c->bptr(b, 0);
  if (C) *C = c->bufs[b].C;
  if (H) *H = c->buf_H(b);
  if (W) *W = c->buf_Wd(b);
  if (elem_bytes) *elem_bytes = c->elem(b);
  return YM_OK;
}

int ym_read_buffer(ym_ctx* c, int b, void* dst, size_t bytes) {
  if (!c || b < 0 || b >= (int)c->bufs.size() || !dst) return fail(YM_EINVAL, "bad buffer id or null dst");
  if (!c->d_arena) return fail(YM_ESTATE, "no workspace yet (run ym_infer first)");
  const size_t cap = (size_t)c->cB * c->buf_P(b) * c->bufs[b].C * c->elem(b);
  if (bytes > cap) return fail(YM_EINVAL, "read of %zu bytes exceeds buffer size %zu", bytes, cap);
  return read_back(c->device, dst, c->bptr(b, 0), bytes);
}

int ym_kpt_shape(ym_ctx* c, int* K, int* ndim) {
  if (int rc = check_ctx(c, "ym_kpt_shape")) return rc;
  if (K) *K = c->kpt_K;
  if (ndim) *ndim = c->kpt_ndim;
  return YM_OK;
}

int ym_read_scratch(ym_ctx* c, int which, void* dst, size_t bytes) {
  if (!c || !dst) return fail(YM_EINVAL, "null context or dst");
  if (!c->d_arena) return fail(YM_ESTATE, "no workspace yet (run ym_infer first)");
  size_t off = 0, cap = 0;
  switch (which) {
    case YM_SCRATCH_KEYS: off = c->nms.keys.off; cap = c->cB * c->nms.keys.stride; break;
    case YM_SCRATCH_COUNTS: off = c->nms.counts.off; cap = c->cB * c->nms.counts.stride; break;
    case YM_SCRATCH_KPTS:
      if (c->task != kTaskPose) return fail(YM_ESTATE, "YM_SCRATCH_KPTS needs a pose plan");
      off = c->off_kpts; cap = (size_t)c->cB * c->A * c->nm * 4;
      break;
    case YM_SCRATCH_POOLED:
      if (c->task != kTaskClassify) return fail(YM_ESTATE, "YM_SCRATCH_POOLED needs a classify plan");
      off = c->off_cls; cap = (size_t)c->cB * kClsHidden * 4;
      break;
    case YM_SCRATCH_OBB_BOXES: case YM_SCRATCH_OBB_COV: case YM_SCRATCH_OBB_SCORES: case YM_SCRATCH_OBB_CLS: {
      if (c->task != kTaskObb) return fail(YM_ESTATE, "the YM_SCRATCH_OBB_* regions need an obb plan");
      const NmsRegion& r = which == YM_SCRATCH_OBB_BOXES ? c->nms.boxes : which == YM_SCRATCH_OBB_SCORES ? c->nms.scores
                                                                                                         : c->nms.cls;
      off = which == YM_SCRATCH_OBB_COV ? c->off_obb_cov : r.off;
      cap = (size_t)c->cB * (which == YM_SCRATCH_OBB_COV ? (size_t)c->A * 16 : r.stride);
      break;
    }
    default: return fail(YM_EINVAL, "unknown scratch region %d", which);
  }
  if (bytes > cap) return fail(YM_EINVAL, "read of %zu bytes exceeds region size %zu", bytes, cap);
  return read_back(c->device, dst, c->d_arena + off, bytes);
}

int ym_sync(ym_ctx* c) {
  if (!c) return fail(YM_EINVAL, "null context");
  HIPCK(hipSetDevice(c->device));
  HIPCK(hipDeviceSynchronize());
  return YM_OK;
}

void ym_destroy(ym_ctx* c) { delete c; }

}  // extern "C"
