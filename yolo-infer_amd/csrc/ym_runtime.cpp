// yolomi runtime: model-blob parsing, device weight/workspace arena, per-op launch, HIP-graph cache, C-ABI.
//
// This is the native replacement for the Ultralytics predictor loop that `YOLO11Model.predict` delegates to
// (/root/reference/core/model.py:118-133): per batch it replays ONE captured HIP graph of the whole forward
// (input /255 rule → 80+ fused conv launches → attention → decode → NMS), so the Python host issues one call.
#include <hip/hip_runtime.h>

#include <dlfcn.h>
#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/yolomi.h"
#include "ym_common.h"
#include "ym_plan.h"
#include "ym_nms_ws.h"
#include "ym_embed.h"
#include "ym_tta.h"
#include "ym_track.h"
#include "ym_annot.h"
#include "ym_contour.h"

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

int fail(int code, const char* fmt, ...) {
  char buf[512];
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(buf, sizeof(buf), fmt, ap);
  va_end(ap);
  g_err = buf;
  return code;
}

#define HIPCK(x)                                                                              \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) return fail(YM_EHIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

constexpr int kSplitCounters = 16384;  // split-K tiles per conv launch (csrc/ym_conv_dma.hip)
constexpr int kChainCtl = 4096;        // ready counters (+ done, give-up words) of the persistent chain kernel
constexpr float kPresortConf = 0.1f;  // NMS keys presorted over several workgroups below this conf (ym_nms.hip)
constexpr int kMaxLanes = 4;           // concurrent batch slices in one forward graph (<= GPU_MAX_HW_QUEUES)
constexpr size_t kMaxGraphs = 16;      // captured forwards cached per context (the oldest is retired first)
// ym_ctx::d_misc and its sub-regions: ym_input_max's statistics (slots, ticket, partials), the control words of
// ym_broadcast_weights, and the words that stand in for the outputs of a forward that writes none (never written)
constexpr size_t kMiscBytes = 16384;
constexpr size_t kMiscStats = 0, kMiscBcast = 8192, kMiscNoDets = 12288;
static_assert(kMiscStats + YM_CTL_BYTES <= kMiscBcast && kMiscBcast + 2 * sizeof(unsigned long long) <= kMiscNoDets &&
                  kMiscNoDets < kMiscBytes, "the d_misc sub-regions fit in kMiscBytes and do not overlap");
static_assert(sizeof(MlState) == kMlStateBytes, "ym_nms_ws.h sizes the multi-label state rows");

// What one launch_forward / launch_op call works on.  A value built per call (and per lane or branch stream inside
// launch_forward), never context state: nothing is left to reset on an early return.
struct Launch {
  int lane = 0;           // split-K slab / counter region of the stream the ops go to
  int img0 = 0;           // first image of the ops being launched (a lane's slice of the batch)
  int B = 0;              // images of the whole call (all lanes)
  bool skip_nms = false;  // ym_tta_forward: the passes' candidates are merged first (ym_tta_nms)
  int stop = -1;          // ym_embed: the last op of the truncated forward (-1: a whole forward)
  bool pool = true;       // (stop >= 0) the embedding pooling stage follows; false: YM_DBG_STOP, a test's bare stop
  float* const* calib_raw = nullptr;  // ym_calibrate: per-op pre-activation output buffers (f32 plans)
};

struct GraphKey {
  int B, H, W;
  int skip_nms;  // 1: a ym_tta_forward capture (no NMS stage)
  int embed_stop;  // ym_embed captures: 1 + the last op of the truncated forward (0: a whole forward) ...
  int embed_n;     // ... the views pooled behind it (GraphEntry::embed_views) ...
  const void* embed_out;  // ... and where their means go
  long long embed_ld;
  const void* in;
  const void* dets;
  const void* counts;
  const void* stream_unused;
  ym_infer_args args;
  bool operator==(const GraphKey& o) const { return memcmp(this, &o, sizeof(GraphKey)) == 0; }
};

// A captured forward.  The detection rows are the caller's (a fresh tensor per predict() call, so the Results of
// earlier calls stay valid without a copy): the key leaves `dets` out when the graph's NMS nodes were found, and a
// replay for other rows re-points those nodes (hipGraphExecKernelNodeSetParams; the lanes' row offsets kept).
struct GraphEntry {
  GraphKey key;
  hipGraph_t graph;
  hipGraphExec_t exec;
  float* dets = nullptr;                 // the rows the exec's NMS nodes write now
  hipEvent_t done = nullptr;             // recorded behind every launch of `exec` (retire_graph waits on it)
  std::vector<hipGraphNode_t> nms_nodes;  // empty: dets is part of the key
  std::vector<NmsArgs> nms_args;
  std::vector<ym_embed_view> embed_views;  // a ym_embed capture: the pooled views (compared with the key)
};

// The NMS kernel nodes of a captured forward and their arguments (false when none is found: the caller keys the
// graph on the output pointer instead)
bool find_nms_nodes(GraphEntry& ge) {
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

int repoint_dets(GraphEntry& ge, float* d_dets) {
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

// Destroy a captured forward only after its last launch has finished on whatever stream it was replayed on: the
// HIP runtime may still hold the exec's launch state (kernel arguments, the packet chain) while it is in flight.
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

}  // namespace

struct ym_ctx {
  int device = 0;
  ym_model_desc desc{};
  bool loaded = false;
  // plan
  int dtype = YM_DT_F16, task = 0, nc = 80, nm = 0, reg_max = 16, nl = 3;
  int strides[4] = {8, 16, 32, 0};
  int input_buf = -1, anchor_buf = -1, proto_buf = -1, no = 0;
  int kpt_K = 0, kpt_ndim = 0, kpt_off = 0;  // pose plans: keypoints, 2 | 3 values each, raw offset in the anchor row
  float* d_lowres = nullptr;  // Segment mask assembly scratch (ym_masks)
  char* d_misc = nullptr;     // 16 KB: ym_input_max statistics region, ym_broadcast_weights control words
  size_t lowres_bytes = 0;
  std::vector<BufDesc> bufs;
  std::vector<Op> ops;
  char* d_weights = nullptr;
  std::vector<char> blob_host;  // the loaded blob as received (what ym_broadcast_weights sends from the root)
  size_t off_wstem = 0;  // stem weights re-laid out as fp32 [27][N] behind the blob's weights (ym_stem.hip)
  size_t off_wtap0 = 0;            // int8 plans: the 3x3 convs' [9][N] int32 tap sums, behind the stem weights
  std::vector<size_t> off_wtap;    // per op: 1 + byte offset from off_wtap0 (0: none)
  // branch schedule of a one-lane forward (ops of independent DAG branches on up to kMaxLanes streams)
  int nbr = 1;
  std::vector<int> br_of;                // per op: branch stream
  std::vector<std::vector<int>> br_wait; // per op: earlier ops (other streams) whose events it waits for
  std::vector<char> br_rec;              // per op: record its event after it
  std::vector<hipEvent_t> op_ev;
  size_t wbytes = 0;
  // workspace for the current (B, H, W)
  int cB = 0, cH = 0, cW = 0;
  char* d_arena = nullptr;
  size_t arena_bytes = 0;
  std::vector<size_t> buf_off;
  size_t off_ctl = 0, off_slab = 0, off_cnt = 0, off_chain = 0, off_kpts = 0, slab_bytes = 0;
  int A = 0;
  // the NMS stage's scratch in the arena.  Multi-label mode (ym_infer_args.multi_label): its regions join at the first
  // workspace (re)build after a multi-label call was seen (check_call sets ml_want; nms.ml: they are there), so a
  // context that never validates pays nothing
  NmsScratch nms;
  bool ml_want = false;
  int lvl_W[4] = {0}, lvl_off[4] = {0};
  hipStream_t cap_stream = nullptr;
  // lanes: the batch is cut into image slices whose op chains are captured as parallel branches of one graph, so
  // the fixed per-launch latency of one slice's small kernels overlaps the other slices' work
  hipStream_t lane_streams[kMaxLanes] = {};
  hipEvent_t fork_ev = nullptr, join_ev[kMaxLanes] = {};
  std::vector<GraphEntry> graphs;
  // feature embeddings (ym_embed): the forward stops early (Launch::stop) and the pooling stage (csrc/ym_embed.hip)
  // reads embed_views into embed_out; d_embed holds the chunk partials of large maps
  std::vector<ym_embed_view> embed_views;
  float* embed_out = nullptr;
  long long embed_ld = 0;
  float* d_embed = nullptr;
  size_t embed_floats = 0;
  // annotated frames (ym_annotate): the records of the B x max_det detection slots, grown on demand
  AnnotRec* d_annot = nullptr;
  size_t annot_recs = 0;
  // instance polygons (ym_mask_contours): n CtSel records, then (planes too large for LDS only) n bit planes of
  // ym_ct_words(H, W) words; grown on demand
  char* d_contour = nullptr;
  size_t contour_bytes = 0;
  // test-time augmentation: ym_tta_forward launches the forward without its NMS stage; the merged candidate set and the
  // NMS scratch over it (ym_tta_nms) belong to the first pass's context and are rebuilt only when the shape changes
  struct TtaWs {
    int B = 0, H = 0, W = 0, nc = 0;
    char* d = nullptr;
    NmsScratch ws;  // over ws.A merged anchors; multi-label regions and class rows on demand (ws.ml)
  } tta;
  // the previous forward: every forward of a context uses the same arena, NMS scratch, split-K slabs /
  // counters and input_stats ticket, so a forward launched on another stream than the previous one first waits for
  // it (ym_infer: hipStreamWaitEvent); last_ev is the replayed graph's `done` event or fwd_ev (eager forwards)
  hipStream_t last_st = nullptr;
  hipEvent_t last_ev = nullptr, fwd_ev = nullptr;
  int order_after_last(hipStream_t st) {
    if (last_ev && last_st != st) {
      const hipError_t e = hipStreamWaitEvent(st, last_ev, 0);
      if (e != hipSuccess) return fail(YM_EHIP, "stream order: %s", hipGetErrorString(e));
    }
    return YM_OK;
  }
  int record_last(hipEvent_t ev, hipStream_t st) {
    HIPCK(hipEventRecord(ev, st));
    last_ev = ev;
    last_st = st;
    return YM_OK;
  }
  int mark_last(hipStream_t st) {  // behind an eager forward (or any other use of the shared scratch) on `st`
    if (!fwd_ev) HIPCK(hipEventCreateWithFlags(&fwd_ev, hipEventDisableTiming));
    return record_last(fwd_ev, st);
  }
  int launch_graph(GraphEntry& g, hipStream_t st) {
    HIPCK(hipGraphLaunch(g.exec, st));
    return record_last(g.done, st);
  }
  void retire(GraphEntry& g) {  // retire_graph, forgetting last_ev when it is that graph's event (now complete)
    if (g.done && g.done == last_ev) last_ev = nullptr;
    retire_graph(g);
  }
  std::vector<hipEvent_t> prof_events;
  // per-shape, per-op conv tile configuration (-1 = heuristic); set by ym_tune / ym_set_op_cfg
  struct ShapeCfg {
    int B, H, W;
    std::vector<int> cfg;
  };
  std::vector<ShapeCfg> cfgs;
  const std::vector<int>* find_cfg(int B, int H, int W) const {
    for (const auto& e : cfgs)
      if (e.B == B && e.H == H && e.W == W) return &e.cfg;
    return nullptr;
  }
  void put_cfg(int B, int H, int W, std::vector<int> v) {
    for (auto& e : cfgs)
      if (e.B == B && e.H == H && e.W == W) { e.cfg = std::move(v); return; }
    cfgs.push_back({B, H, W, std::move(v)});
  }
  void drop_cfg(int B, int H, int W) {
    for (size_t i = 0; i < cfgs.size(); ++i)
      if (cfgs[i].B == B && cfgs[i].H == H && cfgs[i].W == W) { cfgs.erase(cfgs.begin() + i); return; }
  }
  // tests (ym_get_op_cfg_taken): per op of the last forward launched, whether its pinned cfg was the kernel that ran
  // ([2i]: the op, or the first conv of a split pair; [2i + 1]: the pair's second conv; ym_launch_conv's `taken`)
  std::vector<int> taken;
  // tests (ym_get_op_variant): per op of that forward, the kernel instantiation a depthwise / SPPF / attention op
  // launched (the launchers' `variant`; -1: another kind, not launched, int8 / fp8)
  std::vector<int> variant;
  int tkB = 0, tkH = 0, tkW = 0;
  int op_cfg(long i, int B) const {  // for the current workspace height/width
    const std::vector<int>* v = find_cfg(B, cH, cW);
    return (v && i >= 0 && i < (long)v->size()) ? (*v)[i] : -1;
  }

  ~ym_ctx() {
    (void)hipSetDevice(device);
    clear_graphs();
    for (auto e : prof_events) (void)hipEventDestroy(e);
    if (d_arena) (void)hipFree(d_arena);
    if (d_weights) (void)hipFree(d_weights);
    if (d_lowres) (void)hipFree(d_lowres);
    if (d_misc) (void)hipFree(d_misc);
    if (tta.d) (void)hipFree(tta.d);
    if (d_embed) (void)hipFree(d_embed);
    if (d_annot) (void)hipFree(d_annot);
    if (d_contour) (void)hipFree(d_contour);
    if (cap_stream) (void)hipStreamDestroy(cap_stream);
    for (int l = 0; l < kMaxLanes; ++l) {
      if (lane_streams[l]) (void)hipStreamDestroy(lane_streams[l]);
      if (join_ev[l]) (void)hipEventDestroy(join_ev[l]);
    }
    if (fork_ev) (void)hipEventDestroy(fork_ev);
    if (fwd_ev) (void)hipEventDestroy(fwd_ev);
    for (hipEvent_t e : op_ev) (void)hipEventDestroy(e);
  }
  void clear_graphs() {
    for (auto& g : graphs) retire(g);
    graphs.clear();
  }
  int buf_P(int b) const {
    const BufDesc& d = bufs[b];
    if (d.f == 0) return A;
    return (cH / d.f) * (cW / d.f);
  }
  int buf_H(int b) const { return bufs[b].f == 0 ? 1 : cH / bufs[b].f; }
  int buf_Wd(int b) const { return bufs[b].f == 0 ? A : cW / bufs[b].f; }
  int elem(int b) const { return (bufs[b].f32 || ym_dt_f32s(dtype)) ? 4 : (ym_dt_q8(dtype) ? 1 : 2); }
  template <typename T> const T* wptr(int32_t off) const {  // a record's *_off slot: unsigned bytes into the weights
    return reinterpret_cast<const T*>(d_weights + (size_t)(uint32_t)off);
  }
  int* variant_of(const Op& op) { return variant.size() == ops.size() ? &variant[&op - ops.data()] : nullptr; }
  float* raw_of(const Launch& L, const Op& op) const { return L.calib_raw ? L.calib_raw[&op - ops.data()] : nullptr; }
  // buffer b from image img0 on: that slice of the whole-batch buffer (all buffers are image-major)
  void* bptr(int b, int img0) const { return d_arena + buf_off[b] + (size_t)img0 * buf_P(b) * bufs[b].C * elem(b); }
};

namespace {

size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Typed pointers into an NmsScratch at `base`, from image img0 on (absent regions: null)
struct NmsView {
  float4 *boxes, *sboxes;
  float *scores, *sareas, *rows;
  int *cls, *counts, *seln;
  unsigned long long *keys, *keys2, *sel, *sel2;
  unsigned char* sup;
  unsigned int* hist;
  MlState* state;
  int A, kstride;
};
NmsView nms_view(char* base, const NmsScratch& s, int img0) {
  NmsView v{};
  auto set = [&](auto*& p, const NmsRegion& r) {
    p = r.stride ? reinterpret_cast<std::remove_reference_t<decltype(p)>>(base + r.at(img0)) : nullptr;
  };
  set(v.boxes, s.boxes); set(v.scores, s.scores); set(v.cls, s.cls);
  set(v.keys, s.keys); set(v.keys2, s.keys2); set(v.counts, s.counts);
  set(v.sboxes, s.sboxes); set(v.sareas, s.sareas); set(v.sup, s.sup);
  set(v.rows, s.rows);
  set(v.sel, s.sel); set(v.sel2, s.sel2); set(v.hist, s.hist); set(v.state, s.state); set(v.seln, s.seln);
  v.A = s.A; v.kstride = s.kstride;
  return v;
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
int conv_args(ym_ctx* c, const Launch& L, const Op& op, int B, const float* d_in, float in_eps, ConvArgs& a,
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
void split_args(ym_ctx* c, const Launch& L, const Op& op, const ConvArgs& a, ConvArgs& A, ConvArgs& Bc) {
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
hipError_t launch_fused(ym_ctx* c, const Launch& L, const Op& op, const ConvArgs& a, int out_f32, int cfg,
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

// Where an NMS stage reads per-candidate rows: the nm extras the NMS kernel copies behind each kept box, and the
// class scores the multi-label candidate stage thresholds (both (B, A, *_ld) fp32; null: none)
struct NmsSource {
  const float* extras; int extras_ld, mask_off;
  const float* cls; int cls_ld, cls_off;
};

// The NMS stage over B images of the candidates in `v` (decode_anchors' or the TTA merge's): single-label, with the
// keys presorted at low conf, or multi-label.  The forward's OP_NMS and ym_tta_nms both end here.
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
    m.conf = args->conf; m.has_classes = args->has_classes;
    for (int i = 0; i < 4; ++i) m.classes[i] = args->classes[i];
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

int launch_op(ym_ctx* c, const Launch& L, const Op& op, int B, const float* d_in, const ym_infer_args* args,
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
      const NmsView v = nms_view(c->d_arena, c->nms, L.img0);
      DecodeArgs a{};
      a.anchors = reinterpret_cast<const float*>(c->bptr(c->anchor_buf, L.img0));
      a.no_tot = c->bufs[c->anchor_buf].C;
      a.boxes = v.boxes; a.scores = v.scores; a.cls = v.cls; a.keys = v.keys; a.counts = v.counts;
      a.A = v.A; a.kstride = v.kstride; a.nc = c->nc; a.reg_max = c->reg_max; a.B = B; a.nl = c->nl;
      for (int l = 0; l < c->nl; ++l) {
        a.lvl_W[l] = c->lvl_W[l]; a.lvl_off[l] = c->lvl_off[l]; a.lvl_stride[l] = (float)c->strides[l];
      }
      a.conf = args->conf;
      a.has_classes = args->has_classes;
      for (int i = 0; i < 4; ++i) a.classes[i] = args->classes[i];
      e = ym_launch_decode(a, st);
      break;
    }
    case OP_NMS: {
      if (L.skip_nms) break;
      const NmsView v = nms_view(c->d_arena, c->nms, L.img0);
      const float* rows = reinterpret_cast<const float*>(c->bptr(c->anchor_buf, L.img0));
      const int no_tot = c->bufs[c->anchor_buf].C;
      NmsSource src{rows, no_tot, c->no, rows, no_tot, 4 * c->reg_max};
      if (c->task == kTaskPose) {
        // Pose: decode the candidates' keypoints (behind decode_anchors, before any NMS kernel) into their own
        // (B, A, nm) rows and let NMS carry its nm extras from there; the raw head rows stay as the convs wrote them
        KptArgs k{};
        k.anchors = rows; k.no_tot = no_tot; k.kpt_off = c->kpt_off;
        k.keys = v.keys; k.counts = v.counts;
        k.out = reinterpret_cast<float*>(c->d_arena + c->off_kpts) + (size_t)L.img0 * c->A * c->nm;
        k.nk_pad = c->nm; k.A = v.A; k.kstride = v.kstride; k.K = c->kpt_K; k.ndim = c->kpt_ndim; k.B = B;
        k.nl = c->nl;
        for (int l = 0; l < c->nl; ++l) {
          k.lvl_W[l] = c->lvl_W[l]; k.lvl_off[l] = c->lvl_off[l]; k.lvl_stride[l] = (float)c->strides[l];
        }
        e = ym_launch_kpts(k, st);
        if (e != hipSuccess) break;
        src.extras = k.out; src.extras_ld = c->nm; src.mask_off = 0;
      }
      // counts_after_dets: this lane's images' words behind the WHOLE batch's rows (d_dets is the lane's)
      const size_t rows_left = (size_t)(L.B - L.img0) * args->max_det * (6 + c->nm);
      int* counts2 = args->counts_after_dets ? reinterpret_cast<int*>(d_dets + rows_left) + L.img0 : nullptr;
      e = launch_nms_stage(v, src, args, B, c->nc, c->nm, c->cH, c->cW, d_dets, d_counts, counts2, st);
      break;
    }
    default:
      return fail(YM_EBLOB, "unknown op kind %d", op.kind);
  }
  if (e != hipSuccess) return fail(YM_EHIP, "launch of op %s failed: %s", op.name, hipGetErrorString(e));
  return YM_OK;
}

// B images of H x W; `who`: the message's prefix ("" or "entry point: ")
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
  if (args->multi_label && nc > 1) {  // (nc == 1: the single-label path, as upstream's multi_label &= nc > 1)
    if (task != 0)
      return fail(YM_EINVAL, "multi_label: %s plans are not supported (validation mode is for detect plans)",
                  ym_task_name(task));
    if (nc > 128) return fail(YM_EINVAL, "multi_label: nc %d > 128 is not supported", nc);
    if (args->max_nms > kMlCap) return fail(YM_EINVAL, "multi_label: max_nms %d > %d is not supported", args->max_nms, kMlCap);
  }
  return YM_OK;
}

int check_call(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
               int* d_counts) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!c->loaded) return fail(YM_ESTATE, "ym_infer before ym_load_weights");
  if (!d_in || !d_dets || !d_counts || !args) return fail(YM_EINVAL, "null pointer argument");
  if (int rc = check_shape(B, H, W, "")) return rc;
  if (int rc = check_nms_args(args, c->nc, c->task)) return rc;
  if (args->multi_label && c->nc > 1) c->ml_want = true;
  return YM_OK;
}

// `reps` calls of launch(stream) captured on the private stream as one graph, replayed on `st`: once warm, then
// `timed` times between two events (device-bound even for tiny kernels).  Returns a HIP failure as YM_EHIP; else
// launch_rc is the first non-zero result of `launch` (nothing was replayed) or 0 with the timed replays' total in ms.
// Graph, exec and events are destroyed on every path.
template <typename F>
int time_captured(ym_ctx* c, hipStream_t st, int reps, int timed, F&& launch, int& launch_rc, float& ms) {
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

}  // namespace

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
  a.part = c->d_embed;
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
  if (need < 0 || (size_t)need > c->embed_floats) return fail(YM_EINVAL, "ym_embed: bad view table");
  const hipError_t e = ym_launch_embed(a, st);
  if (e != hipSuccess) return fail(YM_EHIP, "embed pooling launch: %s", hipGetErrorString(e));
  return YM_OK;
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

// Behind check_call, for every entry point that launches ops: device, workspace, stream order; L: one whole-batch launch
static int begin_launch(ym_ctx* c, int B, int H, int W, hipStream_t st, Launch& L) {
  HIPCK(hipSetDevice(c->device));
  if (int rc = ensure_workspace(c, B, H, W)) return rc;
  L = Launch{};
  L.B = B;
  return c->order_after_last(st);
}

// ym_infer, (skip_nms) ym_tta_forward and (stop >= 0) ym_embed
static int infer_impl(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, float* d_dets,
                      int* d_counts, void* stream, bool skip_nms, int stop) {
  int rc = check_call(c, d_in, B, H, W, args, d_dets, d_counts);
  if (rc) return rc;
  hipStream_t st = static_cast<hipStream_t>(stream);
  Launch L;
  if ((rc = begin_launch(c, B, H, W, st, L))) return rc;
  L.skip_nms = skip_nms; L.stop = stop;
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
  return infer_impl(c, d_in, B, H, W, args, d_dets, d_counts, stream, false, -1);
}

// ---------------------------------------------------------------------------------- test-time augmentation
int ym_tta_shape(int H, int W, int pass, int* Hs, int* Ws, int* hc, int* wc) {
  if (int rc = check_shape(1, H, W, "ym_tta_shape: ")) return rc;
  if (pass < 0 || pass >= kTtaPasses) return fail(YM_EINVAL, "ym_tta_shape: pass is 0..%d", kTtaPasses - 1);
  int v[4];
  ym_tta_pass_shape(H, W, pass, v[0], v[1], v[2], v[3]);
  if (Hs) *Hs = v[0];
  if (Ws) *Ws = v[1];
  if (hc) *hc = v[2];
  if (wc) *wc = v[3];
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
  const hipError_t e = ym_launch_tta_scale(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(YM_EHIP, "tta scale launch: %s", hipGetErrorString(e));
  return YM_OK;
}

int ym_tta_forward(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, void* stream) {
  if (!c || !args) return fail(YM_EINVAL, "null argument");
  if (c->loaded && c->task != 0)
    return fail(YM_EINVAL, "test-time augmentation: %s plans are not supported (detect plans only)", ym_task_name(c->task));
  ym_infer_args fa = *args;  // one capture serves the single- and the multi-label NMS that follows
  fa.multi_label = 0;
  fa.counts_after_dets = 0;
  // (the NMS stage is the only reader of the outputs: any device words do, they are never written)
  float* nodets = reinterpret_cast<float*>(c->d_misc + kMiscNoDets);
  return infer_impl(c, d_in, B, H, W, &fa, nodets, reinterpret_cast<int*>(nodets), stream, true, -1);
}

// ---------------------------------------------------------------------------------- feature embeddings
int ym_embed(ym_ctx* c, const float* d_in, int B, int H, int W, const ym_infer_args* args, const ym_embed_view* views,
             int n_views, float* d_out, long long out_stride, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!c->loaded) return fail(YM_ESTATE, "ym_embed before ym_load_weights");
  if (!d_in || !args || !views || !d_out) return fail(YM_EINVAL, "null pointer argument");
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
  if ((size_t)need > c->embed_floats) {  // the chunk partials grow: no captured pooling stage may keep the old ones
    c->clear_graphs();
    if (c->d_embed) {
      HIPCK(hipDeviceSynchronize());
      HIPCK(hipFree(c->d_embed));
      c->d_embed = nullptr;
      c->embed_floats = 0;
    }
    const hipError_t e = hipMalloc(&c->d_embed, (size_t)need * sizeof(float));
    if (e != hipSuccess) {
      c->d_embed = nullptr;
      return fail(YM_ENOMEM, "embed partials hipMalloc(%ld floats): %s", need, hipGetErrorString(e));
    }
    c->embed_floats = (size_t)need;
  }
  // what reaches the truncated forward: the /255 rule's inputs and the launch mode; one lane; no output is written
  ym_infer_args fa{};
  fa.conf = 0.25f; fa.max_wh = 7680.f; fa.iou = 0.7; fa.max_det = 300; fa.max_nms = 30000;
  fa.in_eps = args->in_eps; fa.use_graph = args->use_graph; fa.lanes = 1; fa.d_batch_max = args->d_batch_max;
  float* nodets = reinterpret_cast<float*>(c->d_misc + kMiscNoDets);
  return infer_impl(c, d_in, B, H, W, &fa, nodets, reinterpret_cast<int*>(nodets), stream, false, stop);
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
  m.conf = args->conf; m.has_classes = args->has_classes;
  for (int i = 0; i < 4; ++i) m.classes[i] = args->classes[i];
  m.img_w = (float)W;
  if (!ml) HIPCK(hipMemsetAsync(m.counts, 0, (size_t)B * 4, st));
  hipError_t e = ym_launch_tta_merge(m, st);
  if (e != hipSuccess) return fail(YM_EHIP, "tta merge launch: %s", hipGetErrorString(e));
  // no extras (detect plans: nm = 0); multi-label thresholds the merged class rows
  const NmsSource src{nullptr, 0, 0, m.rows, c->nc, 0};
  int* counts2 = args->counts_after_dets ? reinterpret_cast<int*>(d_dets + (size_t)B * args->max_det * 6) : nullptr;
  e = launch_nms_stage(v, src, args, B, c->nc, 0, H, W, d_dets, d_counts, counts2, st);
  if (e != hipSuccess) return fail(YM_EHIP, "tta NMS launch: %s", hipGetErrorString(e));
  // the merge read every pass's arena: a later forward of any of them on another stream waits for this call
  for (int p = 0; p < kTtaPasses; ++p)
    if (int rc = ctxs[p]->mark_last(st)) return rc;
  return YM_OK;
}

int ym_tta_counts(ym_ctx* c, int* dst, int B) {
  if (!c || !dst || B < 1) return fail(YM_EINVAL, "bad ym_tta_counts arguments");
  if (!c->tta.d || B > c->tta.B) return fail(YM_ESTATE, "no merged scratch for %d images yet (run ym_tta_nms first)", B);
  HIPCK(hipSetDevice(c->device));
  HIPCK(hipDeviceSynchronize());
  HIPCK(hipMemcpy(dst, c->tta.d + c->tta.ws.counts.off, (size_t)B * 4, hipMemcpyDefault));
  return YM_OK;
}

int ym_input_max(ym_ctx* c, const float* d_in, size_t n, float* d_max, void* stream) {
  if (!c || !d_in || !d_max || n == 0) return fail(YM_EINVAL, "bad ym_input_max arguments");
  HIPCK(hipSetDevice(c->device));
  const hipError_t e = ym_launch_input_max(d_in, (long)n, reinterpret_cast<float*>(c->d_misc + kMiscStats), d_max,
                                           static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(YM_EHIP, "input max: %s", hipGetErrorString(e));
  return YM_OK;
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
    if (k != OP_CONV && k != OP_DW && k != OP_SPPF && k != OP_ATTN) continue;
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
  HIPCK(hipSetDevice(c->device));
  HIPCK(hipDeviceSynchronize());
  HIPCK(hipMemcpy(dst, c->bptr(b, 0), bytes, hipMemcpyDefault));
  return YM_OK;
}

int ym_kpt_shape(ym_ctx* c, int* K, int* ndim) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!c->loaded) return fail(YM_ESTATE, "ym_kpt_shape before ym_load_weights");
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
    default: return fail(YM_EINVAL, "unknown scratch region %d", which);
  }
  if (bytes > cap) return fail(YM_EINVAL, "read of %zu bytes exceeds region size %zu", bytes, cap);
  HIPCK(hipSetDevice(c->device));
  HIPCK(hipDeviceSynchronize());
  HIPCK(hipMemcpy(dst, c->d_arena + off, bytes, hipMemcpyDefault));
  return YM_OK;
}

int ym_letterbox(ym_ctx* c, const void* d_src, int h, int w, int row_bytes, int bgr, int uh, int uw, int top,
                 int left, float* d_dst, int Hn, int Wn, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_src || !d_dst || h < 1 || w < 1 || uh < 1 || uw < 1 || top < 0 || left < 0 || top + uh > Hn ||
      left + uw > Wn || row_bytes < 3 * w)
    return fail(YM_EINVAL, "bad ym_letterbox geometry (%dx%d -> %dx%d at (%d, %d) in %dx%d)", h, w, uh, uw, top, left,
                Hn, Wn);
  HIPCK(hipSetDevice(c->device));
  LetterboxArgs a{};
  a.src = static_cast<const unsigned char*>(d_src);
  a.h = h; a.w = w; a.row_bytes = row_bytes; a.bgr = bgr ? 1 : 0;
  a.uh = uh; a.uw = uw; a.top = top; a.left = left;
  a.scale_x = 1.0 / ((double)uw / w);  // cv2: scale_x = 1. / inv_scale_x, inv_scale_x = (double)dsize.width / ssize.width
  a.scale_y = 1.0 / ((double)uh / h);
  a.dst = d_dst; a.Hn = Hn; a.Wn = Wn;
  hipError_t e = ym_launch_letterbox(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(YM_EHIP, "letterbox launch: %s", hipGetErrorString(e));
  return YM_OK;
}

static int launch_masks(ym_ctx* c, MaskArgs& a, int B, int H, int W, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (c->task != 1 || c->proto_buf < 0) return fail(YM_ESTATE, "ym_masks needs a segment plan");
  if (!c->d_arena || B > c->cB || H != c->cH || W != c->cW)
    return fail(YM_ESTATE, "ym_masks must follow ym_infer of the same (B, H, W) (workspace %dx%dx%d)", c->cB, c->cH,
                c->cW);
  HIPCK(hipSetDevice(c->device));
  a.proto = reinterpret_cast<const float*>(c->bptr(c->proto_buf, 0));
  a.MH = c->buf_H(c->proto_buf); a.MW = c->buf_Wd(c->proto_buf); a.nm = c->nm;
  a.no = 6 + c->nm; a.B = B; a.H = H; a.W = W;
  if (a.total == 0) return YM_OK;
  if (!ym_masks_fused(a)) {  // the two-kernel path: (total, MH, MW) prototype-resolution scratch
    const size_t need = (size_t)a.total * a.MH * a.MW * sizeof(float);
    if (need > c->lowres_bytes) {
      if (c->d_lowres) HIPCK(hipFree(c->d_lowres));
      c->d_lowres = nullptr;
      hipError_t e = hipMalloc(&c->d_lowres, need);
      if (e != hipSuccess) return fail(YM_ENOMEM, "mask scratch hipMalloc(%zu): %s", need, hipGetErrorString(e));
      c->lowres_bytes = need;
    }
    a.lowres = c->d_lowres;
  }
  const hipError_t e = ym_launch_masks(a, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(YM_EHIP, "mask kernels: %s", hipGetErrorString(e));
  return YM_OK;
}

int ym_masks(ym_ctx* c, const float* d_dets, int B, int max_det, const int* d_offsets, int total, int H, int W,
             unsigned char* d_masks, int* d_nonempty, void* stream) {
  if (total < 0 || max_det < 1 || (total > 0 && (!d_dets || !d_offsets || !d_masks || !d_nonempty)))
    return fail(YM_EINVAL, "bad ym_masks arguments");
  MaskArgs a{};
  a.dets = d_dets; a.max_det = max_det; a.offsets = d_offsets; a.total = total;
  a.masks = d_masks; a.nonempty = d_nonempty;
  return launch_masks(c, a, B, H, W, stream);
}

int ym_masks_slots(ym_ctx* c, const float* d_dets, int B, int max_det, const int* d_counts, int cap, int H, int W,
                   unsigned char* d_masks, int* d_flags, void* stream) {
  if (B < 1 || cap < 1 || max_det < 1 || cap > max_det || !d_dets || !d_counts || !d_masks || !d_flags)
    return fail(YM_EINVAL, "bad ym_masks_slots arguments");
  MaskArgs a{};
  a.dets = d_dets; a.max_det = max_det; a.counts = d_counts; a.cap = cap; a.total = B * cap;
  a.masks = d_masks; a.nonempty = d_flags;
  return launch_masks(c, a, B, H, W, stream);
}

int ym_masks_native(ym_ctx* c, const float* d_dets, int det_stride, int B, int max_det, const int* d_offsets, int total,
                    int H, int W, const int* shapes, const int* d_shapes, const long long* d_mask_offsets,
                    unsigned char* d_masks, int* d_nonempty, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (B < 1 || total < 0 || max_det < 1 || !shapes || !d_dets || !d_offsets || !d_shapes || !d_mask_offsets ||
      (total > 0 && (!d_masks || !d_nonempty)))
    return fail(YM_EINVAL, "bad ym_masks_native arguments");
  long long max_bytes = 0;
  for (int b = 0; b < B; ++b) {
    const long long h0 = shapes[2 * b], w0 = shapes[2 * b + 1];
    if (h0 < 1 || w0 < 1 || h0 * w0 > (1ll << 30))
      return fail(YM_EINVAL, "ym_masks_native: native size %lld x %lld of image %d (1 x 1 .. 2^30 pixels)", h0, w0, b);
    max_bytes = std::max(max_bytes, h0 * w0);
  }
  if (c->task != 1 || c->proto_buf < 0) return fail(YM_ESTATE, "ym_masks_native needs a segment plan");
  if (det_stride < 6 + c->nm) return fail(YM_EINVAL, "ym_masks_native: row stride %d below %d", det_stride, 6 + c->nm);
  if (!c->d_arena || B > c->cB || H != c->cH || W != c->cW)
    return fail(YM_ESTATE, "ym_masks_native must follow ym_infer of the same (B, H, W) (workspace %dx%dx%d)", c->cB,
                c->cH, c->cW);
  if (total == 0) return YM_OK;
  HIPCK(hipSetDevice(c->device));
  MaskNativeArgs a{};
  a.proto = reinterpret_cast<const float*>(c->bptr(c->proto_buf, 0));
  a.MH = c->buf_H(c->proto_buf); a.MW = c->buf_Wd(c->proto_buf); a.nm = c->nm;
  a.dets = d_dets; a.max_det = max_det; a.stride = det_stride;
  a.offsets = d_offsets; a.B = B; a.total = total;
  a.shapes = d_shapes; a.byte_off = d_mask_offsets; a.masks = d_masks; a.nonempty = d_nonempty;
  const hipError_t e = ym_launch_masks_native(a, max_bytes, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(YM_EHIP, "native mask kernel: %s", hipGetErrorString(e));
  return YM_OK;
}

// ---------------------------------------------------------------------------------------------- RCCL (xGMI)
// The init-time weight broadcast of the batch-sharded multi-GPU path: RCCL is resolved at run time
// (dlopen of the process's already-loaded librccl — torch's, when the host is Python — else the ROCm one), so
// libyolomi.so itself has no link-time dependency on it.  Only the four entry points below are used.
namespace {
struct Rccl {
  typedef int (*GetUniqueId)(void*);
  typedef int (*CommInitRank)(void**, int, ym_rccl_id, int);
  typedef int (*CommDestroy)(void*);
  typedef int (*CommUserRank)(void*, int*);
  typedef int (*CommCount)(void*, int*);
  typedef int (*Broadcast)(const void*, void*, size_t, int, int, void*, hipStream_t);
  typedef int (*AllReduce)(const void*, void*, size_t, int, int, void*, hipStream_t);
  typedef const char* (*ErrStr)(int);
  GetUniqueId get_id = nullptr;
  CommInitRank init = nullptr;
  CommDestroy destroy = nullptr;
  CommUserRank user_rank = nullptr;
  CommCount count = nullptr;
  Broadcast bcast = nullptr;
  AllReduce allreduce = nullptr;
  ErrStr err = nullptr;
  bool ok = false;
};

const Rccl* rccl() {
  static Rccl r = [] {
    Rccl x;
    void* h = nullptr;
    for (const char* n : {"librccl.so.1", "librccl.so"})
      if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
    for (const char* n : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"})
      if (!h) h = dlopen(n, RTLD_NOW | RTLD_LOCAL);
    if (!h) return x;
    x.get_id = (Rccl::GetUniqueId)dlsym(h, "ncclGetUniqueId");
    x.init = (Rccl::CommInitRank)dlsym(h, "ncclCommInitRank");
    x.destroy = (Rccl::CommDestroy)dlsym(h, "ncclCommDestroy");
    x.user_rank = (Rccl::CommUserRank)dlsym(h, "ncclCommUserRank");
    x.count = (Rccl::CommCount)dlsym(h, "ncclCommCount");
    x.bcast = (Rccl::Broadcast)dlsym(h, "ncclBroadcast");
    x.allreduce = (Rccl::AllReduce)dlsym(h, "ncclAllReduce");
    x.err = (Rccl::ErrStr)dlsym(h, "ncclGetErrorString");
    x.ok = x.get_id && x.init && x.destroy && x.user_rank && x.count && x.bcast && x.allreduce && x.err;
    return x;
  }();
  return r.ok ? &r : nullptr;
}

#define RCCLCK(x)                                                                                       \
  do {                                                                                                  \
    const int r_ = (x);                                                                                 \
    if (r_ != 0) return fail(YM_EHIP, "%s: RCCL error %d (%s)", #x, r_, R->err ? R->err(r_) : "?");     \
  } while (0)
constexpr int kNcclUint8 = 1, kNcclUint64 = 5;  // ncclDataType_t
constexpr int kNcclSum = 0;                       // ncclRedOp_t
constexpr size_t kBcastChunk = 16u << 20;         // blob bytes per broadcast (one staging buffer per rank)
}  // namespace

int ym_rccl_get_unique_id(ym_rccl_id* id) {
  if (!id) return fail(YM_EINVAL, "null id");
  const Rccl* R = rccl();
  if (!R) return fail(YM_ESTATE, "RCCL (librccl.so) is not available in this process");
  RCCLCK(R->get_id(id));
  return YM_OK;
}

int ym_rccl_comm_init(int device, int nranks, const ym_rccl_id* id, int rank, void** comm) {
  if (!id || !comm || nranks < 1 || rank < 0 || rank >= nranks) return fail(YM_EINVAL, "bad ym_rccl_comm_init arguments");
  const Rccl* R = rccl();
  if (!R) return fail(YM_ESTATE, "RCCL (librccl.so) is not available in this process");
  HIPCK(hipSetDevice(device));
  *comm = nullptr;
  RCCLCK(R->init(comm, nranks, *id, rank));
  return YM_OK;
}

int ym_rccl_comm_destroy(void* comm) {
  if (!comm) return YM_OK;
  const Rccl* R = rccl();
  if (!R) return fail(YM_ESTATE, "RCCL (librccl.so) is not available in this process");
  RCCLCK(R->destroy(comm));
  return YM_OK;
}

// ---- the init-time weight broadcast: one rank's side, shared by the two transports
// (ym_broadcast_weights: RCCL, one rank per process; ym_broadcast_weights_local: every rank's context in this process,
// the fake backend of SURVEY §4.4) — staging buffer, the root's upload, a receiver's copy-out and load, and the
// verdict every rank agrees on.  The transports only move the chunk between staging buffers and sum control words.
struct BcastRank {
  ym_ctx* c = nullptr;
  int rank = -1;
  bool hip_ok = true, copy_ok = true;
  char* d = nullptr;  // kBcastChunk staging bytes on the context's device
  std::vector<char> h;  // a receiver's copy of the blob
  int rc = YM_OK;
  BcastRank() = default;
  BcastRank(const BcastRank&) = delete;
  BcastRank& operator=(const BcastRank&) = delete;
  ~BcastRank() {
    if (d) (void)hipFree(d);
  }
  // step (1): this rank's contribution to {the root's blob size (0: the root has no weights), staging failures}
  void open(int root, unsigned long long h1[2]) {
    hip_ok = hipSetDevice(c->device) == hipSuccess;
    const bool alloc_ok = hip_ok && hipMalloc(&d, kBcastChunk) == hipSuccess;
    if (!alloc_ok) d = nullptr;
    h1[0] += (rank == root && c->loaded) ? (unsigned long long)c->blob_host.size() : 0ull;
    h1[1] += alloc_ok ? 0ull : 1ull;
    copy_ok = hip_ok;
  }
  // step (2), per chunk: the root uploads it into its staging buffer before the transport moves it ...
  void put(int root, unsigned long long off, size_t len, hipStream_t st) {
    if (rank == root)
      copy_ok = copy_ok && hipMemcpyAsync(d, c->blob_host.data() + off, len, hipMemcpyHostToDevice, st) == hipSuccess;
  }
  // ... and a receiver copies it out after (the staging buffer is reused by the next chunk)
  void get(int root, unsigned long long off, size_t len, hipStream_t st) {
    if (rank != root)
      copy_ok = copy_ok && hipMemcpyAsync(h.data() + off, d, len, hipMemcpyDeviceToHost, st) == hipSuccess;
    copy_ok = copy_ok && hipStreamSynchronize(st) == hipSuccess;
  }
  // step (3): a receiver loads what it got; returns this rank's failure count for the verdict all-reduce
  unsigned long long load(int root, unsigned long long nbytes) {
    rc = copy_ok ? YM_OK : fail(YM_EHIP, "blob staging copy failed");
    if (rc == YM_OK && rank != root) rc = ym_load_weights(c, h.data(), nbytes);
    return rc == YM_OK ? 0ull : 1ull;
  }
};

// The identical-on-every-rank verdict on step (1)'s sums: YM_OK or the error every rank returns before step (2).
static int bcast_check(const unsigned long long h1[2], bool is_root, int root) {
  if (h1[0] == 0)
    return fail(YM_ESTATE, is_root ? "the root context has no weights to broadcast"
                                   : "the root rank %d has no weights to broadcast", root);
  if (h1[0] < sizeof(PlanHeader) || h1[0] > (1ull << 34)) return fail(YM_EBLOB, "broadcast blob size %llu", h1[0]);
  if (h1[1]) return fail(YM_ENOMEM, "%llu rank(s) could not allocate the %zu-byte staging buffer", h1[1], kBcastChunk);
  return YM_OK;
}

// The root rank's loaded blob (plan + weights, exactly the bytes its ym_load_weights received) goes to every rank
// of `comm` over RCCL (xGMI) and each non-root rank loads it into `c` (ym_load_weights), so every rank ends with an
// identical model without touching the file system.  Synchronous.
// Every rank issues the same sequence of collectives whatever fails locally, so no rank is left waiting inside RCCL
// for one that returned early: (1) an all-reduce (sum) of {root's blob size (0: the root has no weights), ranks
// whose staging buffer failed to allocate}; only if both are valid, (2) the blob broadcast in kBcastChunk pieces
// and (3) an all-reduce of the per-rank copy / load failures, so every rank returns the same verdict.  Errors in the
// arguments themselves (null pointers, root out of range) are identical on every rank and return before any
// collective; an RCCL error is communicator-wide.
int ym_broadcast_weights(ym_ctx* c, void* comm, int root, void* stream) {
  if (!c || !comm) return fail(YM_EINVAL, "null argument");
  const Rccl* R = rccl();
  if (!R) return fail(YM_ESTATE, "RCCL (librccl.so) is not available in this process");
  int rank = -1, n = 0;
  RCCLCK(R->user_rank(comm, &rank));
  RCCLCK(R->count(comm, &n));
  if (root < 0 || root >= n) return fail(YM_EINVAL, "root %d out of range (%d ranks)", root, n);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  BcastRank me;
  me.c = c;
  me.rank = rank;
  // control words in the context's scratch (allocated by ym_create, so nothing can fail before step 1)
  unsigned long long* dctl = reinterpret_cast<unsigned long long*>(c->d_misc + kMiscBcast);
  auto allreduce_sum = [&](unsigned long long* h, int cnt) -> int {
    me.hip_ok = me.hip_ok && hipMemcpyAsync(dctl, h, 8 * cnt, hipMemcpyHostToDevice, st) == hipSuccess;
    const int r = R->allreduce(dctl, dctl, cnt, kNcclUint64, kNcclSum, comm, st);
    if (r) return r;
    me.hip_ok = me.hip_ok && hipMemcpyAsync(h, dctl, 8 * cnt, hipMemcpyDeviceToHost, st) == hipSuccess &&
                hipStreamSynchronize(st) == hipSuccess;
    return 0;
  };
  unsigned long long h1[2] = {0ull, 0ull};
  me.open(root, h1);
  int r = allreduce_sum(h1, 2);  // (1)
  if (r) return fail(YM_EHIP, "ncclAllReduce(size): %s", R->err(r));
  if (int e = bcast_check(h1, rank == root, root)) return e;
  const unsigned long long nbytes = h1[0];
  if (rank != root) me.h.resize(nbytes);
  for (unsigned long long off = 0; off < nbytes; off += kBcastChunk) {  // (2)
    const size_t len = (size_t)std::min<unsigned long long>(kBcastChunk, nbytes - off);
    me.put(root, off, len, st);
    r = R->bcast(me.d, me.d, len, kNcclUint8, root, comm, st);
    if (r) return fail(YM_EHIP, "ncclBroadcast(blob): %s", R->err(r));
    me.get(root, off, len, st);
  }
  unsigned long long h3[1] = {me.load(root, nbytes)};  // (3)
  r = allreduce_sum(h3, 1);
  if (r) return fail(YM_EHIP, "ncclAllReduce(status): %s", R->err(r));
  if (me.rc != YM_OK) return me.rc;
  if (h3[0]) return fail(YM_EBLOB, "the weight broadcast failed on %llu other rank(s)", h3[0]);
  return YM_OK;
}

// The fake backend of the same broadcast (N ranks as N contexts of this process, e.g. on one GPU):
// rank i is ctxs[i]; the all-reduces are host sums and the chunk moves from the root's staging buffer to every
// other rank's by a device-to-device copy on `stream`, between the same BcastRank put / get / load steps the RCCL
// transport runs.  Returns the status of the first failing rank (every rank's context is left loaded or not as in
// the RCCL path); on success every context holds the root's blob.
int ym_broadcast_weights_local(ym_ctx* const* ctxs, int n, int root, void* stream) {
  if (!ctxs || n < 1) return fail(YM_EINVAL, "null / empty context list");
  if (root < 0 || root >= n) return fail(YM_EINVAL, "root %d out of range (%d ranks)", root, n);
  for (int i = 0; i < n; ++i)
    if (!ctxs[i]) return fail(YM_EINVAL, "null context for rank %d", i);
  const hipStream_t st = static_cast<hipStream_t>(stream);
  std::vector<BcastRank> ranks(n);
  unsigned long long h1[2] = {0ull, 0ull};
  for (int i = 0; i < n; ++i) {  // (1)
    ranks[i].c = ctxs[i];
    ranks[i].rank = i;
    ranks[i].open(root, h1);
  }
  if (int e = bcast_check(h1, true, root)) return e;
  const unsigned long long nbytes = h1[0];
  for (int i = 0; i < n; ++i)
    if (i != root) ranks[i].h.resize(nbytes);
  for (unsigned long long off = 0; off < nbytes; off += kBcastChunk) {  // (2)
    const size_t len = (size_t)std::min<unsigned long long>(kBcastChunk, nbytes - off);
    ranks[root].put(root, off, len, st);
    for (int i = 0; i < n; ++i)
      if (i != root)
        ranks[i].copy_ok = ranks[i].copy_ok && ranks[root].copy_ok &&
                           hipMemcpyAsync(ranks[i].d, ranks[root].d, len, hipMemcpyDeviceToDevice, st) == hipSuccess;
    for (int i = 0; i < n; ++i) ranks[i].get(root, off, len, st);
  }
  unsigned long long h3 = 0;  // (3)
  for (int i = 0; i < n; ++i) h3 += ranks[i].load(root, nbytes);
  for (int i = 0; i < n; ++i)
    if (ranks[i].rc != YM_OK) return ranks[i].rc;
  return h3 ? fail(YM_EBLOB, "the weight broadcast failed on %llu rank(s)", h3) : YM_OK;
}

// ---------------------------------------------------------------------------------------------- tracking
// ByteTrack state of `streams` video streams in device memory; ym_track_update is one launch of csrc/ym_track.hip.
static_assert(YM_TRACK_CAPACITY == kTrackCap && YM_TRACK_MAX_DET == kTrackMaxDet && YM_TRACK_MAX_STRIDE == kTrackMaxStride &&
                  YM_TRACK_STATE_WORDS <= (int)(sizeof(TrackHead) / sizeof(int)), "yolomi.h states ym_track.h's limits");
struct ym_tracker {
  int device = 0, streams = 0, cap = 0;
  ym_track_cfg cfg{};
  TrackSlot* d_slots = nullptr;
  TrackHead* d_heads = nullptr;
  ~ym_tracker() {
    if (d_slots || d_heads) (void)hipSetDevice(device);
    if (d_slots) (void)hipFree(d_slots);
    if (d_heads) (void)hipFree(d_heads);
  }
};

int ym_track_create(ym_ctx* c, int streams, const ym_track_cfg* cfg, ym_tracker** out) {
  if (!c || !cfg || !out) return fail(YM_EINVAL, "ym_track_create: null context, cfg or out");
  if (streams < 1 || streams > YM_TRACK_MAX_STREAMS)
    return fail(YM_EINVAL, "ym_track_create: %d streams (1..%d)", streams, YM_TRACK_MAX_STREAMS);
  const double th[4] = {cfg->track_high_thresh, cfg->track_low_thresh, cfg->new_track_thresh, cfg->match_thresh};
  for (double t : th)
    if (!(t >= 0.0 && t <= 1.0)) return fail(YM_EINVAL, "ym_track_create: threshold %g outside [0, 1]", t);
  if (cfg->track_buffer < 0 || cfg->capacity < 0 || cfg->capacity > YM_TRACK_CAPACITY)
    return fail(YM_EINVAL, "ym_track_create: track_buffer %d (>= 0), capacity %d (0..%d)", cfg->track_buffer,
                cfg->capacity, YM_TRACK_CAPACITY);
  HIPCK(hipSetDevice(c->device));
  ym_tracker* t = new ym_tracker();
  t->device = c->device;
  t->streams = streams;
  t->cap = cfg->capacity ? cfg->capacity : YM_TRACK_CAPACITY;
  t->cfg = *cfg;
  const size_t sb = (size_t)streams * t->cap * sizeof(TrackSlot), hb = (size_t)streams * sizeof(TrackHead);
  hipError_t e = hipMalloc(reinterpret_cast<void**>(&t->d_slots), sb);
  if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&t->d_heads), hb);
  if (e == hipSuccess) e = hipMemset(t->d_slots, 0, sb);
  if (e == hipSuccess) e = hipMemset(t->d_heads, 0, hb);
  if (e == hipSuccess) e = hipDeviceSynchronize();  // the first update may come on a non-blocking stream
  if (e != hipSuccess) {
    delete t;
    return fail(e == hipErrorOutOfMemory ? YM_ENOMEM : YM_EHIP, "ym_track_create: %s", hipGetErrorString(e));
  }
  *out = t;
  return YM_OK;
}

void ym_track_destroy(ym_tracker* t) { delete t; }

int ym_track_reset(ym_tracker* t, void* stream) {
  if (!t) return fail(YM_EINVAL, "null tracker");
  HIPCK(hipSetDevice(t->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  HIPCK(hipMemsetAsync(t->d_slots, 0, (size_t)t->streams * t->cap * sizeof(TrackSlot), st));
  HIPCK(hipMemsetAsync(t->d_heads, 0, (size_t)t->streams * sizeof(TrackHead), st));
  return YM_OK;
}

int ym_track_update(ym_tracker* t, const float* d_dets, int det_stride, int B, int max_det, const int* d_counts,
                    float* d_tracks, int* d_idx, int* d_track_counts, void* stream) {
  if (!t) return fail(YM_EINVAL, "null tracker");
  if (!d_dets || !d_counts || !d_tracks || !d_idx || !d_track_counts)
    return fail(YM_EINVAL, "ym_track_update: null pointer");
  if (B != t->streams) return fail(YM_EINVAL, "ym_track_update: batch %d, but the tracker holds %d streams", B, t->streams);
  if (max_det < 1 || max_det > YM_TRACK_MAX_DET)
    return fail(YM_EINVAL, "ym_track_update: max_det %d (1..%d)", max_det, YM_TRACK_MAX_DET);
  if (det_stride < 6 || det_stride > YM_TRACK_MAX_STRIDE)
    return fail(YM_EINVAL, "ym_track_update: row stride %d (6..%d)", det_stride, YM_TRACK_MAX_STRIDE);
  HIPCK(hipSetDevice(t->device));
  TrackArgs a{};
  a.slots = t->d_slots; a.heads = t->d_heads; a.cap = t->cap;
  a.dets = d_dets; a.det_stride = det_stride; a.max_det = max_det; a.counts = d_counts;
  a.tracks = d_tracks; a.idx = d_idx; a.track_counts = d_track_counts;
  a.high = (float)t->cfg.track_high_thresh; a.low = (float)t->cfg.track_low_thresh;
  a.new_thresh = (float)t->cfg.new_track_thresh; a.match = t->cfg.match_thresh;
  a.max_time_lost = t->cfg.track_buffer; a.fuse = t->cfg.fuse_score ? 1 : 0;
  const hipError_t e = ym_launch_track(a, B, static_cast<hipStream_t>(stream));
  if (e != hipSuccess) return fail(YM_EHIP, "track kernel: %s", hipGetErrorString(e));
  return YM_OK;
}

int ym_track_read_state(ym_tracker* t, int* state, int n_streams) {
  if (!t || !state) return fail(YM_EINVAL, "null tracker or state");
  if (n_streams < 1 || n_streams > t->streams)
    return fail(YM_EINVAL, "ym_track_read_state: %d streams of %d", n_streams, t->streams);
  HIPCK(hipSetDevice(t->device));
  HIPCK(hipDeviceSynchronize());
  std::vector<TrackHead> h(n_streams);
  HIPCK(hipMemcpy(h.data(), t->d_heads, (size_t)n_streams * sizeof(TrackHead), hipMemcpyDeviceToHost));
  for (int b = 0; b < n_streams; ++b) {
    int* o = state + (size_t)b * YM_TRACK_STATE_WORDS;
    o[0] = h[b].frame_id; o[1] = h[b].issued + 1; o[2] = h[b].n_tracked;
    o[3] = h[b].n_lost; o[4] = h[b].n_unconfirmed; o[5] = h[b].drops;
  }
  return YM_OK;
}

// ---------------------------------------------------------------------------------- annotated frames
int ym_annotate(ym_ctx* c, const void* d_frames, int frames_are_f32_chw, int B, int H, int W, const float* d_dets,
                int max_det, const int* d_counts, const unsigned char* d_masks, const long long* d_mask_offsets,
                int mask_h, int mask_w, const int* d_mask_geo, const unsigned char* d_names, const ym_annotate_args* args,
                unsigned char* d_out, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_frames || !d_dets || !d_counts || !args || !d_out) return fail(YM_EINVAL, "ym_annotate: null pointer argument");
  if (!args->d_font) return fail(YM_EINVAL, "ym_annotate: no font table (ym_annotate_args.d_font)");
  if (B < 1 || B > 65535 || H < 1 || W < 1 || H > YM_ANNOT_MAX_SIDE || W > YM_ANNOT_MAX_SIDE)
    return fail(YM_EINVAL, "ym_annotate: batch %d of %d x %d frames (1..65535 of 1..%d a side)", B, H, W, YM_ANNOT_MAX_SIDE);
  if (max_det < 1 || max_det > (1 << 20)) return fail(YM_EINVAL, "ym_annotate: max_det %d", max_det);
  if (args->line_width < 1 || args->line_width > kAnnotMaxLw || args->kpt_radius < 0 || args->kpt_radius > kAnnotMaxLw)
    return fail(YM_EINVAL, "ym_annotate: line width %d (1..%d), keypoint radius %d (0..%d)", args->line_width, kAnnotMaxLw,
                args->kpt_radius, kAnnotMaxLw);
  if (args->K < 0 || args->K > kAnnotMaxK || (args->K > 0 && args->ndim != 2 && args->ndim != 3))
    return fail(YM_EINVAL, "ym_annotate: keypoint shape (%d, %d) (K 0..%d, ndim 2 | 3)", args->K, args->ndim, kAnnotMaxK);
  const int tracked = args->tracked ? 1 : 0;
  if (args->det_stride < 6 + tracked + args->K * (args->K ? args->ndim : 0) || args->det_stride > (1 << 16))
    return fail(YM_EINVAL, "ym_annotate: row stride %d below the %d values of a row with %d x %d keypoints",
                args->det_stride, 6 + tracked + args->K * args->ndim, args->K, args->ndim);
  if (args->color_mode != YM_ANNOT_COLOR_CLASS && args->color_mode != YM_ANNOT_COLOR_INSTANCE)
    return fail(YM_EINVAL, "ym_annotate: color_mode %d", args->color_mode);
  if (args->flags & ~(YM_ANNOT_BOXES | YM_ANNOT_LABELS | YM_ANNOT_CONF | YM_ANNOT_MASKS | YM_ANNOT_KPT_LINE | YM_ANNOT_CLIP_KPTS))
    return fail(YM_EINVAL, "ym_annotate: unknown switch bits 0x%x", args->flags);
  if (args->nc < 0 || (args->nc > 0 && !d_names)) return fail(YM_EINVAL, "ym_annotate: %d class names, null table", args->nc);
  if (d_masks && (!d_mask_offsets || mask_h < 1 || mask_w < 1 || mask_h > YM_ANNOT_MAX_SIDE || mask_w > YM_ANNOT_MAX_SIDE ||
                  args->mask_cap < 0))
    return fail(YM_EINVAL, "ym_annotate: masks of %d x %d bytes, offsets %p, cap %d", mask_h, mask_w,
                (const void*)d_mask_offsets, args->mask_cap);
  HIPCK(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const size_t need = (size_t)B * max_det;
  if (need > c->annot_recs) {  // (an earlier call may still read the old records)
    if (c->d_annot) {
      HIPCK(hipDeviceSynchronize());
      HIPCK(hipFree(c->d_annot));
      c->d_annot = nullptr;
      c->annot_recs = 0;
    }
    const hipError_t e = hipMalloc(&c->d_annot, need * sizeof(AnnotRec));
    if (e != hipSuccess) {
      c->d_annot = nullptr;
      return fail(YM_ENOMEM, "ym_annotate: %zu records: %s", need, hipGetErrorString(e));
    }
    c->annot_recs = need;
  }
  AnnotArgs a{};
  a.st.H = H; a.st.W = W; a.st.lw = args->line_width; a.st.radius = args->kpt_radius; a.st.flags = args->flags;
  a.st.by_instance = args->color_mode == YM_ANNOT_COLOR_INSTANCE; a.st.tracked = tracked;
  a.st.K = args->K; a.st.ndim = args->K ? args->ndim : 0; a.st.nc = args->nc;
  a.st.det_stride = args->det_stride; a.st.max_det = max_det;
  a.frames = d_frames; a.f32_chw = frames_are_f32_chw ? 1 : 0; a.B = B;
  a.dets = d_dets; a.counts = d_counts;
  a.masks = d_masks; a.mask_offsets = d_mask_offsets; a.mask_h = mask_h; a.mask_w = mask_w;
  a.mask_cap = args->mask_cap ? args->mask_cap : max_det; a.mask_geo = d_mask_geo;
  a.names = d_names; a.font = static_cast<const unsigned char*>(args->d_font);
  a.recs = c->d_annot; a.out = d_out;
  const hipError_t e = ym_launch_annotate(a, st);
  if (e != hipSuccess) return fail(YM_EHIP, "annotate kernels: %s", hipGetErrorString(e));
  return YM_OK;
}

// ---------------------------------------------------------------------------------- instance polygons
int ym_mask_contours(ym_ctx* c, const unsigned char* d_masks, int n, int H, int W, long long plane_stride, int* d_points,
                     long long cap_points, long long* d_offsets, void* stream) {
  if (!c) return fail(YM_EINVAL, "null context");
  if (!d_offsets || (n > 0 && !d_masks) || (cap_points > 0 && !d_points))
    return fail(YM_EINVAL, "ym_mask_contours: null pointer argument");
  if (n < 0 || H < 1 || W < 1 || (long long)H * W > kContourMaxPixels || cap_points < 0)
    return fail(YM_EINVAL, "ym_mask_contours: %d planes of %d x %d (1 x 1 .. 2^27 pixels), capacity %lld", n, H, W, cap_points);
  if (plane_stride < (long long)H * W)
    return fail(YM_EINVAL, "ym_mask_contours: plane stride %lld below %d x %d", plane_stride, H, W);
  HIPCK(hipSetDevice(c->device));
  hipStream_t st = static_cast<hipStream_t>(stream);
  const long long words = ym_ct_words(H, W);
  const bool in_lds = words <= kContourLdsWords;
  const size_t sel_bytes = ((size_t)n * sizeof(CtSel) + 255) & ~(size_t)255;
  const size_t need = sel_bytes + (in_lds ? 0 : (size_t)n * (size_t)words * sizeof(uint32_t));
  if (need > c->contour_bytes) {  // (an earlier call may still use the old scratch)
    if (c->d_contour) {
      HIPCK(hipDeviceSynchronize());
      HIPCK(hipFree(c->d_contour));
      c->d_contour = nullptr;
      c->contour_bytes = 0;
    }
    const hipError_t e = hipMalloc(&c->d_contour, need);
    if (e != hipSuccess) {
      c->d_contour = nullptr;
      return fail(YM_ENOMEM, "ym_mask_contours: %zu scratch bytes: %s", need, hipGetErrorString(e));
    }
    c->contour_bytes = need;
  }
  const hipError_t e = ym_launch_contours(d_masks, plane_stride, n, H, W,
                                          in_lds ? nullptr : reinterpret_cast<uint32_t*>(c->d_contour + sel_bytes),
                                          reinterpret_cast<CtSel*>(c->d_contour), d_points, cap_points, d_offsets, st);
  if (e != hipSuccess) return fail(YM_EHIP, "contour kernels: %s", hipGetErrorString(e));
  return YM_OK;
}

int ym_sync(ym_ctx* c) {
  if (!c) return fail(YM_EINVAL, "null context");
  HIPCK(hipSetDevice(c->device));
  HIPCK(hipDeviceSynchronize());
  return YM_OK;
}

void ym_destroy(ym_ctx* c) { delete c; }

}  // extern "C"
