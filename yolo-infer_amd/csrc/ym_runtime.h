// What the runtime's units share (private, not installed; DESIGN.md §5 maps the units).  Everything between the
// visibility pragmas is hidden: shared by the units, absent from the library's dynamic symbol table.
#pragma once
#include <hip/hip_runtime.h>
#include <cstring>
#include <type_traits>
#include <vector>
#include "../../include/yolomi.h"
#include "ym_common.h"
#include "ym_plan.h"
#include "ym_nms_ws.h"
#include "ym_classify.h"
#include "ym_devbuf.h"

#pragma GCC visibility push(hidden)

int fail(int code, const char* fmt, ...);  // sets ym_last_error's thread-local text (ym_runtime.cpp), returns code

// The status of the launch that ends an entry point: YM_OK, or YM_EHIP with "<what>: <HIP's text>"
inline int launched(hipError_t e, const char* what) {
  return e == hipSuccess ? YM_OK : fail(YM_EHIP, "%s: %s", what, hipGetErrorString(e));
}

#define HIPCK(x)                                                                            \
  do {                                                                                        \
    hipError_t e_ = (x);                                                                      \
    if (e_ != hipSuccess) return fail(YM_EHIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); \
  } while (0)

// A host read of device memory (tests, tools): every stream of the device drains first
inline int read_back(int device, void* dst, const void* src, size_t bytes) {
  HIPCK(hipSetDevice(device));
  HIPCK(hipDeviceSynchronize());
  HIPCK(hipMemcpy(dst, src, bytes, hipMemcpyDefault));
  return YM_OK;
}

constexpr int kSplitCounters = 16384;  // split-K tiles per conv launch (csrc/ym_conv_dma.hip)
constexpr int kChainCtl = 4096;        // ready counters (+ done, give-up words) of the persistent chain kernel
constexpr float kPresortConf = 0.1f;  // NMS keys presorted over several workgroups below this conf (ym_nms.hip)
constexpr int kMaxLanes = 4;           // concurrent batch slices in one forward graph (<= GPU_MAX_HW_QUEUES)
constexpr size_t kMaxGraphs = 16;      // captured forwards cached per context (the oldest is retired first)
// ym_ctx::d_misc and its sub-regions: ym_input_max's statistics (slots, ticket, partials), the control words of
// ym_broadcast_weights, and the words that stand in for the outputs of a forward that writes none (never written)
constexpr size_t kMiscBytes = 16384, kMiscStats = 0, kMiscBcast = 8192, kMiscNoDets = 12288;
static_assert(kMiscStats + YM_CTL_BYTES <= kMiscBcast && kMiscBcast + 2 * sizeof(unsigned long long) <= kMiscNoDets &&
                  kMiscNoDets < kMiscBytes, "the d_misc sub-regions fit in kMiscBytes and do not overlap");

inline size_t align_up(size_t x, size_t a) { return (x + a - 1) / a * a; }

// Where a ym_classify call's results go (null members: the context's own scratch, ym_ctx::cls_view)
struct ClsOut {
  float* probs = nullptr;
  long long ld = 0;
  float* logits = nullptr;
  int* topk = nullptr;
  float* topk_conf = nullptr;
};

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
  ClsOut cls;             // ym_classify: the caller's outputs
};

struct GraphKey {
  int B, H, W;
  int skip_nms;  // 1: a ym_tta_forward capture (no NMS stage)
  int embed_stop;  // ym_embed captures: 1 + the last op of the truncated forward (0: a whole forward) ...
  int embed_n;     // ... the views pooled behind it (GraphEntry::embed_views) ...
  const void* embed_out;  // ... and where their means go
  long long embed_ld;
  ClsOut cls;  // ym_classify captures: the outputs the head's launches write
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

// Destroy a captured forward only after its last launch has finished on whatever stream it was replayed on: the
// HIP runtime may still hold the exec's launch state (kernel arguments, the packet chain) while it is in flight.
void retire_graph(GraphEntry& g);

#pragma GCC visibility pop

struct ym_ctx {
  int device = 0;
  ym_model_desc desc{};
  bool loaded = false;
  // plan
  int dtype = YM_DT_F16, task = 0, nc = 80, nm = 0, reg_max = 16, nl = 3;
  int strides[4] = {8, 16, 32, 0};
  int input_buf = -1, anchor_buf = -1, proto_buf = -1, no = 0;
  int kpt_K = 0, kpt_ndim = 0, kpt_off = 0;  // pose plans: keypoints, 2 | 3 values each, raw offset in the anchor row
  char* d_misc = nullptr;     // 16 KB: ym_input_max statistics region, ym_broadcast_weights control words
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
  // obb plans: per anchor the (theta, A, B, C) float4 of obb_decode, the sorted ObbEntry and the keep byte, per image
  // the sorted count (csrc/ym_obb.hip); the regions hold cB images each
  size_t off_obb_cov = 0, off_obb_sorted = 0, off_obb_keep = 0, off_obb_nsel = 0;
  // classify plans: the head's op and its scratch in the arena — pooled (B, 1280), then logits, probs (B, nc each),
  // top-k classes and probabilities (B, kClsTopK each), all fp32 / int32; a call's own outputs replace the last four
  int cls_op = -1;
  size_t off_cls = 0;
  size_t cls_bytes(int nB) const { return (size_t)nB * (kClsHidden + 2 * (size_t)nc + 2 * kClsTopK) * 4; }
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
  // reads embed_views into embed_out; `embed` holds the chunk partials of large maps
  std::vector<ym_embed_view> embed_views;
  float* embed_out = nullptr;
  long long embed_ld = 0;
  // Scratch grown on demand (ym_devbuf.h), each private to one stage beside the forward: ym_embed's chunk partials;
  // ym_masks' (total, MH, MW) prototype-resolution planes (two-kernel path); ym_annotate's AnnotRec records of the
  // B x max_det detection slots; ym_mask_contours' n CtSel records, then (planes too large for LDS only) n bit planes of
  // ym_ct_words(H, W) words; ym_mask_rle's per (plane, strip) two RleAgg, the set pixels and the strip's bit words, per
  // plane one RleAgg (ym_rle.h RleScratch)
  DevBuf embed, lowres, annot, contour, rle;
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
  // (the two members that take a GraphEntry are hidden as it is)
  __attribute__((visibility("hidden"))) int launch_graph(GraphEntry& g, hipStream_t st) {
    HIPCK(hipGraphLaunch(g.exec, st));
    return record_last(g.done, st);
  }
  // retire_graph, forgetting last_ev when it is that graph's event (now complete)
  __attribute__((visibility("hidden"))) void retire(GraphEntry& g) {
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

  ~ym_ctx() {  // (the DevBuf members free themselves behind this body, on the device it sets)
    (void)hipSetDevice(device);
    clear_graphs();
    for (auto e : prof_events) (void)hipEventDestroy(e);
    if (d_arena) (void)hipFree(d_arena);
    if (d_weights) (void)hipFree(d_weights);
    if (d_misc) (void)hipFree(d_misc);
    if (tta.d) (void)hipFree(tta.d);
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

#pragma GCC visibility push(hidden)

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
inline NmsView nms_view(char* base, const NmsScratch& s, int img0) {
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

// Where an NMS stage reads per-candidate rows: the nm extras the NMS kernel copies behind each kept box, and the
// class scores the multi-label candidate stage thresholds (both (B, A, *_ld) fp32; null: none)
struct NmsSource {
  const float* extras; int extras_ld, mask_off;
  const float* cls; int cls_ld, cls_off;
};

// An entry point's first checks: a context, a plan loaded into it and (want: "an obb", "a classify") of that task
int check_ctx(const ym_ctx* c, const char* who, int task = -1, const char* want = nullptr);
// B images of H x W; `who`: the message's prefix ("" or "entry point: ")
int check_shape(int B, int H, int W, const char* who);
int check_nms_args(const ym_infer_args* args, int nc, int task);
int ensure_workspace(ym_ctx* c, int B, int H, int W);
// Behind the checks, for every entry point that launches ops: device, workspace, stream order; L: one whole-batch launch
int begin_launch(ym_ctx* c, int B, int H, int W, hipStream_t st, Launch& L);
// The NMS stage over B images of the candidates in `v` (decode_anchors' or the TTA merge's): single-label, with the
// keys presorted at low conf, or multi-label.  The forward's OP_NMS and ym_tta_nms both end here.
hipError_t launch_nms_stage(const NmsView& v, const NmsSource& src, const ym_infer_args* args, int B, int nc, int nm,
                            int H, int W, float* dets, int* out_counts, int* counts2, hipStream_t st);

// What reaches a forward that writes no detections (ym_classify, ym_embed): the /255 rule's inputs and the launch
// mode of `args`; one lane; the NMS defaults ...
inline ym_infer_args forward_only_args(const ym_infer_args* args) {
  ym_infer_args fa{};
  fa.conf = 0.25f; fa.max_wh = 7680.f; fa.iou = 0.7; fa.max_det = 300; fa.max_nms = 30000;
  fa.in_eps = args->in_eps; fa.use_graph = args->use_graph; fa.lanes = 1; fa.d_batch_max = args->d_batch_max;
  return fa;
}
// ... and the device words that stand in for its rows and counts (the NMS stage is their only writer: never written)
inline float* no_dets(const ym_ctx* c) { return reinterpret_cast<float*>(c->d_misc + kMiscNoDets); }
// The Detect levels' geometry at the workspace shape, for any kernel argument struct that carries it ...
template <typename A> void set_levels(A& a, const ym_ctx* c) {
  a.nl = c->nl;
  for (int l = 0; l < c->nl; ++l) {
    a.lvl_W[l] = c->lvl_W[l]; a.lvl_off[l] = c->lvl_off[l]; a.lvl_stride[l] = (float)c->strides[l];
  }
}
template <typename A> void set_filter(A& a, const ym_infer_args* args) {  // ... and a call's candidate filter
  a.conf = args->conf; a.has_classes = args->has_classes;
  for (int i = 0; i < 4; ++i) a.classes[i] = args->classes[i];
}
// counts_after_dets: image img0's count word behind the `images_left` images' rows (row_floats each) at d_dets
inline int* counts_behind(float* d_dets, int images_left, int max_det, int row_floats, int img0) {
  return reinterpret_cast<int*>(d_dets + (size_t)images_left * max_det * row_floats) + img0;
}

#pragma GCC visibility pop
