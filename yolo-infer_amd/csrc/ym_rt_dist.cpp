// yolomi runtime, multi-GPU: the RCCL loader and the init-time weight broadcast.  Of a context it uses the device, the
// loaded blob, the control words in d_misc and ym_load_weights.
#include <dlfcn.h>

#include <algorithm>

#include "ym_runtime.h"

extern "C" {

// ---------------------------------------------------------------------------------------------- RCCL (xGMI)
// The init-time weight broadcast of the batch-sharded multi-GPU path: RCCL is resolved at run time
// (dlopen of the process's already-loaded librccl — torch's, when the host is Python — else the ROCm one), so
// libyolomi.so itself has no link-time dependency on it.  Only the four entry points below are used.
namespace {
struct Rccl {
  int (*get_id)(void*) = nullptr;
  int (*init)(void**, int, ym_rccl_id, int) = nullptr;
  int (*destroy)(void*) = nullptr;
  int (*user_rank)(void*, int*) = nullptr;
  int (*count)(void*, int*) = nullptr;
  int (*bcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  int (*allreduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;
  const char* (*err)(int) = nullptr;
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
    auto sym = [h](auto& fn, const char* name) { fn = reinterpret_cast<std::decay_t<decltype(fn)>>(dlsym(h, name)); };
    sym(x.get_id, "ncclGetUniqueId");      sym(x.init, "ncclCommInitRank");
    sym(x.destroy, "ncclCommDestroy");     sym(x.user_rank, "ncclCommUserRank");
    sym(x.count, "ncclCommCount");         sym(x.bcast, "ncclBroadcast");
    sym(x.allreduce, "ncclAllReduce");     sym(x.err, "ncclGetErrorString");
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

}  // extern "C"
