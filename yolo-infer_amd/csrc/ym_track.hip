// ByteTrack behind the NMS: one launch per frame batch, one workgroup (a single wavefront) per stream, the track
// table resident in device memory (Ultralytics BYTETracker.update with bytetrack.yaml's defaults).
//
// Why one wavefront: the hot loop is the assignment's augmenting-path step — scan the columns for the smallest
// reduced weight, reduce to the minimum, update the potentials.  With at most kTrackDim = 512 columns that is 8
// columns per lane, and the reduction over 64 lanes is six cross-lane exchanges; a second wavefront would turn every
// step's reduction into an LDS round trip with a barrier.  The Kalman steps are per track (fp64, 8 x 8) and run one
// track per lane.
//
// Phases (a barrier between every two; every loop has a compile-time bound):
//   load        detections and the slots' discrete state into LDS
//   predict     pool = activated tracked + lost: Kalman predict (a lost track's height velocity zeroed first); every
//               live track's fp32 box from its mean
//   assoc 1     pool x high detections, 1 - IoU * conf, match_thresh         -> update / re-activate
//   assoc 2     unmatched tracked pool rows x second detections, 1 - IoU, 0.5 -> update; the rest become lost
//   assoc 3     unconfirmed x remaining high detections, 1 - IoU * conf, 0.7  -> update; the rest are removed
//   age out     tracks lost before this frame and older than max_time_lost
//   start       remaining high detections >= new_track_thresh take free slots and new ids in row order
//   dedupe      tracked / lost pairs with 1 - IoU < 0.15: the one seen for fewer frames goes (a tie: the tracked one)
//   output      activated tracked tracks in ascending id order, each with the row index of its detection
// Costs are computed from the LDS boxes when the assignment asks for them; no cost matrix is stored.
#include <hip/hip_runtime.h>

#include <climits>

#include "ym_track.h"

namespace {

struct TrackShared {
  float dbox[kTrackMaxDet][4];
  float dconf[kTrackMaxDet];
  float tbox[kTrackCap][4];
  double u[kTrackDim + 1], v[kTrackDim + 1], minv[kTrackDim + 1];
  int p[kTrackDim + 1], way[kTrackDim + 1], sel[kTrackDim + 1];
  int r2c[kTrackDim];
  int rows[kTrackCap], rows2[kTrackCap];  // slot lists
  int cols[kTrackMaxDet];                 // a detection list
  int s_id[kTrackCap], s_det[kTrackCap], s_age[kTrackCap];
  unsigned char s_state[kTrackCap], s_act[kTrackCap], s_drop[kTrackCap];
  unsigned char used[kTrackDim + 1];
  unsigned char dused[kTrackMaxDet];
};
static_assert(sizeof(TrackShared) <= 64 * 1024, "the tracker's LDS fits the static limit");

struct WaveLanes {
  __device__ int lane() const { return threadIdx.x; }
  __device__ int lanes() const { return kTrackLanes; }
  __device__ void sync() const { __syncthreads(); }
  __device__ void argmin(double& val, int& j) const {
    int jj = j < 0 ? INT_MAX : j;
    for (int off = kTrackLanes / 2; off > 0; off >>= 1) {
      const double ov = __shfl_xor(val, off, kTrackLanes);
      const int oj = __shfl_xor(jj, off, kTrackLanes);
      if (ov < val || (ov == val && oj < jj)) {
        val = ov;
        jj = oj;
      }
    }
    j = jj == INT_MAX ? -1 : jj;
  }
  __device__ void take_min(int* a, int v) const { atomicMin(a, v); }
};

// list[0 .. count) = the j < n with pred(j), ascending; every lane returns the count.  n <= kTrackDim.
template <class Pred>
__device__ int compact(int n, int* list, Pred pred) {
  const int ln = threadIdx.x;
  int base = 0;
  for (int c = 0; c < kTrackDim; c += kTrackLanes) {
    if (c >= n) break;
    const int j = c + ln;
    const bool f = j < n && pred(j);
    const unsigned long long m = __ballot(f);
    if (f) list[base + __popcll(m & ((1ull << ln) - 1ull))] = j;
    base += __popcll(m);
  }
  return base;
}

struct Frame {
  TrackShared* sh;
  TrackSlot* slots;
  const float* drow;
  int stride, frame;
};

// The matched track takes the detection: Kalman update, then upstream's STrack.update / re_activate bookkeeping.
__device__ void take_detection(const Frame& f, int s, int d) {
  TrackShared& sh = *f.sh;
  TrackSlot& t = f.slots[s];
  double m[8], c[64], z[4];
  for (int i = 0; i < 8; ++i) m[i] = t.mean[i];
  for (int i = 0; i < 64; ++i) c[i] = t.cov[i];
  ym_xyxy_to_xyah(sh.dbox[d], z);
  ym_kf_update(m, c, z);
  for (int i = 0; i < 8; ++i) t.mean[i] = m[i];
  for (int i = 0; i < 64; ++i) t.cov[i] = c[i];
  t.tracklet_len = sh.s_state[s] == YM_TRK_TRACKED ? t.tracklet_len + 1 : 0;
  t.state = YM_TRK_TRACKED;
  t.is_activated = 1;
  t.end_frame = f.frame;
  t.score = sh.dconf[d];
  t.cls = f.drow[(size_t)d * f.stride + 5];
  sh.s_state[s] = YM_TRK_TRACKED;
  sh.s_act[s] = 1;
  sh.s_det[s] = d;
  sh.dused[d] = 1;
}

// One association: rows (slots) x cols (detections), then the matches' updates.  r2c is left for the caller.
__device__ __noinline__ void associate(const Frame& f, const int* rows, int nr, const int* cols, int nc, bool fuse,
                                       double thresh) {
  TrackShared& sh = *f.sh;
  const AssignWork ws{sh.u, sh.v, sh.minv, sh.p, sh.way, sh.sel, sh.used};
  auto w = [&](int i, int j) -> double {
    const int d = cols[j];
    const float iou = ym_iou32(sh.tbox[rows[i]], sh.dbox[d]);
    const float c = 1.0f - (fuse ? iou * sh.dconf[d] : iou);
    return (double)c < thresh ? (double)c - thresh : 0.0;  // a NaN cost is no match
  };
  ym_assign(nr, nc, w, WaveLanes{}, ws, sh.r2c);
  for (int i = threadIdx.x; i < kTrackCap; i += kTrackLanes) {
    if (i >= nr) break;
    const int c = sh.r2c[i];
    if (c >= 0) take_detection(f, rows[i], cols[c]);
  }
  __syncthreads();
}

__global__ __launch_bounds__(kTrackLanes) void track_update(const TrackArgs a) {
  __shared__ TrackShared sh;
  const int b = blockIdx.x, ln = threadIdx.x;
  const int cap = a.cap < kTrackCap ? a.cap : kTrackCap;
  TrackSlot* slots = a.slots + (size_t)b * a.cap;
  TrackHead* head = a.heads + b;
  int n = a.counts[b];
  n = n < 0 ? 0 : n > a.max_det ? a.max_det : n;
  n = n > kTrackMaxDet ? kTrackMaxDet : n;
  if (n == 0) {  // upstream's callback leaves a frame without detections alone: the tracker does not advance
    if (ln == 0) a.track_counts[b] = 0;
    return;
  }
  const float* drow = a.dets + (size_t)b * a.max_det * a.det_stride;
  const int tstride = a.det_stride + 1;
  float* trow = a.tracks + (size_t)b * a.max_det * tstride;
  int* irow = a.idx + (size_t)b * a.max_det;
  const int frame = head->frame_id + 1;
  const Frame f{&sh, slots, drow, a.det_stride, frame};

  // ---- load
  for (int j = ln; j < kTrackDim; j += kTrackLanes) {
    if (j < n) {
      for (int k = 0; k < 4; ++k) sh.dbox[j][k] = drow[(size_t)j * a.det_stride + k];
      sh.dconf[j] = drow[(size_t)j * a.det_stride + 4];
      sh.dused[j] = 0;
    }
    if (j < cap) {
      sh.s_state[j] = (unsigned char)slots[j].state;
      sh.s_act[j] = slots[j].is_activated != 0;
      sh.s_id[j] = slots[j].id;
      sh.s_age[j] = slots[j].state == YM_TRK_LOST;  // until the duplicates phase: lost before this frame
      sh.s_det[j] = -1;
      sh.s_drop[j] = 0;
    }
  }
  __syncthreads();

  // ---- predict the pool; boxes of every live track
  for (int s = ln; s < kTrackCap; s += kTrackLanes) {
    if (s >= cap) break;
    const int st = sh.s_state[s];
    if (st == YM_TRK_FREE) continue;
    TrackSlot& t = slots[s];
    double m[8], xy[4];
    for (int i = 0; i < 8; ++i) m[i] = t.mean[i];
    if (st == YM_TRK_LOST || sh.s_act[s]) {
      double c[64];
      for (int i = 0; i < 64; ++i) c[i] = t.cov[i];
      if (st != YM_TRK_TRACKED) m[7] = 0;
      ym_kf_predict(m, c);
      for (int i = 0; i < 8; ++i) t.mean[i] = m[i];
      for (int i = 0; i < 64; ++i) t.cov[i] = c[i];
    }
    ym_mean_to_xyxy(m, xy);
    for (int k = 0; k < 4; ++k) sh.tbox[s][k] = (float)xy[k];
  }
  __syncthreads();

  // ---- association 1: pool x high
  const float high = a.high, low = a.low;
  int nr = compact(cap, sh.rows, [&](int s) { return sh.s_state[s] == YM_TRK_LOST || (sh.s_state[s] && sh.s_act[s]); });
  int nc = compact(n, sh.cols, [&](int j) { return sh.dconf[j] >= high; });
  __syncthreads();
  associate(f, sh.rows, nr, sh.cols, nc, a.fuse != 0, a.match);

  // ---- association 2: the pool's unmatched tracked rows x second detections; then the unmatched become lost
  const int nr2 = compact(nr, sh.rows2, [&](int i) { return sh.r2c[i] < 0 && sh.s_state[sh.rows[i]] == YM_TRK_TRACKED; });
  nc = compact(n, sh.cols, [&](int j) { return sh.dconf[j] > low && sh.dconf[j] < high; });
  __syncthreads();
  for (int i = ln; i < kTrackCap; i += kTrackLanes) {  // positions in rows -> slots
    if (i >= nr2) break;
    sh.rows2[i] = sh.rows[sh.rows2[i]];
  }
  __syncthreads();
  associate(f, sh.rows2, nr2, sh.cols, nc, false, 0.5);
  for (int i = ln; i < kTrackCap; i += kTrackLanes) {
    if (i >= nr2) break;
    if (sh.r2c[i] < 0) {
      const int s = sh.rows2[i];
      slots[s].state = YM_TRK_LOST;
      sh.s_state[s] = YM_TRK_LOST;
    }
  }
  __syncthreads();

  // ---- association 3: unconfirmed x the high detections association 1 left; unmatched unconfirmed tracks go
  nr = compact(cap, sh.rows, [&](int s) { return sh.s_state[s] == YM_TRK_TRACKED && !sh.s_act[s]; });
  nc = compact(n, sh.cols, [&](int j) { return sh.dconf[j] >= high && !sh.dused[j]; });
  __syncthreads();
  associate(f, sh.rows, nr, sh.cols, nc, a.fuse != 0, 0.7);
  for (int i = ln; i < kTrackCap; i += kTrackLanes) {
    if (i >= nr) break;
    if (sh.r2c[i] < 0) {
      const int s = sh.rows[i];
      slots[s].state = YM_TRK_FREE;
      sh.s_state[s] = YM_TRK_FREE;
    }
  }
  // ---- age out
  __syncthreads();
  for (int s = ln; s < kTrackCap; s += kTrackLanes) {
    if (s >= cap) break;
    if (sh.s_age[s] && sh.s_state[s] == YM_TRK_LOST && frame - slots[s].end_frame > a.max_time_lost) {
      slots[s].state = YM_TRK_FREE;
      sh.s_state[s] = YM_TRK_FREE;
    }
  }
  __syncthreads();

  // ---- start new tracks: the k-th remaining detection takes the k-th free slot and id issued + 1 + k
  const float newt = a.new_thresh;
  const int nfree = compact(cap, sh.rows, [&](int s) { return sh.s_state[s] == YM_TRK_FREE; });
  const int nnew = compact(n, sh.cols, [&](int j) { return sh.dconf[j] >= high && !sh.dused[j] && sh.dconf[j] >= newt; });
  __syncthreads();
  const int issued = head->issued;
  const int started = nnew < nfree ? nnew : nfree;
  for (int k = ln; k < kTrackMaxDet; k += kTrackLanes) {
    if (k >= started) break;
    const int s = sh.rows[k], d = sh.cols[k];
    TrackSlot& t = slots[s];
    double m[8], c[64], z[4];
    ym_xyxy_to_xyah(sh.dbox[d], z);
    ym_kf_initiate(z, m, c);
    for (int i = 0; i < 8; ++i) t.mean[i] = m[i];
    for (int i = 0; i < 64; ++i) t.cov[i] = c[i];
    t.state = YM_TRK_TRACKED;
    t.id = issued + 1 + k;
    t.score = sh.dconf[d];
    t.cls = drow[(size_t)d * a.det_stride + 5];
    t.start_frame = t.end_frame = frame;
    t.tracklet_len = 0;
    t.is_activated = frame == 1;
    sh.s_state[s] = YM_TRK_TRACKED;
    sh.s_act[s] = frame == 1;
    sh.s_id[s] = t.id;
    sh.s_det[s] = d;
  }
  __syncthreads();

  // ---- duplicates: boxes from the updated means, tracked x lost
  for (int s = ln; s < kTrackCap; s += kTrackLanes) {
    if (s >= cap) break;
    if (sh.s_state[s] == YM_TRK_FREE) continue;
    double xy[4];
    ym_mean_to_xyxy(slots[s].mean, xy);
    for (int k = 0; k < 4; ++k) sh.tbox[s][k] = (float)xy[k];
    sh.s_age[s] = slots[s].end_frame - slots[s].start_frame;
  }
  __syncthreads();
  const int na = compact(cap, sh.rows, [&](int s) { return sh.s_state[s] == YM_TRK_TRACKED; });
  const int nb = compact(cap, sh.rows2, [&](int s) { return sh.s_state[s] == YM_TRK_LOST; });
  __syncthreads();
  const int pairs = na * nb;  // na + nb <= kTrackCap
  for (int it = 0; it < kTrackCap * kTrackCap / 4 / kTrackLanes; ++it) {
    if (it * kTrackLanes >= pairs) break;
    const int q = it * kTrackLanes + ln;
    if (q < pairs) {
      const int sa = sh.rows[q / nb], sb = sh.rows2[q % nb];
      if (1.0f - ym_iou32(sh.tbox[sa], sh.tbox[sb]) < 0.15f) sh.s_drop[sh.s_age[sa] > sh.s_age[sb] ? sb : sa] = 1;
    }
  }
  __syncthreads();
  for (int s = ln; s < kTrackCap; s += kTrackLanes) {
    if (s >= cap) break;
    if (sh.s_drop[s]) {
      slots[s].state = YM_TRK_FREE;
      sh.s_state[s] = YM_TRK_FREE;
    }
  }
  __syncthreads();

  // ---- output: activated tracked tracks by ascending id
  const int nout = compact(cap, sh.rows, [&](int s) { return sh.s_state[s] == YM_TRK_TRACKED && sh.s_act[s]; });
  const int nlost = compact(cap, sh.rows2, [&](int s) { return sh.s_state[s] == YM_TRK_LOST; });
  __syncthreads();
  const int nunc = compact(cap, sh.rows2, [&](int s) { return sh.s_state[s] == YM_TRK_TRACKED && !sh.s_act[s]; });
  for (int k = ln; k < kTrackCap; k += kTrackLanes) {
    if (k >= nout) break;
    const int s = sh.rows[k], id = sh.s_id[s];
    int r = 0;
    for (int k2 = 0; k2 < kTrackCap; ++k2) {
      if (k2 >= nout) break;
      r += sh.s_id[sh.rows[k2]] < id;
    }
    if (r >= a.max_det) continue;  // cannot happen: every output track took a distinct detection of this frame
    const TrackSlot& t = slots[s];
    double xy[4];
    ym_mean_to_xyxy(t.mean, xy);
    float* o = trow + (size_t)r * tstride;
    for (int i = 0; i < 4; ++i) o[i] = (float)xy[i];
    o[4] = (float)id;
    o[5] = t.score;
    o[6] = t.cls;
    const int d = sh.s_det[s];
    for (int e = 6; e < kTrackMaxStride; ++e) {  // the detection's extras (pose: its keypoints)
      if (e >= a.det_stride) break;
      o[e + 1] = d >= 0 ? drow[(size_t)d * a.det_stride + e] : 0.0f;
    }
    irow[r] = d;
  }
  if (ln == 0) {
    head->frame_id = frame;
    head->issued = issued + started;
    head->drops += nnew - started;
    head->n_tracked = nout;
    head->n_lost = nlost;
    head->n_unconfirmed = nunc;
    a.track_counts[b] = nout < a.max_det ? nout : a.max_det;
  }
}

}  // namespace

hipError_t ym_launch_track(const TrackArgs& a, int B, hipStream_t st) {
  if (B < 1 || a.cap < 1 || a.cap > kTrackCap || a.max_det < 1 || a.max_det > kTrackMaxDet || a.det_stride < 6 ||
      a.det_stride > kTrackMaxStride)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(track_update, dim3(B), dim3(kTrackLanes), 0, st, a);
  return hipGetLastError();
}
