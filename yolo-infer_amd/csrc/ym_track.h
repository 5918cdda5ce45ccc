// Multi-object tracking behind the NMS (csrc/ym_track.hip; driven by ym_track_update in ym_runtime.cpp): Ultralytics
// BYTETracker.update with bytetrack.yaml's defaults, one workgroup per stream, tracker state resident in device memory.
//
// This header holds what the kernel and a stand-alone host program share (tests/track_check.cpp includes only this
// file): the table layout, the XYAH constant-velocity Kalman filter on plain fp64 arrays, the fp32 IoU of upstream's
// bbox_ioa, and the assignment — a shortest-augmenting-path (Hungarian / Jonker-Volgenant) solver on clipped weights
// that is written against a small "lanes" interface, so the same text runs serially on the host and across the lanes
// of one wavefront on the device.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#define YM_HD __host__ __device__
#else
#define YM_HD
#endif

constexpr int kTrackCap = 512;     // track slots per stream (tracked + lost + unconfirmed), at most
constexpr int kTrackMaxDet = 300;  // detections per frame and stream, at most (predict's default max_det)
constexpr int kTrackLanes = 64;    // one wavefront per stream
constexpr int kTrackMaxStride = 64; // floats per detection row, at most (pose: 6 + 52)
constexpr int kTrackDim = kTrackCap > kTrackMaxDet ? kTrackCap : kTrackMaxDet;  // the assignment's longer side

enum { YM_TRK_FREE = 0, YM_TRK_TRACKED = 1, YM_TRK_LOST = 2 };  // FREE = 0: a zeroed table is an empty one

struct TrackSlot {
  double mean[8];   // cx, cy, a = w / h, h and their velocities
  double cov[64];   // row-major 8 x 8
  int state;        // YM_TRK_*
  int id;
  float score, cls;
  int start_frame, end_frame;  // end_frame: the frame of the last update (upstream STrack.frame_id)
  int tracklet_len;
  int is_activated;
};

struct TrackHead {  // per stream; zeroed by a reset
  int frame_id;
  int issued;  // ids handed out so far: the next track gets issued + 1
  int n_tracked, n_lost, n_unconfirmed;  // after the last update: activated tracked, lost, not yet activated
  int drops;   // detections that would have started a track while the table was full
  int reserved[2];
};

struct TrackArgs {
  TrackSlot* slots;  // (streams, cap)
  TrackHead* heads;  // (streams)
  int cap;           // slots per stream in use, 1..kTrackCap
  const float* dets; // (B, max_det, det_stride) NMS rows [x1 y1 x2 y2 conf cls extras]
  int det_stride, max_det;
  const int* counts;  // (B)
  float* tracks;      // (B, max_det, det_stride + 1) rows [x1 y1 x2 y2 id score cls extras]
  int* idx;           // (B, max_det): the detection row that fed each track row
  int* track_counts;  // (B)
  float high, low, new_thresh;  // score thresholds, compared in fp32 like upstream's fp32 scores
  double match;                 // association 1's cost limit
  int max_time_lost, fuse;
};

// ------------------------------------------------------------------------------------------------ Kalman filter
constexpr double kKfPos = 1.0 / 20, kKfVel = 1.0 / 160;

// Detection corners (fp32 values) -> the measurement [cx, cy, a, h].
YM_HD inline void ym_xyxy_to_xyah(const float b[4], double z[4]) {
  const double w = (double)b[2] - (double)b[0], h = (double)b[3] - (double)b[1];
  z[0] = (double)b[0] + w / 2;
  z[1] = (double)b[1] + h / 2;
  z[2] = w / h;
  z[3] = h;
}

// The filter mean -> corners (upstream STrack.tlwh, then xyxy).
YM_HD inline void ym_mean_to_xyxy(const double mean[8], double out[4]) {
  const double w = mean[2] * mean[3], h = mean[3];
  out[0] = mean[0] - w / 2;
  out[1] = mean[1] - h / 2;
  out[2] = out[0] + w;
  out[3] = out[1] + h;
}

YM_HD inline void ym_kf_initiate(const double z[4], double mean[8], double cov[64]) {
  for (int i = 0; i < 4; ++i) {
    mean[i] = z[i];
    mean[4 + i] = 0;
  }
  const double h = z[3];
  const double sd[8] = {2 * kKfPos * h, 2 * kKfPos * h, 1e-2, 2 * kKfPos * h,
                        10 * kKfVel * h, 10 * kKfVel * h, 1e-5, 10 * kKfVel * h};
  for (int i = 0; i < 64; ++i) cov[i] = 0;
  for (int i = 0; i < 8; ++i) cov[9 * i] = sd[i] * sd[i];
}

// mean = F mean, cov = F cov F^T + Q with F = [[I, I], [0, I]]: two passes of row / column additions.
YM_HD inline void ym_kf_predict(double mean[8], double cov[64]) {
  const double h = mean[3];
  const double sd[8] = {kKfPos * h, kKfPos * h, 1e-2, kKfPos * h, kKfVel * h, kKfVel * h, 1e-5, kKfVel * h};
  for (int i = 0; i < 4; ++i) mean[i] += mean[4 + i];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 8; ++j) cov[8 * i + j] += cov[8 * (i + 4) + j];
  for (int i = 0; i < 8; ++i)
    for (int j = 0; j < 4; ++j) cov[8 * i + j] += cov[8 * i + j + 4];
  for (int i = 0; i < 8; ++i) cov[9 * i] += sd[i] * sd[i];
}

// Project to measurement space (S = H cov H^T + R), then the gain through S's Cholesky factor:
// K = cov H^T S^-1, mean += K (z - H mean), cov -= K S K^T.
YM_HD inline void ym_kf_update(double mean[8], double cov[64], const double z[4]) {
  const double h = mean[3];
  const double sd[4] = {kKfPos * h, kKfPos * h, 1e-1, kKfPos * h};
  double S[16], L[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) S[4 * i + j] = cov[8 * i + j] + (i == j ? sd[i] * sd[i] : 0.0);
  for (int i = 0; i < 16; ++i) L[i] = 0;
  for (int j = 0; j < 4; ++j) {  // S = L L^T, L lower
    double d = S[4 * j + j];
    for (int k = 0; k < j; ++k) d -= L[4 * j + k] * L[4 * j + k];
    d = sqrt(d);
    L[4 * j + j] = d;
    for (int i = j + 1; i < 4; ++i) {
      double s = S[4 * i + j];
      for (int k = 0; k < j; ++k) s -= L[4 * i + k] * L[4 * j + k];
      L[4 * i + j] = s / d;
    }
  }
  double K[32], KS[32];
  for (int r = 0; r < 8; ++r) {  // row r of K solves S k = (cov H^T)[r, :]
    double y[4];
    for (int i = 0; i < 4; ++i) {
      double s = cov[8 * r + i];
      for (int k = 0; k < i; ++k) s -= L[4 * i + k] * y[k];
      y[i] = s / L[4 * i + i];
    }
    for (int i = 3; i >= 0; --i) {
      double s = y[i];
      for (int k = i + 1; k < 4; ++k) s -= L[4 * k + i] * K[4 * r + k];
      K[4 * r + i] = s / L[4 * i + i];
    }
  }
  double inn[4];
  for (int i = 0; i < 4; ++i) inn[i] = z[i] - mean[i];
  for (int r = 0; r < 8; ++r) {
    double s = 0;
    for (int k = 0; k < 4; ++k) s += inn[k] * K[4 * r + k];
    mean[r] += s;
  }
  for (int r = 0; r < 8; ++r)
    for (int j = 0; j < 4; ++j) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += K[4 * r + k] * S[4 * k + j];
      KS[4 * r + j] = s;
    }
  for (int r = 0; r < 8; ++r)
    for (int c = 0; c < 8; ++c) {
      double s = 0;
      for (int k = 0; k < 4; ++k) s += KS[4 * r + k] * K[4 * c + k];
      cov[8 * r + c] -= s;
    }
}

// ------------------------------------------------------------------------------------------------ IoU
// upstream bbox_ioa(iou=True) on fp32 corners, eps 1e-7
YM_HD inline float ym_iou32(const float a[4], const float b[4]) {
  float iw = (a[2] < b[2] ? a[2] : b[2]) - (a[0] > b[0] ? a[0] : b[0]);
  float ih = (a[3] < b[3] ? a[3] : b[3]) - (a[1] > b[1] ? a[1] : b[1]);
  iw = iw > 0 ? iw : 0;
  ih = ih > 0 ? ih : 0;
  const float inter = iw * ih;
  const float area = (b[2] - b[0]) * (b[3] - b[1]) + (a[2] - a[0]) * (a[3] - a[1]) - inter;
  return inter / (area + 1e-7f);
}

// ------------------------------------------------------------------------------------------------ assignment
// The partial matching that maximises the sum of (thresh - cost) over its pairs, i.e. lap.lapjv(cost, extend_cost=True,
// cost_limit=thresh): with weights w(i, j) = min(cost - thresh, 0) <= 0 it is a minimum-weight matching of every row of
// the shorter side, from which the zero-weight pairs are then dropped.
//
// Lanes interface (Par): lane(), lanes(), sync() — a barrier that also makes the work arrays' writes visible —,
// argmin(value, index) — every lane receives the smallest value and, among equal values, the smallest index — and
// take_min(address, value) — *address = min(*address, value), atomically among the lanes.
struct AssignWork {  // all of kTrackDim + 1 entries (index 0 of the column arrays is the solver's dummy column)
  double* u;     // row potentials
  double* v;     // column potentials
  double* minv;  // per column: the smallest reduced weight seen from the current tree
  int* p;        // column -> its row (1-based; 0: free)
  int* way;      // column -> the previous column on the alternating path (and the claims of the row reduction)
  int* sel;      // row -> its cheapest column, then 1 if the row still needs an augmenting path, else 0
  unsigned char* used;
};

struct SerialLanes {
  YM_HD int lane() const { return 0; }
  YM_HD int lanes() const { return 1; }
  YM_HD void sync() const {}
  YM_HD void argmin(double&, int&) const {}
  YM_HD void take_min(int* a, int v) const {
    if (v < *a) *a = v;
  }
};

// n <= m.  On return p[j] (j = 1..m) is the row matched to column j - 1, plus one.
// Start (row reduction, one row per lane): u[i] = the row's smallest weight, v = 0 — dual feasible, with v = 0 on
// every column as a column that stays free needs — and a row takes its cheapest column when no row of lower index
// claims the same one (that pair is tight).  A row without a weight below zero is left out: it could only be matched
// at weight 0, which the caller drops.  A track that overlaps only its own detection is matched here; only the rows
// that lost a claim go through the augmenting paths below.
// Paths: column j belongs to lane j % lanes: only that lane touches minv / used / v / way of the column, so the scan
// and the update of one step need no barrier between them; u is shared and a barrier follows its update.
// Returns false only if the weights were not finite.
template <class Weight, class Par>
YM_HD inline bool ym_assign_rows(int n, int m, Weight w, const Par& par, const AssignWork& ws) {
  const int ln = par.lane(), nl = par.lanes();
  const double inf = 1e300;
  for (int j = ln; j <= kTrackDim; j += nl) {
    if (j > m) break;
    ws.v[j] = 0;
    ws.p[j] = 0;
    ws.u[j] = 0;  // n <= m: covers rows 0..n
    ws.way[j] = kTrackDim + 1;  // no claim
  }
  par.sync();
  for (int i = 1 + ln; i <= kTrackDim; i += nl) {
    if (i > n) break;
    double best = inf;
    int bj = 1;
    for (int j = 1; j <= kTrackDim; ++j) {
      if (j > m) break;
      const double c = w(i - 1, j - 1);
      if (c < best) {
        best = c;
        bj = j;
      }
    }
    if (best < 0) {
      ws.u[i] = best;
      ws.sel[i] = bj;
      par.take_min(&ws.way[bj], i);
    } else {
      ws.sel[i] = 0;  // no pair under the limit: the row stays out (it could only take a column at weight 0)
    }
  }
  par.sync();
  for (int i = 1 + ln; i <= kTrackDim; i += nl) {
    if (i > n) break;
    const int bj = ws.sel[i];
    if (bj == 0) continue;
    const bool won = ws.way[bj] == i;
    if (won) ws.p[bj] = i;
    ws.sel[i] = won ? 0 : 1;
  }
  par.sync();
  bool ok = true;
  for (int i = 1; i <= kTrackDim; ++i) {
    if (i > n || !ok) break;
    if (ws.sel[i] == 0) continue;  // matched by the row reduction
    for (int j = ln; j <= kTrackDim; j += nl) {
      if (j > m) break;
      ws.minv[j] = inf;
      ws.used[j] = 0;
    }
    if (ln == 0) ws.p[0] = i;
    par.sync();
    int j0 = 0;
    for (int it = 0; it <= kTrackDim; ++it) {  // every step adds one column to the tree
      const int i0 = ws.p[j0];
      const double ui0 = ws.u[i0];
      if (j0 % nl == ln) ws.used[j0] = 1;
      double best = inf;
      int bj = -1;
      for (int j = ln; j <= kTrackDim; j += nl) {
        if (j > m) break;
        if (j == 0 || ws.used[j]) continue;
        const double cur = w(i0 - 1, j - 1) - ui0 - ws.v[j];
        if (cur < ws.minv[j]) {
          ws.minv[j] = cur;
          ws.way[j] = j0;
        }
        if (ws.minv[j] < best) {
          best = ws.minv[j];
          bj = j;
        }
      }
      par.argmin(best, bj);
      if (bj <= 0 || bj > m) {
        ok = false;
        break;
      }
      for (int j = ln; j <= kTrackDim; j += nl) {
        if (j > m) break;
        if (ws.used[j]) {
          ws.u[ws.p[j]] += best;
          ws.v[j] -= best;
        } else {
          ws.minv[j] -= best;
        }
      }
      par.sync();
      j0 = bj;
      if (ws.p[j0] == 0) break;
    }
    if (ok && ln == 0) {
      for (int it = 0; it <= kTrackDim; ++it) {
        const int j1 = ws.way[j0];
        ws.p[j0] = ws.p[j1];
        j0 = j1;
        if (j0 == 0) break;
      }
    }
    par.sync();
  }
  return ok;
}

// nr rows x nc columns of any shape; w(i, j) <= 0.  row_to_col[i] = the column matched to row i with w < 0, else -1.
template <class Weight, class Par>
YM_HD inline void ym_assign(int nr, int nc, Weight w, const Par& par, const AssignWork& ws, int* row_to_col) {
  const int ln = par.lane(), nl = par.lanes();
  for (int i = ln; i < kTrackDim; i += nl) {
    if (i >= nr) break;
    row_to_col[i] = -1;
  }
  par.sync();
  if (nr <= 0 || nc <= 0) return;
  if (nr <= nc) {
    const bool ok = ym_assign_rows(nr, nc, w, par, ws);
    for (int j = 1 + ln; j <= kTrackDim; j += nl) {
      if (j > nc || !ok) break;
      const int i = ws.p[j] - 1;
      if (i >= 0 && w(i, j - 1) < 0) row_to_col[i] = j - 1;
    }
  } else {
    const bool ok = ym_assign_rows(nc, nr, [&](int c, int r) { return w(r, c); }, par, ws);
    for (int j = 1 + ln; j <= kTrackDim; j += nl) {
      if (j > nr || !ok) break;
      const int c = ws.p[j] - 1;
      if (c >= 0 && w(j - 1, c) < 0) row_to_col[j - 1] = c;
    }
  }
  par.sync();
}

#if defined(__HIPCC__)
hipError_t ym_launch_track(const TrackArgs& a, int B, hipStream_t st);
#endif
