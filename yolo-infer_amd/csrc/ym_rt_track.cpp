// yolomi runtime, tracking: ByteTrack state of `streams` video streams in device memory; ym_track_update is one launch
// of csrc/ym_track.hip.  Of a context it uses the device only.
#include "ym_runtime.h"
#include "ym_track.h"

extern "C" {

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
  return launched(ym_launch_track(a, B, static_cast<hipStream_t>(stream)), "track kernel");
}

int ym_track_read_state(ym_tracker* t, int* state, int n_streams) {
  if (!t || !state) return fail(YM_EINVAL, "null tracker or state");
  if (n_streams < 1 || n_streams > t->streams)
    return fail(YM_EINVAL, "ym_track_read_state: %d streams of %d", n_streams, t->streams);
  std::vector<TrackHead> h(n_streams);
  if (int rc = read_back(t->device, h.data(), t->d_heads, (size_t)n_streams * sizeof(TrackHead))) return rc;
  for (int b = 0; b < n_streams; ++b) {
    int* o = state + (size_t)b * YM_TRACK_STATE_WORDS;
    o[0] = h[b].frame_id; o[1] = h[b].issued + 1; o[2] = h[b].n_tracked;
    o[3] = h[b].n_lost; o[4] = h[b].n_unconfirmed; o[5] = h[b].drops;
  }
  return YM_OK;
}

}  // extern "C"
