"""CPU restatement of Ultralytics ByteTrack (8.3.x: trackers/byte_tracker.py BYTETracker.update and STrack,
trackers/utils/kalman_filter.py KalmanFilterXYAH, trackers/utils/matching.py linear_assignment / iou_distance /
fuse_score, with trackers/cfg/bytetrack.yaml's defaults), in numpy float64.  TEST INFRASTRUCTURE ONLY.

One `update(dets)` per frame, dets = (n, >= 6) rows [x1, y1, x2, y2, conf, cls, ...] in NMS order:

    frame_id += 1
    high = conf >= track_high_thresh; second = track_low_thresh < conf < track_high_thresh
    pool = activated tracked + lost; Kalman predict every pool track (mean[7] = 0 first unless Tracked)
    1. pool x high, cost 1 - IoU * conf (fuse_score), limit match_thresh: Tracked -> update, Lost -> re_activate
    2. unmatched Tracked pool rows x second, cost 1 - IoU, limit 0.5 -> update; still unmatched -> Lost
    3. unconfirmed x high left by 1, cost as 1, limit 0.7 -> update; unmatched -> removed
    tracks lost before this frame with frame_id - end_frame > max_time_lost -> removed
    remaining high with conf >= new_track_thresh -> new tracks in row order (is_activated only on frame 1)
    duplicates: tracked x lost with 1 - IoU < 0.15: the one with the smaller end_frame - start_frame goes, the
        tracked one on a tie
    output: activated tracked tracks, [xyxy of the filter mean, id, score, cls] and the detection row that fed each

The assignment is lap.lapjv(cost, extend_cost=True, cost_limit=limit): the partial matching maximising the sum of
(limit - cost) over its pairs; here scipy.optimize.linear_sum_assignment on min(cost - limit, 0), keeping cost < limit.

Where this restatement (and the kernel, csrc/ym_track.hip) departs from upstream, DESIGN.md §16 lists it: ids count
from 1 per tracker, rows in ascending id order, an aged-out lost track leaves at once, detection boxes enter as their
fp32 corners (upstream round-trips them through fp32 xywh / tlwh), a capacity bounds the live tracks.

`margin` is the smallest decision margin met so far: the minimum over |cost - limit| of every pair of every
association, the gap between the best and the second-best assignment value, |conf - threshold| of every detection
against the three score thresholds, and |1 - IoU - 0.15| of every duplicate candidate.  A run whose margin is well above
fp32 rounding has no discrete decision that a float32 IoU could flip.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import numpy as np
from scipy.linalg import cho_factor, cho_solve
from scipy.optimize import linear_sum_assignment

DEFAULT_CFG = {"track_high_thresh": 0.25, "track_low_thresh": 0.1, "new_track_thresh": 0.25, "track_buffer": 30,
               "match_thresh": 0.8, "fuse_score": True}
W_POS, W_VEL = 1.0 / 20, 1.0 / 160
TRACKED, LOST = 1, 2

_F = np.eye(8)
for _i in range(4):
    _F[_i, 4 + _i] = 1.0
_H = np.eye(4, 8)


def kf_initiate(z: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    mean = np.r_[np.asarray(z, dtype=np.float64), np.zeros(4)]
    h = z[3]
    std = [2 * W_POS * h, 2 * W_POS * h, 1e-2, 2 * W_POS * h, 10 * W_VEL * h, 10 * W_VEL * h, 1e-5, 10 * W_VEL * h]
    return mean, np.diag(np.square(std))


def kf_predict(mean: np.ndarray, cov: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    h = mean[3]
    std = [W_POS * h, W_POS * h, 1e-2, W_POS * h, W_VEL * h, W_VEL * h, 1e-5, W_VEL * h]
    return _F @ mean, _F @ cov @ _F.T + np.diag(np.square(std))


def kf_update(mean: np.ndarray, cov: np.ndarray, z: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    h = mean[3]
    std = [W_POS * h, W_POS * h, 1e-1, W_POS * h]
    pm = _H @ mean
    S = _H @ cov @ _H.T + np.diag(np.square(std))
    K = cho_solve(cho_factor(S, lower=True, check_finite=False), (cov @ _H.T).T, check_finite=False).T
    return mean + (np.asarray(z, dtype=np.float64) - pm) @ K.T, cov - K @ S @ K.T


def xyxy_to_xyah(b: np.ndarray) -> np.ndarray:
    w, h = b[2] - b[0], b[3] - b[1]
    return np.array([b[0] + w / 2, b[1] + h / 2, w / h, h])


def mean_to_xyxy(mean: np.ndarray) -> np.ndarray:
    w, h = mean[2] * mean[3], mean[3]
    x1, y1 = mean[0] - w / 2, mean[1] - h / 2
    return np.array([x1, y1, x1 + w, y1 + h])


def iou_matrix(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """bbox_ioa(a, b, iou=True), eps 1e-7, in float64."""
    a, b = np.asarray(a, dtype=np.float64).reshape(-1, 4), np.asarray(b, dtype=np.float64).reshape(-1, 4)
    iw = (np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])).clip(0)
    ih = (np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])).clip(0)
    inter = iw * ih
    area = ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))[None, :] + ((a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]))[:, None] - inter
    return inter / (area + 1e-7)


def assign(cost: np.ndarray, limit: float) -> Tuple[List[Tuple[int, int]], float]:
    """(pairs (row, col) with cost < limit of the optimal partial matching, its value sum(cost - limit) <= 0)."""
    cost = np.asarray(cost, dtype=np.float64)
    if cost.size == 0:
        return [], 0.0
    w = np.minimum(cost - limit, 0.0)
    r, c = linear_sum_assignment(w)
    pairs = [(int(i), int(j)) for i, j in zip(r, c) if cost[i, j] < limit]
    return pairs, float(sum(w[i, j] for i, j in pairs))


def assign_gap(cost: np.ndarray, limit: float) -> float:
    """Value of the best matching that differs from the optimum, minus the optimum's (inf when nothing is matched):
    any other matching lacks one of the optimum's pairs, so each pair is ruled out in turn."""
    cost = np.asarray(cost, dtype=np.float64)
    pairs, best = assign(cost, limit)
    gap = np.inf
    for i, j in pairs:
        c2 = cost.copy()
        c2[i, j] = limit  # weight 0: choosing the pair is now the same as leaving both unmatched
        gap = min(gap, assign(c2, limit)[1] - best)
    return gap


class Track:
    __slots__ = ("mean", "cov", "state", "id", "score", "cls", "start_frame", "end_frame", "tracklet_len",
                 "is_activated", "idx")

    def xyxy(self):
        return mean_to_xyxy(self.mean)


class ByteTrackOracle:
    def __init__(self, cfg: Optional[Dict] = None, capacity: int = 512):
        self.cfg = dict(DEFAULT_CFG, **(cfg or {}))
        self.capacity = capacity
        self.max_time_lost = int(self.cfg["track_buffer"])
        self.margin = np.inf
        self.margins: Dict[str, float] = {}  # the same, by kind of decision
        self.reset()

    def reset(self):
        self.frame_id, self.next_id, self.drops = 0, 1, 0
        self.tie_seen = False  # some association so far had two optimal matchings
        self.tracked: List[Track] = []
        self.lost: List[Track] = []

    def _note(self, values, what):
        values = np.asarray(values, dtype=np.float64).reshape(-1)
        if values.size:
            m = float(np.abs(values).min())
            self.margin = min(self.margin, m)
            self.margins[what] = min(self.margins.get(what, np.inf), m)

    def _dists(self, tracks, boxes, conf, fuse, limit):
        cost = 1.0 - iou_matrix([t.xyxy() for t in tracks], boxes)
        if fuse and cost.size:
            cost = 1.0 - (1.0 - cost) * conf[None, :]
        pairs, _ = assign(cost, limit)
        if cost.size:
            self._note(cost - limit, "cost limit")
            gap = assign_gap(cost, limit)
            self._note(gap, "assignment gap")
            if gap <= 1e-9:  # a second matching of equal value: which one a solver returns is its tie-break
                self.tie_seen = True
        mt, md = {i for i, _ in pairs}, {j for _, j in pairs}
        return pairs, [i for i in range(len(tracks)) if i not in mt], [j for j in range(len(boxes)) if j not in md]

    def _take(self, t: Track, det, j: int):
        t.mean, t.cov = kf_update(t.mean, t.cov, xyxy_to_xyah(det[:4]))
        t.tracklet_len = t.tracklet_len + 1 if t.state == TRACKED else 0
        t.state, t.is_activated, t.end_frame = TRACKED, True, self.frame_id
        t.score, t.cls, t.idx = float(det[4]), float(det[5]), int(j)

    def update(self, dets: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """dets: (n, >= 6).  Returns ((k, 7) float64 rows [x1, y1, x2, y2, id, score, cls], (k,) detection rows).
        A frame without detections changes nothing and returns no rows (upstream's predictor callback skips it)."""
        if len(dets) == 0:
            return np.zeros((0, 7)), np.zeros((0,), dtype=np.int64)
        dets = np.asarray(dets, dtype=np.float32).astype(np.float64).reshape(len(dets), -1)
        c = self.cfg
        self.frame_id += 1
        conf = dets[:, 4]
        high_t, low_t = float(np.float32(c["track_high_thresh"])), float(np.float32(c["track_low_thresh"]))
        new_t = float(np.float32(c["new_track_thresh"]))
        self._note(np.r_[conf - high_t, conf - low_t, conf - new_t], "score threshold")
        hi = np.flatnonzero(conf >= high_t)
        sec = np.flatnonzero((conf > low_t) & (conf < high_t))

        unconfirmed = [t for t in self.tracked if not t.is_activated]
        pool = [t for t in self.tracked if t.is_activated] + self.lost
        was_lost = {id(t) for t in self.lost}  # upstream ages out over the lost list of the frame's start
        for t in pool:
            if t.state != TRACKED:
                t.mean[7] = 0.0
            t.mean, t.cov = kf_predict(t.mean, t.cov)
        # 1
        pairs, u_track, u_det = self._dists(pool, dets[hi, :4], conf[hi], c["fuse_score"], c["match_thresh"])
        for i, j in pairs:
            self._take(pool[i], dets[hi[j]], hi[j])
        # 2
        rest = [pool[i] for i in u_track if pool[i].state == TRACKED]
        pairs, u_rest, _ = self._dists(rest, dets[sec, :4], conf[sec], False, 0.5)
        for i, j in pairs:
            self._take(rest[i], dets[sec[j]], sec[j])
        for i in u_rest:
            rest[i].state = LOST
        # 3
        hi3 = hi[u_det]
        pairs, u_unc, u_det3 = self._dists(unconfirmed, dets[hi3, :4], conf[hi3], c["fuse_score"], 0.7)
        for i, j in pairs:
            self._take(unconfirmed[i], dets[hi3[j]], hi3[j])
        removed = {id(unconfirmed[i]) for i in u_unc}
        # age out
        everyone = [t for t in self.tracked + self.lost if id(t) not in removed]
        everyone = [t for t in everyone if not (id(t) in was_lost and t.state == LOST
                                                and self.frame_id - t.end_frame > self.max_time_lost)]
        # new tracks
        for j in hi3[u_det3]:
            if conf[j] < new_t:
                continue
            if len(everyone) >= self.capacity:
                self.drops += 1
                continue
            t = Track()
            t.mean, t.cov = kf_initiate(xyxy_to_xyah(dets[j, :4]))
            t.state, t.id, t.score, t.cls, t.idx = TRACKED, self.next_id, float(conf[j]), float(dets[j, 5]), int(j)
            t.start_frame = t.end_frame = self.frame_id
            t.tracklet_len, t.is_activated = 0, self.frame_id == 1
            self.next_id += 1
            everyone.append(t)
        tracked = [t for t in everyone if t.state == TRACKED]
        lost = [t for t in everyone if t.state == LOST]
        # duplicates
        drop = set()
        if tracked and lost:
            pd = 1.0 - iou_matrix([t.xyxy() for t in tracked], [t.xyxy() for t in lost])
            self._note(pd - float(np.float32(0.15)), "duplicate distance")
            for p, q in zip(*np.where(pd < float(np.float32(0.15)))):
                tp, tq = tracked[p], lost[q]
                drop.add(id(tq) if tp.end_frame - tp.start_frame > tq.end_frame - tq.start_frame else id(tp))
        self.tracked = [t for t in tracked if id(t) not in drop]
        self.lost = [t for t in lost if id(t) not in drop]
        out = sorted((t for t in self.tracked if t.is_activated), key=lambda t: t.id)
        rows = np.array([np.r_[t.xyxy(), t.id, t.score, t.cls] for t in out], dtype=np.float64).reshape(-1, 7)
        return rows, np.array([t.idx for t in out], dtype=np.int64)

    def state(self) -> Tuple[int, int, int, int, int, int]:
        """(frame_id, next id, activated tracked, lost, unconfirmed, drops): what ym_track_read_state reports."""
        act = sum(1 for t in self.tracked if t.is_activated)
        return self.frame_id, self.next_id, act, len(self.lost), len(self.tracked) - act, self.drops
