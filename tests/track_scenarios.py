"""Scripted detection sequences for the tracker tests (tests/test_track_host.py on the oracle, tests/test_gpu_track.py on
the kernel).  A scenario is a list of frames; a frame is an (n, 6) float32 array of NMS-like rows [x1, y1, x2, y2, conf,
cls].  Boxes are 100 x 100 unless stated.  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

from typing import List

import numpy as np

BUF3 = {"track_buffer": 3}  # the gap scenarios' tracker: max_time_lost = 3 keeps the sequences short


def det(x, y, conf=0.9, cls=0.0, w=100.0, h=100.0):
    return [x, y, x + w, y + h, conf, cls]


def frame(*rows) -> np.ndarray:
    return np.asarray(rows, dtype=np.float32).reshape(-1, 6)


def keeps_id(n=6) -> List[np.ndarray]:
    """One object drifting 3 px a frame: id 1 on every frame."""
    return [frame(det(10 + 3 * t, 20 + t, 0.9, 2)) for t in range(n)]


def late_start(n=6) -> List[np.ndarray]:
    """A from frame 1; B (other class) first seen on frame 3: B is reported from frame 4, its second match."""
    return [frame(det(0, 0, 0.8), *([det(300, 0, 0.7, 1)] if t >= 2 else [])) for t in range(n)]


def low_conf(n=6) -> List[np.ndarray]:
    """A at 0.9 for two frames, then at 0.15: the second association keeps id 1 alive.  D is at 0.15 from the start
    and never becomes a track."""
    return [frame(det(400, 400, 0.15, 3), det(0, 0, 0.9 if t < 2 else 0.15)) for t in range(n)]


def gap(absent: int, tail=3) -> List[np.ndarray]:
    """A on frames 1-2, away for `absent` frames, back for `tail`; C is always there (a frame without detections
    would not count).  With track_buffer 3: absent <= 3 re-finds id 1, absent = 4 gives id 3."""
    seq = [True, True] + [False] * absent + [True] * tail
    return [frame(*([det(0, 0, 0.9)] if a else []), det(500, 0, 0.85, 1)) for a in seq]


def crossing(n=5) -> List[np.ndarray]:
    """Tracks at x = 0 (id 1) and x = 50 (id 2); from frame 3 the detections sit at x = 30 and x = 95.  IoU x 0.9:
    id1-30 0.485, id2-30 0.6, id2-95 0.341, id1-95 0.023.  Greedy takes id2-30 first and loses id 1 (0.023 is over the
    limit); the optimum is id1-30 + id2-95."""
    out = []
    for t in range(n):
        out.append(frame(det(0, 0), det(50, 0)) if t < 2 else frame(det(95, 0), det(30, 0)))
    return out


def duplicate(n=12) -> List[np.ndarray]:
    """A moves 30 px a frame for five frames and vanishes; its lost track coasts on into B, which has stood at x = 236
    since frame 1.  When the two boxes agree to 1 - IoU < 0.15, B (seen for more frames) stays and A's track goes,
    long before track_buffer = 30 would age it out."""
    return [frame(*([det(30 * t, 0)] if t < 5 else []), det(236, 0, 0.9, 1)) for t in range(n)]


def duplicate_younger(n=17) -> List[np.ndarray]:
    """The other outcome: A stands for six frames, moves 30 px a frame for five and vanishes (seen over 10 frames); B
    has stood at x = 196 since frame 6 only.  When A's coasting track reaches B, B is the one seen for fewer frames:
    the tracked B goes, A stays lost, and B's next detection re-activates A — id 1 continues on B's object."""
    out = []
    for t in range(n):
        rows = [det(0, 0)] if t < 6 else [det(30 * (t - 5), 0)] if t < 11 else []
        out.append(frame(*rows, *([det(196, 0, 0.9, 1)] if t >= 5 else [])))
    return out


def with_empty_frames() -> List[np.ndarray]:
    """keeps_id with frames without detections in between: they do not advance the tracker."""
    e = np.zeros((0, 6), dtype=np.float32)
    k = keeps_id(5)
    return [k[0], e, k[1], e, e, k[2], k[3], e, k[4]]


def table_full() -> List[np.ndarray]:
    """For a capacity of 6: ten objects on frame 1 (6 tracks, 4 drops), again on frame 2 (+4 drops), then three of
    the tracked ones and two strangers (the table still holds three lost tracks: +2 drops), then the three alone."""
    grid = [det(150 * i, 200 * (i % 2), 0.9 - 0.01 * i, i % 3) for i in range(10)]
    return [frame(*grid), frame(*grid), frame(*grid[:3], det(0, 600), det(300, 600)), frame(*grid[:3])]


def churn(shift=0.0) -> List[np.ndarray]:
    """Forty objects at a time, three disjoint sets A, B, C: A, B, B, C, C, A, A.  By frame 6 the pool holds 80 lost
    tracks (A from frame 1, B), so A's return is a 40 x 80+ assignment with more tracks than detections — more than
    one column per lane of the kernel's wavefront, rows and columns swapped."""
    def grid(x0):
        return frame(*[det(x0 + shift + 150 * (i % 8), 150 * (i // 8), 0.9 - 0.005 * i, i % 4) for i in range(40)])
    a, b, c = grid(0.0), grid(2000.0), grid(4000.0)
    return [a, b, b, c, c, a, a]


def merged(*scenarios, dy=700.0) -> List[np.ndarray]:
    """Several scenarios in one scene, scenario k shifted down by k * dy so that they do not interact."""
    n = max(len(s) for s in scenarios)
    out = []
    for t in range(n):
        rows = []
        for k, s in enumerate(scenarios):
            if t < len(s):
                f = s[t].copy()
                f[:, [1, 3]] += k * dy
                rows.append(f)
        out.append(np.concatenate(rows, axis=0) if rows else np.zeros((0, 6), dtype=np.float32))
    return out


def gpu_trackers():
    """What tests/test_gpu_track.py replays: tracker name -> (cfg, capacity, three streams of equal length; a shorter
    stream is continued with frames without detections)."""
    def pad(streams):
        n = max(len(s) for s in streams)
        e = np.zeros((0, 6), dtype=np.float32)
        return [list(s) + [e] * (n - len(s)) for s in streams]
    return {"default": (None, 512, pad([merged(keeps_id(), late_start(), low_conf(), crossing()),
                                        merged(duplicate(), duplicate_younger()), with_empty_frames()])),
            "churn": (None, 512, pad([churn(), churn(7.0)[:5], keeps_id()])),
            "buffer0": ({"track_buffer": 0}, 512, pad([gap(1), gap(2), late_start()])),
            "buffer3_capacity6": (BUF3, 6, pad([gap(3), gap(4), table_full()]))}
