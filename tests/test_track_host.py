"""Host tests of the tracker: known-answer scenarios on the numpy oracle (tests/track_oracle.py), the decision margin of
the scenarios the GPU test replays, the host build of the kernel's shared header (tests/track_check.cpp: the
assignment against scipy, the Kalman filter against the oracle's), and the facade's refusals that need no GPU."""
import os
import subprocess

import numpy as np
import pytest
from scipy.optimize import linear_sum_assignment

from tests import track_scenarios as S
from tests.test_plan_format import _compiler
from tests.track_oracle import (ByteTrackOracle, assign, assign_gap, iou_matrix, kf_initiate, kf_predict, kf_update,
                                mean_to_xyxy)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def play(frames, cfg=None, capacity=512):
    """[(ids, idx, rows, state)] per frame, and the oracle."""
    o = ByteTrackOracle(cfg, capacity)
    out = []
    for f in frames:
        rows, idx = o.update(f)
        out.append((rows[:, 4].astype(int).tolist(), idx.tolist(), rows, o.state()))
    return out, o


# ------------------------------------------------------------------------------------------------ scenarios
def test_keeps_id():
    out, o = play(S.keeps_id())
    assert [ids for ids, *_ in out] == [[1]] * 6
    assert out[-1][3] == (6, 2, 1, 0, 0, 0)
    # the filter follows the drift: the reported box lies between the previous box and the detection
    assert 10 + 3 * 4 < out[-1][2][0, 0] <= 10 + 3 * 5
    assert out[-1][2][0, 5] == pytest.approx(0.9) and out[-1][2][0, 6] == 2


def test_late_track_is_reported_from_its_second_match():
    out, _ = play(S.late_start())
    assert [ids for ids, *_ in out] == [[1], [1], [1], [1, 2], [1, 2], [1, 2]]
    assert out[2][3][4] == 1 and out[3][3][4] == 0  # unconfirmed on frame 3, activated on frame 4
    assert out[3][1] == [0, 1]


def test_low_confidence_keeps_a_track_but_starts_none():
    out, o = play(S.low_conf())
    assert [ids for ids, *_ in out] == [[1]] * 6
    assert [idx for _, idx, *_ in out] == [[1]] * 6  # row 1 is A; D (row 0) never becomes a track
    assert out[-1][2][0, 5] == pytest.approx(0.15)
    assert o.state()[1] == 2 and o.state()[3] == 0


def test_gap_within_the_buffer_refinds_the_id():
    out, _ = play(S.gap(3), S.BUF3)
    ids = [i for i, *_ in out]
    assert ids[:2] == [[1, 2]] * 2 and ids[2:5] == [[2]] * 3 and ids[5:] == [[1, 2]] * 3
    assert out[4][3][3] == 1  # still lost on frame 5


def test_longer_gap_gives_a_new_id():
    out, _ = play(S.gap(4), S.BUF3)
    ids = [i for i, *_ in out]
    assert ids[5] == [2] and out[5][3][3] == 0  # aged out on frame 6: 6 - 2 > 3
    assert ids[6] == [2] and out[6][3][4] == 1  # back on frame 7: a new, unconfirmed track
    assert ids[7] == [2, 3] and ids[8] == [2, 3]


def test_crossing_takes_the_optimal_assignment_not_the_greedy_one():
    frames = S.crossing()
    out, _ = play(frames)
    assert out[2][0] == [1, 2] and out[2][1] == [1, 0]  # id 1 -> the box at x = 30 (row 1), id 2 -> x = 95 (row 0)
    # what a greedy matcher would do with frame 3's costs
    boxes = np.array([[0, 0, 100, 100], [50, 0, 150, 100]], dtype=np.float64)
    cost = 1.0 - iou_matrix(boxes, frames[2][:, :4]) * 0.9
    i, j = np.unravel_index(np.argmin(cost), cost.shape)
    assert (i, j) == (1, 1) and cost[0, 0] > 0.8  # greedy pairs id 2 with x = 30 first; id 1 is then left over the limit
    assert sorted(assign(cost, 0.8)[0]) == [(0, 1), (1, 0)]


def test_duplicate_removal_keeps_the_older_track():
    out, o = play(S.duplicate())
    lost = [st[3] for *_, st in out]
    assert lost[4] == 0 and lost[5] == 1  # A is lost from frame 6 on
    gone = lost.index(0, 5)               # ... and removed as B's duplicate on this frame (0-based)
    assert gone + 1 - 5 < 30              # not aged out: track_buffer is 30
    assert all(ids == [2] for ids, *_ in out[5:]) and o.state()[1] == 3  # B keeps id 2; nothing new was started


def test_duplicate_removal_drops_the_tracked_one_when_it_is_younger():
    out, o = play(S.duplicate_younger())
    k = next(t for t in range(11, len(out)) if out[t][0] == [])  # the frame on which B was dropped as the duplicate
    assert out[k - 1][0] == [2] and out[k - 1][3][2:5] == (1, 1, 0)
    assert out[k][3][2:5] == (0, 1, 0)   # the tracked B is gone; A is still lost
    assert out[k + 1][0] == [1] and out[k + 1][3][2:5] == (1, 0, 0)  # B's next detection re-activates A
    assert o.state()[1] == 3


def test_a_track_lost_in_this_frame_is_not_aged_out_in_it():
    """track_buffer 0: upstream ages out over the lost list of the frame's start, so a track that has just been lost
    stays lost for that frame; its detection on the next frame re-finds it, and only a second frame away removes it."""
    out, _ = play(S.gap(1), {"track_buffer": 0})
    assert out[2][0] == [2] and out[2][3][3] == 1     # frame 3: lost, still there
    assert out[3][0] == [1, 2] and out[3][3][3] == 0  # frame 4: re-found, id 1
    out, _ = play(S.gap(2), {"track_buffer": 0})
    assert out[2][3][3] == 1 and out[3][3][3] == 0    # frame 4: 4 - 2 > 0, removed
    assert out[4][0] == [2] and out[5][0] == [2, 3]   # back on frame 5 as a new track, reported from frame 6


def test_frames_without_detections_do_not_advance():
    out, o = play(S.with_empty_frames())
    ref, _ = play(S.keeps_id(5))
    got = [x for x in out if x[0]]
    assert len(got) == 5 and o.state()[0] == 5
    for a, b in zip(got, ref):
        assert a[0] == b[0] and np.array_equal(a[2], b[2])


def test_table_full_drops_and_counts():
    out, _ = play(S.table_full(), capacity=6)
    assert [st for *_, st in out] == [(1, 7, 6, 0, 0, 4), (2, 7, 6, 0, 0, 8), (3, 7, 3, 3, 0, 10), (4, 7, 3, 3, 0, 10)]


def test_gpu_scenarios_have_a_wide_decision_margin():
    """tests/test_gpu_track.py asks the kernel (fp32 IoU) for the oracle's (float64) discrete decisions: legitimate
    only if no decision of these scenarios is closer than 1e-4 — 100x the fp32 IoU rounding — to flipping."""
    for name, (cfg, capacity, streams) in S.gpu_trackers().items():
        assert len(streams) == 3
        for frames in streams:
            assert len(frames) <= 20 and max(len(f) for f in frames) <= 40
            _, o = play(frames, cfg, capacity)
            assert o.margin >= 1e-4, (name, o.margin)


# ------------------------------------------------------------------------------------------------ track_check
@pytest.fixture(scope="session")
def track_check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    exe = tmp_path_factory.mktemp("track_check") / "track_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "track_check.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # no sanitizer runtimes: a plain build
        subprocess.run(cmd, check=True)

    def run(mode, text):
        p = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True, timeout=120)
        assert p.stderr == "", p.stderr  # the sanitizers stay silent
        assert p.returncode == 0, p.stdout
        return p.stdout
    return run


def _problems():
    rng = np.random.default_rng(11)
    out = [(np.zeros((0, 4)), 0.8), (np.zeros((4, 0)), 0.8), (np.array([[0.3]]), 0.8), (np.array([[0.9]]), 0.8)]
    for shape in ((7, 3), (3, 7), (40, 40), (40, 40), (12, 25), (25, 12)):
        out.append((rng.uniform(0.0, 1.0, shape), 0.8))
    out.append((rng.uniform(0.0, 1.0, (40, 40)), 0.3))  # sparse: most pairs over the limit
    out.append((rng.uniform(0.81, 1.0, (7, 5)), 0.8))   # every cost over the limit
    dup = rng.uniform(0.0, 0.7, (3, 6))
    out.append((np.concatenate([dup, dup[:2]], axis=0), 0.8))    # duplicate rows: the optimum is not unique
    out.append((np.concatenate([dup, dup[:2]], axis=0).T, 0.8))  # duplicate columns
    out.append((np.round(rng.uniform(0.0, 1.0, (9, 9)), 1), 0.5))  # many ties
    for _ in range(40):  # small random shapes and limits: contested columns, rows with no pair under the limit
        shape = tuple(int(v) for v in rng.integers(1, 14, 2))
        out.append((rng.uniform(0.0, 1.0, shape) ** float(rng.uniform(0.3, 3.0)), float(rng.uniform(0.2, 0.9))))
    return out


def test_assignment_matches_scipy(track_check):
    probs = _problems()
    text = "".join(f"{c.shape[0]} {c.shape[1]} {lim!r}\n" + " ".join(repr(float(v)) for v in c.reshape(-1)) + "\n"
                   for c, lim in probs)
    lines = track_check("assign", text).strip().splitlines()
    assert len(lines) == len(probs)
    for (cost, lim), line in zip(probs, lines):
        v = [int(t) for t in line.split()]
        pairs = list(zip(v[1::2], v[2::2]))
        assert v[0] == len(pairs)
        assert len({i for i, _ in pairs}) == len(pairs) == len({j for _, j in pairs})  # a matching
        assert all(cost[i, j] < lim for i, j in pairs)
        ref, best = assign(cost, lim)
        assert sum(cost[i, j] - lim for i, j in pairs) == pytest.approx(best, abs=1e-9)
        if cost.size and assign_gap(cost, lim) > 1e-9:  # the optimum is unique: the same pairs
            assert sorted(pairs) == sorted(ref)
    assert lines[0] == "0" and lines[1] == "0" and lines[2] == "1 0 0" and lines[3] == "0"
    assert lines[11] == "0"


def test_kalman_matches_the_oracle(track_check):
    rng = np.random.default_rng(5)
    steps, ref = [], []
    z = np.array([320.0, 240.0, 0.5, 180.0])
    steps.append("I " + " ".join(repr(float(v)) for v in z))
    mean, cov = kf_initiate(z)
    ref.append((mean, cov))
    for t in range(40):
        if t in (17, 18, 19):  # a lost spell: predictions only, the height velocity zeroed first
            steps.append("Z")
            mean = mean.copy()
            mean[7] = 0.0
            ref.append((mean, cov))
        steps.append("P")
        mean, cov = kf_predict(mean, cov)
        ref.append((mean, cov))
        if t not in (17, 18, 19):
            z = z + np.array([4.0, -2.5, 0.002, 1.5]) + rng.normal(0, [1.5, 1.5, 0.005, 1.0])
            steps.append("U " + " ".join(repr(float(v)) for v in z))
            mean, cov = kf_update(mean, cov, z)
            ref.append((mean, cov))
    lines = track_check("kalman", "\n".join(steps) + "\n").strip().splitlines()
    assert len(lines) == len(ref)
    for line, (mean, cov) in zip(lines, ref):
        v = np.array([float(t) for t in line.split()])
        # 1e-12 relative, element by element; an entry that is exactly 0 in the oracle must be exactly 0
        assert np.allclose(v[:8], mean, rtol=1e-12, atol=0.0), np.abs(v[:8] - mean).max()
        assert np.allclose(v[8:].reshape(8, 8), cov, rtol=1e-12, atol=0.0), np.abs(v[8:].reshape(8, 8) - cov).max()
    assert np.all(np.isfinite(mean_to_xyxy(mean)))


def test_iou_is_upstreams_fp32_bbox_ioa(track_check):
    rng = np.random.default_rng(3)
    a = rng.uniform(0, 400, (50, 2)).astype(np.float32)
    b = a + rng.uniform(-60, 60, (50, 2)).astype(np.float32)
    boxes = np.concatenate([a, a + rng.uniform(20, 200, (50, 2)).astype(np.float32),
                            b, b + rng.uniform(20, 200, (50, 2)).astype(np.float32)], axis=1)
    out = track_check("iou", "".join(" ".join(repr(float(v)) for v in r) + "\n" for r in boxes))
    got = np.array([float(t) for t in out.split()])
    ref = np.array([iou_matrix(r[:4], r[4:])[0, 0] for r in boxes])
    assert np.abs(got - ref).max() < 5e-7  # fp32 arithmetic against float64


def test_header_is_plain_cxx():
    src = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "ym_track.h")).read()
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cmath>"]


# ------------------------------------------------------------------------------------------------ facade, no GPU
def test_tracker_config():
    from yolomi.track import tracker_config
    d = tracker_config("bytetrack.yaml")
    assert d == {"track_high_thresh": 0.25, "track_low_thresh": 0.1, "new_track_thresh": 0.25, "track_buffer": 30,
                 "match_thresh": 0.8, "fuse_score": True}
    assert tracker_config("bytetrack") == d and tracker_config(None) == d
    assert tracker_config({"track_buffer": 3, "tracker_type": "bytetrack"})["track_buffer"] == 3
    for bad in ({"gmc_method": "sparseOptFlow"}, {"track_high_thresh": 1.5}, {"track_buffer": -1}, "sort.yaml",
                {"tracker_type": "deepsort"}):
        with pytest.raises(ValueError):
            tracker_config(bad)
    for bot in ("botsort.yaml", "botsort", {"tracker_type": "botsort", "gmc_method": "sparseOptFlow"}):
        with pytest.raises(NotImplementedError):
            tracker_config(bot)


def test_tracker_config_from_a_yaml_file(tmp_path):
    from yolomi.track import tracker_config
    p = tmp_path / "mytrack.yaml"
    p.write_text("tracker_type: bytetrack # ByteTrack\ntrack_high_thresh: 0.3\ntrack_buffer: 12\nfuse_score: False\n")
    d = tracker_config(str(p))
    assert d["track_high_thresh"] == 0.3 and d["track_buffer"] == 12 and d["fuse_score"] is False
    assert d["match_thresh"] == 0.8
    p.write_text("tracker_type: botsort\n")
    with pytest.raises(NotImplementedError):
        tracker_config(p)


def test_facade_refuses_before_it_needs_a_gpu():
    from core.model import YOLO11Model
    m = YOLO11Model.__new__(YOLO11Model)  # no engine: the refusals below come first
    m.task = "detect"
    with pytest.raises(NotImplementedError):
        m.track(None, tracker="botsort.yaml")
    with pytest.raises(ValueError):
        m.track(None, tracker={"no_such_key": 1})
    m.task = "segment"
    with pytest.raises(NotImplementedError):
        m.track(None)


def test_boxes_tracked_columns():
    import torch
    from core.results import Boxes, Results
    six = torch.tensor([[1.0, 2, 3, 4, 0.5, 7]])
    seven = torch.tensor([[1.0, 2, 3, 4, 9, 0.5, 7], [5.0, 6, 7, 8, 11, 0.25, 3]])
    b6, b7 = Boxes(six, (10, 10)), Boxes(seven, (10, 10))
    assert not b6.is_track and b6.id is None and b6.conf.tolist() == [0.5] and b6.cls.tolist() == [7]
    assert b7.is_track and b7.id.tolist() == [9, 11] and b7.conf.tolist() == [0.5, 0.25] and b7.cls.tolist() == [7, 3]
    assert b7.xyxy.shape == (2, 4)
    names = {3: "c3", 7: "c7"}
    s = Results(None, names, seven).summary()
    assert [r["track_id"] for r in s] == [9, 11] and s[1]["class"] == 3 and s[1]["confidence"] == 0.25
    assert "track_id" not in Results(None, names, six).summary()[0]
