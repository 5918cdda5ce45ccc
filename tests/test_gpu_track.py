"""GPU tests of tracking: the ByteTrack kernel (csrc/ym_track.hip) alone on scripted detections, then model.track()
end to end, against tests/track_oracle.py.

Bars: every discrete result (ids, the detection row behind each track, counts, the tracker's state words) equals the
oracle's — tests/test_track_host.py holds the scripted scenarios' decision margin at >= 1e-4, so the kernel's fp32 IoU
cannot legitimately flip one — and every reported box is within the project's 1e-3 px of the oracle's float64 rows
(score and class are copies of the detection's fp32 values: equal)."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import track_scenarios as S
from tests.golden.make_golden import make_input
from tests.track_oracle import ByteTrackOracle

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TOL_XY = 1e-3
_cache = {}


def model(task="detect"):
    from core.model import YOLO11Model
    if task not in _cache:
        m = YOLO11Model(task=task, size="n", device="cuda:0", dtype="x3", verbose=False)
        m.model.engine.autotune = False
        _cache[task] = m
    return _cache[task]


def check_rows(got_rows, got_idx, ref_rows, ref_idx, what):
    """Ids and detection rows equal; score / class equal as fp32; boxes within TOL_XY.  Returns the largest box
    difference."""
    assert got_rows.shape[0] == ref_rows.shape[0], (what, got_rows[:, 4], ref_rows[:, 4])
    if not len(ref_rows):
        return 0.0
    assert got_rows[:, 4].astype(np.int64).tolist() == ref_rows[:, 4].astype(np.int64).tolist(), what
    assert got_idx.tolist() == ref_idx.tolist(), what
    assert np.array_equal(got_rows[:, 5:7], ref_rows[:, 5:7].astype(np.float32)), what
    d = float(np.abs(got_rows[:, :4].astype(np.float64) - ref_rows[:, :4]).max())
    assert d <= TOL_XY, (what, d)
    return d


# ------------------------------------------------------------------------------------------------ the tracker alone
@pytest.mark.parametrize("name", sorted(S.gpu_trackers()))
def test_tracker_alone(name):
    """Scripted rows straight into Runtime.track_create / Tracker.update, no forward: three streams per tracker, every
    frame against the oracle.  Rows carry four extra columns (as a pose row carries its keypoints) that must arrive
    with the track; rows behind the counts are NaN and must not be read."""
    from yolomi.lib import Runtime
    cfg, capacity, streams = S.gpu_trackers()[name]
    rt = Runtime(0, None)
    trk = rt.track_create(3, cfg, 0 if capacity == 512 else capacity)
    oracles = [ByteTrackOracle(cfg, capacity) for _ in streams]
    max_det, stride = 40, 10
    rng = np.random.default_rng(1)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    worst = 0.0
    for t in range(len(streams[0])):
        host = np.full((3, max_det, stride), np.nan, dtype=np.float32)
        counts = np.zeros((3,), dtype=np.int32)
        for b, frames in enumerate(streams):
            f = frames[t]
            counts[b] = len(f)
            host[b, : len(f), :6] = f
            host[b, : len(f), 6:] = rng.uniform(-1, 1, (len(f), stride - 6))
        dets, cnt = torch.from_numpy(host).to(DEV), torch.from_numpy(counts).to(DEV)
        tracks = torch.full((3, max_det, stride + 1), float("nan"), dtype=torch.float32, device=DEV)
        idx = torch.full((3, max_det), -7, dtype=torch.int32, device=DEV)
        tcnt = torch.full((3,), -7, dtype=torch.int32, device=DEV)
        trk.update(dets.data_ptr(), stride, 3, max_det, cnt.data_ptr(), tracks.data_ptr(), idx.data_ptr(),
                   tcnt.data_ptr(), stream)
        state = trk.read_state()
        tracks, idx, tcnt = tracks.cpu().numpy(), idx.cpu().numpy(), tcnt.cpu().tolist()
        for b, o in enumerate(oracles):
            ref_rows, ref_idx = o.update(streams[b][t])
            what = (name, "frame", t + 1, "stream", b)
            assert tcnt[b] == len(ref_rows), what
            assert state[b] == o.state(), what
            n = tcnt[b]
            worst = max(worst, check_rows(tracks[b, :n, :7], idx[b, :n], ref_rows, ref_idx, what))
            assert np.array_equal(tracks[b, :n, 7:], host[b, idx[b, :n], 6:]), what  # the extras of the feeding row
            assert np.isnan(tracks[b, n:]).all() and (idx[b, n:] == -7).all(), what  # nothing behind the count
    assert all(o.margin >= 1e-4 for o in oracles)
    print(f"tracker alone [{name}]: max |box - float64 oracle| = {worst:.3g} px")
    trk.close()
    rt.close()


def test_reset_restarts_the_streams():
    from yolomi.lib import Runtime
    rt = Runtime(0, None)
    trk = rt.track_create(1, None, 0)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    frames = S.late_start()
    for rep in range(2):
        o = ByteTrackOracle()
        for f in frames:
            dets = torch.from_numpy(f).to(DEV).contiguous()
            cnt = torch.tensor([len(f)], dtype=torch.int32, device=DEV)
            tracks = torch.zeros((1, len(f), 7), dtype=torch.float32, device=DEV)
            idx = torch.zeros((1, len(f)), dtype=torch.int32, device=DEV)
            tcnt = torch.zeros((1,), dtype=torch.int32, device=DEV)
            trk.update(dets.data_ptr(), 6, 1, len(f), cnt.data_ptr(), tracks.data_ptr(), idx.data_ptr(), tcnt.data_ptr(),
                       stream)
            ref_rows, ref_idx = o.update(f)
            n = int(tcnt.item())
            check_rows(tracks[0, :n].cpu().numpy(), idx[0, :n].cpu().numpy(), ref_rows, ref_idx, (rep, "reset"))
        assert trk.read_state() == [o.state()] and o.state()[:2] == (6, 3)
        trk.reset(stream)
        assert trk.read_state() == [(0, 1, 0, 0, 0, 0)]
    trk.close()
    rt.close()


# ------------------------------------------------------------------------------------------------ C-ABI refusals
def test_c_abi_refusals():
    from yolomi.lib import Runtime, TrackCfg, YMError, load_library
    lib = load_library()
    rt = Runtime(0, None)
    trk = rt.track_create(2, None, 0)
    d = torch.zeros((2, 300, 7), dtype=torch.float32, device=DEV)
    i = torch.zeros((2, 300), dtype=torch.int32, device=DEV)
    ptrs = [d.data_ptr(), i.data_ptr(), d.data_ptr(), i.data_ptr(), i.data_ptr()]  # dets, counts, tracks, idx, tcounts

    def update(p, B=2, max_det=300, stride=6, t=trk.trk):
        return lib.ym_track_update(t, C.c_void_p(p[0]), stride, B, max_det, C.c_void_p(p[1]), C.c_void_p(p[2]),
                                   C.c_void_p(p[3]), C.c_void_p(p[4]), None)
    assert update(ptrs) == 0
    for k in range(5):
        assert update([None if j == k else p for j, p in enumerate(ptrs)]) == -1
    assert update(ptrs, t=None) == -1
    assert update(ptrs, B=1) == -1 and update(ptrs, B=3) == -1
    assert b"streams" in lib.ym_last_error()
    assert update(ptrs, max_det=301) == -1 and update(ptrs, max_det=0) == -1
    assert update(ptrs, stride=5) == -1 and update(ptrs, stride=65) == -1
    out = C.c_void_p()
    cfg = TrackCfg(0.25, 0.1, 0.25, 0.8, 30, 1, 0, 0)
    assert lib.ym_track_create(None, 2, C.byref(cfg), C.byref(out)) == -1
    assert lib.ym_track_create(rt.ctx, 2, None, C.byref(out)) == -1
    assert lib.ym_track_create(rt.ctx, 2, C.byref(cfg), None) == -1
    assert lib.ym_track_create(rt.ctx, 0, C.byref(cfg), C.byref(out)) == -1
    for bad in (TrackCfg(1.5, 0.1, 0.25, 0.8, 30, 1, 0, 0), TrackCfg(0.25, 0.1, 0.25, 0.8, -1, 1, 0, 0),
                TrackCfg(0.25, 0.1, 0.25, 0.8, 30, 1, 513, 0), TrackCfg(float("nan"), 0.1, 0.25, 0.8, 30, 1, 0, 0)):
        assert lib.ym_track_create(rt.ctx, 2, C.byref(bad), C.byref(out)) == -1
    assert lib.ym_track_reset(None, None) == -1
    state = (C.c_int * 12)()
    assert lib.ym_track_read_state(trk.trk, state, 3) == -1 and lib.ym_track_read_state(trk.trk, None, 2) == -1
    assert lib.ym_track_read_state(trk.trk, state, 2) == 0
    with pytest.raises(YMError):
        trk.update(0, 6, 2, 300, ptrs[1], ptrs[2], ptrs[3], ptrs[4], 0)
    trk.close()
    rt.close()


# ------------------------------------------------------------------------------------------------ end to end
def frames_of(task, B=2, n=3):
    """n batches: the golden uniform input at 128 x 128, each frame the previous one rolled by (3, 2) pixels."""
    x0 = make_input("uniform", [3 + b for b in range(B)], 128)
    return [torch.roll(x0, shifts=(2 * t, 3 * t), dims=(2, 3)).contiguous().to(DEV) for t in range(n)]


@pytest.mark.parametrize("task", ["detect", "pose"])
def test_track_end_to_end(task):
    """Three track(x_t, persist=True) calls; the oracle is fed the GPU's own NMS rows of the same frames
    (predict(conf=0.1)) and must give the same ids, detection rows, boxes and state as Results.boxes — for every
    stream until one of its associations has two matchings of equal value (ByteTrackOracle.tie_seen), where the
    answer is no longer unique; the checks that do not depend on the tie-break go on."""
    m = model(task)
    xs = frames_of(task)
    B = xs[0].shape[0]
    oracles = [ByteTrackOracle() for _ in range(B)]
    total, strict, worst = 0, 0, 0.0
    for t, x in enumerate(xs):
        res = m.track(x, persist=t > 0)
        assert len(res) == B
        # asynchronous: the Results share the call's device counts, unread until first access
        from core.results import LazyCounts
        assert all(isinstance(r._n, LazyCounts) and r._n is res[0]._n for r in res)
        assert res[0]._n._host is None
        pred = m.predict(x, conf=0.1)
        assert res[0]._n._host is None
        state = None
        for b in range(B):
            rows = pred[b].boxes.data.cpu().numpy()
            ref_rows, ref_idx = oracles[b].update(rows)
            bx = res[b].boxes
            got, gidx = bx.data.cpu().numpy(), res[b].det_idx.cpu().numpy()
            assert bx.is_track and got.shape[1] == 7 and gidx.shape == (len(got),)
            if not oracles[b].tie_seen:
                # every association of this stream so far had one optimal matching: the oracle's is the answer
                worst = max(worst, check_rows(got, gidx, ref_rows, ref_idx, (task, t, b)))
                state = state or m.model.engine.tracker_state()
                assert state[b] == oracles[b].state(), (task, t, b)
                strict += 1
            else:
                # real NMS rows can give two matchings of equal value; which one a solver returns is
                # its tie-break, and the stream may differ from the oracle's from there on.  What holds either way:
                ids = got[:, 4].astype(np.int64)
                assert np.array_equal(got[:, 4], ids) and (np.diff(ids) > 0).all() and (ids >= 1).all()
                assert len(set(gidx.tolist())) == len(gidx) and ((gidx >= 0) & (gidx < len(rows))).all()
            n = len(got)
            assert bx.id.shape == (n,) and bx.id.dtype == torch.float32
            assert torch.equal(bx.conf, bx.data[:, 5]) and torch.equal(bx.cls, bx.data[:, 6])
            assert torch.equal(bx.id, bx.data[:, 4]) and bx.xyxy.shape == (n, 4)
            if n:  # score and class are the feeding detection's
                assert np.array_equal(got[:, 5:7], rows[gidx][:, 4:6])
                assert [r["track_id"] for r in res[b].summary()] == got[:, 4].astype(int).tolist()
            if task == "pose":
                k = res[b].keypoints.data
                assert k.shape == (n, 17, 3)
                assert torch.equal(k, pred[b].keypoints.data[res[b].det_idx.long()])
            else:
                assert res[b].keypoints is None
            total += n
    print(f"track end to end [{task}]: {total} track rows, {strict} of {B * len(xs)} stream-frames held to the oracle, "
          f"max |box - float64 oracle| = {worst:.3g} px, "
          f"oracle margins {[{k: float(f'{v:.3g}') for k, v in o.margins.items()} for o in oracles]}")
    assert total > 0 and strict >= B and oracles[0].state()[0] == len(xs)
    # persist=False starts over: frame 1 again, ids from 1
    res = m.track(xs[0], persist=False)
    for b in range(B):
        o = ByteTrackOracle()
        ref_rows, _ = o.update(m.predict(xs[0], conf=0.1)[b].boxes.data.cpu().numpy())
        assert res[b].boxes.id.int().tolist() == list(range(1, len(ref_rows) + 1))
    assert [s[0] for s in m.model.engine.tracker_state()] == [1] * B
    # image b is stream b: another batch size cannot continue the live tracker
    with pytest.raises(ValueError):
        m.track(xs[0][:1], persist=True)
    assert len(m.track(xs[0][:1], persist=False)) == 1
    with pytest.raises(ValueError):
        m.track(xs[0], max_det=301)
    with pytest.raises(NotImplementedError):
        m.track(xs[0], tracker="botsort.yaml")


@pytest.mark.parametrize("task", ["detect", "pose"])
def test_track_image_sources(task):
    """Two 120 x 160 uint8 BGR ndarrays (letterboxed to 128 x 160): the synchronous branch of track().  On frame 1
    every detection at or over track_high_thresh starts an activated track whose filter box is the detection's, so
    the rows are predict()'s rows of those detections in order — boxes after scale_boxes, a pose model's keypoints
    after scale_coords from column 7 — with ids 1..n in the id column."""
    from yolomi.synth import uniform
    imgs = [(uniform(8400 + i, 120 * 160 * 3) * 256).astype(np.uint8).reshape(120, 160, 3) for i in range(2)]
    m = model(task)
    res = m.track(imgs, imgsz=160, persist=False)
    pred = m.predict(imgs, imgsz=160, conf=0.1)
    assert len(res) == 2
    seen = 0
    for r, p in zip(res, pred):
        assert r.orig_shape == (120, 160) and r.orig_img.shape == (120, 160, 3)
        rows = p.boxes.data.cpu().numpy()
        keep = np.flatnonzero(rows[:, 4] >= np.float32(0.25))
        bx = r.boxes
        got = bx.data.cpu().numpy()
        assert bx.is_track and got.shape == (len(keep), 7) and bx.orig_shape == (120, 160)
        assert bx.id.int().tolist() == list(range(1, len(keep) + 1))
        assert np.array_equal(got[:, 5:7], rows[keep, 4:6])
        if len(keep):
            assert np.abs(got[:, :4].astype(np.float64) - rows[keep, :4]).max() <= TOL_XY
            assert [q["track_id"] for q in r.summary()] == list(range(1, len(keep) + 1))
        if task == "pose":
            assert r.keypoints.data.shape == (len(keep), 17, 3)
            assert torch.equal(r.keypoints.data, p.keypoints.data[torch.from_numpy(keep).to(DEV)])
        else:
            assert r.keypoints is None
        seen += len(keep)
    assert seen > 0
    again = m.track(imgs, imgsz=160, persist=True)  # the same frame again: the same tracks, matched
    for r, a in zip(res, again):
        assert a.boxes.id.tolist() == r.boxes.id.tolist()
        assert (a.boxes.xyxy - r.boxes.xyxy).abs().max().item() <= TOL_XY if len(r.boxes) else True
    assert [st[0] for st in m.model.engine.tracker_state()] == [2, 2]


def test_track_refuses_a_segment_model():
    from core.model import YOLO11Model
    m = YOLO11Model(task="segment", size="n", device="cuda:0", dtype="x3", verbose=False)
    with pytest.raises(NotImplementedError):
        m.track(torch.zeros((1, 3, 128, 128), device=DEV))
    with pytest.raises(NotImplementedError):
        m.model.engine.track(torch.zeros((1, 3, 128, 128), device=DEV))
