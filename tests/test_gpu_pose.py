"""GPU tests of the pose task (yolo11n-pose, nc 1, kpt_shape (17, 3)): the keypoint decode kernel (csrc/ym_kpts.hip),
the padded head layout, NMS carrying the 52 keypoint extras, and the public surface, against tests/pose_oracle.py.

Bars (the x3 plan's, tests/test_gpu_x3.py): boxes through tests/matching.py at TOL_XY 1e-3 px beyond the fp32
oracle's own distance from its float64 evaluation (ref_f64_slack), TOL_S 5e-5, and the GPU's own distance from the
float64 evaluation at TOL_EXACT_XY 5e-4; every keypoint coordinate of a matched pair within 1e-3 px plus that
element's own |fp32 oracle − float64 oracle|, every visibility within 5e-5.  The kernel itself is held bit for bit
to the fp32 formula on the GPU's own raw head output.
"""
import json
import os

import numpy as np
import pytest
import torch

from tests.golden.make_golden import make_input
from tests.matching import MatchReport, iou_matrix, match_image, ref_f64_slack
from tests.pose_oracle import PoseOracle
from tests.test_gpu_x3 import TOL_EXACT_XY, TOL_S, TOL_XY
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEV = torch.device("cuda", 0)
K, ND, NK = 17, 3, 51
_cache = {}


def oracle():
    if "o" not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _cache["o"] = PoseOracle("n", synth_weights("n", "pose", 0))
    return _cache["o"]


def model(dtype="x3"):
    """The heuristic tile configurations (no on-device tuning of the test shapes: tuned tables for pose are out of
    scope); test_public_surface runs the default, tuning constructor."""
    from core.model import YOLO11Model
    if ("m", dtype) not in _cache:
        m = YOLO11Model(task="pose", size="n", device="cuda:0", dtype=dtype, verbose=False)
        m.model.engine.autotune = False
        _cache[("m", dtype)] = m
    return _cache[("m", dtype)]


def golden():
    g = json.load(open(os.path.join(GOLD, "pose_n_uniform.json")))
    return g, make_input(g["input"]["kind"], g["input"]["seeds"], g["input"]["size"])


def reference(x, conf=0.25, iou=0.7, orig_shape=None):
    """(fp32 oracle, float64 oracle) per-image dicts, computed once per input."""
    key = ("ref", x.shape, float(x.sum()), conf, iou, orig_shape)
    if key not in _cache:
        _cache[key] = (oracle().predict(x, conf, iou, orig_shape=orig_shape),
                       oracle().predict_exact(x, conf, iou, orig_shape=orig_shape))
    return _cache[key]


def run_rows(m, x, shape=None, **kw):
    """Device rows of eng.run as per-image (n, 6 + 51) arrays: boxes as the NMS kernel clips them, keypoints clipped
    to the image on the host (scale_coords with equal shapes; the Keypoints masking not applied)."""
    eng = m.model.engine
    dets, counts = eng.run(x.to(DEV), **kw)
    H, W = shape or x.shape[2:]
    out = []
    for b, n in enumerate(counts[: x.shape[0]].tolist()):
        r = dets[b, :n, : 6 + NK].cpu().clone()
        k = r[:, 6:].view(n, K, ND)
        k[..., 0].clamp_(0, W)
        k[..., 1].clamp_(0, H)
        out.append(r.numpy())
    return out


def _exact_rows(ref, exact):
    """For each fp32-oracle row its float64 counterpart (same class, IoU >= 0.99, nearest), or -1."""
    idx = np.full(len(ref), -1)
    if len(ref) and len(exact):
        ious = iou_matrix(ref[:, :4], exact[:, :4])
        for i in range(len(ref)):
            cand = np.where((exact[:, 5] == ref[i, 5]) & (ious[i] >= 0.99))[0]
            if len(cand):
                idx[i] = cand[np.abs(exact[cand, :4] - ref[i, :4]).max(1).argmin()]
    return idx


def check_pose(refs, exacts, got_rows, conf=0.25, iou=0.7, max_det=300, tol_xy=TOL_XY, tol_s=TOL_S, tol_k=TOL_XY,
               tol_v=TOL_S, min_frac=1.0):
    """Boxes exactly as tests/test_gpu_x3.py check(); then the keypoints of every matched pair."""
    rep, rex = MatchReport(), MatchReport()
    worst_k = worst_v = 0.0
    total = 0
    for r, e, got in zip(refs, exacts, got_rows):
        ref = r["boxes"].numpy()
        ex = e["boxes"].numpy()
        total += len(ref)
        rk = r["kpts_raw"].numpy().astype(np.float64)
        ek = e["kpts_raw"].numpy()
        tol = ref_f64_slack(ref, ex, tol_xy) if min_frac >= 1.0 else tol_xy
        one = MatchReport()
        match_image(ref, got[:, :6], conf, iou, tol, tol_s, rep=one, max_det=max_det)
        if min_frac >= 1.0:
            match_image(ex, got[:, :6].astype(np.float64), conf, iou, TOL_EXACT_XY, tol_s, rep=rex, max_det=max_det)
        ei = _exact_rows(ref, ex)
        for i, j in one.pairs:
            gk = got[j, 6:].reshape(K, ND).astype(np.float64)
            slack = np.abs(rk[i] - ek[ei[i]])[:, :2] if ei[i] >= 0 else 0.0
            dk = np.abs(gk[:, :2] - rk[i][:, :2])
            dv = np.abs(gk[:, 2] - rk[i][:, 2])
            worst_k, worst_v = max(worst_k, float((dk - slack).max())), max(worst_v, float(dv.max()))
            assert (dk <= tol_k + slack).all(), f"keypoint xy off by {dk.max():.3g} (slack {np.max(slack):.3g})"
            assert (dv <= tol_v).all(), f"keypoint visibility off by {dv.max():.3g}"
        for f in ("matched", "exempt", "unmatched_ref", "unmatched_build"):
            setattr(rep, f, getattr(rep, f) + getattr(one, f))
        rep.max_dxy, rep.max_dscore = max(rep.max_dxy, one.max_dxy), max(rep.max_dscore, one.max_dscore)
        rep.failures += one.failures
    print(f"pose parity: {rep}; GPU vs float64: {rex}; keypoints: max |dxy| beyond the oracle's own error "
          f"{worst_k:.3g}, max |dv| {worst_v:.3g}")
    assert rep.matched > 0
    if min_frac >= 1.0:
        assert rep.ok, f"{rep}; {rep.failures[:3]}"
        assert rex.ok and rex.matched > 0, f"GPU vs float64: {rex}; {rex.failures[:3]}"
    else:
        assert rep.matched + rep.exempt >= min_frac * total, f"{rep}; {rep.failures[:3]}"
    return rep


def _grid(anchors: torch.Tensor, H: int, W: int):
    """(grid x, grid y, stride) as fp32 tensors for anchor indices of an H x W input (make_anchors − 0.5)."""
    gx, gy, st = torch.empty(len(anchors)), torch.empty(len(anchors)), torch.empty(len(anchors))
    off = 0
    for s in (8, 16, 32):
        h, w = H // s, W // s
        m = (anchors >= off) & (anchors < off + h * w)
        p = anchors[m] - off
        gx[m], gy[m], st[m] = (p % w).float(), (p // w).float(), float(s)
        off += h * w
    return gx, gy, st


def test_kpts_kernel_bit_exact_on_the_gpus_own_raw_output():
    g, x = golden()
    eng = model().model.engine
    dets, counts = eng.run(x.to(DEV), conf=g["conf"], iou=g["iou"], use_graph=False)
    kept = counts[:2].tolist()
    A = 2100
    gr = eng.graph
    raw = eng.read_buffer(gr.anchor_buf.id, 2).reshape(2, A, gr.anchor_buf.C)
    assert gr.anchor_buf.C == 120 and gr.kpt_off == 68 and eng.nm == 52 and eng.nk == NK and eng.kpt_shape == (K, ND)
    cands = eng.candidates(2, 320, 320)
    rows = eng.keypoint_rows(2, 320, 320)
    # the raw head rows are as the convs wrote them (the kernel writes its own buffer): the keypoint columns match
    # the oracle's raw cv4 output on every anchor — candidates' rows included, where decoded values would be pixels
    _, _, ex = oracle().raw(x)
    ref_raw = ex["kpt"].transpose(1, 2)  # (B, A, 51)
    assert (raw[..., 68:119] - ref_raw).abs().max().item() / ref_raw.abs().max().item() < 1e-4
    assert not raw[..., 65:68].any() and not raw[..., 119].any()  # pad channels: zero weights and bias
    for b in range(2):
        idx = cands[b]
        assert len(idx) >= kept[b] >= 5 and len(set(idx.tolist())) == len(idx) and int(idx.max()) < A
        assert (raw[b, idx, 68:119] - ref_raw[b, idx]).abs().max().item() / ref_raw.abs().max().item() < 1e-4
        r = raw[b, idx, 68:119].reshape(len(idx), K, ND)
        gx, gy, st = _grid(idx, 320, 320)
        got = rows[b, idx]
        gk = got[:, :NK].reshape(len(idx), K, ND)
        want_x = (r[..., 0] * 2.0 + gx[:, None]) * st[:, None]
        want_y = (r[..., 1] * 2.0 + gy[:, None]) * st[:, None]
        assert torch.equal(gk[..., 0], want_x) and torch.equal(gk[..., 1], want_y)
        dv = (gk[..., 2] - torch.sigmoid(r[..., 2])).abs().max().item()
        print(f"image {b}: {len(idx)} candidates, {kept[b]} kept, max |dv| {dv:.3g}")
        assert dv <= TOL_S
        assert not got[:, NK:].any()  # the pad column
        # the NMS rows carry exactly those decoded rows
        out = dets[b, : kept[b]].cpu()
        assert not out[:, 6 + NK:].any()
        pool = {tuple(v.tolist()) for v in got}
        assert all(tuple(v.tolist()) in pool for v in out[:, 6:])


@pytest.mark.parametrize("case", ["golden_320_b2", "640_b1"])
def test_x3_pose_matches_oracle(case):
    if case == "golden_320_b2":
        g, x = golden()
        refs, exacts = reference(x)
        for r, rows in zip(refs, g["nms_rows"]):  # the committed rows are what the restatement gives here
            rows = np.asarray(rows, np.float32).reshape(-1, 6 + NK)
            assert len(rows) == len(r["boxes"]) and np.allclose(rows[:, :6], r["boxes"].numpy(), atol=2e-3)
    else:
        x = make_input("uniform", (8201,), 640)
        refs, exacts = reference(x)
    check_pose(refs, exacts, run_rows(model(), x))


def test_x3_pose_low_conf_many_candidates():
    """conf 0.05 at 640²: thousands of candidates (the blocked NMS path and the presort), rows 58 floats wide."""
    x = make_input("uniform", (8201,), 640)
    refs, exacts = reference(x, conf=0.05)
    check_pose(refs, exacts, run_rows(model(), x, conf=0.05), conf=0.05)
    cands = model().model.engine.candidates(1, 640, 640)
    assert len(cands[0]) > 4096


def test_pose_graph_replay_equals_eager():
    """Two consecutive different batches through one captured graph (the second a replay): rows and counts bitwise
    equal to eager runs — a replay that skipped the keypoint kernel would emit the first batch's stale rows."""
    eng = model().model.engine
    xs = [make_input("uniform", (8101, 8102), 320), make_input("uniform", (8103, 8104), 320)]
    xin = torch.empty_like(xs[0], device=DEV)
    graph, eager = [], []
    for x in xs:
        xin.copy_(x)
        d, c = eng.run(xin, use_graph=True)
        graph.append((d.clone(), c.clone()))
    for x in xs:
        xin.copy_(x)
        d, c = eng.run(xin, use_graph=False)
        eager.append((d.clone(), c.clone()))
    assert not torch.equal(graph[0][1], graph[1][1]) or not torch.equal(graph[0][0], graph[1][0])
    for (gd, gc), (ed, ec) in zip(graph, eager):
        assert torch.equal(gc[:2], ec[:2]) and min(gc[:2].tolist()) >= 5
        for b, n in enumerate(gc[:2].tolist()):
            assert torch.equal(gd[b, :n], ed[b, :n])


def test_f16_pose_plan():
    """The f16 throughput plan at the bar of tests/test_gpu_parity.py test_f16_plan_matches_golden: 1 px / 1e-2 with
    >= 90 % of the oracle's detections matched or exempt; keypoints of the matches at the same 1 px / 1e-2."""
    g, x = golden()
    refs, exacts = reference(x)
    check_pose(refs, exacts, run_rows(model("f16"), x), tol_xy=1.0, tol_s=1e-2, tol_k=1.0, tol_v=1e-2, min_frac=0.9)
    x = make_input("uniform", (8201,), 640)
    refs, exacts = reference(x)
    check_pose(refs, exacts, run_rows(model("f16"), x), tol_xy=1.0, tol_s=1e-2, tol_k=1.0, tol_v=1e-2, min_frac=0.9)


def _check_results(res, refs, exacts, shape):
    """Public Results against the oracle's predict: boxes by the matching protocol, keypoints of the matches as the
    Keypoints view shows them (xy zeroed below visibility 0.5; elements within 5e-5 of 0.5 may fall either way)."""
    H, W = shape
    for r, ref, ex in zip(res, refs, exacts):
        n = len(r.boxes)
        k = r.keypoints
        assert k.data.shape == (n, K, ND) and k.xy.shape == (n, K, 2) and k.conf.shape == (n, K) and k.has_visible
        assert k.orig_shape == (H, W) and len(k) == n
        kd = k.data.cpu()
        assert (kd[..., 0] >= 0).all() and (kd[..., 0] <= W).all() and (kd[..., 1] >= 0).all() and (kd[..., 1] <= H).all()
        assert not kd[..., :2][kd[..., 2] < 0.5].any()
        assert torch.allclose(k.xyn.cpu(), kd[..., :2] / torch.tensor([W, H], dtype=torch.float32))
        rb, eb = ref["boxes"].numpy(), ex["boxes"].numpy()
        one = MatchReport()
        match_image(rb, r.boxes.data.cpu().numpy(), 0.25, 0.7, ref_f64_slack(rb, eb, TOL_XY), TOL_S, rep=one)
        assert one.ok and one.matched > 0, f"{one}; {one.failures[:3]}"
        ei = _exact_rows(rb, eb)
        rk, rm, ek = ref["kpts_raw"].numpy(), ref["keypoints"].numpy(), ex["kpts_raw"].numpy()
        for i, j in one.pairs:
            g = kd[j].numpy().astype(np.float64)
            assert np.abs(g[:, 2] - rk[i][:, 2]).max() <= TOL_S
            slack = np.abs(rk[i].astype(np.float64) - ek[ei[i]])[:, :2] if ei[i] >= 0 else 0.0
            sure = np.abs(rk[i][:, 2] - 0.5) > TOL_S
            assert (np.abs(g[:, :2] - rm[i][:, :2]) <= TOL_XY + slack)[sure].all()


def test_public_surface_tensor_source():
    from core.model import YOLO11Factory
    g, x = golden()
    m = YOLO11Factory.create_pose_estimator("n", device="cuda:0", verbose=False)
    assert m.task == "pose" and m.model.names == {0: "person"}
    res = m.predict(x.to(DEV))
    assert len(res) == 2 and res[0].masks is None
    refs, exacts = reference(x)
    _check_results(res, refs, exacts, (320, 320))
    assert len(res[0].keypoints) == len(refs[0]["boxes"])


def test_public_surface_image_source():
    """One 240x320 uint8 BGR ndarray: letterboxed on the GPU (to 256x320), keypoints and boxes mapped back with
    scale_coords / scale_boxes, against the oracle run on the same letterboxed tensor."""
    from yolomi.preprocess import letterbox_batch
    from yolomi.synth import uniform
    img = (uniform(8301, 240 * 320 * 3) * 256).astype(np.uint8).reshape(240, 320, 3)
    m = model()
    res = m.predict(img, imgsz=320)
    xl, shapes = letterbox_batch(m.model.engine.rt, [img], DEV, imgsz=320)
    torch.cuda.synchronize()
    assert tuple(xl.shape) == (1, 3, 256, 320) and tuple(shapes[0]) == (240, 320)
    refs, exacts = reference(xl.cpu(), orig_shape=(240, 320))
    assert res[0].orig_shape == (240, 320) and len(refs[0]["boxes"]) >= 3
    _check_results(res, refs, exacts, (240, 320))


def test_capi_detect_context_refuses_a_pose_blob():
    from yolomi.lib import Runtime, YMError
    from yolomi.plan import pack_model
    blob = pack_model("n", "pose", synth_weights("n", "pose", 0), "x3")
    with pytest.raises(YMError, match="EBLOB.*blob task pose, context created for detect"):
        Runtime(0, blob, scale="n", task="detect", dtype="x3")
    rt = Runtime(0, blob, scale="n", task="pose", dtype="x3")
    assert rt.kpt_shape() == (17, 3)
    rt.close()
    det_blob = pack_model("n", "detect", synth_weights("n", "detect", 0), "x3")
    det = Runtime(0, det_blob, task="detect")
    assert det.kpt_shape() == (0, 0)
    det.close()
    with pytest.raises(YMError, match="blob task detect, context created for pose"):
        Runtime(0, det_blob, task="pose")
