"""GPU tests of pose validation (MI355X): `YOLO11Model.val` / `YOLO11Validator.validate` on a pose model end to end,
and the rows `Engine.run` returns at the validator's settings (conf 0.001, multi_label=True: the single-label NMS on
a one-class plan) against tests/pose_oracle.py.

yolo11n-pose, synthetic weights seed 0, the x3 plan with the heuristic tiles, as tests/test_gpu_pose.py.  The bars of
the rows test are that file's (check_pose as test_x3_pose_low_conf_many_candidates calls it); the end-to-end numbers
are compared bit for bit with metrics.evaluate_pose of a loop written out by hand.
"""
import os

import numpy as np
import pytest
import torch

from tests.pose_oracle import PoseOracle
from tests.test_gpu_pose import check_pose, run_rows
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
K, ND, NK = 17, 3, 51
SHAPES = [(96, 128), (128, 96), (128, 128), (64, 128)]
IMGSZ, BATCH = 128, 2
_cache = {}


def model():
    from core.model import YOLO11Model
    if "m" not in _cache:
        m = YOLO11Model(task="pose", size="n", device="cuda:0", dtype="x3", verbose=False)
        m.model.engine.autotune = False
        _cache["m"] = m
    return _cache["m"]


def _write_images(root):
    from PIL import Image
    rng = np.random.default_rng(5)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "labels"), exist_ok=True)
    imgs = []
    for i, (h, w) in enumerate(SHAPES):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(os.path.join(root, "images", f"im{i}.png"))
        imgs.append(np.ascontiguousarray(rgb[..., ::-1]))
    return imgs


def _native_rows(eng, V, imgs, batches, **kw):
    """Per image (boxes (n, 6), keypoints (n, K, 3)) in native pixels of Engine.run on the val batches."""
    out = [None] * len(imgs)
    for b in batches:
        x = V.make_batch(eng, [imgs[i] for i in b["indices"]], b)
        d, c = eng.run(x, **kw)
        d, c = d.cpu().numpy(), c.tolist()
        for k, i in enumerate(b["indices"]):
            out[i] = (V.to_native(d[k, :c[k], :6], b["geo"][k], b["gain"][k], SHAPES[i]),
                      V.kpts_to_native(d[k, :c[k], 6:6 + NK].reshape(c[k], K, ND), b["geo"][k], b["gain"][k],
                                       SHAPES[i]))
    return out


def dataset(tmp_path_factory):
    """The dataset of the end-to-end tests, written once: labels = the model's own conf-0.25 rows in native pixels,
    every keypoint labelled (v = 2)."""
    if "ds" not in _cache:
        from yolomi import val as V
        root = str(tmp_path_factory.mktemp("pose_val") / "ds")
        imgs = _write_images(root)
        batches = V.build_batches(SHAPES, IMGSZ, BATCH)
        n_labels = 0
        for i, (r, kn) in enumerate(_native_rows(model().model.engine, V, imgs, batches, conf=0.25)):
            h0, w0 = SHAPES[i]
            with open(os.path.join(root, "labels", f"im{i}.txt"), "w") as f:
                for (x1, y1, x2, y2, _, cl), kk in zip(r, kn):
                    v = [(x1 + x2) / 2 / w0, (y1 + y2) / 2 / h0, (x2 - x1) / w0, (y2 - y1) / h0]
                    for x, y, _ in kk:
                        v += [x / w0, y / h0, 2]
                    f.write(f"{int(cl)} " + " ".join(repr(float(t)) for t in v) + "\n")
                    n_labels += 1
        _cache["ds"] = (root, imgs, batches, n_labels)
    return _cache["ds"]


def test_pose_val_end_to_end(tmp_path_factory, tmp_path):
    """Every label is one of the model's own detections, so val() must find it again with its box (IoU >= 0.5) and its
    keypoints (OKS >= 0.5); the ten numbers val() returns are metrics.evaluate_pose of the same loop written out here.
    No mAP of ~1 is asserted: with the fp32 oracle in the GPU's place this dataset gives pose AP 0.995 but box AP 0.958,
    because boxes clipped to the 64 x 128 image coincide and upstream's tie rule then drops a true positive
    (tests/test_pose_val_host.py)."""
    from core.validator import YOLO11Validator
    from yolomi import val as V
    from yolomi.metrics import OKS_SIGMA, box_iou, evaluate_pose, kpt_iou
    root, imgs, batches, n_labels = dataset(tmp_path_factory)
    assert n_labels >= 1, "the model detects nothing at conf 0.25 on these images"
    m = model()
    res = m.val(data=root, imgsz=IMGSZ, batch=BATCH)
    # the same loop by hand
    ds = V.load_dataset(root, kpt_shape=(K, ND))
    assert sum(len(lb) for lb in ds.labels) == n_labels and all(lb.shape[1] == 5 + NK for lb in ds.labels)
    rows = _native_rows(m.model.engine, V, imgs, batches, conf=0.001, iou=0.7, max_det=300, multi_label=True)
    preds, pk = [r[0] for r in rows], [r[1] for r in rows]
    gts = [V.labels_to_native(lb[:, :5], s) for lb, s in zip(ds.labels, SHAPES)]
    gk = [V.label_kpts_to_native(lb, s, K) for lb, s in zip(ds.labels, SHAPES)]
    for p, g, a, c in zip(preds, gts, pk, gk):
        assert len(p) < 300  # under max_det: nothing was cut
        iou = box_iou(g[:, :4], p[:, :4]) * (g[:, None, 5] == p[None, :, 5])
        assert len(g) == 0 or (iou.max(1) >= 0.5).all(), "a label's box is not matched by any prediction"
        oks = kpt_iou(c, a, (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) * 0.53, OKS_SIGMA)
        assert len(g) == 0 or (oks.max(1) >= 0.5).all(), "a label's keypoints are not matched by any prediction"
    want = evaluate_pose(preds, gts, pk, gk, OKS_SIGMA)
    print(f"pose val: {n_labels} labels, predictions {[len(p) for p in preds]}, {want}")
    for got, w in ((res.box, want["box"]), (res.pose, want["pose"])):
        assert (got.map50, got.map75, got.map, got.mp, got.mr) == (w["map50"], w["map75"], w["map"], w["precision"],
                                                                    w["recall"])
    assert res.pose.map50 > 0 and res.box.map50 > 0
    assert res.n_images == 4 and res.n_labels == n_labels
    assert {"preprocess", "inference", "postprocess"} <= set(res.speed)
    assert res.results_dict["metrics/mAP50-95(P)"] == res.pose.map
    assert res.results_dict["metrics/mAP50-95(B)"] == res.box.map
    assert res.results_dict["fitness"] == (0.1 * res.box.map50 + 0.9 * res.box.map) + (0.1 * res.pose.map50
                                                                                        + 0.9 * res.pose.map)
    # collect: the keypoint arrays come along
    from yolomi.val import run_val
    got = []
    run_val(m.model.engine, root, imgsz=IMGSZ, batch=BATCH, collect=got)
    assert len(got) == 4 and all(len(t) == 4 for t in got)
    for (p, g, a, c), p0, a0, c0 in zip(got, preds, pk, gk):
        assert np.array_equal(p, p0) and np.array_equal(a, a0) and np.array_equal(c, c0) and a.shape[1:] == (K, ND)
    v = YOLO11Validator(m, device="cuda:0", output_dir=str(tmp_path / "val_out"))
    out = v.validate(root, imgsz=IMGSZ, batch=BATCH, conf=0.001, iou=0.7)
    assert {"timestamp", "validation_time_seconds", "device", "model_info", "box_metrics", "pose_metrics",
            "speed_metrics"} <= set(out)
    assert set(out["pose_metrics"]) == {"mAP50-95", "mAP50", "mAP75", "precision", "recall"}
    assert out["pose_metrics"]["mAP50"] == want["pose"]["map50"] and out["box_metrics"]["mAP50"] == want["box"]["map50"]
    assert out["pose_metrics"]["mAP50-95"] == want["pose"]["map"]
    assert "Pose Metrics:" in (tmp_path / "val_out" / "validation_summary.txt").read_text()


def test_rows_at_the_validators_settings_match_the_oracle(tmp_path_factory):
    """The 160 x 160 rect batch of that dataset (A = 525) through Engine.run(conf=0.001, multi_label=True): boxes and
    keypoints against the fp32 and float64 oracle at the bars of tests/test_gpu_pose.py's low-conf case."""
    from yolomi import val as V
    _, imgs, batches, _ = dataset(tmp_path_factory)
    b = batches[1]
    assert b["shape"] == (160, 160) and b["indices"] == [2, 1]
    m = model()
    x = V.make_batch(m.model.engine, [imgs[i] for i in b["indices"]], b).cpu()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    orc = PoseOracle("n", synth_weights("n", "pose", 0))
    refs, exacts = orc.predict(x, 0.001, 0.7), orc.predict_exact(x, 0.001, 0.7)
    rows = run_rows(m, x, conf=0.001, multi_label=True)
    assert all(len(r["boxes"]) >= 20 for r in refs) and all(0 < len(r) < 300 for r in rows)
    check_pose(refs, exacts, rows, conf=0.001)


def test_val_augment_on_a_pose_model_is_the_single_scale_val(tmp_path_factory, caplog):
    import logging
    root = dataset(tmp_path_factory)[0]
    m = model()
    plain = m.val(data=root, imgsz=IMGSZ, batch=BATCH)
    with caplog.at_level(logging.WARNING, logger="yolomi.val"):
        aug = m.val(data=root, imgsz=IMGSZ, batch=BATCH, augment=True)
    assert aug.results_dict == plain.results_dict and aug.pose.map75 == plain.pose.map75
    assert any("augment=True" in r.getMessage() for r in caplog.records)
    with pytest.raises(ValueError, match="detect plans"):  # the augmented run itself refuses a pose plan
        m.model.engine.run_tta(torch.zeros((1, 3, 32, 32), device=DEV), conf=0.25)


def test_run_val_on_a_segment_engine_still_raises(tmp_path_factory):
    from core.model import YOLO11Model
    from yolomi.val import run_val
    root = dataset(tmp_path_factory)[0]
    seg = YOLO11Model(task="segment", size="n", device="cuda:0", dtype="f32", verbose=False)
    with pytest.raises(NotImplementedError, match="segment"):
        run_val(seg.model.engine, root, imgsz=IMGSZ, batch=BATCH)
    with pytest.raises(NotImplementedError, match="segment"):
        seg.val(data=root, imgsz=IMGSZ, batch=BATCH)
