"""GPU tests of validation mode (MI355X): `Engine.run(multi_label=True)` (csrc/ym_nms_ml.hip: every (anchor, class) pair
above conf a candidate, exact top-max_nms selection, sort, NMS) against the CPU restatement tests/val_oracle.py of
Ultralytics `non_max_suppression(multi_label=True)`, and `YOLO11Model.val` / `YOLO11Validator.validate` end to end.

Parity protocol: tests/matching.py at the bars of test_gpu_parity.test_nms_paths_f32 (1e-3 px, 1e-3 score) for the f32
plan; no unmatched detection on either side and at most 2 % of the reference's detections exempt.  The x3 case uses
the x3 parity tests' bars (1e-3 px beyond the fp32 oracle's own distance from its float64 evaluation, 5e-5 score).
Inputs: yolo11n synthetic weights, 320x320 U[0,1) images, so one image has ~168 k pairs at conf 0.001 (almost every
(anchor, class) pair: A * nc = 2,100 * 80) and ~2.3 k at 0.05.
"""
import copy
import os

import numpy as np
import pytest
import torch

from oracle.predict import OracleModel
from tests.golden.make_golden import make_input
from tests.matching import MatchReport, match_image, ref_f64_slack
from tests.val_oracle import multi_label_nms
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S = 320
SEEDS2 = (1, 2)
SEEDS8 = tuple(range(1, 9))

_cache = {}


def oracle():
    if "o" not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _cache["o"] = OracleModel("n", "detect", synth_weights("n", "detect", 0))
    return _cache["o"]


def model(dtype="f32", task="detect"):
    from core.model import YOLO11Model
    k = ("m", dtype, task)
    if k not in _cache:
        _cache[k] = YOLO11Model(task=task, size="n", device="cuda:0", dtype=dtype, verbose=False)
    return _cache[k]


def head(seeds):
    """(input, the oracle's fp32 head output (B, 84, A)) of the shared inputs: computed once per seed tuple."""
    k = ("y", seeds)
    if k not in _cache:
        x = make_input("uniform", seeds, S)
        _, y, _ = oracle().raw(x)
        _cache[k] = (x, y)
    return _cache[k]


def head64(seeds):
    k = ("y64", seeds)
    if k not in _cache:
        om = oracle()
        if getattr(om, "_net64", None) is None:
            om._net64 = copy.deepcopy(om.net).double()
        with torch.no_grad():
            _cache[k] = om._net64(head(seeds)[0].double())[0][0]
    return _cache[k]


def run_ml(eng, x, **kw):
    """(rows per image, kept counts, pair counts) of one multi-label run."""
    B = x.shape[0]
    dets, counts = eng.run(x.to(DEV), multi_label=True, **kw)
    torch.cuda.synchronize()
    n = counts[:B].tolist()
    rows = dets[:B].cpu().numpy()
    return [rows[b, :n[b]].copy() for b in range(B)], n, eng.candidate_counts(B)


def parity(eng, seeds, conf, max_nms, max_det, tol_xy_fn=None, tol_s=1e-3, xy=None, **kw):
    x, y = xy if xy is not None else head(seeds)
    ref_counts = []
    ref = multi_label_nms(y, conf=conf, iou=0.7, max_det=max_det, max_nms=max_nms, img_shape=(S, S),
                          counts=ref_counts, **kw)
    got, n, pairs = run_ml(eng, x, conf=conf, iou=0.7, max_det=max_det, max_nms=max_nms, **kw)
    rep = MatchReport()
    for b in range(len(ref)):
        tol = tol_xy_fn(b, ref[b]) if tol_xy_fn else 1e-3
        match_image(ref[b], got[b], conf, 0.7, tol, tol_s, rep=rep, max_det=max_det)
    total = sum(len(r) for r in ref)
    print(f"multi-label conf={conf} max_nms={max_nms} max_det={max_det} {kw}: pairs gpu {pairs} oracle {ref_counts}; "
          f"kept gpu {n} oracle {[len(r) for r in ref]}; {rep}")
    assert rep.ok, f"{rep}; {rep.failures[:3]}"
    assert rep.matched > 0 and rep.exempt <= 0.02 * total, rep
    return pairs, n


# ------------------------------------------------------------------------------------------------ oracle parity
def test_ml_few_dozen_pairs():
    pairs, _ = parity(model().model.engine, SEEDS2, 0.25, 30000, 300)
    assert all(0 < p <= 512 for p in pairs), pairs


def test_ml_untruncated_max_det_1024():
    pairs, n = parity(model().model.engine, SEEDS2, 0.05, 30000, 1024)
    assert all(1024 < p <= 30000 for p in pairs), pairs  # no cut; more than one sort chunk is not needed here
    assert all(k > 512 for k in n), n  # beyond nms_image's kept-list size: the multi-label kernel's own


def test_ml_truncated_at_small_max_nms():
    pairs, n = parity(model().model.engine, SEEDS2, 0.05, 200, 300)
    assert all(p > 200 for p in pairs) and all(k <= 200 for k in n), (pairs, n)


def test_ml_validator_conf_full_selection():
    """conf 0.001: ~168 k pairs per image, so the radix select cuts to 30,000, 15 sort chunks are merged and the NMS
    scans 30,000 candidates."""
    pairs, _ = parity(model().model.engine, SEEDS2, 0.001, 30000, 1024)
    assert all(p > 30000 for p in pairs), pairs


def test_ml_agnostic():
    pairs, _ = parity(model().model.engine, SEEDS2, 0.05, 30000, 300, agnostic=True)
    assert all(p > 300 for p in pairs), pairs


def test_ml_small_max_wh():
    """max_wh 64 < the image: boxes of different classes intersect, the class shortcut must be off."""
    pairs, _ = parity(model().model.engine, SEEDS2, 0.05, 30000, 300, max_wh=64.0)
    assert all(p > 300 for p in pairs), pairs


def test_ml_classes_filter():
    pairs, _ = parity(model().model.engine, SEEDS2, 0.05, 30000, 300, classes=[0, 17, 45, 79])
    full = model().model.engine
    _, _, all_pairs = run_ml(full, head(SEEDS2)[0], conf=0.05, max_det=300)
    assert all(0 < p < q for p, q in zip(pairs, all_pairs)), (pairs, all_pairs)


def test_ml_one_class_low_conf():
    pairs, _ = parity(model().model.engine, SEEDS2, 0.01, 30000, 1024, classes=[3])
    assert all(0 < p <= 2100 for p in pairs), pairs  # at most one pair per anchor


def test_ml_b8_default_lanes():
    pairs, _ = parity(model().model.engine, SEEDS8, 0.05, 30000, 300)
    assert len(pairs) == 8 and all(p > 300 for p in pairs), pairs


def test_ml_x3_plan():
    y64 = head64(SEEDS2)
    exact = multi_label_nms(y64, conf=0.05, iou=0.7, max_det=300, max_nms=30000, img_shape=(S, S))
    pairs, _ = parity(model("x3").model.engine, SEEDS2, 0.05, 30000, 300,
                      tol_xy_fn=lambda b, ref: ref_f64_slack(ref, exact[b], 1e-3), tol_s=5e-5)
    assert all(p > 300 for p in pairs), pairs


def test_ml_equal_scores_at_the_cut():
    """Class head with zero weights: every anchor's logit for class c is the bias, one of 4 values shared by 20 classes,
    so 42,000 pairs per image have each score.  The cut (30,000, then 777) falls inside the best score's group and
    must take its first pairs in (anchor, class) order — the index digits of the radix select, which distinct scores
    never reach.  A wrong tie order keeps other boxes: unmatched, or exempt beyond the 2 % bound (all scores are equal,
    so the max_det exemption would cover them)."""
    from core.model import YOLO11Model
    sd = dict(synth_weights("n", "detect", 0))
    for l in range(3):
        sd[f"model.23.cv3.{l}.2.weight"] = np.zeros_like(sd[f"model.23.cv3.{l}.2.weight"])
        sd[f"model.23.cv3.{l}.2.bias"] = (-2.0 + 0.25 * (np.arange(80) % 4)).astype(np.float32)
    x = head(SEEDS2)[0][:1]
    _, y, _ = OracleModel("n", "detect", sd).raw(x)
    assert len(np.unique(y[0, 4:].numpy())) <= 8  # (4 values; an ulp of slack for the oracle's conv arithmetic)
    eng = YOLO11Model(task="detect", size="n", device="cuda:0", dtype="f32", verbose=False, state_dict=sd).model.engine
    for max_nms in (30000, 777):
        pairs, n = parity(eng, None, 0.001, max_nms, 300, xy=(x, y))
        assert pairs == [2100 * 80] and n[0] > 20, (pairs, n)


# ------------------------------------------------------------------------------------------------ exact properties
def test_ml_equals_single_label_where_they_coincide():
    """conf just above the largest second-best class score of any anchor: every candidate anchor has exactly one class
    above conf, so both modes see the same candidates and must give bit-identical rows."""
    eng = model().model.engine
    x = head(SEEDS2)[0].to(DEV)
    eng.run(x, conf=0.25)
    B = 2
    no = eng.graph.anchor_buf.C
    h = eng.read_buffer(eng.graph.anchor_buf.id, B).reshape(B, -1, no)
    sc = torch.sigmoid(h[..., 64:64 + 80])
    top2 = sc.topk(2, dim=-1).values
    conf = float(np.nextafter(np.float32(top2[..., 1].max().item()), np.float32(1.0))) + 1e-6
    assert int((top2[..., 0] > conf).sum()) >= 3, "the inputs leave fewer than 3 single-class anchors"
    d0, c0 = eng.run(x, conf=conf, max_det=300)
    d0, c0 = d0.clone(), c0.clone()
    d1, c1 = eng.run(x, conf=conf, max_det=300, multi_label=True)
    assert c0[:B].tolist() == c1[:B].tolist() and min(c0[:B].tolist()) >= 1
    for b in range(B):
        assert torch.equal(d0[b, :int(c0[b])], d1[b, :int(c1[b])])


def test_ml_deterministic():
    eng = model().model.engine
    x0 = head(SEEDS2)[0][:1]
    x = torch.cat([x0, x0])
    r1, n1, p1 = run_ml(eng, x, conf=0.001, max_det=1024)
    assert p1[0] == p1[1] > 30000 and n1[0] == n1[1] > 0
    assert np.array_equal(r1[0], r1[1])
    r2, n2, p2 = run_ml(eng, x, conf=0.001, max_det=1024)
    assert n2 == n1 and p2 == p1 and np.array_equal(r2[0], r1[0]) and np.array_equal(r2[1], r1[1])


def test_ml_cut_at_the_pair_count():
    """max_nms = n (the cut falls exactly on the last candidate) and n + 1 (no cut) select the same keys."""
    eng = model().model.engine
    x = head(SEEDS2)[0][:1]
    _, _, pairs = run_ml(eng, x, conf=0.05, max_det=300)
    n = pairs[0]
    assert 300 < n < 30000
    ra, na, pa = run_ml(eng, x, conf=0.05, max_det=300, max_nms=n)
    rb, nb, pb = run_ml(eng, x, conf=0.05, max_det=300, max_nms=n + 1)
    assert pa == pb == [n] and na == nb and np.array_equal(ra[0], rb[0])
    rc, nc_, _ = run_ml(eng, x, conf=0.05, max_det=300, max_nms=n - 1)  # one candidate less: the lowest key is cut
    assert nc_[0] <= na[0]


def test_ml_lanes_bitwise_equal():
    eng = model().model.engine
    x = head(SEEDS2)[0]
    r1, n1, p1 = run_ml(eng, x, conf=0.05, max_det=300, lanes=1)
    r2, n2, p2 = run_ml(eng, x, conf=0.05, max_det=300, lanes=2)
    assert n1 == n2 and p1 == p2 and all(np.array_equal(a, b) for a, b in zip(r1, r2))


# ------------------------------------------------------------------------------------------------ defaults, rejections
def test_default_path_unchanged_by_the_argument():
    eng = model().model.engine
    x = head(SEEDS2)[0].to(DEV)
    d0, c0 = eng.run(x, conf=0.05)
    d0, c0 = d0.clone(), c0.clone()
    d1, c1 = eng.run(x, conf=0.05, multi_label=False)
    assert torch.equal(c0, c1) and torch.equal(d0, d1)


def test_multi_label_rejections():
    from yolomi.lib import YMError
    x = head(SEEDS2)[0].to(DEV)
    with pytest.raises(YMError, match="EINVAL"):
        model().model.engine.run(x, conf=0.05, multi_label=2)
    with pytest.raises(YMError, match="EINVAL"):
        model("f32", "segment").model.engine.run(x, conf=0.05, multi_label=True)


def test_multi_label_on_a_one_class_plan_is_the_single_label_path():
    eng = model("f32", "pose").model.engine  # nc 1: upstream's multi_label &= nc > 1
    x = head(SEEDS2)[0].to(DEV)
    d0, c0 = eng.run(x, conf=0.05)
    d0, c0 = d0.clone(), c0.clone()
    d1, c1 = eng.run(x, conf=0.05, multi_label=True)
    assert torch.equal(c0, c1) and torch.equal(d0, d1)


# ------------------------------------------------------------------------------------------------ end to end
def _write_dataset(root, shapes, seed=5):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "labels"), exist_ok=True)
    imgs = []
    for i, (h, w) in enumerate(shapes):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(os.path.join(root, "images", f"im{i}.png"))
        imgs.append(np.ascontiguousarray(rgb[..., ::-1]))
    return imgs


def _plain_forward_ok(eng, x, conf):
    """The single-label forward of this batch against the oracle (the f32 plan's parity bars)."""
    ref = oracle().predict(x.cpu(), conf=conf)
    d, c = eng.run(x, conf=conf)
    rep = MatchReport()
    for b, r in enumerate(ref):
        match_image(r["boxes"].numpy(), d[b, :int(c[b])].cpu().numpy(), conf, 0.7, 1e-3, 1e-3, rep=rep)
    return rep.ok, rep


def test_val_end_to_end(tmp_path):
    """Labels = the model's own single-label detections at conf 0.25 on the val batches, so every label must be found
    again by val(); the returned mAPs must be metrics.evaluate of Engine.run(multi_label=True) on the same batches."""
    from core.validator import YOLO11Validator
    from yolomi import val as V
    from yolomi.metrics import box_iou, evaluate
    m = model()
    eng = m.model.engine
    for shapes, imgsz in (([(96, 128), (128, 96), (128, 128), (64, 128)], 128), ([(320, 320)] * 4, 320)):
        root = str(tmp_path / f"ds{imgsz}")
        imgs = _write_dataset(root, shapes)
        batches = V.build_batches(shapes, imgsz, 2)
        why = None
        for b in batches:
            x = V.make_batch(eng, [imgs[i] for i in b["indices"]], b)
            ok, rep = _plain_forward_ok(eng, x, 0.25)
            if not ok:
                why = f"plain forward differs from the oracle at batch shape {b['shape']}: {rep}"
        if why is None:
            break
        print(f"imgsz {imgsz} dataset left out: {why}")  # the all-320 images are the fallback
    assert why is None, why
    n_labels = 0
    for b in batches:
        x = V.make_batch(eng, [imgs[i] for i in b["indices"]], b)
        d, c = eng.run(x, conf=0.25)
        d, c = d.cpu().numpy(), c.tolist()
        for k, i in enumerate(b["indices"]):
            h0, w0 = shapes[i]
            r = V.to_native(d[k, :c[k], :6], b["geo"][k], b["gain"][k], shapes[i])
            with open(os.path.join(root, "labels", f"im{i}.txt"), "w") as f:
                for x1, y1, x2, y2, _, cl in r:
                    v = [(x1 + x2) / 2 / w0, (y1 + y2) / 2 / h0, (x2 - x1) / w0, (y2 - y1) / h0]
                    f.write(f"{int(cl)} " + " ".join(repr(float(t)) for t in v) + "\n")
                    n_labels += 1
    assert n_labels >= 1, "the model detects nothing at conf 0.25 on these images"
    res = m.val(data=root, imgsz=imgsz, batch=2)
    # the same loop by hand
    ds = V.load_dataset(root)
    preds, gts = [None] * len(ds), [None] * len(ds)
    for b in batches:
        x = V.make_batch(eng, [imgs[i] for i in b["indices"]], b)
        d, c = eng.run(x, conf=0.001, iou=0.7, max_det=300, multi_label=True)
        d, c = d.cpu().numpy(), c.tolist()
        for k, i in enumerate(b["indices"]):
            preds[i] = V.to_native(d[k, :c[k], :6], b["geo"][k], b["gain"][k], shapes[i])
            gts[i] = V.labels_to_native(ds.labels[i], shapes[i])
    for p, g in zip(preds, gts):
        iou = box_iou(g[:, :4], p[:, :4]) * (g[:, None, 5] == p[None, :, 5])
        assert len(g) == 0 or (iou.max(1) >= 0.5).all(), "a label is not matched by any prediction of its class"
    want = evaluate(preds, gts)
    assert (res.box.map50, res.box.map75, res.box.map) == (want["map50"], want["map75"], want["map"])
    assert (res.box.mp, res.box.mr) == (want["precision"], want["recall"])
    assert res.box.map50 > 0
    assert {"preprocess", "inference", "postprocess"} <= set(res.speed)
    assert res.results_dict["metrics/mAP50-95(B)"] == res.box.map
    v = YOLO11Validator(m, device="cuda:0", output_dir=str(tmp_path / "val_out"))
    out = v.validate(root, imgsz=imgsz, batch=2, conf=0.001, iou=0.7)
    assert {"timestamp", "validation_time_seconds", "device", "model_info", "box_metrics", "speed_metrics"} <= set(out)
    assert set(out["box_metrics"]) == {"mAP50-95", "mAP50", "mAP75", "precision", "recall"}
    assert out["box_metrics"]["mAP50"] == want["map50"]
    assert v.validation_history == [out] and (tmp_path / "val_out" / "validation_summary.txt").is_file()
