"""Host-side tests of pose validation (no GPU): the object keypoint similarity and the matching rule factored out of
match_predictions (yolomi/metrics.py), pose label parsing and the native-pixel helpers (yolomi/val.py), evaluate_pose,
the PoseMetrics keys of ValResults and the validator's `pose_metrics` (core/validator.py).  Known answers are worked by
hand in float64 from the rules DESIGN.md §14 restates; tests/pose_val_oracle.py is the torch fp32 restatement of
upstream's kpt_iou / PoseValidator._process_batch.
"""
import math
import os

import numpy as np
import pytest
import torch

from tests import pose_val_oracle as O
from yolomi import val as V
from yolomi.metrics import (IOUV, OKS_SIGMA, box_iou, evaluate, evaluate_pose, kpt_iou, match_iou, match_predictions)

EPS = 1e-7


# ------------------------------------------------------------------------------------------------ kpt_iou
def test_oks_sigma_is_upstreams():
    assert OKS_SIGMA.shape == (17,) and OKS_SIGMA.dtype == np.float64
    assert np.array_equal(OKS_SIGMA, O.OKS_SIGMA)
    assert OKS_SIGMA[0] == 0.26 / 10 and OKS_SIGMA[11] == 1.07 / 10 and OKS_SIGMA[16] == 0.89 / 10


def test_kpt_iou_one_visible_keypoint_at_a_known_offset():
    """K = 1, σ = 0.5 so (2σ)² = 1; offset (3, 4): d = 25; area 100: e = 25 / ((100 + eps) · 2);
    OKS = exp(−e) / (1 + eps)."""
    g = np.array([[[10.0, 10.0, 2.0]]])
    p = np.array([[[13.0, 14.0]]])
    got = kpt_iou(g, p, np.array([100.0]), np.array([0.5]))
    assert got.shape == (1, 1) and got.dtype == np.float64
    assert abs(got[0, 0] - math.exp(-25.0 / ((100.0 + EPS) * 2.0)) / (1.0 + EPS)) <= 1e-12
    # a predicted visibility column is not read; two predictions, two ground truths: (m, n) = (2, 2)
    g2 = np.array([[[10.0, 10.0, 2.0]], [[0.0, 0.0, 1.0]]])
    p2 = np.array([[[13.0, 14.0, 0.1]], [[0.0, 0.0, 0.9]]])
    got = kpt_iou(g2, p2, np.array([100.0, 50.0]), np.array([0.5]))
    want = [[math.exp(-25.0 / ((100.0 + EPS) * 2.0)), math.exp(-200.0 / ((100.0 + EPS) * 2.0))],
            [math.exp(-365.0 / ((50.0 + EPS) * 2.0)), 1.0]]
    assert np.abs(got - np.array(want) / (1.0 + EPS)).max() <= 1e-12


def test_kpt_iou_ground_truth_without_labelled_keypoints_is_zero():
    g = np.zeros((2, 17, 3))
    g[..., :2] = 5.0
    g[1, :, 2] = 2.0
    p = np.full((3, 17, 3), 5.0)  # exactly on every ground-truth keypoint
    got = kpt_iou(g, p, np.array([40.0, 40.0]), OKS_SIGMA)
    assert (got[0] == 0.0).all()  # 0 / (0 + eps)
    assert np.abs(got[1] - 17.0 / (17.0 + EPS)).max() <= 1e-12
    assert kpt_iou(np.zeros((0, 17, 3)), p, np.zeros(0), OKS_SIGMA).shape == (0, 3)
    assert kpt_iou(g, np.zeros((0, 17, 3)), np.array([40.0, 40.0]), OKS_SIGMA).shape == (2, 0)


def test_kpt_iou_unlabelled_keypoint_counts_on_neither_side():
    """K = 3, σ = (0.5, 0.5, 0.25); v = (2, 0, 1).  Keypoint 0 is off by (3, 4), keypoint 1 (unlabelled) by a mile,
    keypoint 2 by (0, 2): e0 = 25 / ((area + eps) · 2), e2 = 4 / (0.25 · (area + eps) · 2);
    OKS = (exp(−e0) + exp(−e2)) / (2 + eps)."""
    g = np.array([[[10.0, 10.0, 2.0], [20.0, 20.0, 0.0], [30.0, 30.0, 1.0]]])
    p = np.array([[[13.0, 14.0], [900.0, -900.0], [30.0, 32.0]]])
    area = 80.0
    got = kpt_iou(g, p, np.array([area]), np.array([0.5, 0.5, 0.25]))[0, 0]
    want = (math.exp(-25.0 / ((area + EPS) * 2.0)) + math.exp(-4.0 / (0.25 * (area + EPS) * 2.0))) / (2.0 + EPS)
    assert abs(got - want) <= 1e-12
    moved = p.copy()
    moved[0, 1] = [20.0, 20.0]  # where the unlabelled keypoint lies does not matter
    assert kpt_iou(g, moved, np.array([area]), np.array([0.5, 0.5, 0.25]))[0, 0] == got


def test_kpt_iou_uniform_sigma_of_a_17x2_model():
    """kpt_shape (17, 2): σ = 1 / 17 for every keypoint; every keypoint off by (1, 0), all labelled:
    e = 1 / ((2 / 17)² · (area + eps) · 2), OKS = 17 · exp(−e) / (17 + eps)."""
    sigma = np.ones(17) / 17
    g = np.zeros((1, 17, 3))
    g[0, :, 0], g[0, :, 1], g[0, :, 2] = np.arange(17) * 3.0, 7.0, 1.0
    p = g[:, :, :2].copy()
    p[..., 0] += 1.0
    area = 12.5
    got = kpt_iou(g, p, np.array([area]), sigma)[0, 0]
    want = 17.0 * math.exp(-1.0 / ((2.0 / 17.0) ** 2 * (area + EPS) * 2.0)) / (17.0 + EPS)
    assert abs(got - want) <= 1e-12


def _random_pose_case(seed, m=6, n=9, K=17, size=128.0):
    rng = np.random.default_rng(seed)
    xy = rng.uniform(0, size - 40, (m, 2))
    wh = rng.uniform(10, 40, (m, 2))
    gt = np.concatenate([xy, xy + wh, np.ones((m, 1)), rng.integers(0, 2, (m, 1))], 1)
    gk = np.concatenate([xy[:, None] + rng.uniform(0, 1, (m, K, 2)) * wh[:, None],
                         rng.integers(0, 3, (m, K, 1)).astype(np.float64)], -1)
    gk[0, :, 2] = 0  # one ground truth without a labelled keypoint
    src = rng.integers(0, m, n)  # each prediction is a jittered copy of some ground truth
    pred = gt[src].copy()
    pred[:, :4] += rng.normal(0, 1.5, (n, 4))
    pred[:, 4] = np.sort(rng.uniform(0.01, 1, n))[::-1]
    pred[:, 5] = np.where(rng.uniform(size=n) < 0.8, gt[src, 5], 1 - gt[src, 5])
    pk = gk[src].copy()
    pk[..., :2] += rng.normal(0, 1, (n, K, 1)) * rng.uniform(0, 4, (n, 1, 1))
    pk[..., 2] = rng.uniform(0, 1, (n, K))
    return pred, gt, pk, gk


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_kpt_iou_agrees_with_the_fp32_restatement(seed):
    """1e-5 absolute: an OKS is a sum of at most 17 terms ≤ 1 divided by their count, so fp32 rounding of the sum is
    ~17 · 2⁻²⁴ ≈ 1e-6, and a term's own error is exp(−e) · e · (a few fp32 ulps) ≤ 0.37 · 4 · 6e-8 ≈ 1e-7."""
    pred, gt, pk, gk = _random_pose_case(seed)
    area = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]) * 0.53
    got = kpt_iou(gk, pk, area, OKS_SIGMA)
    ref = O.kpt_iou(torch.from_numpy(gk).float(), torch.from_numpy(pk).float(), torch.from_numpy(area).float(),
                    O.OKS_SIGMA).numpy()
    assert got.shape == ref.shape == (len(gt), len(pred)) and got.max() > 0.3 and (got[0] == 0).all()
    assert np.abs(got - ref).max() <= 1e-5
    # and the (17, 2) rule
    sig = np.ones(17) / 17
    ref = O.kpt_iou(torch.from_numpy(gk).float(), torch.from_numpy(pk[..., :2]).float(),
                    torch.from_numpy(area).float(), sig).numpy()
    assert np.abs(kpt_iou(gk, pk[..., :2], area, sig) - ref).max() <= 1e-5


# ------------------------------------------------------------------------------------------------ matching
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_match_iou_reproduces_match_predictions(seed):
    pred, gt, pk, gk = _random_pose_case(seed, m=8, n=40)
    tp = match_predictions(pred, gt)
    assert tp.shape == (40, 10) and tp.dtype == bool and tp[:, 0].any() and not tp.all()
    assert np.array_equal(match_iou(box_iou(gt[:, :4], pred[:, :4]), pred[:, 5], gt[:, 5]), tp)
    # the rule itself against upstream's, fed the same float64 IoU / OKS matrices
    for iou in (box_iou(gt[:, :4], pred[:, :4]),
                kpt_iou(gk, pk, (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]) * 0.53, OKS_SIGMA)):
        assert np.abs(iou[:, :, None] - IOUV).min() > 1e-6  # no value on a threshold: fp32 and float64 thresholds agree
        ref = O.match_predictions(torch.from_numpy(pred[:, 5]), torch.from_numpy(gt[:, 5]), torch.from_numpy(iou))
        assert np.array_equal(match_iou(iou, pred[:, 5], gt[:, 5]), ref.numpy())


def test_match_iou_empty_sides():
    assert match_iou(np.zeros((0, 3)), np.zeros(3), np.zeros(0)).shape == (3, 10)
    assert not match_iou(np.zeros((0, 3)), np.zeros(3), np.zeros(0)).any()
    assert match_iou(np.zeros((2, 0)), np.zeros(0), np.zeros(2)).shape == (0, 10)
    assert match_predictions(np.zeros((0, 6)), np.ones((2, 6))).shape == (0, 10)


def test_process_batch_restatement_matches_on_oks_or_iou():
    """The two branches of upstream's _process_batch against match_iou on this module's float64 matrices."""
    pred, gt, pk, gk = _random_pose_case(7, m=8, n=40)
    t = lambda a: torch.from_numpy(a).float()  # noqa: E731
    area = (gt[:, 2] - gt[:, 0]) * (gt[:, 3] - gt[:, 1]) * 0.53
    oks = kpt_iou(gk, pk, area, OKS_SIGMA)
    iou = box_iou(gt[:, :4], pred[:, :4])
    for mat in (oks, iou):
        assert np.abs(mat[:, :, None] - IOUV).min() > 1e-5  # (fp32 matrices: no value within rounding of a threshold)
    assert np.array_equal(O.process_batch(t(pred), t(gt[:, :4]), t(gt[:, 5]), t(pk), t(gk)).numpy(),
                          match_iou(oks, pred[:, 5], gt[:, 5]))
    assert np.array_equal(O.process_batch(t(pred), t(gt[:, :4]), t(gt[:, 5])).numpy(), match_predictions(pred, gt))


# ------------------------------------------------------------------------------------------------ labels, dataset
def _png(path, h, w, seed=0):
    from PIL import Image
    rgb = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(rgb).save(path)


def test_read_pose_labels_ndim3(tmp_path):
    p = tmp_path / "a.txt"
    p.write_text("0 0.5 0.5 0.2 0.4 0.1 0.2 2 0.3 0.4 0 0.5 0.6 1\n\n0 0.25 0.75 0.1 0.1 0 0 0 0.9 0.8 2 0.7 0.6 2\n")
    a = V.read_pose_labels(str(p), (3, 3))
    assert a.shape == (2, 14) and a.dtype == np.float32
    assert a[0].tolist() == [np.float32(v) for v in (0, .5, .5, .2, .4, .1, .2, 2, .3, .4, 0, .5, .6, 1)]
    assert a[1, 5:8].tolist() == [0, 0, 0] and a[1, 8:11].tolist() == [np.float32(.9), np.float32(.8), 2]


def test_read_pose_labels_ndim2_visibility_from_the_sign(tmp_path):
    """verify_image_label: ndim 2 labels gain v = 1, or 0 where x < 0 or y < 0."""
    p = tmp_path / "a.txt"
    p.write_text("0 0.5 0.5 0.2 0.4 0.1 0.2 -1 0.4 0.5 -0.001 0 0\n")
    a = V.read_pose_labels(str(p), (4, 2))
    assert a.shape == (1, 5 + 4 * 3)
    k = a[0, 5:].reshape(4, 3)
    assert k[:, 2].tolist() == [1, 0, 0, 1]  # (0, 0) is not negative: labelled
    assert k[:, :2].tolist() == [[np.float32(.1), np.float32(.2)], [-1, np.float32(.4)], [.5, np.float32(-.001)], [0, 0]]


def test_read_pose_labels_wrong_column_count_names_the_expected_one(tmp_path):
    p = tmp_path / "a.txt"
    p.write_text("0 0.5 0.5 0.2 0.4 0.1 0.2 2 0.3 0.4\n")  # 10 columns
    with pytest.raises(ValueError, match="56 columns"):
        V.read_pose_labels(str(p), (17, 3))
    with pytest.raises(ValueError, match="11 columns"):
        V.read_pose_labels(str(p), (3, 2))
    p.write_text("0 0.5 0.5 0.2 0.4\n")  # a detect label is not a pose label
    with pytest.raises(ValueError, match="56 columns"):
        V.read_pose_labels(str(p), (17, 3))
    assert V.read_labels(str(p)).shape == (1, 5)  # the detect reader is as before


def test_read_pose_labels_empty_or_missing_file_is_background(tmp_path):
    p = tmp_path / "a.txt"
    p.write_text("\n  \n")
    for path in (p, tmp_path / "none.txt"):
        a = V.read_pose_labels(str(path), (17, 2))
        assert a.shape == (0, 5 + 51) and a.dtype == np.float32


def _pose_root(tmp_path, yaml_extra=""):
    _png(str(tmp_path / "root" / "images" / "val" / "a.png"), 16, 24)
    _png(str(tmp_path / "root" / "images" / "val" / "b.png"), 16, 24, 1)
    os.makedirs(tmp_path / "root" / "labels" / "val", exist_ok=True)
    (tmp_path / "root" / "labels" / "val" / "a.txt").write_text("0 0.5 0.5 1 1 0.25 0.5 2 0.75 0.5 0\n")
    y = tmp_path / "data.yaml"
    y.write_text("path: root\nval: images/val\nnames:\n  0: person\n" + yaml_extra)
    return str(y)


def test_load_dataset_with_kpt_shape(tmp_path):
    y = _pose_root(tmp_path, "kpt_shape: [2, 3]\n")
    ds = V.load_dataset(y, kpt_shape=(2, 3))
    assert len(ds) == 2 and ds.names == {0: "person"}
    assert ds.labels[0].shape == (1, 11) and ds.labels[1].shape == (0, 11)
    assert ds.labels[0][0].tolist() == [0, .5, .5, 1, 1, .25, .5, 2, .75, .5, 0]
    # an absent entry: the model's shape is used
    assert V.load_dataset(_pose_root(tmp_path), kpt_shape=(2, 3)).labels[0].shape == (1, 11)
    # a directory dataset
    assert V.load_dataset(str(tmp_path / "root"), kpt_shape=[2, 3]).labels[0].shape == (1, 11)
    # the native-pixel keypoints of the label: x · w0, y · h0
    k = V.label_kpts_to_native(ds.labels[0], (16, 24), 2)
    assert k.dtype == np.float64 and k.tolist() == [[[6.0, 8.0, 2.0], [18.0, 8.0, 0.0]]]
    assert V.labels_to_native(ds.labels[0][:, :5], (16, 24))[0].tolist() == [0, 0, 24, 16, 1, 0]


def test_yaml_kpt_shape_mismatch_raises(tmp_path):
    y = _pose_root(tmp_path, "kpt_shape: [2, 3]\n")
    with pytest.raises(ValueError, match=r"kpt_shape \[2, 3\].*\[17, 3\]"):
        V.load_dataset(y, kpt_shape=(17, 3))
    with pytest.raises(ValueError, match="kpt_shape"):
        V.load_dataset(y, kpt_shape=(2, 2))
    # without a model shape the entry is not read and the detect reader runs, as before
    assert V.load_dataset(y).labels[0].shape == (1, 5)


def test_in_memory_pose_dataset():
    im = np.zeros((8, 12, 3), np.uint8)
    ds = V.load_dataset([(im, [[0, .5, .5, .5, .5, .1, .2, -1, .4]]), (im, np.zeros((0, 9)))], kpt_shape=(2, 2))
    assert ds.labels[0].shape == (1, 11) and ds.labels[1].shape == (0, 11)
    assert ds.labels[0][0, 5:].tolist() == [np.float32(.1), np.float32(.2), 1, -1, np.float32(.4), 0]
    ds = V.load_dataset([(im, np.zeros((3, 11)))], kpt_shape=(2, 3))
    assert ds.labels[0].shape == (3, 11)
    with pytest.raises(ValueError, match="11 columns"):
        V.load_dataset([(im, np.zeros((3, 5)))], kpt_shape=(2, 3))
    assert V.load_dataset([(im, np.zeros((3, 5)))]).labels[0].shape == (3, 5)  # kpt_shape=None: as before


def test_kpts_to_native_is_scale_coords_with_ratio_pad():
    b = V.build_batches([(480, 640)], imgsz=320, batch=1)[0]
    geo, gain = b["geo"][0], b["gain"][0]  # (240, 320, top 8, left 16), gain 0.5
    assert geo == (240, 320, 8, 16) and gain == 0.5
    k = np.array([[[16.0, 8.0, 0.7], [336.0, 248.0, 0.2], [176.0, 128.0, 0.5]],
                  [[0.0, 0.0, 0.1], [400.0, 300.0, 0.9], [17.0, 9.5, 1.0]]], np.float32)
    r = V.kpts_to_native(k, geo, gain, (480, 640))
    assert r.dtype == np.float64 and r.shape == (2, 3, 3)
    assert r[0].tolist() == [[0, 0, np.float32(.7)], [640, 480, np.float32(.2)], [320, 240, .5]]
    assert r[1].tolist() == [[0, 0, np.float32(.1)], [640, 480, np.float32(.9)], [2, 3, 1]]  # clipped; visibility kept
    assert k[1, 0, 0] == 0.0 and V.kpts_to_native(k[..., :2], geo, gain, (480, 640)).shape == (2, 3, 2)
    assert V.kpts_to_native(np.zeros((0, 3, 3), np.float32), geo, gain, (480, 640)).shape == (0, 3, 3)
    # the same gain and pad as the boxes' to_native
    box = np.array([[17.0, 9.5, 176.0, 128.0, 0.9, 0]], np.float32)
    assert V.to_native(box, geo, gain, (480, 640))[0, :4].tolist() == [2, 3, 320, 240]


# ------------------------------------------------------------------------------------------------ evaluate_pose
def _hand_case():
    """One image, one class, K = 2 with σ = (0.5, 0.5), so (2σ)² = 1.  Two 100 x 100 labels A and B (area · 0.53 =
    5,300) with both keypoints labelled.  Prediction 1 (conf 0.9) is A exactly.  Prediction 2 (conf 0.8) has B's box
    exactly but both keypoints displaced by (60, 0): d = 3,600, e = 3,600 / 10,600, OKS = exp(−0.33962) = 0.7120."""
    gts = [np.array([[0, 0, 100, 100, 1, 0], [200, 200, 300, 300, 1, 0]], np.float64)]
    gk = [np.array([[[20, 30, 2], [70, 60, 1]], [[220, 230, 2], [270, 260, 2]]], np.float64)]
    preds = [np.array([[0, 0, 100, 100, 0.9, 0], [200, 200, 300, 300, 0.8, 0]], np.float64)]
    pk = [gk[0].copy()]
    pk[0][1, :, 0] += 60.0
    pk[0][..., 2] = 0.9
    return preds, gts, pk, gk


def test_evaluate_pose_box_and_oks_matches_differ():
    """Box branch: both predictions are true positives at all ten thresholds: AP 0.995 each (the 101-point integral of
    a precision of 1 up to recall 1, as test_evaluate_old_keys_bit_unchanged records it).
    Pose branch: prediction 2's OKS 0.712 passes 0.50–0.70 and fails 0.75–0.95.  There the curve is recall (½, ½),
    precision (1, ½): the envelope is 1 up to recall ½, drops to ½ there and falls linearly to 0 at recall 1, so the
    integral is 0.49 + (1 + ½) / 2 · 0.01 + ½ · ½ · ½ = 0.6225.  mAP50 = 0.995, mAP75 = 0.6225,
    mAP50-95 = (5 · 0.995 + 5 · 0.6225) / 10 = 0.80875."""
    preds, gts, pk, gk = _hand_case()
    sigma = np.array([0.5, 0.5])
    oks = kpt_iou(gk[0], pk[0], np.array([5300.0, 5300.0]), sigma)
    want = 2.0 * math.exp(-3600.0 / ((5300.0 + EPS) * 2.0)) / (2.0 + EPS)
    assert abs(oks[1, 1] - want) <= 1e-12 and abs(want - 0.7120) < 1e-4 and oks[0, 0] == 2.0 / (2.0 + EPS)
    m = evaluate_pose(preds, gts, pk, gk, sigma)
    assert set(m) == {"box", "pose"}
    for k in ("box", "pose"):
        assert set(m[k]) == {"map", "map50", "map75", "precision", "recall"}
    assert m["box"] == evaluate(preds, gts)  # the box branch is evaluate itself
    assert m["box"]["map50"] == pytest.approx(0.995, abs=1e-12) and m["box"]["map"] == pytest.approx(0.995, abs=1e-12)
    assert m["pose"]["map50"] == pytest.approx(0.995, abs=1e-12)
    assert m["pose"]["map75"] == pytest.approx(0.6225, abs=1e-12)
    assert m["pose"]["map"] == pytest.approx(0.80875, abs=1e-12)
    assert m["pose"]["precision"] == pytest.approx(1.0) and m["pose"]["recall"] == pytest.approx(1.0)  # at OKS 0.5
    # the other way round: the right keypoints on a box that misses (the same curve, now at every box threshold)
    preds[0][1, :4] = [260, 260, 360, 360]  # IoU 1600 / 18400 = 0.087 with B
    pk[0][1] = gk[0][1]
    m = evaluate_pose(preds, gts, pk, gk, sigma)
    assert m["box"]["map"] == pytest.approx(0.6225, abs=1e-12) and m["pose"]["map"] == pytest.approx(0.995, abs=1e-12)
    assert (m["box"]["precision"], m["box"]["recall"]) != (m["pose"]["precision"], m["pose"]["recall"])


def test_evaluate_pose_empty_images():
    preds, gts, pk, gk = _hand_case()
    sigma = np.array([0.5, 0.5])
    one = evaluate_pose(preds, gts, pk, gk, sigma)
    # a background image without predictions, and an image whose predictions have no label: false positives
    preds += [np.zeros((0, 6)), np.array([[0, 0, 10, 10, 0.1, 0]], np.float64)]
    gts += [np.zeros((0, 6)), np.zeros((0, 6))]
    pk += [np.zeros((0, 2, 3)), np.zeros((1, 2, 3))]
    gk += [np.zeros((0, 2, 3)), np.zeros((0, 2, 3))]
    m = evaluate_pose(preds, gts, pk, gk, sigma)
    # the false positive ranks below every true positive of the box branch and of the pose branch at OKS 0.5
    assert m["box"]["map"] == one["box"]["map"] and m["pose"]["map50"] == one["pose"]["map50"]
    assert m["box"] == evaluate(preds, gts)
    none = evaluate_pose([np.zeros((0, 6))], [np.zeros((0, 6))], [np.zeros((0, 2, 3))], [np.zeros((0, 2, 3))], sigma)
    assert none["box"]["map"] == 0.0 and none["pose"] == none["box"]


# ------------------------------------------------------------------------------------------------ surface
BOX = {"map": 0.4, "map50": 0.6, "map75": 0.45, "precision": 0.7, "recall": 0.5}
POSE = {"map": 0.3, "map50": 0.5, "map75": 0.35, "precision": 0.65, "recall": 0.55}


def test_results_dict_keys_and_fitness():
    r = V.ValResults(BOX, {"inference": 1.0}, 4, 9, pose=POSE)
    assert list(r.results_dict) == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)",
                                    "metrics/mAP50-95(B)", "metrics/precision(P)", "metrics/recall(P)",
                                    "metrics/mAP50(P)", "metrics/mAP50-95(P)", "fitness"]
    assert (r.pose.map, r.pose.map50, r.pose.map75, r.pose.mp, r.pose.mr) == (0.3, 0.5, 0.35, 0.65, 0.55)
    assert (r.box.map, r.box.map50, r.box.map75, r.box.mp, r.box.mr) == (0.4, 0.6, 0.45, 0.7, 0.5)
    assert r.results_dict["metrics/mAP50-95(P)"] == 0.3 and r.results_dict["metrics/recall(P)"] == 0.55
    assert r.results_dict["fitness"] == (0.1 * 0.6 + 0.9 * 0.4) + (0.1 * 0.5 + 0.9 * 0.3)
    d = V.ValResults(BOX, {"inference": 1.0}, 4, 9)  # a detect result: key for key as before
    assert list(d.results_dict) == ["metrics/precision(B)", "metrics/recall(B)", "metrics/mAP50(B)",
                                    "metrics/mAP50-95(B)", "fitness"]
    assert d.results_dict["fitness"] == 0.1 * 0.6 + 0.9 * 0.4 and not hasattr(d, "pose")


class _FakePoseModel:
    def benchmark(self, *a, **k):
        raise AssertionError("not used")

    def get_model_info(self):
        return {"task": "pose", "size": "n"}

    def val(self, **kw):
        return V.ValResults(BOX, {"preprocess": 1.0, "inference": 2.0, "loss": 0.0, "postprocess": 3.0}, 4, 9,
                            pose=POSE)


def test_validate_schema_with_pose_metrics(tmp_path):
    from core.validator import YOLO11Validator
    v = YOLO11Validator(_FakePoseModel(), device="cpu", output_dir=str(tmp_path / "out"))
    out = v.validate("data.yaml", imgsz=320, batch=4)
    assert set(out) == {"timestamp", "validation_time_seconds", "device", "model_info", "box_metrics", "pose_metrics",
                        "speed_metrics"}
    assert out["box_metrics"] == {"mAP50-95": 0.4, "mAP50": 0.6, "mAP75": 0.45, "precision": 0.7, "recall": 0.5}
    assert out["pose_metrics"] == {"mAP50-95": 0.3, "mAP50": 0.5, "mAP75": 0.35, "precision": 0.65, "recall": 0.55}
    txt = (tmp_path / "out" / "validation_summary.txt").read_text()
    assert "Pose Metrics:" in txt and "mAP50-95: 0.3000" in txt and "Box Detection Metrics:" in txt
    assert txt.index("Box Detection Metrics:") < txt.index("Pose Metrics:") < txt.index("Speed Metrics:")


class _StubEngine:
    def __init__(self, task):
        self.task = task


def test_run_val_still_refuses_segment_plans():
    with pytest.raises(NotImplementedError, match="segment") as e:
        V.run_val(_StubEngine("segment"), [])
    assert "pose" not in str(e.value).split("(")[0]  # the refusal names segment only
    with pytest.raises(NotImplementedError):
        V.run_val(_StubEngine("obb"), [])


# ------------------------------------------------------------------------------------------------ the GPU test's dataset
def test_the_gpu_tests_dataset_with_the_fp32_oracle_standing_in():
    """tests/test_gpu_pose_val.py's end-to-end dataset with tests/pose_oracle.py in the GPU's place (the images need no
    resize at imgsz 128, so the letterbox is a 114 border): labels = the conf-0.25 rows in native pixels, predictions =
    the conf-0.001 rows.  31 labels, 6–10 per image; 69–86 predictions per image, under max_det; every label is found
    again at IoU 1 and OKS > 0.9999999 (17 / (17 + 1e-7), less the labels' float32 rounding).  Pose AP is 0.995 at all
    ten thresholds.  Box AP is 0.958: boxes clipped to the 64 x 128 image become identical, and upstream's tie rule
    (each label keeps its most confident pair, after each prediction kept its best) then drops one true positive."""
    from tests.pose_oracle import PoseOracle
    from yolomi.synth import synth_weights
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    orc = PoseOracle("n", synth_weights("n", "pose", 0))
    shapes = [(96, 128), (128, 96), (128, 128), (64, 128)]
    rng = np.random.default_rng(5)
    imgs = [np.ascontiguousarray(rng.integers(0, 256, (h, w, 3), dtype=np.uint8)[..., ::-1]) for h, w in shapes]
    batches = V.build_batches(shapes, 128, 2)
    assert [b["shape"] for b in batches] == [(128, 160), (160, 160)] and batches[1]["indices"] == [2, 1]

    def rows(b, conf):
        x = np.full((len(b["indices"]), *b["shape"], 3), 114, np.uint8)
        for k, i in enumerate(b["indices"]):
            uh, uw, top, left = b["geo"][k]
            assert (uh, uw) == shapes[i] and b["gain"][k] == 1.0
            x[k, top:top + uh, left:left + uw] = imgs[i][..., ::-1]
        x = torch.from_numpy(np.ascontiguousarray(x.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255))
        for k, o in enumerate(orc.predict(x, conf=conf, iou=0.7, max_det=300)):
            i = b["indices"][k]
            yield i, (V.to_native(o["boxes"].numpy(), b["geo"][k], b["gain"][k], shapes[i]),
                      V.kpts_to_native(o["kpts_raw"].numpy(), b["geo"][k], b["gain"][k], shapes[i]))

    labels = [None] * 4
    for b in batches:
        for i, (r, kn) in rows(b, 0.25):
            h0, w0 = shapes[i]
            lb = [[cl, (x1 + x2) / 2 / w0, (y1 + y2) / 2 / h0, (x2 - x1) / w0, (y2 - y1) / h0]
                  + [v for x, y, _ in kk for v in (x / w0, y / h0, 2.0)] for (x1, y1, x2, y2, _, cl), kk in zip(r, kn)]
            labels[i] = np.array(lb, np.float32).reshape(-1, 5 + 51)  # what read_pose_labels returns: float32
    assert sum(len(lb) for lb in labels) == 31 and all(6 <= len(lb) <= 10 for lb in labels)
    preds, gts, pk, gk = [None] * 4, [None] * 4, [None] * 4, [None] * 4
    for b in batches:
        for i, (r, kn) in rows(b, 0.001):
            preds[i], pk[i] = r, kn
            gts[i] = V.labels_to_native(labels[i][:, :5], shapes[i])
            gk[i] = V.label_kpts_to_native(labels[i], shapes[i], 17)
    assert all(69 <= len(p) <= 86 for p in preds)
    for p, g, a, c in zip(preds, gts, pk, gk):
        assert (box_iou(g[:, :4], p[:, :4]).max(1) > 0.999999).all()
        area = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) * 0.53
        assert (kpt_iou(c, a, area, OKS_SIGMA).max(1) > 0.9999999).all()
    m = evaluate_pose(preds, gts, pk, gk, OKS_SIGMA)
    for k in ("map50", "map75", "map"):  # equal at 0.50, 0.75 and in the mean: the same AP at all ten thresholds
        assert m["pose"][k] == pytest.approx(0.995, abs=1e-9)
        assert m["box"][k] == pytest.approx(0.958, abs=5e-4)
