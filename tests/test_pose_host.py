"""Host-side (no GPU) tests of the pose task: plan, head layout, blob, synthetic weights, Keypoints, scale_coords and
the CPU restatement (tests/pose_oracle.py) against its golden."""
import hashlib
import json
import os

import numpy as np
import pytest
import torch

from yolomi.arch import GraphBuilder, infer_arch, infer_kpt_shape
from yolomi.plan import check_state_dict, fuse_default, pack_graph, pack_model, unpack_blob
from yolomi.synth import synth_weights

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_cache = {}


def pose_sd():
    if "sd" not in _cache:
        _cache["sd"] = synth_weights("n", "pose", 0)
    return _cache["sd"]


def test_pose_parameter_names_and_shapes():
    """Ultralytics yolo11n-pose names and shapes (c4 = max(64 // 4, 51) = 51), so a real state dict passes
    check_state_dict; the plan pads channels, the parameters do not."""
    g = GraphBuilder("n", "pose")
    assert g.nc == 1 and g.kpt_shape == (17, 3) and g.nk == 51
    shapes = {p.name: tuple(p.shape) for p in g.params}
    for l, cin in enumerate((64, 128, 256)):
        assert shapes[f"model.23.cv4.{l}.0.conv.weight"] == (51, cin, 3, 3)
        assert shapes[f"model.23.cv4.{l}.1.conv.weight"] == (51, 51, 3, 3)
        for j in (0, 1):
            for s in ("weight", "bias", "running_mean", "running_var"):
                assert shapes[f"model.23.cv4.{l}.{j}.bn.{s}"] == (51,)
        assert shapes[f"model.23.cv4.{l}.2.weight"] == (51, 51, 1, 1)
        assert shapes[f"model.23.cv4.{l}.2.bias"] == (51,)
        assert shapes[f"model.23.cv3.{l}.2.weight"] == (1, 64, 1, 1)
        assert shapes[f"model.23.cv3.{l}.2.bias"] == (1,)
    assert not any(n.startswith("model.23.proto.") for n in shapes)
    det = {p.name: tuple(p.shape) for p in GraphBuilder("n", "detect", nc=1).params}
    assert {k: v for k, v in shapes.items() if ".cv4." not in k} == det  # layers 0-22 + Detect(nc=1) unchanged
    check_state_dict(g, pose_sd())
    assert {p.name for p in g.params} == set(pose_sd())


def test_infer_arch_pose():
    sd = pose_sd()
    assert infer_arch(sd) == ("n", "pose", 1)
    assert infer_kpt_shape(sd) == (17, 3)
    assert infer_kpt_shape(sd, (17, 3)) == (17, 3)
    with pytest.raises(ValueError):
        infer_kpt_shape(sd, (17, 2))
    assert infer_kpt_shape(synth_weights("n", "detect", 0)) is None
    assert infer_arch(synth_weights("n", "detect", 0)) == ("n", "detect", 80)
    g2 = GraphBuilder("n", "pose", kpt_shape=(13, 2), pad_head=False)
    sd2 = {p.name: np.zeros(p.shape, np.float32) for p in g2.params}
    assert infer_kpt_shape(sd2) == (13, 2) and infer_arch(sd2) == ("n", "pose", 1)  # 26 channels: not K x 3


@pytest.mark.parametrize("fuse", [False, True, "x3"])
def test_pose_head_layout(fuse):
    """[64 box | 4 cls | 52 kpt], pitch 120; every head conv has N % 4 == 0, Cin % 8 == 0 and a 4-aligned slice."""
    g = GraphBuilder("n", "pose", fuse=fuse)
    assert g.anchor_buf.C == 120 and g.no == 68 and g.kpt_off == 68 and g.nm == g.nk_pad == 52
    slices = set()
    for op in g.ops:
        if op.kind != "conv":
            continue
        a = op.args
        last = a.get("pair") or a
        assert a["c1"] % 8 == 0 or op.name == "model.0", op.name
        assert a["c2"] % 4 == 0 and last["c2"] % 4 == 0, op.name
        if a["anchor_level"] >= 0:
            d = a["dst"]
            assert d.buf is g.anchor_buf and d.coff % 4 == 0 and d.C % 4 == 0 and d.C == last["c2"]
            slices.add((d.coff, d.C))
    assert slices == {(0, 64), (64, 4), (68, 52)}
    # detect and segment plans keep their layout
    assert GraphBuilder("n", "detect").anchor_buf.C == 144 and GraphBuilder("s", "segment").anchor_buf.C == 176


def _records(blob):
    h, _, ops, names, woff = unpack_blob(blob)
    return h, dict(zip(names, ops)), woff


def test_pose_blob_header_and_zero_padding():
    sd = pose_sd()
    blob = pack_model("n", "pose", sd, "f32")
    h, ops, woff = _records(blob)
    assert h[3] == 2 and h[4] == 1 and h[5] == 52 and h[18] == 68
    assert list(h[20:24]) == [17, 3, 68, 4]
    r = ops["model.23.cv4.0.2"]  # 1x1, Cin 64 (51 + 13 zero columns), N 52 (51 + 1 zero row), Kpad 64
    assert (r[1], r[3], r[4], r[21], r[14]) == (1, 64, 52, 64, 68)
    w = np.frombuffer(blob, np.float32, 52 * 64, woff + r[19]).reshape(52, 64)
    b = np.frombuffer(blob, np.float32, 52, woff + r[20])
    assert np.array_equal(w[:51, :51], sd["model.23.cv4.0.2.weight"].reshape(51, 51))
    assert not w[51].any() and not w[:, 51:].any() and b[51] == 0
    assert np.array_equal(b[:51], sd["model.23.cv4.0.2.bias"])
    r = ops["model.23.cv3.0.2"]
    assert (r[3], r[4], r[14]) == (64, 4, 64)
    w = np.frombuffer(blob, np.float32, 4 * 64, woff + r[19]).reshape(4, 64)
    b = np.frombuffer(blob, np.float32, 4, woff + r[20])
    assert np.array_equal(w[0], sd["model.23.cv3.0.2.weight"].reshape(64)) and not w[1:].any() and not b[1:].any()
    r = ops["model.23.cv4.0.0"]  # 3x3 64 -> 64 (51 real rows): the pad rows' folded bias is 0, so they output SiLU(0) = 0
    b = np.frombuffer(blob, np.float32, 64, woff + r[20])
    assert r[4] == 64 and b[:51].all() and not b[51:].any()


# sha256 of pack_model(scale, task, synth_weights(scale, task, 0), dtype) on the commit before the pose task (the
# detect and segment x3 / f16 plans) and on the commit before the blob's slots were named (the others); all twelve are
# checked by tests/test_plan_format.py
PARENT_BLOBS = {
    ("n", "detect", "x3"): "a246e70f1b491e5e976cd0579d59153dea0f2f0058840efbb35103b57f4097d2",
    ("n", "detect", "f16"): "9fa916da2e40a79ffb4a8f0f4fccbec5062d9afba929d638d6cae8842423d7f2",
    ("s", "segment", "x3"): "d36a6654fbb913376f4b9de5a3b59046f37901d7b7d07027ab356d5703e2f59d",
    ("s", "segment", "f16"): "0b5102be191732a75f37af8939dc2ceff534be5904ba1dd616c19d16aec4bb0e",
    ("n", "detect", "f32"): "6440e6b27fac17bad14d138d662943d557ca07fbe7c1650dcf9ea91807ceb99e",
    ("s", "segment", "f32"): "c516009640fa27d84ba8548d15ad4496c5051e81db9ab2f48a73c68ca0f03fc4",
    ("n", "pose", "f16"): "564624ae663f3a6564858fc2f544aa94c7457f2d4c4ad4611249561d7358a6b4",
    ("n", "pose", "f32"): "5b9c9ca7ed1f443da8bf54a7dcd7a548e7344956226ef47a82c8a24651793be1",
    ("n", "pose", "x3"): "a2c1c2126e1505e4454e8cfadfeb823145928c689165f8bbb1ade5f1b25f62dc",
}
# one-byte plans: (fixture under tests/golden whose qparams and weights seed the plan is packed with, dtype) -> sha256
PARENT_QBLOBS = {
    ("det_n_i8_qnnpack", "i8"): "8815f7639bf8bb454c3fd65d4fa0dccfd5e8aa9878533b4b0c1d12fbdb9fb59b",
    ("det_n_i8_fbgemm_320", "i8"): "33d1df4f7e34ce3b14478d23ddd521b1ed47a8911871c9a238347338e9bfe702",
    ("det_n_f8", "f8"): "37679b55a4f276fa2ac87e6a94f80857939145b27d2115f3d9baeca0535cca3b",
}


@pytest.mark.parametrize("scale,task", [("n", "detect"), ("s", "segment")])
def test_detect_and_segment_blobs_are_byte_identical(scale, task, monkeypatch):
    for v in ("YM_FUSE", "YM_FUSE_DW", "YM_DW_FUSE_STRIDES"):
        monkeypatch.delenv(v, raising=False)
    sd = synth_weights(scale, task, 0)
    for dtype in ("x3", "f16"):
        assert hashlib.sha256(pack_model(scale, task, sd, dtype)).hexdigest() == PARENT_BLOBS[(scale, task, dtype)]


def test_pose_quantized_plans_raise():
    with pytest.raises(ValueError, match="PTQ"):
        pack_model("n", "pose", pose_sd(), "i8")
    with pytest.raises(ValueError, match="PTQ"):
        pack_graph(GraphBuilder("n", "pose", quant=True), pose_sd(), "f8", {"backend": "fp8"})
    with pytest.raises(ValueError, match="pad_head"):
        pack_graph(GraphBuilder("n", "pose", pad_head=False, fuse=fuse_default("f32")), pose_sd(), "f32")


def test_pose_golden_reproduced_by_the_restatement():
    from tests.golden.make_golden import layer_stats, make_input
    from tests.golden.make_pose_golden import head_rows
    from tests.pose_oracle import PoseOracle
    g = json.load(open(os.path.join(GOLD, "pose_n_uniform.json")))
    assert g["task"] == "pose" and g["kpt_shape"] == [17, 3]
    assert all(5 <= len(r) < 300 for r in g["nms_rows"])  # non-degenerate at conf 0.25
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    om = PoseOracle("n", pose_sd())
    x = make_input("uniform", g["input"]["seeds"], g["input"]["size"])
    _, _, ex = om.raw(x)
    st = layer_stats(head_rows(ex, 2))
    assert st["shape"] == g["head"]["shape"] == [2, 2100, 116]
    assert np.allclose(st["samples"], g["head"]["samples"], rtol=1e-4, atol=1e-5)
    assert abs(st["abs_sum"] - g["head"]["abs_sum"]) <= 1e-5 * g["head"]["abs_sum"]
    res = om.predict(x, conf=g["conf"], iou=g["iou"])
    for r, rows in zip(res, g["nms_rows"]):
        rows = np.asarray(rows, np.float32).reshape(-1, 57)
        assert len(r["boxes"]) == len(rows)
        assert np.allclose(r["boxes"].numpy(), rows[:, :6], rtol=0, atol=2e-3)
        k = rows[:, 6:].reshape(-1, 17, 3)
        assert np.allclose(r["kpts_raw"].numpy(), k, rtol=0, atol=2e-3)
        assert (k[..., 0] >= 0).all() and (k[..., 0] <= 320).all() and (k[..., 1] >= 0).all() and (k[..., 1] <= 320).all()
        assert (k[..., 2] > 0).all() and (k[..., 2] < 1).all()


def test_kpts_decode_formula_by_hand():
    """One P3 anchor at grid (x 5, y 2), stride 8: x = (raw·2 + 5)·8, y = (raw·2 + 2)·8, v = sigmoid(raw)."""
    from tests.pose_oracle import Pose
    head = Pose(1, (2, 3), ch=(16, 16, 16)).eval()
    feats = [torch.zeros(1, 16, 4, 8), torch.zeros(1, 16, 2, 4), torch.zeros(1, 16, 1, 2)]
    raw = torch.zeros(1, 6, 42)
    a = 2 * 8 + 5
    raw[0, :, a] = torch.tensor([0.25, -1.5, 0.0, 3.0, 0.5, 2.0])
    from oracle.yolo11 import make_anchors
    head.anchors, head.strides = (t.transpose(0, 1) for t in make_anchors(feats, head.stride, 0.5))
    y = head.kpts_decode(1, raw)[0, :, a]
    assert y[:2].tolist() == [(0.25 * 2 + 5) * 8, (-1.5 * 2 + 2) * 8] and y[2] == 0.5
    assert y[3:5].tolist() == [(3.0 * 2 + 5) * 8, (0.5 * 2 + 2) * 8]
    assert abs(float(y[5]) - 1 / (1 + np.exp(-2.0))) < 1e-7
    y32 = head.kpts_decode(1, raw)[0, :, 32 + 5]  # first P4 anchor row (y 0), x 5 would be out of its 4 columns:
    assert y32[0] == (0 * 2 + 1) * 16               # anchor 37 = P4 index 5 = (x 1, y 1), stride 16


def test_keypoints_view_masking_xyn_conf():
    from core.results import Keypoints
    d = torch.tensor([[[10.0, 20.0, 0.9], [30.0, 40.0, 0.49], [50.0, 60.0, 0.5]]])
    k = Keypoints(d.clone(), (100, 200))
    assert k.data.shape == (1, 3, 3) and len(k) == 1 and k.has_visible
    assert k.xy.tolist() == [[[10.0, 20.0], [0.0, 0.0], [50.0, 60.0]]]  # visibility < 0.5 → xy zeroed; 0.5 stays
    assert torch.allclose(k.xyn, torch.tensor([[[0.05, 0.2], [0.0, 0.0], [0.25, 0.6]]]))
    assert torch.equal(k.conf, torch.tensor([[0.9, 0.49, 0.5]]))
    assert k.xy.tolist() == [[[10.0, 20.0], [0.0, 0.0], [50.0, 60.0]]]  # xyn did not touch the data
    k2 = Keypoints(torch.tensor([[[10.0, 20.0], [30.0, 40.0]]]), (100, 200))
    assert k2.conf is None and not k2.has_visible and k2.xy.shape == (1, 2, 2)
    n = k.cpu().numpy()
    assert isinstance(n.data, np.ndarray) and n.orig_shape == (100, 200) and n.data.shape == (1, 3, 3)
    assert k[0].data.shape == (1, 3, 3)  # one instance keeps the leading dimension, like Boxes
    from tests.pose_oracle import keypoints_mask
    assert torch.equal(keypoints_mask(d), k.data)


def test_scale_coords_by_hand():
    """A 240x320 image letterboxed to 320x320: gain min(320/240, 320/320) = 1, pad x round(0 - 0.1) = 0,
    pad y round(40 - 0.1) = 40: y' = y - 40, then x clipped to [0, 320], y to [0, 240]."""
    from tests.pose_oracle import scale_coords as ref_scale
    from yolomi.preprocess import scale_coords
    k = torch.tensor([[[100.0, 100.0, 0.7], [330.0, 30.0, 0.2], [-5.0, 300.0, 0.9]]])
    want = torch.tensor([[[100.0, 60.0, 0.7], [320.0, 0.0, 0.2], [0.0, 240.0, 0.9]]])
    assert torch.equal(scale_coords((320, 320), k.clone(), (240, 320)), want)
    assert torch.equal(ref_scale((320, 320), k.clone(), (240, 320)), want)
    # a 2x down-scaled source: 480x640 → 320x320 canvas, gain 0.5, pad y round((320 - 240) / 2 - 0.1) = 40
    k = torch.tensor([[[100.0, 100.0], [0.0, 39.0]]])
    want = torch.tensor([[[200.0, 120.0], [0.0, 0.0]]])
    assert torch.equal(scale_coords((320, 320), k.clone(), (480, 640)), want)
    assert torch.equal(ref_scale((320, 320), k.clone(), (480, 640)), want)
    # equal shapes (tensor sources): clip only
    k = torch.tensor([[[-1.0, 321.0, 0.3], [7.25, 8.5, 0.6]]])
    assert torch.equal(scale_coords((320, 320), k.clone(), (320, 320)),
                       torch.tensor([[[0.0, 320.0, 0.3], [7.25, 8.5, 0.6]]]))


def test_results_keypoints_lazy_and_none_for_other_tasks():
    from core.results import Results
    dets = torch.zeros(1, 4, 6 + 52)
    dets[0, 0, :6] = torch.tensor([1.0, 2.0, 30.0, 40.0, 0.9, 0.0])
    dets[0, 0, 6:6 + 51] = torch.arange(51, dtype=torch.float32) - 3.0  # kpt 0 = (-3, -2, -1): clipped, then masked
    dets[0, 0, 6 + 51] = 123.0  # the pad column never shows
    im = torch.zeros(1, 3, 32, 32)
    r = Results.from_batch(im, 0, {0: "person"}, dets, 1, kpt_shape=(17, 3))
    k = r.keypoints
    assert k.data.shape == (1, 17, 3) and k.orig_shape == (32, 32)
    assert k.data[0, 0].tolist() == [0.0, 0.0, -1.0]
    assert k.data[0, 1].tolist() == [0.0, 1.0, 2.0] and k.data[0, 16].tolist() == [32.0, 32.0, 47.0]
    assert dets[0, 0, 6] == -3.0  # the device rows are not modified
    assert Results.from_batch(im, 0, {0: "a"}, dets, 1).keypoints is None
    assert Results(im[0], {0: "a"}, dets[0, :1, :6]).keypoints is None
    assert r.cpu().keypoints.data.shape == (1, 17, 3) and r[0].keypoints.data.shape == (1, 17, 3)


def test_pose_facade_contract_without_gpu():
    from core.model import YOLO11Model
    assert "pose" in YOLO11Model.HIP_TASKS
    with pytest.raises(RuntimeError, match="no HIP path"):
        YOLO11Model(task="pose", device="cpu")
    with pytest.raises(NotImplementedError):
        YOLO11Model(task="obb", device="cuda")


def test_visualization_keypoints(tmp_path):
    from core.results import Results
    from utils.visualization import draw_keypoints, save_detection_results
    box = torch.tensor([[1.0, 2.0, 30.0, 40.0, 0.9, 0.0]])
    kp = torch.tensor([[[10.0, 5.0, 0.9], [20.0, 6.0, 0.1]]])
    r = Results(torch.zeros(3, 32, 32), {0: "person"}, box, keypoints=kp)
    img = draw_keypoints(np.zeros((32, 32, 3), np.uint8), r, radius=1)
    assert img[5, 10].tolist() == [0, 255, 0] and img.sum() == 9 * 255  # the invisible keypoint is not drawn
    p = tmp_path / "o.json"
    save_detection_results(r, str(p), "json")
    d = json.load(open(p))["detections"][0]
    assert d["keypoints"][0] == [10.0, 5.0, pytest.approx(0.9)] and d["keypoints"][1][:2] == [0.0, 0.0]
    save_detection_results(Results(torch.zeros(3, 32, 32), {0: "a"}, box), str(p), "json")
    assert "keypoints" not in json.load(open(p))["detections"][0]
