"""Host-side tests of validation mode (no GPU): dataset parsing, the val loader's rect batching, precision / recall,
and the YOLO11Validator.validate schema (yolomi/val.py, yolomi/metrics.py, core/validator.py)."""
import ctypes
import os

import numpy as np
import pytest

from yolomi import val as V
from yolomi.metrics import evaluate


def _png(path, h, w, seed=0):
    from PIL import Image
    rgb = np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(rgb).save(path)
    return np.ascontiguousarray(rgb[..., ::-1])


# ------------------------------------------------------------------------------------------------ dataset parsing
def test_label_path_rule():
    s = os.sep
    assert V.img2label_path(f"{s}d{s}images{s}val{s}a.jpg") == f"{s}d{s}labels{s}val{s}a.txt"
    # only the LAST /images/ is replaced
    assert V.img2label_path(f"{s}images{s}x{s}images{s}b.png") == f"{s}images{s}x{s}labels{s}b.txt"
    assert V.img2label_path(f"{s}d{s}pics{s}c.jpeg") == f"{s}d{s}pics{s}c.txt"


def test_directory_dataset(tmp_path):
    a = _png(str(tmp_path / "images" / "a.png"), 20, 30, 1)
    _png(str(tmp_path / "images" / "sub" / "b.png"), 30, 20, 2)
    os.makedirs(tmp_path / "labels" / "sub")
    (tmp_path / "labels" / "a.txt").write_text("3 0.5 0.5 0.2 0.4\n\n7 0.25 0.75 0.1 0.1\n")
    ds = V.load_dataset(str(tmp_path))  # b.png has no label file: a background image
    assert [os.path.basename(p) for p in ds.images] == ["a.png", "b.png"]
    assert ds.labels[0].shape == (2, 5) and ds.labels[0][1].tolist() == [7, 0.25, 0.75, np.float32(0.1), np.float32(0.1)]
    assert ds.labels[1].shape == (0, 5)
    assert np.array_equal(ds.image(0), a)  # HWC uint8 BGR
    g = V.labels_to_native(ds.labels[0], (20, 30))
    assert g[0].tolist() == pytest.approx([12, 6, 18, 14, 1, 3])


def test_yaml_dataset(tmp_path):
    _png(str(tmp_path / "root" / "images" / "val" / "a.png"), 16, 16)
    os.makedirs(tmp_path / "root" / "labels" / "val")
    (tmp_path / "root" / "labels" / "val" / "a.txt").write_text("1 0.5 0.5 1 1\n")
    y = tmp_path / "data.yaml"
    y.write_text("path: root\nval: images/val\nnames:\n  0: cat\n  1: dog\n")
    ds = V.load_dataset(str(y))
    assert len(ds) == 1 and ds.names == {0: "cat", 1: "dog"} and ds.labels[0].tolist() == [[1, 0.5, 0.5, 1, 1]]
    lst = tmp_path / "root" / "val.txt"
    lst.write_text("images/val/a.png\n")
    y.write_text(f"path: {tmp_path / 'root'}\nval: val.txt\nnames: [cat, dog]\n")
    ds = V.load_dataset(str(y))
    assert len(ds) == 1 and ds.names == {0: "cat", 1: "dog"} and len(ds.labels[0]) == 1
    with pytest.raises(FileNotFoundError):
        V.load_dataset(str(tmp_path / "nothing"))


def test_in_memory_dataset():
    im = np.zeros((8, 12, 3), np.uint8)
    ds = V.load_dataset([(im, [[2, 0.5, 0.5, 0.5, 0.5]]), (im, np.zeros((0, 5)))])
    assert len(ds) == 2 and ds.labels[0].shape == (1, 5) and ds.labels[1].shape == (0, 5) and ds.image(1) is not None
    with pytest.raises(ValueError):
        V.load_dataset([(np.zeros((8, 12), np.uint8), [])])


# ------------------------------------------------------------------------------------------------ rect batching
def test_rect_batches_known_answers():
    """(h, w) = (480, 640), (640, 480), (500, 500), (300, 900) at imgsz 320, batch 2, worked by hand:
    h / w = 0.75, 1.333, 1.0, 0.333 → order 3, 0, 2, 1.
    Batch [3, 0]: maxi 0.75 < 1 → factor [0.75, 1] → ceil(0.75·320/32 + 0.5) = 8, ceil(10.5) = 11 → 256 x 352.
      image 3: r = 320/900, w = min(ceil(320.0…), 320) = 320, h = ceil(106.67) = 107; top = round(74.5 − 0.1) = 74,
               left = round(16 − 0.1) = 16.   image 0: r = 0.5 → 240 x 320; top = round(8 − 0.1) = 8, left 16.
    Batch [2, 1]: mini 1.0 is not > 1, maxi 1.333 is not < 1 → [1, 1] → 352 x 352.
      image 2: 320 x 320, top = left = 16.   image 1: 320 x 240, top 16, left = round(56 − 0.1) = 56."""
    b = V.build_batches([(480, 640), (640, 480), (500, 500), (300, 900)], imgsz=320, batch=2)
    assert [x["indices"] for x in b] == [[3, 0], [2, 1]]
    assert [x["shape"] for x in b] == [(256, 352), (352, 352)]
    assert b[0]["geo"] == [(107, 320, 74, 16), (240, 320, 8, 16)]
    assert b[1]["geo"] == [(320, 320, 16, 16), (320, 240, 16, 56)]
    assert b[0]["gain"] == pytest.approx([107 / 300, 0.5]) and b[1]["gain"] == pytest.approx([0.64, 0.5])
    # a tall batch: mini > 1 → [1, 1 / mini]
    t = V.build_batches([(640, 320), (600, 200)], imgsz=640, batch=2)
    assert t[0]["indices"] == [0, 1] and t[0]["shape"] == (672, 352)  # ceil(20.5) = 21, ceil(0.5·20 + 0.5) = 11
    assert t[0]["geo"] == [(640, 320, 16, 16), (640, 214, 16, 69)]  # 200·640/600 = 213.3 → 214; (352 − 214)/2 = 69
    # equal aspect ratios keep the dataset order (stable sort); the last batch may be short
    e = V.build_batches([(10, 10)] * 3, imgsz=32, batch=2)
    assert [x["indices"] for x in e] == [[0, 1], [2]] and e[0]["shape"] == (64, 64)


def test_to_native_inverts_the_letterbox():
    b = V.build_batches([(480, 640)], imgsz=320, batch=1)[0]
    uh, uw, top, left = b["geo"][0]
    box = np.array([[left, top, left + uw, top + uh, 0.9, 4], [0, 0, 400, 400, 0.5, 1]], np.float32)
    r = V.to_native(box, b["geo"][0], b["gain"][0], (480, 640))
    assert r[0].tolist() == pytest.approx([0, 0, 640, 480, 0.9, 4])
    assert r[1, :4].tolist() == [0, 0, 640, 480]  # clipped to the native image


# ------------------------------------------------------------------------------------------------ metrics
GT = [np.array([[10, 10, 50, 50, 1, 3], [100, 100, 150, 180, 1, 5]], np.float64)]


def test_precision_recall_known_answers():
    m = evaluate([GT[0].copy()], GT)
    assert (m["precision"], m["recall"]) == (1.0, 1.0)
    shifted = GT[0].copy()
    shifted[1, :4] += 20  # class 5's only prediction is a false positive: p = r = 0 for it, 1 for class 3
    m = evaluate([shifted], GT)
    assert (m["precision"], m["recall"]) == (0.5, 0.5)
    m = evaluate([np.zeros((0, 6))], GT)
    assert (m["precision"], m["recall"]) == (0.0, 0.0)
    # one class, two labels; predictions TP (0.9), FP (0.6), TP (0.3): recall 0.5, 0.5, 1 and precision 1, 1/2, 2/3.
    # F1 is 2/3 at confidence 0.9, lower in between and 0.8 from 0.3 down: the maximum is the plateau p = 2/3, r = 1
    g = [np.array([[0, 0, 10, 10, 1, 2], [20, 20, 30, 30, 1, 2]], np.float64)]
    p = [np.array([[0, 0, 10, 10, .9, 2], [50, 50, 60, 60, .6, 2], [20, 20, 30, 30, .3, 2]], np.float64)]
    m = evaluate(p, g)
    assert m["precision"] == pytest.approx(2 / 3) and m["recall"] == pytest.approx(1.0)


def test_evaluate_old_keys_bit_unchanged():
    """map / map50 / map75 as the parent computed them (values recorded from the parent's evaluate)."""
    assert evaluate([GT[0].copy()], GT)["map"] == 0.9950000000000001
    shifted = GT[0].copy()
    shifted[1, :4] += 20
    m = evaluate([shifted], GT)
    assert (m["map50"], m["map75"], m["map"]) == (0.4975, 0.4975, 0.49749999999999994)
    assert {"map", "map50", "map75", "precision", "recall"} == set(m)


# ------------------------------------------------------------------------------------------------ surface
def test_infer_args_layout():
    """multi_label is carved out of reserved[4]: size and every other offset unchanged."""
    from yolomi.lib import InferArgs, Runtime
    assert ctypes.sizeof(InferArgs) == 88
    assert InferArgs.d_batch_max.offset == 64 and InferArgs.multi_label.offset == 72
    assert InferArgs.reserved.offset == 76 and InferArgs.reserved.size == 12
    assert Runtime.make_args().multi_label == 0 and Runtime.make_args(multi_label=True).multi_label == 1


class _FakeBox:
    map, map50, map75, mp, mr = 0.4, 0.6, 0.45, 0.7, 0.5


class _FakeModel:
    def __init__(self):
        self.calls = []

    def benchmark(self, *a, **k):
        raise AssertionError("not used")

    def get_model_info(self):
        return {"task": "detect", "size": "n"}

    def val(self, **kw):
        self.calls.append(kw)
        r = type("R", (), {})()
        r.box = _FakeBox()
        r.speed = {"preprocess": 1.0, "inference": 2.0, "loss": 0.0, "postprocess": 3.0}
        return r


def test_validate_schema_and_history(tmp_path):
    from core.validator import YOLO11Validator
    fm = _FakeModel()
    v = YOLO11Validator(fm, device="cpu", output_dir=str(tmp_path / "out"))
    out = v.validate("data.yaml", imgsz=320, batch=4)
    assert fm.calls[0]["data"] == "data.yaml" and fm.calls[0]["imgsz"] == 320 and fm.calls[0]["batch"] == 4
    assert fm.calls[0]["conf"] == 0.001 and fm.calls[0]["iou"] == 0.6  # the reference's defaults
    assert set(out) == {"timestamp", "validation_time_seconds", "device", "model_info", "box_metrics", "speed_metrics"}
    assert out["box_metrics"] == {"mAP50-95": 0.4, "mAP50": 0.6, "mAP75": 0.45, "precision": 0.7, "recall": 0.5}
    assert out["speed_metrics"]["inference"] == 2.0 and out["device"] == "cpu"
    assert out["model_info"] == {"task": "detect", "size": "n"}
    v.validate("data.yaml")
    assert len(v.validation_history) == 2 and v.validation_history[0] is out
    txt = (tmp_path / "out" / "validation_summary.txt").read_text()
    assert "mAP50-95: 0.4000" in txt and "inference: 2.0000" in txt


def test_model_surface_val_is_implemented_train_export_raise():
    from core.model import YOLO11Model
    assert YOLO11Model.val is not YOLO11Model.train and YOLO11Model.export is YOLO11Model.train
    m = YOLO11Model.__new__(YOLO11Model)
    for f in (m.train, m.export):
        with pytest.raises(NotImplementedError):
            f()
