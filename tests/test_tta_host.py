"""Host-side checks of test-time augmentation (no GPU): the pass geometry, the C-ABI surface and the validator's
forwarding of `augment`."""
import os
import re

import pytest

from tests import tta_oracle
from yolomi import tta

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("hw, shapes, kept", [
    ((640, 640), [(640, 640, 640, 640), (544, 544, 531, 531), (448, 448, 428, 428)], [8000, 6069, 980]),
    ((320, 320), [(320, 320, 320, 320), (288, 288, 265, 265), (224, 224, 214, 214)], [2000, 1701, 245]),
    ((96, 160), [(96, 160, 96, 160), (96, 160, 79, 132), (96, 128, 64, 107)], [300, 315, 60]),
])
def test_pass_shapes_and_kept_anchors(hw, shapes, kept):
    assert tta.pass_shapes(*hw) == shapes == tta_oracle.pass_shapes(*hw)
    k = tta.kept_anchors(*hw)
    assert [n for _, n in k] == kept
    A = [tta.num_anchors(s[0], s[1]) for s in shapes]
    assert k[0] == (0, A[0] - A[0] // 21) and k[1] == (0, A[1]) and k[2] == ((A[2] // 21) * 16, A[2] - (A[2] // 21) * 16)
    # at these shapes the clipped tails are exactly pass 0's stride-32 level and the last pass's stride-8 level
    assert A[0] // 21 == (shapes[0][0] // 32) * (shapes[0][1] // 32)
    assert k[2][0] == (shapes[2][0] // 8) * (shapes[2][1] // 8)


def test_oracle_scaled_inputs_have_the_pass_shapes():
    import torch
    x = torch.rand(1, 3, 96, 160)
    xs = tta_oracle.pass_inputs(x)
    assert [tuple(t.shape[2:]) for t in xs] == [s[:2] for s in tta.pass_shapes(96, 160)]
    assert torch.equal(xs[0], x)
    hs, ws, hc, wc = tta.pass_shapes(96, 160)[2]
    pad = torch.tensor(0.447)
    assert (xs[2][..., hc:, :] == pad).all() and (xs[2][..., :, wc:] == pad).all()
    assert not (xs[2][..., :hc, :wc] == pad).all()


def test_new_symbols_in_header_and_binding():
    from yolomi.lib import EXPORTED
    hdr = open(os.path.join(ROOT, "include", "yolomi.h")).read()
    names = ("ym_tta_shape", "ym_tta_scale", "ym_tta_forward", "ym_tta_nms", "ym_tta_counts")
    for n in names:
        assert re.search(rf"\bint {n}\(", hdr), n
        assert n in EXPORTED, n
    # the argument block and the version did not move
    from yolomi.lib import InferArgs
    import ctypes
    assert ctypes.sizeof(InferArgs) == 88
    src = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "ym_runtime.cpp")).read()
    assert re.search(r"int ym_version\(void\) \{ return 1; \}", src)
    mk = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "Makefile")).read()
    assert "build/ym_tta.o" in mk


class _FakeModel:
    task, size = "detect", "n"

    def __init__(self):
        self.calls = []

    def get_model_info(self):
        return {"task": self.task, "size": self.size}

    def benchmark(self, *a, **k):
        return {}

    def val(self, **kw):
        self.calls.append(kw)

        class R:
            pass

        r, r.box = R(), R()
        r.box.map, r.box.map50, r.box.map75, r.box.mp, r.box.mr = 0.4, 0.6, 0.45, 0.7, 0.5
        r.speed = {"preprocess": 1.0, "inference": 2.0, "loss": 0.0, "postprocess": 3.0}
        return r


def test_validate_forwards_augment(tmp_path, caplog):
    import logging
    from core.validator import YOLO11Validator
    fm = _FakeModel()
    v = YOLO11Validator(fm, device="cpu", output_dir=str(tmp_path / "out"))
    with caplog.at_level(logging.INFO):
        out = v.validate("data.yaml", imgsz=320, batch=4, augment=True)
    assert fm.calls[0]["augment"] is True and fm.calls[0]["data"] == "data.yaml"
    assert not any("ignoring" in r.getMessage() and "augment" in r.getMessage() for r in caplog.records)
    v.validate("data.yaml")
    assert not fm.calls[1].get("augment", False)
    assert set(out) == {"timestamp", "validation_time_seconds", "device", "model_info", "box_metrics", "speed_metrics"}


@pytest.mark.parametrize("task, dtype, blob, word", [("detect", "i8", b"x", "quantized"), ("detect", "f8", b"x", "quantized"),
                                                     ("segment", "f32", b"x", "detect"), ("pose", "x3", b"x", "detect"),
                                                     ("detect", "x3", None, "blob")])
def test_unsupported_plans_say_so(task, dtype, blob, word):
    from yolomi.engine import Engine
    e = Engine.__new__(Engine)  # (no context: the checks come before any pass engine is created)
    e.task, e.dtype, e.blob, e._tta = task, dtype, blob, None
    with pytest.raises(ValueError, match=word):
        e._tta_engines()


def test_model_val_and_run_val_take_augment():
    import inspect
    from core.model import YOLO11Model
    from yolomi.val import run_val
    assert inspect.signature(YOLO11Model.val).parameters["augment"].default is False
    assert inspect.signature(run_val).parameters["augment"].default is False
