"""CPU tests of the OBB rules (tests/obb_oracle.py), the plan's task inference and the facade contract."""
import math

import numpy as np
import pytest
import torch

from tests.obb_oracle import EPS, corners, probiou, regularize
from yolomi.arch import GraphBuilder, infer_arch
from yolomi.synth import synth_weights


def _p(a, b):
    return float(probiou(np.array([a], np.float64), np.array([b], np.float64))[0, 0])


def test_probiou_known_answers():
    """A box against itself: sums 2A, 2B, 2C, t1 = t2 = 0, det = 4 (AB - C²) = 4 sqrt(d1 d2), so t3 = 0.5 log(1 + ~eps)
    < eps and bd clamps to eps: probiou = 1 - sqrt(1 - exp(-eps) + eps) = 1 - sqrt(eps + eps) to first order.
    theta and theta + pi: cos² and sin² and cos sin are unchanged, so (A, B, C) and the value are.
    A square: a' = b', so A = B = a', C = 0 at any theta.
    Far apart (dx = 1000, 10 px squares: a' = 8.33, t1 = 0.25 * 16.7 * 1e6 / 278 = 1.5e4): bd clamps to 100,
    probiou = 1 - sqrt(1 - exp(-100) + eps) = 1 - sqrt(1 + eps) (slightly below 0)."""
    box = [50.0, 40.0, 30.0, 8.0, 0.3]
    assert _p(box, box) == pytest.approx(1 - math.sqrt(EPS + EPS), abs=1e-9)
    other = [57.0, 44.0, 20.0, 12.0, 1.1]
    assert _p(box, other) == pytest.approx(_p(box[:4] + [0.3 + math.pi], other), abs=1e-12)
    sq = [50.0, 40.0, 10.0, 10.0]
    assert _p(sq + [0.0], other) == pytest.approx(_p(sq + [0.7], other), abs=1e-12)
    assert _p(sq + [0.0], [1050.0, 40.0, 10.0, 10.0, 0.0]) == pytest.approx(1 - math.sqrt(1 + EPS), abs=1e-15)


def test_regularize_and_corner_order():
    """(10, 20, w 2, h 4, theta 0): w <= h, so w and h swap and theta becomes pi / 2.  Then v1 = (w / 2)(cos, sin) =
    (0, 2) and v2 = (h / 2)(-sin, cos) = (-1, 0): corners (9, 22), (11, 22), (11, 18), (9, 18)."""
    rb = regularize(np.array([[10.0, 20.0, 2.0, 4.0, 0.0]]))
    assert rb.tolist() == [[10.0, 20.0, 4.0, 2.0, math.pi / 2]]
    want = [[9, 22], [11, 22], [11, 18], [9, 18]]
    assert np.allclose(corners(rb)[0], want, atol=1e-12)
    from core.results import OBB, obb_rows_to_results
    data = obb_rows_to_results(torch.tensor([[10.0, 20.0, 2.0, 4.0, 0.9, 3.0, 0.0]], dtype=torch.float64))
    obb = OBB(data, (40, 40))
    assert data[0].tolist() == [10.0, 20.0, 4.0, 2.0, math.pi / 2, 0.9, 3.0]
    assert np.allclose(obb.xyxyxyxy[0].numpy(), want, atol=1e-12)
    assert np.allclose(obb.numpy().xyxy, [[9, 18, 11, 22]], atol=1e-12) and len(obb) == 1
    assert float(obb.conf[0]) == 0.9 and float(obb.cls[0]) == 3.0 and obb.xyxyxyxyn[0, 0].tolist() == [9 / 40, 22 / 40]


def test_infer_arch_tells_obb_from_pose():
    assert infer_arch(synth_weights("n", "obb", 0)) == ("n", "obb", 15)
    assert infer_arch(synth_weights("s", "obb", 1, nc=3)) == ("s", "obb", 3)
    assert infer_arch(synth_weights("n", "pose", 0))[1] == "pose"
    g = GraphBuilder("n", "obb")
    assert (g.nm, g.no, g.anchor_buf.C) == (1, 80, 84)
    with pytest.raises(ValueError):
        GraphBuilder("n", "obb", quant=True)


def test_weights_decide_the_task():
    """A bare task="obb" raises as before; with weights the request gets past the task check (and, on a host without
    the GPU, as far as the device check)."""
    from core.model import YOLO11Model
    with pytest.raises(NotImplementedError):
        YOLO11Model(task="obb", device="cpu", verbose=False)
    with pytest.raises(RuntimeError, match="MI355X"):
        YOLO11Model(task="obb", device="cpu", verbose=False, state_dict=synth_weights("n", "obb", 0))
