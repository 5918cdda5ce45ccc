"""Generate the pose golden fixture from the CPU restatement (tests/pose_oracle.py).

    python tests/golden/make_pose_golden.py

pose_n_uniform.json: yolo11n-pose (nc 1, kpt_shape (17, 3), synthetic weights seed 0), 2 x U[0,1) 320x320 (seeds 8101,
8102), conf 0.25 iou 0.7: per image the NMS rows [x1 y1 x2 y2 conf cls | 17 x (x, y, v)] with boxes and keypoints
clipped to the image (scale_boxes / scale_coords with equal shapes) and the keypoints NOT masked by visibility, and
checksums / samples of the raw head output (B, A, 64 + nc + nk: box bins, class logit, raw keypoints).
"""
from __future__ import annotations

import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "yolo-infer_amd"))
sys.path.insert(0, ROOT)

from tests.golden.make_golden import layer_stats, make_input  # noqa: E402
from tests.pose_oracle import PoseOracle  # noqa: E402
from yolomi.synth import synth_weights  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
SEEDS, SIZE, CONF, IOU = (8101, 8102), 320, 0.25, 0.7


def head_rows(ex, B: int) -> torch.Tensor:
    """(B, A, 64 + nc + nk): the head's raw output per anchor, levels concatenated (the GPU's anchor rows minus pads)."""
    det = torch.cat([f.view(B, f.shape[1], -1) for f in ex["feats"]], 2)
    return torch.cat([det, ex["kpt"]], 1).transpose(1, 2)


def pose_fixture(scale="n"):
    om = PoseOracle(scale, synth_weights(scale, "pose", 0))
    x = make_input("uniform", SEEDS, SIZE)
    _, _, ex = om.raw(x)
    res = om.predict(x, conf=CONF, iou=IOU)
    rows = [torch.cat([r["boxes"], r["kpts_raw"].reshape(len(r["boxes"]), -1)], 1).tolist() for r in res]
    return {
        "scale": scale, "task": "pose", "nc": 1, "kpt_shape": [17, 3], "weights_seed": 0,
        "input": {"kind": "uniform", "seeds": list(SEEDS), "size": SIZE}, "conf": CONF, "iou": IOU, "max_det": 300,
        "head": layer_stats(head_rows(ex, x.shape[0])), "nms_rows": rows,
    }


if __name__ == "__main__":
    fx = pose_fixture("n")
    assert all(5 <= len(r) < 300 for r in fx["nms_rows"]), [len(r) for r in fx["nms_rows"]]
    with open(os.path.join(HERE, "pose_n_uniform.json"), "w") as f:
        json.dump(fx, f)
    print("pose_n_uniform.json:", [len(r) for r in fx["nms_rows"]], "rows")
