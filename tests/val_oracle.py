"""CPU restatement of Ultralytics `utils/ops.py:non_max_suppression(..., multi_label=True)` (8.3.x), the validator's
post-processing.  TEST INFRASTRUCTURE ONLY (the single-label restatement is oracle/postprocess.py).

Per image:
    i, j = where(cls_scores > conf)          strict >, row-major: anchor-major, class-minor
    x = [box[i], cls_scores[i, j], j]        the anchor's box repeated for each of its classes
    classes filter; if n > max_nms: x = x[stable argsort by score, descending][:max_nms]
    keep = nms(box + cls * (0 if agnostic else max_wh), score, iou)[:max_det]
The greedy NMS is torchvision's CPU kernel (oracle.postprocess.nms_greedy's arithmetic: fp32 areas and IoU with one
rounding per operation, suppress iff double(IoU) > iou), vectorised per kept box and stopped once max_det boxes are
kept — greedy keeps in score order, so the first max_det kept boxes are nms(...)[:max_det].
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch

from oracle.postprocess import xywh2xyxy


def nms_greedy_np(boxes: np.ndarray, scores: np.ndarray, iou_thres: float, max_keep: int) -> np.ndarray:
    """Indices kept by torchvision.ops.nms (stable descending sort, greedy, IoU > thr), at most max_keep of them."""
    n = len(boxes)
    if n == 0:
        return np.zeros(0, np.int64)
    order = np.argsort(-scores, kind="stable")
    b = boxes[order]
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    areas = (x2 - x1) * (y2 - y1)  # in the boxes' dtype (fp32 for the fp32 head output)
    alive = np.ones(n, bool)
    keep = []
    for i in range(n):
        if not alive[i]:
            continue
        keep.append(i)
        if len(keep) >= max_keep:
            break
        r = np.nonzero(alive[i + 1:])[0] + i + 1
        if not len(r):
            continue
        w = np.maximum(np.minimum(x2[r], x2[i]) - np.maximum(x1[r], x1[i]), 0)
        h = np.maximum(np.minimum(y2[r], y2[i]) - np.maximum(y1[r], y1[i]), 0)
        inter = w * h
        ovr = inter / ((areas[i] + areas[r]) - inter)
        alive[r[ovr.astype(np.float64) > iou_thres]] = False
    return order[np.asarray(keep, np.int64)]


def multi_label_nms(prediction: torch.Tensor, conf=0.001, iou=0.7, classes: Optional[Sequence[int]] = None,
                    agnostic=False, max_det=300, max_nms=30000, max_wh=7680.0, img_shape=None,
                    counts: Optional[list] = None) -> List[np.ndarray]:
    """prediction: (B, 4 + nc, A) head output (xywh + class scores), fp32 — or float64 (the oracle's float64 evaluation),
    then every step runs in float64.  Returns per image the (n, 6) rows (the prediction's dtype)
    [x1, y1, x2, y2, score, cls] in keep order, clipped to img_shape (h, w) when given (the predictor's scale_boxes
    onto the same shape is a clip).  counts, when a list, receives the per-image pair counts before the max_nms cut."""
    out = []
    dt = np.float64 if prediction.dtype == torch.float64 else np.float32
    pred = (prediction if dt == np.float64 else prediction.float()).transpose(-1, -2)  # (B, A, 4 + nc)
    for x in pred:
        box = xywh2xyxy(x[:, :4]).numpy()
        cls = x[:, 4:].numpy()
        i, j = np.nonzero(cls > dt(conf))  # row-major: anchor-major, class-minor
        if classes is not None:
            m = np.isin(j, np.asarray(list(classes)))
            i, j = i[m], j[m]
        if counts is not None:
            counts.append(int(len(i)))
        score = cls[i, j]
        if len(i) > max_nms:
            o = np.argsort(-score, kind="stable")[:max_nms]
            i, j, score = i[o], j[o], score[o]
        b = box[i]
        off = (j.astype(dt) * dt(0.0 if agnostic else max_wh))[:, None]
        keep = nms_greedy_np(b + off, score, iou, max_det)
        rows = np.concatenate([b[keep], score[keep, None], j[keep, None].astype(dt)], 1).astype(dt)
        if img_shape is not None and len(rows):
            rows[:, [0, 2]] = rows[:, [0, 2]].clip(0, img_shape[1])
            rows[:, [1, 3]] = rows[:, [1, 3]].clip(0, img_shape[0])
        out.append(rows.reshape(-1, 6))
    return out
