"""CPU restatement of Ultralytics test-time augmentation for Detect models (8.3.x: nn/tasks.py
DetectionModel._predict_augment, _descale_pred, _clip_augmented; utils/torch_utils.py scale_img), on the oracle's
network and torch's own F.interpolate / F.pad.  TEST INFRASTRUCTURE ONLY.

    for s, f in zip((1, 0.83, 0.67), (None, 3, None)):
        xi = scale_img(x.flip(f) if f else x, s, gs=32)
        yi = forward(xi)                     # (B, 4 + nc, A_i), xywh in pass pixels
        yi[:, :4] /= s; if f == 3: yi[:, 0] = W - yi[:, 0]
    y0 = y0[..., :-(A_0 // 21)]; y2 = y2[..., (A_2 // 21) * 16:]
    y = cat((y0, y1, y2), -1)  ->  the usual non_max_suppression

dtype float64: the same steps in float64 on the float64 copy of the network (the de-scale divisor stays the float32
value of the ratio), for tests.matching.ref_f64_slack.
"""
from __future__ import annotations

import copy
import math
from typing import List, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from oracle import postprocess as pp
from tests.val_oracle import multi_label_nms

RATIOS = (1.0, 0.83, 0.67)
FLIPS = (None, 3, None)
PAD = 0.447


def scale_img(img: torch.Tensor, ratio: float, gs: int = 32) -> torch.Tensor:
    if ratio == 1.0:
        return img
    h, w = img.shape[2:]
    s = (int(h * ratio), int(w * ratio))
    img = F.interpolate(img, size=s, mode="bilinear", align_corners=False)
    h, w = (math.ceil(x * ratio / gs) * gs for x in (h, w))
    return F.pad(img, [0, w - s[1], 0, h - s[0]], value=PAD)


def pass_inputs(x: torch.Tensor, dtype=torch.float32) -> List[torch.Tensor]:
    """x: the batch as predict() receives it; the three passes' inputs after LoadTensor's /255 rule, resized in
    `dtype` arithmetic."""
    x = pp.load_tensor_check(x.float().cpu()).to(dtype)
    return [scale_img(x.flip(f) if f else x, s) for s, f in zip(RATIOS, FLIPS)]


def pass_shapes(H: int, W: int):
    """(Hs, Ws, hc, wc) per pass."""
    return [(H, W, H, W) if s == 1.0 else
            (math.ceil(H * s / 32) * 32, math.ceil(W * s / 32) * 32, int(H * s), int(W * s)) for s in RATIOS]


@torch.no_grad()
def merged_head(om, x: torch.Tensor, dtype=torch.float32) -> torch.Tensor:
    """(B, 4 + nc, Am): the augmented head of OracleModel `om` on batch x, in `dtype` arithmetic."""
    net = om.net
    if dtype == torch.float64:
        if getattr(om, "_net64", None) is None:
            om._net64 = copy.deepcopy(om.net).double()
        net = om._net64
    W = x.shape[3]
    ys = []
    for xi, s, f in zip(pass_inputs(x, dtype), RATIOS, FLIPS):
        y = net(xi)[0][0].clone()
        y[:, :4] /= float(np.float32(s)) if dtype == torch.float64 else s
        if f == 3:
            y[:, 0] = W - y[:, 0]
        ys.append(y)
    i = ys[0].shape[-1] // 21
    ys[0] = ys[0][..., :-i]
    i = (ys[-1].shape[-1] // 21) * 16
    ys[-1] = ys[-1][..., i:]
    return torch.cat(ys, -1)


def nms_rows(y: torch.Tensor, shape, conf=0.25, iou=0.7, classes: Optional[Sequence[int]] = None, agnostic=False,
             max_det=300, max_nms=30000) -> List[np.ndarray]:
    """Single-label non_max_suppression + scale_boxes onto the same shape (a clip): (n, 6) rows per image."""
    out = []
    for d in pp.non_max_suppression(y, conf, iou, classes, agnostic, max_det, max_nms=max_nms):
        d = d.clone()
        d[:, :4] = pp.scale_boxes(shape, d[:, :4], shape)
        out.append(d[:, :6].numpy())
    return out


def predict(om, x: torch.Tensor, dtype=torch.float32, **kw) -> List[np.ndarray]:
    return nms_rows(merged_head(om, x, dtype), tuple(x.shape[2:]), **kw)


def predict_multi_label(om, x: torch.Tensor, dtype=torch.float32, counts: Optional[list] = None, **kw):
    return multi_label_nms(merged_head(om, x, dtype), img_shape=tuple(x.shape[2:]), counts=counts, **kw)
