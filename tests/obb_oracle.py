"""CPU restatement of the Ultralytics 8.3.x OBB path on top of the oracle's YOLO11 graph.  TEST INFRASTRUCTURE ONLY.

Upstream: `nn/modules/head.py:OBB`, `utils/tal.py:dist2rbox`, `utils/ops.py:{non_max_suppression(rotated=True),
nms_rotated, regularize_rboxes, scale_boxes(xywh=True), xywhr2xyxyxyxy}`, `utils/metrics.py:batch_probiou`,
`models/yolo/obb/predict.py:OBBPredictor`.  The numpy functions take any float dtype: float64 is the reference the
GPU tests hold the kernels to.
"""
from __future__ import annotations

import copy
import math
from typing import Dict, List

import numpy as np
import torch
import torch.nn as nn

from oracle import postprocess as pp
from oracle.yolo11 import YOLO11, Conv, Detect, make_anchors

EPS = 1e-7


def covariance(w, h, t):
    """_get_covariance_matrix: (A, B, C) of boxes (w, h, theta)."""
    a, b = w * w / 12.0, h * h / 12.0
    c, s = np.cos(t), np.sin(t)
    return a * c * c + b * s * s, a * s * s + b * c * c, (a - b) * c * s


def probiou(b1, b2):
    """batch_probiou of (n, 5) against (m, 5) boxes (x, y, w, h, theta): (n, m)."""
    x1, y1 = b1[:, 0:1], b1[:, 1:2]
    x2, y2 = b2[None, :, 0], b2[None, :, 1]
    A1, B1, C1 = (v[:, None] for v in covariance(b1[:, 2], b1[:, 3], b1[:, 4]))
    A2, B2, C2 = (v[None, :] for v in covariance(b2[:, 2], b2[:, 3], b2[:, 4]))
    sA, sB, sC = A1 + A2, B1 + B2, C1 + C2
    den = sA * sB - sC ** 2 + EPS
    t1 = (sA * (y1 - y2) ** 2 + sB * (x1 - x2) ** 2) / den * 0.25
    t2 = (sC * (x2 - x1) * (y1 - y2)) / den * 0.5
    d1 = np.clip(A1 * B1 - C1 ** 2, 0, None)
    d2 = np.clip(A2 * B2 - C2 ** 2, 0, None)
    t3 = 0.5 * np.log((sA * sB - sC ** 2) / (4 * np.sqrt(d1 * d2) + EPS) + EPS)
    bd = np.clip(t1 + t2 + t3, EPS, 100.0)
    return 1.0 - np.sqrt(1.0 - np.exp(-bd) + EPS)


def offset_boxes(boxes, cls, agnostic, max_wh):
    """(n, 5) float64 NMS boxes: the class offset added to x in fp32, as the GPU and torch do."""
    x = boxes[:, 0].astype(np.float32)
    if not agnostic:
        x = x + cls.astype(np.float32) * np.float32(max_wh)
    return np.concatenate([x.astype(np.float64)[:, None], boxes[:, 1:5].astype(np.float64)], 1)


def fast_nms(boxes, scores, cls, anchors, conf, iou, max_det=300, max_nms=30000, agnostic=False, max_wh=7680.0):
    """non_max_suppression(rotated=True) of one image from decoded candidates: boxes (A, 5) (cx, cy, w, h, theta),
    scores / cls / anchor indices (A,).  Returns (kept indices into the inputs in score order, the sorted order, the
    (n, n) probiou of the sorted offset boxes)."""
    cand = np.flatnonzero(scores > conf)
    order = cand[np.lexsort((anchors[cand], -scores[cand].astype(np.float64)))][:max_nms]
    nb = offset_boxes(boxes[order], cls[order], agnostic, max_wh)
    p = np.triu(probiou(nb, nb), 1)
    keep = p.max(0, initial=0.0) < iou if len(order) else np.zeros(0, bool)
    return order[keep][:max_det], order, p


def regularize(rb):
    """regularize_rboxes on (n, >= 5) rows (x, y, w, h, theta): w >= h, theta in [0, pi)."""
    x, y, w, h, t = (rb[:, i] for i in range(5))
    swap = w <= h
    w_, h_ = np.where(swap, h, w), np.where(swap, w, h)
    t = np.where(swap, t + math.pi / 2, t) % math.pi
    return np.stack([x, y, w_, h_, t], 1)


def corners(rb):
    """xywhr2xyxyxyxy: (n, 4, 2) corners ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2."""
    ctr = rb[:, :2]
    c, s = np.cos(rb[:, 4]), np.sin(rb[:, 4])
    v1 = np.stack([rb[:, 2] / 2 * c, rb[:, 2] / 2 * s], 1)
    v2 = np.stack([-rb[:, 3] / 2 * s, rb[:, 3] / 2 * c], 1)
    return np.stack([ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2], 1)


def scale_xywh(rb, shape, orig_shape):
    """scale_boxes(xywh=True): the pad off the centre, all four by the gain, no clip (a copy)."""
    gain = min(shape[0] / orig_shape[0], shape[1] / orig_shape[1])
    pad = (round((shape[1] - orig_shape[1] * gain) / 2 - 0.1), round((shape[0] - orig_shape[0] * gain) / 2 - 0.1))
    rb = rb.copy()
    rb[:, 0] -= pad[0]
    rb[:, 1] -= pad[1]
    rb[:, :4] /= gain
    return rb


def decode(rows, H, W, nc, cls_pad):
    """dist2rbox of head rows (A, 64 + cls_pad + >= 1) [DFL | cls | angle logit] in the rows' dtype:
    (boxes (A, 5), scores (A,), cls (A,))."""
    f = rows.dtype.type
    pts, st = [], []
    for s in (8, 16, 32):
        yy, xx = np.meshgrid(np.arange(H // s), np.arange(W // s), indexing="ij")
        pts.append(np.stack([xx.ravel() + 0.5, yy.ravel() + 0.5], 1))
        st.append(np.full(xx.size, s))
    pts, st = np.concatenate(pts).astype(rows.dtype), np.concatenate(st).astype(rows.dtype)
    d = rows[:, :64].reshape(-1, 4, 16)
    e = np.exp(d - d.max(2, keepdims=True))
    l, t, r, b = ((e * np.arange(16, dtype=rows.dtype)).sum(2) / e.sum(2)).T
    th = (f(1) / (f(1) + np.exp(-rows[:, 64 + cls_pad])) - f(0.25)) * f(math.pi)
    xf, yf = (r - l) / 2, (b - t) / 2
    c, s = np.cos(th), np.sin(th)
    boxes = np.stack([(xf * c - yf * s + pts[:, 0]) * st, (xf * s + yf * c + pts[:, 1]) * st, (l + r) * st,
                      (t + b) * st, th], 1)
    sc = 1 / (1 + np.exp(-rows[:, 64:64 + nc]))
    return boxes, sc.max(1), sc.argmax(1)


class OBB(Detect):
    def __init__(self, nc=15, ne=1, ch=()):
        super().__init__(nc, ch)
        self.ne = ne
        c4 = max(ch[0] // 4, ne)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, ne, 1)) for x in ch)

    def forward(self, x):
        bs = x[0].shape[0]
        ang = torch.cat([self.cv4[i](x[i]).view(bs, self.ne, -1) for i in range(self.nl)], 2)
        feats = [torch.cat((self.cv2[i](x[i]), self.cv3[i](x[i])), 1) for i in range(self.nl)]
        return torch.cat([f.view(bs, self.no, -1) for f in feats], 2), ang  # (B, 64 + nc, A) logits, (B, 1, A)


def build_obb(scale="n", state_dict=None, nc=15) -> YOLO11:
    m = YOLO11(scale, "detect", nc)
    ch = [seq[0].conv.in_channels for seq in m.model[23].cv2]
    m.model[23] = OBB(nc, 1, ch)
    m.task = "obb"
    m = m.eval().requires_grad_(False)
    if state_dict is not None:
        m.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict.items()}, strict=True)
    return m.fuse().requires_grad_(False)


class ObbOracle:
    def __init__(self, scale: str, state_dict: Dict, nc: int = 15):
        self.nc = nc
        self.net = build_obb(scale, state_dict, nc)
        self._net64 = None

    @torch.no_grad()
    def head_rows(self, im: torch.Tensor, exact=False) -> np.ndarray:
        """(B, A, 64 + nc + 1) raw head rows [DFL | cls | angle] (fp32, or the float64 evaluation of the graph)."""
        x = pp.load_tensor_check(im.float().cpu())
        if exact:
            if self._net64 is None:
                self._net64 = copy.deepcopy(self.net).double()
            (y, ang), _ = self._net64(x.double())
        else:
            (y, ang), _ = self.net(x.float())
        return torch.cat([y, ang], 1).transpose(1, 2).contiguous().numpy()

    def predict(self, im, conf=0.25, iou=0.7, max_det=300, exact=False, orig_shape=None) -> List[np.ndarray]:
        """Per image the (n, 7) rows [cx, cy, w, h, conf, cls, theta] as OBBPredictor leaves them: regularised, in the
        pixels of orig_shape (default: the input's own)."""
        H, W = im.shape[2:]
        out = []
        for rows in self.head_rows(im, exact):
            boxes, sc, cl = decode(rows, H, W, self.nc, self.nc)
            keep, _, _ = fast_nms(boxes, sc, cl, np.arange(len(sc)), conf, iou, max_det)
            rb = scale_xywh(regularize(boxes[keep]), (H, W), orig_shape or (H, W))
            out.append(np.concatenate([rb[:, :4], sc[keep, None], cl[keep, None].astype(rb.dtype), rb[:, 4:5]], 1))
        return out
