"""CPU restatement of the Ultralytics 8.3.x pose path (Pose head, kpts_decode, PosePredictor.postprocess, Keypoints)
on top of the oracle's YOLO11 graph.  TEST INFRASTRUCTURE ONLY.

Upstream: `nn/modules/head.py:Pose`, `models/yolo/pose/predict.py:PosePredictor.postprocess`,
`utils/ops.py:{scale_coords, clip_coords}`, `engine/results.py:Keypoints`.
"""
from __future__ import annotations

import copy
from typing import Dict, List

import torch
import torch.nn as nn

from oracle import postprocess as pp
from oracle.yolo11 import YOLO11, Conv, Detect, make_anchors


class Pose(Detect):
    def __init__(self, nc=1, kpt_shape=(17, 3), ch=()):
        super().__init__(nc, ch)
        self.kpt_shape = tuple(kpt_shape)
        self.nk = kpt_shape[0] * kpt_shape[1]
        c4 = max(ch[0] // 4, self.nk)
        self.cv4 = nn.ModuleList(nn.Sequential(Conv(x, c4, 3), Conv(c4, c4, 3), nn.Conv2d(c4, self.nk, 1)) for x in ch)

    def forward(self, x):
        bs = x[0].shape[0]
        kpt = torch.cat([self.cv4[i](x[i]).view(bs, self.nk, -1) for i in range(self.nl)], -1)
        # anchors / strides as Detect._inference makes them (from the level shapes, before Detect.forward rebinds x[i])
        self.anchors, self.strides = (t.transpose(0, 1) for t in make_anchors(x, self.stride, 0.5))
        y, feats = Detect.forward(self, x)
        return torch.cat([y, self.kpts_decode(bs, kpt)], 1), (feats, kpt)

    def kpts_decode(self, bs, kpts):
        ndim = self.kpt_shape[1]
        y = kpts.clone()
        if ndim == 3:
            y[:, 2::ndim] = y[:, 2::ndim].sigmoid()
        y[:, 0::ndim] = (y[:, 0::ndim] * 2.0 + (self.anchors[0] - 0.5)) * self.strides
        y[:, 1::ndim] = (y[:, 1::ndim] * 2.0 + (self.anchors[1] - 0.5)) * self.strides
        return y


def build_pose(scale="n", state_dict=None, nc=1, kpt_shape=(17, 3)) -> YOLO11:
    """YOLO11(scale, "detect", nc) with layer 23 replaced by the Pose head; strict load, fused."""
    m = YOLO11(scale, "detect", nc)
    det = m.model[23]
    ch = [seq[0].conv.in_channels for seq in det.cv2]
    m.model[23] = Pose(nc, kpt_shape, ch)
    m.task = "pose"
    m = m.eval().requires_grad_(False)
    if state_dict is not None:
        m.load_state_dict({k: torch.as_tensor(v) for k, v in state_dict.items()}, strict=True)
    return m.fuse().requires_grad_(False)


def scale_coords(img1_shape, coords, img0_shape):
    """ops.scale_coords (padding=True, normalize=False) + clip_coords, in place."""
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    pad = (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1),
           round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))
    coords[..., 0] -= pad[0]
    coords[..., 1] -= pad[1]
    coords[..., 0] /= gain
    coords[..., 1] /= gain
    coords[..., 0] = coords[..., 0].clamp(0, img0_shape[1])
    coords[..., 1] = coords[..., 1].clamp(0, img0_shape[0])
    return coords


def keypoints_mask(data: torch.Tensor) -> torch.Tensor:
    """Keypoints.__init__: x, y of a keypoint with visibility < 0.5 are zeroed (a copy)."""
    data = data.clone()
    if data.shape[-1] == 3:
        mask = data[..., 2] < 0.5
        data[..., :2][mask] = 0
    return data


class PoseOracle:
    def __init__(self, scale: str, state_dict: Dict, nc: int = 1, kpt_shape=(17, 3)):
        self.scale, self.nc, self.kpt_shape = scale, nc, tuple(kpt_shape)
        self.net = build_pose(scale, state_dict, nc, kpt_shape)
        self._net64 = None

    @torch.no_grad()
    def raw(self, im: torch.Tensor):
        """(preprocessed input, y (B, 4 + nc + nk, A), dict(feats, kpt = raw cv4 output (B, nk, A)))."""
        im = pp.load_tensor_check(im.float().cpu()).float()
        (y, (feats, kpt)), _ = self.net(im)
        return im, y, dict(feats=feats, kpt=kpt)

    def _post(self, y, shape, orig_shape, conf, iou, max_det, mask=True) -> List[Dict]:
        out = []
        for d in pp.non_max_suppression(y, conf, iou, None, False, max_det, nc=self.nc):
            d = d.clone()
            d[:, :4] = pp.scale_boxes(shape, d[:, :4], orig_shape)
            k = d[:, 6:].reshape(len(d), *self.kpt_shape).clone()
            k = scale_coords(shape, k, orig_shape)
            out.append({"boxes": d[:, :6], "kpts_raw": k, "keypoints": keypoints_mask(k) if mask else k})
        return out

    @torch.no_grad()
    def predict(self, im, conf=0.25, iou=0.7, max_det=300, orig_shape=None) -> List[Dict]:
        """Per image: boxes (n, 6), kpts_raw (n, K, ndim) scaled and clipped, keypoints = kpts_raw masked as the
        Keypoints view does.  orig_shape: map back to an original image (letterboxed input), else the input's own."""
        im, y, _ = self.raw(im)
        shape = tuple(im.shape[2:])
        return self._post(y, shape, orig_shape or shape, conf, iou, max_det)

    @torch.no_grad()
    def predict_exact(self, im, conf=0.25, iou=0.7, max_det=300, orig_shape=None) -> List[Dict]:
        """The same graph and weights in float64 (oracle/predict.py predict_exact), same NMS, scaling and clip."""
        if self._net64 is None:
            self._net64 = copy.deepcopy(self.net).double()
        x = pp.load_tensor_check(im.float().cpu()).double()
        (y, _), _ = self._net64(x)
        shape = tuple(x.shape[2:])
        return self._post(y, shape, orig_shape or shape, conf, iou, max_det)
