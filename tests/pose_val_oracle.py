"""Torch fp32 restatement of the Ultralytics 8.3.x pose validator's matching: `utils/metrics.py:kpt_iou / OKS_SIGMA`,
`models/yolo/pose/val.py:PoseValidator._process_batch` and `engine/validator.py:BaseValidator.match_predictions`
(the non-scipy branch).  TEST INFRASTRUCTURE ONLY.

Written from the upstream sources as remembered (the package is not available offline): the
tensors are fp32 and the ten thresholds are `torch.linspace(0.5, 0.95, 10)`, as upstream has them, where
yolomi/metrics.py works in float64.
"""
from __future__ import annotations

import numpy as np
import torch

OKS_SIGMA = (np.array([0.26, 0.25, 0.25, 0.35, 0.35, 0.79, 0.79, 0.72, 0.72, 0.62, 0.62, 1.07, 1.07, 0.87, 0.87, 0.89,
                       0.89]) / 10.0)
IOUV = torch.linspace(0.5, 0.95, 10)


def box_iou(box1: torch.Tensor, box2: torch.Tensor, eps: float = 1e-7) -> torch.Tensor:
    """metrics.box_iou: (N, 4), (M, 4) xyxy → (N, M)."""
    (a1, a2), (b1, b2) = box1.float().unsqueeze(1).chunk(2, 2), box2.float().unsqueeze(0).chunk(2, 2)
    inter = (torch.min(a2, b2) - torch.max(a1, b1)).clamp_(0).prod(2)
    return inter / ((a2 - a1).prod(2) + (b2 - b1).prod(2) - inter + eps)


def kpt_iou(kpt1: torch.Tensor, kpt2: torch.Tensor, area: torch.Tensor, sigma, eps: float = 1e-7) -> torch.Tensor:
    """metrics.kpt_iou: kpt1 (N, K, 3) ground truth, kpt2 (M, K, 2 | 3) predictions, area (N,), sigma K values →
    (N, M) object keypoint similarity."""
    d = (kpt1[:, None, :, 0] - kpt2[..., 0]).pow(2) + (kpt1[:, None, :, 1] - kpt2[..., 1]).pow(2)  # (N, M, K)
    sigma = torch.tensor(sigma, device=kpt1.device, dtype=kpt1.dtype)  # (K,)
    kpt_mask = kpt1[..., 2] != 0  # (N, K)
    e = d / ((2 * sigma).pow(2) * (area[:, None, None] + eps) * 2)
    return ((-e).exp() * kpt_mask[:, None]).sum(-1) / (kpt_mask.sum(-1)[:, None] + eps)


def match_predictions(pred_classes: torch.Tensor, true_classes: torch.Tensor, iou: torch.Tensor) -> torch.Tensor:
    """BaseValidator.match_predictions(use_scipy=False): (n,), (m,), iou (m, n) → correct (n, 10) bool."""
    correct = np.zeros((pred_classes.shape[0], IOUV.shape[0])).astype(bool)
    correct_class = true_classes[:, None] == pred_classes
    iou = (iou * correct_class).cpu().numpy()
    for i, threshold in enumerate(IOUV.tolist()):
        matches = np.array(np.nonzero(iou >= threshold)).T
        if matches.shape[0]:
            if matches.shape[0] > 1:
                matches = matches[iou[matches[:, 0], matches[:, 1]].argsort()[::-1]]
                matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
            correct[matches[:, 1].astype(int), i] = True
    return torch.tensor(correct, dtype=torch.bool)


def xyxy2xywh(x: torch.Tensor) -> torch.Tensor:
    y = torch.empty_like(x)
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def process_batch(detections: torch.Tensor, gt_bboxes: torch.Tensor, gt_cls: torch.Tensor, pred_kpts=None,
                  gt_kpts=None, sigma=OKS_SIGMA) -> torch.Tensor:
    """PoseValidator._process_batch: detections (n, 6) [xyxy, conf, cls], gt_bboxes (m, 4), gt_cls (m,); with
    pred_kpts (n, K, ndim) and gt_kpts (m, K, 3) the matches are made on OKS (area = 0.53 · w · h of the ground-truth
    box), else on box IoU.  Returns correct (n, 10) bool."""
    if pred_kpts is not None and gt_kpts is not None:
        area = xyxy2xywh(gt_bboxes)[:, 2:].prod(1) * 0.53
        iou = kpt_iou(gt_kpts, pred_kpts, sigma=sigma, area=area)
    else:
        iou = box_iou(gt_bboxes, detections[:, :4])
    return match_predictions(detections[:, 5], gt_cls, iou)
