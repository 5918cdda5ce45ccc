"""Offline detection and pose metrics: mAP50 / mAP50-95, precision / recall, OKS keypoint mAP.

Semantics of the numbers the reference reads from Ultralytics val (`core/validator.py:339-352`:
`results.box.map`, `.map50`, `.map75`, `.mp`, `.mr`): per class, predictions sorted by confidence, a prediction is
a TP at IoU threshold t as upstream `BaseValidator.match_predictions` decides it (ultralytics 8.3.x,
engine/validator.py); AP = area under the 101-point COCO-interpolated precision envelope; mAP = mean over classes
present in the ground truth, mAP50-95 = mean over t ∈ {0.50, 0.55, ..., 0.95}.  Precision / recall (`.mp`, `.mr`) are
upstream `ap_per_class`'s: per class the IoU-0.5 precision and recall curves over a 1000-point confidence grid, read at
the confidence that maximises the smoothed class-mean F1, then averaged over classes.

Pose (`evaluate_pose`, upstream `PoseValidator._process_batch` / `PoseMetrics`): the same matching rule and AP applied
twice to the same predictions, once with box IoU and once with the object keypoint similarity `kpt_iou` in its place.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np

IOUV = np.linspace(0.5, 0.95, 10)
# upstream utils/metrics.py OKS_SIGMA: the COCO per-keypoint constants of the 17-keypoint person skeleton
OKS_SIGMA = np.array([.26, .25, .25, .35, .35, .79, .79, .72, .72, .62, .62, 1.07, 1.07, .87, .87, .89, .89]) / 10.0


def box_iou(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    if len(a) == 0 or len(b) == 0:
        return np.zeros((len(a), len(b)))
    lt = np.maximum(a[:, None, :2], b[None, :, :2])
    rb = np.minimum(a[:, None, 2:4], b[None, :, 2:4])
    inter = np.clip(rb - lt, 0, None).prod(2)
    aa = (a[:, 2:4] - a[:, :2]).prod(1)
    ab = (b[:, 2:4] - b[:, :2]).prod(1)
    return inter / np.maximum(aa[:, None] + ab[None] - inter, 1e-9)


def kpt_iou(gt_kpts: np.ndarray, pred_kpts: np.ndarray, area: np.ndarray, sigma: np.ndarray,
            eps: float = 1e-7) -> np.ndarray:
    """Upstream metrics.kpt_iou in float64: the object keypoint similarity of gt_kpts (m, K, 3) [x, y, visibility]
    against pred_kpts (n, K, 2 | 3), area (m,) the ground truths' areas, sigma (K,) → (m, n).

    d = dx² + dy², e = d / ((2σ)² · (area + eps) · 2), OKS = Σ_k exp(−e) [v_gt ≠ 0] / (Σ_k [v_gt ≠ 0] + eps): a keypoint
    the ground truth does not label counts on neither side, and a ground truth without labelled keypoints has OKS 0."""
    g = np.asarray(gt_kpts, np.float64)
    p = np.asarray(pred_kpts, np.float64)
    if len(g) == 0 or len(p) == 0:
        return np.zeros((len(g), len(p)))
    sigma = np.asarray(sigma, np.float64)
    area = np.asarray(area, np.float64)
    d = (g[:, None, :, 0] - p[None, :, :, 0]) ** 2 + (g[:, None, :, 1] - p[None, :, :, 1]) ** 2  # (m, n, K)
    mask = g[..., 2] != 0  # (m, K)
    e = d / ((2 * sigma) ** 2 * (area[:, None, None] + eps) * 2)
    return (np.exp(-e) * mask[:, None]).sum(-1) / (mask.sum(-1)[:, None] + eps)


def match_iou(iou: np.ndarray, pred_cls: np.ndarray, gt_cls: np.ndarray) -> np.ndarray:
    """iou (m, n): similarity of m ground truths and n predictions (NMS, i.e. confidence-descending, order), pred_cls
    (n,), gt_cls (m,) → TP (n, 10) bool.

    Upstream's non-scipy branch: the (gt, pred) pairs with IoU >= t and equal class, sorted by IoU descending; keep
    each prediction's best pair (np.unique on the prediction index, which leaves the pairs in prediction-index
    order); then each ground truth keeps its FIRST remaining pair in that order — the lowest prediction index, i.e.
    the most confident prediction, not the highest IoU (upstream's re-sort by IoU between the two steps is commented
    out).  Equal IoUs: upstream's `argsort()[::-1]` leaves their order to numpy's quicksort; here it is stable."""
    tp = np.zeros((len(pred_cls), len(IOUV)), bool)
    if len(pred_cls) == 0 or len(gt_cls) == 0:
        return tp
    iou = iou * (np.asarray(gt_cls)[:, None] == np.asarray(pred_cls)[None, :])
    for k, t in enumerate(IOUV):
        m = np.argwhere(iou >= t)
        if len(m):
            if len(m) > 1:
                v = iou[m[:, 0], m[:, 1]]
                m = m[np.argsort(-v, kind="stable")]
                m = m[np.unique(m[:, 1], return_index=True)[1]]
                m = m[np.unique(m[:, 0], return_index=True)[1]]
            tp[m[:, 1], k] = True
    return tp


def match_predictions(pred: np.ndarray, gt: np.ndarray) -> np.ndarray:
    """pred (n,6) [xyxy,conf,cls] in NMS (confidence-descending) order, gt (m,6) [xyxy,-,cls] → TP (n, 10) bool:
    match_iou on the boxes' IoU."""
    if len(pred) == 0 or len(gt) == 0:
        return np.zeros((len(pred), len(IOUV)), bool)
    return match_iou(box_iou(gt[:, :4], pred[:, :4]), pred[:, 5], gt[:, 5])


def compute_ap(recall: np.ndarray, precision: np.ndarray) -> float:
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    y = np.interp(x, mrec, mpre)
    return float(((y[1:] + y[:-1]) / 2 * np.diff(x)).sum())


def smooth(y: np.ndarray, f: float = 0.05) -> np.ndarray:
    """Upstream metrics.smooth: box filter of fraction f (odd length), the ends padded with the end values."""
    nf = round(len(y) * f * 2) // 2 + 1
    p = np.ones(nf // 2)
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def precision_recall(tp50: np.ndarray, conf: np.ndarray, pc: np.ndarray, gc: np.ndarray):
    """Upstream ap_per_class's (mp, mr): tp50 (n,) bool at IoU 0.5, conf / pc (n,) sorted by confidence descending,
    gc the ground-truth classes.  A class without predictions has precision and recall 0."""
    classes = np.unique(gc)
    if len(classes) == 0:
        return 0.0, 0.0
    px = np.linspace(0, 1, 1000)
    p_curve = np.zeros((len(classes), 1000))
    r_curve = np.zeros((len(classes), 1000))
    for ci, c in enumerate(classes):
        sel = pc == c
        n_gt = int((gc == c).sum())
        if sel.sum() == 0 or n_gt == 0:
            continue
        tpc = tp50[sel].astype(np.float64).cumsum()
        fpc = (1 - tp50[sel].astype(np.float64)).cumsum()
        recall = tpc / (n_gt + 1e-16)
        precision = tpc / (tpc + fpc)
        r_curve[ci] = np.interp(-px, -conf[sel], recall, left=0)
        p_curve[ci] = np.interp(-px, -conf[sel], precision, left=1)
    f1 = 2 * p_curve * r_curve / (p_curve + r_curve + 1e-16)
    i = int(smooth(f1.mean(0), 0.1).argmax())
    return float(p_curve[:, i].mean()), float(r_curve[:, i].mean())


def _cat(parts: List[np.ndarray], empty: np.ndarray) -> np.ndarray:
    return np.concatenate(parts) if parts else empty


def ap_per_class(tp: np.ndarray, conf: np.ndarray, pred_cls: np.ndarray, gt_cls: np.ndarray) -> Dict[str, float]:
    """tp (n, 10) bool, conf / pred_cls (n,) of all predictions (any order), gt_cls (m,) of all ground truths → map50,
    map75, map, and precision / recall (precision_recall)."""
    order = np.argsort(-conf, kind="stable")
    tp, pc, gc = tp[order], pred_cls[order], gt_cls
    mp, mr = precision_recall(tp[:, 0], conf[order], pc, gc)
    classes = np.unique(gc)
    ap = np.zeros((len(classes), len(IOUV)))
    for ci, c in enumerate(classes):
        sel = pc == c
        n_gt = int((gc == c).sum())
        if sel.sum() == 0 or n_gt == 0:
            continue
        fpc = (1 - tp[sel]).cumsum(0)
        tpc = tp[sel].cumsum(0)
        recall = tpc / (n_gt + 1e-16)
        precision = tpc / (tpc + fpc)
        for k in range(len(IOUV)):
            ap[ci, k] = compute_ap(recall[:, k], precision[:, k])
    if len(classes) == 0:
        return {"map50": 0.0, "map75": 0.0, "map": 0.0, "precision": 0.0, "recall": 0.0}
    return {"map50": float(ap[:, 0].mean()), "map75": float(ap[:, 5].mean()), "map": float(ap.mean()),
            "precision": mp, "recall": mr}


def evaluate(preds: List[np.ndarray], gts: List[np.ndarray]) -> Dict[str, float]:
    """preds/gts: per-image (n,6) arrays [x1,y1,x2,y2,conf,cls] (gt conf ignored). Returns map50, map75, map, and
    precision / recall (precision_recall)."""
    tps, confs, pcls, gcls = [], [], [], []
    for p, g in zip(preds, gts):
        p = np.asarray(p, np.float64).reshape(-1, 6)
        g = np.asarray(g, np.float64).reshape(-1, 6)
        tps.append(match_predictions(p, g))
        confs.append(p[:, 4])
        pcls.append(p[:, 5])
        gcls.append(g[:, 5])
    return ap_per_class(_cat(tps, np.zeros((0, 10), bool)), _cat(confs, np.zeros(0)), _cat(pcls, np.zeros(0)),
                        _cat(gcls, np.zeros(0)))


def evaluate_pose(preds: List[np.ndarray], gts: List[np.ndarray], pred_kpts: List[np.ndarray],
                  gt_kpts: List[np.ndarray], sigma: np.ndarray) -> Dict[str, Dict[str, float]]:
    """Per image preds (n,6) / gts (m,6) as evaluate takes them, pred_kpts (n, K, 2 | 3) and gt_kpts (m, K, 3) in the
    same pixels as the boxes, sigma (K,).  Returns {"box": evaluate's dict, "pose": the same five keys}: the box branch
    matches on box IoU, the pose branch on kpt_iou with area = w · h · 0.53 of the ground-truth box (upstream
    PoseValidator._process_batch); confidences, classes and thresholds are shared, and each branch reads its
    precision / recall at its own F1-maximising confidence (PoseMetrics runs ap_per_class once per branch)."""
    K = len(sigma)
    tpb, tpp, confs, pcls, gcls = [], [], [], [], []
    for p, g, pk, gk in zip(preds, gts, pred_kpts, gt_kpts):
        p = np.asarray(p, np.float64).reshape(-1, 6)
        g = np.asarray(g, np.float64).reshape(-1, 6)
        pk = np.asarray(pk, np.float64)
        pk = pk.reshape(len(p), K, pk.shape[-1] if pk.ndim == 3 else 2)
        gk = np.asarray(gk, np.float64).reshape(len(g), K, 3)
        tpb.append(match_predictions(p, g))
        area = (g[:, 2] - g[:, 0]) * (g[:, 3] - g[:, 1]) * 0.53
        tpp.append(match_iou(kpt_iou(gk, pk, area, sigma), p[:, 5], g[:, 5]))
        confs.append(p[:, 4])
        pcls.append(p[:, 5])
        gcls.append(g[:, 5])
    conf, pc, gc = _cat(confs, np.zeros(0)), _cat(pcls, np.zeros(0)), _cat(gcls, np.zeros(0))
    return {"box": ap_per_class(_cat(tpb, np.zeros((0, 10), bool)), conf, pc, gc),
            "pose": ap_per_class(_cat(tpp, np.zeros((0, 10), bool)), conf, pc, gc)}
