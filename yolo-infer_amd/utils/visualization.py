"""Result writers: `save_detection_results(results, output_path, format)` with the reference's file formats
(/root/reference/utils/visualization.py:342-437).

The reference walks the boxes one at a time (`boxes.cls[i].cpu().numpy()` ... three device->host copies per
detection); here one (n, 6) copy per Results feeds all three formats:
  * txt: `"{cls} {conf:.6f} {x1:.6f} {y1:.6f} {x2:.6f} {y2:.6f}"` per line;
  * json: `{"detections": [{"class_id", "confidence", "bbox": [x1, y1, x2, y2]}, ...]}` with indent 2;
  * csv: header `class_id,confidence,x1,y1,x2,y2`, one row per detection.
Values are the fp32 tensor values (printed through Python floats, as the reference's numpy float32 -> float).
Pose results: the json format adds each detection's "keypoints" ([[x, y(, visibility)], ...]), and `draw_keypoints`
paints them on an image.  `draw_detections` (the reference's signature, utils/visualization.py:18) returns the image
with boxes, labels, masks and skeletons drawn in by the GPU annotator behind `Results.plot`.
"""
from __future__ import annotations

import csv
import json
from pathlib import Path
from typing import Any, List

import numpy as np


def _rows(results: Any) -> List[tuple]:
    boxes = getattr(results, "boxes", None)
    if boxes is None or len(boxes) == 0:
        return []
    data = boxes.data
    arr = data.detach().cpu().numpy() if hasattr(data, "detach") else np.asarray(data)
    arr = arr.astype(np.float32, copy=False)
    return [(int(r[5]), r[4], r[0], r[1], r[2], r[3]) for r in arr]


def _keypoints(results: Any):
    k = getattr(results, "keypoints", None)
    if k is None or len(k) == 0:
        return None
    data = k.data
    return data.detach().cpu().numpy() if hasattr(data, "detach") else np.asarray(data)


def draw_keypoints(image: np.ndarray, results: Any, radius: int = 2, color=(0, 255, 0)) -> np.ndarray:
    """A copy of the HWC uint8 `image` with a (2·radius + 1)² square at every keypoint of `results.keypoints` (those
    with visibility below 0.5 are skipped); the image itself when the results carry no keypoints."""
    kp = _keypoints(results)
    if kp is None:
        return image
    out = np.array(image, copy=True)
    h, w = out.shape[:2]
    for x, y, *v in kp.reshape(-1, kp.shape[-1]):
        if v and v[0] < 0.5:
            continue
        xi, yi = int(round(float(x))), int(round(float(y)))
        out[max(yi - radius, 0):min(yi + radius + 1, h), max(xi - radius, 0):min(xi + radius + 1, w)] = color
    return out


def draw_detections(image: np.ndarray, results: Any, class_names=None, line_thickness: int = 2, font_scale: float = 0.5,
                    font_thickness: int = 1) -> np.ndarray:
    """The reference's `draw_detections(image, results, class_names, line_thickness, ...)`: a copy of the HWC uint8 BGR
    `image` with the results drawn in — `results.plot(img=image, line_width=line_thickness)`, so the drawing runs on the
    GPU and follows Results.plot's rules.  class_names (a dict or a list) replaces the results' own names for this
    picture; font_scale and font_thickness have no meaning for the fixed bitmap font and are ignored.  results may be
    one Results or predict()'s list (its first element); None returns a copy of the image."""
    if isinstance(results, (list, tuple)):
        results = results[0] if results else None
    if results is None:
        return np.array(image, copy=True)
    if class_names:
        import copy
        results = copy.copy(results)
        results.names = dict(class_names) if isinstance(class_names, dict) else dict(enumerate(class_names))
    return results.plot(img=image, line_width=int(line_thickness))


def save_detection_results(results: Any, output_path: str, format: str = "txt") -> None:
    """Save one image's detections to `output_path` as 'txt', 'json' or 'csv' (the reference's formats)."""
    Path(output_path).parent.mkdir(parents=True, exist_ok=True)
    fmt = format.lower()
    if fmt not in ("txt", "json", "csv"):
        raise ValueError(f"Unsupported format: {format}")
    rows = _rows(results)
    if fmt == "txt":
        with open(output_path, "w") as f:
            for c, conf, x1, y1, x2, y2 in rows:
                f.write(f"{c} {conf:.6f} {x1:.6f} {y1:.6f} {x2:.6f} {y2:.6f}\n")
    elif fmt == "json":
        dets = [{"class_id": c, "confidence": float(conf), "bbox": [float(x1), float(y1), float(x2), float(y2)]}
                for c, conf, x1, y1, x2, y2 in rows]
        kp = _keypoints(results)
        if kp is not None:
            for d, k in zip(dets, kp):
                d["keypoints"] = [[float(v) for v in pt] for pt in k]
        with open(output_path, "w") as f:
            json.dump({"detections": dets}, f, indent=2)
    else:
        with open(output_path, "w", newline="") as f:
            w = csv.writer(f)
            w.writerow(["class_id", "confidence", "x1", "y1", "x2", "y2"])
            for c, conf, x1, y1, x2, y2 in rows:
                w.writerow([c, float(conf), float(x1), float(y1), float(x2), float(y2)])
