"""Validation mode (host side): dataset parsing, the Ultralytics val loader's rect batching, the val loop, metrics.

Restates, from the Ultralytics 8.3.x sources as remembered (the package is not available offline):
`data/utils.py:img2label_paths`, `data/base.py:BaseDataset.{set_rectangle, load_image}` (rect=True, pad 0.5, stride 32),
`data/augment.py:LetterBox(auto=False, scaleup=False, center=True)`, and `models/yolo/detect/val.py:DetectionValidator`
(non_max_suppression(multi_label=True, max_det=300) → scale_boxes with the image's own ratio and pad →
match_predictions → ap_per_class).  The GPU work is `Engine.run(multi_label=True)` (csrc/ym_nms_ml.hip) and one
`ym_letterbox` call per image with the geometry computed here.

Pose plans restate `models/yolo/pose/val.py:PoseValidator` on top of that: labels with K·ndim keypoint
columns (`data/utils.py:verify_image_label`), the predictions' keypoints to native pixels with the image's own ratio
and pad (`ops.scale_coords`), and box and OKS metrics side by side (`metrics.evaluate_pose`, upstream `PoseMetrics`).
"""
from __future__ import annotations

import logging
import math
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .metrics import OKS_SIGMA, evaluate, evaluate_pose
from .preprocess import IMG_SUFFIXES, load_image

logger = logging.getLogger(__name__)

STRIDE = 32
PAD = 0.5


def img2label_path(path: str) -> str:
    """The label file of an image: the last `/images/` of its path replaced by `/labels/`, suffix `.txt`."""
    sa, sb = f"{os.sep}images{os.sep}", f"{os.sep}labels{os.sep}"
    p = os.fspath(path)
    if sa in p:
        p = sb.join(p.rsplit(sa, 1))
    return os.path.splitext(p)[0] + ".txt"


def read_labels(path: str) -> np.ndarray:
    """(m, 5) [cls, cx, cy, w, h] normalised rows of a YOLO txt file; a missing or empty file is a background image."""
    if not os.path.isfile(path):
        return np.zeros((0, 5), np.float32)
    rows = [ln.split() for ln in open(path).read().splitlines() if ln.strip()]
    if not rows:
        return np.zeros((0, 5), np.float32)
    a = np.array([[float(v) for v in r[:5]] for r in rows], np.float32)
    if a.shape[1] != 5:
        raise ValueError(f"{path}: label rows are `cls cx cy w h`")
    return a


def _pose_rows(rows, kpt_shape, what: str) -> np.ndarray:
    """Label rows of `cls cx cy w h` and K·ndim keypoint values → (m, 5 + K·3) float32; any other row length is an
    error.  ndim 2 gains a visibility column as verify_image_label writes it: 1, or 0 where x < 0 or y < 0."""
    K, nd = int(kpt_shape[0]), int(kpt_shape[1])
    if nd not in (2, 3):
        raise ValueError(f"kpt_shape {(K, nd)}: ndim is 2 (x, y) or 3 (x, y, visibility)")
    rows = [np.asarray(r, np.float32).reshape(-1) for r in rows]
    for r in rows:
        if len(r) != 5 + K * nd:
            raise ValueError(f"{what}: pose label rows have {5 + K * nd} columns (`cls cx cy w h` and {K} x {nd} "
                             f"keypoint values for kpt_shape {(K, nd)}), got {len(r)}")
    if not rows:
        return np.zeros((0, 5 + K * 3), np.float32)
    a = np.stack(rows)
    if nd == 3:
        return a
    k = a[:, 5:].reshape(len(a), K, 2)
    v = np.where((k[..., 0] < 0) | (k[..., 1] < 0), 0.0, 1.0).astype(np.float32)
    return np.concatenate([a[:, :5], np.concatenate([k, v[..., None]], -1).reshape(len(a), K * 3)], 1)


def read_pose_labels(path: str, kpt_shape) -> np.ndarray:
    """(m, 5 + K·3) [cls, cx, cy, w, h, (x, y, v) · K] normalised rows of a YOLO pose txt file (_pose_rows); a missing
    or empty file is a background image."""
    rows = []
    if os.path.isfile(path):
        rows = [[float(v) for v in ln.split()] for ln in open(path).read().splitlines() if ln.strip()]
    return _pose_rows(rows, kpt_shape, path)


def _image_files(root: str) -> List[str]:
    out = []
    for d, _, files in sorted(os.walk(root)):
        out += [os.path.join(d, f) for f in sorted(files) if os.path.splitext(f)[1].lower() in IMG_SUFFIXES]
    return out


class Dataset:
    """Images (paths or in-memory HWC uint8 BGR arrays), their labels and the class names."""

    def __init__(self, images: list, labels: List[np.ndarray], names: Optional[Dict[int, str]] = None):
        self.images, self.labels, self.names = images, labels, names

    def __len__(self):
        return len(self.images)

    def image(self, i: int) -> np.ndarray:
        im = self.images[i]
        return load_image(im) if isinstance(im, (str, os.PathLike)) else im


def load_dataset(data, kpt_shape=None) -> Dataset:
    """data: a YAML file (path / val / names), a directory holding images/ and labels/, or a list of
    (HWC uint8 BGR ndarray, (m, 5) [cls, cx, cy, w, h] normalised) pairs.
    kpt_shape = (K, ndim), a pose model's: the labels are (m, 5 + K·3) rows (read_pose_labels); in-memory pairs carry
    (m, 5 + K·ndim); a YAML's own `kpt_shape` entry, when present, must be the model's."""
    if kpt_shape is not None:
        kpt_shape = (int(kpt_shape[0]), int(kpt_shape[1]))
    if isinstance(data, (list, tuple)):
        imgs, labels = [], []
        for im, lb in data:
            im = np.ascontiguousarray(im)
            if im.ndim != 3 or im.shape[2] != 3 or im.dtype != np.uint8:
                raise ValueError(f"in-memory images must be HWC uint8 BGR, got {im.shape} {im.dtype}")
            imgs.append(im)
            if kpt_shape is None:
                labels.append(np.asarray(lb, np.float32).reshape(-1, 5))
            else:
                labels.append(_pose_rows(lb, kpt_shape, f"in-memory image {len(imgs) - 1}"))
        return Dataset(imgs, labels)
    p = os.fspath(data)
    names = None
    if os.path.isdir(p):
        files = _image_files(os.path.join(p, "images"))
    elif os.path.isfile(p) and os.path.splitext(p)[1].lower() in (".yaml", ".yml"):
        import yaml
        cfg = yaml.safe_load(open(p)) or {}
        if "val" not in cfg:
            raise ValueError(f"{p}: a dataset YAML needs a `val` entry")
        if kpt_shape is not None and cfg.get("kpt_shape") is not None:
            ks = cfg["kpt_shape"]
            if not isinstance(ks, (list, tuple)) or tuple(int(v) for v in ks) != kpt_shape:
                raise ValueError(f"{p}: kpt_shape {ks} is not the model's {list(kpt_shape)}")
        root =cfg.get("path") or os.path.dirname(os.path.abspath(p))
        if not os.path.isabs(root):
            root = os.path.join(os.path.dirname(os.path.abspath(p)), root)
        n = cfg.get("names")
        if isinstance(n, (list, tuple)):
            names = dict(enumerate(n))
        elif isinstance(n, dict):
            names = {int(k): v for k, v in n.items()}
        files = []
        for v in cfg["val"] if isinstance(cfg["val"], (list, tuple)) else [cfg["val"]]:
            v = v if os.path.isabs(v) else os.path.join(root, v)
            if os.path.isdir(v):
                files += _image_files(v)
            elif os.path.isfile(v):  # a txt list of image paths (relative ones to the list's directory)
                for ln in open(v).read().splitlines():
                    if ln.strip():
                        f = ln.strip()
                        files.append(f if os.path.isabs(f) else os.path.normpath(os.path.join(os.path.dirname(v), f)))
            else:
                raise FileNotFoundError(f"{p}: val entry {v} does not exist")
    else:
        raise FileNotFoundError(f"dataset {p!r}: expected a YAML file or a directory with images/ and labels/")
    if not files:
        raise FileNotFoundError(f"dataset {p!r}: no images found")
    if kpt_shape is not None:
        return Dataset(files, [read_pose_labels(img2label_path(f), kpt_shape) for f in files], names)
    return Dataset(files, [read_labels(img2label_path(f)) for f in files], names)


def build_batches(shapes: Sequence[Tuple[int, int]], imgsz: int = 640, batch: int = 16, stride: int = STRIDE,
                  pad: float = PAD) -> List[Dict]:
    """The val loader's rect batching for images of (h, w) `shapes`: sorted by aspect ratio h / w (stable), cut into
    batches of `batch`; per batch the shape factor is [maxi, 1] if maxi < 1, [1, 1 / mini] if mini > 1, else [1, 1]
    (mini / maxi: the batch's smallest / largest h / w) and batch_shape = ceil(factor * imgsz / stride + pad) * stride.
    Each image is resized so that its long side is imgsz (w, h = min(ceil(w0 r), imgsz), min(ceil(h0 r), imgsz)) and
    centred on the batch shape (LetterBox, scaleup=False: no further scaling unless the canvas is smaller).
    Returns per batch {"indices", "shape": (Hb, Wb), "geo": [(uh, uw, top, left)], "gain": [resized h / h0 * r]}."""
    s = np.asarray(shapes, np.float64).reshape(-1, 2)
    ar = s[:, 0] / s[:, 1]
    order = np.argsort(ar, kind="stable")
    out = []
    for b0 in range(0, len(order), batch):
        idx = order[b0:b0 + batch]
        mini, maxi = ar[idx].min(), ar[idx].max()
        f = [maxi, 1.0] if maxi < 1 else ([1.0, 1.0 / mini] if mini > 1 else [1.0, 1.0])
        Hb, Wb = (int(math.ceil(v * imgsz / stride + pad)) * stride for v in f)
        geo, gain = [], []
        for i in idx:
            h0, w0 = int(shapes[i][0]), int(shapes[i][1])
            r = imgsz / max(h0, w0)
            h, w = (h0, w0) if r == 1 else (min(math.ceil(h0 * r), imgsz), min(math.ceil(w0 * r), imgsz))
            rl = min(Hb / h, Wb / w, 1.0)  # LetterBox(scaleup=False)
            uh, uw = int(round(h * rl)), int(round(w * rl))
            top, left = int(round((Hb - uh) / 2 - 0.1)), int(round((Wb - uw) / 2 - 0.1))
            geo.append((uh, uw, top, left))
            gain.append(h / h0 * rl)
        out.append({"indices": [int(i) for i in idx], "shape": (Hb, Wb), "geo": geo, "gain": gain})
    return out


def to_native(rows: np.ndarray, geo, gain: float, shape0) -> np.ndarray:
    """ops.scale_boxes(batch shape, rows, shape0, ratio_pad=((gain, gain), (left, top))): letterboxed xyxy rows to the
    native image's pixels, clipped to it.  Returns a float64 copy."""
    r = np.array(rows, np.float64).reshape(-1, rows.shape[-1] if rows.ndim == 2 else 6)
    r[:, [0, 2]] -= geo[3]
    r[:, [1, 3]] -= geo[2]
    r[:, :4] /= gain
    r[:, [0, 2]] = r[:, [0, 2]].clip(0, shape0[1])
    r[:, [1, 3]] = r[:, [1, 3]].clip(0, shape0[0])
    return r


def labels_to_native(lb: np.ndarray, shape0) -> np.ndarray:
    """(m, 5) [cls, cx, cy, w, h] normalised → (m, 6) [x1, y1, x2, y2, 1, cls] in native pixels."""
    lb = np.asarray(lb, np.float64).reshape(-1, 5)
    h0, w0 = shape0
    out = np.ones((len(lb), 6), np.float64)
    out[:, 0] = (lb[:, 1] - lb[:, 3] / 2) * w0
    out[:, 1] = (lb[:, 2] - lb[:, 4] / 2) * h0
    out[:, 2] = (lb[:, 1] + lb[:, 3] / 2) * w0
    out[:, 3] = (lb[:, 2] + lb[:, 4] / 2) * h0
    out[:, 5] = lb[:, 0]
    return out


def kpts_to_native(kpts: np.ndarray, geo, gain: float, shape0) -> np.ndarray:
    """ops.scale_coords(batch shape, kpts, shape0, ratio_pad=((gain, gain), (left, top))): letterboxed (n, K, ndim)
    keypoints to the native image's pixels with to_native's gain and pad, x clipped to [0, w0] and y to [0, h0]
    (scale_coords always clips).  A visibility column passes through.  Returns a float64 copy."""
    k = np.array(kpts, np.float64)
    k[..., 0] = ((k[..., 0] - geo[3]) / gain).clip(0, shape0[1])
    k[..., 1] = ((k[..., 1] - geo[2]) / gain).clip(0, shape0[0])
    return k


def label_kpts_to_native(lb: np.ndarray, shape0, K: int) -> np.ndarray:
    """(m, 5 + K·3) normalised pose labels → their (m, K, 3) keypoints [x · w0, y · h0, v] in native pixels."""
    k = np.array(np.asarray(lb, np.float64).reshape(-1, 5 + K * 3)[:, 5:].reshape(-1, K, 3))
    k[..., 0] *= shape0[1]
    k[..., 1] *= shape0[0]
    return k


def make_batch(engine, imgs: Sequence[np.ndarray], b: Dict):
    """The (nb, 3, Hb, Wb) fp32 device batch of one build_batches entry: one ym_letterbox call per image."""
    import torch
    Hb, Wb = b["shape"]
    x = torch.empty((len(imgs), 3, Hb, Wb), dtype=torch.float32, device=engine.device)
    stream = torch.cuda.current_stream(engine.device).cuda_stream
    srcs = [torch.from_numpy(np.ascontiguousarray(im)).to(engine.device) for im in imgs]
    for i, (src, (uh, uw, top, left)) in enumerate(zip(srcs, b["geo"])):
        h0, w0 = src.shape[:2]
        engine.rt.letterbox(src.data_ptr(), h0, w0, src.stride(0), True, uh, uw, top, left, x[i].data_ptr(), Hb, Wb,
                            stream)
    torch.cuda.synchronize(engine.device)  # the source images are released with this frame
    return x


class BoxMetrics:
    def __init__(self, m: Dict[str, float]):
        self.map, self.map50, self.map75 = m["map"], m["map50"], m["map75"]
        self.mp, self.mr = m["precision"], m["recall"]


class ValResults:
    """What `YOLO11Model.val` returns: `.box.map / .map50 / .map75 / .mp / .mr`, `.speed` (ms per image) and
    `.results_dict` (upstream DetMetrics keys).  A pose run also has `.pose` (the same attributes from the OKS
    matches) and upstream PoseMetrics' keys: the (B) keys, the (P) keys, fitness = box fitness + pose fitness."""

    def __init__(self, m: Dict[str, float], speed: Dict[str, float], n_images: int, n_labels: int,
                 pose: Optional[Dict[str, float]] = None):
        self.box = BoxMetrics(m)
        self.speed = speed
        self.n_images, self.n_labels = n_images, n_labels
        self.results_dict = {"metrics/precision(B)": self.box.mp, "metrics/recall(B)": self.box.mr,
                             "metrics/mAP50(B)": self.box.map50, "metrics/mAP50-95(B)": self.box.map,
                             "fitness": 0.1 * self.box.map50 + 0.9 * self.box.map}
        if pose is not None:
            self.pose = BoxMetrics(pose)
            fitness = self.results_dict.pop("fitness")
            self.results_dict.update({"metrics/precision(P)": self.pose.mp, "metrics/recall(P)": self.pose.mr,
                                      "metrics/mAP50(P)": self.pose.map50, "metrics/mAP50-95(P)": self.pose.map,
                                      "fitness": fitness + (0.1 * self.pose.map50 + 0.9 * self.pose.map)})

    def __repr__(self):
        return f"ValResults(images={self.n_images}, labels={self.n_labels}, {self.results_dict})"


def run_val(engine, data, imgsz: int = 640, batch: int = 16, conf: float = 0.001, iou: float = 0.7,
            max_det: int = 300, collect: Optional[list] = None, augment: bool = False) -> ValResults:
    """The validation loop on one Engine (a detect or pose plan).  collect, when a list, receives per image
    (native-pixel predictions (n, 6), native-pixel labels (m, 6)) in dataset order.  augment: every batch through
    Engine.run_tta (Ultralytics val(augment=True)) instead of Engine.run.
    A pose plan runs the same batches (its one class makes multi_label the single-label NMS, as upstream's
    `multi_label &= nc > 1`), takes the rows' K·ndim keypoints to native pixels as well and returns box and OKS
    metrics (`.box`, `.pose`); collect then receives (predictions, labels, predicted keypoints (n, K, ndim), label
    keypoints (m, K, 3)); augment is not supported by the pose head: a warning, then single-scale, as upstream."""
    import torch
    if engine.task == "segment":
        raise NotImplementedError("validation is not implemented for segment plans (detect and pose plans are)")
    if engine.task not in ("detect", "pose"):
        raise NotImplementedError(f"validation is implemented for detect and pose plans (got task {engine.task!r})")
    pose = engine.task == "pose"
    if pose and augment:
        # upstream BaseModel._predict_augment's words (only DetectionModel itself overrides it)
        logger.warning("Model does not support 'augment=True', reverting to single-scale prediction.")
        augment = False
    kpt_shape = tuple(engine.kpt_shape) if pose else None
    if isinstance(data, Dataset):
        ds = data
    else:
        ds = load_dataset(data, kpt_shape) if pose else load_dataset(data)
    imgs_cache = {}
    shapes = []
    for i in range(len(ds)):
        if isinstance(ds.images[i], (str, os.PathLike)):  # the header is enough for the batching
            from PIL import Image
            with Image.open(ds.images[i]) as im:
                shapes.append((im.size[1], im.size[0]))
        else:
            imgs_cache[i] = ds.images[i]
            shapes.append(tuple(ds.images[i].shape[:2]))
    preds: List[np.ndarray] = [None] * len(ds)
    gts: List[np.ndarray] = [None] * len(ds)
    pkpts: List[np.ndarray] = [None] * len(ds)
    gkpts: List[np.ndarray] = [None] * len(ds)
    K, nk = (kpt_shape[0], engine.nk) if pose else (0, 0)
    t_pre = t_inf = t_post = 0.0
    for b in build_batches(shapes, imgsz, batch):
        t0 = time.perf_counter()
        imgs = [imgs_cache[i] if i in imgs_cache else ds.image(i) for i in b["indices"]]
        x = make_batch(engine, imgs, b)
        t1 = time.perf_counter()
        run = engine.run_tta if augment else engine.run
        dets, counts = run(x, conf=conf, iou=iou, max_det=max_det, multi_label=True)
        torch.cuda.synchronize(engine.device)
        t2 = time.perf_counter()
        n = counts[:len(imgs)].tolist()
        rows = dets[:len(imgs)].cpu().numpy()
        for k, i in enumerate(b["indices"]):
            preds[i] = to_native(rows[k, :n[k], :6], b["geo"][k], b["gain"][k], shapes[i])
            if pose:
                pkpts[i] = kpts_to_native(rows[k, :n[k], 6:6 + nk].reshape(n[k], *kpt_shape), b["geo"][k],
                                          b["gain"][k], shapes[i])
                gts[i] = labels_to_native(ds.labels[i][:, :5], shapes[i])
                gkpts[i] = label_kpts_to_native(ds.labels[i], shapes[i], K)
            else:
                gts[i] = labels_to_native(ds.labels[i], shapes[i])
        t3 = time.perf_counter()
        t_pre, t_inf, t_post = t_pre + t1 - t0, t_inf + t2 - t1, t_post + t3 - t2
    t3 = time.perf_counter()
    if pose:
        # upstream PoseValidator.init_metrics: the COCO constants for the 17-keypoint skeleton, else uniform 1 / K
        sigma = OKS_SIGMA if kpt_shape == (17, 3) else np.ones(K) / K
        mm = evaluate_pose(preds, gts, pkpts, gkpts, sigma)
        m, mpose = mm["box"], mm["pose"]
    else:
        m, mpose = evaluate(preds, gts), None
    t_post += time.perf_counter() - t3
    if collect is not None:
        collect.extend(zip(preds, gts, pkpts, gkpts) if pose else zip(preds, gts))
    k = 1e3 / max(len(ds), 1)
    speed = {"preprocess": t_pre * k, "inference": t_inf * k, "loss": 0.0, "postprocess": t_post * k}
    return ValResults(m, speed, len(ds), int(sum(len(g) for g in gts)), pose=mpose)
