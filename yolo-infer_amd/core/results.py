"""Results / Boxes / Masks: the per-image result objects `YOLO11Model.predict` returns.

Mirrors the subset of the Ultralytics Results contract the reference's consumers read
(/root/reference/demos/detection_demo.py:116-132 `.boxes.xyxy/.conf/.cls` per box, `.cpu().numpy()`;
/root/reference/utils/visualization.py:46-74, 370-437 `.names`, `len(boxes)`, iteration, `.masks.data`).
Tensors stay on the model's device, like upstream.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch


class _TensorView:
    def __init__(self, data):
        self.data = data

    def cpu(self):
        return self.__class__(self.data.cpu(), *self._extra()) if isinstance(self.data, torch.Tensor) else self

    def numpy(self):
        d = self.data.cpu().numpy() if isinstance(self.data, torch.Tensor) else self.data
        return self.__class__(d, *self._extra())

    def cuda(self):
        return self.__class__(torch.as_tensor(self.data).cuda(), *self._extra())

    def to(self, *args, **kwargs):
        return self.__class__(torch.as_tensor(self.data).to(*args, **kwargs), *self._extra())

    def _extra(self):
        return ()

    @property
    def shape(self):
        return self.data.shape

    def __len__(self):
        return len(self.data)

    def __getitem__(self, idx):
        return self.__class__(self.data[idx], *self._extra())

    def __iter__(self):
        for i in range(len(self)):
            yield self[i]


class Boxes(_TensorView):
    """(n, 6) [x1, y1, x2, y2, conf, cls] detections of one image, or with tracking (n, 7) [x1, y1, x2, y2, id, conf,
    cls] (upstream `ultralytics.engine.results.Boxes`)."""

    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        super().__init__(boxes)
        self.orig_shape = orig_shape

    def _extra(self):
        return (self.orig_shape,)

    @property
    def xyxy(self):
        return self.data[:, :4]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def id(self):
        return self.data[:, -3] if self.is_track else None

    @property
    def is_track(self):
        return self.data.shape[-1] == 7

    @property
    def xywh(self):
        x = self.xyxy
        y = x.clone() if isinstance(x, torch.Tensor) else np.copy(x)
        y[..., 0] = (x[..., 0] + x[..., 2]) / 2
        y[..., 1] = (x[..., 1] + x[..., 3]) / 2
        y[..., 2] = x[..., 2] - x[..., 0]
        y[..., 3] = x[..., 3] - x[..., 1]
        return y

    @property
    def xyxyn(self):
        x = self.xyxy.clone() if isinstance(self.xyxy, torch.Tensor) else np.copy(self.xyxy)
        x[..., [0, 2]] /= self.orig_shape[1]
        x[..., [1, 3]] /= self.orig_shape[0]
        return x

    @property
    def xywhn(self):
        x = self.xywh
        x[..., [0, 2]] /= self.orig_shape[1]
        x[..., [1, 3]] /= self.orig_shape[0]
        return x


class Masks(_TensorView):
    """(n, H, W) binary instance masks of one image (upstream `ultralytics.engine.results.Masks`).

    `xy` / `xyn`: the instances' polygons, upstream's `masks2segments` (strategy "largest") traced on the GPU by the
    engine that made the masks (Engine.mask_contours, csrc/ym_contour.hip; the contour definition is DESIGN.md §18's,
    not cv2's), then `scale_coords((H, W), points, orig_shape)`.  Computed on first access (one launch, two small
    device->host reads for all n instances) and cached; a hand-built Masks needs `engine=`: there is no host tracer.

    `rle` / `area`: the planes' COCO run-length encoding and their set pixels, encoded on the GPU by the same engine
    (Engine.mask_rle, csrc/ym_rle.hip), lossless where `xy` keeps one outline.  The planes are encoded
    as they are: with `retina_masks=True` they have the original image's size and the RLE is what a COCO consumer
    (pycocotools' `segm` evaluation, upstream's `pred_to_json`) takes; by default they are the letterboxed
    network-input planes, exact for that frame but not COCO-ready for an image of another size."""

    def __init__(self, masks, orig_shape=None, engine=None):
        super().__init__(masks)
        self.orig_shape = orig_shape
        self._engine = engine
        self._xy = None
        self._rle = None  # (list of {"size", "counts"}, int64 areas)

    def _extra(self):
        return (self.orig_shape, self._engine)

    def _carry(self, other, idx=None):
        """Hand the computed polygons and RLE (all, or those `idx` selects) to `other`, a view of the same planes."""
        if isinstance(idx, torch.Tensor):
            idx = idx.cpu().numpy()
        if self._xy is not None:
            if idx is None:
                other._xy = self._xy
            else:
                sel = np.arange(len(self._xy))[idx]
                other._xy = [self._xy[i] for i in np.atleast_1d(sel).tolist()]
        if self._rle is not None:
            if idx is None:
                other._rle = self._rle
            else:
                sel = np.atleast_1d(np.arange(len(self._rle[0]))[idx])
                other._rle = ([self._rle[0][i] for i in sel.tolist()], self._rle[1][sel])
        return other

    def _planes(self, what):
        """The (n, H, W) uint8 / bool planes on the engine's device; `what`: the refusal's first words."""
        if self._engine is None:
            raise RuntimeError(f"{what} on the GPU: this Masks was built by hand without "
                               "engine= (an Engine, e.g. model.model.engine); there is no host fallback")
        planes = torch.as_tensor(self.data)
        if planes.dim() == 2:
            planes = planes[None]
        if planes.dtype not in (torch.uint8, torch.bool):
            planes = planes != 0
        if planes.device != self._engine.device:  # after Results.cpu(): one upload
            planes = planes.to(self._engine.device)
        return planes

    def __getitem__(self, idx):
        return self._carry(super().__getitem__(idx), idx)

    def cpu(self):
        return self._carry(super().cpu())

    def numpy(self):
        return self._carry(super().numpy())

    def cuda(self):
        return self._carry(super().cuda())

    def to(self, *args, **kwargs):
        return self._carry(super().to(*args, **kwargs))

    @property
    def xy(self):
        """A list of n (k_i, 2) float32 numpy arrays: each instance's polygon, (x, y) in the original image's pixels."""
        if self._xy is None:
            planes = self._planes("Masks.xy traces the polygons")
            from yolomi.preprocess import scale_coords
            shape = tuple(planes.shape[-2:])
            orig = self.orig_shape if self.orig_shape is not None else shape
            self._xy = [scale_coords(shape, torch.from_numpy(p.astype(np.float32)), orig).numpy()
                        for p in self._engine.mask_contours(planes)]
        return self._xy

    @property
    def xyn(self):
        """`xy` with x divided by the original image's width and y by its height."""
        shape = self.orig_shape if self.orig_shape is not None else tuple(self.data.shape[-2:])
        wh = np.array([shape[1], shape[0]], dtype=np.float32)
        return [p / wh for p in self.xy]

    def _encode(self, what):
        if self._rle is None:
            planes = self._planes(f"Masks.{what} is encoded")
            size = [int(planes.shape[-2]), int(planes.shape[-1])]
            enc = self._engine.mask_rle(planes)
            self._rle = ([{"size": size, "counts": s} for _, s, _ in enc],
                         np.array([a for _, _, a in enc], dtype=np.int64))
        return self._rle

    @property
    def rle(self):
        """A list of n {"size": [H, W], "counts": bytes}: each plane's COCO RLE (pycocotools' compressed form), at the
        planes' own size: COCO-ready with `retina_masks=True` (the image's size), the letterboxed frame otherwise."""
        return self._encode("rle")[0]

    @property
    def area(self):
        """(n,) int64: the set pixels of each plane (the sum of its RLE's odd-indexed counts), from the same call."""
        return self._encode("area")[1]


class Keypoints(_TensorView):
    """(n, K, 2 | 3) keypoints of one image (upstream `ultralytics.engine.results.Keypoints`): x, y in the original
    image's pixels and, with 3 values, the visibility; x and y of a keypoint whose visibility is below 0.5 are zeroed
    (in place, as upstream does: hand in a tensor you own)."""

    def __init__(self, keypoints, orig_shape):
        if keypoints.ndim == 2:
            keypoints = keypoints[None, :]
        if keypoints.shape[-1] == 3:
            mask = keypoints[..., 2] < 0.5
            keypoints[..., :2][mask] = 0
        super().__init__(keypoints)
        self.orig_shape = orig_shape
        self.has_visible = self.data.shape[-1] == 3

    def _extra(self):
        return (self.orig_shape,)

    @property
    def xy(self):
        return self.data[..., :2]

    @property
    def xyn(self):
        xy = self.xy.clone() if isinstance(self.xy, torch.Tensor) else np.copy(self.xy)
        xy[..., 0] /= self.orig_shape[1]
        xy[..., 1] /= self.orig_shape[0]
        return xy

    @property
    def conf(self):
        return self.data[..., 2] if self.has_visible else None


class OBB(_TensorView):
    """(n, 7) [cx, cy, w, h, theta, conf, cls] oriented boxes of one image (upstream `ultralytics.engine.results.OBB`):
    centre and size in the original image's pixels, theta in radians, regularised (w >= h, theta in [0, pi))."""

    def __init__(self, boxes, orig_shape):
        if boxes.ndim == 1:
            boxes = boxes[None, :]
        super().__init__(boxes)
        self.orig_shape = orig_shape

    def _extra(self):
        return (self.orig_shape,)

    @property
    def xywhr(self):
        return self.data[:, :5]

    @property
    def conf(self):
        return self.data[:, -2]

    @property
    def cls(self):
        return self.data[:, -1]

    @property
    def xyxyxyxy(self):
        """(n, 4, 2) corners ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2 (upstream's xywhr2xyxyxyxy), with
        v1 = (w / 2)(cos, sin) and v2 = (h / 2)(-sin, cos)."""
        d = self.data
        xp = torch if isinstance(d, torch.Tensor) else np
        c, s = xp.cos(d[:, 4]), xp.sin(d[:, 4])
        ctr = d[:, :2]
        v1 = xp.stack([d[:, 2] / 2 * c, d[:, 2] / 2 * s], -1)
        v2 = xp.stack([-d[:, 3] / 2 * s, d[:, 3] / 2 * c], -1)
        return xp.stack([ctr + v1 + v2, ctr + v1 - v2, ctr - v1 - v2, ctr - v1 + v2], -2)

    @property
    def xyxyxyxyn(self):
        p = self.xyxyxyxy
        p = p.clone() if isinstance(p, torch.Tensor) else np.copy(p)
        p[..., 0] /= self.orig_shape[1]
        p[..., 1] /= self.orig_shape[0]
        return p

    @property
    def xyxy(self):
        """(n, 4) the axis-aligned hull of the corners."""
        p = self.xyxyxyxy
        xp = torch if isinstance(p, torch.Tensor) else np
        x, y = p[..., 0], p[..., 1]
        return xp.stack([x.min(-1)[0] if xp is torch else x.min(-1), y.min(-1)[0] if xp is torch else y.min(-1),
                         x.max(-1)[0] if xp is torch else x.max(-1), y.max(-1)[0] if xp is torch else y.max(-1)], -1)


def obb_rows_to_results(rows, in_shape=None, orig_shape=None):
    """NMS rows (n, 7) [cx, cy, w, h, conf, cls, theta] -> OBB data (n, 7) [cx, cy, w, h, theta, conf, cls] as
    OBBPredictor builds it: regularize_rboxes (w <= h: swap and theta + pi / 2; theta mod pi), then, for a letterboxed
    source, scale_boxes(xywh=True): the pad off the centre, all four by the gain, no clip."""
    import math
    x, y, w, h, conf, c, t = rows.unbind(-1)
    swap = w <= h
    w_, h_ = torch.where(swap, h, w), torch.where(swap, w, h)
    t = torch.where(swap, t + math.pi / 2, t) % math.pi
    if in_shape is not None and orig_shape is not None and tuple(in_shape) != tuple(orig_shape):
        gain = min(in_shape[0] / orig_shape[0], in_shape[1] / orig_shape[1])
        px = round((in_shape[1] - orig_shape[1] * gain) / 2 - 0.1)
        py = round((in_shape[0] - orig_shape[0] * gain) / 2 - 0.1)
        x, y, w_, h_ = (x - px) / gain, (y - py) / gain, w_ / gain, h_ / gain
    return torch.stack([x, y, w_, h_, t, conf, c], -1)


class Probs(_TensorView):
    """Upstream `Probs`: the class probabilities of one image.  `data` is the (nc,) softmax the head's kernel wrote;
    top1 / top5 / top1conf / top5conf read that kernel's own top-k (csrc/ym_classify.hip: descending, equal
    probabilities to the lower class) — nothing is sorted on the host.  top1 and top5 read the device (one small
    copy, cached); data, top1conf and top5conf stay tensors, and move with cpu() / numpy() / cuda() / to() as data
    does.  An index (probs[idx]) gives the Probs of data[idx], its top-k taken from those values."""

    def __init__(self, probs, topk=None, topk_conf=None):
        super().__init__(probs)
        if topk is None:  # a hand-built or indexed Probs: the same order from a stable sort
            topk_conf, topk = torch.sort(torch.as_tensor(probs).reshape(-1), descending=True, stable=True)
            topk, topk_conf = topk[:5].to(torch.int32), topk_conf[:5]
            if not isinstance(probs, torch.Tensor):
                topk, topk_conf = topk.numpy(), topk_conf.numpy()
        self._topk, self._conf, self._host = topk, topk_conf, None

    def _moved(self, f):
        return Probs(f(self.data), f(self._topk), f(self._conf))

    def cpu(self):
        return self._moved(lambda t: t.cpu() if isinstance(t, torch.Tensor) else t)

    def numpy(self):
        return self._moved(lambda t: t.cpu().numpy() if isinstance(t, torch.Tensor) else t)

    def cuda(self):
        return self._moved(lambda t: torch.as_tensor(t).cuda())

    def to(self, *args, **kwargs):
        return self._moved(lambda t: torch.as_tensor(t).to(*args, **kwargs))

    def __getitem__(self, idx):
        return Probs(self.data[idx])

    @property
    def top5(self) -> List[int]:
        if self._host is None:
            self._host = torch.as_tensor(self._topk).tolist()
        return self._host

    @property
    def top1(self) -> int:
        return self.top5[0]

    @property
    def top5conf(self):
        return self._conf

    @property
    def top1conf(self):
        return self._conf[0]


class LazyCounts:
    """The B detection counts of one asynchronous predict() call, still on the device (the words the NMS kernel
    writes behind the call's rows): read to the host once, on the first access by any of the call's Results."""

    def __init__(self, dev_counts: torch.Tensor, stream=None):
        self._dev = dev_counts
        self._host = None
        self._ev = None
        if stream is not None:  # the launch stream's point: the read may happen under another current stream
            self._ev = torch.cuda.Event()
            self._ev.record(stream)

    def __getitem__(self, b: int) -> int:
        if self._host is None:
            if self._ev is not None:
                self._ev.synchronize()
            self._host = self._dev.tolist()  # the device->host read of this call
        return self._host[b]


class Results:
    def __init__(self, orig_tensor: Optional[torch.Tensor], names: Dict[int, str], boxes: torch.Tensor,
                 masks: Optional[torch.Tensor] = None, path: str = "image0.jpg", speed=None,
                 keypoints: Optional[torch.Tensor] = None, annotator=None):
        """keypoints: (n, K, 2 | 3), already in the original image's coordinates and clipped to it (scale_coords).
        annotator: what plot() draws with — an Engine (anything with its `annotate` and `device`); predict() and track()
        hand in their own."""
        self._annotator = annotator
        self._mask_geo = None
        self._orig_tensor = orig_tensor
        self._orig_img = None
        self.orig_shape = tuple(orig_tensor.shape[-2:]) if orig_tensor is not None else None
        self.names = names
        self._dets = None
        self.boxes = Boxes(boxes, self.orig_shape) if boxes is not None else None  # (None: a classification result)
        self.masks = Masks(masks, self.orig_shape, engine=annotator) if masks is not None else None
        self.path = path
        self.speed = speed or {"preprocess": None, "inference": None, "postprocess": None}
        self.probs = None
        self._kpts = Keypoints(keypoints, self.orig_shape) if keypoints is not None else None
        self._ksrc = None
        self.obb = None

    @classmethod
    def from_batch(cls, batch: torch.Tensor, b: int, names: Dict[int, str], dets: torch.Tensor, n,
                   path: str = "image0.jpg", speed=None, masks: Optional[torch.Tensor] = None,
                   moff: int = 0, kpt_shape: Optional[tuple] = None, tracked: bool = False,
                   det_idx: Optional[torch.Tensor] = None, annotator=None) -> "Results":
        """Image b of a predict() batch: boxes = dets[b, :n, :6], the input slice batch[b] and (Segment) the masks
        masks[moff : moff + n], all taken (as tensor views) on first access, so building the B Results of a call
        costs no tensor operations.  n: the count, or the call's LazyCounts (read from the device on first access).
        kpt_shape (Pose): (K, ndim); the keypoints are dets[b, :n, 6 : 6 + K·ndim], copied, clipped to the image
        (scale_coords with equal shapes) and masked by visibility on first access.
        tracked: dets holds track() rows, [x1, y1, x2, y2, id, conf, cls, extras]: the boxes take 7 columns and the
        keypoints start at column 7; det_idx: the call's (B, max_det) detection row behind each track row."""
        r = cls.__new__(cls)
        r._annotator = annotator
        r._mask_geo = None
        r._ncol = 7 if tracked else 6
        r._didx = det_idx
        r._batch, r._b, r._dets, r._n = batch, b, dets, n
        r._orig_tensor_v = None
        r._orig_img = None
        r.orig_shape = tuple(batch.shape[-2:])
        r.names = names
        r._boxes = None
        r._masks = None
        r._msrc = (masks, moff) if masks is not None else None
        r.path = path
        r.speed = speed or {"preprocess": None, "inference": None, "postprocess": None}
        r.probs = r.obb = None
        r._kpts = None
        r._ksrc = tuple(kpt_shape) if kpt_shape else None
        return r

    @classmethod
    def from_image(cls, img_bgr: np.ndarray, path: str, names: Dict[int, str], boxes: torch.Tensor,
                   masks: Optional[torch.Tensor] = None, speed=None,
                   keypoints: Optional[torch.Tensor] = None, annotator=None, mask_geo=None) -> "Results":
        """An image-file / ndarray source: `orig_img` is the HWC uint8 BGR image as loaded (cv2.imread order),
        boxes (and keypoints) are in its coordinates (already mapped back by scale_boxes / scale_coords).
        mask_geo: (uh, uw, top, left), the letterbox window of the mask plane this image occupies (plot() maps canvas
        pixels into it); None when the masks are at the image's own resolution."""
        r = cls(None, names, boxes, masks=masks, path=path, speed=speed, keypoints=keypoints, annotator=annotator)
        r._mask_geo = tuple(int(v) for v in mask_geo) if mask_geo is not None else None
        r._orig_img = img_bgr
        r.orig_shape = tuple(img_bgr.shape[:2])
        if r.boxes is not None:
            r.boxes.orig_shape = r.orig_shape
        if r._kpts is not None:
            r._kpts.orig_shape = r.orig_shape
        if r.masks is not None:
            r.masks.orig_shape = r.orig_shape
        return r

    @property
    def _orig_tensor(self):
        if self._orig_tensor_v is None and getattr(self, "_batch", None) is not None:
            self._orig_tensor_v = self._batch[self._b]
        return self._orig_tensor_v

    @_orig_tensor.setter
    def _orig_tensor(self, t):
        self._orig_tensor_v = t
        self._batch = None

    @property
    def _count(self) -> int:
        return self._n if isinstance(self._n, int) else self._n[self._b]

    @property
    def boxes(self) -> "Boxes":
        if self._boxes is None and self._dets is not None:
            self._boxes = Boxes(self._dets[self._b, : self._count, :self._ncol], self.orig_shape)
        return self._boxes

    @boxes.setter
    def boxes(self, b):
        self._boxes = b

    @property
    def masks(self) -> Optional["Masks"]:
        if self._masks is None and getattr(self, "_msrc", None) is not None:
            mb, moff = self._msrc
            self._masks = Masks(mb[moff:moff + self._count], self.orig_shape, engine=self._annotator)
        return self._masks

    @masks.setter
    def masks(self, m):
        self._masks = m
        self._msrc = None

    @property
    def keypoints(self) -> Optional["Keypoints"]:
        if self._kpts is None and getattr(self, "_ksrc", None) is not None:
            K, nd = self._ksrc
            n = self._count
            k = self._dets[self._b, :n, self._ncol:self._ncol + K * nd].reshape(n, K, nd).clone()
            k[..., 0].clamp_(0, self.orig_shape[1])  # ops.scale_coords(shape, kpts, shape): gain 1, pad 0, clip
            k[..., 1].clamp_(0, self.orig_shape[0])
            self._kpts = Keypoints(k, self.orig_shape)
        return self._kpts

    @keypoints.setter
    def keypoints(self, k):
        self._kpts = k
        self._ksrc = None

    @property
    def det_idx(self) -> Optional[torch.Tensor]:
        """track() results of a tensor source: per box, the row of this frame's detection (in predict()'s order for
        the same call) that fed the track; None otherwise."""
        d = getattr(self, "_didx", None)
        return d[self._b, : self._count] if d is not None else None

    @property
    def orig_img(self) -> np.ndarray:
        """HWC uint8 copy of the input image, as upstream `convert_torch2numpy_batch` makes it
        ((x.permute(1,2,0)*255).clamp(0,255).to(uint8)); materialised (one device→host copy) on first access.  An
        image source's is the image itself; a device frame's (uint8 HWC tensor sources) is copied to the host on first
        access too, and an NV12 frame's (NV12Frames sources) is converted to BGR on the device first."""
        if isinstance(self._orig_img, torch.Tensor):  # a device frame source: its kept copy, moved on first access
            self._orig_img = self._orig_img.cpu().numpy()
        elif hasattr(self._orig_img, "to_bgr"):  # an NV12 frame source: converted (ym_nv12_to_bgr) on first access
            self._orig_img = self._orig_img.to_bgr()
        if self._orig_img is None and self._orig_tensor is not None:
            t = self._orig_tensor
            self._orig_img = (t.permute(1, 2, 0).contiguous() * 255).clamp_(0, 255).to(torch.uint8).cpu().numpy()
        return self._orig_img

    def __len__(self):  # (upstream: the length of the first field that is set; a classification result: its nc)
        if self.boxes is None and self.obb is not None:
            return len(self.obb)
        return len(self.boxes) if self.boxes is not None else (len(self.probs) if self.probs is not None else 0)

    def _no_detections(self, what: str):
        if self.boxes is None and self.probs is not None:
            raise NotImplementedError(f"{what} needs detections: a classification result has probs only")
        if self.obb is not None:
            raise NotImplementedError(f"{what} is not offered for oriented boxes (Results.obb)")

    def verbose(self) -> str:
        """Upstream `Results.verbose`: "name conf, " of a classification result's top-5; else "n name(s), " per detected
        class in ascending class order, "(no detections), " for none."""
        if self.probs is not None:
            p = self.probs
            return ", ".join(f"{self.names[j]} {c:.2f}"
                             for j, c in zip(p.top5, torch.as_tensor(p.top5conf).tolist())) + ", "
        if len(self) == 0:
            return "(no detections), "
        cls, n = torch.as_tensor((self.boxes if self.boxes is not None else self.obb).cls).unique(return_counts=True)
        return "".join(f"{k} {self.names[int(c)]}{'s' * (k > 1)}, " for c, k in zip(cls.tolist(), n.tolist()))

    def _like(self, orig_tensor, boxes, masks, keypoints=None):
        r = Results(orig_tensor, self.names, boxes, masks, self.path, self.speed, keypoints=keypoints,
                    annotator=getattr(self, "_annotator", None))
        r._mask_geo = getattr(self, "_mask_geo", None)
        if orig_tensor is None:  # image-file / ndarray source: keep the loaded image and its shape
            r._orig_img = self._orig_img
            r.orig_shape = self.orig_shape
            if r.boxes is not None:
                r.boxes.orig_shape = self.orig_shape
            if r.masks is not None:
                r.masks.orig_shape = self.orig_shape
            if r.keypoints is not None:
                r.keypoints.orig_shape = self.orig_shape
        return r

    def __getitem__(self, idx):
        if self.boxes is None:  # a classification result: its probs, indexed; an OBB result: its rows
            r = self._like(self._orig_tensor, None, None)
            r.probs = self.probs[idx] if self.probs is not None else None
            r.obb = self.obb[idx] if self.obb is not None else None
            return r
        k = self.keypoints
        r = self._like(self._orig_tensor, self.boxes.data[idx],
                       self.masks.data[idx] if self.masks is not None else None,
                       k.data[idx].clone() if k is not None else None)
        if self.masks is not None:  # polygons already traced are sliced, not traced again
            self.masks._carry(r.masks, idx)
        return r

    def cpu(self):
        if self.boxes is None:  # a classification result: its probs on the host
            r = self._like(self._orig_tensor.cpu() if self._orig_tensor is not None else None, None, None)
            r.probs = self.probs.cpu() if self.probs is not None else None
            r.obb = self.obb.cpu() if self.obb is not None else None
            return r
        k = self.keypoints
        r = self._like(self._orig_tensor.cpu() if self._orig_tensor is not None else None, self.boxes.data.cpu(),
                       self.masks.data.cpu() if self.masks is not None else None,
                       k.data.cpu().clone() if k is not None else None)
        if self.masks is not None:
            self.masks._carry(r.masks)
        return r

    def plot(self, conf=True, line_width=None, kpt_radius=5, kpt_line=True, labels=True, boxes=True, masks=True,
             img=None, color_mode="class", save=False, filename=None, **ignored) -> np.ndarray:
        """Upstream `Results.plot`: the HWC uint8 image (channel order of `orig_img`) with boxes, labels, masks, keypoints,
        skeletons and track ids drawn in — by the GPU annotator of the engine that made this Results (csrc/ym_annot.hip,
        Engine.annotate; the drawing rules are DESIGN.md §17's, not OpenCV's).  img replaces the canvas; color_mode
        "class" | "instance"; save / filename as upstream.  font, font_size, pil, im_gpu, probs, show and any other
        keyword (upstream's txt_color, say) are accepted and ignored, with one log line, so ported calls keep working.
        A hand-built Results needs `annotator=`: there is no host painter, so RuntimeError without one.
        `orig_img`, the rows and the masks are left as they are."""
        from yolomi.annotate import plot_results
        self._no_detections("plot()")
        if ignored:
            import logging
            logging.getLogger(__name__).info(f"plot: ignoring {sorted(ignored)}")
        ann = getattr(self, "_annotator", None)
        if ann is None:
            raise RuntimeError("Results.plot() draws on the GPU: this Results was built by hand without annotator= "
                               "(an Engine, e.g. model.model.engine); there is no host fallback")
        out = plot_results(self, ann, conf=conf, line_width=line_width, kpt_radius=kpt_radius, kpt_line=kpt_line,
                           labels=labels, boxes=boxes, masks=masks, img=img, color_mode=color_mode)
        if save:
            self._write(out, filename)
        return out

    def save(self, filename=None, **plot_args):
        """Upstream `Results.save`: plot() written to `filename` (default: results_<name of path>) through Pillow, the
        BGR canvas converted to RGB.  Returns the file name."""
        return self._write(self.plot(**plot_args), filename)

    def _write(self, bgr: np.ndarray, filename=None) -> str:
        import os
        from PIL import Image
        filename = str(filename) if filename else f"results_{os.path.basename(self.path)}"
        Image.fromarray(np.ascontiguousarray(bgr[..., ::-1])).save(filename)
        return filename

    def summary(self, normalize=False, decimals=5):
        """Upstream `Results.summary`: one dict per detection; with masks, its polygon as "segments": {"x": [...],
        "y": [...]} (Masks.xy, divided by the image's width / height when `normalize`), rounded to `decimals`."""
        if self.probs is not None:  # classification: the top-1
            p = self.probs
            return [{"name": self.names[p.top1], "class": p.top1, "confidence": round(float(p.top1conf), decimals)}]
        if self.obb is not None:  # upstream: the four corners as "box"
            h, w = self.orig_shape if normalize and self.orig_shape is not None else (1, 1)
            pts = torch.as_tensor(self.obb.xyxyxyxy).cpu().tolist()
            return [{"name": self.names[int(row[-1])], "class": int(row[-1]), "confidence": round(row[-2], decimals),
                     "box": {f"{a}{k + 1}": round(p[k][j] / d, decimals) for k in range(4)
                             for j, (a, d) in enumerate((("x", w), ("y", h)))}}
                    for row, p in zip(torch.as_tensor(self.obb.data).cpu().tolist(), pts)]
        out = []
        is_track = self.boxes.is_track
        segs = self.masks.xy if self.masks is not None else None
        h, w = self.orig_shape if normalize and self.orig_shape is not None else (1, 1)
        for i, row in enumerate(self.boxes.data.tolist()):
            (x1, y1, x2, y2), conf, c = row[:4], row[-2], row[-1]
            out.append({"name": self.names[int(c)], "class": int(c), "confidence": round(conf, decimals),
                        "box": {"x1": round(x1, decimals), "y1": round(y1, decimals), "x2": round(x2, decimals),
                                "y2": round(y2, decimals)}})
            if is_track:
                out[-1]["track_id"] = int(row[-3])
            if segs is not None:
                out[-1]["segments"] = {"x": (segs[i][:, 0].astype(np.float64) / w).round(decimals).tolist(),
                                       "y": (segs[i][:, 1].astype(np.float64) / h).round(decimals).tolist()}
        return out

    def to_coco(self, image_id=None, class_map=None):
        """Upstream `pred_to_json`'s entries, one dict per detection: "image_id", "category_id" (the class, through
        `class_map` when given), "bbox" [x, y, w, h] of the top-left corner rounded to 3 decimals, "score" rounded to 5
        and, with masks, "segmentation": Masks.rle with "counts" as str (see Masks for which planes are COCO-ready)."""
        self._no_detections("to_coco()")
        if self.boxes is None:
            return []
        rles = self.masks.rle if self.masks is not None else None
        out = []
        for i, row in enumerate(torch.as_tensor(self.boxes.data).cpu().tolist()):
            (x1, y1, x2, y2), conf, c = row[:4], row[-2], int(row[-1])
            out.append({"image_id": image_id, "category_id": class_map[c] if class_map is not None else c,
                        "bbox": [round(x1, 3), round(y1, 3), round(x2 - x1, 3), round(y2 - y1, 3)],
                        "score": round(conf, 5)})
            if rles is not None:
                out[-1]["segmentation"] = {"size": list(rles[i]["size"]), "counts": rles[i]["counts"].decode("ascii")}
        return out

    def save_txt(self, txt_file, save_conf=False):
        """Upstream `Results.save_txt`: one line per detection appended to `txt_file` — `cls x y w h` (the box,
        normalised) for detect, `cls x1 y1 x2 y2 ...` (Masks.xyn) for segment, the box then the normalised keypoints
        (with their visibility when they have one) for pose; then the confidence when `save_conf`, then the track id of
        tracked rows.  Values are written with %g.  Nothing is written for an image without detections."""
        import os
        self._no_detections("save_txt()") if self.obb is not None else None
        if self.probs is not None:  # classification: upstream's "{conf:.2f} {name}" lines of the top-5
            p = self.probs
            texts = [f"{c:.2f} {self.names[j]}" for j, c in zip(p.top5, torch.as_tensor(p.top5conf).tolist())]
            d = os.path.dirname(str(txt_file))
            if d:
                os.makedirs(d, exist_ok=True)
            with open(txt_file, "a", encoding="utf-8") as f:
                f.writelines(t + "\n" for t in texts)
            return
        boxes, masks, kpts = self.boxes, self.masks, self.keypoints
        xywhn = torch.as_tensor(boxes.xywhn).cpu().tolist()
        rows = torch.as_tensor(boxes.data).cpu().tolist()
        segs = masks.xyn if masks is not None else None
        kxyn = torch.as_tensor(kpts.xyn).cpu() if kpts is not None else None
        kconf = torch.as_tensor(kpts.conf).cpu() if kpts is not None and kpts.has_visible else None
        texts = []
        for j, row in enumerate(rows):
            line = (int(row[-1]), *xywhn[j])
            if segs is not None:
                line = (int(row[-1]), *segs[j].reshape(-1).tolist())
            if kxyn is not None:
                k = torch.cat((kxyn[j], kconf[j][:, None]), 1) if kconf is not None else kxyn[j]
                line += (*k.reshape(-1).tolist(),)
            line += (row[-2],) * bool(save_conf) + ((int(row[-3]),) if boxes.is_track else ())
            texts.append(("%g " * len(line)).rstrip() % line)
        if texts:
            d = os.path.dirname(str(txt_file))
            if d:
                os.makedirs(d, exist_ok=True)
            with open(txt_file, "a", encoding="utf-8") as f:
                f.writelines(t + "\n" for t in texts)

    def __repr__(self):
        if self.boxes is None and self.probs is not None:
            return f"Results(probs={tuple(self.probs.shape)}, orig_shape={self.orig_shape})"
        if self.boxes is None and self.obb is not None:
            return f"Results(obb={len(self.obb)}, orig_shape={self.orig_shape})"
        return f"Results(boxes={len(self.boxes)}, orig_shape={self.orig_shape})"
