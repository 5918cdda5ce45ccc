"""Results / Boxes / Masks: the per-image result objects `YOLO11Model.predict` returns.

Mirrors the subset of the Ultralytics Results contract the reference's consumers read
(/root/reference/demos/detection_demo.py:116-132 `.boxes.xyxy/.conf/.cls` per box, `.cpu().numpy()`;
/root/reference/utils/visualization.py:46-74, 370-437 `.names`, `len(boxes)`, iteration, `.masks.data`).
Tensors stay on the model's device, like upstream.
"""
from __future__ import annotations

from typing import Dict, Optional

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
    device->host reads for all n instances) and cached; a hand-built Masks needs `engine=`: there is no host tracer."""

    def __init__(self, masks, orig_shape=None, engine=None):
        super().__init__(masks)
        self.orig_shape = orig_shape
        self._engine = engine
        self._xy = None

    def _extra(self):
        return (self.orig_shape, self._engine)

    def _carry(self, other, idx=None):
        """Hand the computed polygons (all, or those `idx` selects) to `other`, a view of the same planes."""
        if self._xy is not None:
            if idx is None:
                other._xy = self._xy
            else:
                if isinstance(idx, torch.Tensor):
                    idx = idx.cpu().numpy()
                sel = np.arange(len(self._xy))[idx]
                other._xy = [self._xy[i] for i in np.atleast_1d(sel).tolist()]
        return other

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
            if self._engine is None:
                raise RuntimeError("Masks.xy traces the polygons on the GPU: this Masks was built by hand without "
                                   "engine= (an Engine, e.g. model.model.engine); there is no host fallback")
            from yolomi.preprocess import scale_coords
            planes = torch.as_tensor(self.data)
            if planes.dim() == 2:
                planes = planes[None]
            if planes.dtype not in (torch.uint8, torch.bool):
                planes = planes != 0
            if planes.device != self._engine.device:  # after Results.cpu(): one upload
                planes = planes.to(self._engine.device)
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
        self.boxes = Boxes(boxes, self.orig_shape)
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
        if self._boxes is None:
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
        ((x.permute(1,2,0)*255).clamp(0,255).to(uint8)); materialised (one device→host copy) on first access."""
        if self._orig_img is None and self._orig_tensor is not None:
            t = self._orig_tensor
            self._orig_img = (t.permute(1, 2, 0).contiguous() * 255).clamp_(0, 255).to(torch.uint8).cpu().numpy()
        return self._orig_img

    def __len__(self):
        return len(self.boxes)

    def _like(self, orig_tensor, boxes, masks, keypoints=None):
        r = Results(orig_tensor, self.names, boxes, masks, self.path, self.speed, keypoints=keypoints,
                    annotator=getattr(self, "_annotator", None))
        r._mask_geo = getattr(self, "_mask_geo", None)
        if orig_tensor is None:  # image-file / ndarray source: keep the loaded image and its shape
            r._orig_img = self._orig_img
            r.orig_shape = self.orig_shape
            r.boxes.orig_shape = self.orig_shape
            if r.masks is not None:
                r.masks.orig_shape = self.orig_shape
            if r.keypoints is not None:
                r.keypoints.orig_shape = self.orig_shape
        return r

    def __getitem__(self, idx):
        k = self.keypoints
        r = self._like(self._orig_tensor, self.boxes.data[idx],
                       self.masks.data[idx] if self.masks is not None else None,
                       k.data[idx].clone() if k is not None else None)
        if self.masks is not None:  # polygons already traced are sliced, not traced again
            self.masks._carry(r.masks, idx)
        return r

    def cpu(self):
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

    def save_txt(self, txt_file, save_conf=False):
        """Upstream `Results.save_txt`: one line per detection appended to `txt_file` — `cls x y w h` (the box,
        normalised) for detect, `cls x1 y1 x2 y2 ...` (Masks.xyn) for segment, the box then the normalised keypoints
        (with their visibility when they have one) for pose; then the confidence when `save_conf`, then the track id of
        tracked rows.  Values are written with %g.  Nothing is written for an image without detections."""
        import os
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
        return f"Results(boxes={len(self.boxes)}, orig_shape={self.orig_shape})"
