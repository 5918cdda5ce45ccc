"""YOLO11Model / YOLO11Factory — drop-in for /root/reference/core/model.py on MI355X.

Same constructor, `predict`, `benchmark`, `get_model_info`, `.model` surface as the reference
(`core/model.py:29-295`), but `predict` runs the hand-written gfx950 path (`yolomi.engine.Engine` → libyolomi.so →
one HIP-graph replay per batch) instead of delegating to `ultralytics.YOLO.predict` (`core/model.py:133`).

Scope: tasks detect/segment/pose, sizes n/s/m/l/x, `torch.Tensor` sources (BCHW or CHW, H,W % 32 == 0,
LoadTensor's /255 rule).  There is no CPU fallback: a CPU device or a missing libyolomi.so raises.
"""
from __future__ import annotations

import logging
import os
import time
from pathlib import Path
from typing import Any, Dict, List, Optional, Union

import numpy as np
import torch

from yolomi.engine import Engine
from yolomi.synth import synth_weights

from .results import LazyCounts, Results

logger = logging.getLogger(__name__)

COCO_NAMES = dict(enumerate((
    "person", "bicycle", "car", "motorcycle", "airplane", "bus", "train", "truck", "boat", "traffic light",
    "fire hydrant", "stop sign", "parking meter", "bench", "bird", "cat", "dog", "horse", "sheep", "cow", "elephant",
    "bear", "zebra", "giraffe", "backpack", "umbrella", "handbag", "tie", "suitcase", "frisbee", "skis", "snowboard",
    "sports ball", "kite", "baseball bat", "baseball glove", "skateboard", "surfboard", "tennis racket", "bottle",
    "wine glass", "cup", "fork", "knife", "spoon", "bowl", "banana", "apple", "sandwich", "orange", "broccoli",
    "carrot", "hot dog", "pizza", "donut", "cake", "chair", "couch", "potted plant", "bed", "dining table", "toilet",
    "tv", "laptop", "mouse", "remote", "keyboard", "cell phone", "microwave", "oven", "toaster", "sink",
    "refrigerator", "book", "clock", "vase", "scissors", "teddy bear", "hair drier", "toothbrush")))


class _ModelHandle:
    """What the reference exposes as `YOLO11Model.model` (an `ultralytics.YOLO`): callers use `.eval()`
    (speed_benchmark.py:323), `.parameters()` / `.model.parameters()` (model.py:240), `.names`."""

    def __init__(self, state_dict: Dict[str, np.ndarray], engine: Engine, names: Dict[int, str]):
        self._sd = state_dict
        self._params = {k: torch.from_numpy(np.asarray(v)) for k, v in state_dict.items()
                        if not k.endswith("num_batches_tracked")}
        for p in self._params.values():
            p.requires_grad_(True)
        self.engine = engine
        self.names = names
        self.model = self
        self.training = False

    def eval(self):
        return self

    def parameters(self):
        return iter(self._params.values())

    def state_dict(self):
        return dict(self._params)

    def state_dict_numpy(self) -> Dict[str, np.ndarray]:
        """The Ultralytics-key weights this model was packed from (what a quantizer re-packs)."""
        if not self._sd:
            raise ValueError("this model was built from a packed blob only; its weights are not on the host")
        return self._sd


def _load_state_dict(path: Path) -> Dict[str, np.ndarray]:
    """Weights file → Ultralytics-key state dict. Loaders that execute nothing from the file only."""
    suf = path.suffix.lower()
    if suf == ".safetensors":
        from safetensors.numpy import load_file
        return dict(load_file(str(path)))
    if suf == ".npz":
        with np.load(path, allow_pickle=False) as z:
            return {k: z[k] for k in z.files}
    if suf == ".pt":
        try:
            obj = torch.load(path, map_location="cpu", weights_only=True)
        except Exception:  # a pickled Ultralytics model (YOLO('yolo11n.pt') checkpoints): restricted unpickler
            from yolomi.ptimport import load_ultralytics_checkpoint
            return load_ultralytics_checkpoint(str(path))
        if isinstance(obj, dict) and "state_dict" in obj:
            obj = obj["state_dict"]
        if not isinstance(obj, dict) or not all(isinstance(v, torch.Tensor) for v in obj.values()):
            raise ValueError(f"{path}: expected a state dict of tensors")
        return {k: v.float().numpy() if v.is_floating_point() else v.numpy() for k, v in obj.items()}
    raise ValueError(f"unsupported weights file {path} (use an Ultralytics .pt, a state-dict .pt, .safetensors or .npz)")


# ---------------------------------------------------------------------- the call path's shared pieces
# predict(), track() and retina_masks share these; they take tensors and plain values (and run on CPU tensors).
def _nms_kwargs(kwargs, conf: float = 0.25) -> Dict[str, Any]:
    """The NMS keywords of a predict / track call under Engine.run's names (conf: the call's default threshold)."""
    return {"conf": float(kwargs.get("conf", conf)), "iou": float(kwargs.get("iou", 0.7)),
            "max_det": int(kwargs.get("max_det", 300)), "classes": kwargs.get("classes", None),
            "agnostic": bool(kwargs.get("agnostic_nms", False))}


def _speed(t0, t1) -> Dict[str, float]:
    """Host ms of the call so far: preprocess = between the two stamps, inference = since the second (a forward still
    in flight on the asynchronous path is not in it)."""
    return {"preprocess": (t1 - t0) * 1e3, "inference": (time.perf_counter() - t1) * 1e3, "postprocess": 0.0}


def _rows_to_source(out, n, in_shape, shapes, kcol: Optional[int] = None, kpt_shape=None):
    """ops.scale_boxes of image b's first n[b] rows back to its source image of shapes[b], in place; kcol: the rows'
    first keypoint column (6, track rows 7) — the (K, ndim) keypoints go through ops.scale_coords; None: boxes only."""
    from yolomi.preprocess import scale_boxes, scale_coords
    for b in range(len(n)):
        if n[b]:
            scale_boxes(in_shape, out[b, : n[b], :4], shapes[b])
            if kcol is not None:
                K, nd = kpt_shape
                scale_coords(in_shape, out[b, : n[b], kcol:kcol + K * nd].view(n[b], K, nd), shapes[b])


def _lazy_results(im, out, cnt, names, eng, t0, t1, sync, tracked=False, det_idx=None) -> List[Results]:
    """The tail of an asynchronous call (tensor source, detect / pose): the NMS kernel wrote this call's rows AND its B
    counts (the int32 words behind the rows) into a fresh buffer, so no host sync is needed: the Results read the counts
    on first access (one device->host read shared by the call's B Results), and back-to-back calls queue their forwards
    with no host gap between them.  sync (per-call latency loops): return only once the forward is done.  tracked,
    det_idx: track()'s rows and the detection row behind each."""
    lazy = LazyCounts(cnt, torch.cuda.current_stream(im.device))
    if sync:
        lazy[0]
    speed = _speed(t0, t1)  # host time of the calls (the forward itself runs asynchronously)
    kpt_shape = eng.kpt_shape
    return [Results.from_batch(im, b, names, out, lazy, path=f"image{b}.jpg", speed=speed, kpt_shape=kpt_shape,
                               tracked=tracked, det_idx=det_idx, annotator=eng) for b in range(im.shape[0])]


def _image_results(imsrc, out, n, names, eng, speed, ncol: int, pose: bool) -> List[Results]:
    """The tail of an image-source detect / pose call: boxes = the first ncol columns of the rows (already in each
    source image's coordinates), a pose model's keypoints the nk columns behind them."""
    return [Results.from_image(imsrc[0][b], imsrc[1][b], names, out[b, : n[b], :ncol], speed=speed,
                               keypoints=(out[b, : n[b], ncol:ncol + eng.nk].reshape(n[b], *eng.kpt_shape)
                                          if pose else None), annotator=eng)
            for b in range(len(n))]


def _segment_results(im, imsrc, names, eng, speed, out, n, keep, offs, planes, whole: bool, geo=None) -> List[Results]:
    """The B Results of a segment call; the predictor keeps only detections whose mask is non-empty (keep: the flags,
    image b's at offs[b]).  whole: planes is one bool tensor of all the call's mask planes, image b's at offs[b] (the
    Results get it whole, with that offset); else a list of B per-image (n[b], h, w) views (retina_masks: native sizes
    differ).  geo: per image (uh, uw, top, left) when an image source's masks are in letterboxed coordinates."""
    res = []
    for b in range(len(n)):
        kb = keep[offs[b]:offs[b] + n[b]]
        if all(kb) and imsrc is None:  # the common case: boxes, masks and input slice as views taken on access
            res.append(Results.from_batch(im, b, names, out, n[b], path=f"image{b}.jpg", speed=speed,
                                          masks=planes if whole else planes[b], moff=offs[b] if whole else 0,
                                          annotator=eng))
            continue
        bx, mk = out[b, :n[b], :6], planes[offs[b]:offs[b] + n[b]] if whole else planes[b]
        if not all(kb):  # else every kept detection has a mask pixel — views, no gathers
            sel = torch.tensor([i for i, k in enumerate(kb) if k], dtype=torch.long, device=out.device)
            bx = out[b].index_select(0, sel)[:, :6] if whole else bx.index_select(0, sel)  # (strides as they were)
            mk = mk.index_select(0, sel)
        if imsrc is None:
            res.append(Results(im[b], names, bx, path=f"image{b}.jpg", speed=speed, masks=mk, annotator=eng))
        else:  # letterboxed masks: plot() maps the image into its window of the plane (geo)
            res.append(Results.from_image(imsrc[0][b], imsrc[1][b], names, bx, speed=speed, masks=mk, annotator=eng,
                                          mask_geo=geo[b] if geo is not None else None))
    return res


class YOLO11Model:
    SUPPORTED_TASKS = {
        "detect": "yolo11n.pt",
        "segment": "yolo11n-seg.pt",
        "classify": "yolo11n-cls.pt",
        "pose": "yolo11n-pose.pt",
        "obb": "yolo11n-obb.pt",
    }
    SUPPORTED_SIZES = ["n", "s", "m", "l", "x"]
    HIP_TASKS = ("detect", "segment", "pose")

    def __init__(self, model_path: Optional[Union[str, Path]] = None, task: str = "detect", size: str = "n",
                 device: Optional[str] = None, verbose: bool = True, dtype: str = "x3", seed: int = 0,
                 weights_blob: Optional[bytes] = None, qparams: Optional[Dict] = None,
                 state_dict: Optional[Dict[str, np.ndarray]] = None, weights_from: Optional[tuple] = None,
                 kpt_shape: Optional[tuple] = None):
        """Extra keyword arguments over the reference: `dtype` — 'x3' (the default: fp32 activations, every conv GEMM
        as three fp16 MFMAs on hi/lo split operands; meets the reference fp32 path's 1e-3 px / score bar, DESIGN.md
        §3), 'f16' (opt-in throughput mode: fp16 storage + fp32 accumulate, ~0.6 px / 3e-3 off the fp32 path),
        'f32' (exact-f32 MFMA), or 'i8' / 'f8' = the PTQ plans, which need calibrated `qparams`; see
        optimization.quantization.PostTrainingQuantizer), `seed` of the synthetic weights used when no `model_path`
        is given, `weights_blob` = an already packed model (e.g. received over an RCCL broadcast from rank 0), and
        `state_dict` = weights already in memory, `weights_from` = (rccl comm, root): receive the root rank's model
        over RCCL, or a yolomi Runtime that already received it (yolomi.dist.rccl_broadcast_model), `kpt_shape` =
        (K, 2 | 3) of a pose model (default: (17, 3) for synthetic weights; for a checkpoint (nk // 3, 3) when its nk
        keypoint channels divide by 3, else (nk // 2, 2))."""
        self.task = task
        self.size = size
        self.device = device or self._get_default_device()
        self.verbose = verbose
        self.model_path = model_path
        self.dtype = dtype
        self.seed = seed
        self._blob = weights_blob
        self._qparams = qparams
        self._sd = state_dict
        self._weights_from = weights_from
        self._kpt_shape = tuple(kpt_shape) if kpt_shape is not None else None
        self.optimization_history: List[Dict[str, Any]] = []
        # batch-sharded multi-GPU (yolomi.dist.enable_global_rule): callable x -> (1,) device max of the GLOBAL batch
        self.global_batch_max = None
        self._mask_cap = 64  # segment: mask slots per image enqueued before the sync (grows on demand)
        self._validate_inputs()
        self.model = self._load_model()
        self.original_model = None
        logger.info(f"YOLO11 model initialized: task={task}, size={size}, device={self.device}")

    def _get_default_device(self) -> str:
        return "cuda" if torch.cuda.is_available() else "cpu"

    def _validate_inputs(self):
        if self.task not in self.SUPPORTED_TASKS:
            raise ValueError(f"Unsupported task: {self.task}. Supported: {list(self.SUPPORTED_TASKS.keys())}")
        if self.size not in self.SUPPORTED_SIZES:
            raise ValueError(f"Unsupported size: {self.size}. Supported: {self.SUPPORTED_SIZES}")
        if self.task not in self.HIP_TASKS:
            raise NotImplementedError(f"task {self.task!r} has no MI355X plan (supported: {self.HIP_TASKS})")

    def _load_model(self) -> _ModelHandle:
        dev = torch.device(self.device)
        if dev.type != "cuda":
            raise RuntimeError(f"YOLO11Model runs on MI355X (gfx950) only; device {self.device!r} has no HIP path")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        self._dev = dev
        try:
            if self._blob is not None or self._weights_from is not None:
                sd = self._sd or {}
            elif self._sd is not None:
                sd = self._sd
            elif self.model_path:
                sd = _load_state_dict(Path(self.model_path))
            else:  # the reference fetches yolo11{size}.pt by name; offline we synthesise weights of that graph
                sd = synth_weights(self.size, self.task, self.seed)
            nc = 1 if self.task == "pose" else 80
            kpt_shape = self._kpt_shape
            if sd and self._blob is None:  # the checkpoint decides the architecture, as YOLO(model_path) does
                from yolomi.arch import infer_arch, infer_kpt_shape
                scale, task, nc = infer_arch(sd, kpt_shape)
                kpt_shape = infer_kpt_shape(sd, kpt_shape) if task == "pose" else None
                if (scale, task) != (self.size, self.task):
                    logger.warning(f"{self.model_path or 'state_dict'} holds a yolo11{scale} {task} model "
                                   f"(nc={nc}); using it instead of size={self.size!r} task={self.task!r}")
                    self.size, self.task = scale, task
            engine = Engine(self.size, self.task, sd, dev, self.dtype, blob=self._blob, qparams=self._qparams, nc=nc,
                            receive=self._weights_from, kpt_shape=kpt_shape if self.task == "pose" else None)
            names = COCO_NAMES if nc == 80 else {i: f"class{i}" for i in range(nc)}
            if self.task == "pose" and nc == 1:
                names = {0: "person"}
        except Exception as e:
            logger.error(f"Failed to load model: {e}")
            raise
        engine.set_names(names)  # the labels of Results.plot() / Engine.annotate
        return _ModelHandle(sd, engine, names)

    # ------------------------------------------------------------------ hot path
    def _as_batch(self, source, imgsz: int = 640):
        """(batch tensor on the device, LoadTensor eps, image-source info or None).  Tensors follow LoadTensor; paths,
        directories, HWC uint8 BGR ndarrays and PIL images are letterboxed on the GPU (yolomi/preprocess.py)."""
        if isinstance(source, (list, tuple)) and source and all(isinstance(s, torch.Tensor) for s in source):
            source = torch.stack(list(source))
        if not isinstance(source, torch.Tensor):
            from yolomi.preprocess import batch_geometry, expand_sources, letterbox_batch
            imgs, paths = expand_sources(source)
            stream = torch.cuda.current_stream(self._dev).cuda_stream
            geo = batch_geometry(imgs, imgsz)  # once: the letterbox kernel and the masks' window use the same values
            im, shapes = letterbox_batch(self.model.engine.rt, imgs, self._dev, imgsz=imgsz, stream=stream, geo=geo)
            return im, torch.finfo(torch.float32).eps, (imgs, paths, shapes,
                                                        [(g[0], g[1], g[2], g[4]) for g in geo])  # (uh, uw, top, left)
        im = source
        if im.dim() != 4:
            if im.dim() != 3:
                raise ValueError("torch.Tensor inputs should be BCHW i.e. shape(1, 3, 640, 640)")
            im = im.unsqueeze(0)
        if im.shape[1] != 3:
            raise ValueError(f"expected 3 input channels, got shape {tuple(im.shape)}")
        if im.shape[2] % 32 or im.shape[3] % 32:
            raise ValueError(f"torch.Tensor inputs should be BCHW divisible by stride 32, got {tuple(im.shape)}")
        if not im.is_floating_point():
            raise TypeError(f"tensor source must be floating point, got {im.dtype}")
        eps = torch.finfo(im.dtype).eps
        if im.device != self._dev:
            im = im.to(self._dev)
        im = im.float().contiguous()
        return im, eps, None

    def _begin(self, source, kwargs):
        """The start of every call: (batch, LoadTensor eps, image-source info or None, the global batch max or None,
        the time stamps before and after preprocessing)."""
        t0 = time.perf_counter()
        im, eps, imsrc = self._as_batch(source, int(kwargs.get("imgsz", 640)))
        t1 = time.perf_counter()
        bm = self.global_batch_max(im) if self.global_batch_max is not None and imsrc is None else None
        return im, eps, imsrc, bm, t0, t1

    def predict(self, source, **kwargs) -> List[Results]:
        nms = _nms_kwargs(kwargs)
        augment = bool(kwargs.get("augment", False))
        if kwargs.get("embed", None) is not None:
            return self._predict_embed(source, kwargs)
        if augment and self.task != "detect":  # as upstream: only the Detect head is augmented
            logger.warning(f"augment=True is not supported for {self.task} models: predicting at a single scale")
            augment = False
        im, eps, imsrc, bm, t0, t1 = self._begin(source, kwargs)
        eng = self.model.engine
        names = self.model.names
        if self.task == "segment" and bool(kwargs.get("retina_masks", False)):  # detect / pose ignore it, as upstream
            return self._predict_retina(im, eps, imsrc, bm, t0, t1, nms)
        run = eng.run_tta if augment else eng.run  # test-time augmentation: three scaled passes, one NMS
        B, max_det = im.shape[0], nms["max_det"]
        if self.task != "segment" and imsrc is None:  # asynchronous: rows and counts in one fresh buffer, no host sync
            out, cnt = eng.rows_buffer(B, max_det)
            run(im, in_eps=eps, batch_max=bm, dets_out=out, counts_after=True, **nms)
            return _lazy_results(im, out, cnt, names, eng, t0, t1, kwargs.get("sync", False))
        # the NMS kernel writes this call's rows straight into a fresh tensor (the Results keep views into it)
        out = torch.empty((B, max_det, 6 + eng.nm), dtype=torch.float32, device=im.device)
        _, counts = run(im, in_eps=eps, batch_max=bm, dets_out=out, **nms)
        pose = self.task == "pose"
        if self.task == "segment":  # process_mask(upsample=True) on the GPU, in letterboxed coordinates
            masks, keep, offs, n = self._masks_for(out, counts[:B], max_det, *im.shape[2:])
        else:
            n = counts[:B].tolist()  # the device→host sync of a predict call
        if imsrc is not None:  # back to each original image
            _rows_to_source(out, n, im.shape[2:], imsrc[2], 6 if pose else None, eng.kpt_shape)
        speed = _speed(t0, t1)
        if self.task != "segment":
            return _image_results(imsrc, out, n, names, eng, speed, 6, pose)
        mb = masks.view(torch.bool).reshape(-1, *im.shape[2:])  # the kernel writes 0/1 bytes: a bool view, no copy
        return _segment_results(im, imsrc, names, eng, speed, out, n, keep, offs, mb, True,
                                imsrc[3] if imsrc is not None else None)

    def _masks_for(self, out, counts, max_det, H, W):
        """The mask planes of a segment call's rows, and the slot policy: (masks, keep, offs, n) — uint8 planes, image
        b's n[b] at plane offs[b], and their non-empty flags at the same offsets — and `_mask_cap` for the next call.
        The masks of the first `cap` detections per image are enqueued behind the forward, reading the device counts, so
        ONE device→host read returns counts and non-empty flags; a batch with more detections per image than `cap` takes
        the exact-size two-read path (and raises `cap` for the next call).
        Memory: the slot buffer is B x cap x H x W bytes, so it is only used within YM_MASK_BUDGET_MB
        (256 MB by default; larger batches take the exact-size path), `cap` follows the recent detection counts down as
        well as up (1.25x the last maximum rounded up to 16, 16..max_det: a steady stream of batches keeps its slots
        over half full, so no compaction copy runs), and a mostly empty slot buffer is compacted before the Results
        views are taken, so results kept by the caller retain at most twice the bytes of their masks."""
        eng = self.model.engine
        B = counts.shape[0]
        cap = min(self._mask_cap, max_det)
        budget = int(os.environ.get("YM_MASK_BUDGET_MB", "256")) << 20
        fl = None
        if B * cap * H * W <= budget:
            mslots, flags = eng.masks_slots(out, counts, cap, H, W)
            fl = flags.tolist()  # the device→host sync of a segment predict call
            n = fl[B * cap:]
        else:
            n = counts.tolist()
        if fl is not None and max(n) <= cap:
            masks, keep = mslots, fl
            offs = [b * cap for b in range(B + 1)]
            if 2 * sum(n) < B * cap:  # compact the kept slots: one gather
                rows = [b * cap + i for b in range(B) for i in range(n[b])]
                masks = mslots.reshape(B * cap, H, W).index_select(
                    0, torch.tensor(rows, dtype=torch.long, device=mslots.device))
                keep = [fl[r] for r in rows]
                offs = [0]
                for b in range(B):
                    offs.append(offs[-1] + n[b])
        else:
            masks, nonempty, offs = eng.masks(out, n, H, W)
            keep = nonempty.tolist()
        self._mask_cap = max(16, min(max_det, -(-(5 * max(max(n), 1)) // 64) * 16))  # ceil(1.25 max / 16) * 16
        return masks, keep, offs, n

    def track(self, source, persist: bool = False, tracker="bytetrack.yaml", **kwargs) -> List[Results]:
        """Ultralytics `model.track(source, persist=..., tracker="bytetrack.yaml")`: predict(), then ByteTrack on the GPU
        right behind the NMS (Engine.track, csrc/ym_track.hip).  Image b of the batch is video stream b:
        call it once per frame (or per batch of B cameras' frames) with persist=True to carry ids across calls;
        persist=False (the default, as upstream) starts over.  `Results.boxes` is (n, 7) [x1, y1, x2, y2, id, conf, cls]
        — the filter's box of every activated track matched in this frame, ascending ids, which count from 1 per
        stream — `boxes.id` / `boxes.is_track` are set, and a pose model's keypoints are those of the detection behind
        each track.  conf defaults to 0.1 (ByteTrack's second association wants the low scores); the other predict
        keywords pass through, max_det <= 300; augment and retina_masks are ignored.  For tensor sources the call is
        asynchronous like predict().  tracker: "bytetrack.yaml", a YAML file with its keys, or a dict
        (yolomi.track.tracker_config); "botsort.yaml" and segment models raise NotImplementedError; a batch size other
        than the live tracker's under persist=True raises ValueError."""
        from yolomi.track import tracker_config
        cfg = tracker_config(tracker)
        if self.task == "segment":
            raise NotImplementedError("track() is offered for detect and pose models: a segment model's masks would "
                                      "have to be re-gathered by the tracks' detection rows")
        ignored = [k for k in ("augment", "retina_masks") if kwargs.get(k, False)]
        if ignored:
            logger.debug(f"track: {', '.join(ignored)} ignored")
        im, eps, imsrc, bm, t0, t1 = self._begin(source, kwargs)
        eng = self.model.engine
        names = self.model.names
        out, cnt, idx = eng.track(im, cfg, persist=bool(persist), **_nms_kwargs(kwargs, conf=0.1), in_eps=eps,
                                  batch_max=bm)
        if imsrc is None:  # asynchronous, as predict(): the counts are read on first access
            return _lazy_results(im, out, cnt, names, eng, t0, t1, kwargs.get("sync", False), True, idx)
        n = cnt.tolist()  # the device->host sync of an image-source call
        pose = self.task == "pose"  # scale_boxes / scale_coords after tracking, on the track rows
        _rows_to_source(out, n, im.shape[2:], imsrc[2], 7 if pose else None, eng.kpt_shape)
        return _image_results(imsrc, out, n, names, eng, _speed(t0, t1), 7, pose)

    def _predict_embed(self, source, kwargs) -> List[torch.Tensor]:
        """predict(source, embed=[layers]): Ultralytics _predict_once's embed branch.  One 1-D fp32 device tensor per
        image (views of one fresh (B, sum C_i) buffer): the global-average-pooled outputs of the named layers,
        concatenated in ascending layer order; the forward stops at the last of them (Engine.embed).  Preprocessing is
        predict's own (letterboxed image sources, LoadTensor's /255 rule for tensors).  augment and retina_masks do
        not apply (upstream returns before either is looked at).  Unlike upstream, which ignores an index no layer
        has and returns ordinary predictions, an index outside 0..22, a non-integer or an empty list raises."""
        from yolomi.arch import normalize_embed
        eng = self.model.engine
        layers = normalize_embed(kwargs["embed"])
        eng._embed_table(layers)  # (raises for a layer the plan does not store, or a quantized plan)
        ignored = [k for k in ("augment", "retina_masks") if kwargs.get(k, False)]
        if ignored:
            logger.debug(f"embed={list(layers)}: {', '.join(ignored)} ignored (the forward stops at layer {layers[-1]})")
        im, eps, _, bm, _, _ = self._begin(source, kwargs)
        # the captured pooling stage writes the engine's own (B, sum C) tensor (its address is part of the graph key:
        # fresh rows per call would capture a graph per call); the caller gets a copy that later calls leave alone
        return list(eng.embed(im, layers, in_eps=eps, batch_max=bm).clone().unbind(0))

    def embed(self, source, **kwargs) -> List[torch.Tensor]:
        """Ultralytics Model.embed: predict(source, embed=[len(model.model) - 2]) unless `embed` is given — layer 22,
        the last neck C3k2 (256 channels for yolo11n, 512 for yolo11s)."""
        from yolomi.arch import DEFAULT_EMBED
        if kwargs.get("embed", None) is None:
            kwargs["embed"] = list(DEFAULT_EMBED)
        return self.predict(source, **kwargs)

    def _predict_retina(self, im, eps, imsrc, bm, t0, t1, nms) -> List[Results]:
        """predict(..., retina_masks=True) on a segment model: SegmentationPredictor.construct_result's other branch.
        The boxes go to each image's native pixels first (scale_boxes; a tensor source is its own native image), then
        ops.process_mask_native on the GPU (Engine.masks_native, csrc/ym_mask_native.hip): the prototype-resolution
        mask's letterbox window resized to (h0, w0), cropped to the box there, > 0; detections whose mask is empty are
        dropped.  `masks.data` is (n, h0, w0) bool and `masks.orig_shape` (h0, w0), per image.
        The output size depends on the counts, so this is the two-read form (counts, then the non-empty flags); there
        is no slot buffer and `_mask_cap` is not touched.  No memory cap either: the packed mask buffer is the sum of
        n_b * h0_b * w0_b bytes, and torch's allocator error propagates when that does not fit."""
        eng = self.model.engine
        B, _, H, W = im.shape
        out = torch.empty((B, nms["max_det"], 6 + eng.nm), dtype=torch.float32, device=im.device)
        _, counts = eng.run(im, in_eps=eps, batch_max=bm, dets_out=out, **nms)
        n = counts[:B].tolist()  # the first device→host read: the counts size the packed mask buffer
        shapes = [(H, W)] * B if imsrc is None else [tuple(s) for s in imsrc[2]]
        if imsrc is not None:
            _rows_to_source(out, n, (H, W), shapes)
        packed, nonempty, offs, boffs = eng.masks_native(out, n, H, W, shapes)
        keep = nonempty.tolist()  # the second read
        speed = _speed(t0, t1)
        pb = packed.view(torch.bool)  # the kernel writes 0/1 bytes: a bool view, no copy
        return _segment_results(im, imsrc, self.model.names, eng, speed, out, n, keep, offs,
                                [pb[boffs[b]:boffs[b + 1]].view(n[b], *shapes[b]) for b in range(B)], False)

    def __call__(self, source, **kwargs):
        return self.predict(source, **kwargs)

    # ------------------------------------------------------------------ reference surface
    def get_model_info(self) -> Dict[str, Any]:
        info = {
            "task": self.task,
            "size": self.size,
            "device": self.device,
            "model_path": self.model_path,
            "optimization_history": self.optimization_history,
        }
        params = list(self.model.model.parameters())
        total = sum(p.numel() for p in params)
        info.update({
            "total_parameters": total,
            "trainable_parameters": sum(p.numel() for p in params if p.requires_grad),
            "model_size_mb": total * 4 / (1024 * 1024),
        })
        return info

    def benchmark(self, data_source, num_runs: int = 100, warmup_runs: int = 10) -> Dict[str, float]:
        """Same protocol as the reference (core/model.py:253-291): warm-up, then wall-clock per predict()."""
        for _ in range(warmup_runs):
            _ = self.predict(data_source, verbose=False, sync=True)
        times = []
        for _ in range(num_runs):  # sync=True: each call's wall clock covers its whole forward (predict is async)
            start = time.time()
            _ = self.predict(data_source, verbose=False, sync=True)
            times.append(time.time() - start)
        avg = sum(times) / len(times)
        return {"avg_inference_time": avg, "min_inference_time": min(times), "max_inference_time": max(times),
                "fps": 1.0 / avg}

    def train(self, *a, **k):
        raise NotImplementedError("training is out of scope for the MI355X inference path (SURVEY §2)")

    export = train

    def val(self, data=None, imgsz: int = 640, batch: int = 16, conf: float = 0.001, iou: float = 0.7,
            max_det: int = 300, augment: bool = False, **ignored):
        """Ultralytics `model.val(data=...)` for detect and pose plans (reference core/validator.py:141): the val
        loader's rect batches, `Engine.run(multi_label=True)` per batch, mAP / precision / recall as upstream computes
        them (yolomi/val.py).  data: a dataset YAML (path / val / names), a directory with images/ and labels/, or a
        list of (HWC uint8 BGR ndarray, (m, 5) normalised labels).  Returns an object with `.box.map / .map50 / .map75 /
        .mp / .mr`, `.speed` and `.results_dict`.  augment=True: every batch goes through the test-time-augmented run
        (Engine.run_tta).  Other Ultralytics val keywords are accepted and ignored.
        A pose model reads pose labels (`cls cx cy w h` and K·ndim keypoint values per row; a YAML `kpt_shape` must be
        the model's; in-memory labels are (m, 5 + K·ndim)) and also returns `.pose` — the same attributes from OKS
        keypoint matches — with upstream PoseMetrics' `(B)` / `(P)` keys in `.results_dict`; augment=True warns and
        validates at a single scale.  Segment models raise NotImplementedError."""
        from yolomi.val import run_val
        if data is None:
            raise ValueError("val() needs data: a dataset YAML, a directory with images/ and labels/, or a list")
        if ignored:
            logger.info(f"val: ignoring {sorted(ignored)}")
        return run_val(self.model.engine, data, imgsz=int(imgsz), batch=int(batch), conf=float(conf), iou=float(iou),
                       max_det=int(max_det), augment=bool(augment))

    def __repr__(self) -> str:
        return (f"YOLO11Model(task={self.task}, size={self.size}, "
                f"device={self.device}, optimized={len(self.optimization_history) > 0})")


class YOLO11Factory:
    @staticmethod
    def create_detector(size: str = "n", **kwargs) -> YOLO11Model:
        return YOLO11Model(task="detect", size=size, **kwargs)

    @staticmethod
    def create_segmenter(size: str = "n", **kwargs) -> YOLO11Model:
        return YOLO11Model(task="segment", size=size, **kwargs)

    @staticmethod
    def create_classifier(size: str = "n", **kwargs) -> YOLO11Model:
        return YOLO11Model(task="classify", size=size, **kwargs)

    @staticmethod
    def create_pose_estimator(size: str = "n", **kwargs) -> YOLO11Model:
        return YOLO11Model(task="pose", size=size, **kwargs)

    @staticmethod
    def create_obb_detector(size: str = "n", **kwargs) -> YOLO11Model:
        return YOLO11Model(task="obb", size=size, **kwargs)
