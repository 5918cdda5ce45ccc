"""Engine: one packed YOLO11 model on one GPU, driven through the C-ABI (one graph replay per batch).

PyTorch is plumbing here: it owns the input/output device tensors and the current HIP stream; every arithmetic op
of the forward runs in libyolomi's gfx950 kernels.
"""
from __future__ import annotations

import json
import os
from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .arch import GraphBuilder
from .lib import Runtime
from .plan import QUANT_DTYPES, fuse_default, pack_graph

# Bump when the meaning of a conv config index (csrc/ym_conv.hip kCfgs) changes: stale tables are then ignored.
TUNE_VERSION = 11  # 11: split-pair cfgs encoded kSplitTag + 256·a + b (8 bits per config)
TUNED_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tuned")  # committed tables


def tune_cache_dir() -> str:
    return os.environ.get("YM_TUNE_DIR", os.path.join(os.path.expanduser("~"), ".cache", "yolomi", "tune"))


class Engine:
    def __init__(self, scale: str, task: str, state_dict: Dict[str, np.ndarray], device: torch.device,
                 dtype: str = "f16", blob: Optional[bytes] = None, qparams: Optional[Dict] = None,
                 nc: Optional[int] = 80, receive: Optional[tuple] = None, kpt_shape: Optional[tuple] = None):
        """dtype: 'x3' (split-f16 MFMA, the f16-tolerance plan), 'f16' (throughput), 'f32' (exact parity mode),
        'i8' (PTQ int8) or 'f8' (PTQ fp8 e4m3); the quantized plans need `qparams` from yolomi.quant.calibrate
        (backend 'fp8' for 'f8'), or a packed `blob`.  receive = (rccl comm, root): this rank's context receives the
        root's blob over RCCL (ym_broadcast_weights, a collective the root joins with broadcast_weights())."""
        if device.type != "cuda":
            raise RuntimeError(f"the yolomi engine runs on a gfx950 GPU (got device {device}); there is no CPU path")
        self.scale, self.task, self.dtype = scale, task, dtype
        self.device = device
        self.qparams = qparams
        if task == "pose" and dtype in QUANT_DTYPES:
            raise ValueError(f"pose plans are x3 / f16 / f32: there is no PTQ pose plan (dtype {dtype!r})")
        self.graph = GraphBuilder(scale, task, nc=nc, quant=dtype in QUANT_DTYPES,
                                  fuse=fuse_default(dtype), **(dict(kpt_shape=kpt_shape) if kpt_shape else {}))
        dev_index = device.index if device.index is not None else torch.cuda.current_device()
        if isinstance(receive, Runtime):  # a context that already received the root's blob (yolomi.dist)
            if receive.n_ops != len(self.graph.ops) or receive.device_index != dev_index:
                raise ValueError("the received context does not hold this plan on this device")
            self.blob = None
            self.rt = receive
        elif receive is not None:  # a non-root rank: the model arrives over RCCL from the root's context
            self.blob = None
            self.rt = Runtime(dev_index, None, scale=scale, task=task, dtype=dtype)
            self.rt.broadcast_weights(receive[0], receive[1], self._stream())
        else:
            self.blob = blob if blob is not None else pack_graph(self.graph, state_dict, dtype, qparams)
            self.rt = Runtime(dev_index, self.blob, scale=scale, task=task, dtype=dtype)
        self.nm = self.graph.nm  # extras per device row (segment: mask coefficients; pose: K·ndim padded to 4)
        self.kpt_shape = self.graph.kpt_shape  # pose: (K, ndim); the first nk = K·ndim extras are the keypoints
        self.nk = self.graph.nk if task == "pose" else 0
        self._out: Dict[int, tuple] = {}
        # Per-shape conv tile tables: on the first call of each (B, H, W) a table is taken from the writable tune
        # cache or the committed `tuned/` directory; failing both, ym_tune measures one on this GPU (and caches it).
        # The exact-f32 parity plan is never autotuned: its tiles (and so its fp32 summation orders) stay the fixed
        # heuristic ones, so its results are reproducible from run to run.
        self.autotune = os.environ.get("YM_AUTOTUNE", "1") != "0" and dtype != "f32"
        # Lanes: the batch runs as up to 4 concurrent image slices (parallel branches of one graph); conv tables are
        # per slice batch.  Default from YM_LANES (1).
        self.lanes = int(os.environ.get("YM_LANES", "1"))
        self._tuned = set()
        self._args_cache = {}
        self._tta = None      # run_tta: [self, pass 1's engine, pass 2's engine]
        self._tta_in = {}     # (pass, B, H, W) -> that pass's scaled input
        self._tta_max = None  # (1,) device word: the batch max of the call
        self._embed_tables = {}    # embed: layer tuple -> (ym_embed view table, total channels)
        self._embed_out = {}       # (B, layer tuple) -> the engine-owned (B, sum C) result
        self._embed_scratch = None  # rows / counts a tuning run of an embed-first shape may write
        self._trackers = {}        # track: (B, cfg items, capacity) -> yolomi.lib.Tracker
        self._live_tracker = None  # the key of the tracker the last track() call advanced
        self.tune_source: Dict[tuple, str] = {}
        self.names = {i: f"class{i}" for i in range(nc or 0)}  # annotate's label names (set_names)
        self._annot_tables = None  # annotate: (device font bytes, device name table, nc), uploaded once
        self.contour_launches = 0  # ym_mask_contours calls so far (tests: Masks.xy caches)

    def broadcast_weights(self, comm: int, root: int = 0):
        """The root's side of the RCCL weight broadcast (ym_broadcast_weights): every rank of `comm` calls it or
        constructs its Engine with receive=(comm, root)."""
        self.rt.broadcast_weights(comm, root, self._stream())

    def _stream(self) -> int:
        """The current HIP stream's handle: every launch of a call goes to the stream current when it is made."""
        return torch.cuda.current_stream(self.device).cuda_stream

    def _table_name(self, B, H, W):
        return f"{self.scale}-{self.task}-{self.dtype}-b{B}-{H}x{W}.json"

    def _load_table(self, B, H, W):
        """The committed table first (the one the tests and the bench pin), then this machine's tune cache — so a
        table this machine tuned (ym_tune) for a shape that also has a committed table is cached but not read back
        unless YM_PREFER_CACHE=1 puts the cache first.  A table is used only when its version, op-name list, device
        architecture and conv-config catalogue size (ym_num_conv_cfgs: the id space its entries index) all match."""
        name = self._table_name(B, H, W)
        arch = torch.cuda.get_device_properties(self.device).gcnArchName
        ops = [op.name for op in self.graph.ops]
        order = [("committed", TUNED_DIR), ("cache", tune_cache_dir())]
        if os.environ.get("YM_PREFER_CACHE", "0") == "1":
            order.reverse()
        for tag, d in order:
            p = os.path.join(d, name)
            try:
                t = json.load(open(p))
            except (OSError, ValueError):
                continue
            dev = t.get("device")
            if (t.get("version") == TUNE_VERSION and t.get("ops") == ops and len(t.get("cfg", [])) == self.rt.n_ops
                    and t.get("ncfg") == self._ncfg() and (dev is None or dev.split(":")[0] == arch.split(":")[0])):
                self.rt.set_op_cfg(B, H, W, t["cfg"])
                return f"{tag} table {name}"
        return None

    def _ncfg(self) -> int:
        from yolomi.lib import DTYPE_CODES, load_library
        return load_library().ym_num_conv_cfgs(DTYPE_CODES[self.dtype])

    def _save_table(self, B, H, W):
        cfg = self.rt.get_op_cfg(B, H, W)
        if cfg is None:
            return
        d = tune_cache_dir()
        try:
            os.makedirs(d, exist_ok=True)
            with open(os.path.join(d, self._table_name(B, H, W)), "w") as f:
                json.dump({"version": TUNE_VERSION, "device": torch.cuda.get_device_properties(self.device).gcnArchName,
                           "ncfg": self._ncfg(), "ops": [op.name for op in self.graph.ops], "cfg": cfg}, f)
        except OSError:
            pass  # a read-only home: the table lives for this process only

    def _prepare_shape(self, x, B, H, W, args, dets, counts, stream):
        src = None if os.environ.get("YM_TUNE_TABLES", "1") == "0" else self._load_table(B, H, W)
        if src is None and self.autotune:
            self.rt.tune(x.data_ptr(), B, H, W, args, dets.data_ptr(), counts.data_ptr(), stream)
            self._save_table(B, H, W)
            src = "ym_tune"
        self.tune_source[(B, H, W)] = src or "heuristic"
        self._tuned.add((B, H, W))

    def _ready(self, x, B, H, W, args, stream, dets=None, counts=None):
        """This (B, H, W) has its conv tile table: its first call takes or measures one (_prepare_shape).  x: a batch of
        at least B images (its address is all that is used); dets, counts: the rows and counts a measuring run may
        write (default: outputs(B, args.max_det))."""
        if (B, H, W) not in self._tuned:
            if dets is None:
                dets, counts = self.outputs(B, args.max_det)
            self._prepare_shape(x, B, H, W, args, dets, counts, stream)

    def _check_input(self, x, in_eps, lanes, batch_max):
        """x is a (B, 3, H, W) fp32 contiguous batch on the device; returns (in_eps, lanes, batch_max pointer) with
        the defaults filled in: fp32's eps, the engine's lanes, 0 for no global max."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[1] == 3
        if in_eps is None:
            in_eps = torch.finfo(torch.float32).eps
        bm = 0
        if batch_max is not None:
            assert batch_max.is_cuda and batch_max.dtype == torch.float32 and batch_max.numel() >= 1
            bm = batch_max.data_ptr()
        return in_eps, self.lanes if lanes is None else lanes, bm

    def _cache_args(self, key, args):
        """The ctypes argument block(s) of a repeated call are reused (predict loops pass the same thresholds): callers
        look `_args_cache` up by key and build the block(s) only on a miss; this is the insert, with its eviction."""
        if len(self._args_cache) > 64:
            self._args_cache.clear()
        self._args_cache[key] = args
        return args

    def _target(self, B, max_det, dets_out, counts_after):
        """The (rows, counts) a call's NMS writes: the engine's own, or the caller's dets_out once checked."""
        dets, counts = self.outputs(B, max_det)
        if dets_out is not None:
            assert (dets_out.is_cuda and dets_out.dtype == torch.float32 and dets_out.is_contiguous()
                    and dets_out.dim() == 3 and dets_out.shape[0] >= B and tuple(dets_out.shape[1:]) == tuple(dets.shape[1:]))
            dets = dets_out
        if counts_after:  # room for the B count words behind the rows, in dets_out's own storage
            need = dets_out.storage_offset() * 4 + B * max_det * (6 + self.nm) * 4 + 4 * B if dets_out is not None else -1
            if dets_out is None or dets_out.untyped_storage().nbytes() < need:
                raise ValueError("counts_after needs dets_out from Engine.rows_buffer (rows followed by B int32 words)")
        return dets, counts

    def outputs(self, B: int, max_det: int):
        key = (B, max_det)
        if key not in self._out:
            dets = torch.zeros((B, max_det, 6 + self.nm), dtype=torch.float32, device=self.device)
            counts = torch.zeros((B,), dtype=torch.int32, device=self.device)
            self._out[key] = (dets, counts)
        return self._out[key]

    def rows_buffer(self, B: int, max_det: int, cols: Optional[int] = None):
        """A fresh flat fp32 device buffer for one call: (rows (B, max_det, 6 + nm) view, counts (B,) int32 view of the
        words behind the rows) — for run(..., dets_out=rows, counts_after=True).  cols: another row width (track's)."""
        no = 6 + self.nm if cols is None else cols
        flat = torch.empty((B * max_det * no + B,), dtype=torch.float32, device=self.device)
        return flat[: B * max_det * no].view(B, max_det, no), flat[B * max_det * no:].view(torch.int32)

    def lane_batch(self, B: int, lanes: Optional[int] = None) -> int:
        """Images per lane (the batch every kernel sees) for a B-image call: ceil(B / clamp(lanes, 1, 4, B))."""
        L = max(1, min(self.lanes if lanes is None else lanes, 4, B))
        return -(-B // L)

    def run(self, x: torch.Tensor, conf=0.25, iou=0.7, max_det=300, classes: Optional[Sequence[int]] = None,
            agnostic=False, in_eps=None, use_graph=True, max_nms=30000, max_wh=7680.0, lanes=None,
            batch_max: Optional[torch.Tensor] = None, dets_out: Optional[torch.Tensor] = None,
            counts_after: bool = False, multi_label=False):
        """x: (B,3,H,W) float32 contiguous on this device. Returns the engine-owned (dets, counts) tensors, or
        (dets_out, counts) when the caller hands in its own (>= B, max_det, 6 + nm) fp32 rows (predict(): a fresh
        tensor per call, written by the NMS kernel directly — a cached graph re-points its NMS nodes, no copy).
        batch_max: optional (1,) fp32 device tensor, the max over the GLOBAL batch (yolomi.dist: a batch-sharded
        rank takes LoadTensor's /255 decision from it instead of from its own shard).
        counts_after (with dets_out = the first B*max_det rows of a flat buffer, see rows_buffer): the NMS also writes
        this call's B detection counts as int32 words right behind those rows, so the caller can read them later
        (predict() reads them lazily: no host sync per call).
        multi_label: validation mode — every (anchor, class) pair above conf is an NMS candidate (Ultralytics
        non_max_suppression(multi_label=True)); detect plans."""
        in_eps, lanes, bm = self._check_input(x, in_eps, lanes, batch_max)
        B, _, H, W = x.shape
        akey = (conf, iou, max_det, max_nms, agnostic, max_wh, in_eps, tuple(classes) if classes is not None else None,
                use_graph, lanes, bm, counts_after, multi_label)
        args = self._args_cache.get(akey) or self._cache_args(akey, Runtime.make_args(
            conf, iou, max_det, max_nms, agnostic, max_wh, in_eps, classes, use_graph, lanes, bm, counts_after,
            multi_label))
        dets, counts = self._target(B, max_det, dets_out, counts_after)
        stream = self._stream()
        self._ready(x, self.lane_batch(B, lanes), H, W, args, stream, dets, counts)
        self.rt.infer(x.data_ptr(), B, H, W, args, dets.data_ptr(), counts.data_ptr(), stream)
        return dets, counts

    def track(self, x: torch.Tensor, cfg: Optional[Dict] = None, persist: bool = True, capacity: int = 0, **kw):
        """run() followed by the tracker launch (csrc/ym_track.hip) on the same stream, with no host sync in between:
        image b of the batch is video stream b of a ByteTrack state that lives in device memory.  cfg: the ByteTrack
        parameters (yolomi.track.tracker_config; default bytetrack.yaml's); the engine owns one tracker per (B, cfg,
        capacity).  persist=False resets the tracker first; persist=True continues the live one, and raises ValueError
        when its batch size is not this call's.  A call whose cfg or capacity differs from the live tracker's at the
        same batch size switches to that key's tracker and starts it over, persist=True or not: state is never carried
        from one parameter set to another.  kw: run()'s thresholds (conf, iou, max_det <= 300, classes, agnostic,
        in_eps, batch_max).  Returns (tracks, counts, idx): fresh tensors of this call — tracks (B, max_det, 7 + nm) fp32
        rows [x1, y1, x2, y2, id, conf, cls, extras] in ascending id order, counts the (B,) int32 words behind them
        (rows_buffer's layout, so LazyCounts reads them), idx (B, max_det) int32, the detection row behind each track
        row.  Segment plans raise NotImplementedError (their masks would have to be re-gathered by idx)."""
        from .lib import TRACK_DEFAULTS, TRACK_MAX_DET
        if self.task == "segment":
            raise NotImplementedError("tracking is offered for detect and pose plans; segment masks are not re-gathered")
        full = dict(TRACK_DEFAULTS, **(cfg or {}))
        max_det = int(kw.get("max_det", 300))
        if not 1 <= max_det <= TRACK_MAX_DET:
            raise ValueError(f"track: max_det {max_det} outside 1..{TRACK_MAX_DET}")
        B = x.shape[0]
        key = (B, tuple(sorted(full.items())), int(capacity))
        live = self._live_tracker
        if persist and live is not None and live[0] != B:
            raise ValueError(f"track(persist=True): the live tracker follows {live[0]} streams, this batch has {B} "
                             f"(image b of a batch is stream b); pass persist=False to start over")
        stream = self._stream()
        trk = self._trackers.get(key)
        if trk is None:
            trk = self._trackers[key] = self.rt.track_create(B, full, capacity)
        elif not persist or live != key:
            trk.reset(stream)
        self._live_tracker = key
        dets, cnt = self.rows_buffer(B, max_det)
        self.run(x, dets_out=dets, counts_after=True, **kw)
        tracks, tcnt = self.rows_buffer(B, max_det, 7 + self.nm)
        idx = torch.empty((B, max_det), dtype=torch.int32, device=self.device)
        trk.update(dets.data_ptr(), 6 + self.nm, B, max_det, cnt.data_ptr(), tracks.data_ptr(), idx.data_ptr(),
                   tcnt.data_ptr(), stream)
        return tracks, tcnt, idx

    def tracker_state(self):
        """The live tracker's per-stream (frame_id, next id, activated tracked, lost, unconfirmed, drops), or None;
        synchronous (tests, debugging)."""
        return self._trackers[self._live_tracker].read_state() if self._live_tracker is not None else None

    def _tta_engines(self):
        """The three passes' engines (this one, then two more contexts holding the same packed model: a context has
        one workspace shape, and the passes' shapes must coexist), created on the first augmented call."""
        if self._tta is None:
            if self.task != "detect":
                raise ValueError(f"test-time augmentation is for detect plans (got task {self.task!r})")
            if self.dtype in QUANT_DTYPES:
                raise ValueError(f"test-time augmentation is not supported for the quantized {self.dtype!r} plans "
                                 f"(their activation ranges were calibrated at full scale); use x3, f16 or f32")
            if self.blob is None:
                raise ValueError("test-time augmentation needs the packed model on the host: this engine received its "
                                 "weights over RCCL and kept no blob")
            subs = [Engine(self.scale, self.task, {}, self.device, self.dtype, blob=self.blob, qparams=self.qparams,
                           nc=self.graph.nc) for _ in range(2)]
            for e in subs:
                e.autotune, e.lanes = self.autotune, self.lanes
            self._tta = [self] + subs
        return self._tta

    def run_tta(self, x: torch.Tensor, conf=0.25, iou=0.7, max_det=300, classes: Optional[Sequence[int]] = None,
                agnostic=False, in_eps=None, use_graph=True, max_nms=30000, max_wh=7680.0, lanes=None,
                batch_max: Optional[torch.Tensor] = None, dets_out: Optional[torch.Tensor] = None,
                counts_after: bool = False, multi_label=False):
        """run() with test-time augmentation (Ultralytics augment=True, detect plans): the forward at scales 1, 0.83
        (mirrored) and 0.67, the three decoded heads merged in front of one NMS (csrc/ym_tta.hip).  Arguments and
        return value as run().  Everything is queued on the current stream; after the first call of a shape nothing
        is allocated and no graph is captured."""
        from .tta import pass_shapes
        in_eps, lanes, bm = self._check_input(x, in_eps, lanes, batch_max)
        engines = self._tta_engines()
        B, _, H, W = x.shape
        stream = self._stream()
        if batch_max is None:  # LoadTensor's statistic once: the scaled views and pass 0's forward read the same word
            if self._tta_max is None:
                self._tta_max = torch.empty((1,), dtype=torch.float32, device=self.device)
            bm = self.input_max(x, out=self._tta_max).data_ptr()
        shapes = pass_shapes(H, W)
        xs = [x]
        for p in (1, 2):
            Hs, Ws = shapes[p][:2]
            xp = self._tta_in.get((p, B, H, W))
            if xp is None:
                xp = self._tta_in[(p, B, H, W)] = torch.empty((B, 3, Hs, Ws), dtype=torch.float32, device=self.device)
            self.rt.tta_scale(x.data_ptr(), B, H, W, p, bm, in_eps, xp.data_ptr(), stream)
            xs.append(xp)
        akey = ("tta", conf, iou, max_det, max_nms, agnostic, max_wh, in_eps,
                tuple(classes) if classes is not None else None, use_graph, lanes, bm, counts_after, multi_label)
        args = self._args_cache.get(akey)
        if args is None:
            mk = lambda bmp, ca, ml: Runtime.make_args(conf, iou, max_det, max_nms, agnostic, max_wh, in_eps, classes,
                                                       use_graph, lanes, bmp, ca, ml)
            # pass 0's forward (the caller's values, the given max), the scaled passes' (already normalised), the NMS
            args = self._cache_args(akey, (mk(bm, False, False), mk(0, False, False),
                                           mk(0, counts_after, multi_label)))
        dets, counts = self._target(B, max_det, dets_out, counts_after)
        for p, e in enumerate(engines):
            Hs, Ws = shapes[p][:2]
            Bl = e.lane_batch(B, lanes)
            e._ready(xs[p], Bl, Hs, Ws, args[min(p, 1)], stream)
            e.rt.tta_forward(xs[p].data_ptr(), B, Hs, Ws, args[min(p, 1)], stream)
        Runtime.tta_nms([e.rt for e in engines], B, H, W, args[2], dets.data_ptr(), counts.data_ptr(), stream)
        return dets, counts

    def tta_candidate_counts(self, B: int):
        """candidate_counts() of the last run_tta: merged anchors above conf, or (anchor, class) pairs."""
        return self.rt.tta_counts(B)

    def input_max(self, x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """(1,) fp32 device tensor: max over x (LoadTensor's statistic; asynchronous on the current stream)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
        if out is None:
            out = torch.empty((1,), dtype=torch.float32, device=self.device)
        self.rt.input_max(x.data_ptr(), x.numel(), out.data_ptr(), self._stream())
        return out

    def embed_layers(self):
        """Layer indices (0..22) whose outputs this plan stores, i.e. the ones embed() can pool.  A plan with fused
        conv pairs never writes the first conv's output (x3 / f16: model.1 runs inside model.2.cv1's launch)."""
        return self.graph.embed_layers()

    def _embed_table(self, layers):
        """(view table, total channels) of a normalised layer tuple, built once."""
        t = self._embed_tables.get(layers)
        if t is None:
            if self.dtype in QUANT_DTYPES:
                raise ValueError(f"embeddings are not supported for the quantized {self.dtype!r} plans (their stored "
                                 f"codes need each buffer's scale and zero point); use x3, f16 or f32")
            views = [(v.buf.id, v.coff, v.C) for i in layers for v in self.graph.layer_views(i)]
            t = self._embed_tables[layers] = (Runtime.embed_views(views), sum(v[2] for v in views))
        return t

    def embed(self, x: torch.Tensor, layers=None, out: Optional[torch.Tensor] = None, in_eps=None, use_graph=True,
              batch_max: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Feature embeddings (Ultralytics _predict_once(embed=layers)): the (B, sum C_i) fp32 device tensor of the
        named layers' global-average-pooled outputs, concatenated in ascending layer order (a duplicate counts once;
        default: layer 22, Model.embed's len(model.model) - 2).  The forward stops at the last named layer (no head,
        decode or NMS; the detection buffers of outputs() are not touched) and the pooling kernel (csrc/ym_embed.hip)
        reads the plan's own storage.  x, in_eps, batch_max, use_graph as run().  out: the caller's (>= B, >= sum C_i)
        fp32 rows with unit column stride (default: an engine-owned tensor per (B, layers), overwritten by the next
        call).  Asynchronous on the current stream; in steady state nothing is allocated.
        ValueError: an index outside 0..22, a non-integer, an empty list, a layer this plan does not store, or a
        quantized plan."""
        from .arch import DEFAULT_EMBED, normalize_embed
        in_eps, _, bm = self._check_input(x, in_eps, 1, batch_max)
        layers = normalize_embed(DEFAULT_EMBED if layers is None else layers)
        views, width = self._embed_table(layers)
        B, _, H, W = x.shape
        if out is None:
            out = self._embed_out.get((B, layers))
            if out is None:
                out = self._embed_out[(B, layers)] = torch.empty((B, width), dtype=torch.float32, device=self.device)
        else:
            assert (out.is_cuda and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] >= B
                    and out.shape[1] >= width and out.stride(1) == 1 and out.stride(0) >= width)
        akey = ("embed", in_eps, use_graph, bm)
        args = self._args_cache.get(akey) or self._cache_args(akey, Runtime.make_args(
            in_eps=in_eps, use_graph=use_graph, lanes=1, batch_max_ptr=bm))
        stream = self._stream()
        if (B, H, W) not in self._tuned:  # the conv tile table of the shape, as run() takes it (one lane)
            if self._embed_scratch is None or self._embed_scratch[0].shape[0] < B:
                self._embed_scratch = (torch.zeros((B, args.max_det, 6 + self.nm), dtype=torch.float32,
                                                   device=self.device),
                                       torch.zeros((B,), dtype=torch.int32, device=self.device))
            self._ready(x, B, H, W, args, stream, *self._embed_scratch)  # (outputs()'s buffers are not touched)
        self.rt.embed(x.data_ptr(), B, H, W, args, views, out.data_ptr(), out.stride(0), stream)
        return out[:B, :width]

    def set_names(self, names: Dict[int, str]):
        """The class names annotate() writes into labels (YOLO11Model hands in its own)."""
        self.names = dict(names)
        self._annot_tables = None

    def annotate(self, frames: torch.Tensor, dets: torch.Tensor, counts: torch.Tensor, *, masks=None,
                 mask_offsets=None, mask_geo=None, mask_cap=None, tracked=False, out=None, kpt_shape=None, **switches):
        """Annotated frames of a whole batch (csrc/ym_annot.hip): the (B, H, W, 3) uint8 device tensor of
        `frames` with boxes, labels, masks, keypoints and skeletons drawn in, as Results.plot() draws one image.
        frames: (B, 3, H, W) fp32 (predict's batch: converted like Results.orig_img, no channel flip) or (B, H, W, 3)
        uint8; dets / counts: predict's or track's row buffers as they are, (B, max_det, stride) fp32 and (B,) int32 —
        tracked=True for track's 7-column rows.  masks: (B, cap, mh, mw) uint8 / bool mask slots (instance i of image
        b at masks[b, i]), or packed planes with mask_offsets ((B,) int64 first byte per image) and mask_cap planes per
        image; mask_geo: (B, 4) int32 (uh, uw, top, left), default the identity.  kpt_shape: (K, ndim) of the rows'
        keypoints (default: this engine's, for a pose plan).  switches: line_width (default upstream's rule from H and
        W), kpt_radius, conf, labels, boxes, masks_on (the `masks` switch of plot), kpt_line, color_mode, names (a class-name
        dict other than set_names's, uploaded for this call), clip_kpts (default True: keypoints are clipped to the
        canvas first, as predict()'s Results hold them, so raw rows draw what Results.plot draws; plot passes False).
        Enqueued on the current stream: no tensor value is read on the host and nothing synchronises.  Calls of one
        engine must be stream-ordered (the records of a call live in one scratch buffer of its context); the first call
        of a larger B * max_det grows that buffer with a device synchronisation, so it cannot be captured."""
        from .annotate import annotate_batch
        return annotate_batch(self, frames, dets, counts, masks=masks, mask_offsets=mask_offsets, mask_geo=mask_geo,
                              mask_cap=mask_cap, tracked=tracked, out=out, kpt_shape=kpt_shape, **switches)

    def mask_contours_device(self, masks: torch.Tensor, cap: Optional[int] = None):
        """Instance polygons of n mask planes, left on the device (csrc/ym_contour.hip).  masks: an
        (n, H, W) bool / uint8 tensor on the engine's device whose planes are contiguous (masks.stride(0) >= H * W is
        the plane stride: a slice of mask slots works as it is).  Returns (points, offsets): (cap, 2) int32 (x, y) and
        (n + 1,) int64; plane i's points are points[offsets[i]:offsets[i + 1]].  cap: the capacity in points (default
        max(4096, 64 n)); when offsets[n] exceeds it, the planes that did not fit are unwritten and the call is to
        be repeated with cap = offsets[n] (mask_contours does).  Enqueued on the current stream; nothing is read."""
        if masks.dim() != 3 or masks.dtype not in (torch.uint8, torch.bool) or masks.device != self.device:
            raise ValueError("mask_contours: masks must be an (n, H, W) uint8 / bool tensor on the engine's device")
        n, H, W = masks.shape
        if H < 1 or W < 1:
            raise ValueError(f"mask_contours: planes of {H} x {W}")
        if n and (masks.stride(2) != 1 or masks.stride(1) != W or (n > 1 and masks.stride(0) < H * W)):
            masks = masks.contiguous()
        cap = max(4096, 64 * n) if cap is None else int(cap)
        points = torch.empty((cap, 2), dtype=torch.int32, device=self.device)
        offsets = torch.empty((n + 1,), dtype=torch.int64, device=self.device)
        stream = self._stream()
        self.rt.mask_contours(masks.data_ptr() if n else 0, n, H, W, masks.stride(0) if n > 1 else H * W,
                              points.data_ptr() if cap else 0, cap, offsets.data_ptr(), stream)
        self.contour_launches += 1
        return points, offsets

    def mask_contours(self, masks: torch.Tensor, cap: Optional[int] = None):
        """Instance polygons of n mask planes: a list of n (k_i, 2) int32 numpy arrays of (x, y) pixel coordinates, the
        outer border of each plane's chosen component ((0, 2) for a plane without foreground).  Two device->host reads:
        the offsets, then exactly the points; a first capacity that proves too small costs one more launch."""
        points, offsets = self.mask_contours_device(masks, cap)
        offs = offsets.cpu().numpy()
        total = int(offs[-1])
        if total > points.shape[0]:
            points, offsets = self.mask_contours_device(masks, total)
        pts = points[:total].cpu().numpy() if total else np.zeros((0, 2), dtype=np.int32)
        return [pts[offs[i]:offs[i + 1]] for i in range(len(offs) - 1)]

    def _profile_call(self, x, kw):
        """profile's and profile_replay's common arguments: an eager argument block, the engine's outputs, a table."""
        B, _, H, W = x.shape
        args = Runtime.make_args(use_graph=False, **kw)
        dets, counts = self.outputs(B, args.max_det)
        stream = self._stream()
        self._ready(x, B, H, W, args, stream, dets, counts)
        return x.data_ptr(), B, H, W, args, dets.data_ptr(), counts.data_ptr(), stream

    def profile(self, x: torch.Tensor, **kw):
        return self.rt.profile(*self._profile_call(x, kw))

    def profile_replay(self, x: torch.Tensor, reps=20, **kw):
        """Per-op device ms from graph-captured back-to-back launches (-1 for input/decode/NMS); clobbers buffers."""
        return self.rt.profile_replay(*self._profile_call(x, kw), reps)

    def masks(self, dets: torch.Tensor, counts: Sequence[int], H: int, W: int):
        """Segment plans: instance masks of the last run()'s detections (process_mask, upsample=True).  Returns the
        (total, H, W) uint8 masks, the (total,) int32 non-empty flags and the per-image row offsets (host list)."""
        B = len(counts)
        offs = [0]
        for n in counts:
            offs.append(offs[-1] + int(n))
        total = offs[-1]
        masks = torch.empty((total, H, W), dtype=torch.uint8, device=self.device)
        nonempty = torch.empty((total,), dtype=torch.int32, device=self.device)  # zeroed by ym_masks
        if total:
            off_t = torch.tensor(offs, dtype=torch.int32).to(self.device, non_blocking=True)
            stream = self._stream()
            self.rt.masks(dets.data_ptr(), B, dets.shape[1], off_t.data_ptr(), total, H, W, masks.data_ptr(),
                          nonempty.data_ptr(), stream)
        return masks, nonempty, offs

    def masks_native(self, dets: torch.Tensor, counts: Sequence[int], H: int, W: int, shapes: Sequence[tuple]):
        """Segment plans: native-resolution masks (process_mask_native, retina_masks=True) of the last run()'s (B, H, W)
        forward.  dets: any (>= B, max_det, >= 6 + nm) fp32 device rows whose boxes are already in native pixels
        (scale_boxes) — run()'s own rows, or crafted ones; counts: rows used per image; shapes: each image's native
        (h0, w0).  Returns the packed uint8 masks (image b's counts[b] masks back to back, h0_b * w0_b bytes each), the
        (total,) int32 non-empty flags, the per-image row offsets (B + 1) and byte offsets (B + 1), both host lists."""
        B = len(counts)
        assert len(shapes) == B and dets.is_cuda and dets.dtype == torch.float32 and dets.dim() == 3
        assert dets.shape[0] >= B and dets.shape[2] >= 6 + self.nm and dets.stride(2) == 1
        assert dets.stride(0) == dets.shape[1] * dets.stride(1) and max(counts, default=0) <= dets.shape[1]
        offs, boffs = [0], [0]
        for n, (h0, w0) in zip(counts, shapes):
            offs.append(offs[-1] + int(n))
            boffs.append(boffs[-1] + int(n) * max(int(h0), 0) * max(int(w0), 0))
        total = offs[-1]
        masks = torch.empty((boffs[-1],), dtype=torch.uint8, device=self.device)
        nonempty = torch.empty((total,), dtype=torch.int32, device=self.device)  # zeroed by ym_masks_native
        # one upload: [row offsets (B + 1) | shapes (2B) | pad to an even count] as int32, then the B int64 byte offsets
        n32 = (3 * B + 2) // 2 * 2
        host = np.zeros((n32 + 2 * B,), dtype=np.int32)
        host[: B + 1] = offs
        host[B + 1: 3 * B + 1] = np.asarray([(int(h), int(w)) for h, w in shapes], dtype=np.int32).reshape(-1)
        host[n32:].view(np.int64)[:] = boffs[:B]
        par = torch.from_numpy(host).to(self.device, non_blocking=True)
        stream = self._stream()
        self.rt.masks_native(dets.data_ptr(), dets.stride(1), B, dets.shape[1], par.data_ptr(), total, H, W, shapes,
                             par[B + 1:].data_ptr(), par[n32:].data_ptr(), masks.data_ptr(), nonempty.data_ptr(),
                             stream)
        return masks, nonempty, offs, boffs

    def masks_slots(self, dets: torch.Tensor, counts: torch.Tensor, cap: int, H: int, W: int):
        """Single-sync form of masks(): enqueued behind the forward, reading the DEVICE counts.  Returns the
        (B, cap, H, W) uint8 masks (slot (b, i) = detection i of image b, for i < min(count_b, cap)) and a (B*cap + B)
        int32 tensor: the slots' non-empty flags, then the B counts (read both with one .tolist())."""
        B = counts.shape[0]
        masks = torch.empty((B, cap, H, W), dtype=torch.uint8, device=self.device)
        flags = torch.empty((B * cap + B,), dtype=torch.int32, device=self.device)
        stream = self._stream()
        self.rt.masks_slots(dets.data_ptr(), B, dets.shape[1], counts.data_ptr(), cap, H, W, masks.data_ptr(),
                            flags.data_ptr(), stream)
        return masks, flags

    def read_buffer(self, buf_id: int, B: int, raw: bool = False) -> torch.Tensor:
        """NHWC contents of plan buffer `buf_id` for the first B images (after run/profile), as a CPU float32 tensor
        (int8 plans: the quantized values q = stored byte + 128; fp8 plans: the e4m3 values of the stored codes;
        over the storage channels).  raw=True: the stored elements as they are (int8 / fp16 / fp32 tensor)."""
        _, C, H, W, eb = self.rt.buffer_info(buf_id)
        dt = {1: torch.int8, 2: torch.float16, 4: torch.float32}[eb]
        pair = self.dtype == "x3" and not self.graph.buffers[buf_id].f32
        if pair:  # x3 pair layout: every 8-channel chunk is [fp16 hi x8 | fp16 lo x8]
            dt = torch.float16
        out = torch.empty((B, H, W, 2 * C if pair else C), dtype=dt)
        torch.cuda.synchronize(self.device)
        self.rt.read_buffer(buf_id, out.data_ptr(), out.numel() * out.element_size())
        if pair:
            if raw:
                return out
            hl = out.float().reshape(B, H, W, C // 8, 2, 8)
            return (hl[..., 0, :] + hl[..., 1, :]).reshape(B, H, W, C)
        if raw or eb != 1:
            return out if raw else out.float()
        if self.dtype == "f8":
            return out.view(torch.uint8).view(torch.float8_e4m3fn).float()
        return out.float() + 128.0

    def candidates(self, B: int, H: int, W: int):
        """The last forward's NMS candidates of the first B images (tests): per image the int64 anchor indices, in
        no fixed order (the low 32 bits of a candidate key are ~anchor)."""
        from .arch import num_anchors
        from .lib import SCRATCH_COUNTS, SCRATCH_KEYS
        A = num_anchors(H, W)
        kstride = 1
        while kstride < A:
            kstride <<= 1
        counts = torch.empty((B,), dtype=torch.int32)
        keys = torch.empty((B, kstride), dtype=torch.int64)
        self.rt.read_scratch(SCRATCH_COUNTS, counts.data_ptr(), 4 * B)
        self.rt.read_scratch(SCRATCH_KEYS, keys.data_ptr(), 8 * B * kstride)
        return [0xFFFFFFFF - (keys[b, : min(int(n), A)] & 0xFFFFFFFF) for b, n in enumerate(counts.tolist())]

    def candidate_counts(self, B: int):
        """The last forward's per-image candidate counts (YM_SCRATCH_COUNTS): anchors above conf, or after a
        multi_label run the (anchor, class) pairs above conf, before the max_nms cut."""
        from .lib import SCRATCH_COUNTS
        counts = torch.empty((B,), dtype=torch.int32)
        torch.cuda.synchronize(self.device)
        self.rt.read_scratch(SCRATCH_COUNTS, counts.data_ptr(), 4 * B)
        return counts.tolist()

    def keypoint_rows(self, B: int, H: int, W: int) -> torch.Tensor:
        """Pose plans: the decoded keypoint buffer (B, A, nm) of the last forward as a CPU tensor (tests).  Only the
        candidates' rows (candidates()) were written by that forward."""
        from .arch import num_anchors
        from .lib import SCRATCH_KPTS
        out = torch.empty((B, num_anchors(H, W), self.nm), dtype=torch.float32)
        self.rt.read_scratch(SCRATCH_KPTS, out.data_ptr(), out.numel() * 4)
        return out

    def raw_shapes(self, B: int, H: int, W: int) -> Dict[int, tuple]:
        """(rows, cols) of every op's pre-activation output in a calibration run (ym_calibrate)."""
        shapes = {}
        for i, op in enumerate(self.graph.ops):
            a = op.args
            if op.kind == "conv":
                fo = self.graph.out_factor(op)
                shapes[i] = (B * (H // fo) * (W // fo), 4 * a["c2"] if a["shuffle2x2"] else a["c2"])
            elif op.kind == "dwconv":
                f = a["src"].buf.f
                shapes[i] = (B * (H // f) * (W // f), a["C"])
            elif op.kind == "attn":
                f = a["qkv"].buf.f
                shapes[i] = (B * (H // f) * (W // f), a["C"])
        return shapes

    def calibrate(self, x: torch.Tensor, **kw) -> Dict[int, torch.Tensor]:
        """One eager f32 forward that also returns every conv-like op's pre-activation output (op index → (rows, C)
        fp32 device tensor): the conv-output observers of PTQ calibration (yolomi.quant.calibrate)."""
        assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4
        B, _, H, W = x.shape
        args = Runtime.make_args(use_graph=False, lanes=1, **kw)
        dets, counts = self.outputs(B, args.max_det)
        raws = {i: torch.empty(sh, dtype=torch.float32, device=self.device)
                for i, sh in self.raw_shapes(B, H, W).items()}
        ptrs = [raws[i].data_ptr() if i in raws else 0 for i in range(len(self.graph.ops))]
        stream = self._stream()
        self.rt.calibrate(x.data_ptr(), B, H, W, args, dets.data_ptr(), counts.data_ptr(), ptrs, stream)
        torch.cuda.synchronize(self.device)
        return raws
