"""The host side of YOLO11Model.predict / track / embed against a scripted engine, on CPU tensors (a helper, not a
test): `trace()` runs a case matrix and returns one text block per case — the engine calls the model made (argument
names, scalar values, tensor shapes and dtypes) interleaved with its `.tolist()` reads (on the GPU each is a
device->host sync), `_mask_cap` afterwards, and per Results the path, orig_shape, shapes and SHA-256 of boxes / masks /
keypoints / ids and whether boxes and masks are views of the engine's buffers or gathers.
tests/golden/predict_trace.txt is this module's output, recorded from the model.py the call-path refactor started from
(`python tests/predict_trace.py > tests/golden/predict_trace.txt`); tests/test_predict_host.py compares.

The fake engine fills every buffer from a per-case seed with values on a 1/8 grid, and the scripted native image shapes
give power-of-two letterbox gains, so scale_boxes / scale_coords are exact and the hashes do not depend on the CPU."""
import hashlib
import inspect
import logging
import os
import sys
import types
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "yolo-infer_amd"), ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)

H, W = 32, 64
# native (h0, w0) of the scripted image sources: gains 0.5, 1, 0.25 and pads (16, 0), (0, 8), (16, 0) against 32 x 64
NATIVE = [(64, 64), (16, 64), (128, 128)]
TASKS = {"detect": dict(nm=0, nk=0, kpt_shape=None), "pose": dict(nm=12, nk=9, kpt_shape=(3, 3)),
         "segment": dict(nm=32, nk=0, kpt_shape=None)}


def _fmt(v):
    if isinstance(v, torch.Tensor):
        return f"{str(v.dtype).replace('torch.', '')}{list(v.shape)}"
    if isinstance(v, dict):
        return "{" + ", ".join(f"{k}: {_fmt(x)}" for k, x in sorted(v.items())) + "}"
    if isinstance(v, (list, tuple)):
        return "[" + ", ".join(_fmt(x) for x in v) + "]"
    return repr(v)


def _logged(fn):
    sig = inspect.signature(fn)

    def wrapper(self, *a, **k):
        bound = sig.bind(self, *a, **k)
        args = dict(list(bound.arguments.items())[1:])
        args.update(args.pop("kw", {}))
        self.log.append(f"{fn.__name__}(" + ", ".join(f"{n}={_fmt(v)}" for n, v in args.items()) + ")")
        return fn(self, *a, **k)
    return wrapper


class FakeEngine:
    """Engine's call surface as YOLO11Model uses it.  counts: detections (or tracks) per image; drop: the (image, row)
    pairs whose mask comes back empty."""

    def __init__(self, task, counts, drop=(), seed=0):
        self.task = task
        self.nm, self.nk, self.kpt_shape = (TASKS[task][k] for k in ("nm", "nk", "kpt_shape"))
        self.counts, self.drop = list(counts), set(drop)
        self.gen = torch.Generator().manual_seed(seed)
        self.log = []
        self.rows = self.planes = self._cnt = None

    def _grid(self, *shape, lo=0, hi=8 * W):
        return torch.randint(lo, hi, shape, generator=self.gen).float() / 8

    def _fill(self, rows, first):
        """Boxes inside the 32 x 64 plane, conf, cls, then the extras (pose: x, y, visibility 0.25 / 0.75)."""
        B, M, no = rows.shape
        rows[..., 0:4:2] = self._grid(B, M, 2)
        rows[..., 1:4:2] = self._grid(B, M, 2, hi=8 * H)
        rows[..., 4:first] = self._grid(B, M, first - 4, hi=8)
        if self.task == "pose":
            k = self._grid(B, M, (no - first) // 3, 3, hi=8 * H)
            k[..., 2] = torch.where(k[..., 2] < H / 2, 0.25, 0.75)
            rows[..., first:] = k.reshape(B, M, -1)
        else:
            rows[..., first:] = self._grid(B, M, no - first, lo=-64, hi=64)
        self.rows = rows

    def _flags(self, n):
        return [0 if (b, i) in self.drop else 1 for b in range(len(n)) for i in range(n[b])]

    def _planes(self, *shape):
        self.planes = torch.randint(0, 2, shape, generator=self.gen).to(torch.uint8)
        return self.planes

    @_logged
    def rows_buffer(self, B, max_det):
        no = 6 + self.nm
        flat = torch.empty((B * max_det * no + B,), dtype=torch.float32)
        self._cnt = flat[B * max_det * no:].view(torch.int32)
        return flat[: B * max_det * no].view(B, max_det, no), self._cnt

    def _run(self, x, dets_out, counts_after):
        self._fill(dets_out, 6)
        counts = torch.tensor(self.counts, dtype=torch.int32)
        if counts_after:
            self._cnt.copy_(counts)
        return dets_out, counts

    @_logged
    def run(self, x, conf=0.25, iou=0.7, max_det=300, classes=None, agnostic=False, in_eps=None, batch_max=None,
            dets_out=None, counts_after=False):
        return self._run(x, dets_out, counts_after)

    @_logged
    def run_tta(self, x, conf=0.25, iou=0.7, max_det=300, classes=None, agnostic=False, in_eps=None, batch_max=None,
                dets_out=None, counts_after=False):
        return self._run(x, dets_out, counts_after)

    @_logged
    def track(self, x, cfg=None, persist=True, capacity=0, **kw):
        B, M, no = x.shape[0], kw["max_det"], 7 + self.nm
        flat = torch.empty((B * M * no + B,), dtype=torch.float32)
        tracks, tcnt = flat[: B * M * no].view(B, M, no), flat[B * M * no:].view(torch.int32)
        self._fill(tracks, 7)
        tcnt.copy_(torch.tensor(self.counts, dtype=torch.int32))
        return tracks, tcnt, torch.randint(0, M, (B, M), generator=self.gen).to(torch.int32)

    @_logged
    def masks_slots(self, dets, counts, cap, H, W):
        B = counts.shape[0]
        fl = torch.zeros((B, cap), dtype=torch.int32)
        for b in range(B):
            for i in range(min(self.counts[b], cap)):
                fl[b, i] = (b, i) not in self.drop
        return self._planes(B, cap, H, W), torch.cat([fl.reshape(-1), counts.to(torch.int32)])

    @_logged
    def masks(self, dets, counts, H, W):
        offs = [0]
        for n in counts:
            offs.append(offs[-1] + int(n))
        return self._planes(offs[-1], H, W), torch.tensor(self._flags(counts), dtype=torch.int32), offs

    @_logged
    def masks_native(self, dets, counts, H, W, shapes):
        offs, boffs = [0], [0]
        for n, (h0, w0) in zip(counts, shapes):
            offs.append(offs[-1] + int(n))
            boffs.append(boffs[-1] + int(n) * h0 * w0)
        return self._planes(boffs[-1]), torch.tensor(self._flags(counts), dtype=torch.int32), offs, boffs

    @_logged
    def _embed_table(self, layers):
        return None, 8 * len(layers)

    @_logged
    def embed(self, x, layers=None, in_eps=None, batch_max=None):
        return self._grid(x.shape[0], 8 * len(layers))


def _case(name, task, fn="predict", image=False, counts=(2, 1), drop=(), cap=64, budget=None, bm=False, **kw):
    kw.setdefault("max_det", 5)
    return dict(name=name, task=task, fn=fn, image=image, counts=list(counts), drop=drop, cap=cap, budget=budget,
                bm=bm, kw=kw)


def cases():
    c = []
    for task in ("detect", "pose"):
        c += [_case(f"{task}-tensor-async", task, counts=(3, 0)),
              _case(f"{task}-tensor-sync-zero", task, counts=(0, 0), sync=True),
              _case(f"{task}-tensor-kwargs-globalmax", task, counts=(5, 1, 2), bm=True, conf=0.5, iou=0.6,
                    classes=[0, 2], agnostic_nms=True, retina_masks=True, imgsz=320),
              _case(f"{task}-image", task, image=True, counts=(2, 0, 5), bm=True, conf=0.3),
              _case(f"{task}-image-zero", task, image=True, counts=(0, 0)),
              _case(f"{task}-tensor-augment", task, counts=(3, 2), augment=True),
              _case(f"{task}-image-augment", task, image=True, counts=(1, 4), augment=True, sync=True),
              _case(f"{task}-track-tensor", task, fn="track", counts=(3, 0)),
              _case(f"{task}-track-tensor-persist-sync", task, fn="track", counts=(0, 0, 0), persist=True, sync=True,
                    bm=True, conf=0.2, iou=0.5, classes=[1], agnostic_nms=True, augment=True),
              _case(f"{task}-track-image", task, fn="track", image=True, counts=(2, 0, 4),
                    tracker={"match_thresh": 0.7}),
              _case(f"{task}-track-image-persist", task, fn="track", image=True, counts=(5, 5), persist=True, bm=True),
              _case(f"{task}-embed-tensor", task, embed=[22, 10], bm=True, augment=True),
              _case(f"{task}-embed-image", task, fn="embed", image=True, bm=True)]
    seg = lambda name, **k: c.append(_case(f"segment-{name}", "segment", **dict(dict(max_det=8), **k)))
    for image in (False, True):
        s = "image" if image else "tensor"
        seg(f"{s}-slots-views", image=image, counts=(5, 4))
        seg(f"{s}-slots-one-zero", image=image, counts=(8, 0), sync=True)
        seg(f"{s}-slots-drop", image=image, counts=(5, 4, 7), drop=((0, 1), (2, 6), (2, 0)))
        seg(f"{s}-zero", image=image, counts=(0, 0))
        seg(f"{s}-compact", image=image, counts=(2, 1, 0), bm=True)
        seg(f"{s}-compact-drop", image=image, counts=(2, 1), drop=((0, 0),))
        seg(f"{s}-above-cap", image=image, counts=(6, 3), cap=4)
        seg(f"{s}-above-cap-drop", image=image, counts=(30, 2), cap=16, max_det=40, drop=((0, 29), (1, 0), (1, 1)))
        seg(f"{s}-cap-follows-down", image=image, counts=(20, 17), cap=64, max_det=40)
        seg(f"{s}-budget-0", image=image, counts=(5, 4), budget="0", drop=((1, 2),))
        seg(f"{s}-augment", image=image, counts=(5, 4), augment=True)
        seg(f"{s}-retina", image=image, counts=(5, 4), retina_masks=True, conf=0.4, iou=0.5, classes=[3],
            agnostic_nms=True)
        seg(f"{s}-retina-drop", image=image, counts=(3, 0, 2), retina_masks=True, drop=((0, 0), (2, 1)), bm=True)
        seg(f"{s}-retina-zero", image=image, counts=(0, 0), retina_masks=True, augment=True)
        seg(f"{s}-track", image=image, fn="track")
        seg(f"{s}-embed", image=image, embed=[4])
    return c


def _sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.detach().numpy()).tobytes()).hexdigest()[:16]


def _same(t, buf):
    return buf is not None and t.untyped_storage().data_ptr() == buf.untyped_storage().data_ptr()


def _describe(r, eng, lines):
    if isinstance(r, torch.Tensor):
        lines.append(f"  embedding {_fmt(r)} {_sha(r)}")
        return
    lines.append(f"  {r.path} orig_shape={r.orig_shape} speed={sorted(r.speed)} mask_geo={r._mask_geo}")
    bx = r.boxes.data
    lines.append(f"    boxes {_fmt(bx)} {_sha(bx)} {'view' if _same(bx, eng.rows) else 'gather'}")
    if r.boxes.id is not None:
        lines.append(f"    id {_fmt(r.boxes.id)} {_sha(r.boxes.id)}")
    if r.det_idx is not None:
        lines.append(f"    det_idx {_fmt(r.det_idx)} {_sha(r.det_idx)}")
    if r.masks is not None:
        mk = r.masks.data
        lines.append(f"    masks {_fmt(mk)} {_sha(mk)} {'view' if _same(mk, eng.planes) else 'gather'} "
                     f"orig_shape={r.masks.orig_shape}")
    if r.keypoints is not None:
        lines.append(f"    keypoints {_fmt(r.keypoints.data)} {_sha(r.keypoints.data)}")


def run_case(case):
    from core.model import YOLO11Model, logger
    seed = zlib.crc32(case["name"].encode())
    B = len(case["counts"])
    eng = FakeEngine(case["task"], case["counts"], case["drop"], seed)
    m = object.__new__(YOLO11Model)
    m.task, m._dev, m._mask_cap = case["task"], torch.device("cpu"), case["cap"]
    m.model = types.SimpleNamespace(engine=eng, names={i: f"class{i}" for i in range(4)})
    m.global_batch_max = None
    if case["bm"]:
        def global_max(x):
            eng.log.append(f"global_batch_max(x={_fmt(x)})")
            return torch.ones(1)
        m.global_batch_max = global_max
    x = torch.rand((B, 3, H, W), generator=torch.Generator().manual_seed(seed))
    source = x
    if case["image"]:
        shapes = NATIVE[:B]
        imgs = [np.full((h, w, 3), b, dtype=np.uint8) for b, (h, w) in enumerate(shapes)]
        geo = [(int(h * min(H / h, W / w)), int(w * min(H / h, W / w)), (H - int(h * min(H / h, W / w))) // 2,
                (W - int(w * min(H / h, W / w))) // 2) for h, w in shapes]
        source = imgs

        def as_batch(src, imgsz=640):
            eng.log.append(f"_as_batch(imgsz={imgsz})")
            return x, torch.finfo(torch.float32).eps, (imgs, [f"frame{b}.png" for b in range(B)], shapes, geo)
        m._as_batch = as_batch
    warned = []
    handler = logging.Handler(level=logging.WARNING)
    handler.emit = lambda rec: warned.append(rec.getMessage())
    logger.addHandler(handler)
    stream, env, tolist = torch.cuda.current_stream, os.environ.get("YM_MASK_BUDGET_MB"), torch.Tensor.tolist
    torch.cuda.current_stream = lambda device=None: None

    def host_read(t):  # on the GPU every .tolist() is a device->host read (a sync): their number and order are pinned
        eng.log.append(f"tolist({_fmt(t)})")
        return tolist(t)
    torch.Tensor.tolist = host_read
    if case["budget"] is not None:
        os.environ["YM_MASK_BUDGET_MB"] = case["budget"]
    lines = [f"case {case['name']}: {case['fn']}({', '.join(f'{k}={v!r}' for k, v in case['kw'].items())})"]
    try:
        res = getattr(m, case["fn"])(source, **case["kw"])
    except Exception as e:
        res = []
        lines.append(f"  raised {type(e).__name__}: {e}")
    finally:
        torch.cuda.current_stream, torch.Tensor.tolist = stream, tolist
        logger.removeHandler(handler)
        os.environ.pop("YM_MASK_BUDGET_MB", None)
        if env is not None:
            os.environ["YM_MASK_BUDGET_MB"] = env
    lines += [f"  warning: {w}" for w in warned]
    lines += [f"  call {c}" for c in eng.log]
    lines.append(f"  _mask_cap {m._mask_cap}")
    for r in res:
        _describe(r, eng, lines)
    return lines


def trace() -> str:
    return "".join(l + "\n" for case in cases() for l in run_case(case))


if __name__ == "__main__":
    sys.stdout.write(trace())
