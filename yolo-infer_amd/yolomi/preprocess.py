"""Image sources for predict(): decoding, Ultralytics LetterBox geometry, and the GPU letterbox.

Ultralytics 8.3.x `BasePredictor.pre_transform` letterboxes a list of HWC BGR uint8 images (cv2.imread order) with
`LetterBox(imgsz, auto=same_shapes, stride=32)` (auto: the canvas shrinks to the stride multiple when every image
has the same shape, else every image goes to imgsz x imgsz), stacks them, flips BGR→RGB, moves to the device and
divides by 255.  Here the geometry is computed on the host (`letterbox_geometry`, the same arithmetic as
`LetterBox.__call__`), each image is copied to the device once, and `ym_letterbox` (csrc/ym_letterbox.hip) writes
its slot of the fp32 NCHW batch.  Detections are mapped back with `scale_boxes` (upstream `ops.scale_boxes`).
Frames that are on the device already (uint8 HWC tensors) skip the copy: `letterbox_frames` writes the whole batch
with one `ym_letterbox_batch` launch (csrc/ym_letterbox_batch.hip), the same bits.  Decoder surfaces (NV12: a Y plane
and an interleaved UV plane) go in as `NV12Frames`: `letterbox_nv12` converts and letterboxes them with one
`ym_letterbox_nv12` launch (csrc/ym_letterbox_nv12.hip).
Classify models take upstream's `classify_transforms` instead: `classify_batch` (Pillow, on the host: the reference)
and `classify_batch_gpu` (`ym_classify_pre`, csrc/ym_cls_pre.hip: one copy and one launch per batch, the same bits).
Reference call sites: /root/reference/demos/detection_demo.py:87-93, 190-196 (path / ndarray sources).
"""
from __future__ import annotations

import os
from typing import List, Sequence, Tuple

import numpy as np
import torch

IMG_SUFFIXES = {".bmp", ".dng", ".jpeg", ".jpg", ".mpo", ".png", ".tif", ".tiff", ".webp", ".pfm", ".heic"}


def letterbox_geometry(h: int, w: int, new_shape=(640, 640), auto=True, stride=32, scaleup=True) -> Tuple:
    """LetterBox.__call__: (unpad_h, unpad_w, top, bottom, left, right) for an h x w image."""
    r = min(new_shape[0] / h, new_shape[1] / w)
    if not scaleup:
        r = min(r, 1.0)
    uw, uh = int(round(w * r)), int(round(h * r))
    dw, dh = new_shape[1] - uw, new_shape[0] - uh
    if auto:
        dw, dh = dw % stride, dh % stride
    dw, dh = dw / 2, dh / 2
    return uh, uw, int(round(dh - 0.1)), int(round(dh + 0.1)), int(round(dw - 0.1)), int(round(dw + 0.1))


def load_image(path: str) -> np.ndarray:
    """HWC uint8 BGR array of an image file (cv2.imread order; decoded with Pillow, which this image ships)."""
    from PIL import Image
    with Image.open(path) as im:
        rgb = np.asarray(im.convert("RGB"))
    return np.ascontiguousarray(rgb[..., ::-1])


def expand_sources(source) -> Tuple[List[np.ndarray], List[str]]:
    """predict() sources other than tensors → (list of HWC uint8 BGR arrays, list of paths)."""
    items = list(source) if isinstance(source, (list, tuple)) else [source]
    imgs, paths = [], []
    for i, s in enumerate(items):
        if isinstance(s, (str, os.PathLike)):
            p = os.fspath(s)
            if os.path.isdir(p):
                files = sorted(f for f in os.listdir(p) if os.path.splitext(f)[1].lower() in IMG_SUFFIXES)
                for f in files:
                    imgs.append(load_image(os.path.join(p, f)))
                    paths.append(os.path.join(p, f))
                continue
            if not os.path.exists(p):
                raise FileNotFoundError(f"{p} does not exist")
            imgs.append(load_image(p))
            paths.append(p)
        elif isinstance(s, np.ndarray):
            if s.ndim == 2:
                s = np.repeat(s[..., None], 3, axis=2)
            if s.ndim != 3 or s.shape[2] != 3 or s.dtype != np.uint8:
                raise ValueError(f"ndarray sources must be HWC uint8 with 3 channels (BGR), got {s.shape} {s.dtype}")
            imgs.append(np.ascontiguousarray(s))
            paths.append(f"image{i}.jpg")
        elif hasattr(s, "convert") and hasattr(s, "size"):  # PIL.Image
            rgb = np.asarray(s.convert("RGB"))
            imgs.append(np.ascontiguousarray(rgb[..., ::-1]))
            paths.append(getattr(s, "filename", "") or f"image{i}.jpg")
        else:
            raise TypeError(f"unsupported source type {type(s).__name__}")
    if not imgs:
        raise FileNotFoundError("no images found in source")
    return imgs, paths


def batch_geometry(imgs: Sequence[np.ndarray], imgsz: int = 640, stride: int = 32) -> List[Tuple]:
    """letterbox_geometry of every image of a predict() batch (auto only when all images share one shape)."""
    same = len({im.shape for im in imgs}) == 1
    return [letterbox_geometry(im.shape[0], im.shape[1], (imgsz, imgsz), auto=same, stride=stride) for im in imgs]


def letterbox_batch(rt, imgs: Sequence[np.ndarray], device: torch.device, imgsz: int = 640, stride: int = 32,
                    stream: int = 0, geo: Sequence[Tuple] = None) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
    """The predictor's preprocessed batch (B, 3, Hn, Wn) fp32 on `device`, built on the GPU.  geo: the images'
    batch_geometry when the caller already has it (predict keeps it for the masks' window), else computed here."""
    if geo is None:
        geo = batch_geometry(imgs, imgsz, stride)
    uh, uw, t, b, l, r = geo[0]
    Hn, Wn = uh + t + b, uw + l + r
    out = torch.empty((len(imgs), 3, Hn, Wn), dtype=torch.float32, device=device)
    srcs = [torch.from_numpy(im).to(device, non_blocking=False) for im in imgs]
    for i, (im, g) in enumerate(zip(srcs, geo)):
        h, w = im.shape[:2]
        rt.letterbox(im.data_ptr(), h, w, im.stride(0), True, g[0], g[1], g[2], g[4], out[i].data_ptr(), Hn, Wn,
                     stream)
    return out, [im.shape[:2] for im in imgs]


# ym_letterbox_desc (include/yolomi.h): one frame of a ym_letterbox_batch launch
LB_DESC = np.dtype([("src", "<u8"), ("h", "<i4"), ("w", "<i4"), ("row_bytes", "<i4"), ("bgr", "<i4"), ("uh", "<i4"),
                    ("uw", "<i4"), ("top", "<i4"), ("left", "<i4"), ("scale_x", "<f8"), ("scale_y", "<f8")])


def is_frame_source(source) -> bool:
    """A predict() source of device frames: a (B, H, W, 3) uint8 tensor or a list of (H, W, 3) uint8 tensors."""
    if isinstance(source, torch.Tensor):
        return source.dtype == torch.uint8 and source.dim() == 4 and source.shape[3] == 3
    return (isinstance(source, (list, tuple)) and len(source) > 0 and all(
        isinstance(s, torch.Tensor) and s.dtype == torch.uint8 and s.dim() == 3 and s.shape[2] == 3 for s in source))


def frames_desc(frames: Sequence[torch.Tensor], geo: Sequence[Tuple], bgr: bool = True) -> np.ndarray:
    """The LB_DESC table of (H, W, 3) uint8 frames with their batch_geometry: each frame's address and row stride as
    they are (no copy), the scales in double as ym_letterbox forms them."""
    desc = np.zeros(len(frames), dtype=LB_DESC)
    for i, (f, g) in enumerate(zip(frames, geo)):
        if f.dtype != torch.uint8 or f.dim() != 3 or f.shape[2] != 3 or f.shape[0] < 1 or f.shape[1] < 1:
            raise TypeError(f"frame {i}: expected a non-empty (H, W, 3) uint8 tensor, got {tuple(f.shape)} {f.dtype}")
        if f.stride(2) != 1 or f.stride(1) != 3 or f.stride(0) < 3 * f.shape[1]:
            raise ValueError(f"frame {i}: strides {tuple(f.stride())} are not interleaved HWC rows (channel stride 1, "
                             f"pixel stride 3, row stride >= 3 * W); make the frame contiguous")
        h, w = int(f.shape[0]), int(f.shape[1])
        desc[i] = (f.data_ptr(), h, w, f.stride(0), int(bool(bgr)), g[0], g[1], g[2], g[4], 1.0 / (g[1] / w),
                   1.0 / (g[0] / h))
    return desc


def letterbox_frames(rt, frames, device: torch.device, imgsz: int = 640, stride: int = 32, stream: int = 0,
                     bgr: bool = True, geo: Sequence[Tuple] = None) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
    """letterbox_batch for frames that already live on `device`: a (B, H, W, 3) uint8 tensor or a list of (H, W, 3)
    uint8 tensors (any row stride; slices of wider tensors as they are).  The geometry is batch_geometry's; one small
    descriptor table goes up through pinned memory and ONE ym_letterbox_batch launch (csrc/ym_letterbox_batch.hip)
    writes the (B, 3, Hn, Wn) fp32 batch — no host sync, no copy of a pixel, the same bits as letterbox_batch.  The
    table is copied on the current stream of `device`, which `stream` should be."""
    device = torch.device(device)
    frames = list(frames.unbind(0)) if isinstance(frames, torch.Tensor) and frames.dim() == 4 else list(frames)
    if not frames:
        raise ValueError("letterbox_frames: no frames")
    for i, f in enumerate(frames):
        if not isinstance(f, torch.Tensor):
            raise TypeError(f"frame {i}: expected a torch.Tensor, got {type(f).__name__}")
        if f.device != device:
            raise ValueError(f"frame {i} is on {f.device}: frames must be on the model's device ({device}); pass "
                             f"host images as ndarrays")
    if geo is None:
        geo = batch_geometry(frames, imgsz, stride)
    desc = frames_desc(frames, geo, bgr)
    uh, uw, t, b, l, r = geo[0]
    Hn, Wn = uh + t + b, uw + l + r
    host = torch.empty(desc.nbytes, dtype=torch.uint8, pin_memory=device.type == "cuda")
    host.numpy()[:] = desc.view(np.uint8)
    dtab = host.to(device, non_blocking=True)  # (the pinned block is recycled only once this copy has run)
    out = torch.empty((len(frames), 3, Hn, Wn), dtype=torch.float32, device=device)
    rt.letterbox_batch(dtab.data_ptr(), desc.ctypes.data, len(frames), out.data_ptr(), Hn, Wn, stream)
    return out, [tuple(f.shape[:2]) for f in frames]


# ym_nv12_desc (include/yolomi.h): one frame of a ym_letterbox_nv12 launch
NV12_DESC = np.dtype([("y", "<u8"), ("uv", "<u8"), ("h", "<i4"), ("w", "<i4"), ("y_pitch", "<i4"), ("uv_pitch", "<i4"),
                      ("uh", "<i4"), ("uw", "<i4"), ("top", "<i4"), ("left", "<i4"), ("scale_x", "<f8"),
                      ("scale_y", "<f8")])
# (standard, full_range) -> (y_off, cy, cub, cug, cvg, cvr), the decimals the fixed-point integers are rounded from
NV12_STANDARDS = {("bt601", False): (16, 1.164, 2.018, -0.391, -0.813, 1.596),
                  ("bt709", False): (16, 1.164, 2.112, -0.213, -0.533, 1.793),
                  ("bt601", True): (0, 1.0, 1.772, -0.344, -0.714, 1.402),
                  ("bt709", True): (0, 1.0, 1.8556, -0.1873, -0.4681, 1.5748)}


def nv12_coefficients(standard: str = "bt601", full_range: bool = False) -> Tuple[int, ...]:
    """(y_off, CY, CUB, CUG, CVG, CVR) of ym_letterbox_nv12 / ym_nv12_to_bgr: each coefficient round(c * 2**20).  BT.601
    limited range gives OpenCV's own COLOR_YUV2BGR_NV12 integers."""
    key = (str(standard).lower(), bool(full_range))
    if key not in NV12_STANDARDS:
        raise ValueError(f"unknown NV12 standard {standard!r}: 'bt601' or 'bt709'")
    y_off, *c = NV12_STANDARDS[key]
    return (y_off,) + tuple(int(round(v * (1 << 20))) for v in c)


class NV12Frames:
    """A predict() / track() / embed() source of decoded video as hardware decoders hand it out: per frame a (H, W) uint8
    luma plane and a (H/2, W/2, 2) uint8 plane of interleaved U, V, on the model's device.  y: a (B, H, W) tensor or a
    list of (H, W) ones; uv: a (B, H/2, W/2, 2) tensor or a list of (H/2, W/2, 2) ones.  Any row stride is taken (pitched
    surfaces as they are, no copy); an element stride other than 1 in y or other than (2, 1) in uv is refused, as are odd
    sizes.  standard / full_range choose the conversion integers (nv12_coefficients)."""

    def __init__(self, y, uv, standard: str = "bt601", full_range: bool = False):
        self.coef = nv12_coefficients(standard, full_range)
        self.standard, self.full_range = str(standard).lower(), bool(full_range)
        for name, p, nd in (("y", y, 3), ("uv", uv, 4)):
            if isinstance(p, torch.Tensor) and p.dim() != nd:
                raise TypeError(f"NV12Frames: {name} must be a ({'B, H, W' if nd == 3 else 'B, H/2, W/2, 2'}) tensor or a "
                                f"list of planes, got shape {tuple(p.shape)}")
            if not isinstance(p, (torch.Tensor, list, tuple)):
                raise TypeError(f"NV12Frames: {name} must be a tensor or a list of tensors, got {type(p).__name__}")
        self.y = list(y.unbind(0)) if isinstance(y, torch.Tensor) else list(y)
        self.uv = list(uv.unbind(0)) if isinstance(uv, torch.Tensor) else list(uv)
        if not self.y or len(self.y) != len(self.uv):
            raise ValueError(f"NV12Frames: {len(self.y)} y planes and {len(self.uv)} uv planes (at least one of each, as "
                             f"many of one as of the other)")
        for i, (p, c) in enumerate(zip(self.y, self.uv)):
            for name, t, nd in (("y", p, 2), ("uv", c, 3)):
                if not isinstance(t, torch.Tensor):
                    raise TypeError(f"frame {i}: {name} is a {type(t).__name__}, not a torch.Tensor")
                if t.dtype != torch.uint8 or t.dim() != nd or (nd == 3 and t.shape[2] != 2):
                    raise TypeError(f"frame {i}: {name} must be a uint8 {'(H, W)' if nd == 2 else '(H/2, W/2, 2)'} plane, "
                                    f"got {tuple(t.shape)} {t.dtype}")
            h, w = int(p.shape[0]), int(p.shape[1])
            if h < 2 or w < 2 or h % 2 or w % 2:
                raise ValueError(f"frame {i}: NV12 sizes are even and at least 2, got {h} x {w}")
            if tuple(c.shape) != (h // 2, w // 2, 2):
                raise ValueError(f"frame {i}: uv plane {tuple(c.shape)} does not belong to a {h} x {w} y plane (expected "
                                 f"{(h // 2, w // 2, 2)})")
            if c.device != p.device:
                raise ValueError(f"frame {i}: y is on {p.device}, uv on {c.device}")
            if p.stride(1) != 1 or p.stride(0) < w:
                raise ValueError(f"frame {i}: y strides {tuple(p.stride())} are not rows of bytes (element stride 1, row "
                                 f"stride >= W)")
            if c.stride(2) != 1 or c.stride(1) != 2 or c.stride(0) < w:
                raise ValueError(f"frame {i}: uv strides {tuple(c.stride())} are not rows of interleaved U, V bytes "
                                 f"(strides (>= W, 2, 1))")

    @classmethod
    def from_surface(cls, t: torch.Tensor, standard: str = "bt601", full_range: bool = False) -> "NV12Frames":
        """The usual decoder surface, (3H/2, W) uint8 or a (B, 3H/2, W) batch of them — H rows of Y, then H/2 rows of
        interleaved U, V at the same pitch — split into views, with no copy."""
        if not isinstance(t, torch.Tensor) or t.dtype != torch.uint8 or t.dim() not in (2, 3):
            raise TypeError("NV12Frames.from_surface: expected a (3H/2, W) or (B, 3H/2, W) uint8 tensor")
        t = t.unsqueeze(0) if t.dim() == 2 else t
        rows, w = int(t.shape[1]), int(t.shape[2])
        if rows < 3 or rows % 3 or w < 2 or w % 2 or t.stride(2) != 1:
            raise ValueError(f"NV12Frames.from_surface: {rows} x {w} is no 3H/2 x W surface of even H and W with "
                             f"element stride 1")
        h = rows // 3 * 2
        return cls(t[:, :h], t[:, h:].unflatten(2, (w // 2, 2)), standard, full_range)

    def __len__(self):
        return len(self.y)

    def clone(self) -> "NV12Frames":
        """The same frames in memory of their own (decoders reuse their surfaces)."""
        r = object.__new__(NV12Frames)
        r.coef, r.standard, r.full_range = self.coef, self.standard, self.full_range
        r.y, r.uv = [p.clone() for p in self.y], [c.clone() for c in self.uv]
        return r

    def image(self, rt, i: int) -> "NV12Image":
        return NV12Image(rt, self.y[i], self.uv[i], self.coef)


class NV12Image:
    """One NV12 frame standing where an image source's HWC BGR ndarray stands (Results.orig_img): it has the image's
    `shape`, and `to_bgr()` converts it with ym_nv12_to_bgr (csrc/ym_letterbox_nv12.hip) and moves it to the host."""

    def __init__(self, rt, y: torch.Tensor, uv: torch.Tensor, coef):
        self.rt, self.y, self.uv, self.coef = rt, y, uv, coef
        self.shape = (int(y.shape[0]), int(y.shape[1]), 3)

    def to_bgr_device(self, stream: int = None) -> torch.Tensor:
        h, w, _ = self.shape
        out = torch.empty(self.shape, dtype=torch.uint8, device=self.y.device)
        if stream is None:
            stream = torch.cuda.current_stream(self.y.device).cuda_stream
        self.rt.nv12_to_bgr(self.y.data_ptr(), self.uv.data_ptr(), h, w, self.y.stride(0), self.uv.stride(0), self.coef,
                            out.data_ptr(), 3 * w, stream)
        return out

    def to_bgr(self) -> np.ndarray:
        return self.to_bgr_device().cpu().numpy()


def nv12_desc(frames: NV12Frames, geo: Sequence[Tuple]) -> np.ndarray:
    """The NV12_DESC table of the frames with their batch_geometry: plane addresses and pitches as they are."""
    desc = np.zeros(len(frames), dtype=NV12_DESC)
    for i, (p, c, g) in enumerate(zip(frames.y, frames.uv, geo)):
        h, w = int(p.shape[0]), int(p.shape[1])
        desc[i] = (p.data_ptr(), c.data_ptr(), h, w, p.stride(0), c.stride(0), g[0], g[1], g[2], g[4],
                   1.0 / (g[1] / w), 1.0 / (g[0] / h))
    return desc


def letterbox_nv12(rt, frames: NV12Frames, device: torch.device, imgsz: int = 640, stride: int = 32, stream: int = 0,
                   geo: Sequence[Tuple] = None) -> Tuple[torch.Tensor, List[Tuple[int, int]]]:
    """letterbox_frames for NV12Frames: the geometry is batch_geometry's of the luma planes, the descriptor table goes up
    through pinned memory and ONE ym_letterbox_nv12 launch (csrc/ym_letterbox_nv12.hip) converts the taps the resize
    uses and writes the (B, 3, Hn, Wn) fp32 batch — no host sync, no converted frame, the bits of letterbox_frames on the
    frames converted to BGR by the integer rule of include/yolomi.h."""
    device = torch.device(device)
    if not isinstance(frames, NV12Frames):
        raise TypeError(f"letterbox_nv12: expected NV12Frames, got {type(frames).__name__}")
    for i, p in enumerate(frames.y):
        if p.device != device:
            raise ValueError(f"frame {i} is on {p.device}: frames must be on the model's device ({device})")
    if geo is None:
        geo = batch_geometry(frames.y, imgsz, stride)
    desc = nv12_desc(frames, geo)
    uh, uw, t, b, l, r = geo[0]
    Hn, Wn = uh + t + b, uw + l + r
    host = torch.empty(desc.nbytes, dtype=torch.uint8, pin_memory=device.type == "cuda")
    host.numpy()[:] = desc.view(np.uint8)
    dtab = host.to(device, non_blocking=True)  # (the pinned block is recycled only once this copy has run)
    out = torch.empty((len(frames), 3, Hn, Wn), dtype=torch.float32, device=device)
    rt.letterbox_nv12(dtab.data_ptr(), desc.ctypes.data, len(frames), frames.coef, out.data_ptr(), Hn, Wn, stream)
    return out, [tuple(p.shape) for p in frames.y]


def classify_geometry(h: int, w: int, imgsz: int = 224) -> Tuple[int, int, int, int]:
    """Upstream classify_transforms' geometry for an h x w image: (rh, rw, top, left) — torchvision Resize(imgsz) puts
    the shorter side at imgsz and the longer at int(imgsz * long / short); CenterCrop(imgsz) then starts at
    int(round((rh - imgsz) / 2.0)) and likewise for the columns."""
    if h <= w:
        rh, rw = imgsz, int(imgsz * w / h)
    else:
        rh, rw = int(imgsz * h / w), imgsz
    return rh, rw, int(round((rh - imgsz) / 2.0)), int(round((rw - imgsz) / 2.0))


def classify_batch(imgs: Sequence[np.ndarray], imgsz: int = 224) -> torch.Tensor:
    """Upstream classify_transforms on the host, with Pillow as upstream itself uses there: every HWC uint8 BGR image
    to RGB, Resize(imgsz) with Image.BILINEAR, CenterCrop(imgsz), ToTensor (/255), Normalize(mean 0, std 1: the
    identity).  Returns the (B, 3, imgsz, imgsz) fp32 CPU batch; imgsz must be a multiple of 32, as the plan's strides
    ask."""
    from PIL import Image
    if imgsz < 32 or imgsz % 32:
        raise ValueError(f"classify: imgsz {imgsz} must be a positive multiple of 32")
    out = np.empty((len(imgs), 3, imgsz, imgsz), dtype=np.float32)
    for i, im in enumerate(imgs):
        rh, rw, top, left = classify_geometry(im.shape[0], im.shape[1], imgsz)
        pil = Image.fromarray(np.ascontiguousarray(im[..., ::-1])).resize((rw, rh), Image.BILINEAR)
        rgb = np.asarray(pil.crop((left, top, left + imgsz, top + imgsz)), dtype=np.uint8)
        out[i] = rgb.transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    return torch.from_numpy(out)


# ym_cls_pre_desc (include/yolomi.h): one image of a ym_classify_pre batch
CLS_DESC = np.dtype([("off", "<i8"), ("h", "<i4"), ("w", "<i4"), ("row_bytes", "<i4"), ("bgr", "<i4"), ("rh", "<i4"),
                     ("rw", "<i4"), ("top", "<i4"), ("left", "<i4")])
CLS_PRE_MAX_SCALE = 64  # csrc/ym_common.h kClsPreMaxScale: the kernel's largest reduction per axis
_cls_stage = {"buf": None, "event": None}  # the pinned staging buffer and the event behind its last copy


def classify_desc(shapes: Sequence[Tuple[int, int]], imgsz: int, bgr: bool = True) -> Tuple[np.ndarray, int]:
    """(the CLS_DESC table of images of `shapes` = (h, w) packed back to back, every start 16-byte aligned, rows 3 * w
    bytes apart; the 16-byte aligned size of the packed images)."""
    desc = np.zeros(len(shapes), dtype=CLS_DESC)
    off = 0
    for i, (h, w) in enumerate(shapes):
        desc[i] = (off, h, w, 3 * w, int(bgr)) + classify_geometry(h, w, imgsz)
        off = (off + 3 * h * w + 15) // 16 * 16
    return desc, off


def classify_batch_gpu(rt, imgs: Sequence[np.ndarray], device: torch.device, imgsz: int = 224,
                       stream: int = 0) -> torch.Tensor:
    """classify_batch on the GPU, bit for bit (csrc/ym_cls_pre.hip): the HWC uint8 BGR images and their descriptor
    table are packed into one pinned staging buffer (kept and grown from call to call), copied to `device` once, and
    one ym_classify_pre launch writes the (B, 3, imgsz, imgsz) fp32 device batch.  A batch with an image the kernel does
    not take (a side reduced more than CLS_PRE_MAX_SCALE-fold) goes through classify_batch whole."""
    if imgsz < 32 or imgsz % 32:
        raise ValueError(f"classify: imgsz {imgsz} must be a positive multiple of 32")
    desc, nbytes = classify_desc([im.shape[:2] for im in imgs], imgsz)
    if bool(np.any(desc["h"] > CLS_PRE_MAX_SCALE * desc["rh"]) or np.any(desc["w"] > CLS_PRE_MAX_SCALE * desc["rw"])):
        return classify_batch(imgs, imgsz).to(device)
    total = nbytes + desc.nbytes
    st = _cls_stage
    if st["event"] is not None:
        st["event"].synchronize()  # the last call's copy has read the buffer
    if st["buf"] is None or st["buf"].numel() < total:
        st["buf"] = torch.empty(max(total, 1 << 22), dtype=torch.uint8, pin_memory=True)
    host = st["buf"].numpy()
    for d, im in zip(desc, imgs):
        o, n = int(d["off"]), im.size
        host[o:o + n] = np.ascontiguousarray(im).reshape(-1)
    host[nbytes:total] = desc.view(np.uint8)
    with torch.cuda.device(device):
        dbuf = st["buf"][:total].to(device, non_blocking=True)
        st["event"] = torch.cuda.Event()
        st["event"].record()
    out = torch.empty((len(imgs), 3, imgsz, imgsz), dtype=torch.float32, device=device)
    rt.classify_pre(dbuf.data_ptr(), dbuf.data_ptr() + nbytes, st["buf"].data_ptr() + nbytes, len(imgs), imgsz,
                    out.data_ptr(), stream)
    return out


def scale_coords(img1_shape, coords: torch.Tensor, img0_shape) -> torch.Tensor:
    """ops.scale_coords(img1_shape, coords, img0_shape) (padding=True) + clip_coords, in place on a (..., >=2) tensor
    of x, y[, visibility] (Pose keypoints): the same gain / pad as scale_boxes, x clipped to [0, w0], y to [0, h0]."""
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    pad = (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1),
           round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))
    coords[..., 0] -= pad[0]
    coords[..., 1] -= pad[1]
    coords[..., 0] /= gain
    coords[..., 1] /= gain
    coords[..., 0].clamp_(0, img0_shape[1])
    coords[..., 1].clamp_(0, img0_shape[0])
    return coords


def mask_window(mh: int, mw: int, shape) -> Tuple[int, int, int, int]:
    """ops.scale_masks' crop of an (mh, mw) mask plane for a native image of `shape` = (h0, w0): (top, bottom, left,
    right), the rows [top, bottom) and columns [left, right) the letterboxed image occupies, which process_mask_native
    (retina_masks=True) resizes to (h0, w0).  csrc/ym_mask_native.hip restates the same rounding on the device.  A
    window that rounds to nothing (an extreme aspect ratio, where upstream's interpolate raises) is widened to one
    row / column."""
    h0, w0 = int(shape[0]), int(shape[1])
    gain = min(mh / h0, mw / w0)
    pad = ((mw - w0 * gain) / 2, (mh - h0 * gain) / 2)
    top, left = int(round(pad[1] - 0.1)), int(round(pad[0] - 0.1))
    bottom, right = mh - int(round(pad[1] + 0.1)), mw - int(round(pad[0] + 0.1))
    top, left = min(max(top, 0), mh - 1), min(max(left, 0), mw - 1)
    return top, min(max(bottom, top + 1), mh), left, min(max(right, left + 1), mw)


def scale_boxes(img1_shape, boxes: torch.Tensor, img0_shape) -> torch.Tensor:
    """ops.scale_boxes(img1_shape, boxes, img0_shape) (padding=True) + clip_boxes, in place on an (n, >=4) tensor."""
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    pad = (round((img1_shape[1] - img0_shape[1] * gain) / 2 - 0.1),
           round((img1_shape[0] - img0_shape[0] * gain) / 2 - 0.1))
    boxes[..., 0] -= pad[0]
    boxes[..., 1] -= pad[1]
    boxes[..., 2] -= pad[0]
    boxes[..., 3] -= pad[1]
    boxes[..., :4] /= gain
    boxes[..., 0].clamp_(0, img0_shape[1])
    boxes[..., 1].clamp_(0, img0_shape[0])
    boxes[..., 2].clamp_(0, img0_shape[1])
    boxes[..., 3].clamp_(0, img0_shape[0])
    return boxes
