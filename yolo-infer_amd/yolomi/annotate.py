"""The Python side of the GPU annotator (csrc/ym_annot.hip): `annotate_batch` behind Engine.annotate
(whole batches, asynchronous, frames stay on the device) and `plot_results` behind Results.plot() (one image)."""
from __future__ import annotations

import logging
from typing import Optional

import numpy as np
import torch

from .lib import (ANNOT_BOXES, ANNOT_CLIP_KPTS, ANNOT_COLOR_MODES, ANNOT_CONF, ANNOT_KPT_LINE, ANNOT_LABELS, ANNOT_MASKS,
                  ANNOT_NAME_BYTES, Runtime)

logger = logging.getLogger(__name__)


def default_line_width(H: int, W: int) -> int:
    """Upstream Annotator: max(round(sum(im.shape) / 2 * 0.003), 2) with the 3 channels in the sum (Python round)."""
    return max(round((H + W + 3) / 2 * 0.003), 2)


def name_table(names) -> np.ndarray:
    """(nc, 24) uint8: names[c] as ASCII, cut to 24 bytes, zero padded; nc = the largest class id + 1."""
    nc = max((int(k) for k in names), default=-1) + 1
    t = np.zeros((nc, ANNOT_NAME_BYTES), dtype=np.uint8)
    for k, v in names.items():
        raw = str(v).encode("ascii", "replace")[:ANNOT_NAME_BYTES]
        t[int(k), : len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return t


def _tables(eng):
    if eng._annot_tables is None:
        from .font6x11 import FONT_BYTES
        font = torch.frombuffer(bytearray(FONT_BYTES), dtype=torch.uint8).to(eng.device)
        nt = name_table(eng.names)
        names = torch.from_numpy(nt).to(eng.device) if nt.shape[0] else None
        eng._annot_tables = (font, names, nt.shape[0])
    return eng._annot_tables


def switch_flags(conf=True, labels=True, boxes=True, masks_on=True, kpt_line=True, clip_kpts=False) -> int:
    return ((ANNOT_CONF if conf else 0) | (ANNOT_LABELS if labels else 0) | (ANNOT_BOXES if boxes else 0) |
            (ANNOT_MASKS if masks_on else 0) | (ANNOT_KPT_LINE if kpt_line else 0) |
            (ANNOT_CLIP_KPTS if clip_kpts else 0))


def annotate_batch(eng, frames, dets, counts, *, masks=None, mask_offsets=None, mask_geo=None, mask_cap=None,
                   tracked=False, out=None, kpt_shape=None, line_width=None, kpt_radius=5, conf=True, labels=True,
                   boxes=True, masks_on=True, kpt_line=True, color_mode="class", names=None, clip_kpts=True):
    """Engine.annotate (documented there).  Only shapes, dtypes and addresses are looked at on the host."""
    dev = eng.device
    if frames.dim() != 4 or frames.device != dev or not frames.is_contiguous():
        raise ValueError("annotate: frames must be a contiguous (B, 3, H, W) fp32 or (B, H, W, 3) uint8 tensor on the "
                         "engine's device")
    if frames.dtype == torch.float32 and frames.shape[1] == 3:
        f32, (B, _, H, W) = True, frames.shape
    elif frames.dtype == torch.uint8 and frames.shape[3] == 3:
        f32, (B, H, W, _) = False, frames.shape
    else:
        raise ValueError(f"annotate: frames of shape {tuple(frames.shape)} and dtype {frames.dtype}")
    if (dets.dim() != 3 or dets.dtype != torch.float32 or dets.device != dev or dets.shape[0] < B or dets.stride(2) != 1
            or dets.stride(0) != dets.shape[1] * dets.stride(1)):
        raise ValueError("annotate: dets must be (>= B, max_det, stride) fp32 rows on the engine's device")
    if counts.dtype != torch.int32 or counts.device != dev or counts.numel() < B or not counts.is_contiguous():
        raise ValueError("annotate: counts must be (>= B,) int32 on the engine's device")
    if color_mode not in ANNOT_COLOR_MODES:
        raise ValueError(f"annotate: color_mode {color_mode!r} (one of {sorted(ANNOT_COLOR_MODES)})")
    if kpt_shape is None:
        kpt_shape = getattr(eng, "kpt_shape", None) if getattr(eng, "task", None) == "pose" else None
    K, nd = (int(kpt_shape[0]), int(kpt_shape[1])) if kpt_shape else (0, 0)
    max_det, stride = dets.shape[1], dets.stride(1)
    lw = int(line_width) if line_width else default_line_width(H, W)
    font, dnames, nc = _tables(eng)
    if names is not None and dict(names) != eng.names:  # a Results with names of its own: a table for this call
        nt = name_table(names)
        dnames, nc = (torch.from_numpy(nt).to(dev) if nt.shape[0] else None), nt.shape[0]
    mp = op = gp = 0
    mh = mw = cap = 0
    if masks is not None:
        if masks.device != dev or masks.dtype not in (torch.uint8, torch.bool) or not masks.is_contiguous():
            raise ValueError("annotate: masks must be contiguous uint8 / bool on the engine's device")
        if mask_offsets is None:
            if masks.dim() != 4 or masks.shape[0] < B:
                raise ValueError("annotate: masks without mask_offsets must be (B, cap, mh, mw) slots")
            cap, mh, mw = masks.shape[1:]
            mask_offsets = torch.arange(B, dtype=torch.int64, device=dev) * (cap * mh * mw)
        else:
            if (masks.dim() < 2 or mask_offsets.dtype != torch.int64 or mask_offsets.device != dev
                    or mask_offsets.numel() < B or mask_cap is None):
                raise ValueError("annotate: packed masks need (B,) int64 mask_offsets on the device and mask_cap")
            mh, mw = masks.shape[-2:]
            cap = int(mask_cap)
        if cap > 0 and mh > 0 and mw > 0:
            mp, op = masks.data_ptr(), mask_offsets.data_ptr()
        if mask_geo is not None:
            if mask_geo.dtype != torch.int32 or mask_geo.device != dev or mask_geo.numel() < 4 * B or not mask_geo.is_contiguous():
                raise ValueError("annotate: mask_geo must be (B, 4) int32 (uh, uw, top, left) on the engine's device")
            gp = mask_geo.data_ptr()
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    elif out.dtype != torch.uint8 or out.device != dev or tuple(out.shape) != (B, H, W, 3) or not out.is_contiguous():
        raise ValueError(f"annotate: out must be a contiguous ({B}, {H}, {W}, 3) uint8 tensor on the engine's device")
    args = Runtime.annotate_args(lw, kpt_radius, switch_flags(conf, labels, boxes, masks_on, kpt_line, clip_kpts),
                                 ANNOT_COLOR_MODES[color_mode], tracked, stride, K, nd, nc, cap, font.data_ptr())
    stream = torch.cuda.current_stream(dev).cuda_stream
    eng.rt.annotate(frames.data_ptr(), f32, B, H, W, dets.data_ptr(), max_det, counts.data_ptr(), mp, op, mh, mw, gp,
                    dnames.data_ptr() if dnames is not None else 0, args, out.data_ptr(), stream)
    return out


def plot_results(res, annotator, conf=True, line_width=None, kpt_radius=5, kpt_line=True, labels=True, boxes=True,
                 masks=True, img: Optional[np.ndarray] = None, color_mode="class") -> np.ndarray:
    """Results.plot(): the rows, masks and canvas of one Results as a batch of one through `annotator.annotate`."""
    dev = annotator.device
    H, W = res.orig_shape
    bx = torch.as_tensor(res.boxes.data).to(dev, torch.float32)
    n = bx.shape[0]
    kp = res.keypoints
    cols = [bx]
    kshape = None
    if kp is not None and kp.data.dim() == 3 and kp.data.shape[1] > 0:
        kd = torch.as_tensor(kp.data).to(dev, torch.float32)
        kshape = (kd.shape[1], kd.shape[2])
        cols.append(kd.reshape(n, kd.shape[1] * kd.shape[2]))  # (explicit width: n may be 0)
    rows = torch.cat(cols, dim=1).contiguous() if len(cols) > 1 else bx.contiguous()
    if n == 0:  # (a row buffer must hold one slot)
        rows = torch.zeros((1, max(rows.shape[1], 6)), dtype=torch.float32, device=dev)
    counts = torch.full((1,), n, dtype=torch.int32, device=dev)
    if img is not None:
        img = np.ascontiguousarray(img)
        if img.ndim != 3 or img.shape[2] != 3 or img.dtype != np.uint8:
            raise ValueError(f"plot: img must be HWC uint8 with 3 channels, got {img.shape} {img.dtype}")
        H, W = img.shape[:2]
        frames = torch.from_numpy(img).to(dev)[None]
    elif res._orig_tensor is not None:
        frames = res._orig_tensor.to(dev, torch.float32).contiguous()[None]
    else:
        frames = torch.from_numpy(np.ascontiguousarray(res.orig_img)).to(dev)[None]
    mk = geo = None
    if masks and res.masks is not None and n:
        md = torch.as_tensor(res.masks.data).to(dev)
        mk = (md if md.dtype in (torch.uint8, torch.bool) else md != 0).contiguous()[None]
        g = getattr(res, "_mask_geo", None)
        if g is None and tuple(mk.shape[-2:]) != (H, W):  # a mask plane of another size: the whole plane, resized
            g = (mk.shape[-2], mk.shape[-1], 0, 0)
        if g is not None:
            geo = torch.tensor([int(v) for v in g], dtype=torch.int32).to(dev)[None]
    out = annotator.annotate(frames, rows[None], counts, masks=mk, mask_geo=geo, tracked=bool(res.boxes.is_track),
                             kpt_shape=kshape or (0, 0), line_width=line_width, kpt_radius=kpt_radius, conf=conf,
                             labels=labels, boxes=boxes, masks_on=masks, kpt_line=kpt_line, color_mode=color_mode,
                             names=res.names, clip_kpts=False)
    return out[0].cpu().numpy()
