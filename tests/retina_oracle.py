"""Restated Ultralytics 8.3.x `ops.scale_masks` + `ops.process_mask_native` (the retina_masks=True branch of
`SegmentationPredictor.construct_result`), written from their definition.  TEST INFRASTRUCTURE ONLY.

    process_mask_native(protos (c, mh, mw), masks_in (n, c), bboxes (n, 4) in NATIVE pixels, shape (h0, w0)):
        m = (masks_in @ protos.view(c, -1)).view(-1, mh, mw)          # no crop at prototype resolution
        m = scale_masks(m[None], shape)[0]                             # letterbox window -> (h0, w0), bilinear
        m = crop_mask(m, bboxes)                                       # x1 <= x < x2, y1 <= y < y2 on float aranges
        return m > 0

Runs in the dtype of its inputs: float32 as upstream, or float64 (the reference of the GPU tests).  The bilinear
resize is written out (torch's upsample_bilinear2d, align_corners=False: source index (dst + 0.5) * in / out - 0.5
clamped at 0, neighbour clamped at in - 1) so the float64 run does not depend on F.interpolate's internal precision;
`interpolate=True` calls F.interpolate itself instead (tests/test_retina_host.py checks the two agree).
"""
from __future__ import annotations

from typing import Sequence, Tuple

import torch
import torch.nn.functional as F


def mask_window(mh: int, mw: int, shape) -> Tuple[int, int, int, int]:
    """scale_masks' crop: (top, bottom, left, right) of the (mh, mw) plane for a native (h0, w0) image."""
    h0, w0 = shape
    gain = min(mh / h0, mw / w0)
    pad = ((mw - w0 * gain) / 2, (mh - h0 * gain) / 2)
    top, left = int(round(pad[1] - 0.1)), int(round(pad[0] - 0.1))
    bottom, right = mh - int(round(pad[1] + 0.1)), mw - int(round(pad[0] + 0.1))
    return top, bottom, left, right


def _axis(n_in: int, n_out: int, dtype):
    scale = torch.tensor(n_in, dtype=dtype) / n_out  # one quotient in the working precision
    f = ((torch.arange(n_out, dtype=dtype) + 0.5) * scale - 0.5).clamp_(min=0)
    i0 = f.floor().long().clamp_(max=n_in - 1)
    i1 = (i0 + 1).clamp_(max=n_in - 1)
    return i0, i1, f - i0.to(dtype)


def resize_bilinear(m: torch.Tensor, shape) -> torch.Tensor:
    """(n, h, w) -> (n, h0, w0): F.interpolate(m[None], shape, mode="bilinear", align_corners=False)[0]."""
    h0, w0 = shape
    y0, y1, ly = _axis(m.shape[1], h0, m.dtype)
    x0, x1, lx = _axis(m.shape[2], w0, m.dtype)
    ly, lx = ly[None, :, None], lx[None, None, :]
    r0, r1 = m[:, y0], m[:, y1]
    return (1 - ly) * ((1 - lx) * r0[:, :, x0] + lx * r0[:, :, x1]) + ly * ((1 - lx) * r1[:, :, x0] + lx * r1[:, :, x1])


def scale_masks(m: torch.Tensor, shape, interpolate: bool = False) -> torch.Tensor:
    """(n, mh, mw) -> (n, h0, w0)."""
    top, bottom, left, right = mask_window(m.shape[1], m.shape[2], shape)
    m = m[:, top:bottom, left:right]
    if interpolate:
        return F.interpolate(m[None], tuple(shape), mode="bilinear", align_corners=False)[0]
    return resize_bilinear(m, shape)


def crop_mask(m: torch.Tensor, boxes: torch.Tensor) -> torch.Tensor:
    _, h, w = m.shape
    x1, y1, x2, y2 = torch.chunk(boxes[:, :, None], 4, 1)
    r = torch.arange(w, dtype=x1.dtype)[None, None, :]
    c = torch.arange(h, dtype=x1.dtype)[None, :, None]
    return m * ((r >= x1) * (r < x2) * (c >= y1) * (c < y2))


def process_mask_native(protos: torch.Tensor, masks_in: torch.Tensor, bboxes: torch.Tensor, shape,
                        interpolate: bool = False) -> torch.Tensor:
    """(n, h0, w0) bool.  protos (c, mh, mw), masks_in (n, c) and bboxes (n, 4, native pixels) share one dtype."""
    c, mh, mw = protos.shape
    m = (masks_in @ protos.reshape(c, -1)).view(-1, mh, mw)
    m = scale_masks(m, shape, interpolate)
    return crop_mask(m, bboxes) > 0


def box_range(box: Sequence[float], shape) -> Tuple[int, int, int, int]:
    """crop_mask's integer pixel range of one box: (x0, x1, y0, y1), columns [x0, x1) and rows [y0, y1)."""
    import math
    h0, w0 = shape
    cl = lambda v, n: int(min(max(math.ceil(v), 0), n))
    return cl(box[0], w0), cl(box[2], w0), cl(box[1], h0), cl(box[3], h0)


def oracle_rows(om, x: torch.Tensor, conf: float, iou: float = 0.7, max_det: int = 300):
    """The oracle's NMS rows (n, 6 + 32) per image, boxes still in network pixels, its prototypes (B, 32, mh, mw) and
    the network (H, W).  om: oracle.predict.OracleModel of a segment model."""
    from oracle import postprocess as pp
    im, y, ex = om.raw(x)
    dets = pp.non_max_suppression(y, conf, iou, None, False, max_det, nc=80)
    return dets, ex["proto"], tuple(im.shape[2:])


def oracle_retina(om, x: torch.Tensor, shapes, conf: float, dtype=torch.float64, iou: float = 0.7):
    """The oracle's predict(retina_masks=True): per image {"boxes": (n, 6) in native pixels, "masks": (n, h0, w0)
    bool}, empty masks dropped.  shapes: the native (h0, w0) per image (a tensor source: its own (H, W))."""
    from oracle import postprocess as pp
    dets, proto, net = oracle_rows(om, x, conf, iou)
    out = []
    for b, d in enumerate(dets):
        d = d.clone()
        d[:, :4] = pp.scale_boxes(net, d[:, :4], shapes[b])
        m = process_mask_native(proto[b].to(dtype), d[:, 6:].to(dtype), d[:, :4].to(dtype), shapes[b])
        keep = m.flatten(1).any(1)
        out.append({"boxes": d[keep, :6], "masks": m[keep]})
    return out
