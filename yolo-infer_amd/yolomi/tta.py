"""Test-time augmentation geometry (Ultralytics DetectionModel._predict_augment; csrc/ym_tta.h states the same rules
for the library): the three passes' shapes and which of their anchors survive _clip_augmented.  Pure Python."""
from __future__ import annotations

import math
from typing import List, Tuple

from .arch import num_anchors  # noqa: F401  (tta.num_anchors: the passes' anchor counts)

RATIOS = (1.0, 0.83, 0.67)
FLIPS = (False, True, False)  # True: the W axis is mirrored
PAD_VALUE = 0.447
GRID = 32


def pass_shapes(H: int, W: int) -> List[Tuple[int, int, int, int]]:
    """Per pass (Hs, Ws, hc, wc): scale_img resizes to hc x wc = int(H s) x int(W s) and pads right / bottom to
    Hs x Ws = the next multiples of 32 of H s x W s; ratio 1 leaves the input as it is."""
    out = []
    for s in RATIOS:
        if s == 1.0:
            out.append((H, W, H, W))
        else:
            out.append((math.ceil(H * s / GRID) * GRID, math.ceil(W * s / GRID) * GRID, int(H * s), int(W * s)))
    return out


def kept_anchors(H: int, W: int) -> List[Tuple[int, int]]:
    """Per pass (first, count) of the anchors that survive _clip_augmented (g = 21): pass 0 loses its last A // 21
    anchors, the last pass its first (A // 21) * 16, the middle one none.  The merged anchor order is pass order."""
    A = [num_anchors(hs, ws) for hs, ws, _, _ in pass_shapes(H, W)]
    first2 = (A[2] // 21) * 16
    return [(0, A[0] - A[0] // 21), (0, A[1]), (first2, A[2] - first2)]
