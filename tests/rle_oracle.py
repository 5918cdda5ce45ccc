"""COCO run-length encoding, restated plainly (pycocotools' rleEncode / rleToString / rleFrString)."""
import numpy as np


def encode(plane):
    """(H, W) plane, non-zero = set -> (counts: uint32 array, string: bytes, area: int)."""
    flat = (np.asarray(plane).T.reshape(-1) != 0).astype(np.int8)  # column-major
    at = np.flatnonzero(np.diff(np.concatenate([[0], flat])))      # pixel i differs from pixel i - 1 (pixel -1 is 0)
    counts = np.diff(np.concatenate([[0], at, [flat.size]])).astype(np.int64)
    out = bytearray()
    for k, x in enumerate(counts.tolist()):
        if k > 2:
            x -= int(counts[k - 2])
        while True:
            c = x & 0x1f
            x >>= 5  # Python's shift of a negative int is arithmetic
            more = (x != -1) if c & 0x10 else (x != 0)
            out.append((c | 0x20 if more else c) + 48)
            if not more:
                break
    return counts.astype(np.uint32), bytes(out), int(counts[1::2].sum())


def decode(string, size):
    """The compressed string and [H, W] -> the (H, W) uint8 plane."""
    counts, i = [], 0
    while i < len(string):
        x, k, more = 0, 0, True
        while more:
            c = string[i] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            i, k = i + 1, k + 1
            if not more and c & 0x10:
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    h, w = size
    assert sum(counts) == h * w
    flat = np.repeat(np.arange(len(counts)) & 1, counts).astype(np.uint8)
    return flat.reshape(w, h).T
