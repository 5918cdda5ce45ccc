"""Sequential restatement of the instance-polygon definition: what `Masks.xy` is before scale_coords.

Per plane: label the 8-connected foreground components and the 4-connected background (outside the plane is
background) by plain floods, keep the components that touch the background region holding the frame, trace each one's
outer border from its raster-first pixel with the Suzuki-Abe rule, compress the cyclic chain (a point stays when the
step into it and the step out of it differ) and choose the border with the most kept points, a tie going to the one
that starts last in raster order.  Nothing here is shared with csrc/ym_contour.h: components and top-level-ness come
from floods, not from the kernel's candidate / cycle-minimum / westward rules.
"""
import numpy as np

# (dx, dy) clockwise on screen (y down) starting at west
CW = [(-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1)]


def _flood(seed_list, ok, H, W, neigh):
    seen = set(seed_list)
    stack = list(seed_list)
    while stack:
        x, y = stack.pop()
        for dx, dy in neigh:
            n = (x + dx, y + dy)
            if 0 <= n[0] < W and 0 <= n[1] < H and n not in seen and ok(n[0], n[1]):
                seen.add(n)
                stack.append(n)
    return seen


def trace(m, sx, sy):
    """The emitted chain of the border that starts at (sx, sy): [(x, y), ...]."""
    H, W = m.shape

    def fg(x, y):
        return 0 <= x < W and 0 <= y < H and bool(m[y, x])

    q = next(((sx + dx, sy + dy) for dx, dy in CW if fg(sx + dx, sy + dy)), None)
    if q is None:
        return [(sx, sy)]
    p, r, chain = (sx, sy), q, []
    while True:
        chain.append(p)
        i = CW.index((r[0] - p[0], r[1] - p[1]))
        for k in range(1, 9):  # counter-clockwise, starting after r; r itself comes last
            dx, dy = CW[(i - k) % 8]
            if fg(p[0] + dx, p[1] + dy):
                nxt = (p[0] + dx, p[1] + dy)
                break
        if nxt == (sx, sy) and p == q:
            return chain
        r, p = p, nxt


def compress(chain):
    n = len(chain)
    if n == 1:
        return list(chain)
    out = []
    for i in range(n):
        a, b, c = chain[i - 1], chain[i], chain[(i + 1) % n]
        if (b[0] - a[0], b[1] - a[1]) != (c[0] - b[0], c[1] - b[1]):
            out.append(b)
    return out


def all_borders(mask):
    """Every top-level component's outer border, in raster order of the start pixels:
    [(start (x, y), emitted chain, kept points)]."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    # the frame's background region, on a plane padded by one pixel (coordinates shifted by +1)
    pad = np.zeros((H + 2, W + 2), dtype=bool)
    pad[1:-1, 1:-1] = m
    frame = _flood([(0, 0)], lambda x, y: not pad[y, x], H + 2, W + 2, [(-1, 0), (1, 0), (0, -1), (0, 1)])
    done = np.zeros((H, W), dtype=bool)
    out = []
    for y in range(H):
        for x in range(W):
            if not m[y, x] or done[y, x]:
                continue
            comp = _flood([(x, y)], lambda a, b: m[b, a], H, W, CW)
            for a, b in comp:
                done[b, a] = True
            top = any((a + 1 + dx, b + 1 + dy) in frame for a, b in comp for dx, dy in ((-1, 0), (1, 0), (0, -1), (0, 1)))
            if top:
                chain = trace(m, x, y)
                out.append(((x, y), chain, compress(chain)))
    return out


def contour(mask):
    """(k, 2) int32 (x, y) points of the chosen border; (0, 2) without foreground."""
    W = np.asarray(mask).shape[1]
    best = None
    for (x, y), _, kept in all_borders(mask):
        key = (len(kept), y * W + x)
        if best is None or key > best[0]:
            best = (key, kept)
    if best is None:
        return np.zeros((0, 2), dtype=np.int32)
    return np.asarray(best[1], dtype=np.int32).reshape(-1, 2)


def contours(masks):
    return [contour(m) for m in np.asarray(masks)]


def contour_fast(mask):
    """contour() for large planes (the 640 x 640 test): the same rules with scipy's labelling in place of the floods."""
    from scipy import ndimage
    m = np.asarray(mask) != 0
    H, W = m.shape
    lab, n = ndimage.label(m, structure=np.ones((3, 3)))
    pad = np.zeros((H + 2, W + 2), dtype=bool)
    pad[1:-1, 1:-1] = m
    bl, _ = ndimage.label(~pad)
    frame = bl == bl[0, 0]
    near = (frame[:-2, 1:-1] | frame[2:, 1:-1] | frame[1:-1, :-2] | frame[1:-1, 2:]) & m
    top = set(np.unique(lab[near]).tolist())
    first = {}
    ys, xs = np.nonzero(m)
    for x, y, l in zip(xs.tolist(), ys.tolist(), lab[ys, xs].tolist()):
        if l not in first:
            first[l] = (x, y)
    best = None
    for l in sorted(top):
        x, y = first[l]
        kept = compress(trace(m, x, y))
        key = (len(kept), y * W + x)
        if best is None or key > best[0]:
            best = (key, kept)
    if best is None:
        return np.zeros((0, 2), dtype=np.int32)
    return np.asarray(best[1], dtype=np.int32).reshape(-1, 2)
