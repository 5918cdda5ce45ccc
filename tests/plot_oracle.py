"""A numpy painter written from the drawing rules of DESIGN.md §17: what Results.plot() / Engine.annotate must produce,
bit for bit.  It paints in draw order (the mask blend, then boxes n-1..0, then keypoints n-1..0), each primitive over
what is there, where the kernel walks topmost-first with an early exit.  Of the package only the font table is read."""
import math

import numpy as np

from yolomi.font6x11 import GLYPHS

PALETTE_HEX = ("042AFF 0BDBEB F3F3F3 00DFB7 111F68 FF6FDD FF444F CCED00 00F344 BD00FF "
               "00B4FF DD00BA 00FFFF 26C000 01FFB3 7D24FF 7B0068 FF1B6C FC6D2F A2FF0B").split()
POSE_PALETTE = [[255, 128, 0], [255, 153, 51], [255, 178, 102], [230, 230, 0], [255, 153, 255], [153, 204, 255],
                [255, 102, 255], [255, 51, 255], [102, 178, 255], [51, 153, 255], [255, 153, 153], [255, 102, 102],
                [255, 51, 51], [153, 255, 153], [102, 255, 102], [51, 255, 51], [0, 255, 0], [0, 0, 255], [255, 0, 0],
                [255, 255, 255]]
KPT_IDX = [16] * 5 + [0] * 6 + [9] * 6
LIMB_IDX = [9, 9, 9, 9, 7, 7, 7, 0, 0, 0, 0, 0, 16, 16, 16, 16, 16, 16, 16]
SKELETON = [[16, 14], [14, 12], [17, 15], [15, 13], [12, 13], [6, 12], [7, 13], [6, 7], [6, 8], [7, 9], [8, 10], [9, 11],
            [2, 3], [1, 2], [1, 3], [2, 4], [3, 5], [4, 6], [5, 7]]
BOX_CLAMP, KPT_CLAMP = 1 << 30, 1 << 20


def palette(i):
    """BGR of Colors[i % 20]."""
    h = PALETTE_HEX[int(i) % 20]
    return (int(h[4:6], 16), int(h[2:4], 16), int(h[0:2], 16))


def pose_colour(i):
    r, g, b = POSE_PALETTE[i]
    return (b, g, r)


def text_colour(bgr):
    b, g, r = bgr
    return (17, 31, 104) if (299 * r + 587 * g + 114 * b) // 1000 >= 160 else (255, 255, 255)


def line_width(H, W, lw=None):
    return lw or max(round((H + W + 3) / 2 * 0.003), 2)


def trunc(v, lim=BOX_CLAMP):
    """int(v) after the clamp to +-lim; None for NaN."""
    v = float(v)
    if math.isnan(v):
        return None
    return lim if v >= lim else -lim if v <= -lim else int(v)


def fmt_conf(v):
    """Python's "%.2f" of the fp32 value while that is d.dd (-0 prints as 0); "?.??" otherwise."""
    v = float(np.float32(v))
    s = "%.2f" % (v + 0.0) if 0 <= v < 10 else ""
    return s if len(s) == 4 else "?.??"


def label_text(tracked, tid, name, conf_on, conf):
    return (("id:%d " % tid) if tracked else "") + name + ((" " + fmt_conf(conf)) if conf_on else "")


def clean_name(names, c):
    if c is None or c not in names:
        return "?"
    raw = str(names[c]).encode("ascii", "replace")[:24]
    return "".join(chr(ch) if 32 <= ch <= 126 else "?" for ch in raw.split(b"\0")[0]) or "?"


def label_layout(X1, Y1, n_chars, lw, W):
    """(left, top, w, h, s)."""
    s = max(1, lw // 2)
    pad = s
    tw, th = 6 * s * n_chars, 11 * s
    left = max(0, W - tw - 2 * pad) if X1 + tw + 2 * pad > W else X1
    top = Y1 - th - 2 * pad
    if top < 0:
        top = Y1
    return left, top, tw + 2 * pad, th + 2 * pad, s


def outline_mask(H, W, X1, Y1, X2, Y2, lw):
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    a = lw // 2
    b = lw - a
    outer = (x >= X1 - a) & (x <= X2 + a) & (y >= Y1 - a) & (y <= Y2 + a)
    inner = (x >= X1 + b) & (x <= X2 - b) & (y >= Y1 + b) & (y <= Y2 - b)
    return outer & ~inner


def rect_mask(H, W, left, top, w, h):
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    return (x >= left) & (x < left + w) & (y >= top) & (y < top + h)


def text_mask(H, W, left, top, s, text):
    m = np.zeros((H, W), dtype=bool)
    pad = s
    for j, ch in enumerate(text):
        c = ord(ch) if 32 <= ord(ch) <= 126 else ord("?")
        g = GLYPHS[c - 32]
        for gy in range(11):
            for gx in range(6):
                if (g[gy] >> (5 - gx)) & 1:
                    x0, y0 = left + pad + (6 * j + gx) * s, top + pad + gy * s
                    ys, ye, xs, xe = max(y0, 0), min(y0 + s, H), max(x0, 0), min(x0 + s, W)
                    if ys < ye and xs < xe:
                        m[ys:ye, xs:xe] = True
    return m


def disc_mask(H, W, cx, cy, r):
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    return (x - cx) ** 2 + (y - cy) ** 2 <= r * r


def limb_mask(H, W, A, B, t):
    """The capsule of thickness t around the integer segment A -> B (exact: Python integers via object arrays would
    be slow; the coordinates here keep every product far below 2^63)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    ax, ay, bx, by = int(A[0]), int(A[1]), int(B[0]), int(B[1])
    ex, ey = bx - ax, by - ay
    L2 = ex * ex + ey * ey
    px, py = x - ax, y - ay
    m = (4 * (px * px + py * py) <= t * t) | (4 * ((x - bx) ** 2 + (y - by) ** 2) <= t * t)
    if L2 > 0:
        dot = px * ex + py * ey
        cr = np.abs(px * ey - py * ex)
        near = cr <= (1 << 30)  # beyond this 4 cr^2 > t^2 L2 for every admissible t and L2
        body = (dot >= 0) & (dot <= L2) & near
        crs = np.where(near, cr, 0)
        m |= body & (4 * crs * crs <= t * t * L2)
    return m


def kpt_drawable(k, ndim, W, H, clip=False):
    """(x, y) integers, or None.  clip: x, y clipped to [0, W], [0, H] first (what predict()'s Results hold)."""
    x, y = np.float32(k[0]), np.float32(k[1])
    if ndim == 3 and not (np.float32(k[2]) >= np.float32(0.5)):
        return None
    if clip:
        x = np.float32(0) if x < 0 else np.float32(W) if x > W else x
        y = np.float32(0) if y < 0 else np.float32(H) if y > H else y
    if not (np.isfinite(x) and np.isfinite(y)) or abs(float(x)) > KPT_CLAMP or abs(float(y)) > KPT_CLAMP:
        return None
    if np.fmod(x, np.float32(W)) == 0 or np.fmod(y, np.float32(H)) == 0:
        return None
    return int(x), int(y)


def canvas_from_tensor(chw):
    """trunc(clamp(x * 255, 0, 255)) in fp32, HWC, no channel flip; NaN -> 0."""
    v = np.asarray(chw, dtype=np.float32) * np.float32(255)
    v = np.where(np.isnan(v), np.float32(0), v)
    return np.clip(v, 0, 255).astype(np.uint8).transpose(1, 2, 0).copy()


def blend_value(u, cols):
    """One channel under the covering colours `cols`: fp32, every operation rounded on its own."""
    f = np.float32
    inv = f(0.5) ** f(len(cols))
    mcs = max(f(f(c) / f(255)) * f(0.5) for c in cols)
    v = f(f(f(f(u) / f(255)) * inv) + mcs) * f(255)
    return int(min(max(v, f(0)), f(255)))


def blend_masks(img, masks, colours, geo):
    """masks: (n, mh, mw); colours: n BGR tuples; geo = (uh, uw, top, left)."""
    H, W = img.shape[:2]
    n, mh, mw = masks.shape
    uh, uw, top, left = geo
    f = np.float32
    ys = top + np.minimum(((2 * np.arange(H, dtype=np.int64) + 1) * uh) // (2 * H), uh - 1)
    xs = left + np.minimum(((2 * np.arange(W, dtype=np.int64) + 1) * uw) // (2 * W), uw - 1)
    ok = ((ys >= 0) & (ys < mh))[:, None] & ((xs >= 0) & (xs < mw))[None, :]
    cov = (masks[:, np.clip(ys, 0, mh - 1)][:, :, np.clip(xs, 0, mw - 1)] != 0) & ok[None]  # (n, H, W)
    k = cov.sum(0)
    inv = np.power(f(0.5), k.astype(f)).astype(f)
    out = img.copy()
    for c in range(3):
        col = np.array([cl[c] for cl in colours], dtype=f)
        half = ((col / f(255)).astype(f) * f(0.5)).astype(f)
        mcs = np.where(cov, half[:, None, None], f(-1)).max(0).astype(f)
        a = ((img[..., c].astype(f) / f(255)).astype(f) * inv).astype(f)
        v = ((a + mcs).astype(f) * f(255)).astype(f)
        out[..., c] = np.where(k > 0, np.clip(v, 0, 255).astype(np.uint8), img[..., c])
    return out


def paint(canvas, rows, names, *, tracked=False, kpt_shape=None, masks=None, mask_geo=None, line_width_=None,
          kpt_radius=5, conf=True, labels=True, boxes=True, masks_on=True, kpt_line=True, color_mode="class",
          clip_kpts=False):
    """canvas: (H, W, 3) uint8 (not modified); rows: (n, stride) fp32 [x1 y1 x2 y2 (id) conf cls kpts...]; masks:
    (n, mh, mw) or None.  Returns the painted copy."""
    img = np.array(canvas, copy=True)
    H, W = img.shape[:2]
    n = len(rows)
    rows = np.asarray(rows, dtype=np.float32).reshape(n, -1) if n else np.zeros((0, 7), dtype=np.float32)
    lw = line_width(H, W, line_width_)
    ccol, kcol = (6, 7) if tracked else (5, 6)
    cls = [trunc(r[ccol]) for r in rows]
    tid = [(trunc(r[4]) or 0) if tracked else 0 for r in rows]
    colours = [palette(((tid[i] if tracked else i) if color_mode == "instance" else (cls[i] or 0))) for i in range(n)]
    if masks_on and masks is not None and n and len(masks):
        m = np.asarray(masks)
        geo = tuple(int(v) for v in mask_geo) if mask_geo is not None else (H, W, 0, 0)
        img = blend_masks(img, m[:n], colours[:len(m)], geo)
    if boxes:
        for i in range(n - 1, -1, -1):
            c = [trunc(v) for v in rows[i, :4]]
            if any(v is None for v in c):
                continue
            X1, Y1, X2, Y2 = c
            img[outline_mask(H, W, X1, Y1, X2, Y2, lw)] = colours[i]
            if labels:
                text = label_text(tracked, tid[i], clean_name(names, cls[i]), conf, rows[i, ccol - 1])
                left, top, w, h, s = label_layout(X1, Y1, len(text), lw, W)
                img[rect_mask(H, W, left, top, w, h)] = colours[i]
                img[text_mask(H, W, left, top, s, text)] = text_colour(colours[i])
    if kpt_shape and kpt_shape[0]:
        K, nd = kpt_shape
        t = (lw + 1) // 2
        for i in range(n - 1, -1, -1):
            pts = [kpt_drawable(rows[i, kcol + k * nd: kcol + (k + 1) * nd], nd, W, H, clip_kpts) for k in range(K)]
            for k, p in enumerate(pts):
                if p is not None:
                    img[disc_mask(H, W, p[0], p[1], kpt_radius)] = pose_colour(KPT_IDX[k]) if K == 17 else palette(k)
            if K == 17 and kpt_line:
                for l, (a, b) in enumerate(SKELETON):
                    if pts[a - 1] is not None and pts[b - 1] is not None:
                        img[limb_mask(H, W, pts[a - 1], pts[b - 1], t)] = pose_colour(LIMB_IDX[l])
    return img


def paint_results(res, **kw):
    """paint() on a Results' own host data (boxes, keypoints, masks, orig_img, names, mask geometry)."""
    bx = np.asarray(res.boxes.data.cpu().numpy() if hasattr(res.boxes.data, "cpu") else res.boxes.data, dtype=np.float32)
    rows, kshape = bx, None
    kp = res.keypoints
    if kp is not None:
        kd = np.asarray(kp.data.cpu().numpy() if hasattr(kp.data, "cpu") else kp.data, dtype=np.float32)
        kshape = kd.shape[1:]
        rows = np.concatenate([bx, kd.reshape(len(bx), kd.shape[1] * kd.shape[2])], axis=1)  # (len(bx) may be 0)
    mk = geo = None
    if res.masks is not None:
        mk = res.masks.data.cpu().numpy().astype(np.uint8) if hasattr(res.masks.data, "cpu") else np.asarray(res.masks.data)
        geo = getattr(res, "_mask_geo", None)
        if geo is None and tuple(mk.shape[-2:]) != tuple(res.orig_shape):
            geo = (mk.shape[-2], mk.shape[-1], 0, 0)
    return paint(res.orig_img, rows, res.names, tracked=bx.shape[1] == 7, kpt_shape=kshape, masks=mk, mask_geo=geo, **kw)
