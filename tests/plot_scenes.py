"""Scripted scenes for the annotator: the same rows, masks and switches go to tests/plot_oracle.py, to the host build of
csrc/ym_annot.h (tests/test_plot_host.py) and to the kernels (tests/test_gpu_plot.py).  A scene is a batch of two images
with different counts; rows behind an image's count hold a full-canvas box that must never be drawn."""
import struct

import numpy as np

NAMES = {0: "person", 1: "bicycle", 2: "car", 3: "a name that is longer than twenty-four characters", 4: "café",
         5: "dog", 7: "truck", 19: "cow", 22: "zebra"}
SIZES = ((72, 104), (40, 136))  # neither side a multiple of the 64 x 16 tile
FLAGS = {"boxes": 1, "labels": 2, "conf": 4, "masks_on": 8, "kpt_line": 16}  # on by default
CLIP_KPTS = 32  # off by default


def name_table(names=None):
    """(nc, 24) uint8: the class-name table of the C-ABI, built here from the rule (ASCII, cut to 24, zero padded)."""
    names = NAMES if names is None else names
    t = np.zeros((max(names) + 1, 24), dtype=np.uint8)
    for k, v in names.items():
        raw = v.encode("ascii", "replace")[:24]
        t[k, :len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    return t


def frames_f32(seed, B, H, W):
    """fp32 CHW in [-0.1, 1.1]: both clamps are exercised."""
    return (np.random.default_rng(seed).random((B, 3, H, W), dtype=np.float32) * np.float32(1.2) - np.float32(0.1))


def frames_u8(seed, B, H, W):
    return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)


def det(x1, y1, x2, y2, conf, cls, *extra, tid=None):
    return [x1, y1, x2, y2] + ([tid] if tid is not None else []) + [conf, cls] + list(extra)


def pose17(cx, cy, s, ndim=3, vis=None):
    """A stick figure around (cx, cy) of size s: 17 keypoints."""
    base = [(0, -4), (-.5, -4.5), (.5, -4.5), (-1, -4), (1, -4), (-2, -2.5), (2, -2.5), (-3, -1), (3, -1), (-3.5, .5),
            (3.5, .5), (-1.5, 1), (1.5, 1), (-1.7, 3), (1.7, 3), (-1.8, 5), (1.8, 5)]
    out = []
    for k, (dx, dy) in enumerate(base):
        out += [cx + dx * s + 0.4, cy + dy * s + 0.7]
        if ndim == 3:
            out.append(0.9 if vis is None else vis[k])
    return out


def scene(name, H, W, rows0, rows1, stride, **kw):
    s = dict(name=name, H=H, W=W, rows=[rows0, rows1], stride=stride, tracked=False, kpt_shape=None, masks=None,
             geo=None, u8=False, opts={}, seed=sum(map(ord, name)))
    s.update(kw)
    return s


def rect_plane(mh, mw, y0, y1, x0, x1):
    m = np.zeros((mh, mw), dtype=np.uint8)
    m[max(y0, 0):y1, max(x0, 0):x1] = 1
    return m


def scenes(H, W):
    out = []
    out.append(scene("count0_count1", H, W, [], [det(10.9, 20.2, 60.5, 33.7, 0.625, 2)], 6))
    # 300 identical poses and boxes over one tile: every chunk of every list is full
    many = [det(3.5, 2.5, 50.5, 14.5, 0.875, 1, *pose17(30, 8, 1.5)) for _ in range(300)]
    many[0] = det(8.5, 4.5, 40.5, 12.5, 0.125, 5, *pose17(24, 9, 1.2))
    many[299] = det(1.5, 1.5, 62.5, 15.5, 0.375, 7, *pose17(36, 7, 1.4))
    out.append(scene("chunks300", H, W, many, [det(5, 5, 30, 30, 0.5, 0, *pose17(20, 20, 2))], 6 + 51,
                     kpt_shape=(17, 3)))
    out.append(scene("overlap_order", H, W,
                     [det(10, 14, 50, 36, 0.91, 0), det(30, 16, 80, 38, 0.82, 2), det(20, 20, 60, 30, 0.73, 19),
                      det(22, 22, 58, 28, 0.64, 22)],
                     [det(0, 0, W, H, 0.995, 3), det(1, 1, 2, 2, 1.0, 4), det(40, 20, 40, 20, 0.0, 6)], 6))
    big = 1e9
    out.append(scene("outside_negative_bad", H, W,
                     [det(-20.5, -10.5, 30.5, 20.5, 0.55, 0), det(W - 20, H - 12, W + 30, H + 30, 0.66, 1),
                      det(W + 5, 5, W + 50, 20, 0.77, 2), det(-60, -60, -5, -5, 0.88, 5), det(20, -30, 70, -1, 0.5, 7),
                      det(W - 8, 30, W - 2, 36, 0.45, 19)],
                     [det(np.nan, 5, 30, 30, 0.5, 0), det(-big, -big, big, big, 0.5, 1), det(big, 5, big, 30, 0.5, 2),
                      det(5, 5, np.inf, 30, 0.5, 5), det(-np.inf, 6, 30, np.nan, 0.5, 7), det(8, 12, 40, 30, np.nan, 2),
                      det(12, 16, 44, 34, 0.5, np.nan), det(16, 20, 48, 38, 0.5, 1e9), det(50, 8, 90, 30, -0.5, -3),
                      det(60, 12, 100, 34, 12.0, 2)], 6))
    # masks: pixels under zero, one and three masks; a mask reaching outside its own box; identity geometry
    m0 = np.stack([rect_plane(H, W, 5, 30, 5, 50), rect_plane(H, W, 10, 36, 20, 70), rect_plane(H, W, 0, H, 40, 60),
                   rect_plane(H, W, 20, 39, 80, 100)])
    rows_m = [det(5, 5, 50, 30, 0.9, 0), det(20, 10, 70, 36, 0.8, 2), det(44, 12, 56, 24, 0.7, 19),
              det(80, 20, 100, 39, 0.6, 22)]
    m1 = rect_plane(H, W, 2, 20, 3, 90)[None]
    out.append(scene("masks_identity", H, W, rows_m, [det(3, 2, 90, 20, 0.5, 1)], 6, masks=[m0, m1]))
    mh, mw = 48, 160
    g0 = np.stack([rect_plane(mh, mw, 6, 30, 8, 60), rect_plane(mh, mw, 0, mh, 50, 90),
                   rect_plane(mh, mw, 20, 44, 0, mw)])
    out.append(scene("masks_geometry", H, W, rows_m[:3], [det(3, 2, 90, 20, 0.5, 1)], 6,
                     masks=[g0, g0[:1]], geo=[(40, 150, 4, 6), (44, 140, 2, 10)]))
    vis = [0.9] * 17
    vis[3], vis[9] = 0.2, 0.49
    p_a = pose17(40, 22, 3, vis=vis)
    p_b = pose17(70, 20, 2)
    p_b[0 * 3], p_b[1 * 3 + 1] = 0.0, 0.0          # at coordinate 0
    p_b[5 * 3] = float(W)                           # x = W
    p_b[7 * 3:7 * 3 + 2] = p_b[5 * 3 + 0] - W + 60, p_b[5 * 3 + 1]
    p_b[13 * 3:13 * 3 + 2] = p_b[11 * 3:11 * 3 + 2]  # a degenerate limb: keypoints 12 and 14 coincide
    p_c = pose17(W - 6, H - 5, 4)                   # partly outside (clipped like upstream's scale_coords would not)
    p_d = pose17(30, 20, 2)
    p_d[0], p_d[4] = np.nan, 1e30
    p_d[6 * 3], p_d[6 * 3 + 1] = -5e5, 7e5          # inside the keypoint clamp, far outside the canvas
    out.append(scene("pose17_v", H, W, [det(20, 5, 60, 38, 0.9, 0, *p_a), det(55, 8, 85, 32, 0.8, 0, *p_b)],
                     [det(W - 30, H - 30, W, H, 0.7, 0, *p_c), det(10, 5, 50, 35, 0.6, 0, *p_d)], 6 + 51,
                     kpt_shape=(17, 3)))
    # keypoints beyond every border, raw and clipped to the canvas first (what predict()'s Results hold)
    for tag, opts in (("raw", {}), ("clip", dict(clip_kpts=True))):
        out.append(scene("pose17_border_" + tag, H, W, [det(W - 30, H - 30, W, H, 0.7, 0, *p_c)],
                         [det(0, 0, 20, 20, 0.6, 0, *pose17(3, 4, 3)), det(10, 5, 50, 35, 0.6, 0, *p_d)], 6 + 51,
                         kpt_shape=(17, 3), opts=opts))
    q_a = pose17(40, 22, 3, ndim=2)
    q_b = pose17(70, 20, 2, ndim=2)
    q_b[0:2] = 0.0, 0.0
    q_b[10] = float(W)
    out.append(scene("pose17_xy", H, W, [det(20, 5, 60, 38, 0.9, 0, *q_a)],
                     [det(55, 8, 85, 32, 0.8, 0, *q_b), det(20, 5, 60, 38, 0.9, 0, *q_a)], 6 + 34 + 2, kpt_shape=(17, 2)))
    k5 = [12.5, 10.5, 0.9, 30.2, 12.9, 0.8, 50.0, 20.0, 0.3, 64.5, 16.5, 0.7, 63.0, 18.0, 0.6]
    out.append(scene("pose5", H, W, [det(8, 6, 70, 26, 0.9, 0, *k5)], [], 6 + 15, kpt_shape=(5, 3)))
    out.append(scene("tracked", H, W,
                     [det(5, 14, 40, 36, 0.91, 0, tid=1), det(30, 16, 70, 38, 0.82, 2, tid=42),
                      det(50, 15, 100, 30, 0.73, 5, tid=1234567)],
                     [det(10, 14, 60, 36, 0.5, 1, tid=-7)], 7, tracked=True))
    out.append(scene("tracked_pose", H, W, [det(20, 5, 60, 38, 0.9, 0, *p_a, tid=3)], [], 7 + 51, tracked=True,
                     kpt_shape=(17, 3)))
    out.append(scene("u8_frames", H, W, rows_m, [det(3, 2, 90, 20, 0.5, 1)], 6, masks=[m0, m1], u8=True))
    # every switch, one at a time, and the other options, on one rich scene: masks, boxes and poses together
    rich0 = [det(20, 5, 60, 38, 0.9, 0, *p_a), det(55, 8, 85, 32, 0.8, 2, *p_b),
             det(30, 12, 75, 30, 0.7, 19, *pose17(50, 20, 2))]
    rich1 = [det(10, 14, 60, 36, 0.5, 1, *pose17(30, 24, 2))]
    for tag, opts in (("boxes_off", dict(boxes=False)), ("labels_off", dict(labels=False)), ("conf_off", dict(conf=False)),
                      ("masks_off", dict(masks_on=False)), ("kpt_line_off", dict(kpt_line=False)),
                      ("instance", dict(color_mode="instance")), ("lw1_r2", dict(line_width_=1, kpt_radius=2)),
                      ("lw3", dict(line_width_=3)), ("lw6_r7", dict(line_width_=6, kpt_radius=7)), ("default", {})):
        out.append(scene("rich_" + tag, H, W, rich0, rich1, 6 + 51, kpt_shape=(17, 3), masks=[m0[:3], m1], opts=opts))
    return out


def batch_arrays(s, max_det=None):
    """(frames, dets (2, max_det, stride), counts (2,), masks (2, cap, mh, mw) | None, geo (2, 4) int32 | None)."""
    H, W = s["H"], s["W"]
    B = 2
    n = [len(r) for r in s["rows"]]
    max_det = max_det or max(max(n), 1) + 2
    fill = det(0, 0, W, H, 0.99, 0, tid=9 if s["tracked"] else None)
    dets = np.zeros((B, max_det, s["stride"]), dtype=np.float32)
    dets[:, :, :len(fill)] = fill
    for b in range(B):
        for i, r in enumerate(s["rows"][b]):
            dets[b, i, :] = 0
            dets[b, i, :len(r)] = r
    frames = frames_u8(s["seed"], B, H, W) if s["u8"] else frames_f32(s["seed"], B, H, W)
    masks = geo = None
    if s["masks"] is not None:
        cap = max(len(m) for m in s["masks"])
        mh, mw = s["masks"][0].shape[1:]
        masks = np.ones((B, cap, mh, mw), dtype=np.uint8)  # (planes behind an image's count are set: never read)
        for b in range(B):
            masks[b, :len(s["masks"][b])] = s["masks"][b]
    if s["geo"] is not None:
        geo = np.asarray(s["geo"], dtype=np.int32)
    return frames, dets, np.asarray(n, dtype=np.int32), masks, geo


def oracle_image(s, b, arrays):
    """The oracle's picture of image b of a scene."""
    from tests import plot_oracle as O
    frames, dets, counts, masks, geo = arrays
    canvas = frames[b] if s["u8"] else O.canvas_from_tensor(frames[b])
    n = int(counts[b])
    return O.paint(canvas, dets[b, :n], NAMES, tracked=s["tracked"], kpt_shape=s["kpt_shape"],
                   masks=masks[b, :n] if masks is not None else None, mask_geo=geo[b] if geo is not None else None,
                   **s["opts"])


def scene_file(s, b, arrays, font_bytes, name_table):
    """Image b of a scene as tests/annot_check.cpp's `render` input."""
    from tests import plot_oracle as O
    frames, dets, counts, masks, geo = arrays
    H, W = s["H"], s["W"]
    o = s["opts"]
    flags = sum(v for k, v in FLAGS.items() if o.get(k, True)) + (CLIP_KPTS if o.get("clip_kpts") else 0)
    K, nd = s["kpt_shape"] or (0, 0)
    n = int(counts[b])
    has_m = masks is not None
    mcap, mh, mw = (masks.shape[1:] if has_m else (0, 0, 0))
    g = geo[b] if geo is not None else (H, W, 0, 0)
    hdr = [H, W, O.line_width(H, W, o.get("line_width_")), o.get("kpt_radius", 5), flags,
           int(o.get("color_mode", "class") == "instance"), int(s["tracked"]), K, nd, name_table.shape[0], s["stride"], n,
           int(not s["u8"]), int(has_m), mh, mw, mcap, *[int(v) for v in g]]
    blob = struct.pack("<21i", *hdr) + font_bytes + name_table.tobytes() + dets[b, :n].tobytes() + frames[b].tobytes()
    if has_m:
        blob += masks[b].tobytes()
    return blob
