"""GPU tests of the frame-batch letterbox (csrc/ym_letterbox_batch.hip through yolomi.preprocess.letterbox_frames and
YOLO11Model's uint8 device-frame sources): the fp32 bits of oracle/letterbox.py, and the ndarray sources' results."""
import numpy as np
import pytest
import torch

from oracle import letterbox as olb
from yolomi.preprocess import letterbox_frames
from yolomi.synth import synth_weights, uniform

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# (h, w, imgsz, geo): geo None = the predictor's own geometry, else (uh, uw, top, bottom, left, right).  The tile is
# 64 x 16 and reads at most 32 source rows, staged in 16 KiB chunks unless a row segment exceeds 2 KiB.
CASES = [
    (37, 53, 64, (45, 57, 9, 10, 3, 4)),      # upscale, odd sizes, borders on all four sides
    (853, 1280, 640, None),                   # the survey's image: 448 x 640 auto canvas, both axes halved
    (64, 96, 96, None),                       # uh == h, uw == w: no pass; the canvas is 1.5 tiles wide
    (33, 1000, 64, None),                     # 15.6-fold horizontal reduction: the segment is gathered, not staged
    (1000, 33, 64, None),                     # the same vertically: row pairs instead of the row span
    (200, 520, 64, None),                     # 8-fold: row pairs, staged in four chunks
    (20, 520, 64, (16, 64, 8, 8, 0, 0)),      # the dense row span, staged in three chunks
    (50, 70, 96, (17, 65, 0, 15, 0, 31)),     # the window ends one past the tile's edge, both axes
    (50, 70, 64, (15, 63, 1, 16, 0, 1)),      # ... and one short of it
    (50, 70, 96, (17, 65, 7, 8, 15, 16)),     # tile edges inside the window on all sides
]
_cache = {}


def runtime():
    if "eng" not in _cache:
        from yolomi.engine import Engine
        _cache["eng"] = Engine("n", "detect", synth_weights("n", "detect", 0), DEV, "x3")
    return _cache["eng"].rt


def image(h, w):
    return np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def reference(img, geo, bgr=True):
    """oracle/letterbox.py's preprocess of one image with the geometry given."""
    uh, uw, t, b, l, r = geo
    out = np.full((uh + t + b, uw + l + r, 3), 114, np.uint8)
    out[t:t + uh, l:l + uw] = img if img.shape[:2] == (uh, uw) else olb.resize_linear_u8(img, uh, uw)
    x = (out[..., ::-1] if bgr else out).transpose(2, 0, 1)
    return torch.from_numpy(np.ascontiguousarray(x).astype(np.float32) / np.float32(255))[None]


def gpu(frames, imgsz, **kw):
    return letterbox_frames(runtime(), frames, DEV, imgsz, 32, torch.cuda.current_stream(DEV).cuda_stream, **kw)[0].cpu()


@pytest.mark.parametrize("h,w,imgsz,geo", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}" + ("-geo%d" % i if c[3] else "")
                                                      for i, c in enumerate(CASES)])
def test_equals_oracle(h, w, imgsz, geo):
    img = image(h, w)
    got = gpu([torch.from_numpy(img).to(DEV)], imgsz, geo=[geo] if geo else None)
    ref = reference(img, geo) if geo else torch.from_numpy(olb.preprocess([img], imgsz))
    assert got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize("geo", [None, (40, 53, 12, 12, 5, 6)], ids=["resized", "identity"])
def test_column_slice_of_a_wider_tensor(geo):
    """Rows 303 bytes apart and a first byte 15 past a 16-byte boundary: the staging's aligned loads and its two ends."""
    wide = torch.from_numpy(image(40, 101)).to(DEV)
    frame = wide[:, 5:58]
    assert frame.data_ptr() % 16 == 15 and frame.stride(0) == 303
    img = frame.cpu().numpy()
    ref = reference(img, geo) if geo else torch.from_numpy(olb.preprocess([img], 64))
    assert torch.equal(gpu([frame], 64, geo=[geo] if geo else None), ref)


@pytest.mark.parametrize("bgr", [True, False])
def test_three_shapes_in_one_launch(bgr):
    imgs = [image(37, 53), image(120, 90), image(64, 64)]
    ref = torch.from_numpy(olb.preprocess(imgs, 64))
    got = gpu([torch.from_numpy(im).to(DEV) for im in imgs], 64, bgr=bgr)
    assert got.shape == (3, 3, 64, 64) and torch.equal(got, ref if bgr else ref.flip(1))


@pytest.mark.parametrize("task", ["detect", "segment"])
def test_frame_sources_equal_ndarray_sources(task):
    from core.model import YOLO11Model
    m = YOLO11Model(task=task, size="n", device="cuda:0", verbose=False)
    m.model.engine.autotune = False
    imgs = [(uniform(8400 + i, 120 * 160 * 3) * 256).astype(np.uint8).reshape(120, 160, 3) for i in range(2)]
    frames = torch.from_numpy(np.stack(imgs)).to(DEV)
    got, ref = m.predict(frames, imgsz=160, conf=0.1), m.predict(imgs, imgsz=160, conf=0.1)
    listed = m.predict(list(frames.unbind(0)), imgsz=160, conf=0.1)
    for g, r, l, im in zip(got, ref, listed, imgs):
        assert g.orig_shape == r.orig_shape == (120, 160) and np.array_equal(g.orig_img, im)
        assert len(g) == len(r) and torch.equal(g.boxes.data, r.boxes.data) and torch.equal(l.boxes.data, r.boxes.data)
        if task == "segment":
            assert torch.equal(g.masks.data, r.masks.data)
    if task == "detect":
        assert sum(len(r) for r in ref) > 0
        # image b is stream b; the first call of each run starts over.  The rows hold the ids (column 4)
        runs = [[[r.boxes.data.cpu() for r in m.track(src, imgsz=160, persist=step > 0)] for step in range(3)]
                for src in (frames, imgs)]
        for a, b in zip(*runs):
            assert len(a) == len(b) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
    with pytest.raises(TypeError):
        m.predict(torch.zeros((2, 3, 128, 160), dtype=torch.uint8, device=DEV))
    with pytest.raises(ValueError, match="model's device"):
        m.predict(frames.cpu())
