"""GPU tests of the NV12 letterbox (csrc/ym_letterbox_nv12.hip through yolomi.preprocess.letterbox_nv12, NV12Frames
sources of YOLO11Model and ym_nv12_to_bgr): the fp32 bits of oracle/letterbox.py on the frame converted by the integer
rule of include/yolomi.h, restated here in int64."""
import numpy as np
import pytest
import torch

from oracle import letterbox as olb
from yolomi.lib import YMError
from yolomi.preprocess import NV12Frames, letterbox_nv12, nv12_coefficients, nv12_desc
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# (h, w, imgsz, geo): geo None = the predictor's own geometry, else (uh, uw, top, bottom, left, right).  The tile is
# 64 x 16 and reads at most 32 luma rows, staged in 14 KiB chunks unless a luma row segment exceeds 1 KiB.
CASES = [
    (46, 70, 96, (59, 89, 18, 19, 3, 4)),     # odd upscale, borders on four sides, windows from odd source rows / columns
    (96, 128, 128, None),                     # uh == h, uw == w: convert only
    (480, 854, 320, None),                    # 2.7-fold: row pairs, several tiles per axis
    (240, 426, 320, None),                    # 1.3-fold: the dense row span
    (50, 70, 96, (17, 65, 0, 15, 0, 31)),     # the window ends one past the tile's edge, both axes
    (50, 70, 64, (15, 63, 1, 16, 0, 1)),      # ... and one short of it
    (1400, 1400, 64, None),                   # 21.9-fold on both axes: the taps are gathered, not staged
    (1000, 1000, 64, None),                   # 15.6-fold, pitch 1008 of 1024: row pairs staged in five chunks
    (20, 520, 64, (16, 64, 8, 8, 0, 0)),      # the dense span in two chunks that share a chroma row
]
_cache = {}


def runtime():
    if "eng" not in _cache:
        from yolomi.engine import Engine
        _cache["eng"] = Engine("n", "detect", synth_weights("n", "detect", 0), DEV, "x3")
    return _cache["eng"].rt


def surface(h, w):
    """(y, uv) device views carved from one buffer of seeded random bytes: y_pitch = w + 37, y based 15 bytes past a
    16-byte boundary, uv_pitch = w + 6, uv based 2 bytes past one; the bytes around and between the rows are random too, so
    a read of one would change the result."""
    yp, cp, y0 = w + 37, w + 6, 64 + 15
    c0 = (y0 + h * yp + 64) // 16 * 16 + 2
    buf = torch.from_numpy(np.random.default_rng(h * 10007 + w).integers(0, 256, c0 + h // 2 * cp + 64, dtype=np.uint8))
    buf = buf.to(DEV)
    y, uv = buf.as_strided((h, w), (yp, 1), y0), buf.as_strided((h // 2, w // 2, 2), (cp, 2, 1), c0)
    assert y.data_ptr() % 16 == 15 and uv.data_ptr() % 16 == 2
    return y, uv


def bgr_u8(y, uv, coef):
    """The normative conversion (include/yolomi.h) of numpy planes, in int64."""
    y_off, cy, cub, cug, cvg, cvr = coef
    u, v = (np.repeat(np.repeat(uv[..., k], 2, 0), 2, 1).astype(np.int64) - 128 for k in (0, 1))
    yy = np.maximum(0, y.astype(np.int64) - y_off) * cy + (1 << 19)
    return np.clip(np.stack([yy + cub * u, yy + cvg * v + cug * u, yy + cvr * v], -1) >> 20, 0, 255).astype(np.uint8)


def reference(img, geo):
    uh, uw, t, b, l, r = geo
    out = np.full((uh + t + b, uw + l + r, 3), 114, np.uint8)
    out[t:t + uh, l:l + uw] = img if img.shape[:2] == (uh, uw) else olb.resize_linear_u8(img, uh, uw)
    return torch.from_numpy(np.ascontiguousarray(out[..., ::-1].transpose(2, 0, 1)).astype(np.float32) / np.float32(255))[None]


def gpu(frames, imgsz, **kw):
    return letterbox_nv12(runtime(), frames, DEV, imgsz, 32, torch.cuda.current_stream(DEV).cuda_stream, **kw)[0].cpu()


@pytest.mark.parametrize("h,w,imgsz,geo", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}" + ("-geo%d" % i if c[3] else "")
                                                      for i, c in enumerate(CASES)])
def test_equals_oracle(h, w, imgsz, geo):
    y, uv = surface(h, w)
    img = bgr_u8(y.cpu().numpy(), uv.cpu().numpy(), nv12_coefficients())
    got = gpu(NV12Frames([y], [uv]), imgsz, geo=[geo] if geo else None)
    ref = reference(img, geo) if geo else torch.from_numpy(olb.preprocess([img], imgsz))
    assert got.shape == ref.shape and torch.equal(got, ref)


@pytest.mark.parametrize("standard,full", [("bt601", False), ("bt709", False), ("bt601", True), ("bt709", True)])
def test_three_shapes_in_one_launch_and_to_bgr(standard, full):
    planes = [surface(46, 70), surface(120, 90), surface(64, 64)]
    coef = nv12_coefficients(standard, full)
    imgs = [bgr_u8(y.cpu().numpy(), uv.cpu().numpy(), coef) for y, uv in planes]
    frames = NV12Frames([p[0] for p in planes], [p[1] for p in planes], standard, full)
    got = gpu(frames, 64)
    assert got.shape == (3, 3, 64, 64) and torch.equal(got, torch.from_numpy(olb.preprocess(imgs, 64)))
    for i, im in enumerate(imgs):  # ym_nv12_to_bgr on the same pitched planes
        assert np.array_equal(frames.image(runtime(), i).to_bgr(), im)


@pytest.mark.parametrize("field,value", [("w", 69), ("y_pitch", 68), ("uv", 0), ("cy", 0)])
def test_refused_before_any_launch(field, value):
    rt, (y, uv) = runtime(), surface(46, 70)
    frames, coef = NV12Frames([y], [uv]), list(nv12_coefficients())
    desc = nv12_desc(frames, [(59, 89, 18, 19, 3, 4)])
    if field == "cy":
        coef[1] = value
    else:
        desc[0][field] = value
        if field == "w":
            desc[0]["scale_x"] = 1.0 / (89 / 69)
    out = torch.full((1, 3, 96, 96), -1.0, device=DEV)
    dtab = torch.from_numpy(desc.view(np.uint8)).to(DEV)
    with pytest.raises(YMError, match="EINVAL"):
        rt.letterbox_nv12(dtab.data_ptr(), desc.ctypes.data, 1, coef, out.data_ptr(), 96, 96, 0)
    if field != "uv":
        with pytest.raises(YMError, match="EINVAL"):
            rt.nv12_to_bgr(y.data_ptr(), uv.data_ptr(), 46, int(desc[0]["w"]), int(desc[0]["y_pitch"]), 76, coef,
                           out.data_ptr(), 3 * 70, 0)
    torch.cuda.synchronize(DEV)
    assert bool((out == -1).all())


@pytest.mark.parametrize("task", ["detect", "segment"])
def test_nv12_sources_equal_ndarray_sources(task):
    from core.model import YOLO11Model
    m = YOLO11Model(task=task, size="n", device="cuda:0", verbose=False)
    m.model.engine.autotune = False
    surf = torch.from_numpy(np.random.default_rng(8400).integers(0, 256, (2, 180, 160), dtype=np.uint8))
    imgs = [bgr_u8(s[:120], s[120:].reshape(60, 80, 2), nv12_coefficients()) for s in surf.numpy()]
    dsurf = surf.to(DEV)
    frames = NV12Frames.from_surface(dsurf)
    got, ref = m.predict(frames, imgsz=160, conf=0.1), m.predict(imgs, imgsz=160, conf=0.1)
    dsurf.zero_()  # the call kept clones of the planes: the decoder may reuse its surface
    for g, r, im in zip(got, ref, imgs):
        assert g.orig_shape == r.orig_shape == (120, 160) and np.array_equal(g.orig_img, im)
        assert len(g) == len(r) and torch.equal(g.boxes.data, r.boxes.data)
        if task == "segment":
            assert torch.equal(g.masks.data, r.masks.data)
    if task == "detect":
        assert sum(len(r) for r in ref) > 0
        frames = NV12Frames.from_surface(surf.to(DEV))
        runs = [[[r.boxes.data.cpu() for r in m.track(src, imgsz=160, persist=step > 0)] for step in range(3)]
                for src in (frames, imgs)]
        for a, b in zip(*runs):
            assert len(a) == len(b) == 2 and all(torch.equal(x, y) for x, y in zip(a, b))
