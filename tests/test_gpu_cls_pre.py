"""GPU tests of the classify preprocessing kernel (csrc/ym_cls_pre.hip through yolomi.preprocess.classify_batch_gpu):
every byte against Pillow's own resize, crop and /255 (yolomi.preprocess.classify_batch), which the kernel restates."""
import numpy as np
import pytest
import torch

from yolomi.preprocess import classify_batch, classify_batch_gpu, classify_desc
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
# (h, w, imgsz, constant): both passes skipped; the same with a crop 32 columns in; and 118 rows down (a short side
# equal to imgsz leaves the long side as it is); up-scaling (3 taps, both edges clamped); one source row; 5 taps,
# fractional scale, left = 6; its transpose; a window 1016 rows from the origin; scale 12.5, 27 taps (several chunks of
# staged rows); the real size; imgsz no multiple of 64; coefficient sums and clip8 on a constant 255 image
CASES = [(32, 32, 32, None), (32, 95, 32, None), (300, 64, 64, None), (17, 23, 32, None), (1, 7, 32, None),
         (33, 47, 32, None), (47, 33, 32, None), (2000, 31, 32, None), (400, 700, 32, None), (500, 375, 224, None),
         (97, 1201, 96, None), (400, 700, 32, 255)]
_cache = {}


def runtime():
    if "eng" not in _cache:
        from yolomi.engine import Engine
        _cache["eng"] = Engine("n", "classify", synth_weights("n", "classify", 0, nc=37), DEV, "x3", nc=37)
    return _cache["eng"].rt


def image(h, w, const=None):
    if const is not None:
        return np.full((h, w, 3), const, dtype=np.uint8)
    return np.random.default_rng(h * 10007 + w).integers(0, 256, (h, w, 3), dtype=np.uint8)


def gpu(imgs, imgsz):
    return classify_batch_gpu(runtime(), imgs, DEV, imgsz, torch.cuda.current_stream(DEV).cuda_stream).cpu()


@pytest.mark.parametrize("h,w,imgsz,const", CASES, ids=[f"{c[0]}x{c[1]}-{c[2]}" + ("-const" if c[3] else "") for c in CASES])
def test_equals_pillow(h, w, imgsz, const):
    im = image(h, w, const)
    assert torch.equal(gpu([im], imgsz), classify_batch([im], imgsz))


def test_mixed_batch():
    imgs = [image(h, w) for h, w in ((33, 47), (2000, 31), (32, 32), (400, 700), (17, 23))]
    got = gpu(imgs, 32)
    assert torch.equal(got, classify_batch(imgs, 32))
    for i, im in enumerate(imgs):  # every slot is its single-image result: descriptor table and packing offsets
        assert torch.equal(got[i], gpu([im], 32)[0])


def test_predict_end_to_end(monkeypatch):
    from core.model import YOLO11Model
    m = YOLO11Model(state_dict=synth_weights("n", "classify", 0, nc=37), device="cuda:0", verbose=False)
    m.model.engine.autotune = False
    imgs = [image(120, 90), image(75, 200)]
    got = torch.stack([r.probs.data for r in m.predict(imgs, imgsz=64)]).cpu()
    ref = m.model.engine.classify(classify_batch(imgs, 64).to(DEV))[0].cpu()
    monkeypatch.setenv("YM_CLS_PRE", "host")
    host = torch.stack([r.probs.data for r in m.predict(imgs, imgsz=64)]).cpu()
    assert got.shape == (2, 37) and torch.equal(got, ref) and torch.equal(got, host)


def raw(im, imgsz=32, null=False, **fields):
    """ym_classify_pre on one image with classify_desc's descriptor, `fields` overridden."""
    desc, _ = classify_desc([im.shape[:2]], imgsz if imgsz % 32 == 0 else 32)
    for k, v in fields.items():
        desc[k] = v
    src, dd = torch.from_numpy(im).to(DEV), torch.from_numpy(desc.view(np.uint8)).to(DEV)
    dst = torch.empty((1, 3, imgsz, imgsz), dtype=torch.float32, device=DEV)
    runtime().classify_pre(0 if null else src.data_ptr(), dd.data_ptr(), desc.ctypes.data, 1, imgsz, dst.data_ptr(),
                           torch.cuda.current_stream(DEV).cuda_stream)
    return dst.cpu()


@pytest.mark.parametrize("h,w,rh,rw", [(40, 100, 40, 50), (100, 40, 50, 40)], ids=["horizontal", "vertical"])
def test_single_pass(h, w, rh, rw):
    """One pass alone (classify_geometry never asks for it: the entry's own geometry), against Pillow's resize."""
    from PIL import Image
    im = image(h, w)
    pil = Image.fromarray(np.ascontiguousarray(im[..., ::-1])).resize((rw, rh), Image.BILINEAR)
    ref = np.asarray(pil)[4:36, 5:37].transpose(2, 0, 1).astype(np.float32) / np.float32(255.0)
    assert torch.equal(raw(im, rh=rh, rw=rw, top=4, left=5)[0], torch.from_numpy(ref))


def test_refusals():
    from yolomi.lib import YMError
    im = image(64, 64)
    raw(im)  # the descriptor itself is accepted
    for words, kw in (("null pointer", dict(null=True)), ("multiple of 32", dict(imgsz=48)),
                      ("row_bytes", dict(row_bytes=3 * 64 - 1)), ("crop window", dict(top=1))):
        with pytest.raises(YMError, match=words):
            raw(im, **kw)
