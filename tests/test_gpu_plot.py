"""GPU tests of the annotator (csrc/ym_annot.hip through Engine.annotate and Results.plot).

Bar: exact equality with the numpy oracle (tests/plot_oracle.py), pixel for pixel and byte for byte — the drawing rules
are integer, the blend is fp32 with every operation rounded on its own, so there is nothing to tolerate.  The scripted
scenes (tests/plot_scenes.py) are batches of two images with different counts on canvases that are no multiple of the
64 x 16 tile; the end-to-end tests run synthetic-weight yolo11n models at 128 x 160."""
import numpy as np
import pytest
import torch

from tests import plot_oracle as O
from tests import plot_scenes as S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_cache = {}
TRACKER = {"track_high_thresh": 0.02, "track_low_thresh": 0.01, "new_track_thresh": 0.02}  # synthetic scores are low


def bare_engine():
    """An Engine around an empty context: the annotator reads rows, not a model."""
    from yolomi.engine import Engine
    from yolomi.lib import Runtime
    if "bare" not in _cache:
        e = Engine.__new__(Engine)
        e.device, e.task, e.kpt_shape = DEV, "detect", None
        e.rt, e.names, e._annot_tables = Runtime(0, None), dict(S.NAMES), None
        _cache["bare"] = e
    return _cache["bare"]


def model(task):
    from core.model import YOLO11Model
    if task not in _cache:
        m = YOLO11Model(task=task, size="n", device="cuda:0", dtype="x3", verbose=False)
        m.model.engine.autotune = False
        _cache[task] = m
    return _cache[task]


def batch(seed=3, B=2, H=128, W=160):
    from yolomi.synth import uniform
    return torch.from_numpy(uniform(seed, B * 3 * H * W).astype(np.float32).reshape(B, 3, H, W)).to(DEV)


def same(got, want, what):
    got = np.asarray(got)
    assert got.shape == want.shape and got.dtype == np.uint8, (what, got.shape, want.shape)
    diff = np.argwhere((got != want).any(-1))
    assert not len(diff), (what, len(diff), diff[:5].tolist())


_SCENES = {(hw, s["name"]): s for hw in S.SIZES for s in S.scenes(*hw)}


@pytest.mark.parametrize("hw,name", sorted(_SCENES), ids=lambda v: v if isinstance(v, str) else f"{v[0]}x{v[1]}")
def test_kernel_equals_oracle(hw, name):
    s = _SCENES[(hw, name)]
    e = bare_engine()
    arrays = S.batch_arrays(s)
    frames, dets, counts, masks, geo = [torch.from_numpy(a).to(DEV) if a is not None else None for a in arrays]
    o = dict(s["opts"])
    out = e.annotate(frames, dets, counts, masks=masks, mask_geo=geo, tracked=s["tracked"],
                     kpt_shape=s["kpt_shape"] or (0, 0), line_width=o.pop("line_width_", None),
                     clip_kpts=o.pop("clip_kpts", False), **o)
    got = out.cpu().numpy()
    for b in range(2):
        same(got[b], S.oracle_image(s, b, arrays), (name, b))
    if int(arrays[2][1]) == 0:  # nothing of image 0 shows in an empty image 1
        base = arrays[0][1] if s["u8"] else O.canvas_from_tensor(arrays[0][1])
        same(got[1], base, (name, "image 1 is its canvas"))


def test_packed_masks_and_out_buffer():
    """The packed mask form (byte offsets + planes per image, image 1's planes stored first) and a caller's output
    tensor, against the slot form."""
    s = _SCENES[(S.SIZES[0], "masks_identity")]
    e = bare_engine()
    arrays = S.batch_arrays(s)
    frames, dets, counts, masks, _ = [torch.from_numpy(a).to(DEV) if a is not None else None for a in arrays]
    ref = e.annotate(frames, dets, counts, masks=masks, clip_kpts=False)
    cap, mh, mw = masks.shape[1:]
    packed = torch.cat([masks[1], masks[0]]).contiguous()  # (2 * cap, mh, mw)
    offs = torch.tensor([cap * mh * mw, 0], dtype=torch.int64, device=DEV)
    out = torch.zeros_like(ref)
    got = e.annotate(frames, dets, counts, masks=packed, mask_offsets=offs, mask_cap=cap, out=out, clip_kpts=False)
    assert got is out and torch.equal(out, ref)
    for b in range(2):
        same(out[b].cpu().numpy(), S.oracle_image(s, b, arrays), b)


# ------------------------------------------------------------------------------------------------ end to end
@pytest.mark.parametrize("task", ["detect", "segment", "pose"])
def test_predict_plot_equals_oracle(task):
    m = model(task)
    x = batch()
    res = m.predict(x, conf=0.01, max_det=12)
    assert sum(len(r) for r in res) > 0
    for b, r in enumerate(res):
        rows = r.boxes.data.clone()
        img0 = r.orig_img.copy()
        got = r.plot()
        same(got, O.paint_results(r), (task, b))
        assert got.shape == (128, 160, 3) and np.array_equal(r.orig_img, img0) and torch.equal(r.boxes.data, rows)
    r = res[0]
    same(r.plot(labels=False, line_width=3, kpt_radius=2), O.paint_results(r, labels=False, line_width_=3, kpt_radius=2),
         (task, "switches"))
    canvas = np.full((128, 160, 3), 200, np.uint8)
    want = O.paint_results(type("R", (), dict(boxes=r.boxes, keypoints=r.keypoints, masks=r.masks, names=r.names,
                                                orig_img=canvas, orig_shape=r.orig_shape, _mask_geo=None))())
    same(r.plot(img=canvas), want, (task, "img="))


@pytest.mark.parametrize("task", ["detect", "pose"])
def test_track_labels_carry_ids(task):
    m = model(task)
    x = batch(5)
    res = m.track(x, conf=0.01, max_det=12, tracker=TRACKER)
    assert sum(len(r) for r in res) > 0 and res[0].boxes.is_track
    for b, r in enumerate(res):
        got = r.plot()
        same(got, O.paint_results(r), (task, b))
        if len(r):
            untracked = O.paint(r.orig_img, r.boxes.data[:, [0, 1, 2, 3, 5, 6]].cpu().numpy(), r.names)
            assert (got != untracked).any()  # the id is in the picture


@pytest.mark.parametrize("task", ["detect", "pose"])
def test_plot_of_an_empty_image(task):
    """conf above every score: no detection (a pose Results then holds (0, 17, 3) keypoints).  plot() is the canvas,
    untracked and tracked, and again on the next frame of the stream."""
    m = model(task)
    x = batch(9)
    for res in (m.predict(x, conf=0.9999), m.track(x, conf=0.9999), m.track(x, conf=0.9999, persist=True)):
        for b, r in enumerate(res):
            assert len(r) == 0 and (task != "pose" or tuple(r.keypoints.data.shape) == (0, 17, 3))
            got = r.plot()
            same(got, r.orig_img, (task, b))
            same(got, O.paint_results(r), (task, b, "oracle"))


@pytest.mark.parametrize("task", ["detect", "pose"])
def test_batch_annotate_equals_stacked_plots(task):
    m = model(task)
    eng = m.model.engine
    x = batch(7)
    res = m.predict(x, conf=0.01, max_det=12)
    dets, cnt = eng.rows_buffer(2, 12)
    eng.run(x, conf=0.01, max_det=12, dets_out=dets, counts_after=True)
    out = eng.annotate(x, dets, cnt)
    assert out.is_cuda and tuple(out.shape) == (2, 128, 160, 3)
    stack = np.stack([r.plot() for r in res])
    assert sum(len(r) for r in res) > 0
    same(out.cpu().numpy().reshape(-1, 160, 3), stack.reshape(-1, 160, 3), task)
    tr, tcnt, _ = eng.track(x, None, persist=False, conf=0.01, max_det=12)  # track's 7-column rows as they are
    tres = m.track(x, conf=0.01, max_det=12)
    tout = eng.annotate(x, tr, tcnt, tracked=True)
    same(tout.cpu().numpy().reshape(-1, 160, 3), np.stack([r.plot() for r in tres]).reshape(-1, 160, 3), (task, "tracked"))


def test_segment_batch_annotate_equals_oracle():
    m = model("segment")
    eng = m.model.engine
    x = batch(7)
    out = torch.empty((2, 12, 6 + eng.nm), dtype=torch.float32, device=DEV)
    dets, counts = eng.run(x, conf=0.01, max_det=12, dets_out=out)
    slots, _ = eng.masks_slots(out, counts[:2], 8, 128, 160)  # 8 mask slots for up to 12 rows: rows 8.. have no mask
    img = eng.annotate(x, out, counts[:2].contiguous(), masks=slots).cpu().numpy()
    n = counts[:2].tolist()
    assert max(n) > 0
    for b in range(2):
        want = O.paint(O.canvas_from_tensor(x[b].cpu().numpy()), out[b, :n[b]].cpu().numpy(), eng.names,
                       masks=slots[b, :min(n[b], 8)].cpu().numpy())
        same(img[b], want, b)


@pytest.mark.parametrize("retina", [False, True])
def test_image_source_segment(retina):
    m = model("segment")
    rng = np.random.default_rng(11)
    image = rng.integers(0, 256, (100, 150, 3), dtype=np.uint8)
    (r,) = m.predict(image, conf=0.01, max_det=12, imgsz=160, retina_masks=retina)
    assert len(r) > 0 and r.masks is not None and r.orig_shape == (100, 150)
    if retina:
        assert tuple(r.masks.data.shape[1:]) == (100, 150) and r._mask_geo is None
    else:
        assert tuple(r.masks.data.shape[1:]) != (100, 150) and r._mask_geo is not None
    got = r.plot()
    same(got, O.paint_results(r), retina)
    assert np.array_equal(r.orig_img, image)


def test_save_round_trips(tmp_path):
    from PIL import Image
    (r, _) = model("detect").predict(batch(), conf=0.01, max_det=12)
    p = tmp_path / "out.png"
    assert r.save(str(p)) == str(p)
    back = np.asarray(Image.open(p).convert("RGB"))
    same(back[..., ::-1], r.plot(), "save")
    q = tmp_path / "plot.png"
    r.plot(save=True, filename=str(q), conf=False)
    same(np.asarray(Image.open(q).convert("RGB"))[..., ::-1], r.plot(conf=False), "plot(save=True)")


def test_draw_detections_and_handbuilt_results():
    from core.results import Results
    from utils.visualization import draw_detections
    eng = model("detect").model.engine
    image = np.random.default_rng(2).integers(0, 256, (50, 90, 3), dtype=np.uint8)
    boxes = torch.tensor([[5.5, 20.5, 40.5, 45.5, 0.625, 2.0], [30.0, 22.0, 88.0, 48.0, 0.875, 7.0]])
    r = Results.from_image(image, "a.jpg", {2: "car", 7: "truck"}, boxes, annotator=eng)
    same(r.plot(), O.paint(image, boxes.numpy(), r.names), "hand-built")
    same(draw_detections(image, r, {2: "auto", 7: "lorry"}, line_thickness=3),
         O.paint(image, boxes.numpy(), {2: "auto", 7: "lorry"}, line_width_=3), "draw_detections")
    assert r.names == {2: "car", 7: "truck"}


# ------------------------------------------------------------------------------------------------ the C-ABI's refusals
def test_abi_refusals():
    from yolomi.lib import Runtime, YMError
    e = bare_engine()
    from yolomi.annotate import _tables
    font = _tables(e)[0]
    frames = torch.zeros((1, 3, 32, 32), device=DEV)
    dets, counts = torch.zeros((1, 4, 6), device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)
    out = torch.zeros((1, 32, 32, 3), dtype=torch.uint8, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream

    def call(B=1, out_ptr=None, stride=6, K=0, nd=0, tracked=0, lw=2, font_ptr=None, flags=31):
        a = Runtime.annotate_args(lw, 5, flags, 0, tracked, stride, K, nd, 0, 0, font.data_ptr() if font_ptr is None else font_ptr)
        e.rt.annotate(frames.data_ptr(), True, B, 32, 32, dets.data_ptr(), 4, counts.data_ptr(), 0, 0, 0, 0, 0, 0, a,
                      out.data_ptr() if out_ptr is None else out_ptr, st)
    call()  # the well-formed call goes through
    for kw in (dict(out_ptr=0), dict(B=0), dict(stride=6 + 50, K=17, nd=3), dict(stride=6, tracked=1), dict(lw=0),
               dict(font_ptr=0), dict(flags=64), dict(stride=40, K=17, nd=1)):
        with pytest.raises(YMError, match="EINVAL"):
            call(**kw)
    torch.cuda.synchronize()
    assert int(out.sum()) == 0  # black frames, no rows: the one good call wrote zeros
