"""retina_masks=True on the GPU (MI355X): csrc/ym_mask_native.hip through ym_masks_native, Engine.masks_native and
YOLO11Model.predict, against the float64 restatement of ops.process_mask_native (tests/retina_oracle.py).

Bars.  Kernel parity is per mask: every pixel outside the box's integer range is 0 exactly; inside it at most
max(2, 0.001 * in-box pixels) pixels disagree with the float64 restatement — 0.001 is the project's mask bar (SURVEY
§8c, test_segment_masks_match_oracle) applied to the box's own pixels, the floor of 2 is there because one flipped
pixel is what upstream's own fp32 arithmetic shows against float64 (tests/test_retina_host.py).  predict() against the
oracle: >= 0.999 pixel agreement on matched detections, matched as test_segment_masks_match_oracle matches them.
"""
import os

import numpy as np
import pytest
import torch

from oracle.predict import OracleModel
from tests import retina_oracle as ro
from tests.golden.make_golden import make_input
from yolomi.lib import YMError
from yolomi.preprocess import scale_boxes
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NET = (320, 320)
SHAPES = [(320, 320), (240, 427), (500, 333), (97, 61)]  # identity, wide up-scale (odd width), tall up-scale, down-scale

_cache = {}


def oracle():
    if "o" not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _cache["o"] = OracleModel("n", "segment", synth_weights("n", "segment", 0))
    return _cache["o"]


def model(dtype="f32", task="segment"):
    from core.model import YOLO11Model
    k = ("m", dtype, task)
    if k not in _cache:
        _cache[k] = YOLO11Model(task=task, size="n", device="cuda:0", dtype=dtype)
    return _cache[k]


def the_input():
    return make_input("uniform", (81, 82), 320)


def gpu_rows(dtype="f32"):
    """engine.run at conf 0.25: (engine, a copy of its rows (2, 300, 38), the counts, its prototypes (2, 80, 80, 32) on
    the CPU).  Run afresh by every test that calls masks_native, which must follow a forward of the same shape."""
    eng = model(dtype).model.engine
    dets, counts = eng.run(the_input().to(DEV), conf=0.25)
    n = counts[:2].tolist()
    rows = dets[:2].clone()
    proto = eng.read_buffer(eng.graph.proto_buf.id, 2)
    assert min(n) > 0 and tuple(proto.shape) == (2, 80, 80, 32)
    return eng, rows, n, proto


def unpack(packed, boffs, counts, shapes):
    """The packed buffer as one (n_b, h0, w0) uint8 CPU tensor per image."""
    p = packed.cpu()
    return [p[boffs[b]:boffs[b + 1]].view(counts[b], *shapes[b]) for b in range(len(counts))]


def compare(g, flags, rows, proto_b, shape):
    """One image: GPU masks g (n, h0, w0) and flags (n,) vs the float64 restatement on the same rows (n, >= 38, boxes in
    native pixels) and prototypes (mh, mw, 32)."""
    rows = rows.cpu().double()
    ref = ro.process_mask_native(proto_b.permute(2, 0, 1).double(), rows[:, 6:38], rows[:, :4], shape)
    assert tuple(g.shape) == tuple(ref.shape)
    worst = 0.0
    for i in range(len(rows)):
        x0, x1, y0, y1 = ro.box_range(rows[i, :4].tolist(), shape)
        inside = torch.zeros(shape, dtype=torch.bool)
        inside[y0:y1, x0:x1] = True
        gi = g[i].bool()
        assert set(g[i].unique().tolist()) <= {0, 1}
        assert not bool(gi[~inside].any()), (i, "pixels set outside the box")
        bad, npx = int((gi != ref[i])[inside].sum()), int(inside.sum())
        worst = max(worst, bad / max(npx, 1))
        assert bad <= max(2, 0.001 * npx), (i, bad, npx)
        assert int(flags[i]) == int(bool(gi.any())), (i, "flag and mask disagree")
        if int(ref[i].sum()) > 2:
            assert int(flags[i]) == 1, i
    return worst


# ------------------------------------------------------------------------------------------------ 1. kernel parity
@pytest.mark.parametrize("shapes", [(s, s) for s in SHAPES] + [((240, 427), (97, 61)), ((7, 5), (1, 1))], ids=str)
def test_kernel_matches_float64_restatement(shapes):
    """The four shapes, each for both images; a batch that mixes two of them (per-image offsets); and rows narrower
    than one 16-byte run next to a one-pixel image (the kernel's pixel-by-pixel store path)."""
    eng, rows, n, proto = gpu_rows()
    for b in range(2):
        scale_boxes(NET, rows[b, : n[b], :4], shapes[b])
    packed, flags, offs, boffs = eng.masks_native(rows, n, *NET, shapes)
    assert offs == [0, n[0], n[0] + n[1]]
    assert boffs == [0, n[0] * shapes[0][0] * shapes[0][1], packed.numel()]
    flags = flags.cpu()
    for b, g in enumerate(unpack(packed, boffs, n, shapes)):
        worst = compare(g, flags[offs[b]:offs[b + 1]], rows[b, : n[b]], proto[b], shapes[b])
        print(f"shapes {shapes} image {b}: {n[b]} masks, worst in-box disagreement {worst:.5f}")


# ------------------------------------------------------------------------------------------------ 2. crafted rows
def test_crafted_rows():
    eng, rows, n, proto = gpu_rows()
    shape = (97, 61)
    coef = rows[0, 0, 6:].clone()
    d = torch.zeros((2, 8, rows.shape[2]), dtype=torch.float32, device=DEV)  # a row buffer of its own size
    boxes = [(100.0, 120.0, 150.0, 160.0),  # wholly outside the image
             (20.0, 30.0, 20.0, 50.0),      # zero area
             (10.0, 5.0, 20.0, 90.0),       # integer edges: column 10 eligible, column 20 not
             (10.0, 5.0, 20.0, 90.0),       # the same with negated coefficients
             (0.0, 0.0, 61.0, 97.0)]        # the whole image
    for i, bx in enumerate(boxes):
        d[0, i, :4] = torch.tensor(bx)
        d[0, i, 6:] = -coef if i == 3 else coef
    d[1, 0, :4] = torch.tensor(boxes[4])
    d[1, 0, 6:] = rows[1, 0, 6:]
    packed, flags, offs, boffs = eng.masks_native(d, [5, 1], *NET, [shape, shape])
    flags = flags.cpu().tolist()
    g0, g1 = unpack(packed, boffs, [5, 1], [shape, shape])
    assert not g0[0].any() and flags[0] == 0
    assert not g0[1].any() and flags[1] == 0
    # every in-box pixel is positive under the coefficients or under their negation (the arithmetic is odd-symmetric,
    # and an exact 0 does not occur), so the two masks tile the box exactly: its integer range is [10, 20) x [5, 90)
    both = g0[2].bool() | g0[3].bool()
    assert not bool((g0[2].bool() & g0[3].bool()).any())
    assert bool(both[5:90, 10:20].all()) and int(both.sum()) == 85 * 10
    assert bool(both[5:90, 10].all()) and not bool(both[:, 20].any())
    compare(g0, flags[:5], d[0, :5], proto[0], shape)
    compare(g1, flags[5:], d[1, :1], proto[1], shape)
    # an image with no detections: no bytes of its own, the other image's offsets and masks intact
    eng, _, _, _ = gpu_rows()
    p2, f2, offs2, boffs2 = eng.masks_native(d, [0, 1], *NET, [shape, shape])
    assert offs2 == [0, 0, 1] and boffs2 == [0, 0, 97 * 61] and p2.numel() == 97 * 61
    assert torch.equal(p2.cpu().view(1, *shape), g1) and f2.cpu().tolist() == flags[5:]
    p3, f3, offs3, boffs3 = eng.masks_native(d, [5, 0], *NET, [shape, shape])
    assert offs3 == [0, 5, 5] and boffs3 == [0, 5 * 97 * 61, 5 * 97 * 61]
    assert torch.equal(p3.cpu().view(5, *shape), g0) and f3.cpu().tolist() == flags[:5]


def test_taps_computed_per_pixel_when_the_tile_is_too_small():
    """A whole-image box at native (64, 64): its taps span the whole 80 x 80 window, 6400 values, above the kernel's
    6144-float LDS tile, so every pixel computes its own four taps; the real detections' boxes at the same shape take
    the staged path.  Both against the restatement, and a box shared by the two calls gives the same mask."""
    eng, rows, n, proto = gpu_rows()
    shape = (64, 64)
    for b in range(2):
        scale_boxes(NET, rows[b, : n[b], :4], shape)
    whole = rows.clone()
    whole[:, :, 0:2] = 0.0
    whole[:, :, 2:4] = 64.0
    for r in (whole, rows):
        packed, flags, offs, boffs = eng.masks_native(r, n, *NET, [shape, shape])
        flags = flags.cpu()
        for b, g in enumerate(unpack(packed, boffs, n, [shape, shape])):
            compare(g, flags[offs[b]:offs[b + 1]], r[b, : n[b]], proto[b], shape)
            if r is whole:
                assert int(g.sum()) > 0
                _cache[("whole", b)] = g
            else:  # the staged path's masks are the per-pixel path's, cropped to the box
                for i in range(n[b]):
                    x0, x1, y0, y1 = ro.box_range(r[b, i, :4].tolist(), shape)
                    assert torch.equal(g[i, y0:y1, x0:x1], _cache[("whole", b)][i, y0:y1, x0:x1]), (b, i)


# ------------------------------------------------------------------------------------------------ 3 / 6. predict, tensor
def _box_iou(a, b):
    lt = torch.maximum(a[:, None, :2], b[None, :, :2])
    rb = torch.minimum(a[:, None, 2:4], b[None, :, 2:4])
    inter = (rb - lt).clamp(min=0).prod(-1)
    area = lambda t: (t[:, 2] - t[:, 0]) * (t[:, 3] - t[:, 1])
    return inter / (area(a)[:, None] + area(b)[None] - inter)


def oracle_retina_ref():
    if "ref" not in _cache:
        _cache["ref"] = ro.oracle_retina(oracle(), the_input(), [NET, NET], 0.25, dtype=torch.float32)
    return _cache["ref"]


def check_predict_vs_oracle(res, agree=0.999):
    ref = oracle_retina_ref()
    total = matched = 0
    for r, g in zip(ref, res):
        rb, gb = r["boxes"], g.boxes.data.cpu()
        total += len(rb)
        if not len(rb) or not len(gb):
            continue
        iou = _box_iou(rb[:, :4], gb[:, :4])
        iou[rb[:, 5][:, None] != gb[:, 5][None, :]] = 0
        used = set()
        for i in torch.argsort(rb[:, 4], descending=True).tolist():
            j = int(torch.argmax(iou[i]))
            if iou[i, j] < 0.99 or j in used:
                continue
            used.add(j)
            matched += 1
            a = (r["masks"][i] == g.masks.data[j].cpu()).float().mean().item()
            assert a >= agree, (i, j, a)
    assert total > 0 and matched >= total - 1, (matched, total)


def check_result_shapes(res, shapes):
    for g, shape in zip(res, shapes):
        assert g.masks is not None and tuple(g.masks.data.shape) == (len(g.boxes), *shape)
        assert g.masks.data.dtype == torch.bool and tuple(g.masks.orig_shape) == tuple(shape)
        assert len(g.boxes) == len(g.masks)
        assert bool(g.masks.data.flatten(1).any(1).all())


def test_predict_tensor_source():
    """Fails without the feature: the keyword is ignored, the default masks (crop, then upsample) come back, and the
    restatement shows them up to 1.4 % away."""
    m = model()
    x = the_input().to(DEV)
    res = m.predict(x, conf=0.25, retina_masks=True)
    check_result_shapes(res, [NET, NET])
    assert sum(len(g.boxes) for g in res) > 0
    eng, rows, n, _ = gpu_rows()
    packed, flags, offs, boffs = eng.masks_native(rows, n, *NET, [NET, NET])
    flags = flags.cpu().bool()
    for b, g in enumerate(unpack(packed, boffs, n, [NET, NET])):
        keep = flags[offs[b]:offs[b + 1]]
        assert torch.equal(res[b].masks.data.cpu(), g.bool()[keep])
        assert torch.equal(res[b].boxes.data.cpu(), rows[b, : n[b], :6].cpu()[keep])
    check_predict_vs_oracle(res)


def test_predict_tensor_source_x3():
    res = model("x3").predict(the_input().to(DEV), conf=0.25, retina_masks=True)
    check_result_shapes(res, [NET, NET])
    check_predict_vs_oracle(res)


# ------------------------------------------------------------------------------------------------ 4. image sources
def test_predict_ndarray_sources():
    """Two ndarrays of different shapes in one call.  Seeded uint8 noise at imgsz 320, conf 0.9: the CPU oracle (through
    oracle/letterbox.py) keeps 7 and 4 detections on these two images, every one with a non-empty native mask."""
    rng = np.random.default_rng(0)
    imgs = [rng.integers(0, 256, (240, 427, 3), dtype=np.uint8), rng.integers(0, 256, (97, 61, 3), dtype=np.uint8)]
    res = model().predict(imgs, conf=0.9, imgsz=320, retina_masks=True)
    shapes = [im.shape[:2] for im in imgs]
    check_result_shapes(res, shapes)
    total = 0
    for g, (h0, w0) in zip(res, shapes):
        assert tuple(g.orig_shape) == (h0, w0) and len(g.boxes) > 0
        bx = g.boxes.data.cpu()
        assert bool((bx[:, [0, 2]] >= 0).all()) and bool((bx[:, [0, 2]] <= w0).all())
        assert bool((bx[:, [1, 3]] >= 0).all()) and bool((bx[:, [1, 3]] <= h0).all())
        mk = g.masks.data.cpu()
        for i in range(len(bx)):
            x0, x1, y0, y1 = ro.box_range(bx[i, :4].tolist(), (h0, w0))
            outside = torch.ones((h0, w0), dtype=torch.bool)
            outside[y0:y1, x0:x1] = False
            assert not bool(mk[i][outside].any()), i
        total += len(bx)
    assert total > 0


# ------------------------------------------------------------------------------------------------ 5. defaults
def test_defaults_unchanged():
    x = the_input().to(DEV)
    m = model()
    a, b = m.predict(x, conf=0.25), m.predict(x, conf=0.25, retina_masks=False)
    for ra, rb in zip(a, b):
        assert torch.equal(ra.boxes.data, rb.boxes.data) and torch.equal(ra.masks.data, rb.masks.data)
        assert tuple(ra.masks.data.shape[1:]) == NET
    det = model(task="detect")
    c, d = det.predict(x, conf=0.25), det.predict(x, conf=0.25, retina_masks=True)
    assert sum(len(r) for r in c) > 0
    for rc, rd in zip(c, d):
        assert torch.equal(rc.boxes.data, rd.boxes.data) and rd.masks is None


def test_no_detections():
    """A batch that keeps nothing: an empty packed buffer, and Results with (0, h0, w0) masks as on the default path."""
    x = the_input().to(DEV)
    m = model()
    for g, d in zip(m.predict(x, conf=0.999, retina_masks=True), m.predict(x, conf=0.999)):
        assert len(g.boxes) == 0 and len(d.boxes) == 0
        assert tuple(g.masks.data.shape) == tuple(d.masks.data.shape) == (0, *NET)
    eng, rows, n, _ = gpu_rows()
    packed, flags, offs, boffs = eng.masks_native(rows, [0, 0], *NET, [(97, 61), (240, 427)])
    assert packed.numel() == 0 and flags.numel() == 0 and offs == [0, 0, 0] and boffs == [0, 0, 0]


# ------------------------------------------------------------------------------------------------ 7. rejections
def test_rejections():
    x = the_input().to(DEV)
    det = model(task="detect").model.engine
    dets, counts = det.run(x, conf=0.25)
    with pytest.raises(YMError, match="ESTATE"):
        det.masks_native(dets[:2], counts[:2].tolist(), *NET, [NET, NET])
    eng, rows, n, _ = gpu_rows()
    with pytest.raises(YMError, match="EINVAL"):
        eng.masks_native(rows, n, *NET, [(0, 61), (97, 61)])
    with pytest.raises(YMError, match="EINVAL"):
        eng.masks_native(rows, n, *NET, [(97, 61), (97, 0)])
