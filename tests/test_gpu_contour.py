"""Instance polygons on the GPU (MI355X): csrc/ym_contour.hip through ym_mask_contours and Engine.mask_contours against
the sequential oracle (tests/contour_oracle.py), bit for bit — points, offsets and order — and Masks.xy / xyn, summary
and save_txt of yolo11n-seg predictions against the oracle applied to the same mask planes.  Everything here fails
without the feature: there is no ym_mask_contours and no Masks.xy."""
import numpy as np
import pytest
import torch
from scipy import ndimage

from tests.contour_oracle import contour, contour_fast, contours
from tests.golden.make_golden import make_input
from yolomi.lib import YMError
from yolomi.preprocess import scale_coords

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_cache = {}


def engine():
    """An Engine around an empty context: the tracer reads planes, not a model."""
    from yolomi.engine import Engine
    from yolomi.lib import Runtime
    if "bare" not in _cache:
        e = Engine.__new__(Engine)
        e.device, e.task, e.kpt_shape = DEV, "detect", None
        e.rt, e.contour_launches = Runtime(0, None), 0
        _cache["bare"] = e
    return _cache["bare"]


def check(planes, ref=None, **kw):
    """One call over the (n, H, W) planes: the device form's offsets and points, then the host form, against the oracle."""
    planes = np.ascontiguousarray(planes, dtype=np.uint8)
    ref = contours(planes) if ref is None else ref
    e = engine()
    t = torch.from_numpy(planes).to(DEV)
    got = e.mask_contours(t, **kw)
    assert len(got) == len(ref)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert g.dtype == np.int32 and g.shape == r.shape and np.array_equal(g, r), (i, planes[i], g, r)
    lens = [len(r) for r in ref]
    pts, offs = e.mask_contours_device(t, cap=max(sum(lens), 1))
    assert offs.dtype == torch.int64 and offs.cpu().tolist() == np.concatenate([[0], np.cumsum(lens)]).astype(int).tolist()
    if sum(lens):
        assert np.array_equal(pts[:sum(lens)].cpu().numpy(), np.concatenate(ref))
    return got


def exhaustive(h, w):
    n = h * w
    bits = (np.arange(1 << n)[:, None] >> np.arange(n)[None, :]) & 1
    return bits.astype(np.uint8).reshape(-1, h, w)


def spiral(n=64):
    """A one-pixel-wide spiral filling n x n: walk inwards, turning when the cell two ahead is taken."""
    m = np.zeros((n, n), dtype=np.uint8)
    x = y = 0
    dx, dy = 1, 0
    m[0, 0] = 1
    for _ in range(n * n):
        nx, ny = x + dx, y + dy
        ax, ay = nx + dx, ny + dy
        ahead_free = not (0 <= ax < n and 0 <= ay < n) or m[ay, ax] == 0
        if 0 <= nx < n and 0 <= ny < n and m[ny, nx] == 0 and ahead_free:
            x, y = nx, ny
            m[y, x] = 1
            continue
        dx, dy = -dy, dx  # turn right on screen
        nx, ny = x + dx, y + dy
        ax, ay = nx + dx, ny + dy
        if not (0 <= nx < n and 0 <= ny < n) or m[ny, nx] or (0 <= ax < n and 0 <= ay < n and m[ay, ax]):
            break
        x, y = nx, ny
        m[y, x] = 1
    return m


def blobs(h, w, seed, sigma=2.0):
    rng = np.random.default_rng(seed)
    return (ndimage.gaussian_filter(rng.random((h, w)), sigma) > 0.5).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ kernel against oracle
@pytest.mark.parametrize("shape", [(3, 4), (4, 3)], ids=str)
def test_every_small_plane(shape):
    check(exhaustive(*shape))  # 4,096 planes in one call


def test_random_5x5_planes():
    rng = np.random.default_rng(5)
    check((rng.random((20000, 5, 5)) < rng.uniform(0.2, 0.8, (20000, 1, 1))).astype(np.uint8))


@pytest.mark.parametrize("shape", [(33, 65), (37, 70), (64, 64)], ids=str)
def test_planes_across_word_boundaries(shape):
    rng = np.random.default_rng(shape[1])
    noise = [(rng.random(shape) < d).astype(np.uint8) for d in (0.3, 0.45, 0.55, 0.7)]
    planes = np.stack(noise + [blobs(*shape, seed=s, sigma=g) for s, g in ((1, 1.5), (2, 2.5), (3, 4.0))] +
                      [np.ones(shape, dtype=np.uint8), np.zeros(shape, dtype=np.uint8)])
    got = check(planes)
    assert max(len(g) for g in got) > 40


def test_thin_planes_and_no_planes():
    rng = np.random.default_rng(9)
    for shape in ((1, 1), (1, 7), (7, 1), (1, 97), (97, 1), (1, 32), (1, 33)):
        planes = (rng.random((16, *shape)) < 0.6).astype(np.uint8)
        planes[0], planes[1] = 1, 0
        check(planes)
    e = engine()
    assert e.mask_contours(torch.zeros((0, 8, 8), dtype=torch.uint8, device=DEV)) == []
    pts, offs = e.mask_contours_device(torch.zeros((0, 8, 8), dtype=torch.bool, device=DEV), cap=0)
    assert offs.cpu().tolist() == [0] and tuple(pts.shape) == (0, 2)


def comb(h=40, w=63):
    m = np.zeros((h, w), dtype=np.uint8)
    m[h - 2, 1:w - 1] = 1
    m[2:h - 2, 1:w - 1:2] = 1
    return m


def test_spiral_comb_and_mixed_lengths():
    sp = spiral()
    assert sp.sum() > 64 * 64 // 2 - 64 and ndimage.label(sp, structure=np.ones((3, 3)))[1] == 1
    ref = contour(sp)
    assert len(ref) > 100
    check(sp[None], ref=[ref])
    c = comb()
    check(np.stack([c, c[::-1].copy()]))
    dot = np.zeros((64, 64), dtype=np.uint8)
    dot[63, 63] = 1
    mixed = np.stack([np.zeros((64, 64), dtype=np.uint8), dot, sp, np.zeros((64, 64), dtype=np.uint8), sp.T.copy(), dot])
    got = check(mixed)
    assert [len(g) for g in got][:2] == [0, 1] and len(got[2]) == len(ref)


def test_overflow_returns_every_point():
    """A first capacity below the need: the offsets still give every count, nothing past the capacity is written, and
    the host form calls again with the exact size."""
    sp = spiral()
    dot = np.zeros((64, 64), dtype=np.uint8)
    dot[5, 7] = 1
    mixed = np.stack([np.zeros((64, 64), dtype=np.uint8), dot, sp, dot, sp])
    ref = contours(mixed)
    total = sum(len(r) for r in ref)
    e = engine()
    t = torch.from_numpy(mixed).to(DEV)
    n0 = e.contour_launches
    got = e.mask_contours(t, cap=16)
    assert e.contour_launches == n0 + 2
    assert all(np.array_equal(g, r) for g, r in zip(got, ref))
    guard = torch.full((40, 2), -7, dtype=torch.int32, device=DEV)
    e.rt.mask_contours(t.data_ptr(), 5, 64, 64, 64 * 64, guard.data_ptr(), 16, torch.empty(6, dtype=torch.int64, device=DEV).data_ptr(),
                       torch.cuda.current_stream(DEV).cuda_stream)
    g = guard.cpu().numpy()
    assert g[0].tolist() == [7, 5] and (g[1:] == -7).all()  # the dot fits; the spiral does not and is left out
    pts, offs = e.mask_contours_device(t, cap=16)
    assert int(offs[-1]) == total > 16
    check(mixed, ref=ref, cap=0)  # a count-only first call


def test_large_plane():
    yy, xx = np.mgrid[:640, :640]
    m = np.zeros((640, 640), dtype=np.uint8)
    for cx, cy, r in ((120, 100, 80), (400, 150, 120.5), (610, 610, 45), (300, 500, 33.3)):
        m |= ((xx - cx) ** 2 + (yy - cy) ** 2 <= r * r).astype(np.uint8)
    d = (xx - 150) ** 2 + (yy - 420) ** 2
    m |= ((d <= 140 ** 2) & (d >= 100 ** 2)).astype(np.uint8)      # a ring ...
    m |= (d <= 60 ** 2).astype(np.uint8)                            # ... with an island that would have more points
    m[400:440, 140:160] = 0
    ref = contour_fast(m)
    assert len(ref) > 200
    check(np.stack([m, m.T.copy()]), ref=[ref, contour_fast(m.T.copy())])
    big = np.zeros((2, 700, 800), dtype=np.uint8)  # past the LDS bit plane: the scratch path
    big[0, 30:670, 100:740] = m
    big[1, 5:690, 3:790] = 1
    big[1, 100:300, 100:300] = 0
    big[1, 150:250, 150:250] = blobs(100, 100, 4)
    check(big, ref=[contour_fast(big[0]), contour_fast(big[1])])


def test_plane_stride_and_bool_planes():
    rng = np.random.default_rng(2)
    slots = (rng.random((6, 3, 20, 24)) < 0.5)
    t = torch.from_numpy(slots).to(DEV)
    e = engine()
    view = t[:, 1]  # plane stride 3 * 20 * 24
    assert view.stride(0) == 3 * 20 * 24 and not view.is_contiguous()
    n0 = e.contour_launches
    got = e.mask_contours(view)
    ref = contours(slots[:, 1].astype(np.uint8))
    assert all(np.array_equal(g, r) for g, r in zip(got, ref)) and e.contour_launches == n0 + 1
    odd = torch.from_numpy((rng.random((4, 17, 29)) < 0.5)).to(DEV)[:, 1:, 3:]  # rows are not contiguous: copied
    assert all(np.array_equal(g, r) for g, r in zip(e.mask_contours(odd), contours(odd.cpu().numpy().astype(np.uint8))))
    vals = torch.from_numpy(slots[:, 0].astype(np.uint8) * 255).to(DEV)  # any non-zero byte is foreground
    assert all(np.array_equal(g, r) for g, r in zip(e.mask_contours(vals), contours(slots[:, 0].astype(np.uint8))))


def test_abi_refusals():
    e = engine()
    m = torch.ones((2, 8, 8), dtype=torch.uint8, device=DEV)
    pts = torch.empty((64, 2), dtype=torch.int32, device=DEV)
    offs = torch.empty((3,), dtype=torch.int64, device=DEV)
    st = torch.cuda.current_stream(DEV).cuda_stream

    def call(masks=m.data_ptr(), n=2, H=8, W=8, stride=64, points=pts.data_ptr(), cap=64, offsets=offs.data_ptr()):
        e.rt.mask_contours(masks, n, H, W, stride, points, cap, offsets, st)

    call()
    assert offs.cpu().tolist() == [0, 4, 8]
    for kw in (dict(masks=0), dict(points=0), dict(offsets=0), dict(H=0), dict(W=0), dict(H=-3), dict(stride=63), dict(n=-1),
               dict(cap=-1)):
        with pytest.raises(YMError, match="EINVAL"):
            call(**kw)
    call(n=0, masks=0)
    assert offs.cpu().tolist()[0] == 0
    with pytest.raises(ValueError):
        e.mask_contours(torch.ones((2, 8, 8), dtype=torch.float32, device=DEV))
    with pytest.raises(ValueError):
        e.mask_contours(torch.ones((8, 8), dtype=torch.uint8, device=DEV))


# ------------------------------------------------------------------------------------------------ end to end
def model():
    from core.model import YOLO11Model
    if "m" not in _cache:
        _cache["m"] = YOLO11Model(task="segment", size="n", device="cuda:0", dtype="f32")
    return _cache["m"]


def sources():
    rng = np.random.default_rng(0)
    return {"tensor": (lambda: make_input("uniform", (81, 82), 320).to(DEV), dict(conf=0.25)),
            "ndarray": (lambda: [rng.integers(0, 256, (240, 427, 3), dtype=np.uint8)], dict(conf=0.9, imgsz=320)),
            "retina": (lambda: make_input("uniform", (81, 82), 320).to(DEV), dict(conf=0.25, retina_masks=True))}


@pytest.mark.parametrize("kind", ["tensor", "ndarray", "retina"])
def test_predict_polygons(kind, tmp_path):
    src, kw = sources()[kind]
    m = model()
    eng = m.model.engine
    res = m.predict(src(), **kw)
    assert sum(len(r.boxes) for r in res) > 0 and all(len(r.boxes) > 0 for r in res)
    for b, r in enumerate(res):
        h0, w0 = r.orig_shape
        planes = r.masks.data.cpu().numpy().astype(np.uint8)
        if kind == "ndarray":
            assert (h0, w0) == (240, 427) and planes.shape[1:] != (h0, w0)  # letterboxed planes: scale_coords has a pad
        else:
            assert planes.shape[1:] == (h0, w0)
        n0 = eng.contour_launches
        xy = r.masks.xy
        n1 = eng.contour_launches
        assert n1 > n0 and len(xy) == len(r.boxes) == len(planes)
        ref = [scale_coords(planes.shape[1:], torch.from_numpy(c.astype(np.float32)), (h0, w0)).numpy()
               for c in (contour_fast(p) for p in planes)]
        wh = np.array([w0, h0], dtype=np.float32)
        xyn = r.masks.xyn
        for g, gn, want in zip(xy, xyn, ref):
            assert g.dtype == np.float32 and np.array_equal(g, want) and np.array_equal(gn, want / wh)
        assert max(len(p) for p in xy) >= 4
        assert r.masks.xy is xy and eng.contour_launches == n1  # cached: no second launch
        sub = r[1:3]
        assert len(sub.masks.xy) == len(ref[1:3]) and all(np.array_equal(a, c) for a, c in zip(sub.masks.xy, ref[1:3]))
        assert eng.contour_launches == n1
        summ = r.summary(normalize=True, decimals=5)
        f = tmp_path / f"{kind}{b}.txt"
        r.save_txt(f, save_conf=True)
        lines = f.read_text().splitlines()
        assert len(lines) == len(summ) == len(xy)
        for i, (line, s) in enumerate(zip(lines, summ)):
            v = line.split()
            assert int(v[0]) == int(r.boxes.cls[i]) and len(v) == 2 + xyn[i].size
            assert np.allclose([float(t) for t in v[1:-1]], xyn[i].reshape(-1), rtol=1e-5, atol=1e-6)
            assert float(v[-1]) == pytest.approx(float(r.boxes.conf[i]), rel=1e-5)
            assert np.allclose(s["segments"]["x"], xyn[i][:, 0], atol=1e-5) and np.allclose(s["segments"]["y"], xyn[i][:, 1], atol=1e-5)
        cpu = r.cpu()
        assert cpu.masks.xy is xy and eng.contour_launches == n1


def test_cpu_results_upload_once():
    m = model()
    eng = m.model.engine
    r = m.predict(make_input("uniform", (81, 82), 320).to(DEV), conf=0.25)[0]
    ref = r.masks.xy
    c = m.predict(make_input("uniform", (81, 82), 320).to(DEV), conf=0.25)[0].cpu()
    assert not c.masks.data.is_cuda
    n0 = eng.contour_launches
    got = c.masks.xy
    assert eng.contour_launches > n0 and all(np.array_equal(a, b) for a, b in zip(got, ref))
