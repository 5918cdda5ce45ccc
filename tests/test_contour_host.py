"""Host tests of the instance polygons: hand-checked answers of the sequential oracle
(tests/contour_oracle.py), properties of its borders that scipy's labelling checks independently, the host build of the
kernels' shared header (tests/contour_check.cpp: the candidate / cycle / westward rules against the oracle's floods),
and the Results surface (Masks.xy / xyn, summary, save_txt) over a stub engine."""
import os
import subprocess

import numpy as np
import pytest
import torch
from scipy import ndimage

from tests.contour_oracle import all_borders, compress, contour, contours, trace
from tests.test_plan_format import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = {(-1, 0), (-1, -1), (0, -1), (1, -1), (1, 0), (1, 1), (0, 1), (-1, 1)}


def plane(h, w, pixels=(), rects=()):
    m = np.zeros((h, w), dtype=np.uint8)
    for x0, y0, x1, y1 in rects:
        m[y0:y1 + 1, x0:x1 + 1] = 1
    for x, y in pixels:
        m[y, x] = 1
    return m


def pts(m):
    return [tuple(p) for p in contour(m).tolist()]


# ------------------------------------------------------------------------------------------------ known answers
def test_filled_rectangle():
    assert pts(plane(7, 9, rects=[(2, 1, 6, 4)])) == [(2, 1), (2, 4), (6, 4), (6, 1)]


def test_three_pixel_row():
    m = plane(3, 5, rects=[(1, 1, 3, 1)])
    assert trace(m != 0, 1, 1) == [(1, 1), (2, 1), (3, 1), (2, 1)]
    assert pts(m) == [(1, 1), (3, 1)]


def test_single_pixel():
    assert pts(plane(3, 4, [(2, 1)])) == [(2, 1)]
    assert contour(plane(3, 4, [(2, 1)])).dtype == np.int32


def test_empty_plane():
    c = contour(plane(3, 4))
    assert c.shape == (0, 2) and c.dtype == np.int32


def test_diagonal_line():
    m = plane(4, 4, [(0, 0), (1, 1), (2, 2)])
    assert trace(m != 0, 0, 0) == [(0, 0), (1, 1), (2, 2), (1, 1)]
    assert pts(m) == [(0, 0), (2, 2)]


def test_plus_is_a_diamond():
    """8-connected tracing cuts the plus's inner corners: the arm tips, counter-clockwise on screen from the top."""
    assert pts(plane(5, 5, [(2, 1), (1, 2), (2, 2), (3, 2), (2, 3)])) == [(2, 1), (1, 2), (2, 3), (3, 2)]


def test_corner_touch_is_one_component():
    m = plane(3, 3, [(0, 0), (1, 1)])
    assert len(all_borders(m)) == 1
    assert pts(m) == [(0, 0), (1, 1)]


def ring(h, w, x0, y0, x1, y1):
    m = plane(h, w, rects=[(x0, y0, x1, y1)])
    m[y0 + 1:y1, x0 + 1:x1] = 0
    return m


def test_ring_with_island():
    m = ring(7, 7, 1, 1, 5, 5)
    m[3, 3] = 1
    b = all_borders(m)
    assert len(b) == 1 and b[0][0] == (1, 1)
    assert pts(m) == [(1, 1), (1, 5), (5, 5), (5, 1)]


def test_nested_rings():
    m = ring(9, 9, 0, 0, 8, 8) | ring(9, 9, 2, 2, 6, 6)
    m[4, 4] = 1
    b = all_borders(m)
    assert len(b) == 1 and b[0][0] == (0, 0)
    assert pts(m) == [(0, 0), (0, 8), (8, 8), (8, 0)]


def test_u_shape_starts_at_the_global_minimum():
    m = plane(5, 5, rects=[(1, 0, 1, 3), (3, 1, 3, 3), (1, 3, 3, 3)])
    b = all_borders(m)
    assert len(b) == 1 and b[0][0] == (1, 0)
    assert (3, 1) in b[0][2] and pts(m)[0] == (1, 0)


def test_tie_goes_to_the_lower_square():
    m = plane(6, 4, rects=[(0, 0, 1, 1), (0, 3, 1, 4)])
    assert [s for s, _, _ in all_borders(m)] == [(0, 0), (0, 3)]
    assert pts(m) == [(0, 3), (0, 4), (1, 4), (1, 3)]
    # more points win over position
    m2 = plane(7, 4, rects=[(0, 0, 2, 2), (0, 4, 1, 5)])
    m2[2, 2] = 0  # the upper square loses a corner and gains a point: it wins although it comes first
    assert pts(m2) == [(0, 0), (0, 2), (1, 2), (2, 1), (2, 0)]


def test_component_touching_all_four_edges():
    m = plane(5, 5, rects=[(0, 2, 4, 2), (2, 0, 2, 4)])
    b = all_borders(m)
    assert len(b) == 1 and b[0][0] == (2, 0)
    # every pixel but the centre, which the diagonal steps between the arms cut off
    assert set(b[0][1]) == {(int(x), int(y)) for y, x in zip(*np.nonzero(m))} - {(2, 2)}
    assert {(2, 0), (0, 2), (2, 4), (4, 2)} <= set(b[0][2])


def test_all_ones_and_thin_planes():
    assert pts(np.ones((4, 5), dtype=np.uint8)) == [(0, 0), (0, 3), (4, 3), (4, 0)]
    assert pts(np.ones((1, 1), dtype=np.uint8)) == [(0, 0)]
    assert pts(np.ones((1, 7), dtype=np.uint8)) == [(0, 0), (6, 0)]
    assert pts(np.ones((7, 1), dtype=np.uint8)) == [(0, 0), (0, 6)]
    assert pts(plane(1, 7, [(1, 0), (2, 0), (5, 0)])) == [(1, 0), (2, 0)]  # 2 points beat the later single pixel
    assert pts(plane(7, 1, [(0, 1), (0, 4)])) == [(0, 4)]


# ------------------------------------------------------------------------------------------------ properties
def random_planes(count=2000, seed=7):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(count):
        h, w = (int(v) for v in rng.integers(1, 13, 2))
        out.append((rng.random((h, w)) < rng.uniform(0.2, 0.8)).astype(np.uint8))
    for _ in range(count // 5):  # uniform noise this small almost never nests: noise inside rings, some of them broken
        h, w = (int(v) for v in rng.integers(7, 13, 2))
        m = (rng.random((h, w)) < rng.uniform(0.2, 0.8)).astype(np.uint8)
        x0, y0 = int(rng.integers(0, w - 5)), int(rng.integers(0, h - 5))
        x1, y1 = int(rng.integers(x0 + 4, w)), int(rng.integers(y0 + 4, h))
        m[y0:y1 + 1, x0:x1 + 1][:2, :] = m[y0:y1 + 1, x0:x1 + 1][-2:, :] = 0
        m[y0:y1 + 1, x0:x1 + 1][:, :2] = m[y0:y1 + 1, x0:x1 + 1][:, -2:] = 0
        m[y0:y1 + 1, [x0, x1]] = 1
        m[[y0, y1], x0:x1 + 1] = 1
        if rng.random() < 0.3:
            m[int(rng.integers(y0, y1 + 1)), x0] = 0
        out.append(m)
    return out


def expand(kept):
    """The emitted chain from the kept points: straight 8-direction runs between cyclic neighbours."""
    if len(kept) == 1:
        return list(kept)
    out = []
    for a, b in zip(kept, kept[1:] + kept[:1]):
        dx, dy = b[0] - a[0], b[1] - a[1]
        n = max(abs(dx), abs(dy))
        assert n > 0 and (dx == 0 or dy == 0 or abs(dx) == abs(dy))
        out += [(a[0] + dx // n * i, a[1] + dy // n * i) for i in range(n)]
    return out


def test_border_properties_against_scipy_labels():
    borders = comps = 0
    for m in random_planes():
        H, W = m.shape
        lab, n = ndimage.label(m, structure=np.ones((3, 3)))
        pad = np.zeros((H + 2, W + 2), dtype=np.uint8)
        pad[1:-1, 1:-1] = m
        bl, _ = ndimage.label(pad == 0)  # 4-connected by default
        frame = bl == bl[0, 0]
        near = frame[:-2, 1:-1] | frame[2:, 1:-1] | frame[1:-1, :-2] | frame[1:-1, 2:]
        top = sorted(set(lab[near & (m != 0)].tolist()))
        got = all_borders(m)
        assert len(got) == len(top)
        seen = set()
        for (sx, sy), chain, kept in got:
            l = int(lab[sy, sx])
            assert l in top and l not in seen
            seen.add(l)
            ys, xs = np.nonzero(lab == l)
            assert (sy, sx) == (ys[0], xs[0])  # np.nonzero is in raster order
            assert all(lab[y, x] == l for x, y in chain)
            if len(chain) > 1:
                assert all((b[0] - a[0], b[1] - a[1]) in STEPS for a, b in zip(chain, chain[1:] + chain[:1]))
            cx, cy = [p[0] for p in chain], [p[1] for p in chain]
            assert (min(cx), max(cx), min(cy), max(cy)) == (xs.min(), xs.max(), ys.min(), ys.max())
            assert kept[0] == (sx, sy) and expand(kept) == chain
        borders += len(got)
        comps += n
    assert borders > 3000 and comps > borders + 300  # the sample holds nested components


# ------------------------------------------------------------------------------------------------ contour_check
@pytest.fixture(scope="session")
def contour_check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    exe = tmp_path_factory.mktemp("contour_check") / "contour_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "contour_check.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # no sanitizer runtimes: a plain build
        subprocess.run(cmd, check=True)

    def run(mode, planes):
        text = "".join(f"{m.shape[0]} {m.shape[1]}\n" + "".join("".join("1" if v else "0" for v in r) + "\n" for r in m)
                       for m in planes)
        p = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True, timeout=300)
        assert p.stderr == "", p.stderr  # the sanitizers stay silent
        assert p.returncode == 0, p.stdout[-500:]
        lines = p.stdout.strip().splitlines()
        assert len(lines) == len(planes)
        return [[int(t) for t in line.split()] for line in lines]
    return run


def exhaustive(h, w):
    n = h * w
    return [np.array([(b >> i) & 1 for i in range(n)], dtype=np.uint8).reshape(h, w) for b in range(1 << n)]


def check_planes():
    rng = np.random.default_rng(3)
    big = [(rng.random((h, w)) < d).astype(np.uint8) for h, w, d in ((33, 65, 0.5), (37, 70, 0.6), (64, 64, 0.4), (40, 31, 0.7))]
    return exhaustive(3, 4) + exhaustive(4, 3) + random_planes() + big


def test_shared_header_selects_what_the_oracle_selects(contour_check):
    planes = check_planes()
    for m, v in zip(planes, contour_check("select", planes)):
        ref = contour(m)
        assert v[0] == len(ref) and v[1:] == ref.reshape(-1).tolist(), m


def test_shared_header_finds_every_top_level_border(contour_check):
    planes = check_planes()
    for m, v in zip(planes, contour_check("all", planes)):
        ref = [k for _, _, k in all_borders(m)]
        got, i = [], 1
        for _ in range(v[0]):
            k = v[i]
            got.append([(v[i + 1 + 2 * j], v[i + 2 + 2 * j]) for j in range(k)])
            i += 1 + 2 * k
        assert i == len(v) and got == ref, m


def test_header_is_plain_cxx():
    src = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "ym_contour.h")).read()
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <stdint.h>"]


# ------------------------------------------------------------------------------------------------ Results surface
class StubEngine:
    """What Masks needs of an Engine: `device` and `mask_contours` (here: the oracle)."""

    def __init__(self):
        self.device = torch.device("cpu")
        self.calls = 0

    def mask_contours(self, masks):
        self.calls += 1
        assert masks.dim() == 3 and masks.dtype in (torch.uint8, torch.bool)
        return contours(masks.numpy())


def seg_planes():
    m = np.zeros((3, 64, 64), dtype=np.uint8)
    m[0, 20:40, 10:30] = 1   # x 10..29, y 20..39
    m[1, 0:64, 5:8] = 1      # reaches into the letterbox bars: y is clipped
    m[2, 30, 40] = 1
    return torch.from_numpy(m)


def seg_results(eng, boxes=None):
    from core.results import Results
    boxes = torch.tensor([[9.0, 4, 28, 22, 0.9, 1], [4, 0, 7, 30, 0.8, 0], [37, 13, 38, 14, 0.7, 2]]) if boxes is None else boxes
    r = Results(None, {0: "a", 1: "b", 2: "c"}, boxes, masks=seg_planes(), annotator=eng)
    r.orig_shape = r.boxes.orig_shape = r.masks.orig_shape = (30, 60)  # an image-file source, letterboxed into 64 x 64
    return r


def test_masks_xy_scales_clips_and_normalises():
    from yolomi.preprocess import scale_coords
    eng = StubEngine()
    r = seg_results(eng)
    xy = r.masks.xy
    assert len(xy) == 3 and all(p.dtype == np.float32 and p.ndim == 2 and p.shape[1] == 2 for p in xy)
    g = np.float32(64 / 60)  # gain; pad (0, 16)
    assert xy[0].tolist() == [[np.float32(10) / g, np.float32(4) / g], [np.float32(10) / g, np.float32(23) / g],
                              [np.float32(29) / g, np.float32(23) / g], [np.float32(29) / g, np.float32(4) / g]]
    assert xy[0][0].tolist() == pytest.approx([9.375, 3.75], rel=1e-6)
    assert xy[1][:, 1].min() == 0.0 and xy[1][:, 1].max() == 30.0  # clipped to the image
    assert xy[2][0].tolist() == pytest.approx([37.5, 13.125], rel=1e-6)
    for p, ref in zip(xy, contours(seg_planes().numpy())):
        assert np.array_equal(p, scale_coords((64, 64), torch.from_numpy(ref.astype(np.float32)), (30, 60)).numpy())
    for p, q in zip(xy, r.masks.xyn):
        assert q.dtype == np.float32 and np.array_equal(q, p / np.array([60, 30], dtype=np.float32))


def test_masks_xy_is_cached_and_sliced():
    eng = StubEngine()
    r = seg_results(eng)
    sub0 = r[1:3]
    assert eng.calls == 0
    xy = r.masks.xy
    assert r.masks.xy is xy and r.masks.xyn is not None and eng.calls == 1
    sub = r[1:3]
    assert [p.tolist() for p in sub.masks.xy] == [p.tolist() for p in xy[1:3]] and eng.calls == 1
    assert r[torch.tensor([2, 0])].masks.xy[0] is xy[2] and r[[True, False, True]].masks.xy[1] is xy[2]
    assert r.cpu().masks.xy is xy and r.masks[0].xy[0] is xy[0] and eng.calls == 1
    assert [p.tolist() for p in sub0.masks.xy] == [p.tolist() for p in xy[1:3]] and eng.calls == 2  # sliced before: traced


def test_hand_built_masks_need_an_engine():
    from core.results import Masks, Results
    with pytest.raises(RuntimeError):
        Masks(seg_planes(), (64, 64)).xy
    with pytest.raises(RuntimeError):
        Masks(seg_planes(), (64, 64)).xyn
    r = Results(torch.zeros(3, 64, 64), {0: "a", 1: "b", 2: "c"}, torch.zeros(3, 6), masks=seg_planes())
    with pytest.raises(RuntimeError):
        r.masks.xy
    m = Masks(seg_planes(), (64, 64), engine=StubEngine())  # tensor source: only the clip
    assert m.xy[0].tolist() == [[10, 20], [10, 39], [29, 39], [29, 20]]


def test_summary_carries_segments():
    r = seg_results(StubEngine())
    s = r.summary()
    assert s[0]["segments"] == {"x": [9.375, 9.375, 27.1875, 27.1875], "y": [3.75, 21.5625, 21.5625, 3.75]}
    assert s[2]["segments"] == {"x": [37.5], "y": [13.125]} and s[2]["name"] == "c"
    n = r.summary(normalize=True, decimals=3)
    assert n[0]["segments"] == {"x": [0.156, 0.156, 0.453, 0.453], "y": [0.125, 0.719, 0.719, 0.125]}
    from core.results import Results
    assert "segments" not in Results(None, {0: "a"}, torch.tensor([[1.0, 2, 3, 4, 0.5, 0]])).summary()[0]


def test_save_txt(tmp_path):
    from core.results import Results
    names = {0: "a", 1: "b", 2: "c"}
    img = torch.zeros(3, 100, 200)
    det = Results(img, names, torch.tensor([[20.0, 10, 60, 50, 0.5, 2], [0, 0, 200, 100, 0.25, 0]]))
    f = tmp_path / "sub" / "det.txt"
    det.save_txt(f)
    assert f.read_text() == "2 0.2 0.3 0.2 0.4\n0 0.5 0.5 1 1\n"
    det.save_txt(f, save_conf=True)  # appended, as upstream
    assert f.read_text().splitlines()[2:] == ["2 0.2 0.3 0.2 0.4 0.5", "0 0.5 0.5 1 1 0.25"]
    trk = Results(img, names, torch.tensor([[20.0, 10, 60, 50, 7, 0.5, 2]]))
    trk.save_txt(tmp_path / "trk.txt")
    assert (tmp_path / "trk.txt").read_text() == "2 0.2 0.3 0.2 0.4 7\n"
    trk.save_txt(tmp_path / "trkc.txt", save_conf=True)
    assert (tmp_path / "trkc.txt").read_text() == "2 0.2 0.3 0.2 0.4 0.5 7\n"
    pose = Results(img, names, torch.tensor([[20.0, 10, 60, 50, 0.5, 2]]),
                   keypoints=torch.tensor([[[50.0, 25, 0.9], [100, 50, 0.8]]]))
    pose.save_txt(tmp_path / "pose.txt")
    assert (tmp_path / "pose.txt").read_text() == "2 0.2 0.3 0.2 0.4 0.25 0.25 0.9 0.5 0.5 0.8\n"
    pose2 = Results(img, names, torch.tensor([[20.0, 10, 60, 50, 0.5, 2]]), keypoints=torch.tensor([[[50.0, 25], [100, 50]]]))
    pose2.save_txt(tmp_path / "pose2.txt", save_conf=True)
    assert (tmp_path / "pose2.txt").read_text() == "2 0.2 0.3 0.2 0.4 0.25 0.25 0.5 0.5 0.5\n"
    seg = seg_results(StubEngine())
    seg.save_txt(tmp_path / "seg.txt", save_conf=True)
    lines = (tmp_path / "seg.txt").read_text().splitlines()
    assert lines[0] == "1 0.15625 0.125 0.15625 0.71875 0.453125 0.71875 0.453125 0.125 0.9"
    assert lines[2] == "2 0.625 0.4375 0.7"
    for line, poly, cls in zip(lines, seg.masks.xyn, (1, 0, 2)):
        v = line.split()
        assert int(v[0]) == cls and len(v) == 1 + poly.size + 1
        assert np.allclose([float(t) for t in v[1:-1]], poly.reshape(-1), rtol=1e-5)
    empty = Results(img, names, torch.zeros(0, 6))
    empty.save_txt(tmp_path / "none.txt")
    assert not (tmp_path / "none.txt").exists()
