"""Host tests of the annotator (Results.plot / Engine.annotate): literal known answers of the drawing rules
against the numpy oracle (tests/plot_oracle.py); the functions the kernels call (csrc/ym_annot.h), compiled into the
stand-alone tests/annot_check.cpp — with AddressSanitizer and UBSan where their runtimes link — against the oracle, bit
for bit, on every scripted scene (tests/plot_scenes.py), and its "%.2f" against Python on 100k fp32 values; the committed
font against Pillow; and the Python facade (no host read in Engine.annotate, the refusal of a Results without an
annotator)."""
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import plot_oracle as O
from tests import plot_scenes as S
from tests.test_plan_format import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FMT_CASES = {0.125: "0.12", 0.375: "0.38", 0.625: "0.62", 0.875: "0.88", 0.995: "1.00", 0.0: "0.00", 1.0: "1.00"}


# ------------------------------------------------------------------------------------------------ known answers
def test_palette_and_tables():
    assert O.palette(0) == (255, 42, 4) and O.palette(20) == O.palette(0)
    assert len(O.PALETTE_HEX) == 20 and len(O.POSE_PALETTE) == 20 and len(O.KPT_IDX) == 17
    assert len(O.SKELETON) == len(O.LIMB_IDX) == 19
    assert O.text_colour((255, 255, 255)) == (17, 31, 104) and O.text_colour(O.palette(0)) == (255, 255, 255)


def test_line_width_rule():
    assert O.line_width(640, 640) == 2 and O.line_width(1080, 1920) == 5 and O.line_width(72, 104) == 2
    assert O.line_width(640, 640, 7) == 7


def test_disc_and_limb_counts():
    assert O.disc_mask(64, 64, 20, 20, 5).sum() == 81 and O.disc_mask(64, 64, 20, 20, 2).sum() == 13
    assert O.limb_mask(64, 64, (1, 1), (11, 5), 1).sum() == 11
    assert O.limb_mask(64, 64, (1, 1), (11, 5), 2).sum() == 27
    assert O.limb_mask(64, 64, (1, 9), (9, 1), 1).sum() == 9
    # a degenerate limb is its end disc, not the whole plane
    assert O.limb_mask(64, 64, (7, 7), (7, 7), 2).sum() == 5 and O.limb_mask(64, 64, (7, 7), (7, 7), 1).sum() == 1


def test_blend_values():
    assert O.blend_value(100, [255]) == 177
    assert O.blend_value(100, [4]) == 52
    assert O.blend_value(200, [42, 219]) == 159
    assert O.blend_value(255, [255, 255, 255]) == 159


def test_blend_one_mask_equals_real_arithmetic():
    from fractions import Fraction
    u, c = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    f = np.float32
    got = np.clip((((u.astype(f) / f(255)) * f(0.5)).astype(f) + ((c.astype(f) / f(255)) * f(0.5)).astype(f)).astype(f)
                  * f(255), 0, 255).astype(np.uint8)
    want = np.array([[int(Fraction(a + b, 2)) for b in range(256)] for a in range(256)], dtype=np.uint8)
    assert np.array_equal(got, want)


def test_fmt_cases():
    for v, s in FMT_CASES.items():
        assert O.fmt_conf(np.float32(v)) == s


def test_outlines_written_out():
    got = {(x, y) for y, x in zip(*np.nonzero(O.outline_mask(16, 16, 3, 4, 7, 6, 1)))}
    want = {(x, 4) for x in range(3, 8)} | {(x, 6) for x in range(3, 8)} | {(3, 5), (7, 5)}  # a = 0, b = 1: the border itself
    assert got == want
    got = {(x, y) for y, x in zip(*np.nonzero(O.outline_mask(16, 16, 4, 4, 10, 9, 3)))}
    # a = 1, b = 2: from one outside to one inside the corners
    want = {(x, y) for x in range(3, 12) for y in range(3, 11)} - {(x, y) for x in range(6, 9) for y in range(6, 8)}
    assert got == want


def test_label_flips_and_shifts():
    lw = 2  # s = 1, pad = 1: a 5-character label is 32 x 13
    assert O.label_layout(10, 20, 5, lw, 100) == (10, 7, 32, 13, 1)     # above the box
    assert O.label_layout(10, 12, 5, lw, 100) == (10, 12, 32, 13, 1)    # top edge: inside the box
    assert O.label_layout(10, 13, 5, lw, 100) == (10, 0, 32, 13, 1)
    assert O.label_layout(90, 20, 5, lw, 100) == (68, 7, 32, 13, 1)     # right edge: shifted left
    assert O.label_layout(68, 20, 5, lw, 100) == (68, 7, 32, 13, 1)
    assert O.label_layout(5, 20, 40, lw, 100) == (0, 7, 242, 13, 1)     # wider than the canvas: from 0
    assert O.label_layout(10, 40, 2, 4, 100) == (10, 14, 28, 26, 2)     # lw 4: glyph scale 2
    img = O.paint(np.zeros((40, 100, 3), np.uint8), [[90, 5, 99, 30, 0.5, 0]], {0: "ab"}, line_width_=2)
    ys, xs = np.nonzero((img == np.array(O.palette(0))).all(-1))
    assert xs.min() == 100 - (6 * 7 + 2) and ys.min() == 4  # "ab 0.50": 7 characters, flipped inside, outline from Y1 - 1


def test_label_text():
    assert O.label_text(True, 42, "car", True, np.float32(0.625)) == "id:42 car 0.62"
    assert O.label_text(False, 0, "car", False, 0.5) == "car"
    assert O.clean_name(S.NAMES, 3) == "a name that is longer th" and O.clean_name(S.NAMES, 4) == "caf?"
    assert O.clean_name(S.NAMES, 6) == "?" and O.clean_name(S.NAMES, None) == "?"


def test_keypoint_rule():
    assert O.kpt_drawable([5.5, 6.5, 0.9], 3, 100, 50) == (5, 6)
    assert O.kpt_drawable([5.5, 6.5, 0.49], 3, 100, 50) is None
    assert O.kpt_drawable([0.0, 6.5], 2, 100, 50) is None and O.kpt_drawable([100.0, 6.5], 2, 100, 50) is None
    assert O.kpt_drawable([5.5, 50.0], 2, 100, 50) is None and O.kpt_drawable([-0.5, 6.5], 2, 100, 50) == (0, 6)
    assert O.kpt_drawable([np.nan, 1.0], 2, 100, 50) is None and O.kpt_drawable([1e30, 1.0], 2, 100, 50) is None


def test_font_matches_pillow():
    from yolomi.font6x11 import FONT_BYTES, GLYPHS
    assert len(GLYPHS) == 95 and all(len(g) == 11 and all(0 <= r < 64 for r in g) for g in GLYPHS)
    assert len(set(GLYPHS)) == 95 and [i for i, g in enumerate(GLYPHS) if not any(g)] == [0]
    assert len(FONT_BYTES) == 95 * 11
    ImageFont = pytest.importorskip("PIL.ImageFont")
    if not hasattr(ImageFont, "load_default_imagefont"):
        pytest.skip("this Pillow has no load_default_imagefont")
    font = ImageFont.load_default_imagefont()
    for c in range(32, 127):
        m = font.getmask(chr(c))
        assert m.size == (6, 11)
        rows = tuple(sum((1 << (5 - x)) for x in range(6) if m.getpixel((x, y))) for y in range(11))
        assert rows == GLYPHS[c - 32], chr(c)


# ------------------------------------------------------------------------------------------------ the header on the host
@pytest.fixture(scope="session")
def annot_check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    d = tmp_path_factory.mktemp("annot_check")
    exe = d / "annot_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off",
           os.path.join(ROOT, "tests", "annot_check.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # no sanitizer runtimes: a plain build
        subprocess.run(cmd, check=True)

    def run(*args):
        p = subprocess.run([str(exe), *map(str, args)], capture_output=True, text=True, timeout=300)
        assert p.stderr == "", p.stderr  # the sanitizers stay silent
        assert p.returncode == 0, p.stdout
        return p.stdout
    run.dir = d
    return run


def test_header_is_plain_cxx():
    src = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "ym_annot.h")).read()
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cmath>", "#include <cstdint>"]


def test_header_counts(annot_check):
    assert annot_check("count", "disc", 20, 20, 5).strip() == "81"
    assert annot_check("count", "disc", 20, 20, 2).strip() == "13"
    assert annot_check("count", "limb", 1, 1, 11, 5, 1).strip() == "11"
    assert annot_check("count", "limb", 1, 1, 11, 5, 2).strip() == "27"
    assert annot_check("count", "limb", 1, 9, 9, 1, 1).strip() == "9"
    assert annot_check("count", "limb", 7, 7, 7, 7, 2).strip() == "5"
    assert annot_check("count", "limb", -1000000, -999999, 1000000, 1000001, 3).strip() == str(
        int(O.limb_mask(64, 64, (-1000000, -999999), (1000000, 1000001), 3).sum()))


def test_header_fmt_matches_python(annot_check):
    rng = np.random.default_rng(5)
    vals = np.concatenate([
        np.array(list(FMT_CASES), dtype=np.float32), rng.random(100000, dtype=np.float32),
        (rng.integers(0, 101, 20000) / 100).astype(np.float32),                       # the two-decimal grid itself
        ((2 * rng.integers(0, 100, 20000) + 1) / 200).astype(np.float32),             # near the rounding ties
        np.nextafter(np.float32(0.125), np.float32([0, 1])), np.float32([1e-45, 1e-30, 0.005, 0.015, 0.004999, 9.994, 9.996]),
        np.float32([-0.0, -1e-9, 10.0, np.nan, np.inf, -np.inf])])
    p = annot_check.dir / "fmt.bin"
    vals.astype("<f4").tofile(p)
    got = annot_check("fmt", p).split("\n")[:-1]
    want = [O.fmt_conf(v) for v in vals]
    assert len(got) == len(want)
    bad = [(float(v), g, w) for v, g, w in zip(vals, got, want) if g != w]
    assert not bad, bad[:10]
    assert got[:7] == list(FMT_CASES.values())


@pytest.mark.parametrize("size", S.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_header_scenes_match_oracle(size, annot_check):
    from yolomi.font6x11 import FONT_BYTES
    table = S.name_table()
    for s in S.scenes(*size):
        arrays = S.batch_arrays(s)
        for b in range(2):
            src, dst = annot_check.dir / "scene.bin", annot_check.dir / "scene.out"
            src.write_bytes(S.scene_file(s, b, arrays, FONT_BYTES, table))
            annot_check("render", src, dst)
            got = np.fromfile(dst, dtype=np.uint8).reshape(s["H"], s["W"], 3)
            want = S.oracle_image(s, b, arrays)
            diff = np.argwhere((got != want).any(-1))
            assert not len(diff), (s["name"], b, len(diff), diff[:5].tolist())


def test_scenes_are_not_trivial():
    """Each scene changes pixels, and image 1 differs from image 0 (so a batch-index slip would show)."""
    for s in S.scenes(*S.SIZES[0]):
        arrays = S.batch_arrays(s)
        imgs = [S.oracle_image(s, b, arrays) for b in range(2)]
        base = [arrays[0][b] if s["u8"] else O.canvas_from_tensor(arrays[0][b]) for b in range(2)]
        assert any((imgs[b] != base[b]).any() for b in range(2)), s["name"]
        if int(arrays[2][1]) == 0:
            assert np.array_equal(imgs[1], base[1])


# ------------------------------------------------------------------------------------------------ the Python facade
class _StubRuntime:
    def __init__(self):
        self.calls = []

    def annotate(self, *a):
        self.calls.append(a)


def _stub_engine(monkeypatch, task="detect", kpt_shape=None):
    from yolomi.engine import Engine
    e = Engine.__new__(Engine)
    e.device, e.task, e.kpt_shape = torch.device("cpu"), task, kpt_shape
    e.rt, e.names, e._annot_tables = _StubRuntime(), dict(S.NAMES), None
    monkeypatch.setattr(torch.cuda, "current_stream", lambda dev=None: type("St", (), {"cuda_stream": 0})())
    return e


def test_annotate_reads_no_tensor_value(monkeypatch):
    e = _stub_engine(monkeypatch, "pose", (17, 3))
    frames = torch.zeros((2, 3, 32, 64))
    dets, counts = torch.zeros((2, 300, 7 + 52)), torch.zeros((2,), dtype=torch.int32)
    masks = torch.zeros((2, 16, 32, 64), dtype=torch.uint8)
    from yolomi import annotate as A
    A._tables(e)  # (the one-time upload of the font and the names is not part of a call)

    def boom(*a, **k):
        raise AssertionError("Engine.annotate read a tensor's value on the host")
    for name in ("cpu", "tolist", "item", "numpy", "__bool__", "__int__", "__float__", "__index__", "__len__"):
        monkeypatch.setattr(torch.Tensor, name, boom)
    monkeypatch.setattr(torch.cuda, "synchronize", boom)
    out = e.annotate(frames, dets, counts, masks=masks, tracked=True)
    assert tuple(out.shape) == (2, 32, 64, 3) and out.dtype == torch.uint8
    (call,) = e.rt.calls
    assert call[0] == frames.data_ptr() and call[1] is True and call[2:5] == (2, 32, 64)
    assert call[5] == dets.data_ptr() and call[6] == 300 and call[7] == counts.data_ptr() and call[8] == masks.data_ptr()
    args = call[14]
    assert (args.line_width, args.kpt_radius, args.flags, args.tracked, args.det_stride) == (2, 5, 63, 1, 59)  # every switch on, clip_kpts too
    assert (args.K, args.ndim, args.mask_cap, args.nc) == (17, 3, 16, 23)
    out2 = e.annotate(frames, dets, counts, out=out, labels=False, color_mode="instance", line_width=4)
    assert out2 is out and e.rt.calls[1][14].flags == 61 and e.rt.calls[1][14].color_mode == 1 and e.rt.calls[1][8] == 0


def test_annotate_refuses_bad_arguments(monkeypatch):
    e = _stub_engine(monkeypatch)
    frames, dets, counts = torch.zeros((1, 3, 32, 32)), torch.zeros((1, 4, 6)), torch.zeros((1,), dtype=torch.int32)
    with pytest.raises(ValueError):
        e.annotate(frames.double(), dets, counts)
    with pytest.raises(ValueError):
        e.annotate(frames, dets, counts.long())
    with pytest.raises(ValueError):
        e.annotate(frames, dets, counts, color_mode="rainbow")
    with pytest.raises(ValueError):
        e.annotate(frames, dets, counts, masks=torch.zeros((4, 32, 32), dtype=torch.uint8))
    assert not e.rt.calls


def test_plot_without_annotator_raises():
    from core.results import Results
    r = Results(torch.zeros((3, 32, 32)), {0: "a"}, torch.tensor([[1.0, 2.0, 10.0, 12.0, 0.5, 0.0]]))
    with pytest.raises(RuntimeError, match="annotator"):
        r.plot()
    with pytest.raises(RuntimeError, match="annotator"):
        r.save("never.png")
    with pytest.raises(RuntimeError, match="annotator"):
        r.plot(txt_color=(255, 255, 255))  # an unknown keyword is ignored, not refused: the annotator is what is missing


def test_plot_through_a_stub_annotator(monkeypatch):
    """Results.plot hands the annotator one batch of one: rows = boxes | keypoints, the masks as one slot row."""
    from core.results import Results
    seen = {}

    class Ann:
        device = torch.device("cpu")

        def annotate(self, frames, dets, counts, **kw):
            seen.update(kw, frames=frames, dets=dets, counts=counts)
            return torch.full((1, frames.shape[2], frames.shape[3], 3), 7, dtype=torch.uint8)
    boxes = torch.tensor([[1.0, 2.0, 10.0, 12.0, 3.0, 0.5, 0.0], [2.0, 3.0, 11.0, 13.0, 4.0, 0.6, 0.0]])
    kp = torch.rand((2, 17, 3)) * 20
    r = Results(torch.rand((3, 32, 64)), {0: "a"}, boxes, keypoints=kp.clone(), annotator=Ann(),
                masks=torch.ones((2, 32, 64), dtype=torch.bool))
    before = r.boxes.data.clone()
    img = r.plot(conf=False, font="Arial.ttf", pil=True)
    assert img.shape == (32, 64, 3) and img.dtype == np.uint8 and (img == 7).all()
    assert tuple(seen["dets"].shape) == (1, 2, 7 + 51) and seen["counts"].tolist() == [2] and seen["tracked"] is True
    assert seen["kpt_shape"] == (17, 3) and tuple(seen["masks"].shape) == (1, 2, 32, 64) and seen["conf"] is False
    assert torch.equal(seen["dets"][0, :, :7], boxes) and torch.equal(r.boxes.data, before)
    assert r[0]._annotator is r._annotator and r.cpu()._annotator is r._annotator


@pytest.mark.parametrize("ncol", [6, 7], ids=["untracked", "tracked"])
@pytest.mark.parametrize("kshape", [(17, 3), (17, 2), (5, 3)], ids=lambda k: f"K{k[0]}x{k[1]}")
def test_plot_of_an_empty_pose_results(ncol, kshape):
    """A pose model's frame without a person: boxes (0, 6 | 7), keypoints (0, K, nd).  plot() hands the annotator one
    zeroed slot of the full row width and count 0, and the oracle returns the canvas."""
    from core.results import Results
    seen = {}

    class Ann:
        device = torch.device("cpu")

        def annotate(self, frames, dets, counts, **kw):
            seen.update(kw, dets=dets, counts=counts)
            return torch.zeros((1, frames.shape[2], frames.shape[3], 3), dtype=torch.uint8)
    x = torch.rand((3, 32, 64))
    r = Results(x, {0: "person"}, torch.zeros((0, ncol)), keypoints=torch.zeros((0, *kshape)), annotator=Ann())
    assert len(r) == 0 and tuple(r.keypoints.data.shape) == (0, *kshape)
    img = r.plot(txt_color="white")
    assert img.shape == (32, 64, 3)
    assert tuple(seen["dets"].shape) == (1, 1, ncol + kshape[0] * kshape[1]) and seen["counts"].tolist() == [0]
    assert seen["kpt_shape"] == kshape and seen["tracked"] is (ncol == 7) and seen["masks"] is None
    assert np.array_equal(O.paint_results(r), r.orig_img)
    # the same through from_batch, as predict() and track() build it (lazy boxes and keypoints of a zero count)
    rows = torch.zeros((1, 4, ncol + kshape[0] * kshape[1]))
    rb = Results.from_batch(x[None], 0, {0: "person"}, rows, 0, kpt_shape=kshape, tracked=ncol == 7, annotator=Ann())
    assert rb.plot().shape == (32, 64, 3) and seen["counts"].tolist() == [0]
    assert np.array_equal(O.paint_results(rb), rb.orig_img)


def test_draw_detections_delegates():
    from utils.visualization import draw_detections

    class Res:
        def plot(self, **kw):
            self.kw = kw
            return np.zeros((4, 4, 3), np.uint8)
    r = Res()
    image = np.full((4, 4, 3), 9, np.uint8)
    out = draw_detections(image, r, line_thickness=3)
    assert out.shape == (4, 4, 3) and r.kw["line_width"] == 3 and r.kw["img"] is image
    assert draw_detections(image, [r], class_names=["x"]).shape == (4, 4, 3)
