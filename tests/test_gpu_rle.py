"""COCO run-length encoding on the GPU: csrc/ym_rle.hip through Engine.mask_rle against tests/rle_oracle.py, counts, bytes
and area exact, at the smallest planes that reach each seam; the capacity protocol; Masks.rle / area / to_coco."""
import numpy as np
import pytest
import torch

from tests.golden.make_golden import make_input
from tests.rle_oracle import decode, encode

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
STRIP_WORDS = 13312  # csrc/ym_rle.h kRleLdsWords: the 32-row column words one workgroup holds
_cache = {}


def engine():  # around an empty context: the encoder reads planes, not a model
    from yolomi.engine import Engine
    from yolomi.lib import Runtime
    if "bare" not in _cache:
        _cache["bare"] = e = Engine.__new__(Engine)
        e.device, e.task, e.kpt_shape, e.rt = DEV, "detect", None, Runtime(0, None)
    return _cache["bare"]


def noise(n, h, w, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.random((n, h, w)) < rng.uniform(0.05, 0.95, (n, 1, 1))).astype(np.uint8)


def edges(h, w=5):  # column 1 ends set and column 2 starts set (one run across the boundary); pixel 0 set; zeros; ones
    m = np.zeros((4, h, w), dtype=np.uint8)
    m[0, -1, 1] = m[0, 0, 2] = m[1, 0, 0] = m[3] = 1
    return np.concatenate([m, noise(4, h, w, seed=h)])


def strips(extra):
    """Just above one workgroup's LDS: four strips of whole columns (40 rows: 2 words a column, 6,656 columns a strip).
    Plane 0: a blob across the first strip boundary, an empty third strip, short runs in the fourth; plane 1: a strip
    of ones (no transition inside it, but area and both neighbours' carries)."""
    cs = STRIP_WORDS // 2
    m = np.zeros((2, 40, 3 * cs + extra), dtype=np.uint8)
    m[0, 5:, cs - 6:cs + 7] = m[0, ::3, 3 * cs + 2:] = m[1, :, cs:2 * cs] = m[1, 7, 5] = 1
    return m


def tall():  # one column taller than a workgroup's LDS: pieces of a column, a run across the piece boundary
    m = np.zeros((1, 32 * STRIP_WORDS + 77, 2), dtype=np.uint8)
    m[0, 32 * STRIP_WORDS - 3:32 * STRIP_WORDS + 40, 0] = m[0, -1, 0] = m[0, 0, 1] = m[0, -5:, 1] = 1
    return m


def long_run():  # a run above 2^15 then runs of 1: groups of up to 4 bytes and negative differences
    m = np.zeros((1, 300, 300), dtype=np.uint8)
    m[0, 100:, 150] = m[0, 5, 200] = m[0, 7, 200] = 1
    return m


CASES = {"1x1": lambda: np.array([[[0]], [[1]]], dtype=np.uint8), "1xW": lambda: noise(6, 1, 70), "Hx1": lambda: noise(6, 70, 1),
         "H31": lambda: edges(31), "H32": lambda: edges(32), "H33": lambda: edges(33), "H65": lambda: edges(65),
         "checkerboard": lambda: (~np.indices((33, 7)).sum(0) & 1).astype(np.uint8)[None],  # pixel 0 set, 33 rows: alternates on
         "odd_width": lambda: noise(20, 37, 67), "aligned_width": lambda: noise(20, 64, 64, seed=1),
         "strips": lambda: strips(10), "strips_aligned": lambda: strips(12), "tall": tall, "long_run": long_run,
         "none": lambda: np.zeros((0, 8, 8), dtype=np.uint8)}


def same(got, ref):
    assert got[0].dtype == np.uint32 and np.array_equal(got[0], ref[0]) and got[1] == ref[1] and got[2] == ref[2]


@pytest.mark.parametrize("case", list(CASES))
def test_engine_against_oracle(case):
    planes = CASES[case]()
    got = engine().mask_rle(torch.from_numpy(planes).to(DEV))
    assert len(got) == len(planes) and (case != "checkerboard" or len(got[0][0]) == 33 * 7 + 1)  # the most runs there are
    [same(g, encode(p)) for g, p in zip(got, planes)]


def test_stride_bool_and_other_values():
    slots = noise(18, 20, 24).reshape(6, 3, 20, 24)
    view = torch.from_numpy(slots).to(DEV)[:, 1]  # plane stride 3 * 20 * 24
    odd = torch.zeros(1 + view.numel(), dtype=torch.uint8, device=DEV)[1:].view(view.shape).copy_(view)  # W % 4 == 0, base % 4 == 1
    assert view.stride(0) == 3 * 20 * 24 and not view.is_contiguous() and odd.data_ptr() % 4 == 1
    ref = [encode(p) for p in slots[:, 1]]
    for t in (view, view.bool(), view * 255, view * 2, odd):
        [same(g, r) for g, r in zip(engine().mask_rle(t), ref)]


def test_capacities_too_small_write_nothing_that_does_not_fit():
    planes = noise(5, 33, 21, seed=4)
    ref = [encode(p) for p in planes]
    runs, nbytes = [len(r[0]) for r in ref], [len(r[1]) for r in ref]
    e, t = engine(), torch.from_numpy(planes).to(DEV)
    cap_c, cap_b = sum(runs[:2]) + 1, sum(nbytes[:3]) + 1  # two planes' counts fit, three planes' bytes
    fill = torch.full((cap_c,), -7, dtype=torch.int32, device=DEV), torch.full((cap_b,), 7, dtype=torch.uint8, device=DEV)
    ro, bo, area = (torch.empty((k,), dtype=torch.int64, device=DEV) for k in (6, 6, 5))
    st = torch.cuda.current_stream(DEV).cuda_stream
    e.rt.mask_rle(t.data_ptr(), 5, 33, 21, 33 * 21, fill[0].data_ptr(), cap_c, fill[1].data_ptr(), cap_b, ro.data_ptr(),
                  bo.data_ptr(), area.data_ptr(), st)
    assert [ro.cpu().tolist(), bo.cpu().tolist()] == [np.concatenate([[0], np.cumsum(v)]).tolist() for v in (runs, nbytes)]
    assert area.cpu().tolist() == [r[2] for r in ref]
    assert fill[0].cpu().numpy().view(np.uint32).tolist() == np.concatenate([r[0] for r in ref[:2]]).tolist() + [2 ** 32 - 7]
    assert fill[1].cpu().numpy().tobytes() == b"".join(r[1] for r in ref[:3]) + b"\x07"
    e.rt.mask_rle(t.data_ptr(), 5, 33, 21, 33 * 21, 0, 0, 0, 0, ro.data_ptr(), bo.data_ptr(), area.data_ptr(), st)  # count-only
    assert ro.cpu().tolist()[-1] == sum(runs) and bo.cpu().tolist()[-1] == sum(nbytes)
    [same(g, r) for g, r in zip(e.mask_rle(t, cap_counts=cap_c, cap_bytes=cap_b), ref)]  # the retry returns everything


@pytest.mark.parametrize("retina", [False, True])
def test_predict_rle_area_and_to_coco(retina):
    from core.model import YOLO11Model
    if "m" not in _cache:
        _cache["m"] = YOLO11Model(task="segment", size="n", device="cuda:0", dtype="f32")
    r = _cache["m"].predict(make_input("uniform", (81, 82), 320).to(DEV), conf=0.25, retina_masks=retina)[0]
    planes = r.masks.data.cpu().numpy().astype(np.uint8)
    rle = r.masks.rle
    assert len(rle) == len(planes) == len(r.boxes) > 0 and r.masks.rle is rle and r.cpu().masks.rle is rle and r.masks.to("cpu").rle is rle
    for e, p in zip(rle, planes):
        assert e["size"] == list(p.shape) and isinstance(e["counts"], bytes) and np.array_equal(decode(e["counts"], e["size"]), p)
    assert r.masks.area.dtype == np.int64 and r.masks.area.tolist() == planes.sum((1, 2)).tolist()
    assert r[1:3].masks.rle == rle[1:3]
    class_map = list(range(100, 200))
    for i, (c, row) in enumerate(zip(r.to_coco(image_id=42, class_map=class_map), r.boxes.data.cpu().tolist())):
        assert set(c) == {"image_id", "category_id", "bbox", "score", "segmentation"} and c["image_id"] == 42
        assert c["category_id"] == 100 + int(row[5]) and c["score"] == round(row[4], 5)
        assert c["bbox"] == [round(v, 3) for v in (row[0], row[1], row[2] - row[0], row[3] - row[1])]
        assert c["segmentation"] == {"size": rle[i]["size"], "counts": rle[i]["counts"].decode("ascii")}
