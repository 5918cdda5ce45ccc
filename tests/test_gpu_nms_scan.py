"""GPU tests (MI355X) at the edges of the shared NMS scan code, csrc/ym_nms_scan.h: the 256-candidate blocks and the
kept-list capacity of nms_blocked_scan (nms_image's blocked path, nms_ml_image) and the 64-row words of nms_scan_word
(nms_image's bit-matrix path).  Greedy NMS is a function of the sorted candidates alone, so wherever two GPU paths see
the same candidates the comparison is bit for bit.

yolo11n, the f32 plan, B = 2 at 320² (A = 2,100), eager runs, inputs make_input("uniform", (1, 2), 320).  With the
synthetic weights every anchor's best class scores above 0.001, so conf 0.001 gives 2,100 candidates per image, and
at iou 0.99 nothing is suppressed (the float64 oracle keeps all 2,100 of each image: checked below)."""
import copy
import os

import numpy as np
import pytest
import torch

from oracle import postprocess as pp
from oracle.predict import OracleModel
from tests.golden.make_golden import make_input
from tests.matching import MatchReport, match_image
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S, B, SEEDS = 320, 2, (1, 2)
NMS_BM, NMS_KEEP = 512, 512  # csrc/ym_common.h, csrc/ym_nms.hip
TOL_EXACT_XY, TOL_S = 5e-4, 5e-5  # the f32 plan's distance from the float64 evaluation (tests/test_gpu_x3.py)

_cache = {}


def engine(sd=None, key="stock"):
    from core.model import YOLO11Model
    if key not in _cache:
        kw = {} if sd is None else {"state_dict": sd}
        _cache[key] = YOLO11Model(task="detect", size="n", device="cuda:0", dtype="f32", verbose=False, **kw)
    return _cache[key].model.engine


def inputs():
    if "x" not in _cache:
        _cache["x"] = make_input("uniform", SEEDS, S)
    return _cache["x"]


def head64():
    """The oracle's head output (B, 84, A) evaluated in float64: computed once."""
    if "y64" not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        net = copy.deepcopy(OracleModel("n", "detect", synth_weights("n", "detect", 0)).net).double()
        with torch.no_grad():
            _cache["y64"] = net(inputs().double())[0][0]
    return _cache["y64"]


def run(eng, per_box=False, **kw):
    """(rows, counts) of one eager run; per_box: the blocked path off (YM_DBG_NMS 9, one box per barrier)."""
    from yolomi import lib as L
    prev = L.set_debug(L.DBG_NMS, 9) if per_box else None
    try:
        d, c = eng.run(inputs().to(DEV), use_graph=False, **kw)
        torch.cuda.synchronize()
        return d[:B].clone(), c[:B].tolist()
    finally:
        if per_box:
            L.set_debug(L.DBG_NMS, prev)


def assert_rows_equal(r0, r1, what):
    (d0, c0), (d1, c1) = r0, r1
    assert c0 == c1, (what, c0, c1)
    for b in range(B):
        assert torch.equal(d0[b, :c0[b]], d1[b, :c1[b]]), (what, b)


@pytest.mark.parametrize("max_nms", [255, 256, 257, 513])
def test_block_edges_single_label(max_nms):
    """ne one below, on and one above the first block boundary, and a third block of one row: nms_image's blocked path
    against the per-box path, bit for bit."""
    eng = engine()
    blocked = run(eng, conf=0.001, max_nms=max_nms)
    assert max(eng.candidate_counts(B)) > NMS_BM  # past the bit-matrix path, and more candidates than max_nms
    assert min(blocked[1]) > 0
    assert_rows_equal(blocked, run(eng, per_box=True, conf=0.001, max_nms=max_nms), max_nms)


def test_kept_list_capacity():
    """iou 0.99 at conf 0.001 keeps every candidate (float64 oracle: 2,100 of 2,100 per image), so the kept count
    runs into max_det.  max_det 511 and 512 (the blocked path's kept lists full to one below and to NMS_KEEP): blocked
    against per-box.  max_det 513 leaves the blocked path by its own guard; its first 512 rows are the 512 rows."""
    kept64 = [len(o) for o in pp.non_max_suppression(head64(), 0.001, 0.99, None, False, 3000)]
    assert min(kept64) >= NMS_KEEP + 1, kept64
    eng = engine()
    rows = {}
    for max_det in (511, 512):
        rows[max_det] = run(eng, conf=0.001, iou=0.99, max_det=max_det)
        assert max(eng.candidate_counts(B)) > NMS_BM
        assert max(rows[max_det][1]) == max_det, rows[max_det][1]
        assert_rows_equal(rows[max_det], run(eng, per_box=True, conf=0.001, iou=0.99, max_det=max_det), max_det)
    d513, c513 = run(eng, conf=0.001, iou=0.99, max_det=513)
    assert max(c513) == 513, c513
    d512, c512 = rows[512]
    for b in range(B):
        assert c512[b] == min(c513[b], 512)
        assert torch.equal(d513[b, :c512[b]], d512[b, :c512[b]]), b


@pytest.mark.parametrize("max_nms", [256, 257])
def test_multi_label_equals_single_label_at_block_edge(max_nms):
    """nms_ml_image and nms_image through one scan: with classes=[c] and c every anchor's best class, the multi-label
    pairs (anchor, c) are the single-label candidates, so rows and counts are identical — at ne on and one past a
    block boundary.  The single-label `classes` filter tests an anchor's best class, the multi-label one the pair's
    class, and with the stock synthetic weights every class scores above 0.001 at nearly every anchor, so no class
    gives the same set in both modes; class c's bias is raised by 6 here (its logit then leads every other class by
    0.8 or more at every anchor, and its scores stay spread over 0.45 .. 0.99).  Both are asserted on the head
    output of the run itself."""
    c = 3
    if "sd3" not in _cache:
        sd = dict(synth_weights("n", "detect", 0))
        for l in range(3):
            bias = sd[f"model.23.cv3.{l}.2.bias"].copy()
            bias[c] += 6.0
            sd[f"model.23.cv3.{l}.2.bias"] = bias
        _cache["sd3"] = sd
    eng = engine(_cache["sd3"], "class3")
    single = run(eng, conf=0.001, classes=[c], max_nms=max_nms)
    logits = eng.read_buffer(eng.graph.anchor_buf.id, B).reshape(B, -1, eng.graph.anchor_buf.C)[..., 64:144]
    sc = torch.sigmoid(logits)
    others = sc.clone()
    others[..., c] = -1.0
    above = sc[..., c] > 0.001
    assert bool((sc[..., c] > others.amax(-1))[above].all())  # the pair set is the anchor set
    assert int(above.sum(-1).min()) > NMS_BM, above.sum(-1).tolist()
    d1, c1 = eng.run(inputs().to(DEV), use_graph=False, conf=0.001, classes=[c], max_nms=max_nms, multi_label=True)
    torch.cuda.synchronize()
    assert min(single[1]) > 0
    assert_rows_equal(single, (d1[:B].clone(), c1[:B].tolist()), max_nms)


@pytest.mark.parametrize("max_nms", [64, 65, 128, 129])
def test_bit_matrix_word_edges(max_nms):
    """conf 0.1 leaves 200 and 304 candidates (float64 oracle), the bit-matrix path; max_nms cuts them to one full
    word, one word and one row, two words, two words and one row.  Against the float64 oracle's NMS of the same cut.
    The scores on either side of each cut are further apart than twice the score tolerance (asserted), so both sides
    cut at the same candidate."""
    conf, iou = 0.1, 0.7
    y64 = head64()
    best = y64[:, 4:84].amax(1)
    for b in range(B):
        s = best[b][best[b] > conf].sort(descending=True).values
        assert 64 < len(s) <= NMS_BM, len(s)
        assert float(s[max_nms - 1] - s[max_nms]) > 2 * TOL_S
    eng = engine()
    d, cnt = run(eng, conf=conf, iou=iou, max_nms=max_nms)
    assert all(64 < n <= NMS_BM for n in eng.candidate_counts(B)), eng.candidate_counts(B)
    ref = pp.non_max_suppression(y64, conf, iou, None, False, 300, max_nms=max_nms)
    rep = MatchReport()
    for b in range(B):
        r = ref[b].clone()
        r[:, :4] = pp.scale_boxes((S, S), r[:, :4], (S, S))
        match_image(r[:, :6].numpy(), d[b, :cnt[b]].cpu().numpy().astype(np.float64), conf, iou, TOL_EXACT_XY, TOL_S,
                    rep=rep)
    print(f"max_nms={max_nms}: kept gpu {cnt} oracle {[len(r) for r in ref]}; {rep}")
    assert rep.ok, f"{rep}; {rep.failures[:3]}"
    assert rep.matched > 0 and rep.exempt <= 0.02 * sum(len(r) for r in ref), rep  # (tests/test_gpu_val.py's bound)
