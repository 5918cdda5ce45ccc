"""GPU tests of the OBB task (MI355X): csrc/ym_obb.hip against the float64 rules of tests/obb_oracle.py.

NMS stage alone (Engine.obb_nms on crafted head rows): the reference is the float64 Fast-NMS on the boxes obb_decode
wrote (read back, class offset added in fp32).  Precondition, asserted: no pair of candidates has |probiou - iou| <
1e-3, so the fp32 kernel and float64 must take the same decisions: kept indices, order and counts are identical and
the rows carry obb_decode's values bit for bit.  Decode: against float64 at the detect bar, 5e-4 px (theta as corner
displacement).  End to end: yolo11n-obb synthetic weights through predict(), tests/matching.py on the boxes' hulls at
the x3 bars of tests/test_gpu_pose.py, then the corners of every matched pair.
"""
import numpy as np
import pytest
import torch

from tests import obb_oracle as oo
from tests.matching import MatchReport, match_image, ref_f64_slack
from tests.test_gpu_x3 import TOL_EXACT_XY, TOL_S, TOL_XY
from yolomi.synth import synth_weights, uniform

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
S = 320  # the NMS stage's input size: 2,100 anchors
_cache = {}


def model(nc=15, dtype="x3"):
    from core.model import YOLO11Model
    k = (nc, dtype)
    if k not in _cache:
        _cache[k] = YOLO11Model(task="detect", state_dict=synth_weights("n", "obb", 0, nc=nc), device="cuda:0",
                                dtype=dtype, verbose=False)
        assert _cache[k].task == "obb"  # the weights decide
    return _cache[k]


def bins(d):
    """(n, 16) DFL logits whose softmax expectation is d (two adjacent bins)."""
    k = np.floor(d).astype(int)
    out = np.full((len(d), 16), -30.0)
    out[np.arange(len(d)), k] = np.log(np.maximum(1 - (d - k), 1e-30))
    out[np.arange(len(d)), k + 1] = np.log(np.maximum(d - k, 1e-30))
    return out


def make_rows(n, nc, seed, dmax=1.5, logit=None):
    """(1, A, 64 + pad4(nc) + 4) head rows at S x S with n candidates on random anchors: ltrb distances U[0.3, dmax]
    cells (sides >= 4.8 px; see below), random class and angle, scores from U[-1, 3] logits (`logit`: all equal)."""
    from yolomi.arch import num_anchors
    rng = np.random.default_rng(seed)
    A, ncp = num_anchors(S, S), -(-nc // 4) * 4
    rows = np.zeros((A, 64 + ncp + 4))
    rows[:, 64:64 + ncp] = -20.0
    pick = rng.permutation(min(A, 3 * n))[:n]  # (a dense patch of the stride-8 level for small n)
    # most boxes are 5 px and isolated; about 150 candidates get sides up to 16 dmax px and overlap their neighbours
    d = np.where(rng.uniform(0, 1, (A, 1)) < 150.0 / max(n, 150), rng.uniform(0.3, dmax, (A, 4)), rng.uniform(0.3, 0.32, (A, 4)))
    rows[:, :64] = np.concatenate([bins(d[:, i]) for i in range(4)], 1)
    rows[pick, 64 + rng.integers(0, nc, n)] = rng.uniform(-1, 3, n) if logit is None else logit
    rows[:, 64 + ncp] = rng.uniform(-3, 3, A)
    return rows.astype(np.float32)[None]


def check_nms(nc, rows, iou=0.5, conf=0.25, max_det=300, agnostic=False, **kw):
    eng = model(nc).model.engine
    dets, counts = eng.obb_nms(torch.from_numpy(rows).to(DEV), S, S, conf=conf, iou=iou, max_det=max_det,
                               agnostic=agnostic, **kw)
    torch.cuda.synchronize()
    boxes, cov, sc, cl = (t[0].numpy() for t in eng.obb_decoded(1, S, S))
    b5 = np.concatenate([boxes, cov[:, :1]], 1)
    keep, order, p = oo.fast_nms(b5.astype(np.float64), sc, cl, np.arange(len(sc)), conf, iou, max_det, agnostic=agnostic,
                                 **kw)
    near = np.abs(p[np.triu_indices(len(order), 1)] - iou)
    assert not len(near) or near.min() >= 1e-3, f"a pair sits {near.min():.2g} from the threshold: pick another seed"
    n = int(counts[0])
    assert n == len(keep), (n, len(keep), len(order))
    want = np.concatenate([boxes[keep], sc[keep, None], cl[keep, None].astype(np.float32), cov[keep, :1]], 1)
    assert np.array_equal(dets[0, :n].cpu().numpy().view(np.uint32), want.view(np.uint32))
    return keep, order


# n: one wave, one block of 256 candidates +- 1, several LDS tiles; seeds picked on the CPU so the precondition holds
@pytest.mark.parametrize("agnostic", [False, True])
@pytest.mark.parametrize("nc", [1, 15])
@pytest.mark.parametrize("n", [1, 64, 65, 257, 1025, 2049])
def test_fast_nms_matches_float64(n, nc, agnostic):
    keep, order = check_nms(nc, make_rows(n, nc, SEEDS[n]), agnostic=agnostic)
    assert len(order) == n
    if n >= 64 and (agnostic or nc == 1):  # (one class space: the picked inputs have overlapping pairs)
        assert len(keep) < n


SEEDS = {1: 0, 64: 0, 65: 2, 257: 0, 1025: 2, 2049: 22}


def test_more_keepers_than_max_det():
    keep, order = check_nms(15, make_rows(257, 15, SEEDS[257]), max_det=10)
    assert len(keep) == 10 and len(order) == 257


def test_equal_scores_go_by_anchor():
    keep, order = check_nms(15, make_rows(65, 15, SEEDS[65], logit=1.0))
    assert (np.diff(order) > 0).all()


def test_max_nms_cut_and_small_max_wh():
    """max_nms below the candidates; max_wh 64 < the image: classes overlap, every pair is evaluated with its offset."""
    check_nms(15, make_rows(257, 15, SEEDS[257]), max_nms=100)
    check_nms(15, make_rows(257, 15, SEEDS[257]), max_wh=64.0)


def test_chain_drops_c():
    """24 px squares on neighbouring stride-8 cells, scores A > B > C: probiou 0.608 at 8 px, 0.302 at 16 px.  At iou 0.5
    A suppresses B, B (suppressed or not) suppresses C, A does not reach C: Fast-NMS keeps A alone, greedy NMS A and C."""
    rows = make_rows(0, 15, 0)
    for i, lg in enumerate((2.0, 1.5, 1.0)):
        rows[0, 500 + i, :64] = np.tile(bins(np.array([1.5])), 4)
        rows[0, 500 + i, 64 + 3] = lg
    keep, order = check_nms(15, rows)
    assert order.tolist() == [500, 501, 502] and keep.tolist() == [500]


def test_decode_against_float64_and_detect_scores():
    rows = make_rows(257, 15, 3, dmax=7.5)
    eng = model(15).model.engine
    eng.obb_nms(torch.from_numpy(rows).to(DEV), S, S)
    boxes, cov, sc, cl = (t[0].numpy() for t in eng.obb_decoded(1, S, S))
    ref, rs, rc = oo.decode(rows[0].astype(np.float64), S, S, 15, 16)
    assert np.abs(boxes - ref[:, :4]).max() <= TOL_EXACT_XY
    got = oo.corners(np.concatenate([boxes, cov[:, :1]], 1).astype(np.float64))
    assert np.abs(got - oo.corners(ref)).max() <= TOL_EXACT_XY
    A_, B_, C_ = oo.covariance(ref[:, 2], ref[:, 3], ref[:, 4])
    # (A, B, C): sums and differences of a', b' <= 19,200: within ~100 fp32 ulps (6e-8 each) of the larger one
    bound = 1e-5 * (ref[:, 2] ** 2 + ref[:, 3] ** 2) / 12 + 1e-6
    assert (np.abs(cov[:, 1:] - np.stack([A_, B_, C_], 1)).max(1) <= bound).all()
    assert (cl == rc).all() and np.abs(sc - rs).max() <= 1e-6
    # the same logits through a detect plan's decode (an nc = 16 detect model shares the 16-channel class slice):
    # candidate keys = score bits << 32 | ~anchor, equal bit for bit
    det = _detect16()
    x = torch.from_numpy(uniform(5, 3 * 64 * 64).astype(np.float32).reshape(1, 3, 64, 64)).to(DEV)
    m16 = model(16, "f32").model.engine
    keys = []
    for e in (det, m16):
        e.run(x, conf=0.05)
        torch.cuda.synchronize()
        head = e.read_buffer(e.graph.anchor_buf.id, 1)[0, 0, :, :80]
        keys.append((head, sorted(_keys(e, 64))))
    assert torch.equal(keys[0][0], keys[1][0]), "the two f32 plans' head logits differ: nothing to compare"
    assert len(keys[0][1]) > 0 and keys[0][1] == keys[1][1]


def _detect16():
    from yolomi.engine import Engine
    sd = {k: v for k, v in synth_weights("n", "obb", 0, nc=16).items() if ".cv4." not in k}
    return Engine("n", "detect", sd, DEV, "f32", nc=16)


def _keys(eng, size):
    from yolomi.arch import num_anchors
    from yolomi.lib import SCRATCH_KEYS
    n = eng.candidate_counts(1)[0]
    k = torch.empty((1 << (num_anchors(size, size) - 1).bit_length(),), dtype=torch.int64)
    eng.rt.read_scratch(SCRATCH_KEYS, k.data_ptr(), k.numel() * 8)
    return k[:n].tolist()


def hull_rows(r):
    """(n, 7) [cx cy w h conf cls theta] -> (n, 6) [x1 y1 x2 y2 conf cls] of the corners' hull, and the corners."""
    c = oo.corners(r[:, [0, 1, 2, 3, 6]])
    return np.concatenate([c.min(1), c.max(1), r[:, 4:6]], 1), c


@pytest.mark.parametrize("dtype", ["x3", "f16"])
def test_predict_end_to_end(dtype):
    """f16: the throughput plan at its own bar (tests/test_gpu_pose.py test_f16_pose_plan): 1 px / 1e-2, 90 % matched."""
    x = torch.from_numpy(uniform(7, 2 * 3 * 128 * 160).astype(np.float32).reshape(2, 3, 128, 160))
    if "ref" not in _cache:
        o = oo.ObbOracle("n", synth_weights("n", "obb", 0))
        _cache["ref"] = (o.predict(x), o.predict(x, exact=True))
    res = model(15, dtype).predict(x.to(DEV))
    rep, rex, total = MatchReport(), MatchReport(), 0
    for ref, ex, r in zip(*_cache["ref"], res):
        assert r.boxes is None and r.obb is not None
        d = r.obb.data.cpu().numpy()
        got, gc = hull_rows(d[:, [0, 1, 2, 3, 5, 6, 4]])
        assert np.abs(r.obb.xyxyxyxy.cpu().numpy() - gc).max() <= 1e-3  # the view's corners are these rows' corners
        (rh, rc), (eh, ec) = hull_rows(ref.astype(np.float64)), hull_rows(ex)
        total += len(ref)
        x3 = dtype == "x3"
        one = match_image(rh, got, 0.25, 0.7, ref_f64_slack(rh, eh, TOL_XY) if x3 else 1.0, TOL_S if x3 else 1e-2,
                          rep=MatchReport())
        if x3:
            match_image(eh, got.astype(np.float64), 0.25, 0.7, TOL_EXACT_XY, TOL_S, rep=rex)
            assert one.ok, one.failures[:3]
            for i, j in one.pairs:  # corners: within 1e-3 px beyond the fp32 oracle's own distance from float64
                k = np.abs(ec - rc[i]).reshape(len(ec), -1).max(1).argmin() if len(ec) else None
                slack = np.abs(ec[k] - rc[i]).max() if k is not None else 0.0
                assert np.abs(gc[j] - rc[i]).max() <= TOL_XY + slack
        rep.matched, rep.exempt = rep.matched + one.matched, rep.exempt + one.exempt
    print(f"obb {dtype}: {rep}; vs float64: {rex}")
    assert total > 0 and rep.matched + rep.exempt >= (1.0 if dtype == "x3" else 0.9) * total
    if dtype == "x3":
        assert rex.ok and rex.matched > 0, rex.failures[:3]


def test_graph_replays_equal_eager():
    eng = model(15).model.engine
    x = torch.from_numpy(uniform(9, 2 * 3 * 64 * 96).astype(np.float32).reshape(2, 3, 64, 96)).to(DEV)
    d, c = eng.run(x, conf=0.05, use_graph=False)
    want = (d.clone(), c.clone())
    assert int(want[1].sum()) > 0
    for _ in range(3):
        d, c = eng.run(x, conf=0.05, use_graph=True)
        assert torch.equal(c, want[1]) and torch.equal(d.view(torch.int32), want[0].view(torch.int32))


def test_refusals():
    from yolomi.lib import YMError
    m = model(15)
    x = torch.zeros((1, 3, 64, 64), device=DEV)
    with pytest.raises(YMError):
        m.model.engine.run(x, multi_label=True)
    for call in (lambda: m.track(x), lambda: m.val(data=None), lambda: m.embed(x), lambda: m.predict(x)[0].plot(),
                 lambda: m.predict(x)[0].to_coco(), lambda: m.model.engine.run_tta(x)):
        with pytest.raises((NotImplementedError, ValueError)):
            call()
