"""GPU tests of test-time augmentation (MI355X): `predict(augment=True)` / `val(augment=True)` / `Engine.run_tta`
(csrc/ym_tta.hip: the scaled views and the merge of the three passes' candidates; the existing NMS kernels over the
merged set) against tests/tta_oracle.py, the CPU restatement of Ultralytics DetectionModel._predict_augment.

Parity protocol: tests/matching.py at the project's bars — f32 plan 1e-3 score, x3 plan 5e-5 score, both plans
coordinates within 1e-3 px beyond the fp32 oracle's own distance from the float64 TTA oracle (ref_f64_slack); no
unmatched detection on either side; at most 5 % of the reference's detections exempt (merging three passes creates more
same-class near-ties at the NMS threshold than the plain tests' 2 % allows for).

Share of the oracle's own detections that the exemption rules (conf margin, IoU margin, max_det cut) cover, measured on
the CPU oracle alone (yolo11n synthetic weights; 320 = make_input("uniform", (1, 2), 320), 96x160 = torch.rand seed 7):
    single-label  320    conf 0.25                      9 of 261   3.4 %
                  96x160 conf 0.25                      0 of  46   0 %
                  320    conf 0.02 classes 0,17,45,79  10 of 441   2.3 %
                  320    conf 0.25 agnostic             3 of 180   1.7 %
                  320    conf 0.05 (max_det 300 cuts)  42 of 600   7.0 %   (5 % without the cut rule's near-cut scores)
                  640    conf 0.001 B=1 (cut at 300)   16 of 300   5.3 %
    multi-label   320    conf 0.05 / 0.001, max_det 300: 38 of 600, 6.3 %;  max_det 50: 4 of 100, 4.0 %
The cases above 5 % are the ones the feature's specification names (320 at conf 0.05; multi-label at 320 for conf 0.05
and 0.001; the presort case at 640, conf 0.001): they run under the same bars and the same 5 % cap on the detections
that actually end up exempt.
"""
import os

import numpy as np
import pytest
import torch

from oracle.predict import OracleModel
from tests import tta_oracle as T
from tests.golden.make_golden import make_input
from tests.matching import MatchReport, match_image, ref_f64_slack
from yolomi import tta
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CLASSES = [0, 17, 45, 79]
EXEMPT_CAP = 0.05

_cache = {}


def oracle():
    if "o" not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _cache["o"] = OracleModel("n", "detect", synth_weights("n", "detect", 0))
    return _cache["o"]


def model(dtype="f32", task="detect"):
    from core.model import YOLO11Model
    k = ("m", dtype, task)
    if k not in _cache:
        m = _cache[k] = YOLO11Model(task=task, size="n", device="cuda:0", dtype=dtype, verbose=False)
        m.model.engine.autotune = False  # heuristic tiles: no tuning runs inside the tests
    return _cache[k]


def inputs(name):
    if ("x", name) not in _cache:
        _cache[("x", name)] = {
            "320": lambda: make_input("uniform", (1, 2), 320),
            "96x160": lambda: torch.rand(2, 3, 96, 160, generator=torch.Generator().manual_seed(7)),
            "640": lambda: make_input("uniform", (1,), 640),
        }[name]()
    return _cache[("x", name)]


def heads(name):
    """(fp32, float64) merged TTA heads of the oracle on a shared input: computed once."""
    k = ("y", name)
    if k not in _cache:
        x = inputs(name)
        _cache[k] = (T.merged_head(oracle(), x), T.merged_head(oracle(), x, torch.float64))
    return _cache[k]


def rows_of(results):
    out = []
    for r in results:
        b = r.boxes
        out.append(torch.cat([b.xyxy, b.conf[:, None], b.cls[:, None]], 1).cpu().numpy())
    return out


def check(ref, exact, got, conf, tol_s, max_det=300, what=""):
    rep = MatchReport()
    for b in range(len(ref)):
        match_image(ref[b], got[b], conf, 0.7, ref_f64_slack(ref[b], exact[b], 1e-3), tol_s, rep=rep, max_det=max_det)
    total = sum(len(r) for r in ref)
    print(f"{what}: kept gpu {[len(g) for g in got]} oracle {[len(r) for r in ref]}; {rep}")
    assert rep.ok, f"{rep}; {rep.failures[:3]}"
    assert rep.matched > 0 and rep.exempt <= EXEMPT_CAP * total, rep
    return rep


TOL_S = {"f32": 1e-3, "x3": 5e-5}


# ------------------------------------------------------------------------------------------------ 1. scaled view
@pytest.mark.parametrize("shape", [(1, 3, 32, 32), (2, 3, 96, 160), (1, 3, 320, 320)])
@pytest.mark.parametrize("hi", [1.0, 255.0])
def test_scaled_view_against_torch(shape, hi):
    """Bound 8 * 2^-24 * M, M = 1 after normalisation: seven fp32 roundings in the four-tap sum, each at most half an
    ulp of a value <= M, doubled for FMA contraction on either side.  Pad cells are bit-equal to float32(0.447)."""
    eng = model().model.engine
    B, _, H, W = shape
    x = torch.rand(shape, generator=torch.Generator().manual_seed(11)) * hi
    if hi > 1:
        x = x.round()
    xd = x.to(DEV).contiguous()
    bm = eng.input_max(xd)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    eps = torch.finfo(torch.float32).eps
    xn = x / 255 if hi > 1 else x
    shapes = tta.pass_shapes(H, W)
    for p in (1, 2):
        Hs, Ws, hc, wc = shapes[p]
        for flip in (False, True):
            # the library mirrors pass 1 only: the other combination is the same kernel on the mirrored input
            src = xd if flip == tta.FLIPS[p] else xd.flip(3).contiguous()
            out = torch.full((B, 3, Hs, Ws), -1.0, device=DEV)
            eng.rt.tta_scale(src.data_ptr(), B, H, W, p, bm.data_ptr(), eps, out.data_ptr(), stream)
            torch.cuda.synchronize()
            ref = T.scale_img(xn.flip(3) if flip else xn, tta.RATIOS[p])
            assert tuple(ref.shape) == tuple(out.shape)
            got = out.cpu()
            err = (got[..., :hc, :wc] - ref[..., :hc, :wc]).abs().max().item()
            print(f"scaled view {shape} x{hi} pass {p} flip {flip}: max err {err * 2 ** 24:.2f} * 2^-24")
            assert err <= 8 * 2.0 ** -24
            pad = torch.tensor(0.447, dtype=torch.float32)
            assert (got[..., hc:, :] == pad).all() and (got[..., :, wc:] == pad).all()


def test_library_and_python_agree_on_the_pass_shapes():
    import ctypes
    from yolomi.lib import load_library
    lib = load_library()
    for H, W in ((640, 640), (320, 320), (96, 160), (32, 32), (384, 1280)):
        for p, want in enumerate(tta.pass_shapes(H, W)):
            v = [ctypes.c_int() for _ in range(4)]
            assert lib.ym_tta_shape(H, W, p, *[ctypes.byref(t) for t in v]) == 0
            assert tuple(t.value for t in v) == want, (H, W, p)
    assert lib.ym_tta_shape(100, 320, 1, None, None, None, None) < 0


# ------------------------------------------------------------------------------------------------ 2. precondition
@pytest.mark.parametrize("name", ["320", "96x160"])
def test_plain_forward_at_the_scaled_shapes(name):
    """Plain Engine.run on the CPU-made scaled inputs (288², 224², 96x128, and the mirrored 96x160) against the plain
    oracle at the f32 plan's bars: a failure here is a forward problem at a new map width, not a TTA problem."""
    eng = model().model.engine
    for xi in T.pass_inputs(inputs(name))[1:]:
        ref = oracle().predict(xi, conf=0.25)
        d, c = eng.run(xi.contiguous().to(DEV), conf=0.25)
        rep = MatchReport()
        for b, r in enumerate(ref):
            match_image(r["boxes"].numpy(), d[b, :int(c[b])].cpu().numpy(), 0.25, 0.7, 1e-3, 1e-3, rep=rep)
        print(f"plain forward at {tuple(xi.shape)}: {rep}")
        assert rep.ok, f"{tuple(xi.shape)}: {rep}; {rep.failures[:3]}"


# ------------------------------------------------------------------------------------------------ 3, 4. single label
SINGLE = [("320", 0.25, {}), ("320", 0.05, {}), ("96x160", 0.25, {}),
          ("320", 0.02, dict(classes=CLASSES)), ("320", 0.25, dict(agnostic_nms=True))]


@pytest.mark.parametrize("dtype", ["f32", "x3"])
@pytest.mark.parametrize("name, conf, kw", SINGLE, ids=[f"{n}-{c}-{'-'.join(k) or 'all'}" for n, c, k in SINGLE])
def test_predict_augment_parity(dtype, name, conf, kw):
    x = inputs(name)
    y, y64 = heads(name)
    okw = {("agnostic" if k == "agnostic_nms" else k): v for k, v in kw.items()}
    ref = T.nms_rows(y, tuple(x.shape[2:]), conf=conf, **okw)
    exact = T.nms_rows(y64, tuple(x.shape[2:]), conf=conf, **okw)
    plain = [p["boxes"].numpy() for p in oracle().predict(x, conf=conf, **kw)]
    # the augmented answer is not the plain one: what makes this test fail where `augment` is ignored
    assert any(len(r) != len(p) or not np.allclose(r, p, atol=1e-2) for r, p in zip(ref, plain))
    got = rows_of(model(dtype).predict(x, conf=conf, augment=True, **kw))
    check(ref, exact, got, conf, TOL_S[dtype], what=f"tta {dtype} {name} conf {conf} {kw}")


def test_f16_plan_runs_augmented():
    """The throughput plan is not a parity plan (~0.6 px / 3e-3 off the fp32 path, which moves a few
    percent of near-threshold decisions): at 1 px / 1e-2 at least 90 % of the oracle's detections must be found."""
    x = inputs("320")
    ref = T.nms_rows(heads("320")[0], (320, 320), conf=0.25)
    got = rows_of(model("f16").predict(x, conf=0.25, augment=True))
    rep = MatchReport()
    for r, g in zip(ref, got):
        match_image(r, g, 0.25, 0.7, 1.0, 1e-2, rep=rep)
    print(f"tta f16 320 conf 0.25: kept gpu {[len(g) for g in got]} oracle {[len(r) for r in ref]}; {rep}")
    assert rep.matched >= 0.9 * sum(len(r) for r in ref), rep


# ------------------------------------------------------------------------------------------------ 5. multi label
@pytest.mark.parametrize("dtype", ["f32", "x3"])
@pytest.mark.parametrize("conf, max_det", [(0.05, 300), (0.001, 300), (0.05, 50)])
def test_run_tta_multi_label_parity(dtype, conf, max_det):
    x = inputs("320")
    y, y64 = heads("320")
    cnt = []
    ref = T.multi_label_nms(y, conf=conf, iou=0.7, max_det=max_det, max_nms=30000, img_shape=(320, 320), counts=cnt)
    exact = T.multi_label_nms(y64, conf=conf, iou=0.7, max_det=max_det, max_nms=30000, img_shape=(320, 320))
    eng = model(dtype).model.engine
    d, c = eng.run_tta(x.to(DEV), conf=conf, iou=0.7, max_det=max_det, multi_label=True)
    torch.cuda.synchronize()
    n = c[:2].tolist()
    got = [d[b, :n[b]].cpu().numpy() for b in range(2)]
    pairs = eng.tta_candidate_counts(2)
    print(f"multi-label tta {dtype} conf {conf}: pairs gpu {pairs} oracle {cnt}")
    if conf == 0.05:  # about 9.4 k and 10.1 k pairs: no cut
        assert all(5000 < p <= 30000 for p in pairs), pairs
    else:  # about 312 k pairs per image, cut to 30,000
        assert all(p > 200000 for p in pairs), pairs
    if dtype == "f32":
        assert all(abs(p - q) <= 0.001 * q for p, q in zip(pairs, cnt)), (pairs, cnt)
    check(ref, exact, got, conf, TOL_S[dtype], max_det=max_det, what=f"tta multi-label {dtype} conf {conf}")


# ------------------------------------------------------------------------------------------------ 6. presort branch
def test_presort_branch_at_640():
    """15,049 merged anchors give a key stride of 16,384, and conf 0.001 < kPresortConf: the merged single-label NMS
    takes ym_launch_nms_presort (every merged anchor is a candidate at this conf, so 512 < n <= 16,384)."""
    x = inputs("640")
    y, y64 = heads("640")
    assert y.shape[-1] == 15049
    ref = T.nms_rows(y, (640, 640), conf=0.001)
    exact = T.nms_rows(y64, (640, 640), conf=0.001)
    m = model()
    got = rows_of(m.predict(x, conf=0.001, augment=True))
    n = m.model.engine.tta_candidate_counts(1)
    assert 512 < n[0] <= 16384, n
    check(ref, exact, got, 0.001, 1e-3, what="tta presort 640 conf 0.001")


# ------------------------------------------------------------------------------------------------ 7. exact properties
def _run(eng, x, **kw):
    B = x.shape[0]
    d, c = eng.run_tta(x, **kw)
    torch.cuda.synchronize()
    return d[:B].clone(), c[:B].clone()


def test_identical_calls_and_batch_one():
    eng = model().model.engine
    x = inputs("320").to(DEV)
    d1, c1 = _run(eng, x, conf=0.25)
    d2, c2 = _run(eng, x, conf=0.25)
    assert torch.equal(c1, c2) and min(c1.tolist()) > 0
    for b in range(2):
        assert torch.equal(d1[b, :int(c1[b])], d2[b, :int(c2[b])])
    # B = 1 (its convs may take other tiles than the B = 2 batch's, so its rows are held to the oracle, not to d1)
    x1 = inputs("320")[:1]
    d3, c3 = _run(eng, x1.to(DEV).contiguous(), conf=0.25)
    y, y64 = (h[:1] for h in heads("320"))  # (per-image: U[0, 1) inputs, no batch-wide /255 decision)
    check(T.nms_rows(y, (320, 320), conf=0.25), T.nms_rows(y64, (320, 320), conf=0.25),
          [d3[0, :int(c3[0])].cpu().numpy()], 0.25, 1e-3, what="tta B=1")


def test_lanes_bitwise_equal_at_b8():
    eng = model().model.engine
    x = make_input("uniform", tuple(range(1, 9)), 320).to(DEV)
    d0, c0 = _run(eng, x, conf=0.25)
    assert min(c0.tolist()) > 0
    for lanes in (1, 2, 4):
        d1, c1 = _run(eng, x, conf=0.25, lanes=lanes)
        assert torch.equal(c0, c1), lanes
        for b in range(8):
            assert torch.equal(d0[b, :int(c0[b])], d1[b, :int(c1[b])]), (lanes, b)


def test_augment_false_is_todays_path():
    m = model()
    x = inputs("320")
    a = rows_of(m.predict(x, conf=0.25))
    b = rows_of(m.predict(x, conf=0.25, augment=False))
    m.predict(x, conf=0.25, augment=True)
    c = rows_of(m.predict(x, conf=0.25))  # and an augmented call in between leaves the plain path as it was
    assert all(np.array_equal(p, q) and np.array_equal(p, r) for p, q, r in zip(a, b, c))
    t = rows_of(m.predict(x, conf=0.25, augment=True))
    assert [len(r) for r in t] != [len(r) for r in a]


@pytest.mark.parametrize("task", ["segment", "pose"])
def test_segment_and_pose_ignore_augment(task, caplog):
    import logging
    m = model("f32", task)
    x = inputs("320")
    a = m.predict(x, conf=0.25)
    with caplog.at_level(logging.WARNING):
        b = m.predict(x, conf=0.25, augment=True)
    assert any("augment" in r.getMessage() for r in caplog.records)
    for p, q in zip(a, b):
        assert torch.equal(p.boxes.data, q.boxes.data)
        if task == "segment":
            assert (p.masks is None and q.masks is None) or torch.equal(p.masks.data, q.masks.data)
        else:
            assert torch.equal(p.keypoints.data, q.keypoints.data)
    with pytest.raises(Exception, match="detect"):
        m.model.engine.run_tta(x.to(DEV))


# ------------------------------------------------------------------------------------------------ 8. steady state
def test_steady_state_keeps_workspaces_and_tables():
    eng = model().model.engine
    x = inputs("320").to(DEV)
    for _ in range(2):
        eng.run_tta(x, conf=0.25)
    torch.cuda.synchronize()
    engines = eng._tta_engines()
    assert len(engines) == 3 and engines[0] is eng and len({id(e.rt) for e in engines}) == 3
    ab = eng.graph.anchor_buf.id
    before = [(e.rt.buffer_info(ab), set(e._tuned)) for e in engines]
    shapes = tta.pass_shapes(320, 320)
    for e, (info, _), s in zip(engines, before, shapes):
        assert info[3] == tta.num_anchors(s[0], s[1])  # every pass's own workspace shape, all three at once
    mem = torch.cuda.memory_allocated(DEV)
    for _ in range(3):
        eng.run_tta(x, conf=0.25)
    torch.cuda.synchronize()
    after = [(e.rt.buffer_info(ab), set(e._tuned)) for e in engines]
    assert after == before
    assert torch.cuda.memory_allocated(DEV) == mem


# ------------------------------------------------------------------------------------------------ 9. image sources
def test_image_sources():
    from yolomi.preprocess import scale_boxes
    m = model()
    rng = np.random.default_rng(3)
    imgs = [rng.integers(0, 256, (240, 320, 3), dtype=np.uint8), rng.integers(0, 256, (200, 150, 3), dtype=np.uint8)]
    res = m.predict(imgs, conf=0.25, augment=True, imgsz=320)
    im, eps, src = m._as_batch(imgs, 320)
    eng = m.model.engine
    d, c = _run(eng, im, conf=0.25, in_eps=eps)
    plain = m.predict(imgs, conf=0.25, imgsz=320)
    assert [len(r.boxes) for r in res] != [len(r.boxes) for r in plain]
    for b, r in enumerate(res):
        n = int(c[b])
        want = d[b, :n].clone()
        if n:
            scale_boxes(im.shape[2:], want[:, :4], src[2][b])
        assert len(r.boxes) == n and n > 0
        assert torch.equal(r.boxes.data[:, :6], want[:, :6])
        assert tuple(r.orig_shape) == imgs[b].shape[:2]


# ------------------------------------------------------------------------------------------------ 10. validation
def _write_dataset(root, shapes, seed=5):
    from PIL import Image
    rng = np.random.default_rng(seed)
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    os.makedirs(os.path.join(root, "labels"), exist_ok=True)
    imgs = []
    for i, (h, w) in enumerate(shapes):
        rgb = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        Image.fromarray(rgb).save(os.path.join(root, "images", f"im{i}.png"))
        imgs.append(np.ascontiguousarray(rgb[..., ::-1]))
    return imgs


def test_val_augment_end_to_end(tmp_path):
    """Labels = the model's own augmented single-label detections at conf 0.25 on the val batches; val(augment=True)
    must return exactly metrics.evaluate of Engine.run_tta(multi_label=True) on the same rect batches, and differ from
    the plain val()."""
    from core.validator import YOLO11Validator
    from yolomi import val as V
    from yolomi.metrics import evaluate
    m = model()
    eng = m.model.engine
    shapes, imgsz = [(320, 320), (240, 320), (320, 240), (320, 320)], 320
    root = str(tmp_path / "ds")
    imgs = _write_dataset(root, shapes)
    batches = V.build_batches(shapes, imgsz, 2)
    n_labels = 0
    for b in batches:
        x = V.make_batch(eng, [imgs[i] for i in b["indices"]], b)
        d, c = eng.run_tta(x, conf=0.25)
        d, c = d.cpu().numpy(), c.tolist()
        for k, i in enumerate(b["indices"]):
            h0, w0 = shapes[i]
            r = V.to_native(d[k, :c[k], :6], b["geo"][k], b["gain"][k], shapes[i])
            with open(os.path.join(root, "labels", f"im{i}.txt"), "w") as f:
                for x1, y1, x2, y2, _, cl in r:
                    v = [(x1 + x2) / 2 / w0, (y1 + y2) / 2 / h0, (x2 - x1) / w0, (y2 - y1) / h0]
                    f.write(f"{int(cl)} " + " ".join(repr(float(t)) for t in v) + "\n")
                    n_labels += 1
    assert n_labels >= 1
    res = m.val(data=root, imgsz=imgsz, batch=2, augment=True)
    ds = V.load_dataset(root)
    preds, gts = [None] * len(ds), [None] * len(ds)
    for b in batches:
        x = V.make_batch(eng, [imgs[i] for i in b["indices"]], b)
        d, c = eng.run_tta(x, conf=0.001, iou=0.7, max_det=300, multi_label=True)
        d, c = d.cpu().numpy(), c.tolist()
        for k, i in enumerate(b["indices"]):
            preds[i] = V.to_native(d[k, :c[k], :6], b["geo"][k], b["gain"][k], shapes[i])
            gts[i] = V.labels_to_native(ds.labels[i], shapes[i])
    want = evaluate(preds, gts)
    assert (res.box.map50, res.box.map75, res.box.map) == (want["map50"], want["map75"], want["map"])
    assert (res.box.mp, res.box.mr) == (want["precision"], want["recall"])
    assert res.box.map50 > 0
    plain = m.val(data=root, imgsz=imgsz, batch=2)
    assert (plain.box.map50, plain.box.map) != (res.box.map50, res.box.map)
    v = YOLO11Validator(m, device="cuda:0", output_dir=str(tmp_path / "val_out"))
    out = v.validate(root, imgsz=imgsz, batch=2, conf=0.001, iou=0.7, augment=True)
    assert set(out["box_metrics"]) == {"mAP50-95", "mAP50", "mAP75", "precision", "recall"}
    assert out["box_metrics"]["mAP50"] == want["map50"]
