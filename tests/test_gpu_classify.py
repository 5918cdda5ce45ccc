"""GPU tests of classification (MI355X): the classify plan and its head (csrc/ym_classify.hip: conv + SiLU + mean,
Linear, softmax + top-k) through Engine.classify, against float64 references formed from the GPU's own layer 9 (pooled
vector), its own pooled vector (logits) and its own logits (probs, top-k); the logits end to end against the float64
oracle; the facade.  The bounds are worst cases built from tests/conv_oracle.py's constants and the chain lengths of
the kernel header (tests/classify_oracle.py k_pool, K_LIN, k_sm), none of them measured on the kernels.

End to end (yolo11n, 224x224, B = 2 U[0,1) images): e32, the fp32 CPU oracle's own relative L2 distance from float64, is
2.3e-7 to 3.7e-7 (it moves with the host's thread count), so 8 * e32 is below the stored-layer bars and those hold:
1e-4 (x3, f32), 1e-2 (f16).
"""
import pytest
import torch

from tests import classify_oracle as CO
from tests.conv_oracle import C_OUT, MARGIN, tol_cap
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
DTYPES = ("x3", "f16", "f32")
# (scale, nc, H, W, B): P = 1; P = 15 under one MFMA tile, nc odd and under one class tile; P = 49, a tile and a tail;
# K = 512, P = 35, k = 2; P = 90: a second 64-pixel pass of the pooling kernel, B = 9: a second image group of the
# Linear
CASES = [("n", 1000, 32, 32, 5), ("n", 37, 96, 160, 3), ("n", 1000, 224, 224, 2), ("s", 2, 160, 224, 1),
         ("n", 37, 320, 288, 9)]
LAYER_BAR = {"x3": 1e-4, "f32": 1e-4, "f16": 1e-2}  # tests/test_gpu_x3.py, tests/test_gpu_parity.py
_cache = {}


def weights(scale, nc):
    if ("sd", scale, nc) not in _cache:
        _cache[("sd", scale, nc)] = synth_weights(scale, "classify", 0, nc=nc)
    return _cache[("sd", scale, nc)]


def engine(scale, nc, dtype):
    from yolomi.engine import Engine
    k = ("eng", scale, nc, dtype)
    if k not in _cache:
        e = _cache[k] = Engine(scale, "classify", weights(scale, nc), DEV, dtype, nc=nc)
        e.autotune = False  # heuristic tiles: no tuning runs inside the tests
    return _cache[k]


def oracle(dtype):
    """(logits, top-1) of the end-to-end images from the CPU oracle in `dtype`, computed once."""
    if ("ref", dtype) not in _cache:
        x = CO.cls_input(2, 224, 224).to(dtype)
        logits, _ = CO.build_cls("n", weights("n", 1000), 1000, dtype)(x)
        _cache[("ref", dtype)] = logits.double()
    return _cache[("ref", dtype)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("scale,nc,H,W,B", CASES, ids=[f"{c[0]}-nc{c[1]}-{c[2]}x{c[3]}-b{c[4]}" for c in CASES])
def test_head_kernels(scale, nc, H, W, B, dtype):
    eng, sd = engine(scale, nc, dtype), weights(scale, nc)
    eng.logits = torch.empty((B, nc), dtype=torch.float32, device=DEV)
    probs, topk, conf = (t.cpu() for t in eng.classify(CO.cls_input(B, H, W).to(DEV), use_graph=False))
    logits, pooled = eng.logits.cpu(), eng.pooled(B)
    v = eng.graph.layer_views(9)[0]
    feat = eng.read_buffer(v.buf.id, B)[..., v.coff:v.coff + v.C]
    P, c1, k = (H // 32) * (W // 32), v.C, min(5, nc)
    assert feat.shape == (B, H // 32, W // 32, {"n": 256, "s": 512}[scale])
    # 1. the pooled vector against the float64 head of the stored layer 9
    ref, A = CO.head64(feat, sd)
    bound = (tol_cap(dtype, c1) * A + C_OUT[dtype] * ref.abs()).mean(1) + (CO.k_pool(P) + 1) * U * ref.abs().mean(1)
    err = (pooled.double() - ref.mean(1)).abs()
    print(f"pooled: max err / bound {float((err / bound).max()):.3f}")
    assert bool((err <= bound).all())
    # 2. the logits against the float64 Linear of the GPU's own pooled vector
    lref, S, babs = CO.linear64(pooled, sd)
    lbound = (CO.K_LIN + 2) * U * (S + babs) + (2.0 ** -11 * S if dtype == "f16" else 0.0)
    lerr = (logits.double() - lref).abs()
    print(f"logits: max err / bound {float((lerr / lbound).max()):.3f}")
    assert bool((lerr <= lbound).all())
    # 3. the probabilities against the float64 softmax of the GPU's own logits
    pref = torch.softmax(logits.double(), 1)
    pb = (CO.k_sm(nc) + 6) * U
    print(f"probs: max rel err / bound {float(((probs.double() - pref).abs() / pref).max() / pb):.3f}")
    assert bool(((probs.double() - pref).abs() <= pb * pref).all())
    assert bool(((probs.double().sum(1) - 1.0).abs() <= pb).all())
    # 4. top-k: a stable descending sort of the GPU's own probabilities, ties to the lower class, exact
    order = torch.sort(probs, dim=1, descending=True, stable=True).indices[:, :k]
    assert topk.shape == (B, k) and torch.equal(topk.long(), order)
    assert torch.equal(conf, torch.gather(probs, 1, order))


@pytest.mark.parametrize("dtype", DTYPES)
def test_logits_end_to_end(dtype):
    eng = engine("n", 1000, dtype)
    eng.logits = torch.empty((2, 1000), dtype=torch.float32, device=DEV)
    _, topk, _ = eng.classify(CO.cls_input(2, 224, 224).to(DEV))
    ref, ref32 = oracle(torch.float64), oracle(torch.float32)
    rel = lambda t: (t.double() - ref).norm(dim=1) / ref.norm(dim=1)  # noqa: E731
    e32, got = rel(ref32), rel(eng.logits.cpu())
    print(f"{dtype}: rel L2 {got.tolist()}, fp32 oracle {e32.tolist()}")
    assert bool((got <= torch.clamp(MARGIN * e32, min=LAYER_BAR[dtype])).all())
    assert torch.equal(topk[:, 0].cpu().long(), ref.argmax(1))


def test_facade_and_refusals():
    from core.model import YOLO11Factory, YOLO11Model
    from core.results import Probs
    from yolomi.lib import YMError, Runtime
    sd = weights("n", 1000)
    m = YOLO11Model(state_dict=sd, device="cuda:0", verbose=False)
    m2 = YOLO11Factory.create_classifier("s", state_dict=sd, device="cuda:0", verbose=False)
    assert m.task == m2.task == "classify" and m2.size == "n"
    eng = m.model.engine
    eng.autotune = False
    x = CO.cls_input(2, 224, 224).to(DEV)
    det = YOLO11Model(task="detect", size="n", device="cuda:0", verbose=False)
    det.model.engine.autotune = False
    rows_before = [r.boxes.data.clone() for r in det.predict(x)]
    res = m.predict(x, conf=0.5)
    probs, topk, conf = (t.clone() for t in eng.classify(x))
    assert all(isinstance(r.probs, Probs) and r.boxes is None and r.masks is None and r.keypoints is None for r in res)
    assert torch.equal(torch.stack([r.probs.data for r in res]), probs)
    assert [r.probs.top5 for r in res] == topk.tolist() and res[0].probs.top1 == int(topk[0, 0])
    assert torch.equal(torch.stack([r.probs.top5conf for r in res]), conf)
    host = res[0].cpu().probs  # the top-k moves with the data
    assert not host.top5conf.is_cuda and host.top5 == res[0].probs.top5 and len(res[0]) == 1000
    for _ in range(10):  # replays of the captured forward, then one eager call: bit-identical
        assert all(torch.equal(a, b) for a, b in zip(eng.classify(x), (probs, topk, conf)))
    assert all(torch.equal(a, b) for a, b in zip(eng.classify(x, use_graph=False), (probs, topk, conf)))
    emb = m.embed(x)
    assert len(emb) == 2 and emb[0].shape == (256,)
    # the C entry's refusals
    args, st = Runtime.make_args(), eng._stream()
    call = lambda rt, p, ld: rt.classify(x.data_ptr(), 2, 224, 224, args, p, ld, 0, topk.data_ptr(), conf.data_ptr(), st)  # noqa: E731
    for rt, p, ld, words in ((eng.rt, 0, 1000, "null pointer"), (eng.rt, probs.data_ptr(), 999, "row stride"),
                             (det.model.engine.rt, probs.data_ptr(), 1000, "not a classify plan")):
        with pytest.raises(YMError, match=words):
            call(rt, p, ld)
    with pytest.raises(YMError, match="classify plan has no detections"):
        eng.run(x)
    assert all(torch.equal(a, r.boxes.data) for a, r in zip(rows_before, det.predict(x)))
