"""GPU tests of feature embeddings (MI355X): `predict(embed=[...])` / `YOLO11Model.embed` / `Engine.embed` / ym_embed
(csrc/ym_embed.hip: one pooling launch, plus a finishing launch for maps of more than 512 pixels, behind a forward
that stops at the last named layer) against the GPU's own stored layers and against tests/embed_oracle.py.

The kernel bar.  Per (image, channel): |got - ref| <= (k + 2) * 2^-24 * m, ref the float64 mean of the stored fp32
values of that plane (Engine.read_buffer), m the float64 mean of their magnitudes, k the longest chain of dependent
fp32 additions the reduction forms for one output, read off csrc/ym_embed.hip for P pixels, nch = ceil(P / 512):
    per thread      min(16, ceil(min(P, 512) / 32))   pixels p, p + 32, ... of one 512-pixel chunk
    wave            3                                  xor-shuffles over the wave's 8 pixel lanes
    workgroup       2                                  (w0 + w1) + (w2 + w3) in LDS
    finishing       ceil(nch / 8) + 3                  only when nch > 1: chunks j, j + 8, ... per lane, then a 3-level tree
so k = 6 for one pixel (32²: layer 22), 6 for 15 pixels (96x160: layer 22), 13 for 256 pixels (32²: layer 0), 31 for
25,600 pixels (320²: layer 0); never above 64 at a tested shape (asserted).  The + 2 covers the hi + lo join of an x3
value and the one fp32 division by H * W.
"""
import logging
import math
import os

import numpy as np
import pytest
import torch

from tests import embed_oracle as EO
from tests.golden.make_golden import make_input
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
_cache = {}


def k_chain(P: int) -> int:
    """Longest chain of dependent fp32 additions of csrc/ym_embed.hip for one output over P pixels (module docstring)."""
    nch = -(-P // 512)
    k = min(16, -(-min(P, 512) // 32)) + 3 + 2
    if nch > 1:
        k += -(-nch // 8) + 3
    return k


def model(dtype="x3", task="detect"):
    from core.model import YOLO11Model
    k = ("m", dtype, task)
    if k not in _cache:
        m = _cache[k] = YOLO11Model(task=task, size="n", device="cuda:0", dtype=dtype, verbose=False)
        m.model.engine.autotune = False  # heuristic tiles: no tuning runs inside the tests
    return _cache[k]


def inputs(name):
    if ("x", name) not in _cache:
        _cache[("x", name)] = {
            "32": lambda: make_input("uniform", (5,), 32),
            "96x160": lambda: torch.rand(3, 3, 96, 160, generator=torch.Generator().manual_seed(7)),
            "320": lambda: make_input("uniform", (1, 2), 320),
        }[name]()
    return _cache[("x", name)]


def oracle_net(dtype=torch.float32):
    if ("net", dtype) not in _cache:
        from oracle.yolo11 import build
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        net = build("n", "detect", synth_weights("n", "detect", 0))
        _cache[("net", dtype)] = net.double() if dtype == torch.float64 else net
    return _cache[("net", dtype)]


def stored_reference(eng, x, layers):
    """After a plain run of x: per requested layer (ascending) the float64 mean and mean magnitude per (image,
    channel) of the values the plan stores, and the pixel count of every column."""
    from yolomi.arch import normalize_embed
    B = x.shape[0]
    eng.run(x, use_graph=False)
    mean, mag, pix = [], [], []
    for i in normalize_embed(layers):
        for v in eng.graph.layer_views(i):
            t = eng.read_buffer(v.buf.id, B)[..., v.coff:v.coff + v.C].double()  # (B, H, W, C)
            mean.append(t.mean((1, 2)))
            mag.append(t.abs().mean((1, 2)))
            pix += [t.shape[1] * t.shape[2]] * v.C
    return torch.cat(mean, 1), torch.cat(mag, 1), torch.tensor(pix)


def check_kernel(eng, x, layers, what):
    ref, mag, pix = stored_reference(eng, x, layers)
    got = eng.embed(x, layers).double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    k = torch.tensor([k_chain(int(p)) for p in pix.tolist()])
    assert int(k.max()) <= 64
    bound = (k + 2).double() * 2.0 ** -24 * mag
    err = (got - ref).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: {got.shape[1]} columns, pixels {sorted(set(pix.tolist()))}, k {sorted(set(k.tolist()))}, "
          f"max err / bound {worst:.3f}")
    assert torch.isfinite(got).all() and float(mag.max()) > 0
    assert (err <= bound).all(), f"{what}: max err / bound {worst}"


# ------------------------------------------------------------------------------- 1. kernel vs the stored layers
@pytest.mark.parametrize("name", ["32", "96x160"])
@pytest.mark.parametrize("dtype", ["f32", "f16", "x3"])
def test_pooled_means_of_the_stored_layers(dtype, name):
    """32²: layer 22 is one pixel, layer 0 16 x 16.  96 x 160, B = 3: non-square maps, layer 22 is 3 x 5 = 15 pixels.
    Layers 0, 4, 10, 22, the Upsample layer 11 (layer 10's view) and the Concat layer 12 (layer 10's view, then 6's)."""
    eng = model(dtype).model.engine
    check_kernel(eng, inputs(name).to(DEV), [0, 4, 10, 22, 12, 11], f"{dtype} {name}")


@pytest.mark.parametrize("dtype", ["f32", "f16", "x3"])
def test_pooled_mean_spanning_workgroups(dtype):
    """Layer 0 at 320²: 25,600 pixels per image and 16 channels — 50 chunks and the finishing launch."""
    eng = model(dtype).model.engine
    x = inputs("320")[:1].contiguous().to(DEV)
    assert k_chain(160 * 160) == 31
    check_kernel(eng, x, [0], f"{dtype} 320 layer 0")


# ------------------------------------------------------------------------------- 2. against the oracle
@pytest.mark.parametrize("dtype,tol", [("x3", 1e-4), ("f32", 1e-4), ("f16", 1e-2)])
def test_embeddings_match_oracle(dtype, tol):
    """||got_i - ref_i||_2 <= tol * ||layer_i ref||_2 / sqrt(H_i W_i) per image and layer slice: the relative bar the
    stored layers already hold (tests/test_gpu_x3.py, tests/test_gpu_parity.py: 1e-4 for x3 and f32, 1e-2 for f16),
    carried through the mean by Cauchy-Schwarz (|mean e| <= rms e)."""
    layers = [4, 10, 16, 22]
    x = inputs("320")
    if "oref" not in _cache:
        xp = EO.preprocess(x)
        _cache["oref"] = (EO.layer_outputs(oracle_net(), xp, layers), torch.stack(EO.embed(oracle_net(), xp, layers)))
    outs, ref = _cache["oref"]
    got = model(dtype).model.engine.embed(x.to(DEV), layers).cpu()
    assert got.shape == ref.shape
    col = 0
    for i in layers:
        t = outs[i]
        C, hw = t.shape[1], t.shape[2] * t.shape[3]
        for b in range(x.shape[0]):
            d = float((got[b, col:col + C].double() - ref[b, col:col + C].double()).norm())
            bar = tol * float(t[b].double().norm()) / math.sqrt(hw)
            print(f"{dtype} layer {i} image {b}: {d:.3e} (bar {bar:.3e})")
            assert d <= bar, (dtype, i, b, d, bar)
        col += C
    assert col == got.shape[1]


# ------------------------------------------------------------------------------- 3. early stop
@pytest.mark.parametrize("task", ["detect", "segment", "pose"])
def test_embed_stops_early_and_leaves_the_detection_path_alone(task):
    m = model("x3", task)
    eng = m.model.engine
    x = inputs("320").to(DEV)
    B = x.shape[0]
    d0, c0 = (t.clone() for t in eng.run(x))
    cc0 = eng.candidate_counts(B)
    assert sum(cc0) > 0
    dets, counts = eng.outputs(B, 300)
    dets.fill_(-7.25)
    counts.fill_(-12345)
    e1 = eng.embed(x, [22]).clone()
    torch.cuda.synchronize()
    assert bool((dets == -7.25).all()) and bool((counts == -12345).all())  # no decode / NMS output was written
    assert eng.candidate_counts(B) == cc0  # nor the decode scratch of the previous forward
    e2 = eng.embed(x, [4]).clone()
    e3 = eng.embed(x, [22]).clone()
    assert e2.shape == (B, eng.graph.layers[4][0].C) and torch.equal(e1, e3)
    assert bool((dets == -7.25).all()) and bool((counts == -12345).all())
    d1, c1 = eng.run(x)  # a plain run afterwards: the rows and counts it returned before
    assert torch.equal(c0, c1) and int(c0.sum()) > 0
    for b, n in enumerate(c0.tolist()):
        assert torch.equal(d0[b, :n], d1[b, :n]), b
    assert eng.candidate_counts(B) == cc0
    outs = m.embed(x)  # the facade on every task: B vectors of layer 22
    assert len(outs) == B and all(o.shape == (256,) and o.dtype == torch.float32 and o.is_cuda for o in outs)
    assert torch.equal(torch.stack(outs), e1)


# ------------------------------------------------------------------------------- 4. determinism
@pytest.mark.parametrize("dtype", ["x3", "f16"])
def test_embed_is_bit_identical_from_call_to_call(dtype):
    """Ten replays and an eager launch, one- and multi-chunk views (f16 detect plans run the branch schedule: the
    pooling stage reads behind the join of every opened stream)."""
    eng = model(dtype).model.engine
    x = inputs("320").to(DEV)
    layers = [0, 4, 12, 22]
    first = eng.embed(x, layers).clone()
    for _ in range(9):
        assert torch.equal(eng.embed(x, layers), first)
    eager = eng.embed(x, layers, use_graph=False).clone()
    assert torch.equal(eager, first)
    assert torch.equal(eng.embed(x, layers), first)


# ------------------------------------------------------------------------------- 5. facade
def test_predict_embed_and_model_embed():
    m = model("x3")
    eng = m.model.engine
    x = inputs("96x160")
    xd = x.to(DEV)
    before = [r.boxes.data.clone() for r in m.predict(x, conf=0.05)]
    c4, c22 = eng.graph.layers[4][0].C, eng.graph.layers[22][0].C
    outs = m.predict(x, embed=[22, 4])
    assert isinstance(outs, list) and len(outs) == x.shape[0]
    assert all(o.dim() == 1 and o.shape[0] == c4 + c22 and o.dtype == torch.float32 and o.is_cuda for o in outs)
    ref = eng.embed(xd, [4, 22]).clone()
    assert torch.equal(torch.stack(outs), ref)  # ascending: layer 4's slice first
    assert torch.equal(ref[:, :c4], eng.embed(xd, [4])) and torch.equal(ref[:, c4:], eng.embed(xd, [22]))
    assert outs[0].untyped_storage().data_ptr() == outs[1].untyped_storage().data_ptr()  # views of one buffer
    assert torch.equal(torch.stack(m.predict(x, embed=(4, 22, 4))), ref)  # a tuple; a duplicate counts once
    e22 = torch.stack(m.predict(x, embed=22))  # a bare int is one layer
    assert torch.equal(e22, ref[:, c4:])
    assert torch.equal(torch.stack(m.embed(x)), e22) and torch.equal(torch.stack(m.embed(x, embed=[4])), ref[:, :c4])
    assert torch.equal(torch.stack(m(x, embed=[22])), e22)
    # a later call leaves the vectors of an earlier one alone
    kept = m.embed(x)
    other = torch.stack(m.embed(x.flip(0).contiguous()))
    assert torch.equal(torch.stack(kept), e22) and not torch.equal(other, e22)
    assert torch.allclose(other, e22.flip(0), rtol=1e-4, atol=1e-6)
    # tensor preprocessing is predict's: LoadTensor's /255 rule
    x255 = (x * 255).round()
    assert torch.allclose(torch.stack(m.embed(x255)), eng.embed((x255 / 255).to(DEV), [22]), rtol=1e-4, atol=1e-6)
    # without the keyword (or with None) predict is what it was
    for again in (m.predict(x, conf=0.05), m.predict(x, conf=0.05, embed=None)):
        assert len(again) == len(before) and sum(len(b) for b in before) > 0
        for r, b in zip(again, before):
            assert torch.equal(r.boxes.data, b)


def test_predict_embed_of_image_sources_uses_the_letterboxed_batch():
    m = model("x3")
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (90, 120, 3), dtype=np.uint8), rng.integers(0, 256, (200, 150, 3), dtype=np.uint8)]
    outs = m.predict(imgs, embed=[22, 10], imgsz=160)
    im, eps, info = m._as_batch(imgs, 160)  # the batch predict builds: both images letterboxed to one shape
    assert info is not None and im.shape[0] == 2 and [tuple(s) for s in info[2]] == [(90, 120), (200, 150)]
    ref = m.model.engine.embed(im, [10, 22], in_eps=eps)
    assert len(outs) == 2 and torch.equal(torch.stack(outs), ref)
    assert not torch.equal(outs[0], outs[1])


def test_augment_and_retina_masks_are_ignored_with_one_debug_line(caplog):
    m = model("x3", "segment")
    x = inputs("96x160")
    ref = torch.stack(m.embed(x))
    with caplog.at_level(logging.DEBUG, logger="core.model"):
        got = torch.stack(m.predict(x, embed=[22], augment=True, retina_masks=True))
    assert torch.equal(got, ref)
    lines = [r for r in caplog.records if r.levelno == logging.DEBUG and "embed" in r.getMessage()]
    assert len(lines) == 1 and "augment" in lines[0].getMessage() and "retina_masks" in lines[0].getMessage()


# ------------------------------------------------------------------------------- 6. refusals
def test_refusals():
    from yolomi.lib import Runtime, YMError
    x = inputs("32").to(DEV)
    m = model("x3")
    eng = m.model.engine
    assert 1 not in eng.embed_layers() and 22 in eng.embed_layers()
    for call in (lambda: eng.embed(x, [1]), lambda: m.predict(x, embed=[4, 1])):
        with pytest.raises(ValueError, match=r"layer 1 .*f32"):
            call()
    f32 = model("f32").model.engine
    assert f32.embed_layers() == list(range(23))
    e = f32.embed(x, [1])
    assert e.shape == (1, f32.graph.layers[1][0].C) and bool(torch.isfinite(e).all())
    for bad in (-1, 23, 1.5, []):
        with pytest.raises(ValueError):
            m.predict(x, embed=bad)
        with pytest.raises(ValueError):
            eng.embed(x, bad)
    # the C entry: a row stride below the pooled channels, an empty table, a view outside its buffer
    v22 = eng.graph.layers[22][0]
    views = Runtime.embed_views([(v22.buf.id, 0, v22.C)])
    out = torch.zeros((1, v22.C), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    args = Runtime.make_args()
    eng.rt.embed(x.data_ptr(), 1, 32, 32, args, views, out.data_ptr(), v22.C, stream)
    assert torch.equal(out, eng.embed(x, [22]))
    with pytest.raises(YMError, match="EINVAL"):
        eng.rt.embed(x.data_ptr(), 1, 32, 32, args, views, out.data_ptr(), v22.C - 8, stream)
    with pytest.raises(YMError, match="EINVAL"):
        eng.rt.embed(x.data_ptr(), 1, 32, 32, args, Runtime.embed_views([]), out.data_ptr(), v22.C, stream)
    with pytest.raises(YMError, match="EINVAL"):
        eng.rt.embed(x.data_ptr(), 1, 32, 32, args, Runtime.embed_views([(v22.buf.id, 8, v22.C)]), out.data_ptr(),
                     v22.C, stream)
    with pytest.raises(YMError, match="EINVAL"):
        eng.rt.embed(x.data_ptr(), 1, 32, 32, args, views, 0, v22.C, stream)


def test_quantized_plans_refuse():
    import json
    from core.model import YOLO11Model
    from oracle import quant as Q
    gold = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "det_n_i8_qnnpack.json")
    g = json.load(open(gold))
    m = _cache[("m", "i8")] = YOLO11Model(task="detect", size=g["scale"], device="cuda:0", dtype="i8",
                                          qparams=Q.qparams_from_json(g["qparams"]), verbose=False)
    x = inputs("32").to(DEV)
    with pytest.raises(ValueError, match="quantized"):
        m.predict(x, embed=[22])
    with pytest.raises(ValueError, match="quantized"):
        m.model.engine.embed(x)
