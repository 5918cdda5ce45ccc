"""Host tests of feature embeddings: the layer map of yolomi.arch.GraphBuilder (where each of layers 0..22 lives in a
plan, without changing the plan), the index validation of predict(embed=...), and known answers of the torch
restatement tests/embed_oracle.py."""
import hashlib

import pytest
import torch

from oracle.yolo11 import YOLO11
from tests import embed_oracle as EO
from tests.test_pose_host import PARENT_BLOBS
from yolomi.arch import DEFAULT_EMBED, EMBED_LAYERS, GraphBuilder, normalize_embed
from yolomi.plan import fuse_default, pack_graph
from yolomi.synth import synth_weights

TASKS = ("detect", "segment", "pose")
_cache = {}


def oracle_channels(scale):
    """Channels of every layer output 0..22 of the oracle network (the backbone and neck are the same for all tasks)."""
    if ("ch", scale) not in _cache:
        net = YOLO11(scale, "detect").eval()
        with torch.no_grad():
            _, saved = net(torch.zeros(1, 3, 64, 64), keep=tuple(range(EMBED_LAYERS)))
        _cache[("ch", scale)] = {i: (t.shape[1], 64 // t.shape[2]) for i, t in saved.items()}
    return _cache[("ch", scale)]


def net_n():
    if "net" not in _cache:
        from oracle.yolo11 import build
        _cache["net"] = build("n", "detect", synth_weights("n", "detect", 0))
        _cache["x"] = torch.rand(2, 3, 64, 96, generator=torch.Generator().manual_seed(3))
    return _cache["net"], _cache["x"]


# ------------------------------------------------------------------------------------------------ layer map
@pytest.mark.parametrize("task", TASKS)
@pytest.mark.parametrize("scale", ["n", "s"])
@pytest.mark.parametrize("fuse", [False, "x3", True])
def test_layer_map_matches_oracle_shapes(scale, task, fuse):
    g = GraphBuilder(scale, task, fuse=fuse)
    ref = oracle_channels(scale)
    assert sorted(g.layers) == list(range(EMBED_LAYERS))
    for i, views in g.layers.items():
        assert sum(v.C for v in views) == ref[i][0], i
        for v in views:
            assert 0 <= v.coff and v.coff + v.C <= v.buf.C and v.C % 8 == 0 and v.coff % 8 == 0
            assert not v.buf.f32 and v.buf.f >= 2
        if i not in EO.UPSAMPLE and i not in EO.CONCAT:
            assert len(views) == 1 and views[0].buf.f == ref[i][1] and views[0].buf.name == f"L{i}"
    assert g.layers[22][0].C == {"n": 256, "s": 512}[scale]


@pytest.mark.parametrize("task", TASKS)
def test_upsample_aliases_and_concat_parts(task):
    g = GraphBuilder("n", task, fuse="x3")
    key = lambda vs: [(v.buf.id, v.coff, v.C) for v in vs]  # noqa: E731
    for up, src in EO.UPSAMPLE.items():
        assert key(g.layers[up]) == key(g.layers[src])
    for cat, parts in EO.CONCAT.items():
        assert key(g.layers[cat]) == [k for p in parts for k in key(g.layers[p])]  # the inputs' views, in order
        assert len({v.buf.f for v in g.layers[cat]}) <= 2  # (an up-sampled part keeps its source's stride)


@pytest.mark.parametrize("scale", ["n", "s"])
def test_fused_layer_is_reported_as_not_stored(scale):
    f32 = GraphBuilder(scale, "detect", fuse=fuse_default("f32"))
    assert f32.embed_layers() == list(range(EMBED_LAYERS)) and f32.layer_stored(1)
    assert [v.buf.name for v in f32.layer_views(1)] == ["L1"]
    for dtype in ("x3", "f16"):
        g = GraphBuilder(scale, "detect", fuse=fuse_default(dtype))
        assert not g.layer_stored(1) and 1 not in g.embed_layers(), dtype
        # only a plain down-sampling Conv can vanish into the 1x1 that follows it (fuse_pairs); the C3k2 / SPPF /
        # C2PSA outputs, and so every Upsample and Concat layer, are stored by every plan
        missing = set(range(EMBED_LAYERS)) - set(g.embed_layers())
        assert 1 in missing and missing <= {1, 3, 5, 7, 17, 20}, (dtype, missing)
        for i in missing:
            with pytest.raises(ValueError, match=rf"layer {i} .*f32"):
                g.layer_views(i)
        assert g.layer_views(22)[0].buf.name == "L22"


@pytest.mark.parametrize("scale,task,dtype", [("n", "detect", "x3"), ("n", "detect", "f16"), ("s", "segment", "x3")])
def test_querying_the_map_changes_no_op_and_no_blob_byte(scale, task, dtype, monkeypatch):
    for v in ("YM_FUSE", "YM_FUSE_DW", "YM_DW_FUSE_STRIDES"):
        monkeypatch.delenv(v, raising=False)
    sd = synth_weights(scale, task, 0)
    plain = GraphBuilder(scale, task, fuse=fuse_default(dtype))
    asked = GraphBuilder(scale, task, fuse=fuse_default(dtype))
    asked.embed_layers()
    for i in asked.embed_layers():
        asked.layer_views(i)
    assert not asked.layer_stored(1)
    assert [(o.kind, o.name, repr(o.args)) for o in plain.ops] == [(o.kind, o.name, repr(o.args)) for o in asked.ops]
    assert [(b.id, b.C, b.f, b.f32, b.name) for b in plain.buffers] == [(b.id, b.C, b.f, b.f32, b.name)
                                                                         for b in asked.buffers]
    b0, b1 = pack_graph(plain, sd, dtype), pack_graph(asked, sd, dtype)
    assert b0 == b1
    assert hashlib.sha256(b1).hexdigest() == PARENT_BLOBS[(scale, task, dtype)]  # and it is the parent's blob


# ------------------------------------------------------------------------------------------------ index validation
@pytest.mark.parametrize("bad", [-1, 23, 1.5, [], [4, -1], [22, 23], [1.5], "22", None, True, [[4]]])
def test_bad_indices_raise(bad):
    with pytest.raises(ValueError):
        normalize_embed(bad)


def test_indices_normalise_to_an_ascending_set():
    assert normalize_embed([22, 4]) == (4, 22)
    assert normalize_embed((22, 4, 22, 4)) == (4, 22)
    assert normalize_embed(22) == (22,) and normalize_embed([0]) == (0,)
    assert normalize_embed(torch.tensor(7)) == (7,)  # (an integer scalar: operator.index)
    assert DEFAULT_EMBED == (22,) == EO.DEFAULT


# ------------------------------------------------------------------------------------------------ restatement
def test_restatement_known_answers():
    net, x = net_n()
    one = lambda ls: torch.stack(EO.embed(net, x, ls))  # noqa: E731
    ch = oracle_channels("n")
    e10, e11, e6, e12 = one([10]), one([11]), one([6]), one([12])
    assert e10.shape == (2, ch[10][0]) and e12.shape == (2, ch[10][0] + ch[6][0])
    # a nearest 2x copy has the same mean: four equal terms per source pixel, so only fp32 rounding differs
    assert torch.allclose(e11, e10, rtol=1e-6, atol=1e-7 * float(e10.abs().max()))
    assert torch.equal(e12, torch.cat([e11, e6], 1))  # Concat pools as the cat of its parts
    e = one([22, 4])
    assert torch.equal(e, torch.cat([one([4]), one([22])], 1))  # ascending, whatever the caller wrote
    assert e.shape[1] == ch[4][0] + ch[22][0]
    assert torch.equal(one([4, 22, 4, 22]), e)  # a duplicate counts once
    outs = EO.embed(net, x)  # the default: layer 22, a tuple of B 1-D tensors
    assert len(outs) == 2 and outs[0].shape == (ch[22][0],) and torch.equal(torch.stack(outs), one([22]))


def test_restatement_runs_in_float64_and_rebuilds_unmaterialised_layers():
    net, x = net_n()
    import copy
    net64 = copy.deepcopy(net).double()
    outs = EO.layer_outputs(net, x, [10, 11, 12, 13])
    assert outs[11].shape[2:] == (2 * outs[10].shape[2], 2 * outs[10].shape[3])
    assert torch.equal(outs[11][:, :, ::2, ::2], outs[10]) and torch.equal(outs[11][:, :, 1::2, 1::2], outs[10])
    _, saved = net(x, keep=(11, 12))  # the oracle network materialises both: the rebuilt ones are the same tensors
    assert torch.equal(outs[11], saved[11]) and torch.equal(outs[12], saved[12])
    e32 = torch.stack(EO.embed(net, x, [4, 12, 22]))
    e64 = torch.stack(EO.embed(net64, x.double(), [4, 12, 22]))
    assert e64.dtype == torch.float64 and e32.dtype == torch.float32
    assert torch.allclose(e32.double(), e64, rtol=1e-3, atol=1e-5)
