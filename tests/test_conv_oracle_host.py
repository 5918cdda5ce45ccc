"""tests/conv_oracle.py on the CPU: every plan's emulation passes its own bound; corruptions a kernel could plausibly
commit fail it (so the 8 x e margin discriminates); and the reference function computes what oracle/yolo11.py's modules
compute in float64 for every kind of op."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import yolo11 as Y
from tests import conv_oracle as CO
from yolomi.arch import GraphBuilder
from yolomi.synth import normal, synth_param, synth_weights

PLANS = ("f16", "x3", "f32")
# (name, k, s, cin, cout, (B, H, W)): a 3x3 64 -> 64 on a 5x7 map, a 1x1 256 -> 64 on a 3x5 map, a 3x3 at K = 2304
CONVS = [("c3", 3, 1, 64, 64, (2, 5, 7)), ("c1", 1, 1, 256, 64, (3, 3, 5)), ("k2304", 3, 1, 256, 32, (1, 4, 6))]


def toy(name, k, s, cin, cout, shape, pair=None, seed=0):
    """(a, sd, x): a one-conv op record with synth_weights-like parameters (yolomi/synth.py synth_param) and an O(1)
    input of the given (B, H, W).  pair: (k2, cout2) appends a fused successor."""
    sd = {}

    def params(key, c1, c2, kk):
        sd[key + ".conv.weight"] = synth_param(key + ".conv.weight", (c2, c1, kk, kk), "conv_w", seed, {})
        for suf, kind in (("weight", "bn_w"), ("bias", "bn_b"), ("running_mean", "bn_mean"), ("running_var", "bn_var")):
            sd[f"{key}.bn.{suf}"] = synth_param(f"{key}.bn.{suf}", (c2,), kind, seed, {})

    params(name, cin, cout, k)
    a = dict(k=k, s=s, c1=cin, c2=cout, act=True, src0=SimpleNamespace(C=cin), up0=False, src1=None, res=None,
             shuffle2x2=False, bn=True, wkey=name)
    if pair:
        k2, n2 = pair
        params(name + ".next", cout, n2, k2)
        a["pair"] = dict(k=k2, c1=cout, c2=n2, act=True, bn=True, wkey=name + ".next")
    B, H, W = shape
    x = torch.from_numpy(normal(77 + seed, B * H * W * cin).astype(np.float32).reshape(B, H, W, cin))
    return a, sd, F.silu(x)  # (activations of the net are SiLU outputs)


def stored(plan, x):
    return CO.round_act(plan, x)


def ratio(got, ref, E):
    return CO.worst(got, ref, E)[0]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("conv", CONVS, ids=[c[0] for c in CONVS])
def test_emulation_passes_its_own_bound(plan, conv):
    a, sd, x = toy(*conv)
    x = stored(plan, x)
    ref, E, _ = CO.reference(plan, a, sd, x)
    r = ratio(CO.emulate(plan, a, sd, x), ref, E)
    print(f"{plan} {conv[0]}: emulation err / E = {r:.3f}")
    assert r <= 1.0


@pytest.mark.parametrize("plan", PLANS)
def test_pair_emulation_passes_its_own_bound(plan):
    a, sd, x = toy("p", 3, 1, 64, 64, (2, 5, 7), pair=(1, 64))
    x = stored(plan, x)
    ref, E, _ = CO.reference(plan, a, sd, x)
    assert ratio(CO.emulate(plan, a, sd, x), ref, E) <= 1.0


def rounded_weights(plan, a, sd):
    return {k: (CO.round_weight(plan, v) if k in ("w", "w2") else v.float()) for k, v in CO.op_weights(a, sd).items()}


@pytest.mark.parametrize("conv", CONVS, ids=[c[0] for c in CONVS])
def test_x3_dropped_cross_term_fails(conv):
    """hi * w_hi + lo * w_hi with the hi * w_lo term dropped: the weights are their fp16 hi part alone."""
    a, sd, x = toy(*conv)
    x = stored("x3", x)
    ref, E, _ = CO.reference("x3", a, sd, x)
    W = rounded_weights("x3", a, sd)
    s = 2.0 ** CO.x3_weight_exp(W["w"].numpy())
    W["w"] = (W["w"] * s).half().float() / s
    assert ratio(CO.emulate("x3", a, sd, x, W=W), ref, E) > 1.0


@pytest.mark.parametrize("plan", ["f32", "x3"])
@pytest.mark.parametrize("conv", CONVS, ids=[c[0] for c in CONVS])
def test_fp16_operands_fail_the_fp32_storage_bounds(plan, conv):
    a, sd, x = toy(*conv)
    x = stored(plan, x)
    ref, E, _ = CO.reference(plan, a, sd, x)
    assert ratio(CO.emulate("f16", a, sd, x), ref, E) > 1.0


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("conv", CONVS, ids=[c[0] for c in CONVS])
def test_skipped_k_chunk_fails(plan, conv):
    """One 8-channel K chunk of one tap never multiplied."""
    a, sd, x = toy(*conv)
    x = stored(plan, x)
    ref, E, _ = CO.reference(plan, a, sd, x)
    W = rounded_weights(plan, a, sd)
    k = a["k"]
    W["w"][:, 16:24, k - 1, k // 2] = 0
    assert ratio(CO.emulate(plan, a, sd, x, W=W), ref, E) > 1.0


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("conv", [CONVS[0], CONVS[2]], ids=["c3", "k2304"])
def test_tap_shifted_on_the_last_column_fails(plan, conv):
    """Tap (ky, kx) = (1, 0) of the last output column reads one pixel to the right of where it should."""
    a, sd, x = toy(*conv)
    x = stored(plan, x)
    ref, E, _ = CO.reference(plan, a, sd, x)
    got = CO.emulate(plan, a, sd, x)
    W = rounded_weights(plan, a, sd)
    tap = W["w"][:, :, 1, 0]  # (N, cin): reads pixel (y, x - 1); wrongly (y, x)
    right, wrong = x[:, :, -2, :].float(), x[:, :, -1, :].float()
    # redo the last column's pre-activation with the wrong pixel, then the activation
    full = CO.forward(dict(a, act=False), W, x, dt=torch.float32)[0]
    col = full[:, :, -1, :] + (wrong - right) @ tap.T
    bad = got.clone()
    bad[:, :, -1, :] = CO.silu32(col)
    assert ratio(bad, ref, E) > 1.0
    assert ratio(bad[:, :, :-1], ref[:, :, :-1], E[:, :, :-1]) <= 1.0  # (the other columns are the emulation's)


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("conv", CONVS, ids=[c[0] for c in CONVS])
def test_unwritten_last_partial_tile_fails(plan, conv):
    """The last M % 64 pixels left at zero (a mis-indexed last partial M tile)."""
    a, sd, x = toy(*conv)
    x = stored(plan, x)
    ref, E, _ = CO.reference(plan, a, sd, x)
    got = CO.emulate(plan, a, sd, x).clone()
    N = got.shape[-1]
    flat = got.reshape(-1, N)
    M = flat.shape[0]
    assert M % 64
    flat[M - M % 64:] = 0
    r, idx, _, _ = CO.worst(flat.reshape(got.shape), ref, E)
    assert r > 1.0
    b, y, xx, _ = idx
    assert (b * got.shape[1] + y) * got.shape[2] + xx >= M - M % 64  # the worst element is named inside that tile


@pytest.mark.parametrize("plan", PLANS)
def test_pair_without_the_intermediate_silu_fails(plan):
    a, sd, x = toy("p", 3, 1, 64, 64, (2, 5, 7), pair=(1, 64))
    x = stored(plan, x)
    ref, E, _ = CO.reference(plan, a, sd, x)
    assert ratio(CO.emulate(plan, a, sd, x, mid_act=lambda t: t), ref, E) > 1.0


def test_tol_never_exceeds_the_worst_case():
    for plan in PLANS:
        assert CO.TOL[plan] == CO.MARGIN * CO.E_MEASURED[plan]
        # the bound uses min(tol, cap) per op, so the cap holds by construction; the largest K of yolo11n/s is 4608
        a, sd, x = toy("c1", 1, 1, 256, 64, (1, 3, 5))
        ref, E, A = CO.reference(plan, a, sd, stored(plan, x))
        assert bool((E <= (CO.tol_cap(plan, 256) * A + CO.C_OUT[plan] * ref.abs()) * (1 + 1e-12)).all())


# ------------------------------------------------------------------------------ the reference vs oracle/yolo11.py
def _op(g, name):
    return next(op for op in g.ops if op.name == name).args


def _rand(B, H, W, C, seed):
    return torch.from_numpy(normal(seed, B * H * W * C).reshape(B, H, W, C)).float()


def _close(out, want_nchw):
    """Agreement up to the fp32 rounding of the folded BatchNorm (the planner folds with numpy, the oracle with torch:
    a weight or bias may differ in its last bit), which is relative to A; a structural mistake is O(1)."""
    ref, _, A = out
    want = want_nchw.permute(0, 2, 3, 1)
    assert ref.shape == want.shape
    assert bool(((ref - want).abs() <= 2.0 ** -20 * A + 1e-9).all()), float((ref - want).abs().max())


@pytest.fixture(scope="module")
def nets():
    sd = synth_weights("n", "detect", 0)
    sds = synth_weights("n", "segment", 0)
    return sd, Y.build("n", "detect", sd, fuse=True).double(), sds, Y.build("n", "segment", sds, fuse=True).double()


def test_reference_matches_the_oracle_modules(nets):
    sd, net, sds, seg = nets
    m = net.model
    n = lambda t: t.permute(0, 3, 1, 2).double()
    with torch.no_grad():
        # plain: model.1, a 3x3 stride-2 conv on an odd map
        g = GraphBuilder("n", "detect")
        a = _op(g, "model.1")
        x = _rand(2, 5, 7, a["c1"], 1)
        _close(CO.reference("f32", a, sd, x), m[1](n(x)))
        # two sources, the first up-sampled: model.13.cv1 on cat(up(L10), L6)
        a = _op(g, "model.13.cv1")
        x0, x1 = _rand(1, 3, 5, a["src0"].C, 2), _rand(1, 6, 10, a["src1"].C, 3)
        _close(CO.reference("f32", a, sd, x0, x1), m[13].cv1(torch.cat([m[11](n(x0)), n(x1)], 1)))
        # residual: the second conv of a Bottleneck
        a = _op(g, "model.2.m.0.cv2")
        h, r = _rand(1, 5, 7, a["c1"], 4), _rand(1, 5, 7, a["c2"], 5)
        _close(CO.reference("f32", a, sd, h, res=r), n(r) + m[2].m[0].cv2(n(h)))
        # merged wkeys: C3k's cv1 || cv2 as one GEMM
        gm = GraphBuilder("n", "detect", fuse="merge")
        a = _op(gm, "model.6.m.0.cv1+cv2")
        x = _rand(1, 3, 5, a["c1"], 6)
        c3k = m[6].m[0]
        _close(CO.reference("f32", a, sd, x), torch.cat([c3k.cv1(n(x)), c3k.cv2(n(x))], 1))
        # pairs: a Bottleneck (3x3 -> 3x3 + shortcut) and a head chain (3x3 -> 1x1, no activation)
        gf = GraphBuilder("n", "detect", fuse=True)
        pairs = {op.name: op.args for op in gf.ops if op.args.get("pair")}
        a = pairs["model.2.m.0.cv1+cv2"]
        x = _rand(1, 5, 7, a["c1"], 7)
        _close(CO.reference("f16", a, sd, x, res=x), m[2].m[0](n(x)))
        a = pairs["model.23.cv2.0.1+2"]
        x = _rand(1, 5, 7, a["c1"], 8)
        _close(CO.reference("f16", a, sd, x), m[23].cv2[0][2](m[23].cv2[0][1](n(x))))
        # depthwise fused in front of its 1x1 (x3 plans)
        gx = GraphBuilder("n", "detect", fuse="x3")
        a = next(op.args for op in gx.ops if op.args.get("dw"))
        assert a["dw"]["wkey"] == "model.23.cv3.0.0.0"
        x = _rand(1, 5, 7, a["c1"], 9)
        _close(CO.reference("x3", a, sd, x), m[23].cv3[0][0](n(x)))
        # ConvTranspose2d as a pixel-shuffled GEMM (segment plans)
        gs = GraphBuilder("n", "segment")
        a = _op(gs, "model.23.proto.upsample")
        x = _rand(1, 3, 5, a["c1"], 10)
        _close(CO.reference("f32", a, sds, x), seg.model[23].proto.upsample(n(x)))
