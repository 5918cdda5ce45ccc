"""tests/misc_oracle.py on the CPU: its references compute what oracle/yolo11.py's Attention, SPPF and DWConv compute in
float64; every plan's emulation passes its own bound; every mutation (a wrong reference of the kind a kernel could
produce) breaks the bound somewhere; the sharpened weight set has the peaked softmax it is there for; and the measured
constants are the ones profiles/misc_op_bounds.txt records."""
import os

import pytest
import torch

from tests import misc_oracle as MO
from yolomi.arch import GraphBuilder
from yolomi.synth import synth_weights

PLANS = ("f16", "x3", "f32")
_cache = {}


def weights(sharp=False):
    if "sd" not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _cache["sd"] = synth_weights("n", "detect", 0)
        _cache["sharp"] = MO.sharpen(_cache["sd"], GraphBuilder("n", "detect").ops, MO.SHARP)
    return _cache["sharp" if sharp else "sd"]


def taps(shape, sharp=False, dt=torch.float32):
    """The oracle yolo11n's tensors around its attention / SPPF / depthwise modules at a shape (computed once)."""
    k = (shape, sharp, dt)
    if k not in _cache:
        _cache[k] = MO.oracle_taps("n", weights(sharp), MO.batch(shape), dt)
    return _cache[k]


def stored(plan, t):
    return MO.CO.round_act(plan, t)


# ---------------------------------------------------------------------------------------------- the references
@pytest.mark.parametrize("shape", ["96x160", "160x224", "32x416"])
def test_references_are_the_oracle_modules_in_float64(shape):
    """3x5 (B = 3), 5x7 and 1x13 maps: Attention's sum in front of proj, SPPF's three pools and every DWConv.  The
    depthwise weights are the planner's fp32 BN fold (what the GPU gets) against torch's fp32 fold in the module: the
    two round differently, a few 2^-24 of a term, so these two agree to 1e-6 of the tensor's maximum, not to 1e-12."""
    t = taps(shape, dt=torch.float64)
    sd = weights()
    assert t["attn"] and t["dw"]
    for a, qkv, want in t["attn"]:
        ref, _, _ = MO.attn_reference("f32", a, sd, qkv, want_bound=False)
        assert float((ref - want).abs().max()) <= 1e-6 * float(want.abs().max())
    for src, cat in t["sppf"]:
        C = src.shape[-1]
        assert torch.equal(cat[..., :C], src) and torch.equal(MO.sppf_reference(src), cat[..., C:])
    for a, src, want in t["dw"]:
        ref, _, _ = MO.dw_reference("f32", a, sd, src)
        assert float((ref - want).abs().max()) <= 1e-6 * float(want.abs().max()), a["wkey"]


# ---------------------------------------------------------------------------------------------- the bound holds
@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("case", [("96x160", False), ("96x160", True), ("352x416", True), ("736x736", False),
                                  ("736x736", True)], ids=lambda c: c[0] + ("-sharp" if c[1] else ""))
def test_attention_emulation_passes_its_own_bound(plan, case):
    shape, sharp = case
    for a, qkv, _ in taps(shape, sharp)["attn"]:
        qkv = stored(plan, qkv)
        ref, E, _ = MO.attn_reference(plan, a, weights(sharp), qkv)
        r, idx, err, e = MO.worst(MO.emulate_attn(plan, a, weights(sharp), qkv), ref, E)
        print(f"{plan} {shape}{' sharp' if sharp else ''}: emulation err / E = {r:.3f}")
        assert r <= 1.0, (idx, err, e)


@pytest.mark.parametrize("plan", PLANS)
def test_depthwise_emulation_passes_its_own_bound(plan):
    for shape in ("96x160", "160x224"):
        for a, src, _ in taps(shape)["dw"]:
            src = stored(plan, src)
            ref, E, _ = MO.dw_reference(plan, a, weights(), src)
            r, idx, err, e = MO.worst(MO.emulate_dw(plan, a, weights(), src), ref, E)
            assert r <= 1.0, (a["wkey"], idx, err, e)


def test_tolerances_stay_under_their_caps():
    for plan in PLANS:
        for N in (13, 15, 35, 143, 529, 1089, 2115):
            ts, to = MO.tols(plan, 32, N)
            assert 0 < ts <= MO.cap_s(plan, 32) and 0 < to <= MO.cap_o(plan, N)


def test_the_measured_constants_are_the_recorded_ones():
    """profiles/misc_op_bounds.txt holds the e_s / e_o lines tools/misc_op_bounds.py printed."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "profiles", "misc_op_bounds.txt")).read()
    for plan in PLANS:
        assert f"{plan}: e_s = {MO.E_S[plan]:.3e}" in text and f"{plan}: e_o = {MO.E_O[plan]:.3e}" in text, plan


# ---------------------------------------------------------------------------------------------- the bound bites
def mutation_ratio(plan, a, sd, qkv, name):
    """The largest |mutated reference - reference| / E: above 1, a kernel that computed the mutation fails."""
    ref, E, _ = MO.attn_reference(plan, a, sd, qkv)
    bad, _, _ = MO.attn_reference(plan, a, sd, qkv, mutation=name)
    return MO.worst(bad, ref, E)[0]


@pytest.mark.parametrize("plan", PLANS)
@pytest.mark.parametrize("name", list(MO.MUTATIONS))
def test_every_mutation_breaks_the_bound(plan, name):
    """On the oracle's own qkv at N = 15 (B = 3), 143 and 529 — and, for the two single-key mutations in f16, on the
    sharpened weights at N = 15 and 143, where one key carries enough weight to show at fp16 precision."""
    single16 = plan == "f16" and name in MO.SINGLE_KEY
    ran = 0
    for shape in ("96x160", "352x416", "736x736"):
        H, W, _ = MO.SHAPES[shape]
        if not MO.applies(name, H // 32, W // 32) or (single16 and shape == "736x736"):
            continue
        for a, qkv, _ in taps(shape, single16)["attn"]:
            r = mutation_ratio(plan, a, weights(single16), stored(plan, qkv), name)
            print(f"{plan} {shape} {name}: |mutation - ref| / E = {r:.1f}")
            assert r > 1.0
            ran += 1
    assert ran


def test_every_mutation_applies_somewhere_and_not_everywhere():
    maps = [(H // 32, W // 32) for H, W, _ in MO.SHAPES.values()]
    for name in MO.MUTATIONS:
        assert any(MO.applies(name, h, w) for h, w in maps), name
    assert not MO.applies("last_partial_tile_dropped", 3, 5) and not MO.applies("last_partial_tile_dropped", 8, 16)
    assert not MO.applies("last_block_dropped", 16, 16) and MO.applies("last_block_dropped", 23, 23)
    assert not MO.applies("pe_no_left_border_test", 1, 13)


def test_a_wrong_pool_is_not_equal():
    src, _ = taps("160x224")["sppf"][0]
    ref = MO.sppf_reference(src)
    C = src.shape[-1]
    x = src.double().permute(0, 3, 1, 2)
    cascade_of_3 = torch.nn.functional.max_pool2d(x, 3, 1, 1)  # a radius-1 window where radius 2 is due
    assert not torch.equal(cascade_of_3.permute(0, 2, 3, 1), ref[..., :C])
    assert not torch.equal(ref[..., :C], ref[..., C:2 * C])  # 5x7 map: the 9-wide window still differs from the 5-wide


# ---------------------------------------------------------------------------------------------- the sharp variant
@pytest.mark.parametrize("shape", MO.SHARP_SHAPES)
def test_sharpened_weights_give_a_peaked_softmax(shape):
    """Query channels x 8: the median row maximum of P exceeds 0.1 at N = 15, 143, 529 and 1089 (it is 0.09 ... 0.003
    on the plain weights), so one key matters and the max subtraction and underflow paths work."""
    for sharp in (False, True):
        for a, qkv, _ in taps(shape, sharp)["attn"]:
            _, _, info = MO.attn_reference("f32", a, weights(sharp), qkv)
            med = float(info["pmax"].median())
            print(f"{shape} {'sharp' if sharp else 'plain'}: median row max of P {med:.3f}")
            assert med > 0.1 if sharp else med < 0.1
