"""The attention, SPPF and depthwise kernels (csrc/ym_attn.hip, ym_sppf.hip, ym_dwconv.hip) op by op against float64
computed from the op's own stored input (tests/misc_oracle.py: the references, the per-element bound E, the mutations
and where every number comes from) — and known to have run: after each forward the runtime says which instantiation
each of these ops launched (ym_get_op_variant), the test restates the launch rule and demands that code, and over the
whole set every code of ym_op_variant_count ran or stands on a reasoned never-run list.

Eager forwards, one lane, no autotune; inputs make_input("uniform", ...) cropped to H x W (misc_oracle.SHAPES).
Shapes and what each reaches (N = (H / 32) (W / 32) tokens; yolo11n, 2 heads, unless stated):

    96x160 B=3     N = 15    NKT 8; N < 16; 49 of 64 queries masked; 3x5 map: every pixel on a border, every pool
                             window wider than the map
    160x224        N = 35    NKT 8; N % 16 = 3; 5x7 map.  Also yolo11s (4 heads)
    256x512        N = 128   NKT 8 exactly full
    352x416        N = 143   NKT 16; N % 16 = 15
    512x512        N = 256   NKT 16 full
    480x672        N = 315   NKT 26
    416x1024       N = 416   NKT 26 full
    640x800        N = 500   NKT 32; N % 16 = 4
    512x1024       N = 512   NKT 32 full; the last N in front of flash
    736x736        N = 529   flash: 3 blocks, the last holds 17 keys
    1056x1056      N = 1089  flash: 5 blocks, the last query block holds one query; SPPF direct path in f32 / x3; the
                             p >= 1024 load loop in f16
    1440x1504      N = 2115  (f16 only) SPPF direct path in f16
    32x416         N = 13    1x13 map: SPPF and pe with H = 1
    yolo11s 96x160 B=128, 352x416 B=15 (f32): the scalar kernel's QB 32 (rows 15..31 of the block masked) and QB 16

The sharp weight set (misc_oracle.sharpen: query channels x 8) runs N = 15, 143, 529, 1089 on all three plans: a peaked
softmax, so one wrong key shows and the max subtraction / underflow paths work.

Power.  On the read-back tensors of each case every mutation that applies must break E at some element, for f32 and x3
everywhere; for f16 the tile, block, head, scale and pe mutations everywhere and the two single-key ones on the sharp
set at N <= 143 (at N = 143 plain, swapping two V rows moves the output by about 1.5e-3 A_o against an f16 bound near
1e-3 A_o: too close to demand; the ratio is printed)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import misc_oracle as MO
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# plan -> (dtype, environment while the model is built); x3nodw keeps the Detect head's depthwise ops as ops of their own
PLANS = {"f16": ("f16", {}), "x3": ("x3", {}), "f32": ("f32", {}), "x3nodw": ("x3", {"YM_FUSE_DW": "0"})}
ATTN_PLANS = ("f16", "x3", "f32")
DW_PLANS = ("f16", "f32", "x3nodw")

# (scale, shape, B, weights, plans, {plan: attention instantiation}) — the (plan, N, B * nh) -> code table, restated from
# csrc/ym_op_select.h ym_select_attn: f16 / x3 with kd 32, hd 64 take the MFMA kernels by ceil(N / 16) <= 8, 16, 26, 32,
# above that flash; f32 takes attn_psa<QB>: 32 when B nh ceil(N / 32) >= 512, else 16 when B nh ceil(N / 16) >= 512, else
# 8 (the LDS budget of 150 KiB holds QB 32 up to N = 1136 and QB 8 up to N = 4256)
_MF = lambda n: {"f16": f"mfma_nkt{n}", "x3": f"x3_nkt{n}", "f32": "scalar_qb8"}
_FLASH = {"f16": "flash_f16", "x3": "flash_x3", "f32": "scalar_qb8"}
CASES = [
    ("n", "96x160", 3, "plain", ATTN_PLANS, _MF(8)),
    ("n", "160x224", 1, "plain", ATTN_PLANS, _MF(8)),
    ("s", "160x224", 1, "plain", ATTN_PLANS, _MF(8)),
    ("n", "256x512", 1, "plain", ATTN_PLANS, _MF(8)),
    ("n", "352x416", 1, "plain", ATTN_PLANS, _MF(16)),
    ("n", "512x512", 1, "plain", ATTN_PLANS, _MF(16)),
    ("n", "480x672", 1, "plain", ATTN_PLANS, _MF(26)),
    ("n", "416x1024", 1, "plain", ATTN_PLANS, _MF(26)),
    ("n", "640x800", 1, "plain", ATTN_PLANS, _MF(32)),
    ("n", "512x1024", 1, "plain", ATTN_PLANS, _MF(32)),
    ("n", "736x736", 1, "plain", ATTN_PLANS, _FLASH),
    ("n", "1056x1056", 1, "plain", ATTN_PLANS, _FLASH),
    ("n", "1440x1504", 1, "plain", ("f16",), _FLASH),
    ("n", "32x416", 1, "plain", ATTN_PLANS, _MF(8)),
    ("s", "96x160", 128, "plain", ("f32",), {"f32": "scalar_qb32"}),  # 512 (image, head) pairs x 1 block of 32
    ("s", "352x416", 15, "plain", ("f32",), {"f32": "scalar_qb16"}),  # 60 x ceil(143 / 32) = 300 < 512 <= 60 x 9
    ("n", "96x160", 3, "sharp", ATTN_PLANS, _MF(8)),
    ("n", "352x416", 1, "sharp", ATTN_PLANS, _MF(16)),
    ("n", "736x736", 1, "sharp", ATTN_PLANS, _FLASH),
    ("n", "1056x1056", 1, "sharp", ATTN_PLANS, _FLASH),
]
# Instantiations no case above (or the flash-off children below) launches, each with the launch condition that excludes
# it.  test_every_variant_ran holds the never-run set to exactly this.
NEVER_RUN = {
    "attn": {"scalar_qb4": "launch_attn_t takes QB 4 only when QB 8 overflows the 150 KiB LDS budget: "
                           "(8 N + 8 * 32 + 64 * 64) * 4 > 153600, N > 4256 tokens, a 2112 x 2112 input"},
    "sppf": {},
    "dwconv": {
        "row4": "dwconv3x3_row<f16, 4> needs B H W C / 8 >= 4 * 128 * 256 pixel chunks (a 640 x 640 batch of 8): it runs, and "
                "is asserted to, in tests/test_gpu_kernels.py::test_dwconv_variants_match_float64 mode 1",
        "strip2": "dwconv3x3_strip needs >= 256 workgroups of 2 x 2 strips (a 640 x 640 batch of 8 of yolo11s): it runs, and is "
                  "asserted to, in tests/test_gpu_kernels.py::test_dwconv_variants_match_float64 mode 2",
        "strip4": "dwconv3x3_strip<T, 4, 4> needs B ceil(H / 4) (W / 4) C / 8 >= 65536 threads: at 640 x 640 a batch of 11 of "
                  "yolo11s, above every batch the suite runs (YM_DW_RT=4 forces it, read once per process)"},
}
TILE_MUTS = ("last_partial_tile_dropped", "last_block_dropped", "heads_swapped", "scale_sqrt2", "pe_no_left_border_test",
             "pe_of_the_wrong_head")

_cache = {}
_ran = {"attn": set(), "sppf": set(), "dwconv": set()}


def weights(scale, kind="plain"):
    if ("sd", scale) not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _cache[("sd", scale)] = synth_weights(scale, "detect", 0)
    if kind == "plain":
        return _cache[("sd", scale)]
    if ("sharp", scale) not in _cache:
        from yolomi.arch import GraphBuilder
        _cache[("sharp", scale)] = MO.sharpen(_cache[("sd", scale)], GraphBuilder(scale, "detect").ops, MO.SHARP)
    return _cache[("sharp", scale)]


def engine(scale, plan, kind="plain"):
    from core.model import YOLO11Model
    k = ("m", scale, plan, kind)
    if k not in _cache:
        dtype, env = PLANS[plan]
        old = {e: os.environ.get(e) for e in env}
        os.environ.update(env)
        try:
            m = YOLO11Model(task="detect", size=scale, device="cuda:0", dtype=dtype, verbose=False,
                            state_dict=weights(scale, kind) if kind != "plain" else None)
        finally:
            for e, v in old.items():
                os.environ.pop(e, None) if v is None else os.environ.__setitem__(e, v)
        m.model.engine.autotune = False
        _cache[k] = m
    return _cache[k].model.engine


def batch(shape, B):
    if ("x", shape, B) not in _cache:
        _cache[("x", shape, B)] = MO.batch(shape, B)
    return _cache[("x", shape, B)]


# ---------------------------------------------------------------------------------------------- views of an op
def _span(v):
    """(buffer id, first channel, end channel) of a View, or of a whole buffer."""
    return (v.buf.id, v.coff, v.coff + v.C) if hasattr(v, "buf") else (v.id, 0, v.C)


def _io(op):
    """The (input, output) channel spans of a misc op, from the graph's records."""
    a = op.args
    if op.kind == "sppf":  # pools cat[0:C] into cat[C:4C] in place
        b, c0, _ = _span(a["src"])
        return (b, c0, c0 + a["C"]), (b, c0 + a["C"], c0 + 4 * a["C"])
    return _span(a["qkv"] if op.kind == "attn" else a["src"]), _span(a["dst"])


def _written(op):
    if op.kind in ("sppf", "attn", "dwconv"):
        return _io(op)[1]
    d = op.args.get("dst")
    return _span(d) if d is not None and (hasattr(d, "buf") or hasattr(d, "id")) else None


def overwritten_later(ops, i):
    """A later op of the forward writes into op i's input or output span (anchor rows of other levels aside)."""
    for j in range(i + 1, len(ops)):
        w = _written(ops[j])
        if w is None:
            continue
        for s in _io(ops[i]):
            if s[0] == w[0] and s[1] < w[2] and w[1] < s[2]:
                li, lj = ops[i].args.get("anchor_level", -1), ops[j].args.get("anchor_level", -1)
                if li >= 0 and lj >= 0 and li != lj:
                    continue
                return True
    return False


class Reader:
    """The spans of one forward: each buffer read back once, raw; values in float64 (an x3 pair as hi + lo, exact)."""

    def __init__(self, eng, B):
        self.eng, self.B, self.bufs = eng, B, {}

    def raw(self, span):
        b, c0, c1 = span
        if b not in self.bufs:
            self.bufs[b] = self.eng.read_buffer(b, self.B, raw=True)
        pair = self.eng.dtype == "x3" and not self.eng.graph.buffers[b].f32
        return (self.bufs[b][..., 2 * c0:2 * c1] if pair else self.bufs[b][..., c0:c1]), pair

    def values(self, span):
        r, pair = self.raw(span)
        if not pair:
            return r.double()
        B, H, W, C2 = r.shape
        hl = r.double().reshape(B, H, W, C2 // 16, 2, 8)
        return (hl[..., 0, :] + hl[..., 1, :]).reshape(B, H, W, C2 // 2)


def run(eng, x):
    """One eager one-lane forward; returns the per-op variant codes."""
    B, _, H, W = x.shape
    eng.run(x.to(DEV), use_graph=False, lanes=1)
    return eng.rt.get_op_variant(B, H, W)


def reader_of(eng, x, i):
    """A Reader on which op i's input and output are the ones op i saw and wrote: the whole forward just run when no
    later op writes into them (the graph's records say), else a forward stopped behind op i (YM_DBG_STOP)."""
    from yolomi import lib as L
    if overwritten_later(eng.graph.ops, i):
        prev = L.set_debug(L.DBG_STOP, i + 1)
        try:
            eng.run(x.to(DEV), use_graph=False, lanes=1)
        finally:
            L.set_debug(L.DBG_STOP, prev)
    return Reader(eng, x.shape[0])


def fail_text(what, idx, err, e, r):
    return f"{what}: worst (b, y, x, c) = {idx}, err {err:.3e} / E {e:.3e} = {r:.2f}"


# ---------------------------------------------------------------------------------------------- attention, SPPF
def required(plan, name, kind, N):
    """Whether a mutation must break E (module docstring); the others' ratios are printed."""
    return plan != "f16" or name in TILE_MUTS or (kind == "sharp" and N <= 143)


def check_attn(plan, a, sd, qkv, got, kind, label, nh):
    """Holds an attention output to E and every applying mutation to breaking it; returns the printed line's tail."""
    ref, E, _ = MO.attn_reference(plan, a, sd, qkv)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    r, idx, err, e = MO.worst(got, ref, E)
    assert r <= 1.0, fail_text(label, idx, err, e, r)
    H, W = qkv.shape[1:3]
    power = []
    for name in MO.MUTATIONS:
        if not MO.applies(name, H, W, nh):
            continue
        bad, _, _ = MO.attn_reference(plan, a, sd, qkv, mutation=name)
        m = MO.worst(bad, ref, E)[0]  # how far the wrong answer lies outside the bound, on these very tensors
        power.append(f"{name} {m:.1f}")
        if required(plan, name, kind, H * W):
            assert m > 1.0, f"{label}: mutation {name} stays within E (|mutation - ref| / E = {m:.2f})"
    return f"worst err/E {r:.3f}; mutations: " + ", ".join(power)


def check_sppf(rd, op, label):
    src, dst = _io(op)
    want = MO.sppf_reference(rd.values(src))
    got = rd.values(dst)
    assert got.shape == want.shape, (label, got.shape, want.shape)
    bad = (got != want).nonzero()
    assert bad.numel() == 0, f"{label}: {len(bad)} pooled values differ, first (b, y, x, c) = {tuple(bad[0].tolist())}"


def check_case(plan, case):
    from yolomi import lib as L
    scale, shape, B, kind, _, expect = case
    eng, sd = engine(scale, plan, kind), weights(scale, kind)
    x = batch(shape, B)
    codes = run(eng, x)
    ops = eng.graph.ops
    label = f"misc-ops {plan} yolo11{scale} {shape} B={B} {kind}"
    n_attn = n_sppf = 0
    for i, op in enumerate(ops):
        if op.kind == "attn":
            name = L.ATTN_VARIANTS[codes[i]] if codes[i] >= 0 else None
            assert name == expect[plan], (label, op.name, name, expect[plan])
            _ran["attn"].add(name)
            rd = reader_of(eng, x, i)
            src, dst = _io(op)
            tail = check_attn(plan, op.args, sd, rd.values(src), rd.values(dst), kind, f"{label} {op.name} {name}",
                              op.args["nh"])
            print(f"{label} attn {name}: {tail}")
            n_attn += 1
        elif op.kind == "sppf":
            HW = (x.shape[2] // 32) * (x.shape[3] // 32)
            want = "sep" if HW * (2 if plan == "f16" else 4) <= 4096 else "direct"  # ym_launch_sppf: 4 images of 8 channels in 128 KiB
            name = L.SPPF_VARIANTS[codes[i]] if codes[i] >= 0 else None
            assert name == want, (label, op.name, name, want)
            _ran["sppf"].add(name)
            check_sppf(reader_of(eng, x, i), op, f"{label} {op.name} {name}")
            print(f"{label} sppf {name}: equal")
            n_sppf += 1
        else:
            assert codes[i] == -1 or op.kind == "dwconv", (op.name, codes[i])
    assert n_attn >= 1 and n_sppf == 1, label
    _cache[("ran", plan) + tuple(case[:4])] = True


def _case_id(c):
    return f"{c[0]}-{c[1]}-b{c[2]}-{c[3]}"


PLAN_CASES = [(plan, c) for c in CASES for plan in c[4]]


@pytest.mark.parametrize("plan,case", PLAN_CASES, ids=[f"{p}-{_case_id(c)}" for p, c in PLAN_CASES])
def test_attention_and_sppf_match_float64(plan, case):
    """One forward of a case: its attention output within E of float64 and every required mutation outside it, its
    three pooled slices equal to float64 max pooling, and both ops on the instantiation the launch rule names."""
    check_case(plan, case)


def flash_off_child(plan, path):
    """Child process body (YM_ATTN_FLASH_OFF=1 is read once per process): yolo11n 736x736, saves the attention op's
    stored qkv and output (float64 values) and its variant code."""
    eng = engine("n", plan)
    x = batch("736x736", 1)
    codes = run(eng, x)
    i = [j for j, op in enumerate(eng.graph.ops) if op.kind == "attn"][0]
    rd = reader_of(eng, x, i)
    src, dst = _io(eng.graph.ops[i])
    np.savez(path, qkv=rd.values(src).numpy(), dst=rd.values(dst).numpy(), code=codes[i])


@pytest.mark.parametrize("plan", ["f16", "x3"])
def test_scalar_attention_on_fp16_and_pair_storage(plan, tmp_path):
    """attn_psa<f16, 8> / attn_psa<P2, 8>: the fall-back of the f16 / x3 plans behind N = 512 when flash is switched
    off, at N = 529, run in a fresh child process; the parent holds the saved tensors to the plan's E."""
    from yolomi import lib as L
    path = str(tmp_path / f"scalar_{plan}.npz")
    code = ("import sys; sys.path[:0] = [%r, %r]; from tests.test_gpu_misc_ops import flash_off_child; "
            "flash_off_child(sys.argv[1], sys.argv[2])" % (os.path.join(ROOT, "yolo-infer_amd"), ROOT))
    subprocess.run([sys.executable, "-c", code, plan, path], check=True, timeout=240,
                   env=dict(os.environ, YM_ATTN_FLASH_OFF="1"))
    z = np.load(path)
    name = L.ATTN_VARIANTS[int(z["code"])]
    assert name == "scalar_qb8", name  # 2 x ceil(529 / 16) = 68 workgroups < 512
    from yolomi.arch import GraphBuilder
    a = [op.args for op in GraphBuilder("n", "detect").ops if op.kind == "attn"][0]
    label = f"misc-ops {plan} yolo11n 736x736 B=1 plain flash-off"
    tail = check_attn(plan, a, weights("n"), torch.from_numpy(z["qkv"]), torch.from_numpy(z["dst"]), "plain", label, a["nh"])
    print(f"{label} attn {name}: {tail}")


@pytest.mark.parametrize("shape", ["352x416", "480x672", "640x800"])
def test_x3_attention_with_eight_key_tiles_per_round_trip(shape):
    """YM_DBG_ATTN_KB = 1 (attn_psa_x3<NKT, 8>, the other KB instantiation of NKT 16 / 26 / 32): within E, the same
    variant code (the code names NKT, not KB)."""
    from yolomi import lib as L
    eng, x = engine("n", "x3"), batch(shape, 1)
    prev = L.set_debug(L.DBG_ATTN_KB, 1)
    try:
        codes = run(eng, x)
        i = [j for j, op in enumerate(eng.graph.ops) if op.kind == "attn"][0]
        rd = reader_of(eng, x, i)
    finally:
        L.set_debug(L.DBG_ATTN_KB, prev)
    op = eng.graph.ops[i]
    nkt = -(-(x.shape[2] // 32) * (x.shape[3] // 32) // 16)
    assert L.ATTN_VARIANTS[codes[i]] == f"x3_nkt{min(n for n in (8, 16, 26, 32) if nkt <= n)}"
    src, dst = _io(op)
    label = f"misc-ops x3 yolo11n {shape} B=1 plain KB=8"
    print(f"{label} attn: " + check_attn("x3", op.args, weights("n"), rd.values(src), rd.values(dst), "plain", label, op.args["nh"]))


@pytest.mark.parametrize("plan", ATTN_PLANS)
@pytest.mark.parametrize("shape,B", [("96x160", 3), ("736x736", 1)])
def test_second_forward_leaves_attention_and_pools_bit_equal(plan, shape, B):
    eng, x = engine("n", plan), batch(shape, B)
    outs = []
    for _ in range(2):
        run(eng, x)
        got = []
        for i, op in enumerate(eng.graph.ops):
            if op.kind in ("attn", "sppf"):
                got.append((op.name, reader_of(eng, x, i).raw(_io(op)[1])[0].clone()))
        outs.append(got)
    assert len(outs[0]) >= 2
    for (n, p), (_, q) in zip(*outs):
        assert torch.equal(p, q), n


# ---------------------------------------------------------------------------------------------- depthwise
def dw_expect(mode, tile, B, H, W, C, f16):
    """csrc/ym_op_select.h ym_select_dwconv restated: mode 0 the LDS tile; mode 2 a strip where the grid keeps >= 256
    workgroups; else (and mode 1) 4 pixels per thread for f16 where that leaves >= 128 workgroups and W % 4 == 0, 2 where
    W is even, the one-pixel kernel at odd widths."""
    if mode == 0:
        return f"lds{tile}"
    total = B * H * W * (C // 8)
    if mode == 2:
        px = 4 if W % 4 == 0 else (2 if W % 2 == 0 else 0)
        blocks = lambda p, rt: (B * -(-H // rt) * (W // p) * (C // 8) + 255) // 256
        rt = (4 if blocks(px, 4) >= 256 else (2 if blocks(px, 2) >= 256 else 0)) if px else 0
        if px == 4 and rt == 4:
            return "strip4"
        if px and rt == 2:
            return "strip2"
    if f16 and total // 4 >= 128 * 256 and W % 4 == 0:
        return "row4"
    return "row2" if W % 2 == 0 else "pixel"


def dw_forward(eng, x, mode, tile):
    """One forward under a depthwise mode / tile; {op name: (variant name, values in, values out, raw out)}."""
    from yolomi import lib as L
    pm, pt = L.set_debug(L.DBG_DW_MODE, mode), L.set_debug(L.DBG_DW_TILE, tile)
    try:
        codes = run(eng, x)
        out = {}
        for i, op in enumerate(eng.graph.ops):
            if op.kind == "dwconv":
                rd = reader_of(eng, x, i)
                src, dst = _io(op)
                out[op.name] = (L.DW_VARIANTS[codes[i]] if codes[i] >= 0 else None, rd.values(src), rd.values(dst),
                                rd.raw(dst)[0].clone())
    finally:
        L.set_debug(L.DBG_DW_MODE, pm)
        L.set_debug(L.DBG_DW_TILE, pt)
    return out


@pytest.mark.parametrize("plan", DW_PLANS)
@pytest.mark.parametrize("shape,B", [("96x160", 3), ("160x224", 1)])
def test_depthwise_variants_match_float64_and_each_other(plan, shape, B):
    """Every dwconv of the Detect head on maps 12x20 ... 3x5 and 20x28 ... 5x7 (widths 4k, 2k and odd): the row /
    one-pixel kernels (mode 1) within E of float64; the four LDS tiles (mode 0) and mode 2 bitwise equal to mode 1, as
    every variant's comment claims; each on the instantiation the launch rule names."""
    dtype = PLANS[plan][0]
    eng, sd, x = engine("n", plan), weights("n"), batch(shape, B)
    ops = {op.name: op.args for op in eng.graph.ops if op.kind == "dwconv"}
    assert len(ops) == 6
    base = dw_forward(eng, x, 1, 0)
    worst_r, widths = 0.0, set()
    for name, (var, src, got, _) in base.items():
        H, W, C = src.shape[1:]
        widths.add(W % 4 == 0 and 4 or (W % 2 == 0 and 2 or 1))
        assert var == dw_expect(1, 0, B, H, W, C, dtype == "f16"), (name, var)
        _ran["dwconv"].add(var)
        ref, E, _ = MO.dw_reference(dtype, ops[name], sd, src)
        r, idx, err, e = MO.worst(got, ref, E)
        assert r <= 1.0, fail_text(f"misc-ops {plan} yolo11n {shape} {name} {var}", idx, err, e, r)
        worst_r = max(worst_r, r)
    assert widths == {4, 2, 1}
    for mode, tile in ((0, 0), (0, 1), (0, 2), (0, 3), (2, 0)):
        for name, (var, src, _, raw) in dw_forward(eng, x, mode, tile).items():
            H, W, C = src.shape[1:]
            assert var == dw_expect(mode, tile, B, H, W, C, dtype == "f16"), (name, mode, tile, var)
            _ran["dwconv"].add(var)
            assert torch.equal(src, base[name][1]), (name, "input differs between forwards")
            assert torch.equal(raw, base[name][3]), f"{plan} {shape} {name}: mode {mode} tile {tile} ({var}) is not bit-equal to mode 1 ({base[name][0]})"
    print(f"misc-ops {plan} yolo11n {shape} B={B} dwconv: mode 1 worst err/E {worst_r:.3f}; LDS tiles 0-3 and mode 2 bit-equal")
    _cache[("ran-dw", plan, shape)] = True


# ---------------------------------------------------------------------------------------------- non-vacuity
def test_every_variant_ran():
    """Over the cases above every code of ym_op_variant_count was launched, or is on NEVER_RUN with its reason; the
    list is exact (an instantiation that starts to run, or a new code, fails here until it is parametrised)."""
    from yolomi import lib as L
    lib = L.load_library()
    names = {"attn": L.ATTN_VARIANTS, "sppf": L.SPPF_VARIANTS, "dwconv": L.DW_VARIANTS}
    kinds = {"attn": L.OP_ATTN, "sppf": L.OP_SPPF, "dwconv": L.OP_DWCONV}
    for k in names:
        assert lib.ym_op_variant_count(kinds[k]) == len(names[k]), k
    for case in CASES:  # whatever this session has not run yet (a forward and its checks)
        for plan in case[4]:
            if ("ran", plan) + tuple(case[:4]) not in _cache:
                check_case(plan, case)
    for plan in DW_PLANS:
        for shape, B in (("96x160", 3), ("160x224", 1)):
            if ("ran-dw", plan, shape) not in _cache:
                test_depthwise_variants_match_float64_and_each_other(plan, shape, B)
    for k in names:
        missing = [n for n in names[k] if n not in _ran[k]]
        print(f"misc-ops never run {k}: {missing}")
        assert missing == [n for n in names[k] if n in NEVER_RUN[k]], (k, missing, sorted(NEVER_RUN[k]))
    assert list(NEVER_RUN["attn"]) == ["scalar_qb4"]
