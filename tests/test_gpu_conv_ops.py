"""Every conv op of a plan, on every conv tile configuration, against float64 computed from the op's own stored input
(tests/conv_oracle.py: the reference, the per-element bound E and where its numbers come from), at small awkward
shapes — and known to have run: after each pinned forward the runtime says per op whether the pinned id's kernel was
the one launched (ym_get_op_cfg_taken), so an id that silently fell back on every op cannot pass for having run.

Shapes (multiples of 32, as ym_infer requires): 96x160 B=3 (maps 48x80 ... 3x5: M = 45 at stride 32, under one tile
and odd; width 5) and 160x224 B=1 (maps 80x112 ... 5x7: M = 35 / 140 / 560, widths 7 / 14 / 28).  yolo11n runs both,
yolo11s (the (64,32,64) / (64,64,64) Bottleneck shapes, the K = 4608 convs) the second.

Views that a later op of the same forward overwrites (C3k's cv1 || cv2 slice, which the last Bottleneck writes into)
are read from a forward stopped behind the op (YM_DBG_STOP)."""
import os

import numpy as np
import pytest
import torch

from tests import conv_oracle as CO
from tests.golden.make_golden import make_input
from yolomi.synth import synth_weights

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SHAPES = {"96x160": (96, 160, (301, 302, 303)), "160x224": (160, 224, (311,)), "32x352": (32, 352, (321,))}
RUNS = {"n": ("96x160", "160x224"), "s": ("160x224",)}  # (scale -> shapes) of every plan
# A third yolo11n shape for the Bottleneck families alone: their 80-pixel-wide tiles split only a map wider than 80
# (csrc/ym_conv_bneck.hip launch: `TW >= a.Wo` is refused), and the widest paired map of the two shapes above is 56.
# 32x352 has an 8x88 map at stride 4.  (A 320x320 input would not do: its stride-4 map is exactly 80 wide.)
WIDE = "32x352"
WIDE_FAMILIES = ("bneck", "bneck_x3")
SPLIT_TAG = 1 << 20  # csrc/ym_conv_catalog.h kSplitTag: a fused pair run as its two convs, ids 256 * first + second
SPLIT = "split"      # the parametrised stand-in for SPLIT_TAG + 256 * 3 + 3 (both halves on direct tile 3)

# csrc/ym_conv.hip's id space (ym_launch_conv): families as (name, first id, count); x3 appends two x3-only families
F16_FAMILIES = (("direct", 0, 12), ("lds", 12, 5), ("dma", 17, 30), ("stream", 47, 31), ("small", 78, 12),
                ("halo", 90, 12), ("bneck", 102, 14))
N_F16 = 116
X3_FAMILIES = (("dma_x3", N_F16, 9), ("bneck_x3", N_F16 + 9, 2))  # x3-only LDS-DMA split-K and Bottleneck ids
# plan variant -> (dtype, environment while the model is built).  The nofuse variants (YM_FUSE=0: no fused pairs, no
# merged GEMM) are there for the streaming family alone: the fused plans hide every conv with a storage K of 64 or, in
# x3, 192 inside a pair, and the streaming kernels of those K steps would otherwise never run on a single conv.
# x3dwall (YM_DW_FUSE_STRIDES=8,16,32: the depthwise ops of every head level fused, not P3's alone) is there for the
# depthwise-fused ids 0..7: its 8-way K split needs 8 K blocks of 32 channels, which only the P5 input (256) has.
PLANS = {"x3": ("x3", {}), "x3nodw": ("x3", {"YM_FUSE_DW": "0"}), "x3nofuse": ("x3", {"YM_FUSE": "0"}),
         "x3dwall": ("x3", {"YM_DW_FUSE_STRIDES": "8,16,32"}),
         "f16": ("f16", {}), "f16nofuse": ("f16", {"YM_FUSE": "0"}), "f32": ("f32", {})}
DTYPE_PLANS = {"x3": ("x3", "x3nodw", "x3nofuse", "x3dwall"), "f16": ("f16", "f16nofuse"), "f32": ("f32",)}
# families of the shared id space that the launchers refuse for every x3 conv (not x3 families: no cap applies; the
# test still holds them to "never taken", so enabling one fails until it is parametrised as a family)
X3_REFUSED = {"small": "csrc/ym_conv_stream.hip dispatch<OutT, X3 = true>: `if constexpr (X3) return "
                       "hipErrorInvalidValue` in front of the small-M kernels (they split K four ways: no x3 pairing)",
              "halo": "csrc/ym_conv_catalog.h kAdmit: the x3 row of a single conv admits the direct, LDS, LDS-DMA and "
                      "streaming families, not `halo`; ym_launch_conv_halo is f16 only"}

_cache = {}


def ncfg(dtype):
    from yolomi.lib import DTYPE_CODES, load_library
    return load_library().ym_num_conv_cfgs(DTYPE_CODES[dtype])


def families(plan):
    fam = list(F16_FAMILIES)
    if PLANS[plan][0] == "x3":
        fam += list(X3_FAMILIES)
    if plan == "f32":
        fam = [("direct", 0, 12)]
    return fam


def plan_ids(plan):
    """The ids a plan is run on.  x3nodw is the x3 plan with its Detect-head depthwise ops unfused, there for the fused
    pairs the default plan does not have: the families that have a pair kernel, not the single-conv ones again."""
    if plan == "f32":
        return [-1] + list(range(12))
    fam = dict((n, (f, c)) for n, f, c in families(plan))
    if plan == "x3nodw":
        ids = [-1, SPLIT]
        for n in ("dma", "stream", "bneck", "bneck_x3"):
            ids += list(range(fam[n][0], fam[n][0] + fam[n][1]))
        return ids
    if plan == "x3dwall":
        return [-1] + list(range(8))
    if plan.endswith("nofuse"):
        return [-1] + list(range(fam["stream"][0], fam["stream"][0] + fam["stream"][1]))
    return [-1, SPLIT] + list(range(sum(c for _, _, c in families(plan))))


def test_the_id_space_is_the_librarys():
    """The families above cover ym_num_conv_cfgs exactly: a configuration added to the library fails here until it is
    parametrised."""
    for plan in ("x3", "f16"):
        assert ncfg(PLANS[plan][0]) == sum(c for _, _, c in families(plan)), plan


def engine(scale, plan):
    from core.model import YOLO11Model
    k = ("m", scale, plan)
    if k not in _cache:
        dtype, env = PLANS[plan]
        old = {e: os.environ.get(e) for e in env}
        os.environ.update(env)
        try:
            m = YOLO11Model(task="detect", size=scale, device="cuda:0", dtype=dtype, verbose=False)
        finally:
            for e, v in old.items():
                os.environ.pop(e, None) if v is None else os.environ.__setitem__(e, v)
        m.model.engine.autotune = False  # no ym_tune, no table written: the test pins every id itself
        _cache[k] = m
    return _cache[k].model.engine


def weights(scale):
    if ("sd", scale) not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        _cache[("sd", scale)] = synth_weights(scale, "detect", 0)
    return _cache[("sd", scale)]


def batch(shape):
    if ("x", shape) not in _cache:
        H, W, seeds = SHAPES[shape]
        _cache[("x", shape)] = make_input("uniform", seeds, 640)[:, :, :H, :W].contiguous()
    return _cache[("x", shape)]


# ---------------------------------------------------------------------------------------------- views of an op
def _written(op):
    """(buffer id, first channel, end channel) an op writes, or None."""
    a = op.args
    if op.kind == "sppf":  # pools cat[0:C] into cat[C:4C] in place
        return a["dst"].id, a["src"].coff + a["C"], a["src"].coff + 4 * a["C"]
    d = a.get("dst")
    if d is None or not hasattr(d, "buf"):
        return None
    return d.buf.id, d.coff, d.coff + d.C


def _views(op):
    a = op.args
    return [v for v in (a["src0"], a["src1"], a["res"], a["dst"]) if v is not None]


def overwritten_later(ops, i):
    """A later op of the forward writes into one of op i's input or output views (found from the graph's records)."""
    for j in range(i + 1, len(ops)):
        w = _written(ops[j])
        if w is None:
            continue
        for v in _views(ops[i]):
            if v.buf.id == w[0] and v.coff < w[2] and w[1] < v.coff + v.C:
                if ops[j].args.get("anchor_level", -1) >= 0 and ops[i].args.get("anchor_level", -1) >= 0 and \
                        ops[j].args["anchor_level"] != ops[i].args["anchor_level"]:
                    continue  # other rows of the anchor-major buffer
                return True
    return False


class Reader:
    """The views of one forward, each buffer read back once."""

    def __init__(self, eng, x, B):
        self.eng, self.x, self.B, self.bufs = eng, x, B, {}

    def view(self, v, level=-1, hw=None):
        g = self.eng.graph
        if v.buf is g.input:
            return self.x.permute(0, 2, 3, 1)[..., :v.C]
        if v.buf.id not in self.bufs:
            self.bufs[v.buf.id] = self.eng.read_buffer(v.buf.id, self.B)
        t = self.bufs[v.buf.id]
        if level >= 0:  # rows [off, off + Ho * Wo) of the anchor-major buffer
            H, W = self.x.shape[2:]
            from yolomi.arch import STRIDES
            off = sum((H // s) * (W // s) for s in STRIDES[:level])
            t = t.reshape(self.B, -1, t.shape[-1])[:, off:off + hw[0] * hw[1]].reshape(self.B, hw[0], hw[1], -1)
        return t[..., v.coff:v.coff + v.C]


def op_cfgs(eng, cid):
    ops = eng.graph.ops
    if cid == SPLIT:
        return [SPLIT_TAG + 256 * 3 + 3 if op.kind == "conv" and op.args.get("pair") else -1 for op in ops]
    return [cid if op.kind == "conv" else -1 for op in ops]


def pinned_forward(eng, x, cid):
    """One eager forward of x with `cid` pinned on every conv op; returns the per-op (taken, taken of the second half)."""
    B, _, H, W = x.shape
    if (B, H, W) not in eng._tuned:
        eng.run(x, use_graph=False, lanes=1)  # the shape's workspace (no table: autotune is off)
    eng.rt.set_op_cfg(B, H, W, op_cfgs(eng, cid))
    eng.run(x, use_graph=False, lanes=1)
    return eng.rt.get_op_cfg_taken(B, H, W)


def check_forward(scale, plan, shape, cid):
    """Pins `cid`, runs, and holds every conv op to its bound.  Returns ({op name: taken}, worst err / E, its op)."""
    from yolomi import lib as L
    eng, sd = engine(scale, plan), weights(scale)
    dtype = PLANS[plan][0]
    x = batch(shape)
    xd = x.to(DEV)
    B = x.shape[0]
    ops = eng.graph.ops
    taken = pinned_forward(eng, xd, cid)
    whole = Reader(eng, x, B)
    n_checked, top, top_taken = 0, (0.0, ""), (0.0, "")
    rec = {}
    convs = [i for i, op in enumerate(ops) if op.kind == "conv"]
    late = [i for i in convs if overwritten_later(ops, i)]
    # the ops whose views survive the whole forward first: a stopped forward rewrites the buffers it reaches
    for i in [i for i in convs if i not in late] + late:
        op = ops[i]
        a = op.args
        rd = whole
        if i in late:  # read its views from a forward that ends behind it
            prev = L.set_debug(L.DBG_STOP, i + 1)
            try:
                eng.run(xd, use_graph=False, lanes=1)
            finally:
                L.set_debug(L.DBG_STOP, prev)
            rd = Reader(eng, x, B)
        src0 = rd.view(a["src0"])
        src1 = rd.view(a["src1"]) if a["src1"] is not None else None
        res = rd.view(a["res"]) if a["res"] is not None else None
        ref, E, _ = CO.reference(dtype, a, sd, src0, src1, res)
        got = rd.view(a["dst"], a["anchor_level"], ref.shape[1:3])
        assert got.shape == ref.shape, (op.name, got.shape, ref.shape)
        r, idx, err, e = CO.worst(got, ref, E)
        rec[op.name] = taken[i]
        if r > top[0]:
            top = (r, op.name)
        if 1 in taken[i] and r > top_taken[0]:
            top_taken = (r, op.name)
        assert r <= 1.0, (f"{plan} yolo11{scale} {shape} op {op.name} cfg {cid} taken {taken[i]}: "
                          f"worst (b, y, x, c) = {idx}, err {err:.3e} / E {e:.3e} = {r:.2f}")
        n_checked += 1
    assert n_checked == sum(op.kind == "conv" for op in ops)
    eng._tuned.discard((B,) + tuple(x.shape[2:]))
    _cache[("taken", scale, plan, shape, cid)] = rec
    print(f"conv-ops {plan} yolo11{scale} {shape} cfg {cid}: worst err/E {top[0]:.3f} at {top[1]}; "
          f"taken on {sum(1 for t in rec.values() if t[0] == 1)} ops, worst of them {top_taken[0]:.3f} at {top_taken[1]}")
    return rec, top


def shapes_of(scale, plan, cid):
    if scale == "n" and cid not in (-1, SPLIT) and any(n in WIDE_FAMILIES and f <= cid < f + c
                                                       for n, f, c in families(plan)):
        return RUNS[scale] + (WIDE,)
    return RUNS[scale]


def taken_of(scale, plan, shape, cid):
    """The taken record of a (scale, plan, shape, id): from the check that ran in this session, else a forward alone."""
    k = ("taken", scale, plan, shape, cid)
    if k not in _cache:
        eng = engine(scale, plan)
        x = batch(shape)
        t = pinned_forward(eng, x.to(DEV), cid)
        eng._tuned.discard((x.shape[0],) + tuple(x.shape[2:]))
        _cache[k] = {op.name: t[i] for i, op in enumerate(eng.graph.ops) if op.kind == "conv"}
    return _cache[k]


def _cases():
    out = []
    for plan in PLANS:
        out += [(plan, c) for c in plan_ids(plan)]
    return out


def pytest_generate_tests(metafunc):
    if "plan_cfg" in metafunc.fixturenames:
        cases = _cases()
        metafunc.parametrize("plan_cfg", cases, ids=[f"{p}-{c}" for p, c in cases])
    if "plan_family" in metafunc.fixturenames:
        cases = []
        for plan in PLANS:
            ids = set(plan_ids(plan))
            cases += [(plan, "heuristic", (-1, SPLIT) if SPLIT in ids else (-1,))]
            for n, f, c in families(plan):
                for lo in range(f, f + c, 8):  # at most 8 ids per case
                    sub = tuple(i for i in range(lo, min(lo + 8, f + c)) if i in ids)
                    if sub:
                        cases.append((plan, f"{n}{(lo - f) // 8}", sub))
        metafunc.parametrize("plan_family", cases, ids=[f"{p}-{n}" for p, n, _ in cases])


def test_yolo11n_conv_ops_match_float64(plan_cfg):
    """yolo11n, both shapes, one id pinned on every conv op: every conv op within its bound of float64."""
    plan, cid = plan_cfg
    for shape in shapes_of("n", plan, cid):
        rec, _ = check_forward("n", plan, shape, cid)
        if cid == SPLIT:  # direct tile 3 takes every conv: both halves of every pair ran on it
            pairs = [t for n, t in rec.items() if t != (-1, -1)]
            assert pairs and all(t == (1, 1) for t in pairs), rec


def test_yolo11s_conv_ops_match_float64(plan_family):
    """yolo11s at 160x224 B=1, the ids of one family (eight at most) in turn."""
    plan, _, ids = plan_family
    for cid in ids:
        check_forward("s", plan, RUNS["s"][0], cid)


# ---------------------------------------------------------------------------------------------- non-vacuity
# Ids that no op of yolo11n (96x160 B=3, 160x224 B=1) or yolo11s (160x224 B=1) takes, per plan, each with the
# launcher condition that excludes it.  test_every_id_ran_somewhere holds the never-taken set to exactly this list.
# Every entry below is a streaming id 47 + i of csrc/ym_conv_stream.hip YM_STREAM_CFGS (i, kind, KS, ...), excluded by
# `launch`: `if (a.Kpad != KS * 32 || a.k != KIND) return hipErrorInvalidValue` — the kernel holds a whole K of exactly
# KS 32-element steps.  Kpad is the storage K rounded up to 64: k*k*cin fp16 elements in f16 plans, twice that in x3.
_K3_KS4 = "3x3, KS 4 (Kpad 128): "
_X3_K3_KS4 = _K3_KS4 + "an x3 3x3 conv has Kpad >= 2*9*8 = 144 -> 192, so no x3 conv of any model can have Kpad 128"
NEVER_TAKEN = {
    "x3": {54: _X3_K3_KS4, 58: _X3_K3_KS4, 65: _X3_K3_KS4, 77: _X3_K3_KS4},
    "f16": {},
    "f32": {},
}
# Ids that no op of a dtype's DEFAULT plan takes and only a plan variant above does (the fused plans have no such
# single conv).
_F16_K3_KS4 = _K3_KS4 + "only a 3x3 conv of 8 input channels (yolo11n model.2.m.0.cv2), inside a fused Bottleneck unless YM_FUSE=0"
_X3_K1_KS2 = ("1x1, KS 2 (x3 Kpad 64: cin <= 32): only yolo11n model.2.cv1 / model.2.m.0 inputs, inside fused pairs "
              "unless YM_FUSE=0")
_X3_K3_KS6 = "3x3, KS 6 (x3 Kpad 192: cin 8): only yolo11n model.2.m.0.cv2, inside a fused Bottleneck unless YM_FUSE=0"
VARIANT_ONLY = {
    "x3": {47: _X3_K1_KS2, 48: _X3_K1_KS2, 49: _X3_K1_KS2, 62: _X3_K1_KS2, 63: _X3_K1_KS2, 75: _X3_K1_KS2,
           55: _X3_K3_KS6, 59: _X3_K3_KS6, 66: _X3_K3_KS6},
    "f16": {54: _F16_K3_KS4, 58: _F16_K3_KS4, 65: _F16_K3_KS4, 77: _F16_K3_KS4},
    "f32": {},
}
# Ids that no op of the default yolo11n plan takes (NEVER_TAKEN, VARIANT_ONLY, and those only yolo11s' channel widths
# admit).  tests/test_gpu_parity.py and tests/test_gpu_x3.py pin ids on the default yolo11n plans: an id may run on no op
# there only if it is listed here.
_F16_K3_KS10 = ("3x3, KS 10 (Kpad 320: cin 32): in yolo11n only inside Bottleneck pairs, which take the kernels of "
                "csrc/ym_conv_bneck.hip alone (ym_launch_conv: k2 == 3); yolo11s has them as single convs")
_X3_K3_KS18 = ("3x3, KS 18 (x3 Kpad 576: cin 32): in yolo11n only inside Bottleneck pairs (ym_launch_conv: k2 == 3 takes "
               "csrc/ym_conv_bneck.hip alone); yolo11s has them in 3x3 -> 1x1 pairs")
NOT_ON_YOLO11N = {
    "x3": {**NEVER_TAKEN["x3"], **VARIANT_ONLY["x3"], 57: _X3_K3_KS18, 61: _X3_K3_KS18},
    "f16": {**VARIANT_ONLY["f16"], 56: _F16_K3_KS10, 60: _F16_K3_KS10, 76: _F16_K3_KS10},
    "f32": {},
}


def ran_somewhere(dtype, cid, plans=None, scales=RUNS):
    for plan in plans or DTYPE_PLANS[dtype]:
        if cid not in plan_ids(plan):
            continue
        for scale in scales:
            for shape in shapes_of(scale, plan, cid):
                if any(t[0] == 1 for t in taken_of(scale, plan, shape, cid).values()):
                    return True
    return False


@pytest.mark.parametrize("dtype", list(DTYPE_PLANS))
def test_every_id_ran_somewhere(dtype):
    """Over the (plan variant, scale, shape) set of a dtype every id is taken by at least one op, or is on NEVER_TAKEN
    with its reason; the list is exact (an id that starts to run, or stops, fails here) and holds at most a quarter
    of a family.  x3: the two families the launchers refuse as a whole (X3_REFUSED) are never taken either."""
    fams = families(DTYPE_PLANS[dtype][0])
    refused = X3_REFUSED if dtype == "x3" else {}
    missing = [cid for n, f, c in fams for cid in range(f, f + c) if not ran_somewhere(dtype, cid)]
    print(f"conv-ops never taken {dtype}: {missing}")
    for n, f, c in fams:
        if n in refused:
            assert all(cid in missing for cid in range(f, f + c)), n
            missing = [cid for cid in missing if not f <= cid < f + c]
    assert missing == sorted(NEVER_TAKEN[dtype]), (missing, sorted(NEVER_TAKEN[dtype]))
    for n, f, c in fams:
        k = sum(1 for i in missing if f <= i < f + c)
        assert 4 * k <= c, (n, k, c)
    variant = [cid for n, f, c in fams for cid in range(f, f + c)
               if ran_somewhere(dtype, cid) and not ran_somewhere(dtype, cid, DTYPE_PLANS[dtype][:1])]
    print(f"conv-ops variant only {dtype}: {variant}")
    assert variant == sorted(VARIANT_ONLY[dtype]), (variant, sorted(VARIANT_ONLY[dtype]))
    not_n = [cid for n, f, c in fams for cid in range(f, f + c)
             if n not in refused and not ran_somewhere(dtype, cid, DTYPE_PLANS[dtype][:1], ("n",))]
    print(f"conv-ops not on yolo11n {dtype}: {not_n}")
    assert not_n == sorted(NOT_ON_YOLO11N[dtype]), (not_n, sorted(NOT_ON_YOLO11N[dtype]))


def _taken_ops(plan, ids, pred):
    """Names of the ops matching pred(args) that took one of `ids`, over the plan's runs."""
    out = set()
    for scale in RUNS:
        eng = engine(scale, plan)
        names = {op.name for op in eng.graph.ops if op.kind == "conv" and pred(op.args)}
        for cid in ids:
            for shape in shapes_of(scale, plan, cid):
                out |= {n for n, t in taken_of(scale, plan, shape, cid).items() if n in names and t[0] == 1}
    return out


def test_every_fused_kernel_ran_somewhere():
    """The fused kernels count apart from the single convs: the streaming FUSE pair kernel, the LDS-DMA fused-epilogue
    GEMM, a Bottleneck / band kernel and every depthwise-fused configuration each ran on at least one fused op."""
    fam = {p: {n: range(f, f + c) for n, f, c in families(p)} for p in ("x3", "x3nodw", "f16")}
    pair1 = lambda a: bool(a.get("pair")) and a["pair"]["k"] == 1
    pair3 = lambda a: bool(a.get("pair")) and a["pair"]["k"] == 3
    assert _taken_ops("x3nodw", fam["x3nodw"]["stream"], pair1), "x3 streaming FUSE"
    assert _taken_ops("f16", fam["f16"]["stream"], pair1), "f16 streaming FUSE"
    assert _taken_ops("x3nodw", fam["x3nodw"]["dma"], pair1), "x3 LDS-DMA FUSE"
    assert _taken_ops("x3nodw", fam["x3nodw"]["bneck"], pair3), "x3 Bottleneck"
    assert _taken_ops("x3nodw", fam["x3nodw"]["bneck_x3"], pair3), "x3-only Bottleneck"
    assert _taken_ops("f16", fam["f16"]["bneck"], pair3), "f16 Bottleneck"
    assert _taken_ops("f16", fam["f16"]["bneck"], pair1), "f16 band kernel (3x3 s2 -> 1x1)"
    isdw = lambda a: bool(a.get("dw"))
    for cid in range(8):  # csrc/ym_conv_dwpw.hip YM_DWPW_CFGS: its own id space 0..7
        assert _taken_ops("x3", [cid], isdw) | _taken_ops("x3dwall", [cid], isdw), f"dwpw {cid}"


# ---------------------------------------------------------------------------------------------- the tuner's path
@pytest.mark.parametrize("plan", ["f16", "x3"])
def test_a_tuned_table_names_kernels_that_run(plan):
    """ym_tune (the strict path of ym_launch_conv: an id that does not apply is refused, not replaced) on yolo11n
    160x224 B=1, one repetition per candidate: every conv entry of the table it writes is -1, an id of the plan's
    catalogue, or a split tag whose halves are; and in a forward on that table no op reports taken == 0 — under strict
    a timed id is its own kernel, so a tuned table never silently falls back.  (The shape already runs every id
    non-strict above, so no kernel meets a shape it has not met.)  f32 is left out: given an `lds` id its plan
    launches the heuristic tile and succeeds even under strict, with taken 0 (a known wart listed in
    csrc/ym_conv_catalog.h), so its tuned table may name one."""
    import time
    from yolomi.lib import Runtime
    eng = engine("n", plan)
    x = batch("160x224").to(DEV)
    B, _, H, W = x.shape
    if (B, H, W) not in eng._tuned:
        eng.run(x, use_graph=False, lanes=1)  # the shape's workspace
    args = Runtime.make_args(use_graph=False, lanes=1)
    dets, counts = eng.outputs(B, args.max_det)
    t0 = time.perf_counter()
    eng.rt.tune(x.data_ptr(), B, H, W, args, dets.data_ptr(), counts.data_ptr(),
                torch.cuda.current_stream(DEV).cuda_stream, reps=1)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    table = eng.rt.get_op_cfg(B, H, W)
    eng.run(x, use_graph=False, lanes=1)
    taken = eng.rt.get_op_cfg_taken(B, H, W)
    ops = eng.graph.ops
    eng.rt.set_op_cfg(B, H, W, [-1] * len(ops))
    eng._tuned.discard((B, H, W))
    n = ncfg(PLANS[plan][0])
    split = sum(1 for c in table if c >= SPLIT_TAG)
    print(f"conv-ops tuned {plan}: ym_tune {dt:.1f} s; {sum(1 for c in table if c >= 0)} ops pinned, {split} split; "
          f"taken 1 on {sum(1 for t in taken if t[0] == 1)} ops, 0 on {sum(1 for t in taken if 0 in t)}")
    assert table is not None and len(table) == len(ops)
    for op, c in zip(ops, table):
        if op.kind != "conv":
            assert c == -1, (op.name, c)
        elif c >= SPLIT_TAG:
            assert op.args.get("pair") and (c - SPLIT_TAG) >> 8 < n and (c - SPLIT_TAG) & 255 < n, (op.name, c)
        else:
            assert -1 <= c < n, (op.name, c)
    assert any(c >= 0 for c in table)
    fell_back = [(op.name, c, t) for op, c, t in zip(ops, table, taken) if 0 in t]
    assert not fell_back, fell_back


# ---------------------------------------------------------------------------------------------- determinism
@pytest.mark.parametrize("plan,cid", [("x3", -1), ("f16", -1), ("f32", -1), ("f16", 17 + 4), ("x3", 17 + 4),
                                      ("f16", 47 + 31), ("x3", 3), ("x3", N_F16)])
def test_second_forward_is_bitwise_equal(plan, cid):
    """The heuristic tiles and one split-K id per family (LDS-DMA 64x64 split 4, the first small-M split-K streaming
    id, the depthwise-fused K split 3 — id 3 on the x3 plan's fused depthwise ops — and the first x3-only LDS-DMA id):
    a second eager forward leaves every plan buffer bit-equal.  (The small-M kernels take no x3 conv.)"""
    eng = engine("n", plan)
    x = batch("96x160").to(DEV)
    B = x.shape[0]
    taken = pinned_forward(eng, x, cid)
    ids = [b.id for b in eng.graph.buffers if b.id != eng.graph.input.id]
    first = [eng.read_buffer(b, B, raw=True) for b in ids]
    eng.run(x, use_graph=False, lanes=1)
    second = [eng.read_buffer(b, B, raw=True) for b in ids]
    eng._tuned.discard((B, 96, 160))
    assert cid < 0 or any(t[0] == 1 for t in taken), "the id ran on no op"
    for b, p, q in zip(ids, first, second):
        assert torch.equal(p, q), eng.graph.buffers[b].name
