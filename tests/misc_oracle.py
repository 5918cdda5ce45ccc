"""Float64 references of the three compute ops that are not convs (csrc/ym_attn.hip, ym_sppf.hip, ym_dwconv.hip) —
`attn` (C2PSA attention), `sppf` (the three max pools) and `dwconv` (depthwise 3x3) — each computed from the op's own
stored input, with a per-element error bound: test infrastructure, CPU only (tests/test_misc_oracle_host.py checks it,
tests/test_gpu_misc_ops.py uses it).  The style is tests/conv_oracle.py's: every constant below is derived here or
measured against a CPU emulation of the plan's operand representation (tools/misc_op_bounds.py, figures in
profiles/misc_op_bounds.txt), never against the kernels.

attn.  The stored qkv view holds, per head h, the channels [q kd | k kd | v hd] at h * (2 kd + hd); the output channel
of head h, dim d is h * hd + d.  With P = softmax_j(scale * q . k_j), scale = kd^-1/2,

    ref = sum_j P_j v_j + pe(v),          pe the depthwise 3x3 (zero padded) of yolomi/plan.py `_dw_weights`,

    E = (e^{2 delta} - 1 + tol_o) * A_o + u_P * N * max_j |v_j| + 11 * 2^-24 * A_pe + c_out * |ref|
    delta = tol_s * scale * max_j sum_c |q_c| |k_jc|      A_o = sum_j P_j |v_j|      A_pe = sum |w| |v| + |b|

  * delta bounds the error of every score of the query's row, so each exp(s_j - m) and their sum are off by a factor
    within e^{+-delta}, each P_j by one within e^{+-2 delta}: (e^{2 delta} - 1) * A_o.
  * tol_s, relative to scale * sum |q_c| |k_jc|: worst case a kd-term fp32 sum and three roundings (the scale, the
    max subtraction, the exponent's argument), (kd + 3) * 2^-24, plus the representation: none for f16 and f32 (the
    stored fp16 / fp32 operands are exact and so are their products in fp32), 2^-22 for x3 (hi * hi + lo * hi + hi * lo:
    the lo * lo product, at most 2^-11 * 2^-11 of the term, is dropped).  That is `cap_s`.
  * tol_o, relative to A_o: an N-term fp32 sum for P . V and another for the softmax denominator, the exponential
    (1 ulp), the reciprocal and its product: 2 (N + 4) * 2^-24, plus the rounding of P in front of the MFMA: 2^-11
    for f16 (one fp16 rounding), 2^-21 for x3 (P = hi + lo leaves 2^-22, the dropped lo * lo another 2^-22), none for
    f32 (the scalar kernel keeps P in fp32).  That is `cap_o`.
  * u_P, the absolute rounding of one stored probability: f16 rounds P (<= 1) to fp16, whose subnormals (below 2^-14)
    are spaced 2^-24: 2^-25.  x3: hi = fp16(P) leaves at most 2^-25 below 2^-14, and lo = fp16(P - hi) of a residual
    under 2^-14 is a subnormal again: max(2^-22 * P, 2^-25), the relative part is in cap_o: 2^-25.  (The flash kernel
    rounds exp(s - running max) <= 1, later scaled by factors <= 1 and divided by a sum >= 1: no more.)  f32: an fp32
    exponential below 2^-126 may be flushed to zero: 2^-126.
  * pe: 9 fmaf and the bias in fp32, and in x3 the fp32 sum hi + lo of a tap: 11 * 2^-24 * A_pe, as conv_oracle's
    fused depthwise.
  * c_out: the fp32 add o + pe (2^-24 of the result) and the store: f16 one fp16 rounding, 2^-11 + 2^-23 together;
    x3 the hi + lo split, 2^-23: 3 * 2^-24; f32 2^-24.  (conv_oracle's C_OUT without the SiLU terms.)
  tol_s = min(MARGIN * e_s, cap_s) and tol_o = min(MARGIN * e_o, cap_o), MARGIN conv_oracle's 8; e_s and e_o are the
  largest |emulation - float64| relative to scale * sum |q| |k| and to A_o, measured by tools/misc_op_bounds.py over the
  shapes and both weight sets of tests/test_gpu_misc_ops.py, the emulation being fp32 torch on operands rounded as the
  plan rounds them (`emulate_attn`: fp16 q / k / v and P rounded to fp16 in front of P . V for f16; the hi + lo splits
  with the lo * lo products dropped for x3; nothing for f32).

dwconv.  ref = float64 conv (+ SiLU); E = f * 11 * 2^-24 * A + conv_oracle.C_OUT[plan] * |ref|, A = sum |w| |x| + |b|,
f = 1.1 (SiLU's largest slope) for an activated op: 9 fmaf, the bias and (x3) the hi + lo sum of a tap in fp32, then
conv_oracle's epilogue.  Derived; nothing is measured.

sppf.  ref = max_pool2d with kernels 5 / 9 / 13, stride 1, -inf padding, in float64 on the stored cat[0:C]; the
three written slices equal it exactly as values (max pooling rounds nothing).

Mutations (`MUTATIONS`): references that are deliberately wrong the way a kernel could be; `applies` says whether a
mutation changes anything at a shape.  The tests demand that each breaks E somewhere.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests import conv_oracle as CO
from yolomi.plan import _dw_weights

MARGIN = CO.MARGIN
D = torch.float64
U = 2.0 ** -24
REPR_S = {"f16": 0.0, "x3": 2.0 ** -22, "f32": 0.0}
REPR_P = {"f16": 2.0 ** -11, "x3": 2.0 ** -21, "f32": 0.0}
U_P = {"f16": 2.0 ** -25, "x3": 2.0 ** -25, "f32": 2.0 ** -126}
C_OUT = {"f16": 2.0 ** -11 + 2.0 ** -23, "x3": 3 * U, "f32": U}
PE_TERMS = 11
# e_s, e_o: the largest |emulation - float64| measured per plan (profiles/misc_op_bounds.txt says where)
E_S = {"f16": 1.276e-07, "x3": 1.650e-07, "f32": 1.446e-07}
E_O = {"f16": 3.750e-04, "x3": 1.522e-06, "f32": 1.530e-06}


def cap_s(plan: str, kd: int) -> float:
    return (kd + 3) * U + REPR_S[plan]


def cap_o(plan: str, N: int) -> float:
    return 2 * (N + 4) * U + REPR_P[plan]


def tols(plan: str, kd: int, N: int):
    return min(MARGIN * E_S[plan], cap_s(plan, kd)), min(MARGIN * E_O[plan], cap_o(plan, N))


# ---------------------------------------------------------------------------------------------- attention
def split_heads(a: dict, qkv: torch.Tensor, dt=D):
    """NHWC qkv (B, H, W, nh * (2 kd + hd)) -> q, k (B, nh, N, kd) and v (B, nh, N, hd) in `dt`."""
    B, H, W, _ = qkv.shape
    nh, kd, hd = a["nh"], a["kd"], a["hd"]
    t = qkv.to(dt).reshape(B, H * W, nh, 2 * kd + hd).permute(0, 2, 1, 3)
    return t[..., :kd], t[..., kd:2 * kd], t[..., 2 * kd:]


def pe_weights(a: dict, sd):
    w9, b = _dw_weights(a["wkey"], sd)  # [9][C], [C]
    return torch.from_numpy(np.ascontiguousarray(w9)), torch.from_numpy(np.asarray(b, np.float32).copy())


def pe_taps(v: torch.Tensor, w9: torch.Tensor, b: torch.Tensor, H: int, W: int, no_left_test: bool = False,
            absolute: bool = False):
    """The positional depthwise 3x3 on v (B, N, C) in v's dtype, tap by tap in (ky, kx) order as the kernels take them.
    no_left_test (a mutation): the x - 1 >= 0 test is missing, so at x = 0 the tap reads flat pixel n - 1 + (ky - 1) W,
    the previous row's last pixel, when that lies inside the tensor."""
    B, N, C = v.shape
    n = torch.arange(N)
    y, x = n // W, n % W
    out = (b.abs() if absolute else b).to(v.dtype).expand(B, N, C).clone()
    for t in range(9):
        iy, ix = y + t // 3 - 1, x + t % 3 - 1
        flat = iy * W + ix
        ok = (iy >= 0) & (iy < H) & (ix < W) & ((flat >= 0) if no_left_test else (ix >= 0))
        tap = v[:, flat.clamp(0, N - 1)] * ok.to(v.dtype)[None, :, None]
        wt = w9[t].to(v.dtype)
        out = out + (tap.abs() * wt.abs() if absolute else tap * wt)
    return out


def _merge(o):  # (B, nh, N, hd) -> (B, N, nh * hd)
    B, nh, N, hd = o.shape
    return o.permute(0, 2, 1, 3).reshape(B, N, nh * hd)


def attn_reference(plan: str, a: dict, sd, qkv: torch.Tensor, mutation: str = None, want_bound: bool = True):
    """(ref, E, info) of the attn op on its stored NHWC qkv view: the float64 output (B, H, W, C), the bound the GPU
    value is held to, and info = dict(A_o, P row maxima).  mutation: a key of MUTATIONS (then E is None)."""
    B, H, W, _ = qkv.shape
    N, nh, kd, hd = H * W, a["nh"], a["kd"], a["hd"]
    q, k, v = split_heads(a, qkv)
    w9, b = pe_weights(a, sd)
    scale = kd ** -0.5
    m = MUTATIONS[mutation] if mutation else {}
    s = (q @ k.transpose(-1, -2)) * (scale * m.get("scale", 1.0))
    keep = m["keys"](N) if "keys" in m else N
    P = torch.softmax(s[..., :keep], -1)
    vv = v[:, :, :keep]
    if m.get("swap_v"):
        vv = vv.clone()
        vv[:, :, [0, 1]] = vv[:, :, [1, 0]]
    o = P @ vv
    if m.get("roll_heads"):
        o = o.roll(1, 1)
    pe = pe_taps(_merge(v), w9, b, H, W, no_left_test=bool(m.get("no_left_test")))
    if m.get("roll_pe"):
        pe = pe.reshape(B, N, nh, hd).roll(1, 2).reshape(B, N, nh * hd)
    ref = (_merge(o) + pe).reshape(B, H, W, nh * hd)
    if mutation or not want_bound:
        return ref, None, None
    tol_s, tol_o = tols(plan, kd, N)
    delta = tol_s * scale * (q.abs() @ k.abs().transpose(-1, -2)).amax(-1, keepdim=True)  # (B, nh, N, 1)
    A_o = P @ v.abs()
    vmax = v.abs().amax(2, keepdim=True)  # (B, nh, 1, hd)
    A_pe = pe_taps(_merge(v), w9, b, H, W, absolute=True)
    E = _merge((torch.expm1(2 * delta) + tol_o) * A_o + U_P[plan] * N * vmax.expand_as(A_o)) + PE_TERMS * U * A_pe
    E = E.reshape(B, H, W, nh * hd) + C_OUT[plan] * ref.abs()
    return ref, E, {"A_o": _merge(A_o).reshape(B, H, W, nh * hd), "pmax": P.amax(-1)}


def _hl(t):
    hi = t.half().float()
    return hi, (t - hi).half().float()


def _mm3(plan, x, y):
    """x @ y in fp32 on the plan's operands: x3 as hi * hi + lo * hi + hi * lo."""
    if plan != "x3":
        return x @ y
    xh, xl = _hl(x)
    yh, yl = _hl(y)
    return xl @ yh + xh @ yl + xh @ yh


def emulate_attn(plan: str, a: dict, sd, qkv: torch.Tensor, P64: torch.Tensor = None, parts: bool = False,
                 p_scale: float = 1.0):
    """The plan's operand representation on the CPU, in fp32 torch (module docstring).  P64: probabilities to use in
    place of the emulation's own softmax (the measurement of e_o isolates P . V with the float64 ones).  parts: return
    (scores, P . V) as (B, nh, N, .) instead of the stored output.  p_scale: a power of two P is multiplied by in front
    of its rounding and P . V divided by behind it (exact): 2^14 keeps every fp16 of P out of the subnormals, leaving
    the relative part of P's rounding alone (the absolute part is the u_P term's)."""
    B, H, W, _ = qkv.shape
    N, nh, kd, hd = H * W, a["nh"], a["kd"], a["hd"]
    q, k, v = (CO.round_act(plan, t) for t in split_heads(a, qkv, torch.float32))
    s = _mm3(plan, q, k.transpose(-1, -2)) * np.float32(kd ** -0.5)
    P = torch.softmax(s, -1) if P64 is None else P64.float()
    P = P * np.float32(p_scale)
    if plan == "f16":
        P = P.half().float()
    o = _mm3(plan, P, v) / np.float32(p_scale)
    if parts:
        return s, o
    w9, b = pe_weights(a, sd)
    out = _merge(o) + pe_taps(_merge(v), w9, b, H, W)
    return CO.round_act(plan, out).reshape(B, H, W, nh * hd)


def measure_attn(plan: str, a: dict, qkv: torch.Tensor):
    """(e_s, e_o) of one stored qkv view: max |fp32 emulation - float64| of the scores relative to scale * sum |q| |k|,
    and of P . V (on the float64 P, rounded as the plan rounds it but for the subnormals: p_scale) relative to A_o."""
    q, k, v = split_heads(a, CO.round_act(plan, qkv))
    scale = a["kd"] ** -0.5
    s64 = (q @ k.transpose(-1, -2)) * scale
    P = torch.softmax(s64, -1)
    s32, o32 = emulate_attn(plan, a, None, qkv, P64=P, parts=True, p_scale=2.0 ** 14)
    e_s = ((s32.double() - s64).abs() / (scale * (q.abs() @ k.abs().transpose(-1, -2))).clamp_min(1e-300)).max()
    e_o = ((o32.double() - P @ v).abs() / (P @ v.abs()).clamp_min(1e-300)).max()
    return float(e_s), float(e_o)


# Deliberately wrong references.  keys: the number of leading keys the softmax and P . V still see.
MUTATIONS = {
    "last_key_dropped": {"keys": lambda N: N - 1},
    "last_partial_tile_dropped": {"keys": lambda N: N - N % 16},
    "last_block_dropped": {"keys": lambda N: 256 * ((N - 1) // 256)},
    "v_rows_0_1_swapped": {"swap_v": True},
    "heads_swapped": {"roll_heads": True},
    "scale_sqrt2": {"scale": math.sqrt(2.0)},
    "pe_no_left_border_test": {"no_left_test": True},
    "pe_of_the_wrong_head": {"roll_pe": True},
}
SINGLE_KEY = ("last_key_dropped", "v_rows_0_1_swapped")


def applies(mutation: str, H: int, W: int, nh: int = 2) -> bool:
    """Whether a mutation changes the op at an H x W map: a partial 16-key tile behind at least one full one, more than
    one 256-key block, a second row for the wrapped tap to read (on a one-row map pixel n - 1 of x = 0 lies in front
    of the tensor), more than one key / head."""
    N = H * W
    return {"last_key_dropped": N > 1, "last_partial_tile_dropped": N > 16 and N % 16 != 0,
            "last_block_dropped": N > 256, "v_rows_0_1_swapped": N > 1, "heads_swapped": nh > 1, "scale_sqrt2": N > 1,
            "pe_no_left_border_test": W > 1 and H > 1, "pe_of_the_wrong_head": nh > 1}[mutation]


def sharpen(sd: dict, graph_ops, factor: float = 8.0) -> dict:
    """A copy of the state dict with the query channels of every attn.qkv conv scaled by `factor` (its BN weight and
    bias on those channels): scores `factor` times as large, so the softmax has a few dominant keys and entries that
    underflow.  graph_ops: the plan's op records (their attn entries name the convs and the head layout)."""
    out = dict(sd)
    for op in graph_ops:
        if op.kind != "attn":
            continue
        a = op.args
        key = a["wkey"][:-len(".pe")] + ".qkv"
        per = 2 * a["kd"] + a["hd"]
        for suf in (".bn.weight", ".bn.bias"):
            t = np.array(sd[key + suf], copy=True)
            for h in range(a["nh"]):
                t[h * per:h * per + a["kd"]] *= factor
            out[key + suf] = t
    return out


# ---------------------------------------------------------------------------------------------- depthwise
def dw_reference(plan: str, a: dict, sd, src: torch.Tensor):
    """(ref, E, A) of a dwconv op on its stored NHWC input (module docstring)."""
    w9, b = _dw_weights(a["wkey"], sd)
    C = w9.shape[1]
    w = torch.from_numpy(np.ascontiguousarray(w9.T)).reshape(C, 1, 3, 3).to(D)
    b = torch.from_numpy(np.asarray(b, np.float32).copy()).to(D)
    x = src.to(D).permute(0, 3, 1, 2)
    ref = F.conv2d(x, w, b, padding=1, groups=C)
    A = F.conv2d(x.abs(), w.abs(), b.abs(), padding=1, groups=C)
    f = CO.SILU_SLOPE if a["act"] else 1.0
    if a["act"]:
        ref = F.silu(ref)
    ref, A = ref.permute(0, 2, 3, 1), A.permute(0, 2, 3, 1)
    return ref, f * PE_TERMS * U * A + CO.C_OUT[plan] * ref.abs(), A


def emulate_dw(plan: str, a: dict, sd, src: torch.Tensor):
    w9, b = _dw_weights(a["wkey"], sd)
    C = w9.shape[1]
    w = torch.from_numpy(np.ascontiguousarray(w9.T)).reshape(C, 1, 3, 3)
    y = F.conv2d(CO.round_act(plan, src).permute(0, 3, 1, 2), w, torch.from_numpy(np.asarray(b, np.float32).copy()),
                 padding=1, groups=C)
    return CO.round_act(plan, CO.silu32(y) if a["act"] else y).permute(0, 2, 3, 1)


# ---------------------------------------------------------------------------------------------- SPPF
def sppf_reference(src: torch.Tensor) -> torch.Tensor:
    """cat[C:4C] of an sppf op from its stored cat[0:C] (NHWC): the 5, 9 and 13 wide max pools, float64."""
    x = src.to(D).permute(0, 3, 1, 2)
    return torch.cat([F.max_pool2d(x, k, 1, k // 2) for k in (5, 9, 13)], 1).permute(0, 2, 3, 1)


def worst(got, ref, E):
    return CO.worst(got, ref, E)


# ---------------------------------------------------------------------------------------------- the tests' inputs
# name -> (H, W, seeds): the shapes of tests/test_gpu_misc_ops.py (its docstring says what each reaches); the e_s / e_o
# above are measured on these.  Larger batches repeat the images of a shape (`batch(name, B)`).
SHAPES = {"96x160": (96, 160, (401, 402, 403)), "160x224": (160, 224, (411,)), "256x512": (256, 512, (412,)),
          "352x416": (352, 416, (413,)), "512x512": (512, 512, (414,)), "480x672": (480, 672, (415,)),
          "416x1024": (416, 1024, (416,)), "640x800": (640, 800, (417,)), "512x1024": (512, 1024, (418,)),
          "736x736": (736, 736, (419,)), "1056x1056": (1056, 1056, (420,)), "1440x1504": (1440, 1504, (421,)),
          "32x416": (32, 416, (422,))}
SHARP_SHAPES = ("96x160", "352x416", "736x736", "1056x1056")  # N = 15, 143, 529, 1089
SHARP = 8.0


def batch(name: str, B: int = None) -> torch.Tensor:
    """The NCHW input of a shape: make_input("uniform", seeds, S) cropped to H x W, its images repeated up to B."""
    from tests.golden.make_golden import make_input
    H, W, seeds = SHAPES[name]
    x = make_input("uniform", seeds, max(640, H, W))[:, :, :H, :W].contiguous()
    if B is not None and B != len(seeds):
        x = x.repeat((B + len(seeds) - 1) // len(seeds), 1, 1, 1)[:B].contiguous()
    return x


def oracle_taps(scale: str, sd, x: torch.Tensor, dt=torch.float32):
    """The oracle model's own tensors around its attention, SPPF and depthwise modules on input x, in dtype dt (NHWC):
    {"attn": [(op args, qkv, Attention's sum in front of proj)], "sppf": [(cv1's output, cv2's input)],
     "dw": [(op args, input, output)]}.  The attention args are the plan's records (yolomi/arch.py)."""
    from oracle import yolo11 as Y
    from yolomi.arch import GraphBuilder
    net = Y.build(scale, "detect", sd, fuse=True).to(dt)
    ops = {op.name: op.args for op in GraphBuilder(scale, "detect").ops if op.kind == "attn"}
    nhwc = lambda t: t.detach().permute(0, 2, 3, 1).contiguous()
    seen, hooks, out = {}, [], {"attn": [], "sppf": [], "dw": []}
    for name, mod in net.named_modules():
        if isinstance(mod, Y.Attention):
            hooks.append(mod.qkv.register_forward_hook(lambda m, i, o, n=name: seen.__setitem__(n + "/qkv", nhwc(o))))
            hooks.append(mod.proj.register_forward_pre_hook(lambda m, i, n=name: seen.__setitem__(n + "/sum", nhwc(i[0]))))
        elif isinstance(mod, Y.SPPF):
            hooks.append(mod.cv1.register_forward_hook(lambda m, i, o: seen.__setitem__("sppf/src", nhwc(o))))
            hooks.append(mod.cv2.register_forward_pre_hook(lambda m, i: seen.__setitem__("sppf/cat", nhwc(i[0]))))
        elif isinstance(mod, Y.DWConv):
            hooks.append(mod.register_forward_hook(
                lambda m, i, o, n=name: out["dw"].append((dict(C=o.shape[1], act=True, wkey=n), nhwc(i[0]), nhwc(o)))))
    with torch.no_grad():
        net(x.to(dt))
    for h in hooks:
        h.remove()
    assert {k.split("/")[0] for k in seen if k.startswith("model")} == set(ops), (sorted(seen), sorted(ops))
    out["attn"] = [(ops[n], seen[n + "/qkv"], seen[n + "/sum"]) for n in ops]
    out["sppf"] = [(seen["sppf/src"], seen["sppf/cat"])]
    return out
