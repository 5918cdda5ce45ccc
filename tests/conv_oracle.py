"""Float64 reference of ONE conv op of a plan, computed from the op's own stored inputs, with a per-element error
bound — test infrastructure, CPU only (tests/test_conv_oracle_host.py checks it, tests/test_gpu_conv_ops.py uses it).

The op is a plan record of yolomi/arch.py (`Op.args`): a 1x1 or 3x3 conv at stride 1 or 2, pad k // 2, over `src0`
(nearest-upsampled 2x when `up0`) concatenated with `src1`, SiLU or none, then `res` added; the merged `wkeys` GEMM; a
`convT` / `shuffle2x2` pixel-shuffled GEMM; a fused `pair` (a second conv on the unstored intermediate, and its
residual); a fused `dw` (depthwise 3x3 + SiLU in front of the 1x1).  The fp32 weights are the ones the planner packs:
yolomi/plan.py `_conv_weights`, `_dw_weights`, `_pad_channels` (pose heads), nothing restated here.

Bound.  `reference()` returns (ref, E): the GPU value of every output element is held to |got - ref| <= E,

    E = tol[plan] * A + c_out[plan] * |ref|,      A = f * (sum |w| |x| + |bias|) + |res|,

A being the same conv with absolute weights on the absolute input, in float64, and f = 1.1 (the largest slope of SiLU)
for an activated op, else 1.  E is per element and scaled by that element's own operands: a small border pixel is
judged as strictly as the tensor's maximum.  A fused pair carries the first conv's bound through the second,

    E2 = f2 * conv(|w2|, 1.1 * E1 + r_mid * |mid|) + tol * A2 + c_out * |ref2|,     E1 = tol * A1,

r_mid the rounding the kernel applies to the unstored intermediate: 2^-11 (fp16) in the f16 plan, 2^-23 (the hi + lo
split) in x3.  A fused depthwise does the same with the depthwise op in front: its 9 fmaf taps and bias in fp32 are
worst case 11 * 2^-24 * A_dw, times 1.1, plus r_mid * |h| for the split of h.

c_out (the epilogue's own error relative to the stored value), from csrc/ym_common.h:
  * f16: one fp16 rounding (2^-11) plus ym_silu_fast's exp2 and rcp (1 ulp of fp32 each): 2^-10.
  * f32: ym_silu = x / (1 + expf(-x)): expf 1 ulp, the add 0.5, the division 1, the residual add 0.5, the bias add 0.5:
    3.5 ulp -> 4 * 2^-24.  (An error of exp(-x) reaches 1 / (1 + exp(-x)) with a factor exp(-x) / (1 + exp(-x)) <= 1.)
  * x3: ym_silu_x3: exp2 1 ulp, the add 0.5, rcp 1 ulp refined by a Newton step of two fmaf (2 ulp together, the
    comment in the header says the same), x * r 0.5, the residual add 0.5, the exp2 argument's rounding
    (|x| * 2^-24 relative in exp(-x), times x * sigmoid(-x) <= 0.28 for x > 0) 0.3: 4.8 ulp -> 5 * 2^-24, plus 2^-23 for
    the stored hi + lo split: 7 * 2^-24.  (For x < 0 the argument's rounding is at most 0.28 * 2^-24 * |x| <= 0.28 *
    2^-24 * A absolute, under one hundredth of tol[x3] * A: carried by tol's margin.)

tol (the accumulation's error relative to A) is measured against a CPU emulation of the plan's operand representation,
not against the kernels: `emulate()` below is an fp32 torch conv on operands rounded as the plan rounds them (fp16 for
f16; the hi + lo split with the planner's power-of-two weight scale for x3; untouched for f32).  e = max |emulation -
float64| / A over every conv op of yolo11n and yolo11s on the inputs of tests/test_gpu_conv_ops.py; tol = MARGIN * the
plan's largest e, and per op never more than the worst case `tol_cap`: (terms + 2) * 2^-24 plus the representation
error (f16: two fp16 roundings per product, 2^-10; x3: 3 * 2^-22; f32: none).  The measured figures are in
profiles/conv_op_bounds.txt.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

from yolomi.plan import _conv_weights, _dw_weights, _pad_channels, x3_weight_exp

SILU_SLOPE = 1.1
C_OUT = {"f16": 2.0 ** -10, "f32": 4 * 2.0 ** -24, "x3": 7 * 2.0 ** -24}
R_MID = {"f16": 2.0 ** -11, "x3": 2.0 ** -23, "f32": 0.0}
REPR = {"f16": 2.0 ** -10, "x3": 3 * 2.0 ** -22, "f32": 0.0}
# e: the largest |emulation - float64| / A measured per plan (profiles/conv_op_bounds.txt says where); tol = MARGIN * e
E_MEASURED = {"f16": 2.683e-4, "x3": 1.003e-6, "f32": 9.223e-7}
MARGIN = 8
TOL = {p: MARGIN * e for p, e in E_MEASURED.items()}


def tol_cap(plan: str, terms: int) -> float:
    """Worst case of a `terms`-long fp32 sum (+ bias, + scale) on the plan's operands, relative to A."""
    return (terms + 2) * 2.0 ** -24 + REPR[plan]


def split_repr(t: torch.Tensor) -> torch.Tensor:
    """tools/x3_emulate.py's hi + lo (its activation branch), loaded lazily: the tool's imports are the oracle's."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    tools = os.path.join(root, "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import x3_emulate
    x3_emulate.SCALE_W["on"] = False
    return x3_emulate.split_repr(t)


def round_act(plan: str, t: torch.Tensor) -> torch.Tensor:
    t = t.float()
    return t.half().float() if plan == "f16" else (split_repr(t) if plan == "x3" else t)


def round_weight(plan: str, w: torch.Tensor) -> torch.Tensor:
    """x3: the split of w * 2^s, s the planner's exponent (yolomi/plan.py x3_weight_exp), scaled back (exact)."""
    w = w.float()
    if plan == "f16":
        return w.half().float()
    if plan == "x3":
        s = 2.0 ** x3_weight_exp(w.numpy())
        return split_repr(w * s) / s
    return w


def op_weights(a: dict, sd, pose: bool = False) -> dict:
    """The fp32 arrays the planner packs for this op, as torch tensors in conv2d layout (N, cin, k, k)."""
    w, b = _conv_weights(a, sd)
    if pose:
        w, b = _pad_channels(w, b, a["c2"], a["c1"])
    out = {"w": torch.from_numpy(np.ascontiguousarray(w)).permute(0, 3, 1, 2).contiguous(), "b": torch.from_numpy(b.copy())}
    if a.get("pair"):
        p = a["pair"]
        w2, b2 = _conv_weights(p, sd)
        if pose:
            w2, b2 = _pad_channels(w2, b2, p["c2"], p["c1"])
        out["w2"] = torch.from_numpy(np.ascontiguousarray(w2)).permute(0, 3, 1, 2).contiguous()
        out["b2"] = torch.from_numpy(b2.copy())
    if a.get("dw"):
        w9, bd = _dw_weights(a["dw"]["wkey"], sd)  # [9][C]
        C = w9.shape[1]
        out["wd"] = torch.from_numpy(np.ascontiguousarray(w9.T)).reshape(C, 1, 3, 3)
        out["bd"] = torch.from_numpy(np.asarray(bd, np.float32).copy())
    return out


def _nchw(t):
    return None if t is None else t.permute(0, 3, 1, 2)


def _gather(a, src0, src1, dt):
    x = _nchw(src0).to(dt)
    if src0.shape[-1] < a["src0"].C:
        raise ValueError("src0 narrower than the op's view")
    if a["up0"]:
        x = x.repeat_interleave(2, 2).repeat_interleave(2, 3)  # nearest 2x
    if a["src1"] is not None:
        x = torch.cat([x, _nchw(src1).to(dt)], 1)
    return x


def _shuffle(a, y):
    """GEMM column n = (dy * 2 + dx) * cout + o of pixel (y, x) -> channel o of pixel (2y + dy, 2x + dx)."""
    if not a["shuffle2x2"]:
        return y
    B, N, H, W = y.shape
    return y.reshape(B, 2, 2, N // 4, H, W).permute(0, 3, 4, 1, 5, 2).reshape(B, N // 4, 2 * H, 2 * W)


def forward(a: dict, W: dict, src0, src1=None, res=None, dt=torch.float64, rnd_mid=None, act=F.silu, mid_act=None):
    """The op in dtype `dt` on NHWC inputs (the views' channels); returns NHWC (out, mid): mid the unstored
    intermediate of a pair (after rnd_mid), else None.  mid_act: the first conv's activation of a pair (default act)."""
    x = _gather(a, src0, src1, dt)
    if a.get("dw"):
        x = F.conv2d(x, W["wd"].to(dt), W["bd"].to(dt), padding=1, groups=x.shape[1])
        x = act(x) if a["dw"]["act"] else x
        if rnd_mid is not None:
            x = rnd_mid(x)
    y = F.conv2d(x, W["w"].to(dt), W["b"].to(dt), stride=a["s"], padding=a["k"] // 2)
    pair = a.get("pair")
    if a["act"]:
        y = (mid_act or act)(y) if pair else act(y)
    mid = None
    if pair:
        mid = rnd_mid(y) if rnd_mid is not None else y
        y = F.conv2d(mid, W["w2"].to(dt), W["b2"].to(dt), padding=pair["k"] // 2)
        if pair["act"]:
            y = act(y)
    y = _shuffle(a, y)
    if res is not None:
        y = y + _nchw(res).to(dt)
    return y.permute(0, 2, 3, 1), (None if mid is None else mid.permute(0, 2, 3, 1))


def reference(plan: str, a: dict, sd, src0, src1=None, res=None, pose: bool = False, tol=None):
    """(ref, E, A): the float64 output of the op (NHWC, the dst view's channels), the bound E the GPU value is held to,
    and A (module docstring).  Inputs: the op's views as read back (NHWC float tensors, the view's channels only)."""
    W = op_weights(a, sd, pose)
    d = torch.float64
    ref, mid = forward(a, W, src0, src1, res, d)
    tol = TOL[plan] if tol is None else tol
    ax = _gather(a, src0, src1, d).abs()
    e_in = None  # the error bound of the 1x1's operand when a depthwise is fused in front of it
    if a.get("dw"):
        x = _gather(a, src0, src1, d)
        a_dw = F.conv2d(ax, W["wd"].to(d).abs(), W["bd"].to(d).abs(), padding=1, groups=ax.shape[1])
        h = F.conv2d(x, W["wd"].to(d), W["bd"].to(d), padding=1, groups=x.shape[1])
        h = F.silu(h) if a["dw"]["act"] else h
        e_in = SILU_SLOPE * 11 * 2.0 ** -24 * a_dw + R_MID[plan] * h.abs()
        ax = h.abs()
    k, s = a["k"], a["s"]
    wabs = W["w"].to(d).abs()
    terms1 = k * k * W["w"].shape[1]
    t1 = min(tol, tol_cap(plan, terms1))
    f1 = SILU_SLOPE if a["act"] else 1.0
    A1 = F.conv2d(ax, wabs, W["b"].to(d).abs(), stride=s, padding=k // 2)
    E1 = t1 * A1
    if e_in is not None:
        E1 = E1 + F.conv2d(e_in, wabs, None, stride=s, padding=k // 2)
    pair = a.get("pair")
    if pair:
        m = mid.permute(0, 3, 1, 2)
        w2abs = W["w2"].to(d).abs()
        k2 = pair["k"]
        f2 = SILU_SLOPE if pair["act"] else 1.0
        t2 = min(tol, tol_cap(plan, k2 * k2 * W["w2"].shape[1]))
        A = f2 * F.conv2d(m.abs(), w2abs, W["b2"].to(d).abs(), padding=k2 // 2)
        E = f2 * F.conv2d(f1 * E1 + R_MID[plan] * m.abs(), w2abs, None, padding=k2 // 2) + t2 * A
        tr = t2
    else:
        A = f1 * A1
        E = f1 * E1
        tr = t1
    A, E = _shuffle(a, A), _shuffle(a, E)
    if res is not None:
        r = _nchw(res).to(d).abs()
        A = A + r
        E = E + tr * r
    A, E = A.permute(0, 2, 3, 1), E.permute(0, 2, 3, 1)
    return ref, E + C_OUT[plan] * ref.abs(), A


def silu32(x):
    return x / (1.0 + torch.exp(-x))


def emulate(plan: str, a: dict, sd, src0, src1=None, res=None, pose: bool = False, W=None, **kw):
    """The plan's operand representation on the CPU: an fp32 torch conv on operands rounded as the plan rounds them
    (stored inputs are already representable, so rounding them again changes nothing), fp32 SiLU, the unstored
    intermediate of a pair / a fused depthwise rounded like a stored tensor.  W: weights to use instead (tests)."""
    if W is None:
        W = {k: (round_weight(plan, v) if k in ("w", "w2") else v.float()) for k, v in op_weights(a, sd, pose).items()}
    r = lambda t: None if t is None else round_act(plan, t)
    out, _ = forward(a, W, r(src0), r(src1), r(res), torch.float32, rnd_mid=lambda t: round_act(plan, t), act=silu32, **kw)
    return out


def worst(got: torch.Tensor, ref: torch.Tensor, E: torch.Tensor):
    """(max err / E, its (b, y, x, c), err, E there) of an NHWC result."""
    err = (got.double() - ref).abs()
    ratio = err / E.clamp_min(1e-300)
    i = int(ratio.argmax())
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(ratio.shape)))
    return float(ratio.reshape(-1)[i]), idx, float(err.reshape(-1)[i]), float(E.reshape(-1)[i])
