"""Reference of the classify graph and of its head — test infrastructure, CPU only (tests/test_classify_host.py,
tests/test_gpu_classify.py).

`build_cls` is the yolo11-cls module (yolo11-cls.yaml: the backbone without SPPF, C2PSA as layer 9) assembled from
oracle/yolo11.py's Conv, C3k2 and C2PSA, plus Classify restated from upstream's definition,
`linear(pool(conv(x)).flatten(1))` with a softmax at inference; it runs in fp32 or float64.  `head64` is the float64
head of a GIVEN layer-9 tensor on the fp32 weights yolomi/plan.py packs, with the quantities the kernel bounds are
made of.  k_pool, k_lin and k_sm restate the chain formulas of csrc/ym_classify.hip's header.
"""
import math

import numpy as np
import torch
import torch.nn as nn

from oracle.yolo11 import C2PSA, C3k2, Conv, SCALES, _md
from yolomi.plan import _conv_weights

HIDDEN = 1280


def k_pool(P: int) -> int:
    return 5 + math.ceil(math.ceil(P / 32) / 2) + 1


K_LIN = 20 + 6 + 1


def k_sm(nc: int) -> int:
    return math.ceil(nc / 256) + 6 + 2


class Classify(nn.Module):
    """ultralytics Classify: x(b, c1, h, w) -> (b, nc); the raw Linear outputs here, the caller takes the softmax."""

    def __init__(self, c1, c2):
        super().__init__()
        self.conv = Conv(c1, HIDDEN, 1, 1)
        self.pool = nn.AdaptiveAvgPool2d(1)
        self.linear = nn.Linear(HIDDEN, c2)

    def forward(self, x):
        return self.linear(self.pool(self.conv(x)).flatten(1))


class YOLO11Cls(nn.Module):
    def __init__(self, scale, nc):
        super().__init__()
        depth, width, mc = SCALES[scale]
        ch = lambda c: _md(min(c, mc) * width, 8)  # noqa: E731
        rep = lambda n: max(round(n * depth), 1) if n > 1 else n  # noqa: E731
        k = scale in "mlx"
        self.model = nn.Sequential(
            Conv(3, ch(64), 3, 2), Conv(ch(64), ch(128), 3, 2), C3k2(ch(128), ch(256), rep(2), k, 0.25),
            Conv(ch(256), ch(256), 3, 2), C3k2(ch(256), ch(512), rep(2), k, 0.25), Conv(ch(512), ch(512), 3, 2),
            C3k2(ch(512), ch(512), rep(2), True), Conv(ch(512), ch(1024), 3, 2), C3k2(ch(1024), ch(1024), rep(2), True),
            C2PSA(ch(1024), ch(1024), rep(2)), Classify(ch(1024), nc))

    def forward(self, x):
        """(logits, layer 9's output)."""
        feat = self.model[:10](x)
        return self.model[10](feat), feat


def build_cls(scale, sd, nc, dtype=torch.float32):
    m = YOLO11Cls(scale, nc).eval().requires_grad_(False)
    m.load_state_dict({k: torch.as_tensor(v) for k, v in sd.items()}, strict=True)
    return m.to(dtype)


def head64(feat, sd):
    """Float64 head conv of layer 9's output `feat` (B, H, W, c1; NHWC as Engine.read_buffer returns it), per pixel:
    (ref, A), both (B, P, 1280) — SiLU(w x + bias) of the folded conv and A_p = 1.1 * (sum |w| |x| + |bias|), as
    tests/conv_oracle.py defines A.  The pooled vector is ref.mean(1)."""
    w, b = _conv_weights(dict(wkey="model.10.conv", bn=True), sd)  # (1280, 1, 1, c1) fp32, folded
    w = torch.from_numpy(np.ascontiguousarray(w)).double().reshape(HIDDEN, -1)
    b = torch.from_numpy(b.copy()).double()
    x = feat.double().reshape(feat.shape[0], -1, feat.shape[-1])  # (B, P, c1)
    y = x @ w.T + b
    ref = torch.nn.functional.silu(y)
    A = 1.1 * (x.abs() @ w.abs().T + b.abs())
    return ref, A


def linear64(pooled, sd):
    """(logits, sum |W| |pooled|, |bias|) in float64 from a (B, 1280) pooled vector and the fp32 Linear."""
    W = torch.from_numpy(sd["model.10.linear.weight"].astype(np.float32)).double()
    b = torch.from_numpy(sd["model.10.linear.bias"].astype(np.float32)).double()
    p = pooled.double()
    return p @ W.T + b, p.abs() @ W.abs().T, b.abs()


def cls_input(B, H, W, seed=1234):
    """tests/parity_report.py make_input("uniform"): U[0, 1) images."""
    from yolomi.synth import uniform
    return torch.from_numpy(uniform(seed, B * 3 * H * W).astype(np.float32).reshape(B, 3, H, W))
