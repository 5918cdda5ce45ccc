#!/usr/bin/env python3
"""Measures e[plan] of tests/conv_oracle.py on the CPU: for every dense conv of yolo11n and yolo11s, on the inputs of
tests/test_gpu_conv_ops.py, max |emulation - float64| / A, where the emulation is an fp32 torch conv on operands rounded
as the plan rounds them and A = f * (sum |w| |x| + |bias|).  Each conv's input is the fp32 oracle's (a forward hook).

    python tools/conv_op_bounds.py            # prints the lines quoted in profiles/conv_op_bounds.txt
"""
import os
import sys
from types import SimpleNamespace

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-infer_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

from oracle import yolo11 as Y  # noqa: E402
from tests import conv_oracle as CO  # noqa: E402
from tests.golden.make_golden import make_input  # noqa: E402
from yolomi.synth import synth_weights  # noqa: E402

SHAPES = {"n": [((96, 160), (301, 302, 303)), ((160, 224), (311,))], "s": [((160, 224), (311,))]}


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    worst = {p: (0.0, "") for p in CO.TOL}
    for scale, shapes in SHAPES.items():
        net = Y.build(scale, "detect", synth_weights(scale, "detect", 0), fuse=True)
        seen = {}
        hooks = []
        for name, mod in net.named_modules():
            conv = getattr(mod, "conv", None)
            if isinstance(mod, Y.Conv) and conv.groups == 1:
                hooks.append(mod.register_forward_hook(lambda m, i, o, n=name: seen.__setitem__(n, (m, i[0].detach()))))
            elif isinstance(mod, nn.Conv2d) and mod.groups == 1 and not name.endswith(".conv") and ".dfl" not in name:
                hooks.append(mod.register_forward_hook(lambda m, i, o, n=name: seen.__setitem__(n, (m, i[0].detach()))))
        for (H, Wd), seeds in shapes:
            x = make_input("uniform", seeds, 640)[:, :, :H, :Wd].contiguous()
            seen.clear()
            with torch.no_grad():
                net(x)
            for name, (m, xin) in seen.items():
                conv = m.conv if isinstance(m, Y.Conv) else m
                act = isinstance(m, Y.Conv) and isinstance(m.act, nn.SiLU)
                k, s = conv.kernel_size[0], conv.stride[0]
                a = dict(k=k, s=s, act=act, up0=False, src1=None, shuffle2x2=False, src0=SimpleNamespace(C=xin.shape[1]))
                W = {"w": conv.weight.detach().clone(), "b": conv.bias.detach().clone()}
                xs = xin.permute(0, 2, 3, 1)
                for plan in worst:
                    src = CO.round_act(plan, xs)  # what the plan would have stored
                    ref, _ = CO.forward(a, W, src)
                    d = torch.float64
                    A = torch.nn.functional.conv2d(src.permute(0, 3, 1, 2).to(d).abs(), W["w"].to(d).abs(),
                                                   W["b"].to(d).abs(), stride=s, padding=k // 2).permute(0, 2, 3, 1)
                    A = A * (CO.SILU_SLOPE if act else 1.0)
                    We = {"w": CO.round_weight(plan, W["w"]), "b": W["b"]}
                    got, _ = CO.forward(a, We, src, dt=torch.float32, act=CO.silu32)
                    e = float(((got.double() - ref).abs() / A).max())
                    if e > worst[plan][0]:
                        worst[plan] = (e, f"yolo11{scale} {H}x{Wd} B={len(seeds)} {name} k={k} cin={xin.shape[1]}")
        for h in hooks:
            h.remove()
    for plan, (e, where) in worst.items():
        cap = CO.tol_cap(plan, 4608)
        print(f"{plan}: e = {e:.3e} at {where}; tol = {CO.MARGIN} x e = {CO.MARGIN * e:.3e} "
              f"(cap at K = 4608: {cap:.3e}); c_out = {CO.C_OUT[plan]:.3e}")


if __name__ == "__main__":
    main()
