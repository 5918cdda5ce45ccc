#!/usr/bin/env python3
"""Measures e_s and e_o of tests/misc_oracle.py on the CPU: over every attention op of yolo11n (all shapes of
tests/misc_oracle.py SHAPES, and the sharpened weight set at SHARP_SHAPES) and yolo11s (96x160, 160x224, 352x416), the
largest |fp32 emulation - float64| of the scores relative to scale * sum |q| |k| and of P . V relative to A_o, per plan;
and the softmax statistics of each case (median row maximum of P, share of P under 2^-24).  The qkv tensors are the fp32
oracle's (a forward hook), rounded as the plan stores them.

    python tools/misc_op_bounds.py            # prints the lines quoted in profiles/misc_op_bounds.txt
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "yolo-infer_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from tests import misc_oracle as MO  # noqa: E402
from yolomi.arch import GraphBuilder  # noqa: E402
from yolomi.synth import synth_weights  # noqa: E402

RUNS = {"n": tuple(MO.SHAPES), "s": ("96x160", "160x224", "352x416")}


def attn_inputs(scale, sd, shape):
    """[(op args, NHWC qkv)] of every attention op of the oracle model on a shape's input."""
    return [(a, qkv) for a, qkv, _ in MO.oracle_taps(scale, sd, MO.batch(shape))["attn"]]


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    plans = ("f16", "x3", "f32")
    worst_s = {p: (0.0, "") for p in plans}
    worst_o = {p: (0.0, "") for p in plans}
    for scale, shapes in RUNS.items():
        sd = synth_weights(scale, "detect", 0)
        sharp = MO.sharpen(sd, GraphBuilder(scale, "detect").ops, MO.SHARP)
        for shape in shapes:
            for tag, w in (("", sd), ("sharp", sharp)):
                if tag and (scale != "n" or shape not in MO.SHARP_SHAPES):
                    continue
                for a, qkv in attn_inputs(scale, w, shape):
                    N = qkv.shape[1] * qkv.shape[2]
                    _, _, info = MO.attn_reference("f32", a, w, qkv)
                    q, k, _ = MO.split_heads(a, qkv)
                    P = torch.softmax((q @ k.transpose(-1, -2)) * a["kd"] ** -0.5, -1)
                    print(f"yolo11{scale} {shape} {tag or 'plain'} N = {N}: median row max of P "
                          f"{float(info['pmax'].median()):.3f}, P < 2^-24: {100 * float((P < 2.0 ** -24).double().mean()):.1f} %")
                    for p in plans:
                        if shape == "1440x1504" and p != "f16":
                            continue
                        e_s, e_o = MO.measure_attn(p, a, qkv)
                        where = f"yolo11{scale} {shape} {tag or 'plain'} N = {N}"
                        if e_s > worst_s[p][0]:
                            worst_s[p] = (e_s, where)
                        if e_o > worst_o[p][0]:
                            worst_o[p] = (e_o, where)
    for p in plans:
        print(f"{p}: e_s = {worst_s[p][0]:.3e} at {worst_s[p][1]}; tol_s = min({MO.MARGIN} x e_s = "
              f"{MO.MARGIN * worst_s[p][0]:.3e}, cap_s(kd 32) = {MO.cap_s(p, 32):.3e})")
        print(f"{p}: e_o = {worst_o[p][0]:.3e} at {worst_o[p][1]}; tol_o = min({MO.MARGIN} x e_o = "
              f"{MO.MARGIN * worst_o[p][0]:.3e}, cap_o(N): {MO.cap_o(p, 15):.3e} at N = 15, {MO.cap_o(p, 529):.3e} at "
              f"529, {MO.cap_o(p, 2115):.3e} at 2115); u_P = {MO.U_P[p]:.3e}; c_out = {MO.C_OUT[p]:.3e}")


if __name__ == "__main__":
    main()
