"""Host side of the NV12 letterbox (yolomi.preprocess.NV12Frames / letterbox_nv12): the descriptor table, the
coefficient table and the refusals, with a runtime that records its one call (CPU tensors stand in for device planes)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from yolomi.preprocess import NV12_DESC, NV12Frames, letterbox_geometry, letterbox_nv12, nv12_coefficients

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class Recorder:
    def __init__(self):
        self.calls = []

    def letterbox_nv12(self, desc_ptr, host_desc_ptr, B, coef, dst_ptr, Hn, Wn, stream):
        host = np.frombuffer(ctypes.string_at(host_desc_ptr, B * NV12_DESC.itemsize), dtype=NV12_DESC)
        dev = np.frombuffer(ctypes.string_at(desc_ptr, B * NV12_DESC.itemsize), dtype=NV12_DESC)
        self.calls.append((host, dev, B, tuple(coef), dst_ptr, Hn, Wn, stream))


def planes(h, w, y_pitch=None, uv_pitch=None):
    y = torch.zeros((h, y_pitch or w), dtype=torch.uint8)[:, :w]
    uv = torch.zeros((h // 2, uv_pitch or w), dtype=torch.uint8)[:, :w].unflatten(1, (w // 2, 2))
    return y, uv


class CDesc(ctypes.Structure):  # ym_nv12_desc as include/yolomi.h declares it
    _fields_ = [("y", ctypes.c_void_p), ("uv", ctypes.c_void_p)] + [(n, ctypes.c_int) for n in (
        "h", "w", "y_pitch", "uv_pitch", "uh", "uw", "top", "left")] + [("scale_x", ctypes.c_double), ("scale_y", ctypes.c_double)]


def test_table_of_pitched_planes_and_of_a_surface():
    rt = Recorder()
    (y0, uv0), (y1, uv1) = planes(120, 160, 197, 166), planes(90, 50)
    out, shapes = letterbox_nv12(rt, NV12Frames([y0, y1], [uv0, uv1], "bt709", True), CPU, 160, 32, 5)
    (host, dev, B, coef, dst, Hn, Wn, stream), = rt.calls
    assert (B, Hn, Wn, stream, dst) == (2, 160, 160, 5, out.data_ptr()) and shapes == [(120, 160), (90, 50)]
    assert out.shape == (2, 3, 160, 160) and out.dtype == torch.float32 and np.array_equal(host, dev)
    assert coef == nv12_coefficients("bt709", True) and NV12_DESC.itemsize == ctypes.sizeof(CDesc) == 64
    assert [NV12_DESC.fields[n][1] for n, _ in CDesc._fields_] == [getattr(CDesc, n).offset for n, _ in CDesc._fields_]
    for d, y, uv in zip(host, (y0, y1), (uv0, uv1)):
        h, w = y.shape
        uh, uw, t, _, l, _ = letterbox_geometry(h, w, (160, 160), auto=False)
        assert (d["y"], d["uv"], d["h"], d["w"]) == (y.data_ptr(), uv.data_ptr(), h, w)
        assert (d["y_pitch"], d["uv_pitch"]) == (y.stride(0), uv.stride(0)) and (d["uh"], d["uw"], d["top"], d["left"]) == (uh, uw, t, l)
        assert (d["scale_x"], d["scale_y"]) == (1.0 / (uw / w), 1.0 / (uh / h))
    assert (host[0]["y_pitch"], host[0]["uv_pitch"]) == (197, 166)
    surf = torch.zeros((2, 180, 160), dtype=torch.uint8)  # two contiguous surfaces: views, no copy
    letterbox_nv12(rt, NV12Frames.from_surface(surf), CPU, 160, 32, 0)
    host = rt.calls[1][0]
    assert [int(p) for p in host["y"]] == [surf[0].data_ptr(), surf[1].data_ptr()] and rt.calls[1][5:7] == (128, 160)
    assert [int(p) for p in host["uv"]] == [int(p) + 120 * 160 for p in host["y"]] and set(host["uv_pitch"]) == {160}
    assert rt.calls[1][3] == nv12_coefficients("bt601", False)


def test_coefficients():
    assert nv12_coefficients() == (16, 1220542, 2116026, -409993, -852492, 1673527)  # OpenCV's ITUR_BT_601_* integers
    assert nv12_coefficients("BT709", True) == (0, 1 << 20, 1945738, -196398, -490838, 1651297)
    with pytest.raises(ValueError):
        nv12_coefficients("bt2020")


@pytest.mark.parametrize("make,device,err", [
    (lambda: NV12Frames([planes(8, 8)[0].float()], [planes(8, 8)[1]]), CPU, TypeError),         # y not uint8
    (lambda: NV12Frames(torch.zeros((8, 8), dtype=torch.uint8), [planes(8, 8)[1]]), CPU, TypeError),  # a bare plane
    (lambda: NV12Frames([planes(8, 8)[0]], [torch.zeros((4, 8), dtype=torch.uint8)]), CPU, TypeError),  # uv of rank 2
    (lambda: NV12Frames([planes(8, 16)[0][:, ::2]], [planes(8, 8)[1]]), CPU, ValueError),       # y element stride 2
    (lambda: NV12Frames([planes(8, 8)[0]], [torch.zeros((4, 2, 4), dtype=torch.uint8).permute(0, 2, 1)]), CPU, ValueError),
    (lambda: NV12Frames([planes(6, 10)[0][:5]], [planes(6, 10)[1]]), CPU, ValueError),          # odd height
    (lambda: NV12Frames([planes(8, 8)[0]], [planes(8, 12)[1]]), CPU, ValueError),               # uv of another frame
    (lambda: NV12Frames([], []), CPU, ValueError),
    (lambda: NV12Frames(*[[p] for p in planes(8, 8)]), torch.device("cuda", 0), ValueError),    # host planes, device model
    (lambda: planes(8, 8), CPU, TypeError),                                                      # not NV12Frames
], ids=["float", "bare", "uv-rank", "y-stride", "uv-stride", "odd", "mismatch", "empty", "host-frame", "tuple"])
def test_refused_before_any_call(make, device, err):
    rt = Recorder()
    with pytest.raises(err):
        letterbox_nv12(rt, make(), device, 64, 32, 0)
    assert not rt.calls


def test_header_and_exported_carry_the_entries():
    import yolomi.lib as L
    hdr = open(os.path.join(ROOT, "include", "yolomi.h")).read()
    for name in ("ym_letterbox_nv12", "ym_nv12_to_bgr"):
        assert re.search(rf"^int {name}\(", hdr, re.M) and name in L.EXPORTED
