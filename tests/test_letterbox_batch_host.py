"""Host side of the frame-batch letterbox (yolomi.preprocess.letterbox_frames): geometry, the descriptor table and the
refusals, with a runtime that records its one call (CPU tensors stand in for device frames)."""
import ctypes

import numpy as np
import pytest
import torch

from yolomi.preprocess import LB_DESC, is_frame_source, letterbox_frames, letterbox_geometry

CPU = torch.device("cpu")


class Recorder:
    def __init__(self):
        self.calls = []

    def letterbox_batch(self, desc_ptr, host_desc_ptr, B, dst_ptr, Hn, Wn, stream):
        host = np.frombuffer(ctypes.string_at(host_desc_ptr, B * LB_DESC.itemsize), dtype=LB_DESC)
        dev = np.frombuffer(ctypes.string_at(desc_ptr, B * LB_DESC.itemsize), dtype=LB_DESC)
        self.calls.append((host, dev, B, dst_ptr, Hn, Wn, stream))


def frame(h, w):
    return torch.zeros((h, w, 3), dtype=torch.uint8)


@pytest.mark.parametrize("shapes,canvas", [([(120, 160), (120, 160)], (128, 160)), ([(120, 160), (90, 50)], (160, 160))],
                         ids=["equal-auto", "mixed-square"])
def test_table_and_geometry(shapes, canvas):
    rt = Recorder()
    wide = torch.zeros((120, 200, 3), dtype=torch.uint8)
    frames = [wide[:, 7:167]] + [frame(*s) for s in shapes[1:]]  # frame 0: a column slice, rows 600 bytes apart
    out, got_shapes = letterbox_frames(rt, frames, CPU, 160, 32, 5, bgr=False)
    (host, dev, B, dst, Hn, Wn, stream), = rt.calls
    assert (B, Hn, Wn, stream, dst) == (len(shapes), *canvas, 5, out.data_ptr()) and got_shapes == shapes
    assert out.shape == (len(shapes), 3, *canvas) and out.dtype == torch.float32 and np.array_equal(host, dev)
    assert LB_DESC.itemsize == 56
    for d, f, (h, w) in zip(host, frames, shapes):
        uh, uw, t, _, l, _ = letterbox_geometry(h, w, (160, 160), auto=len(set(shapes)) == 1)
        assert (d["src"], d["h"], d["w"], d["row_bytes"], d["bgr"]) == (f.data_ptr(), h, w, f.stride(0), 0)
        assert (d["uh"], d["uw"], d["top"], d["left"]) == (uh, uw, t, l)
        assert (d["scale_x"], d["scale_y"]) == (1.0 / (uw / w), 1.0 / (uh / h))
    assert host[0]["row_bytes"] == 600 and host[0]["src"] == wide.data_ptr() + 21
    batch = torch.zeros((2, 120, 160, 3), dtype=torch.uint8)  # a 4-D batch is its frames
    letterbox_frames(rt, batch, CPU, 160, 32, 0)
    assert [int(p) for p in rt.calls[1][0]["src"]] == [batch[0].data_ptr(), batch[1].data_ptr()]


@pytest.mark.parametrize("frames,device,err", [
    ([frame(8, 8).float()], CPU, TypeError),                          # not uint8
    ([torch.zeros((3, 8, 8), dtype=torch.uint8)], CPU, TypeError),    # CHW
    ([frame(8, 24).view(8, 8, 3, 3)[:, :, :, 0]], CPU, ValueError),   # pixel stride 9
    ([frame(8, 8).permute(1, 0, 2)], CPU, ValueError),                # transposed: row stride below 3 * W
    ([frame(8, 8)], torch.device("cuda", 0), ValueError),             # a host frame for a device model
    ([], CPU, ValueError),
], ids=["float", "chw", "pixel-stride", "transposed", "host-frame", "empty"])
def test_refused_before_any_call(frames, device, err):
    rt = Recorder()
    with pytest.raises(err):
        letterbox_frames(rt, frames, device, 64, 32, 0)
    assert not rt.calls


def test_frame_source_rule():
    u8 = torch.uint8
    assert is_frame_source(torch.zeros((2, 8, 8, 3), dtype=u8)) and is_frame_source([frame(8, 8), frame(4, 6)])
    assert not is_frame_source(torch.zeros((2, 3, 8, 8), dtype=u8)) and not is_frame_source(frame(8, 8))
    assert not is_frame_source([frame(8, 8).float()]) and not is_frame_source([]) and not is_frame_source(np.zeros((8, 8, 3), np.uint8))
