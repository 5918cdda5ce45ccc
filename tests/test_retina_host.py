"""retina_masks=True, host side (no GPU): the scale_masks window arithmetic, the C-ABI entry, and how far the fp32
restatement of process_mask_native is from its float64 evaluation (what the GPU tests' per-mask floor rests on)."""
import os
import re

import pytest
import torch

from oracle.predict import OracleModel
from tests import retina_oracle as ro
from tests.golden.make_golden import make_input
from yolomi.preprocess import mask_window
from yolomi.synth import synth_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(320, 320), (240, 427), (500, 333), (97, 61)]
WINDOWS = {(320, 320): (0, 80, 0, 80), (240, 427): (17, 62, 0, 80), (500, 333): (0, 80, 13, 67),
           (97, 61): (0, 80, 15, 65)}

_cache = {}


def oracle_rows():
    """yolo11n-seg (synthetic weights, seed 0) on make_input("uniform", (81, 82), 320) at conf 0.25, computed once."""
    if "rows" not in _cache:
        torch.set_num_threads(min(16, os.cpu_count() or 1))
        om = OracleModel("n", "segment", synth_weights("n", "segment", 0))
        _cache["rows"] = ro.oracle_rows(om, make_input("uniform", (81, 82), 320), 0.25)
    return _cache["rows"]


@pytest.mark.parametrize("shape", SHAPES)
def test_mask_window_values(shape):
    assert mask_window(80, 80, shape) == WINDOWS[shape]
    assert ro.mask_window(80, 80, shape) == WINDOWS[shape]


def test_mask_window_never_empty():
    """An aspect ratio whose window rounds to nothing (upstream's interpolate raises there) still gets one row."""
    for shape in ((1, 10000), (10000, 1), (1, 1), (3, 7)):
        t, b, l, r = mask_window(80, 80, shape)
        assert 0 <= t < b <= 80 and 0 <= l < r <= 80, (shape, t, b, l, r)


def test_capi_declares_masks_native():
    import yolomi.lib as L
    hdr = open(os.path.join(ROOT, "include", "yolomi.h")).read()
    assert re.search(r"^int\s+ym_masks_native\s*\(", hdr, re.M)
    assert "ym_masks_native" in L.EXPORTED


def test_oracle_input_keeps_28_and_2():
    dets, proto, net = oracle_rows()
    assert [len(d) for d in dets] == [28, 2] and net == (320, 320) and tuple(proto.shape) == (2, 32, 80, 80)


@pytest.mark.parametrize("shape", SHAPES)
def test_restatement_fp32_within_one_pixel_of_float64(shape):
    """Per mask, the fp32 restatement (upstream's precision) and its float64 evaluation differ by at most 1 pixel; every
    mask is non-empty in both.  F.interpolate itself agrees with the written-out bilinear resize to the same bar."""
    from oracle import postprocess as pp
    dets, proto, net = oracle_rows()
    for b, d in enumerate(dets):
        d = d.clone()
        d[:, :4] = pp.scale_boxes(net, d[:, :4], shape)
        args32 = (proto[b], d[:, 6:], d[:, :4], shape)
        m32 = ro.process_mask_native(*args32)
        m64 = ro.process_mask_native(proto[b].double(), d[:, 6:].double(), d[:, :4].double(), shape)
        mi = ro.process_mask_native(*args32, interpolate=True)
        assert tuple(m32.shape) == (len(d), *shape) and m32.dtype == torch.bool
        diff = (m32 != m64).flatten(1).sum(1)
        print(f"shape {shape} image {b}: fp32 vs float64 max {int(diff.max())} px, "
              f"F.interpolate vs written-out max {int((mi != m32).flatten(1).sum(1).max())} px")
        assert int(diff.max()) <= 1, diff.tolist()
        assert int((mi != m64).flatten(1).sum(1).max()) <= 1
        assert bool(m64.flatten(1).any(1).all()) and bool(m32.flatten(1).any(1).all())
