"""Host test of the Python call path (core/model.py predict / track / embed) on CPU tensors against a scripted engine
(tests/predict_trace.py): the trace of the working tree equals the one recorded from the code before the call path was
refactored, byte for byte — the engine calls and their arguments, `_mask_cap`, and every Results' shapes, hashes and
view-or-gather structure."""
import os

from tests.predict_trace import cases, trace

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "predict_trace.txt")


def test_predict_reproduces_the_recorded_trace():
    got = trace().splitlines()
    ref = open(GOLDEN).read().splitlines()
    for i, (g, r) in enumerate(zip(got, ref)):
        if g != r:
            head = next(l for l in reversed(ref[:i + 1]) if l.startswith("case "))
            assert g == r, f"line {i + 1} of {head!r}: got {g!r}, recorded {r!r}"
    assert len(got) == len(ref)


def test_the_trace_covers_the_case_matrix():
    text = open(GOLDEN).read()
    blocks = text.split("case ")[1:]
    assert len(blocks) == len(cases()) == len({b.split(":")[0] for b in blocks})
    by = {b.split(":")[0]: b for b in blocks}
    # one device->host read on the slot path means masks() is not called there; the exact-size path calls it
    assert "call masks(" not in by["segment-tensor-slots-views"] and "call masks(" in by["segment-tensor-above-cap"]
    assert "call masks_slots(" not in by["segment-tensor-budget-0"]
    assert " gather " in by["segment-tensor-compact"] and " gather " in by["segment-tensor-slots-drop"]
    assert "call run_tta(" in by["detect-tensor-augment"] and "call run(" in by["pose-tensor-augment"]
    assert "_mask_cap 40" in by["segment-tensor-above-cap-drop"]
    assert "_mask_cap 32" in by["segment-tensor-cap-follows-down"]
    for task in ("detect", "pose"):
        for path in ("tensor-async", "image", "track-tensor", "track-image-persist", "embed-tensor", "embed-image"):
            assert f"{task}-{path}" in by
    for src in ("tensor", "image"):
        for path in ("retina", "retina-drop", "zero", "slots-one-zero"):
            assert f"segment-{src}-{path}" in by
