"""Host tests of the NMS scratch layout (csrc/ym_nms_ws.h), which the forward's arena and the merged test-time-
augmentation scratch both go through.  The checks of one layout (alignment, bounds, disjoint regions, enough bytes for
what each kernel indexes, kstride) run in tests/nms_ws_check.cpp, a stand-alone host program that includes only that
header, built here with AddressSanitizer and UBSan where the compiler has their runtimes; the total is compared here
with the sum the runtime's workspace arithmetic gave for the same regions before the layout had a header of its own."""
import os
import subprocess

import pytest

from tests.test_plan_format import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ML_CAP, ML_STATE_BYTES = 32768, 24  # csrc/ym_nms_ml.hip: keys per image of sel / sel2; sizeof(MlState)


@pytest.fixture(scope="session")
def nms_ws_check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    exe = tmp_path_factory.mktemp("nms_ws_check") / "nms_ws_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "nms_ws_check.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # no sanitizer runtimes: a plain build
        subprocess.run(cmd, check=True)

    def run(nB, A, ml, rows):
        p = subprocess.run([str(exe), str(nB), str(A), str(ml), str(rows)], capture_output=True, text=True, timeout=60)
        return p.returncode, p.stdout.strip(), p.stderr.strip()
    return run


def _al(x):
    return (x + 255) // 256 * 256


def parent_total(nB, A, ml, rows):
    """ensure_workspace's (rows = 0) and ensure_tta's sum over the NMS regions: each region rounded up to 256 bytes."""
    ks = 1
    while ks < A:
        ks *= 2
    BA = nB * A
    t = 2 * _al(BA * 16) + 3 * _al(BA * 4) + 2 * _al(nB * ks * 8) + _al(nB * 4) + _al(BA)
    if rows:
        t += _al(BA * rows * 4)
    if ml:
        t += 2 * _al(nB * ML_CAP * 8) + _al(nB * 1024 * 4) + _al(nB * ML_STATE_BYTES) + _al(nB * 4)
    return t, ks


@pytest.mark.parametrize("rows", [0, 80])
@pytest.mark.parametrize("ml", [0, 1])
@pytest.mark.parametrize("nB,A", [(1, 21), (3, 2100), (8, 8400), (2, 7917)])
def test_layout(nB, A, ml, rows, nms_ws_check):
    code, out, err = nms_ws_check(nB, A, ml, rows)
    assert err == "", err  # the sanitizers stay silent
    assert code == 0, out
    total, ks = parent_total(nB, A, ml, rows)
    assert ks >= A and (ks == 1 or ks // 2 < A) and ks & (ks - 1) == 0
    assert out == f"OK {total} {ks}"


def test_header_is_plain_cxx():
    src = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "ym_nms_ws.h")).read()
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>"]
