"""Host tests of the conv-config catalogue and its dispatch routine (yolo-infer_amd/csrc/ym_conv_catalog.h), built with a
plain C++ compiler (tests/conv_dispatch_check.cpp): the dispatch trace over every (dtype, shape class, strict, stub policy,
cfg) against the golden recorded from the dispatch code the routine replaced, the resolver against the family ranges
the GPU tests state on their own, and the split-pair helpers."""
import os
import subprocess

import pytest

from tests.test_plan_format import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "conv_dispatch_trace.txt")
# tests/test_gpu_conv_ops.py F16_FAMILIES / X3_FAMILIES, restated (that module needs torch and the GPU marker)
F16_FAMILIES = (("direct", 0, 12), ("lds", 12, 5), ("dma", 17, 30), ("stream", 47, 31), ("small", 78, 12),
                ("halo", 90, 12), ("bneck", 102, 14))
N_F16 = 116
X3_FAMILIES = (("dma_x3", N_F16, 9), ("bneck_x3", N_F16 + 9, 2))
DT_F16, DT_F32, DT_I8, DT_F8, DT_X3 = range(5)  # csrc/ym_plan.h YM_DT_*


@pytest.fixture(scope="session")
def check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    exe = tmp_path_factory.mktemp("conv_dispatch_check") / "conv_dispatch_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "conv_dispatch_check.cpp"),
           "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # no sanitizer runtimes: a plain build
        subprocess.run(cmd, check=True)

    def run(mode, text=""):
        p = subprocess.run([str(exe), mode], input=text, capture_output=True, text=True, timeout=120)
        assert p.stderr == "", p.stderr  # the sanitizers stay silent
        assert p.returncode == 0, p.stdout[-500:]
        return p.stdout
    return run


def test_dispatch_reproduces_the_recorded_trace(check):
    got = check("trace").splitlines()
    ref = open(GOLDEN).read().splitlines()
    for i, (g, r) in enumerate(zip(got, ref)):
        if g != r:
            head = next(l for l in reversed(ref[:i + 1]) if not l.startswith(" "))
            assert g == r, f"line {i + 1} of {head!r}: got {g!r}, recorded {r!r}"
    assert len(got) == len(ref)


def test_the_trace_covers_the_case_grid():
    """5 dtypes x the 8 shape classes of the grid (and one more: unmet int8 preconditions) x strict x 4 policies."""
    heads = [l.split() for l in open(GOLDEN).read().splitlines() if not l.startswith(" ")]
    assert len(heads) == len({tuple(h) for h in heads}) == 5 * 9 * 2 * 4
    assert {h[0] for h in heads} == {"f16", "f32", "x3", "int8", "fp8"}
    assert {h[1] for h in heads} >= {"1x1", "1x1-concat", "3x3", "3x3-up0", "pair-k2=1", "pair-k2=3", "dw", "kpad%64"}
    assert {h[3] for h in heads} == {"accept", "refuse", "only2", "error"}
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f))
                                          for f in os.listdir(os.path.dirname(GOLDEN)) if f != os.path.basename(GOLDEN))


def test_resolver_maps_the_family_ranges(check):
    q, want = [], []
    for dt, fams in ((DT_F16, F16_FAMILIES), (DT_F32, F16_FAMILIES), (DT_X3, F16_FAMILIES + X3_FAMILIES)):
        for name, first, count in fams:
            q += [(dt, 0, first), (dt, 0, first + count - 1)]
            want += [f"{name} 0", f"{name} {count - 1}"]
        end = fams[-1][1] + fams[-1][2]
        q += [(dt, 0, -1), (dt, 0, end)]
        want += ["none -1", "none -1"]
    # int8: conv_i8 tiles, the int8 streaming ids (35 in all), then LDS-DMA in its Q8 mode; fp8: the 35; dwpw: 0..7
    q += [(DT_I8, 0, 0), (DT_I8, 0, 11), (DT_I8, 0, 12), (DT_I8, 0, 34), (DT_I8, 0, 35), (DT_I8, 0, 64), (DT_I8, 0, 65),
          (DT_F8, 0, 34), (DT_F8, 0, 35), (DT_X3, 1, 0), (DT_X3, 1, 7), (DT_X3, 1, 8), (DT_F16, 1, 7)]
    want += ["conv_i8 0", "conv_i8 11", "i8_stream 0", "i8_stream 22", "dma 0", "dma 29", "none -1",
             "i8_stream 22", "none -1", "dwpw 0", "dwpw 7", "none -1", "dwpw 7"]
    got = check("resolve", "".join(f"{a} {b} {c}\n" for a, b, c in q)).splitlines()
    assert got == want, [(a, g, w) for a, g, w in zip(q, got, want) if g != w]


def test_split_pair_helpers_round_trip(check):
    assert check("split") == "ok\n"


def test_header_is_plain_cxx():
    src = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "ym_conv_catalog.h")).read()
    assert [l.split("//")[0].strip() for l in src.splitlines() if l.startswith("#include")] == ['#include "ym_plan.h"']
