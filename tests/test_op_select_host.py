"""Host test of the launch rules of the attention, depthwise and SPPF ops (yolo-infer_amd/csrc/ym_op_select.h), built
with a plain C++ compiler (tests/op_select_check.cpp): the variant code the rules select over a grid of dtypes, shapes
and switches against the golden recorded from the three launchers the rules were written out of."""
import os
import subprocess

import pytest

from tests.test_plan_format import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "op_select_trace.txt")


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    exe = tmp_path_factory.mktemp("op_select_check") / "op_select_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "op_select_check.cpp"),
           "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # no sanitizer runtimes: a plain build
        subprocess.run(cmd, check=True)

    def run(*args):
        p = subprocess.run([str(exe), *args], capture_output=True, text=True, timeout=120)
        assert p.stderr == "", p.stderr  # the sanitizers stay silent
        assert p.returncode == 0, p.stdout[-500:]
        return p.stdout
    return run


def test_rules_reproduce_the_recorded_trace(check):
    got = check("trace")
    ref = open(GOLDEN).read()
    gl, rl = got.splitlines(), ref.splitlines()
    for i, (g, r) in enumerate(zip(gl, rl)):
        if g != r:
            head = next(l for l in reversed(rl[:i + 1]) if not l.startswith(" "))
            assert g == r, f"line {i + 1} of {head!r}: got {g!r}, recorded {r!r}"
    assert len(gl) == len(rl)
    assert got == ref  # byte for byte


def test_sections_are_the_trace_in_parts(check):
    """The once-per-process switches are arguments of the rules: a section per value is the whole trace."""
    parts = [check("attn", "0"), check("attn", "1")]
    parts += [check("dw", str(p), str(r)) for p, r in ((0, 0), (2, 0), (4, 0), (0, 2), (0, 4))]
    assert "".join(parts + [check("sppf")]) == open(GOLDEN).read()


def test_the_trace_covers_the_case_grid():
    lines = open(GOLDEN).read().splitlines()
    heads = [l for l in lines if not l.startswith(" ")]
    assert [h.split(":")[0].rsplit(" ", 1)[0] for h in heads] == (
        ["attn flash_off=0", "attn flash_off=1"] +
        [f"dw pxt={p} rt={r} (C," for p, r in ((0, 0), (2, 0), (4, 0), (0, 2), (0, 4))] + ["sppf"])
    rows = [l.split(":")[0].strip() for l in lines if l.startswith(" ")]
    attn = 3 * 4 * 5               # dtypes x (plain, raw, misaligned d_coff, kd 16) x (B, nh); 16 N per row
    dw = 8 * 2 * 3 * 4             # maps x raw x modes x tiles; 3 dtypes x 4 C x 3 B per row
    assert len(rows) == 2 * attn + 5 * dw + 5 * 2
    codes = {int(t) for l in lines if l.startswith(" ") for t in l.split(":")[1].split() if t.lstrip("-").isdigit()}
    assert codes == set(range(-1, 14))  # every variant code of the three ops (the largest count is attention's 14)
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f))
                                          for f in os.listdir(os.path.dirname(GOLDEN)) if f != os.path.basename(GOLDEN))


def test_header_is_plain_cxx():
    src = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "ym_op_select.h")).read()
    assert [l.split("//")[0].strip() for l in src.splitlines() if l.startswith("#include")] == ['#include "ym_plan.h"']
