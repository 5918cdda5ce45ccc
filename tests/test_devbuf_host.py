"""Host test of the grow-on-demand device buffer (csrc/ym_devbuf.h), which the embed partials and the mask, annotator,
contour and RLE scratch all go through.  The checks run in tests/devbuf_check.cpp, a stand-alone host program that
includes only that header (and yolomi.h for the status codes) and stands a malloc / free device with an injectable
failure under it; built here with -Wall -Werror, and with AddressSanitizer and UBSan where the compiler has their
runtimes."""
import os
import subprocess

import pytest

from tests.test_plan_format import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def devbuf_check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    exe = tmp_path_factory.mktemp("devbuf_check") / "devbuf_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "devbuf_check.cpp"), "-o", str(exe)]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run(cmd + san, capture_output=True).returncode != 0:  # no sanitizer runtimes: a plain build
        subprocess.run(cmd, check=True)
    return str(exe)


def test_grow_free_and_failure_sequence(devbuf_check):
    p = subprocess.run([devbuf_check], capture_output=True, text=True, timeout=60)
    assert p.stderr.strip() == "", p.stderr  # the sanitizers stay silent
    assert p.returncode == 0, p.stdout
    assert p.stdout.strip() == "OK"


def test_header_is_plain_cxx():
    src = open(os.path.join(ROOT, "yolo-infer_amd", "csrc", "ym_devbuf.h")).read()
    assert [l for l in src.splitlines() if l.startswith("#include")] == ["#include <cstddef>"]
