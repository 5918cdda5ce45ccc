"""COCO RLE without a GPU: the oracle on answers worked by hand; csrc/ym_rle.h run serially by tests/rle_check.cpp."""
import os
import subprocess

import numpy as np
import pytest

from tests.rle_oracle import decode, encode
from tests.test_plan_format import _compiler

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def plane(h, w, set_indices):  # the given column-major indices set
    flat = np.zeros(h * w, dtype=np.uint8)
    flat[list(set_indices)] = 1
    return flat.reshape(w, h).T


KNOWN = [(plane(3, 3, [4]), [4, 1, 4], b"414"), (plane(3, 3, range(9)), [0, 9], b"09"),
         (plane(3, 3, [2, 6]), [2, 1, 3, 1, 2], b"2130O"), (plane(10, 10, []), [100], b"T3")]


@pytest.mark.parametrize("m,counts,string", KNOWN, ids=[s.decode() for _, _, s in KNOWN])
def test_known_answers(m, counts, string):
    got = encode(m)
    assert got[0].dtype == np.uint32 and got[0].tolist() == counts and got[1] == string and got[2] == int(m.sum())
    assert np.array_equal(decode(string, m.shape), m)


@pytest.mark.parametrize("shape,density", [((5, 7), 0.5), ((33, 65), 0.3), ((640, 3), 0.02), ((64, 64), 0.98)], ids=str)
def test_decode_inverts_encode(shape, density):
    m = (np.random.default_rng(shape[0]).random(shape) < density).astype(np.uint8)
    counts, string, area = encode(m)
    assert int(counts.sum()) == m.size and area == int(m.sum()) and np.array_equal(decode(string, shape), m)


def test_entry_is_bound():
    from yolomi.lib import EXPORTED
    assert "ym_mask_rle" in EXPORTED


def test_shared_header_against_a_per_pixel_loop(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    exe = tmp_path / "rle_check"
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", os.path.join(ROOT, "tests", "rle_check.cpp"), "-o", str(exe)]
    if subprocess.run(cmd + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"],
                      capture_output=True).returncode != 0:  # no sanitizer runtimes: a plain build
        subprocess.run(cmd, check=True)
    p = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert p.stderr == "" and p.returncode == 0 and p.stdout.startswith("ok "), p.stderr[-500:]  # sanitizers silent
