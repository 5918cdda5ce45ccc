"""Host tests of the plan blob format (csrc/ym_plan.h, yolomi/plan.py): the two sides name the slots alike, the
packer's bytes have not moved, and the parser every load goes through (ym_plan_parse) accepts the packer's blobs and
rejects malformed ones with a message.  The parser runs in tests/plan_check.cpp, a stand-alone host program built
here with AddressSanitizer and UBSan, so a check that reads out of bounds before it rejects fails too."""
import glob
import hashlib
import json
import os
import re
import shutil
import struct
import subprocess

import pytest

from tests.test_pose_host import PARENT_BLOBS, PARENT_QBLOBS
from yolomi.plan import HDR_FIELDS, OP_FIELDS, field_offset, pack_model, unpack_blob
from yolomi.synth import synth_weights

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yolo-infer_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")


def _compiler():
    cands = [shutil.which("c++")] + sorted(glob.glob("/opt/rocm*/llvm/bin/clang++") +
                                           glob.glob("/opt/rocm*/lib/llvm/bin/clang++"))
    return next((c for c in cands if c), None)


@pytest.fixture(scope="session")
def plan_check(tmp_path_factory):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler (c++ or ROCm's clang++)")
    exe = tmp_path_factory.mktemp("plan_check") / "plan_check"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "plan_check.cpp"), os.path.join(CSRC, "ym_plan.cpp"), "-o", str(exe)],
                   check=True)
    scratch = tmp_path_factory.mktemp("blobs")

    def run(blob: bytes):
        path = scratch / "blob.bin"
        path.write_bytes(blob)
        p = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=60)
        return p.returncode, p.stdout.strip(), p.stderr.strip()
    return run


@pytest.fixture(scope="session")
def blobs():
    """The twelve plans of PARENT_BLOBS / PARENT_QBLOBS, packed once with the fusion switches at their defaults."""
    from oracle import quant as Q
    saved = {v: os.environ.pop(v, None) for v in ("YM_FUSE", "YM_FUSE_DW", "YM_DW_FUSE_STRIDES")}
    try:
        out, sds = {}, {}
        for scale, task, dtype in PARENT_BLOBS:
            if (scale, task) not in sds:
                sds[(scale, task)] = synth_weights(scale, task, 0)
            out[(scale, task, dtype)] = pack_model(scale, task, sds[(scale, task)], dtype)
        for name, dtype in PARENT_QBLOBS:
            g = json.load(open(os.path.join(GOLD, name + ".json")))
            sd = synth_weights(g["scale"], g["task"], g["weights_seed"])
            out[(name, dtype)] = pack_model(g["scale"], g["task"], sd, dtype, Q.qparams_from_json(g["qparams"]))
        return out
    finally:
        os.environ.update({v: x for v, x in saved.items() if x is not None})


def _members(struct_name: str):
    src = open(os.path.join(CSRC, "ym_plan.h")).read()
    body = src[src.index(f"struct {struct_name} {{"):]
    body = body[body.index("fields begin"):body.index("fields end")]
    return tuple(re.findall(r"^\s*int32_t\s+(\w+);", body, re.M))


def test_field_names_match_the_header():
    assert _members("PlanHeader") == HDR_FIELDS and len(HDR_FIELDS) == 32
    assert _members("OpRec") == OP_FIELDS and len(OP_FIELDS) == 32
    assert [f for f in HDR_FIELDS if f.startswith("stride")] == ["stride0", "stride1", "stride2"]


def test_blobs_are_byte_identical_to_the_parent(blobs):
    want = {**PARENT_BLOBS, **PARENT_QBLOBS}
    assert len(want) == len(blobs) == 12
    got = {k: hashlib.sha256(b).hexdigest() for k, b in blobs.items()}
    assert got == want


def test_unpack_blob_round_trip(blobs):
    blob = blobs[("n", "detect", "f16")]
    h, bufs, ops, names, woff = unpack_blob(blob)
    assert h.nbuf == h[11] == len(bufs) and h.nop == h[12] == len(ops) == len(names)
    assert len(blob) == woff + (h.wbytes_lo | h.wbytes_hi << 32)
    i = next(i for i, r in enumerate(ops) if r.kind == 2)
    assert struct.unpack_from("<i", blob, field_offset(h, "kpad", i))[0] == ops[i].kpad == ops[i][21]
    assert struct.unpack_from("<i", blob, field_offset(h, "nop"))[0] == h.nop


def test_parser_accepts_every_packed_plan(blobs, plan_check):
    for key, blob in blobs.items():
        assert plan_check(blob) == (0, "OK", ""), key


def _set(blob: bytes, off: int, val: int) -> bytes:
    b = bytearray(blob)
    struct.pack_into("<i", b, off, val)
    return bytes(b)


def _first(ops, pred):
    return next(i for i, r in enumerate(ops) if pred(r))


# (case, the plan it mutates, mutation(blob, header, ops) -> bytes, words of the message the parser answers with)
RECORDS = "buffer id, channel view or weight range out of bounds"
DET, I8, POSE = ("n", "detect", "f16"), ("det_n_i8_qnnpack", "i8"), ("n", "pose", "f16")


def _conv(field, val):  # a slot of the first conv record; val may depend on the header
    def m(blob, h, ops):
        v = val(h) if callable(val) else val
        return _set(blob, field_offset(h, field, _first(ops, lambda r: r.kind == 2)), v)
    return m


MUTATIONS = [
    ("bad magic", DET, lambda b, h, ops: _set(b, field_offset(h, "magic"), 0x12345678), "magic"),
    ("nop 5000", DET, lambda b, h, ops: _set(b, field_offset(h, "nop"), 5000), "buffer/op counts"),
    ("nl 4", DET, lambda b, h, ops: _set(b, field_offset(h, "nl"), 4), "level count"),
    ("one weight byte short", DET, lambda b, h, ops: b[:-1], "truncated"),
    ("wbytes beyond the blob", DET, lambda b, h, ops: _set(b, field_offset(h, "wbytes_lo"), len(b) + 1), "truncated"),
    ("conv src0 = nbuf + 7", DET, _conv("src0", lambda h: h.nbuf + 7), RECORDS),
    ("conv src0_coff = -1", DET, _conv("src0_coff", -1), RECORDS),
    ("conv c0 = 1 << 20", DET, _conv("c0", 1 << 20), RECORDS),
    ("conv dst = -1", DET, _conv("dst", -1), RECORDS),
    ("conv kpad = 0", DET, _conv("kpad", 0), RECORDS),
    ("conv w_off = 0x7FFFFFF0", DET, _conv("w_off", 0x7FFFFFF0), RECORDS),
    ("fused pair mid = nbuf", DET,
     lambda b, h, ops: _set(b, field_offset(h, "mid", _first(ops, lambda r: r.kind == 2 and r.k2)), h.nbuf), RECORDS),
    ("i8 q_off = wbytes", I8,
     lambda b, h, ops: _set(b, field_offset(h, "q_off", _first(ops, lambda r: r.kind == 2)), h.wbytes_lo), RECORDS),
    ("pose kpt_off = 66", POSE, lambda b, h, ops: _set(b, field_offset(h, "kpt_off"), 66), "pose head geometry"),
]


@pytest.mark.parametrize("case,plan,mutate,words", MUTATIONS, ids=[m[0].replace(" ", "_") for m in MUTATIONS])
def test_parser_rejects_malformed_blob(case, plan, mutate, words, blobs, plan_check):
    blob = blobs[plan]
    h, _, ops, _, _ = unpack_blob(blob)
    assert h.wbytes_hi == 0
    bad = mutate(blob, h, ops)
    assert bad != blob
    code, out, err = plan_check(bad)
    assert err == "", err  # the sanitizers stay silent
    assert code == 1 and words in out, (case, code, out)
