"""Model blob packer: Ultralytics-style state dict + YOLO11 plan → one binary blob for `ym_load_weights`.

Replaces what Ultralytics' AutoBackend(fuse=True) does on first predict: Conv+BN folding
(`fuse_conv_and_bn`, restated bit-for-bit in fp32: W' = (γ/√(eps+σ²))·W, b' = β − γ·μ/√(σ²+eps)), then — the MI355X
part — packing every conv as a K-contiguous GEMM B operand [N][Kpad] with K ordered (ky, kx, c) to match the NHWC
implicit-GEMM loader (`csrc/ym_conv.hip`), the stem's Cin padded 3→8, ConvTranspose2d(2,2) re-laid out as a 1x1
GEMM with N = 4·C (pixel-shuffle epilogue), depthwise weights as [9][C] fp32.

int8 plans (dtype "i8", the runtime of the reference's PostTrainingQuantizer.convert,
`optimization/quantization/quantizers.py:77`): weights quantized with the torch.ao observer of the calibrated
backend, K padded to 16-channel granules per tap, and per op a `QRec` (csrc/ym_common.h: requantisation of the conv
output, the 256-entry post-activation table, the stored tensor's / residual's / input's quantisation), the fp32
s_in·s_w per output channel and the int32 zero-point correction Σ_k (128 - z_in)·w (activations are stored as q - 128).

x3 plans (dtype "x3", the parity plan benched): activations in the pair layout of csrc/ym_common.h (every 8-channel
chunk as fp16 hi = fp16(x) then lo = fp16(x - hi)); every conv weight row except the stem's likewise, [hi x8 | lo x8]
per K chunk, of the weights scaled by a power of two 2^s (max |w·2^s| in (2^13, 2^14], so the lo parts stay normal;
the record's x3 exponents), so kpad counts fp16 storage elements: 2·K padded to 64.  The stem
keeps fp32 rows.

Blob layout: `csrc/ym_plan.h` (PlanHeader, OpRec) describes every slot; HDR_FIELDS and OP_FIELDS below name them with
the same words, in the same order.
"""
from __future__ import annotations

import struct
from collections import namedtuple
from typing import Dict, List

import numpy as np

from .arch import REG_MAX, STRIDES, GraphBuilder

MAGIC = 0x4C504D59
VERSION = 1
OP_IDS = {"input": 1, "conv": 2, "dwconv": 3, "sppf": 4, "attn": 5, "decode": 6, "nms": 7, "requant": 8}
DTYPES = {"f16": 0, "f32": 1, "i8": 2, "f8": 3, "x3": 4}
QUANT_DTYPES = ("i8", "f8")  # one-byte PTQ plans: int8 affine (torch.ao qconfig) and fp8 e4m3 (yolomi/quant.py)
BK = 64  # conv K is padded to the kernel K step (csrc/ym_conv.hip KSTEP)

# The 32 header and 32 op-record slots by name: the members of PlanHeader / OpRec in csrc/ym_plan.h, in blob order
HDR_FIELDS = ("magic", "version", "dtype", "task", "nc", "nm", "reg_max", "nl", "stride0", "stride1", "stride2", "nbuf",
              "nop", "wbytes_lo", "wbytes_hi", "input_buf", "anchor_buf", "proto_buf", "no", "scale", "kpt_k",
              "kpt_ndim", "kpt_off", "cls_pad") + tuple(f"rsv{i}" for i in range(24, 32))
OP_FIELDS = ("kind", "k", "s", "cin", "n", "act", "src0", "src0_coff", "c0", "up0", "src1", "src1_coff", "c1", "dst",
             "dst_coff", "level", "shuffle", "res", "res_coff", "w_off", "b_off", "kpad", "q_off", "sasw_off",
             "biasi_off", "w2_off", "b2_off", "n2", "act2", "kpad2", "k2", "mid")
# records: named access (r.kpad), tuple indexing (r[21]); slots not given are 0
Header = namedtuple("Header", HDR_FIELDS, defaults=(0,) * 32)
OpRecord = namedtuple("OpRecord", OP_FIELDS, defaults=(0,) * 32)


def fuse_conv_bn(w: np.ndarray, gamma, beta, mean, var, eps=1e-3):
    """ultralytics.utils.torch_utils.fuse_conv_and_bn in fp32 (bit-identical to the torch CPU path)."""
    f = np.float32
    w = w.astype(f)
    scale = gamma.astype(f) / np.sqrt(f(eps) + var.astype(f))
    wf = (scale.reshape(-1, *([1] * (w.ndim - 1))) * w).astype(f)
    bf = (beta.astype(f) - (gamma.astype(f) * mean.astype(f)) / np.sqrt(var.astype(f) + f(eps))).astype(f)
    return wf, bf


class _WeightArena:
    def __init__(self):
        self.chunks: List[bytes] = []
        self.size = 0

    def add(self, arr: np.ndarray) -> int:
        off = self.size
        b = np.ascontiguousarray(arr).tobytes()
        pad = (-len(b)) % 256
        self.chunks.append(b + b"\0" * pad)
        self.size += len(b) + pad
        return off

    def bytes(self) -> bytes:
        return b"".join(self.chunks)


def _conv_weights(a: dict, sd: Dict[str, np.ndarray]):
    if a.get("wkeys"):  # sibling convs on one input merged into one GEMM (arch.py C3k): output channels concatenated
        parts = [_conv_weights(dict(a, wkeys=None, wkey=k), sd) for k in a["wkeys"]]
        return np.concatenate([w for w, _ in parts]), np.concatenate([b for _, b in parts])
    key = a["wkey"]
    if a.get("convT"):
        wt = sd[key + ".weight"].astype(np.float32)  # (in, out, 2, 2)
        cin, cout = wt.shape[0], wt.shape[1]
        # GEMM column n = (dy*2 + dx)*cout + o  ←  wt[c, o, dy, dx]
        wg = np.transpose(wt, (2, 3, 1, 0)).reshape(4 * cout, cin)
        bg = np.tile(sd[key + ".bias"].astype(np.float32), 4)
        return wg[:, None, None, :], bg  # (N, 1, 1, cin)
    if a["bn"]:
        w, b = fuse_conv_bn(sd[key + ".conv.weight"], sd[key + ".bn.weight"], sd[key + ".bn.bias"],
                            sd[key + ".bn.running_mean"], sd[key + ".bn.running_var"])
    else:
        w, b = sd[key + ".weight"].astype(np.float32), sd[key + ".bias"].astype(np.float32)
    return np.transpose(w, (0, 2, 3, 1)), b  # (cout, k, k, cin) = NHWC-K order


def _dw_weights(key: str, sd):
    w, b = fuse_conv_bn(sd[key + ".conv.weight"], sd[key + ".bn.weight"], sd[key + ".bn.bias"],
                        sd[key + ".bn.running_mean"], sd[key + ".bn.running_var"])
    C = w.shape[0]
    return np.ascontiguousarray(w.reshape(C, 9).T).astype(np.float32), b  # [9][C]


def _pad_channels(w: np.ndarray, b: np.ndarray, N: int, cin: int):
    """(N', k, k, cin') weights and (N',) bias → (N, k, k, cin), (N,): zero rows / input columns / bias for the pad
    channels of a pose head (GraphBuilder.Detect).  A zero-bias pad row of an activated conv outputs SiLU(0) = 0."""
    n0, c0 = w.shape[0], w.shape[3]
    if (n0, c0) == (N, cin):
        return w, b
    assert n0 <= N and c0 <= cin, (w.shape, N, cin)
    wp = np.zeros((N,) + w.shape[1:3] + (cin,), w.dtype)
    wp[:n0, :, :, :c0] = w
    bp = np.zeros(N, b.dtype)
    bp[:n0] = b
    return wp, bp


X3_WEXP_MAX = 64  # |s| the runtime accepts for an x3 weight scale 2^s (csrc/ym_runtime.cpp conv_args)
X3_WMAX_LOG2 = 14  # x3 weight scaling: max |w|·2^s in (2^13, 2^14] (fp16 max 65504; csrc/ym_common.h ConvArgs::wsc)


def x3_weight_exp(w: np.ndarray) -> int:
    """Power-of-two exponent s of an x3 weight matrix: stored as w·2^s so that the fp16 lo part of the split
    (lo = fp16(w·2^s - hi)) stays normal for every weight above 2^-17 of the matrix's max — unscaled, the typical
    folded weight (~0.03) sits where lo is subnormal and keeps ~1e-6 relative precision (tools/x3_emulate.py).
    The kernels multiply the accumulator by 2^-s in the epilogue (exact)."""
    m = float(np.abs(w).max()) if w.size else 0.0
    if not np.isfinite(m):
        raise ValueError("non-finite conv weight")
    if m == 0.0:
        return 0
    # clamped to the range ym_load_weights accepts (conv_args: |s| <= X3_WEXP_MAX): a nearly pruned matrix (max |w|
    # below 2^-50) keeps s = 64 and with it subnormal lo parts, instead of a blob the loader rejects
    return int(min(max(X3_WMAX_LOG2 - np.ceil(np.log2(m)), -X3_WEXP_MAX), X3_WEXP_MAX))


def x3_pair_rows(w: np.ndarray, s: int) -> np.ndarray:
    """(N, K) fp32 weights → [N][2K] fp16 pair-chunk rows of w·2^s: every 8-element K chunk as [hi x8 | lo x8]."""
    N, K = w.shape
    wr = (w.astype(np.float32).reshape(N, K // 8, 8) * np.float32(2.0 ** s)).astype(np.float32)
    hi = wr.astype(np.float16)
    lo = (wr - hi.astype(np.float32)).astype(np.float16)
    return np.stack([hi, lo], axis=2).reshape(N, 2 * K)


def _qrec(inv_sc, zc, qlo, qhi, mode, post, inv_so=1.0, zo=0, s_r=0.0, z_r=0, s_in=0.0, z_in=0, inv_s_in=0.0) -> bytes:
    """csrc/ym_common.h `QRec` (1088 bytes)."""
    head = struct.pack("<fiiiifififif4i", inv_sc, int(zc), int(qlo), int(qhi), int(mode), inv_so, int(zo), s_r,
                       int(z_r), s_in, int(z_in), inv_s_in, 0, 0, 0, 0)
    return head + np.asarray(post, np.float32).tobytes()


def fuse_default(dtype: str):
    """GraphBuilder `fuse` of a plan unless YM_FUSE=0: f16 plans fuse conv pairs (GraphBuilder.fuse_pairs) and merge
    C3k's cv1 ‖ cv2; x3 plans merge and fuse the pairs with a 1x1 successor ("x3": GraphBuilder)."""
    import os
    if os.environ.get("YM_FUSE", "1") == "0":
        return False
    return {"f16": True, "x3": "x3"}.get(dtype, False)


def check_state_dict(g: GraphBuilder, sd: Dict[str, np.ndarray]) -> None:
    """Every parameter the plan reads must exist with exactly the shape the graph declares: a checkpoint of another
    scale, task or class count is rejected here instead of being packed with the wrong K pitch / channel count."""
    for p in g.params:
        if p.kind in ("count", "dfl"):
            continue
        if p.name not in sd:
            raise ValueError(f"state dict has no {p.name!r} (plan yolo11{g.scale} {g.task}, nc={g.nc})")
        shape = tuple(np.shape(sd[p.name]))
        if shape != tuple(p.shape):
            raise ValueError(f"{p.name}: checkpoint shape {shape} != plan shape {tuple(p.shape)} "
                             f"(plan yolo11{g.scale} {g.task}, nc={g.nc}: scale/task/class-count mismatch)")


def pack_model(scale: str, task: str, sd: Dict[str, np.ndarray], dtype: str = "f16", qparams: Dict = None) -> bytes:
    g = GraphBuilder(scale, task, quant=dtype in QUANT_DTYPES, fuse=fuse_default(dtype))
    return pack_graph(g, sd, dtype, qparams)


def pack_graph(g: GraphBuilder, sd: Dict[str, np.ndarray], dtype: str = "f16", qparams: Dict = None) -> bytes:
    if dtype not in DTYPES:
        raise ValueError(f"dtype {dtype!r} not in {list(DTYPES)}")
    quant = dtype in QUANT_DTYPES
    f8 = dtype == "f8"
    if quant != bool(g.quant):
        raise ValueError("int8/fp8 blobs need GraphBuilder(quant=True), float blobs quant=False")
    pose = g.task == "pose"
    if pose and quant:
        raise ValueError(f"pose plans are x3 / f16 / f32: there is no PTQ pose plan (dtype {dtype!r})")
    if pose and not g.pad_head:
        raise ValueError("GraphBuilder(pad_head=False) is not a plan the GPU runs")
    check_state_dict(g, sd)
    if quant:
        from .quant import (BACKENDS, inv32, post_table, post_table_fp8, qrange, quantize_weight,
                            quantize_weight_fp8)
        if not qparams or qparams.get("backend") not in BACKENDS or (qparams["backend"] == "fp8") != f8:
            raise ValueError(f"dtype {dtype!r} needs calibrated qparams (yolomi.quant.calibrate) of backend "
                             f"{'fp8' if f8 else 'qnnpack / fbgemm'}")
        if f8 and g.task != "detect":
            raise ValueError("the fp8 plan covers detect models")
        per_channel = BACKENDS[qparams["backend"]][1]
        qlo, qhi = qrange(qparams["backend"])

        def qweight(w, pc):  # (codes as int8 bytes, fp32 scale per output channel)
            if f8:
                c, sw_ = quantize_weight_fp8(w)
                return c.view(np.int8), sw_
            return quantize_weight(w, pc)

        def post(s_, z_, act):
            return post_table_fp8(s_, act) if f8 else post_table(s_, z_, act)

        def qp(key):
            if key not in qparams:
                raise ValueError(f"qparams has no entry {key!r}")
            s_, z_ = qparams[key]
            return float(np.float32(s_)), int(z_)
    np_dt = np.float16 if dtype == "f16" else np.float32
    arena = _WeightArena()
    op_recs: List[OpRecord] = []
    names: List[bytes] = []
    for op in g.ops:
        a = op.args
        r = {"kind": OP_IDS[op.kind]}  # OP_FIELDS slots of this op
        if op.kind == "conv":
            w, b = _conv_weights(a, sd)  # (N, k, k, cin)
            if pose:
                w, b = _pad_channels(w, b, a["c2"], a["c1"])
            src0 = a["src0"]
            C0 = src0.C
            stem = src0.buf is g.input
            if quant:
                w, sw = qweight(w, per_channel and not a.get("convT"))  # int8 / e4m3 (N, k, k, cin), fp32 (N,)
            if stem:  # stem: RGB padded to 8 channels
                pad = 8 - C0
                w = np.concatenate([w, np.zeros(w.shape[:3] + (pad,), w.dtype)], axis=3)
                C0 = 8
            elif quant and C0 % 16:  # int8 K chunks are 16 channels of one tap
                pad = 16 - C0 % 16
                w = np.concatenate([w, np.zeros(w.shape[:3] + (pad,), w.dtype)], axis=3)
                C0 += pad
            N = w.shape[0]
            K = w.shape[1] * w.shape[2] * w.shape[3]
            bk = 2 * BK if dtype == "i8" else BK  # int8: whole 128-byte K stages for the LDS-DMA kernels' Q8 mode
            Kpad = (K + bk - 1) // bk * bk
            wp = np.zeros((N, Kpad), np.int8 if quant else np.float32)
            wp[:, :K] = w.reshape(N, K)
            if dtype == "x3" and not stem:  # pair-chunk rows of W·2^s: every 8-channel K chunk as [hi x8 | lo x8]
                ws = x3_weight_exp(w)
                K2 = 2 * K
                Kpad = (K2 + BK - 1) // BK * BK  # the 64-deep storage step (32 logical K)
                wp = np.zeros((N, Kpad), np.float16)
                wp[:, :K2] = x3_pair_rows(w.reshape(N, K), ws)
                r["q_off"] = ws  # (x3 plans: the slot holds the exponent)
            src1 = a["src1"]
            C1 = src1.C if src1 is not None else 0
            dst, res = a["dst"], a["res"]
            r.update(k=a["k"], s=a["s"], cin=C0 + C1, n=N, act=int(bool(a["act"])))
            r.update(src0=src0.buf.id, src0_coff=src0.coff, c0=C0, up0=int(bool(a["up0"])))
            r.update(src1=src1.buf.id if src1 is not None else -1, src1_coff=src1.coff if src1 is not None else 0, c1=C1)
            r.update(dst=dst.buf.id, dst_coff=dst.coff, level=a["anchor_level"], shuffle=int(bool(a["shuffle2x2"])))
            r.update(res=res.buf.id if res is not None else -1, res_coff=res.coff if res is not None else 0)
            r["w_off"] = arena.add(wp if quant or wp.dtype == np.float16 else wp.astype(np_dt))  # (x3 stem: fp32)
            r["b_off"] = arena.add(b.astype(np.float32))
            r["kpad"] = Kpad
            if a.get("dw") is not None:  # fused depthwise (GraphBuilder.fuse_dw): 1 + offset of [9][C] ‖ bias [C]
                if dtype not in ("f16", "x3"):
                    raise ValueError(f"op {op.name}: fused depthwise convs are f16 / x3 only")
                w9, bdw = _dw_weights(a["dw"]["wkey"], sd)
                assert w9.shape == (9, C0)
                r["biasi_off"] = 1 + arena.add(
                    np.concatenate([w9.reshape(-1), np.asarray(bdw, np.float32)]).astype(np.float32))
            pair = a.get("pair")
            if pair is not None:  # fused successor (GraphBuilder.fuse_pairs): W2 [N2][Kpad2], K = (ky, kx, this conv's N)
                if dtype not in ("f16", "x3"):
                    raise ValueError(f"op {op.name}: fused conv pairs are f16 / x3 only")
                w2, b2 = _conv_weights(pair, sd)  # (N2, k2, k2, N)
                if pose:
                    w2, b2 = _pad_channels(w2, b2, pair["c2"], pair["c1"])
                N2, k2 = w2.shape[0], pair["k"]
                assert w2.shape[1:] == (k2, k2, N)
                K2 = k2 * k2 * N
                if dtype == "x3":  # pair-chunk rows of W2·2^s2 like W (storage K 2·K2, padded to 64)
                    ws2 = x3_weight_exp(w2)
                    Kpad2 = (2 * K2 + BK - 1) // BK * BK
                    w2h = np.zeros((N2, Kpad2), np.float16)
                    w2h[:, :2 * K2] = x3_pair_rows(w2.reshape(N2, K2), ws2)
                    r["sasw_off"] = ws2  # (x3 plans: W2's exponent)
                else:
                    Kpad2 = (K2 + BK - 1) // BK * BK
                    w2p = np.zeros((N2, Kpad2), np.float32)
                    w2p[:, :K2] = w2.reshape(N2, K2)
                    w2h = w2p.astype(np.float16)
                r.update(w2_off=arena.add(w2h), b2_off=arena.add(b2.astype(np.float32)))
                r.update(n2=N2, act2=int(bool(pair["act"])), kpad2=Kpad2, k2=k2, mid=pair["mid"].buf.id)
            if quant:
                s_in, z_in = qp("act:input" if stem else src0.buf.qkey)
                so, zo = qp("out:" + a["wkey"])
                d = dst.buf
                mode = 2 if d.f32 else (1 if d.qkind == "out" else 0)
                s_b, z_b = (1.0, 0) if mode else qp(d.qkey)
                s_r, z_r = qp(res.buf.qkey) if res is not None else (0.0, 0)
                rec = _qrec(inv32(so), zo, qlo, qhi, mode, post(so, zo, bool(a["act"])), inv32(s_b), z_b, s_r,
                            z_r, s_in, z_in, inv32(s_in))
                biasi = np.zeros(N, np.int64) if (stem or f8) else (128 - z_in) * wp.astype(np.int64).sum(1)
                assert np.abs(biasi).max() < 2 ** 31
                r["q_off"] = arena.add(np.frombuffer(rec, np.uint8))
                r["sasw_off"] = arena.add((np.float32(s_in) * sw).astype(np.float32))
                r["biasi_off"] = arena.add(biasi.astype(np.int32))
        elif op.kind == "dwconv":
            w9, b = _dw_weights(a["wkey"], sd)
            r.update(cin=a["C"], act=int(bool(a["act"])))
            r.update(src0=a["src"].buf.id, src0_coff=a["src"].coff, dst=a["dst"].buf.id, dst_coff=a["dst"].coff)
            if quant:
                wq, sw = qweight(np.ascontiguousarray(w9.T), per_channel)  # (C, 9): per output channel
                s_in, z_in = qp(a["src"].buf.qkey)
                so, zo = qp("out:" + a["wkey"])
                s_b, z_b = qp(a["dst"].buf.qkey)
                rec = _qrec(inv32(so), zo, qlo, qhi, 0, post(so, zo, bool(a["act"])), inv32(s_b), z_b,
                            s_in=s_in, z_in=z_in)
                r.update(w_off=arena.add(np.ascontiguousarray(wq.T)), b_off=arena.add(b))
                r["q_off"] = arena.add(np.frombuffer(rec, np.uint8))
                r["sasw_off"] = arena.add((np.float32(s_in) * sw).astype(np.float32))
            else:
                r.update(w_off=arena.add(w9), b_off=arena.add(b))
        elif op.kind == "sppf":  # pooled in place: the dst slot names the buffer, the src0_coff slot y0's offset in it
            r.update(cin=a["C"], src0_coff=a["src"].coff, dst=a["dst"].id)
        elif op.kind == "attn":  # heads, key dim and value dim per head in the n, act and up0 slots
            w9, b = _dw_weights(a["wkey"], sd)
            r.update(cin=a["C"], n=a["nh"], act=a["kd"], up0=a["hd"])
            r.update(src0=a["qkv"].buf.id, src0_coff=a["qkv"].coff, dst=a["dst"].buf.id, dst_coff=a["dst"].coff)
            # the kpad slot: the fp32 bits of the attention scale
            r["kpad"] = struct.unpack("<i", struct.pack("<f", float(np.float32(a["kd"] ** -0.5))))[0]
            if quant:
                wq, sw = qweight(np.ascontiguousarray(w9.T), per_channel)
                s_in, z_in = qp(a["qkv"].buf.qkey)
                so, zo = qp("out:" + a["wkey"])
                s_b, z_b = qp(a["dst"].buf.qkey)
                rec = _qrec(inv32(so), zo, qlo, qhi, 0, post(so, zo, False), inv32(s_b), z_b, s_in=s_in,
                            z_in=z_in)
                r.update(w_off=arena.add(np.ascontiguousarray(wq.T)), b_off=arena.add(b))
                r["q_off"] = arena.add(np.frombuffer(rec, np.uint8))
                r["sasw_off"] = arena.add((np.float32(s_in) * sw).astype(np.float32))
            else:
                r.update(w_off=arena.add(w9), b_off=arena.add(b))
        elif op.kind == "requant":
            src, dst = a["src"], a["dst"]
            r.update(cin=dst.C, src0=src.buf.id, src0_coff=src.coff, up0=int(bool(a["up"])))
            r.update(dst=dst.buf.id, dst_coff=dst.coff)
            s_in, z_in = qp(src.buf.qkey)
            s_b, z_b = qp(dst.buf.qkey)
            rec = _qrec(1.0, 0, qlo, qhi, 0, np.zeros(256, np.float32), inv32(s_b), z_b, s_in=s_in, z_in=z_in)
            r["q_off"] = arena.add(np.frombuffer(rec, np.uint8))
        op_recs.append(OpRecord(**r))
        nm = op.name.encode()[:47]
        names.append(nm + b"\0" * (48 - len(nm)))

    wbytes = arena.bytes()
    assert len(STRIDES) == 3  # the header's stride slots
    hdr = Header(
        magic=MAGIC, version=VERSION, dtype=DTYPES[dtype], task={"detect": 0, "segment": 1, "pose": 2}[g.task],
        nc=g.nc, nm=g.nm, reg_max=REG_MAX, nl=len(STRIDES), stride0=STRIDES[0], stride1=STRIDES[1], stride2=STRIDES[2],
        nbuf=len(g.buffers), nop=len(g.ops), wbytes_lo=len(wbytes) & 0xFFFFFFFF, wbytes_hi=len(wbytes) >> 32,
        input_buf=g.input.id, anchor_buf=g.anchor_buf.id, proto_buf=g.proto_buf.id if g.task == "segment" else -1,
        no=g.no, scale=ord(g.scale))  # (scale: checked against ym_model_desc.scale)
    if pose:  # nm = nk_pad, the extras NMS carries
        hdr = hdr._replace(kpt_k=g.kpt_shape[0], kpt_ndim=g.kpt_shape[1], kpt_off=g.kpt_off, cls_pad=g.no - 4 * REG_MAX)
    head = struct.pack("<32i", *hdr)
    bufs = b"".join(struct.pack("<8i", b.Cs or b.C, b.f, int(b.f32), 0, 0, 0, 0, 0) for b in g.buffers)
    ops = b"".join(struct.pack("<32i", *rr) for rr in op_recs)
    meta = head + bufs + ops + b"".join(names)
    meta += b"\0" * ((-len(meta)) % 256)
    return meta + wbytes


def field_offset(header: Header, field: str, op: int = None) -> int:
    """Byte offset in the blob of a header slot (op None) or of a slot of op record `op`."""
    if op is None:
        return 4 * HDR_FIELDS.index(field)
    return 128 + 32 * header.nbuf + 128 * op + 4 * OP_FIELDS.index(field)


def unpack_blob(blob: bytes):
    """(header, buffers, ops, names, woff) of a packed blob: a Header, the (C, f, f32) of every buffer, an OpRecord and
    a name per op, and the byte offset of the weight section (a record's *_off slots count from there)."""
    h = Header(*struct.unpack_from("<32i", blob, 0))
    o_buf, o_op = 128, 128 + 32 * h.nbuf
    o_name = o_op + 128 * h.nop
    buffers = [struct.unpack_from("<3i", blob, o_buf + 32 * i) for i in range(h.nbuf)]
    ops = [OpRecord(*struct.unpack_from("<32i", blob, o_op + 128 * i)) for i in range(h.nop)]
    names = [blob[o_name + 48 * i: o_name + 48 * (i + 1)].split(b"\0")[0].decode() for i in range(h.nop)]
    return h, buffers, ops, names, -(-(o_name + 48 * h.nop) // 256) * 256

