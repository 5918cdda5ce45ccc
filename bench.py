#!/usr/bin/env python3
"""Headline benchmark: images/s of batched YOLO11 inference at 640x640 on MI355X (+ mAP50-95 vs the CPU oracle).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--model s] [--batch 8] [--size 640] [--dtype f16]
                    [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nproc-per-node N --master-addr 127.0.0.1 bench.py --gpus N

Default workload = BASELINE.json config 3, the one the 1/2/4/8-GPU metric is quoted on: yolo11s detect, 640x640,
batch 8 per GPU, on the x3 plan — fp16 MFMAs on split operands with fp32-equivalent storage, the plan whose detections
meet the north-star bar (1e-3 px absolute on coordinates, 1e-3 on scores, class exact; the plain f16 plan is ~0.6 px
and 3e-3 off), reported under `--full` with its parity against the CPU oracle on the timed batch (`parity`)
and beside the f16 throughput plan measured in the same run (`f16_throughput_plan`).  (`--model n` gives config 2, `--dtype i8`
config 4, `--model s --task segment --batch 4` config 5.)

One step = one `YOLO11Model.predict(batch)` call (the reference's timed unit: core/model.py:277-282,
benchmarks/speed_benchmark.py:330-335) over synthetic U[0,1) 640x640 images already resident in HBM: input /255
rule → forward (one HIP-graph replay) → decode → NMS → per-image Results (one D2H sync).
Multi-GPU: one process per GPU (`--gpus N` without a launcher spawns the N ranks itself through
torch.distributed.run, as a child process); rank 0 packs the weights once and broadcasts the blob over RCCL (xGMI)
(torch.distributed "nccl" broadcast of one uint8 tensor, yolomi.dist.broadcast_blob; `--cabi-bcast`: through the
C-ABI, yolomi.dist.rccl_broadcast_model → ym_broadcast_weights); each rank runs its own batch shard ("weak" scaling,
8 images per GPU).  LoadTensor's /255 rule reads the batch every step at every N (the same per-step work): at N = 1
the forward's own input_stats kernel takes the batch max; at N > 1 each rank's shard max (ym_input_max) is
all-reduced (MAX) over the ranks every step and handed to the forward (yolomi.dist.enable_global_rule), so the
decision is the global batch's.

Rank 0 prints ONE JSON line.  A plain run does what the headline figure needs and no more: set-up, warm-up, the timed
steps, the result line.  `--full` adds the rest, each in runs of its own after the timed loop: `device_images_per_s`
(back-to-back graph replays, no host sync), `roofline` (conv implicit-GEMM kernels, live HIP-event timing), `kernels`
(per-kind device time and achieved HBM GB/s of the non-conv kernels), `f16_throughput_plan` (x3 runs), `cpu_baseline`
(the oracle on host cores, N=1 only, B=1 and B=8 samples), `accuracy` (mAP50-95 of GPU detections against oracle
detections as pseudo ground truth, N=1 only) and `parity`; `--no-roofline`, `--no-f16` and `--no-cpu` drop parts of it.

`--dump-outputs DIR` writes what the last timed predict() returned, per image g of the global batch (rank * batch + b):
`DIR/boxes_<g>.npy`, float32 (n, 6) rows [x1, y1, x2, y2, conf, cls], and for Segment `DIR/masks_<g>.npy`, float32
(n, k): the masks at k pixel positions drawn by a generator seeded with g (every pixel while the dump stays within its
size budget, DUMP_BUDGET_BYTES for the whole batch).  The inputs are functions of the arguments alone, so two builds
run with the same arguments can be compared file for file.
"""
from __future__ import annotations

import argparse
import json
import os
import socket
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "yolo-infer_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

METRIC = "images/sec @640×640 (1/2/4/8 MI355X) + mAP50-95 vs CPU ref"
# dense MFMA peaks (MI355X_MICROARCH.md; i8 = TOP/s; f8 = 2.5 PF: the fp8 plan runs v_mfma_f32_32x32x16_fp8_fp8, the
# non-scaled fp8 form, at the bf16/f16 rate — the 5 PF figure is the block-scaled f8f6f4 form's)
# x3 (fp32 storage, split-f16 MFMA): the algorithmic FLOPs against the f16 peak, although each K chunk issues three
# f16 MFMAs (so its MFMA-issue ceiling is a third of that)
PEAK_TFLOPS = {"f16": 2500.0, "f32": 157.3, "i8": 5000.0, "f8": 2500.0, "x3": 2500.0}
ACT_BYTES = {"f16": 2, "f32": 4, "i8": 1, "f8": 1, "x3": 4}
PEAK_HBM_GBS = 8000.0
EXACT_TOL_XY, EXACT_TOL_S = 5e-4, 5e-5  # the GPU's own distance from the float64 answer (tests/test_gpu_x3.py)
# LoadTensor's /255 rule inside the timed step, by N (verdict r5 item 7: the same per-step work at every N)
BATCH_RULE = {False: "per step: the forward's input_stats kernel reads the batch for its max",
              True: "per step: the shard max (ym_input_max, one read of the shard) all-reduced MAX over the ranks, "
                    "handed to the forward"}


def synthetic_batch(B, S, seed, device):
    from yolomi.synth import uniform
    x = uniform(seed, B * 3 * S * S).astype(np.float32).reshape(B, 3, S, S)
    return torch.from_numpy(x).to(device)


def pmc_traffic(workload):
    """HBM-side bytes per forward of the conv family from the newest committed PMC summary of this workload
    (profiles/<round>_pmc.json, produced by tools/rocprof_summary.py from separate rocprofv3 --pmc passes)."""
    import glob
    best = None
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json"))):
        try:
            j = json.load(open(p))
        except (OSError, ValueError):
            continue
        # the summary names the network/batch/dtype; the bench line appends how it was driven (", predict() loop")
        if j.get("workload") == workload.split(",")[0] and "conv" in j.get("families", {}):
            best = (p, j)
    if best is None:
        return None, None
    return best[1]["families"]["conv"]["bytes_corrected"], os.path.relpath(best[0], ROOT)


PROFILE_ROUND = "r06"  # the roofline cites only profiles of this round's tree (verdict r5 item 4)


def _newest_profile(pattern, workload):
    """The newest committed profiles/<PROFILE_ROUND><pattern> file whose "workload" is this bench workload (without
    ", predict() loop"); (path relative to the repo, parsed json) or (None, None)."""
    import glob
    best = (None, None)
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", PROFILE_ROUND + pattern))):
        try:
            j = json.load(open(p))
        except (OSError, ValueError):
            continue
        if isinstance(j, dict) and j.get("workload") == workload.split(",")[0]:
            best = (os.path.relpath(p, ROOT), j)
    return best


def concurrency_view(flops, dtype, workload):
    """The conv family under the real schedule (verdict r2: the isolated replay hides the stretching concurrent
    branches cause): FLOPs per forward ÷ the rocprof conv time per forward of the same bench command (committed
    profiles/*_summary.json), and the time-weighted MFMA busy of the conv launches from the per-op SQ table
    (profiles/*_ops.json: SQ_VALU_MFMA_BUSY_CYCLES / (GRBM cycles x 1024 SIMDs), weighted by each op's time)."""
    out = {}
    src, summ = _newest_profile("*_summary.json", workload)
    if summ and "conv" in summ.get("families", {}):
        ms = summ["families"]["conv"]["ms_per_forward"]
        ach = flops / (ms * 1e-3) / 1e12
        out.update(frac_rocprof=round(ach / PEAK_TFLOPS[dtype], 4), achieved_rocprof=round(ach, 2),
                   conv_ms_per_forward_rocprof=ms, rocprof_source=src)
    src, ops = _newest_profile("*_ops.json", workload)
    if ops:
        conv = [r for r in ops["ops"] if r.get("kind") == "conv" and r.get("us")]
        t = sum(r["us"] for r in conv)
        if t > 0:
            out.update(mfma_busy=round(sum(r["mfma_busy"] * r["us"] for r in conv) / t, 4), mfma_busy_source=src)
    return out


def conv_roofline(model, x, dtype, workload, reps=20):
    """Live per-op device times on the launch stream → conv-family roofline.

    Each conv launch of the forward is captured as a HIP graph of `reps` back-to-back launches on the real
    activation buffers and bracketed by one HIP event pair (ym_profile_replay): per-launch device time without the
    per-op marker packets an eager event pair would add.  `achieved` = Σ algorithmic FLOPs of the forward's conv
    launches ÷ Σ their per-launch times (per-unit figures: DESIGN.md §4)."""
    eng = model.model.engine
    B, _, H, W = x.shape
    Bl = eng.lane_batch(B)  # every kernel of a lane sees Bl images: time and count one lane's launches
    x = x[:Bl]
    costs = eng.graph.op_costs(Bl, H, W, ACT_BYTES[dtype])
    times = np.array(eng.profile_replay(x, reps=reps))
    eng.run(x, lanes=1)  # restore the buffers the replay clobbered
    kinds = [op.kind for op in eng.graph.ops]
    conv = [i for i, k in enumerate(kinds) if k == "conv"]
    t_conv = float(times[conv].sum()) * 1e-3
    fl = float(sum(costs[i][0] for i in conv))
    by = float(sum(costs[i][1] for i in conv))
    per_kind = {}
    for k, t in zip(kinds, times):
        if t >= 0:
            per_kind[k] = per_kind.get(k, 0.0) + float(t)
    top = sorted(((float(times[i]), eng.graph.ops[i].name, costs[i][0] / max(times[i] * 1e-3, 1e-12) / 1e12)
                  for i in conv), reverse=True)[:8]
    ach = fl / t_conv / 1e12
    # each launch priced at whichever roof bounds it (most YOLO11 convs at B = 8 are HBM-side, not MFMA, bound)
    floor_s = sum(max(costs[i][0] / (PEAK_TFLOPS[dtype] * 1e12), costs[i][1] / (PEAK_HBM_GBS * 1e9)) for i in conv)
    traffic, tsrc = pmc_traffic(workload)
    # in context, live: one eager forward with a HIP event pair around every op on the launch stream (ym_profile,
    # serial order: every kernel sees the caches the previous one left), median of 5
    ev = np.median(np.array([eng.profile(x) for _ in range(5)]), axis=0)
    t_eager = float(ev[conv].sum()) * 1e-3
    ach_eager = fl / t_eager / 1e12
    ctx = concurrency_view(fl, dtype, workload)
    # frac: the in-context figure of the bench command under rocprofv3 (4 branch streams, concurrent kernels stretch
    # each other) when this round's profile of it is committed, else the live eager in-forward one
    ach_main = ctx.get("achieved_rocprof", ach_eager)
    return {
        "bound": "mfma", "achieved": round(ach_main, 2), "peak": PEAK_TFLOPS[dtype], "unit": "TFLOP/s",
        "frac": round(ach_main / PEAK_TFLOPS[dtype], 4), "traffic": traffic,
        "frac_basis": ("rocprofv3 in-context conv time per forward of this bench command (%s)" % ctx["rocprof_source"]
                       if "achieved_rocprof" in ctx else
                       "live: eager forward, HIP event pair per op on the launch stream (ym_profile), median of 5"),
        "frac_live_eager_forward": round(ach_eager / PEAK_TFLOPS[dtype], 4),
        "achieved_live_eager_forward": round(ach_eager, 2),
        "frac_live_isolated_replay": round(ach / PEAK_TFLOPS[dtype], 4), "achieved_live_isolated_replay": round(ach, 2),
        **({"frac_of_x3_issue_ceiling": round(ach_main / (PEAK_TFLOPS[dtype] / 3), 4),
            "x3_issue_ceiling_note": "x3 issues three f16 MFMAs per K chunk: its MFMA-issue ceiling is peak / 3"}
           if dtype == "x3" else {}),
        "traffic_note": (f"HBM-side bytes per forward of all conv launches (PMC FETCH_SIZE x2 + WRITE_SIZE, {tsrc}); "
                         f"algorithmic bytes per forward {int(by)}") if traffic else "no PMC summary for this workload",
        "kernel": "conv implicit GEMM (%s): all %d conv launches of one lane's forward (%d images), aggregated%s"
                  % ({"i8": "conv_i8 + conv_dma<Q8> (LDS-DMA), v_mfma_i32_32x32x32_i8",
                      "f8": "conv_i8<fp8>, v_mfma_f32_32x32x16_fp8_fp8 (accumulation restated in oracle/quant.py)",
                      "x3": "conv_dma (LDS-DMA ring) / conv_stream / conv_bneck / conv_dwpw on the x3 pair layout, "
                            "3x v_mfma_f32_32x32x16_f16 per K chunk"}.get(
                      dtype, "conv_stream/conv_small/conv_dma/conv_lds/conv_bneck/conv_halo/conv_igemm"), len(conv),
                     Bl, "; int8 ops counted as FLOPs" if dtype == "i8" else ""),
        "timing": f"isolated replay: HIP events around a graph of {reps} back-to-back launches per op, on the launch "
                  "stream; eager: an event pair per op of one serial forward; rocprof: the bench command's own trace",
        "launches": len(conv), "avg_launch_us": round(t_conv / len(conv) * 1e6, 2),
        "flops_per_forward": fl, "bytes_per_forward_algorithmic": by,
        "hbm_algorithmic_GBps": round(by / t_conv / 1e9, 1), "hbm_frac": round(by / t_conv / 1e9 / PEAK_HBM_GBS, 4),
        "per_launch_roofline_frac": round(floor_s / t_conv, 4),
        "per_launch_roofline_note": "sum over the conv launches of max(FLOPs / MFMA peak, algorithmic bytes / 8 TB/s) "
                                    "divided by the sum of their measured times",
        "ms_by_kind_replay": {k: round(v, 4) for k, v in per_kind.items()},
        "top_convs": [{"op": n, "ms": round(t, 4), "tflops": round(tf, 1)} for t, n, tf in top],
        **ctx,
    }


def pmc_family_bytes(workload):
    """Per-forward HBM-side bytes of every kernel family in the newest committed PMC summary of this workload."""
    import glob
    best = None
    for p in sorted(glob.glob(os.path.join(ROOT, "profiles", "*_pmc.json"))):
        try:
            j = json.load(open(p))
        except (OSError, ValueError):
            continue
        if j.get("workload") == workload.split(",")[0]:
            best = (p, j)
    if best is None:
        return {}, None
    return {k: v.get("bytes_corrected") for k, v in best[1].get("families", {}).items()}, os.path.relpath(best[0], ROOT)


# op kind (yolomi/arch.py) → the rocprof kernel family of tools/rocprof_summary.py
KIND_FAMILY = {"stem": "stem", "dwconv": "dwconv3x3", "sppf": "sppf", "attn": "attn_psa", "decode": "decode_anchors",
               "input": "input_stats", "nms": "nms_image"}


def kernel_table(model, x, dtype, workload):
    """Device time and achieved HBM GB/s of the non-conv kernel families of one forward (pointwise /
    pooling / decode kernels are judged against HBM, not MFMA).  Times: one eager forward with a HIP event pair
    around every op on the launch stream (ym_profile), the median of 5; bytes: algorithmic (each input element read
    once, each output written once, yolomi/arch.py op_costs) and, when a committed PMC summary of this workload
    exists, the measured HBM-side bytes."""
    eng = model.model.engine
    B, _, H, W = x.shape
    costs = eng.graph.op_costs(B, H, W, ACT_BYTES[dtype])
    runs = np.array([eng.profile(x) for _ in range(5)])
    t = np.median(runs, axis=0)
    pmc, src = pmc_family_bytes(workload)
    agg = {}
    for i, op in enumerate(eng.graph.ops):
        kind = "stem" if op.kind == "conv" and op.args["src0"].buf is eng.graph.input else op.kind
        if kind not in KIND_FAMILY:
            continue
        e = agg.setdefault(kind, {"launches": 0, "us": 0.0, "bytes": 0})
        e["launches"] += 1
        e["us"] += float(t[i]) * 1e3
        e["bytes"] += int(costs[i][1])
    out = {}
    for kind, e in agg.items():
        d = {"launches": e["launches"], "us_per_forward": round(e["us"], 2), "bytes_algorithmic": e["bytes"]}
        if e["bytes"] and e["us"] > 0:
            gbs = e["bytes"] / (e["us"] * 1e-6) / 1e9
            d.update(GBps_algorithmic=round(gbs, 1), hbm_frac=round(gbs / PEAK_HBM_GBS, 4))
        pb = pmc.get(KIND_FAMILY[kind])
        if pb and e["us"] > 0:
            d.update(bytes_pmc=int(pb), GBps_pmc=round(pb / (e["us"] * 1e-6) / 1e9, 1))
        out[kind] = d
    return {"timing": "eager forward, HIP event pair per op on the launch stream (ym_profile), median of 5",
            "peak_GBps": PEAK_HBM_GBS, "pmc_source": src, "by_kind": out}


def cpu_baseline(scale, task, x_gpu_dets, xs, seconds, qparams=None):
    """Oracle (torch CPU fp32, fused; or the int8 oracle of oracle/quant.py for an int8 run) timed on this host at
    B=1 and at B=8 (half the time budget each); also mAP of the GPU dets against the oracle's dets (and, for int8,
    against the float oracle's: the quantisation loss)."""
    from oracle.predict import OracleModel
    from oracle.quant import Int8OracleModel
    from yolomi.metrics import evaluate
    from yolomi.synth import synth_weights
    nthreads = int(os.environ.get("OMP_NUM_THREADS", 0)) or len(os.sched_getaffinity(0))
    torch.set_num_threads(nthreads)
    if qparams is not None:
        om = Int8OracleModel(scale, task, synth_weights(scale, task, 0), qparams)
    else:
        om = OracleModel(scale, task, synth_weights(scale, task, 0))
    rates = {}
    for B in (1, min(8, xs.shape[0])):
        xb = xs[:B].cpu()
        om.predict(xb)  # warm-up
        n, t0 = 0, time.perf_counter()
        while time.perf_counter() - t0 < seconds / 2:
            om.predict(xb)
            n += B
        dt = time.perf_counter() - t0
        rates[B] = (n, dt)
    ref = om.predict(xs.cpu())
    gts = [r["boxes"].numpy() for r in ref]
    exact = None if qparams is not None else [e.numpy() for e in om.predict_exact(xs.cpu())]
    m = evaluate(x_gpu_dets, gts)
    try:
        cpu_name = next((ln.split(":", 1)[1].strip() for ln in open("/proc/cpuinfo") if ln.startswith("model name")),
                        "unknown")
    except OSError:
        cpu_name = "unknown"
    fp8 = bool(qparams) and qparams.get("backend") == "fp8"
    what = ("fp8 oracle (oracle/quant.py backend fp8: e4m3 via torch.float8_e4m3fn, exact float64 convs)" if fp8 else
            "int8 oracle (oracle/quant.py: integer convs as exact float64 convs)" if qparams else "oracle")
    bmax = max(rates)
    n8, dt8 = rates[bmax]
    n1, dt1 = rates[1]
    base = {"value": round(n8 / dt8, 3), "unit": "images/s", "cores": nthreads, "kind": "port",
            "value_b1": round(n1 / dt1, 3),
            "sample": f"{what} predict yolo11{scale} {task} 640x640 U[0,1) on {cpu_name} (os.cpu_count="
                      f"{os.cpu_count()}): B={bmax}: {n8} images in {dt8:.1f}s (value); B=1: {n1} images in "
                      f"{dt1:.1f}s (value_b1)"}
    acc = {"map50_95": round(m["map"], 4), "map50": round(m["map50"], 4), "images": len(gts),
           "gt": (f"{'fp8' if fp8 else 'int8'} oracle (CPU) detections, same qparams, as pseudo ground truth" if qparams else
                  "oracle (CPU fp32) detections as pseudo ground truth"),
           "dets_gpu": int(sum(len(d) for d in x_gpu_dets)), "dets_oracle": int(sum(len(g) for g in gts))}
    if qparams is not None:  # quantisation loss: int8 GPU detections vs the float oracle's
        fl = OracleModel(scale, task, synth_weights(scale, task, 0)).predict(xs.cpu())
        mf = evaluate(x_gpu_dets, [r["boxes"].numpy() for r in fl])
        acc["vs_fp32_oracle"] = {"map50_95": round(mf["map"], 4), "map50": round(mf["map50"], 4)}
    if fp8:  # the oracle the fp8 plan is bit-exact against: the restated fp8 MFMA accumulation (slow: image 0 only)
        mm = Int8OracleModel(scale, task, synth_weights(scale, task, 0), qparams, accum="mfma")
        r0 = mm.predict(xs[:1].cpu())[0]["boxes"].numpy()
        m0 = evaluate(x_gpu_dets[:1], [r0])
        acc["vs_fp8_mfma_oracle_image0"] = {"map50_95": round(m0["map"], 4), "dets_oracle": int(len(r0)),
                                            "dets_gpu": int(len(x_gpu_dets[0])),
                                            "note": "oracle/quant.py accum='mfma' (the fp8 MFMA's accumulation restated); "
                                                    "map50_95 / gt above: the exact-sum fp8 oracle"}
    return base, acc, gts, exact


def parity(gpu_dets, gts, conf=0.25, iou=0.7, tol_xy=1e-3, tol_s=1e-3, exact=None):
    """SURVEY §8(c) matching of the timed batch's GPU detections against the oracle's (tests/matching.py) at the
    north-star bar (BASELINE.json): 1e-3 px absolute on coordinates, 1e-3 on scores, class exact, every detection
    matched or exempt.  `exact`: the same graph in float64 (oracle predict_exact) — then also the GPU's and the fp32
    oracle's own distances from it, and the bar beyond the oracle's own rounding (tests/matching.py ref_f64_slack)."""
    from tests.matching import MatchReport, match_image, ref_f64_slack
    rep, rex = MatchReport(), MatchReport()
    dxy, ds, slack_ok = [], [], []
    for b, (g, r) in enumerate(zip(gpu_dets, gts)):
        before = len(rep.pairs)
        match_image(r, g, conf, iou, 10.0, 1.0, rep=rep)  # match loosely, then grade the deltas
        sl = ref_f64_slack(r, exact[b], tol_xy) if exact is not None else None
        for i, j in rep.pairs[before:]:
            dxy.append(float(np.abs(r[i, :4] - g[j, :4]).max()))
            ds.append(float(abs(r[i, 4] - g[j, 4])))
            if sl is not None:
                slack_ok.append(dxy[-1] <= sl[i])
        if exact is not None:  # the same protocol against the float64 evaluation, at the exact bar
            match_image(np.asarray(exact[b], np.float64), np.asarray(g, np.float64), conf, iou, EXACT_TOL_XY,
                        EXACT_TOL_S, rep=rex)
    ok = rep.ok and (not dxy or (max(dxy) <= tol_xy and max(ds) <= tol_s))
    out = {"tolerance": f"|dxy| <= {tol_xy:g} px, |dscore| <= {tol_s:g}, class exact, all matched or exempt "
                        "(BASELINE north star, SURVEY 8c)",
           "meets_tolerance": bool(ok), "matched": rep.matched, "exempt": rep.exempt,
           "unmatched_oracle": rep.unmatched_ref, "unmatched_gpu": rep.unmatched_build,
           "max_dxy_px": round(max(dxy), 6) if dxy else None, "max_dscore": round(max(ds), 7) if ds else None,
           "within_tolerance_frac": round(float(np.mean([(a <= tol_xy and b <= tol_s) for a, b in zip(dxy, ds)])), 4)
           if dxy else None}
    if exact is not None:
        oracle_ex = []
        for r, e in zip(gts, exact):
            if len(r) and len(e):
                oracle_ex.extend((ref_f64_slack(r, e, 0.0)).tolist())
        out.update(meets_tolerance_beyond_oracle_rounding=bool(rep.ok and all(slack_ok) and max(ds, default=0) <= tol_s),
                   max_dxy_px_gpu_vs_float64=round(rex.max_dxy, 6) if rex.matched else None,
                   max_dscore_gpu_vs_float64=round(rex.max_dscore, 7) if rex.matched else None,
                   gpu_vs_float64_matched=rex.matched, gpu_vs_float64_exempt=rex.exempt,
                   meets_gpu_vs_float64_bar=bool(rex.ok and rex.matched > 0),
                   gpu_vs_float64_bar=f"the SURVEY 8c protocol with the float64 evaluation as the reference: every "
                                      f"detection within {EXACT_TOL_XY:g} px / {EXACT_TOL_S:g} score, matched or "
                                      "exempt (tests/test_gpu_x3.py TOL_EXACT_XY)",
                   max_dxy_px_oracle_vs_float64=round(max(oracle_ex), 6) if oracle_ex else None,
                   float64_note="the same graph and weights evaluated in float64 (oracle/predict.py predict_exact): the "
                                "fp32 oracle's own distance from it bounds how closely any fp32 evaluation can agree")
    return out


DUMP_BUDGET_BYTES = 48 << 20  # --dump-outputs: the whole dump (all ranks) stays under this


def dump_outputs(res, out_dir, first_image, n_images):
    """--dump-outputs: the Results of one predict() call as float32 .npy files (layout: the module docstring).
    `first_image`: the global index of res[0]; `n_images`: the global batch, which shares DUMP_BUDGET_BYTES."""
    os.makedirs(out_dir, exist_ok=True)
    per_image = DUMP_BUDGET_BYTES // n_images
    for b, r in enumerate(res):
        g = first_image + b
        boxes = r.boxes.data.cpu().numpy().astype(np.float32)
        np.save(os.path.join(out_dir, f"boxes_{g:03d}.npy"), boxes)
        if r.masks is None:
            continue
        m = r.masks.data.cpu().numpy()
        m = m.reshape(m.shape[0], int(np.prod(m.shape[1:])))  # (n, H*W), n = 0 included
        k = min(m.shape[1], (per_image - boxes.nbytes) // (4 * max(m.shape[0], 1)))
        if k < m.shape[1]:  # a prefix of one seeded permutation of the pixels: the same positions in every build
            m = m[:, np.sort(np.random.default_rng(g).permutation(m.shape[1])[:k])]
        np.save(os.path.join(out_dir, f"masks_{g:03d}.npy"), m.astype(np.float32))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def spawn_ranks(n: int) -> int:
    """`--gpus N` without a launcher: run this script under torch.distributed.run with N ranks (the driver's own
    form), as a CHILD process — this process has not touched the GPU and is never replaced by exec — and return
    its exit status."""
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    return subprocess.call(cmd, env=env)


def plumbing(a, world, rank):
    """--plumbing: the multi-rank protocol of the bench on CPU (gloo), no GPU: blob broadcast, global batch-max
    all-reduce per step, barrier + max-over-ranks timing, one JSON line from rank 0 (tests/test_dist.py)."""
    from yolomi.dist import GlobalBatchMax, broadcast_blob, digest
    from yolomi.plan import pack_model
    from yolomi.synth import synth_weights
    dist.init_process_group("gloo")
    dev = torch.device("cpu")
    blob = pack_model(a.model, a.task, synth_weights(a.model, a.task, 0), "f16") if rank == 0 else None
    blob = broadcast_blob(blob, dev)
    h = torch.tensor(list(bytes.fromhex(digest(blob))), dtype=torch.uint8)
    hs = [torch.zeros_like(h) for _ in range(world)]
    dist.all_gather(hs, h)
    rule = GlobalBatchMax(device=dev)
    reads = [0]

    def local_max(x):  # stands in for ym_input_max: one read of the shard per call
        reads[0] += 1
        return rule.buf.copy_(x.amax().reshape(1))
    rule.local_max = local_max
    x = torch.rand(a.batch, 3, 32, 32) * (255.0 if rank == world - 1 else 1.0)

    def step():  # a stand-in for one forward: busy for the x3 yolo11s B=8 forward's ~1.6 ms
        t = time.perf_counter()
        while time.perf_counter() - t < 1.6e-3:
            pass
    for _ in range(a.warmup):
        rule(x)
        step()
    dist.barrier()
    reads[0] = 0
    t0 = time.perf_counter()
    for _ in range(a.steps):  # the bench's step at N > 1: the shard max all-reduced, then the forward
        m = rule(x)
        step()
    dist.barrier()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64)
    dist.all_reduce(el, op=dist.ReduceOp.MAX)
    if rank == 0:
        print(json.dumps({"metric": METRIC, "plumbing": True, "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
                          "value": round(world * a.batch * a.steps / float(el.item()), 2), "unit": "images/s",
                          "blob_bytes": len(blob), "blob_equal_on_all_ranks": all(torch.equal(hs[0], y) for y in hs),
                          "global_batch_max": float(m.item()), "batch_rule": BATCH_RULE[world > 1],
                          "batch_max_reads_per_step": reads[0] / a.steps}),
              flush=True)
    dist.destroy_process_group()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--model", default="s", help="scale (default s: BASELINE config 3, the headline workload)")
    ap.add_argument("--task", default="detect")
    ap.add_argument("--batch", type=int, default=8, help="images per GPU per step")
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--dtype", default="x3", choices=["f16", "f32", "i8", "f8", "x3"],
                    help="plan: x3 (default: split-f16 MFMA, meets the 1e-3 bar), f16, f32, i8, f8")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure what the headline figure does not need: device-loop "
                         "throughput, conv roofline and kernel table, the f16 throughput plan (x3 runs), the CPU "
                         "baseline with accuracy and parity against the oracle")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the detections (and masks) of the last timed step as DIR/<name>.npy, float32")
    ap.add_argument("--no-f16", action="store_true", help="--full x3 runs: skip the f16 throughput-plan comparison")
    ap.add_argument("--backend", default="qnnpack", choices=["qnnpack", "fbgemm"], help="i8: PTQ qconfig")
    ap.add_argument("--calib-batches", type=int, default=4, help="i8: calibration batches (B images each)")
    ap.add_argument("--cpu-seconds", type=float, default=16.0)
    ap.add_argument("--no-cpu", action="store_true", help="--full: skip the CPU baseline, accuracy and parity")
    ap.add_argument("--no-roofline", action="store_true", help="--full: skip the roofline and the kernel table")
    ap.add_argument("--plumbing", action="store_true", help="CPU/gloo rehearsal of the multi-rank protocol (no GPU)")
    ap.add_argument("--cabi-bcast", action="store_true",
                    help="N > 1: broadcast the weights through the C-ABI's ym_broadcast_weights instead of torch's "
                         "RCCL broadcast of the blob (the C-ABI receive path is tested on one GPU by its local "
                         "transport, ym_broadcast_weights_local; its RCCL transport has not run on >= 2 GPUs)")
    ap.add_argument("--lanes", type=int, default=int(os.environ.get("YM_LANES", "1")),
                    help="concurrent image slices per forward graph (yolomi lanes)")
    a = ap.parse_args()

    if "WORLD_SIZE" not in os.environ and a.gpus > 1:
        sys.exit(spawn_ranks(a.gpus))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        print(f"[bench] --gpus {a.gpus} but WORLD_SIZE={world}: refusing to report a mislabelled run", file=sys.stderr)
        sys.exit(2)
    if a.plumbing:
        return plumbing(a, world, rank)
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    if world > 1:
        dist.init_process_group("nccl", device_id=dev)

    from core.model import YOLO11Model
    from yolomi.dist import broadcast_blob, enable_global_rule, rccl_broadcast_model
    from yolomi.plan import pack_model
    from yolomi.synth import synth_weights

    # weights: packed once on rank 0, broadcast over RCCL by the C-ABI.  i8: rank 0 first runs the PTQ
    # calibration (exact-f32 plan + torch.ao observers, yolomi.quant) on synthetic batches disjoint from the timed one
    t_init = time.perf_counter()
    qp = None
    if rank == 0 and a.dtype in ("i8", "f8"):
        from yolomi.engine import Engine
        from yolomi.quant import calibrate
        ce = Engine(a.model, a.task, synth_weights(a.model, a.task, 0), dev, "f32")
        qp = calibrate(ce, [synthetic_batch(a.batch, a.size, 500 + i, dev) for i in range(a.calib_batches)],
                       "fp8" if a.dtype == "f8" else a.backend)
        del ce
    blob = pack_model(a.model, a.task, synth_weights(a.model, a.task, 0), a.dtype, qp) if rank == 0 else None

    def make_model(**kw):
        return YOLO11Model(task=a.task, size=a.model, device=f"cuda:{local}", dtype=a.dtype, **kw)
    if world > 1 and a.cabi_bcast:  # rank 0's blob into every rank's context over RCCL by the C-ABI
        model = rccl_broadcast_model(make_model, blob, dev, scale=a.model, task=a.task, dtype=a.dtype)
    elif world > 1:  # rank 0's blob as one uint8 tensor over RCCL (torch.distributed "nccl" = RCCL on ROCm)
        model = make_model(weights_blob=broadcast_blob(blob, dev))
    else:
        model = make_model(weights_blob=blob)
    model.model.engine.lanes = a.lanes
    init_s = time.perf_counter() - t_init

    B = a.batch
    x = synthetic_batch(B, a.size, 1000 + rank, dev)
    if world > 1:  # LoadTensor's /255 rule over the global batch: one read of the shard + an all-reduce every step
        enable_global_rule(model)
    for _ in range(a.warmup):
        model.predict(x)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        res = model.predict(x)
    torch.cuda.synchronize()
    if world > 1:
        dist.barrier()
    el = torch.tensor([time.perf_counter() - t0], dtype=torch.float64, device=dev)
    if world > 1:
        dist.all_reduce(el, op=dist.ReduceOp.MAX)
    elapsed = float(el.item())
    value = world * B * a.steps / elapsed
    if a.dump_outputs:
        dump_outputs(res, a.dump_outputs, rank * B, world * B)

    out = {
        "metric": METRIC, "value": round(value, 2), "unit": "images/s", "n_gpus": world, "steps": a.steps,
        "warmup": a.warmup, "ms_per_step": round(elapsed / a.steps * 1e3, 4), "higher_is_better": True,
        "scaling": "weak", "vs_baseline": None,
        "dtype": "f16x3" if a.dtype == "x3" else a.dtype,  # x3: fp16 MFMAs on hi/lo split operands, fp32 accumulation
        "data": "synthetic",
        "config": {"workload": f"yolo11{a.model} {a.task} {a.size}x{a.size} batch {B}/GPU {a.dtype}, predict() loop",
                   "model": f"yolo11{a.model}{'-seg' if a.task == 'segment' else ''}",
                   "batch_per_gpu": B, "global_batch": B * world, "image_size": a.size,
                   "parallelism": f"dp{world} (batch-sharded, RCCL weight broadcast)",
                   "batch_rule": BATCH_RULE[world > 1]},
        "init_s": round(init_s, 3),
    }
    Bl = model.model.engine.lane_batch(B)
    out["config"]["lanes"] = -(-B // Bl)
    out["config"]["conv_tiles"] = model.model.engine.tune_source.get((Bl, a.size, a.size), "heuristic")
    if a.full:
        # device-side throughput: back-to-back graph replays without the per-batch host sync of predict()
        eng = model.model.engine
        for _ in range(5):
            eng.run(x)
        torch.cuda.synchronize()
        td = time.perf_counter()
        for _ in range(a.steps):
            eng.run(x)
        torch.cuda.synchronize()
        out["device_images_per_s"] = round(B * a.steps / (time.perf_counter() - td) * world, 2)
    if a.full and rank == 0 and not a.no_roofline:
        out["roofline"] = conv_roofline(model, x, a.dtype, out["config"]["workload"])
        out["kernels"] = kernel_table(model, x, a.dtype, out["config"]["workload"])
    f16_dets = None
    if a.full and rank == 0 and world == 1 and a.dtype == "x3" and not a.no_f16:
        # the f16 throughput plan on the same batch and loop, for the cost of the tolerance
        m16 = YOLO11Model(task=a.task, size=a.model, device=f"cuda:{local}", dtype="f16",
                          weights_blob=pack_model(a.model, a.task, synth_weights(a.model, a.task, 0), "f16"))
        for _ in range(a.warmup):
            m16.predict(x)
        torch.cuda.synchronize()
        t16 = time.perf_counter()
        for _ in range(a.steps):
            r16 = m16.predict(x)
        torch.cuda.synchronize()
        el16 = time.perf_counter() - t16
        e16 = m16.model.engine
        td = time.perf_counter()
        for _ in range(a.steps):
            e16.run(x)
        torch.cuda.synchronize()
        f16_dets = [r.boxes.data.cpu().numpy() for r in r16]
        out["f16_throughput_plan"] = {
            "value": round(B * a.steps / el16, 2), "unit": "images/s", "ms_per_step": round(el16 / a.steps * 1e3, 4),
            "device_images_per_s": round(B * a.steps / (time.perf_counter() - td), 2),
            "conv_tiles": e16.tune_source.get((e16.lane_batch(B), a.size, a.size), "heuristic"),
            "x3_to_f16_ratio": round(value / (B * a.steps / el16), 4),
            "note": "fp16 storage + fp32 accumulation; misses the 1e-3 bar (see parity)"}
        del m16, e16
    if a.full and rank == 0 and world == 1 and not a.no_cpu:
        gdets = [r.boxes.data.cpu().numpy() for r in res]
        base, acc, gts, exact = cpu_baseline(a.model, a.task, gdets, x, a.cpu_seconds, qp)
        out["cpu_baseline"] = base
        out["accuracy"] = acc
        if qp is None:
            out["parity"] = parity(gdets, gts, exact=exact)
            if f16_dets is not None:
                out["f16_throughput_plan"]["parity"] = parity(f16_dets, gts)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
