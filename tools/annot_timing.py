"""Device time of the annotator (Engine.annotate = ym_annotate: annot_records + annot_draw), DESIGN §17.

B = 8 fp32 CHW frames at 640 x 640 and three scripted row sets — detect, 20 boxes per image; pose, 300 instances of 17
keypoints per image; segment, 50 boxes per image with 640 x 640 masks — on an empty context (the annotator reads rows,
not a model).  Per case: 5 repeats of one pair of device events around `--launches` (>= 200) back-to-back calls after a
warm-up, reported as the median and the spread (min, max) of the per-call time over the repeats; next to it the byte
floor, i.e. the bytes the call must move (frames in 12 B/px, canvas out 3 B/px, sum n * H * W mask bytes) over the
HBM rate a streaming kernel reaches on this part (6.29 TB/s measured float4 copy; 8 TB/s is the specification).

    python tools/annot_timing.py [--launches 200 --out profiles/annot_timing.json]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-infer_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_TBPS = 6.29
B, H, W = 8, 640, 640
NAMES = {0: "person", 1: "bicycle", 2: "car", 3: "motorcycle"}


def rows_detect(rng, n, stride=6):
    r = np.zeros((B, 300, stride), dtype=np.float32)
    x1, y1 = rng.uniform(0, W - 80, (B, n)), rng.uniform(0, H - 80, (B, n))
    w, h = rng.uniform(30, 300, (B, n)), rng.uniform(30, 300, (B, n))
    r[:, :n, 0], r[:, :n, 1] = x1, y1
    r[:, :n, 2], r[:, :n, 3] = np.minimum(x1 + w, W), np.minimum(y1 + h, H)
    r[:, :n, 4], r[:, :n, 5] = rng.uniform(0.25, 1, (B, n)), rng.integers(0, 4, (B, n))
    return r


def rows_pose(rng, n):
    r = rows_detect(rng, n, 6 + 52)
    r[:, :, 5] = 0
    cx, cy = (r[:, :n, 0] + r[:, :n, 2]) / 2, (r[:, :n, 1] + r[:, :n, 3]) / 2
    sx, sy = (r[:, :n, 2] - r[:, :n, 0]) / 2, (r[:, :n, 3] - r[:, :n, 1]) / 2
    k = rng.uniform(-1, 1, (B, n, 17, 2))
    kp = np.zeros((B, n, 17, 3), dtype=np.float32)
    kp[..., 0] = cx[..., None] + k[..., 0] * sx[..., None]
    kp[..., 1] = cy[..., None] + k[..., 1] * sy[..., None]
    kp[..., 2] = rng.uniform(0.3, 1, (B, n, 17))
    r[:, :n, 6:6 + 51] = kp.reshape(B, n, 51)
    return r


def masks_for(rows, n):
    m = np.zeros((B, n, H, W), dtype=np.uint8)
    for b in range(B):
        for i in range(n):
            x1, y1, x2, y2 = rows[b, i, :4].astype(int)
            m[b, i, y1:y2, x1:x2] = 1
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200, help="calls between the two events, at least 200")
    ap.add_argument("--repeats", type=int, default=5, help="at least 5")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "annot_timing.json"))
    ap.add_argument("--case", default=None, help="run one case only (detect20 | pose300 | segment50), e.g. under a profiler")
    a = ap.parse_args()
    if a.launches < 200 or a.repeats < 5:  # the recorded figures stay comparable: never fewer than these
        ap.error("--launches must be at least 200 and --repeats at least 5")
    from yolomi.engine import Engine
    from yolomi.lib import Runtime
    dev = torch.device("cuda", 0)
    e = Engine.__new__(Engine)
    e.device, e.task, e.kpt_shape = dev, "detect", None
    e.rt, e.names, e._annot_tables = Runtime(0, None), dict(NAMES), None
    rng = np.random.default_rng(17)
    frames = torch.from_numpy(rng.random((B, 3, H, W), dtype=np.float32)).to(dev)
    seg_rows = rows_detect(rng, 50)
    cases = {"detect20": (rows_detect(rng, 20), 20, None, None), "pose300": (rows_pose(rng, 300), 300, (17, 3), None),
             "segment50": (seg_rows, 50, None, masks_for(seg_rows, 50))}
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    result = {"B": B, "H": H, "W": W, "frames": "fp32 CHW", "launches_per_repeat": a.launches, "repeats": a.repeats,
              "hbm_TBps_for_floor": HBM_TBPS, "cases": {}}
    for name, (rows, n, kshape, masks) in cases.items():
        if a.case and a.case != name:
            continue
        dets = torch.from_numpy(rows).to(dev)
        counts = torch.full((B,), n, dtype=torch.int32, device=dev)
        mk = torch.from_numpy(masks).to(dev) if masks is not None else None

        def call():
            e.annotate(frames, dets, counts, masks=mk, kpt_shape=kshape or (0, 0), out=out)
        for _ in range(10):
            call()
        torch.cuda.synchronize(dev)
        us = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                call()
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1e3 / a.launches)
        nbytes = B * H * W * (12 + 3) + (B * n * H * W if masks is not None else 0)
        floor = nbytes / (HBM_TBPS * 1e12) * 1e6
        result["cases"][name] = {"instances_per_image": n, "bytes_moved_at_least": nbytes,
                                 "us_per_call_median_of_repeats": float(np.median(us)),
                                 "us_per_call_min_of_repeats": float(min(us)), "us_per_call_max_of_repeats": float(max(us)),
                                 "byte_floor_us": floor, "median_over_floor": float(np.median(us)) / floor,
                                 "images_per_s_at_median": B / (float(np.median(us)) * 1e-6)}
    print(json.dumps(result))
    if a.out and not a.case:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
