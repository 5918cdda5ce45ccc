"""Time of the instance polygons (Engine.mask_contours = ym_mask_contours + its two reads) next to the device->host copy of
the same mask planes, DESIGN §18.

The batch of the segment bench config: yolo11s-seg (synthetic weights), B = 4 at 640 x 640, bench.py's seeded batch,
default predict().  The mask planes of all four images are gathered once into one (n, 640, 640) device tensor; then,
after a warm-up, two things are timed with a host clock around work that ends in a device->host read (so each figure
holds what a user waits for: launches, kernels, copies and the synchronisation), alternating, `--repeats` times each:

  contours   Engine.mask_contours(planes): three launches, the n + 1 offsets read, then exactly the points read
  copy       planes.cpu(): what any host tracer pays before it can start (pageable destination, as .cpu() gives)
  copy_pinned the same bytes into a pinned buffer allocated once (the best a host tracer can arrange)

Also reported: the device time of the three launches alone (device events around `--launches` back-to-back calls)
and of a count-only call (capacity 0: selection and offsets, nothing written).

    python tools/contour_timing.py [--repeats 30 --launches 200 --out profiles/contour_timing.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "yolo-infer_amd"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30, help="at least 5")
    ap.add_argument("--launches", type=int, default=200, help="calls between the two device events, at least 200")
    ap.add_argument("--dtype", default="x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contour_timing.json"))
    a = ap.parse_args()
    if a.repeats < 5 or a.launches < 200:
        ap.error("--repeats must be at least 5 and --launches at least 200")
    from bench import synthetic_batch
    from core.model import YOLO11Model
    dev = torch.device("cuda", 0)
    m = YOLO11Model(task="segment", size="s", device="cuda:0", dtype=a.dtype)
    eng = m.model.engine
    B, S = 4, 640
    res = m.predict(synthetic_batch(B, S, 1000, dev))
    counts = [len(r.boxes) for r in res]
    planes = torch.cat([r.masks.data for r in res]).contiguous()
    if planes.dtype == torch.bool:
        planes = planes.view(torch.uint8)
    n = planes.shape[0]
    polys = eng.mask_contours(planes)
    points = int(sum(len(p) for p in polys))
    pinned = torch.empty(planes.shape, dtype=planes.dtype, pin_memory=True)

    def contours():
        eng.mask_contours(planes)

    def copy():
        planes.cpu()

    def copy_pinned():
        pinned.copy_(planes, non_blocking=True)
        torch.cuda.synchronize(dev)

    what = {"contours": contours, "copy": copy, "copy_pinned": copy_pinned}
    for f in what.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize(dev)
    us = {k: [] for k in what}
    for _ in range(a.repeats):  # alternating: a drift of the host hits all three alike
        for k, f in what.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            us[k].append((time.perf_counter() - t0) * 1e6)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    cap = max(points, 1)
    pts = torch.empty((cap, 2), dtype=torch.int32, device=dev)
    offs = torch.empty((n + 1,), dtype=torch.int64, device=dev)
    st = torch.cuda.current_stream(dev).cuda_stream

    def launch():
        eng.rt.mask_contours(planes.data_ptr(), n, S, S, S * S, pts.data_ptr(), cap, offs.data_ptr(), st)
    for _ in range(10):
        launch()
    torch.cuda.synchronize(dev)
    e0.record()
    for _ in range(a.launches):
        launch()
    e1.record()
    e1.synchronize()
    c0, c1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    c0.record()
    for _ in range(a.launches):  # capacity 0: selection and offsets only, no point is written
        eng.rt.mask_contours(planes.data_ptr(), n, S, S, S * S, 0, 0, offs.data_ptr(), st)
    c1.record()
    c1.synchronize()
    med = {k: float(np.median(v)) for k, v in us.items()}
    result = {"model": f"yolo11s-seg {a.dtype}", "B": B, "H": S, "W": S, "counts": counts, "planes": n,
              "plane_bytes": int(planes.numel()), "points": points, "point_bytes": 8 * points + 8 * (n + 1),
              "longest_polygon": int(max((len(p) for p in polys), default=0)), "repeats": a.repeats,
              "contours_us_median": med["contours"], "contours_us_min": float(min(us["contours"])),
              "contours_us_max": float(max(us["contours"])),
              "copy_us_median": med["copy"], "copy_us_min": float(min(us["copy"])), "copy_us_max": float(max(us["copy"])),
              "copy_pinned_us_median": med["copy_pinned"], "copy_pinned_us_min": float(min(us["copy_pinned"])),
              "copy_pinned_us_max": float(max(us["copy_pinned"])),
              "contours_over_copy": med["contours"] / med["copy"] if med["copy"] else None,
              "contours_over_copy_pinned": med["contours"] / med["copy_pinned"] if med["copy_pinned"] else None,
              "launches_device_us": e0.elapsed_time(e1) * 1e3 / a.launches,
              "count_only_device_us": c0.elapsed_time(c1) * 1e3 / a.launches, "launches_timed": a.launches}
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
