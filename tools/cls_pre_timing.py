"""Time of classify preprocessing on the GPU (yolomi.preprocess.classify_batch_gpu: staging, one copy, one
ym_classify_pre launch) next to the host path it replaces (classify_batch: Pillow, then .to(device)), DESIGN §21.

Batches of 16 seeded random HWC uint8 images at 500 x 375 and at 1080 x 1920, imgsz 224.  After a warm-up the two paths
are timed with a host clock around work that ends in a device synchronise, alternating, `--repeats` times each.  Also
reported: the device time of the kernel alone (device events around `--launches` back-to-back launches on a batch that
is already on the device).

    python tools/cls_pre_timing.py [--repeats 30 --launches 200 --out profiles/cls_pre_timing.json]
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
    ap.add_argument("--repeats", type=int, default=30, help="at least 30")
    ap.add_argument("--launches", type=int, default=200, help="launches between the two device events, at least 200")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cls_pre_timing.json"))
    a = ap.parse_args()
    if a.repeats < 30 or a.launches < 200:
        ap.error("--repeats must be at least 30 and --launches at least 200")
    from yolomi.engine import Engine
    from yolomi.preprocess import classify_batch, classify_batch_gpu, classify_desc
    from yolomi.synth import synth_weights
    dev = torch.device("cuda", 0)
    rt = Engine("n", "classify", synth_weights("n", "classify", 0, nc=1000), dev, "x3", nc=1000).rt
    st = torch.cuda.current_stream(dev).cuda_stream
    B, S = 16, 224
    result = {"B": B, "imgsz": S, "repeats": a.repeats, "launches_timed": a.launches, "sizes": {}}
    for h, w in ((500, 375), (1080, 1920)):
        rng = np.random.default_rng(h)
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(B)]

        def host():
            classify_batch(imgs, S).to(dev)

        def gpu():
            classify_batch_gpu(rt, imgs, dev, S, st)

        what = {"host": host, "gpu": gpu}
        for f in what.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize(dev)
        us = {k: [] for k in what}
        for _ in range(a.repeats):  # alternating: a drift of the host hits both alike
            for k, f in what.items():
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                f()
                torch.cuda.synchronize(dev)
                us[k].append((time.perf_counter() - t0) * 1e6)
        desc, nbytes = classify_desc([(h, w)] * B, S)
        packed = np.zeros(nbytes + desc.nbytes, dtype=np.uint8)
        for d, im in zip(desc, imgs):
            packed[int(d["off"]):int(d["off"]) + im.size] = im.reshape(-1)
        packed[nbytes:] = desc.view(np.uint8)
        dbuf = torch.from_numpy(packed).to(dev)
        out = torch.empty((B, 3, S, S), dtype=torch.float32, device=dev)

        def launch():
            rt.classify_pre(dbuf.data_ptr(), dbuf.data_ptr() + nbytes, desc.ctypes.data, B, S, out.data_ptr(), st)
        for _ in range(10):
            launch()
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.launches):
            launch()
        e1.record()
        e1.synchronize()
        r = {"image_bytes": int(nbytes), "kernel_device_us": e0.elapsed_time(e1) * 1e3 / a.launches}
        for k, v in us.items():
            r[f"{k}_us_median"], r[f"{k}_us_min"], r[f"{k}_us_max"] = float(np.median(v)), float(min(v)), float(max(v))
        r["gpu_below_host_by_more_than_host_spread"] = bool(
            r["host_us_median"] - r["gpu_us_median"] > r["host_us_max"] - r["host_us_min"])
        result["sizes"][f"{h}x{w}"] = r
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
