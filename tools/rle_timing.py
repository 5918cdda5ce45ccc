"""Time of the COCO run-length encoding on the GPU (ym_mask_rle) next to what it replaces: the device->host
copy of the same mask planes, and that copy plus the numpy oracle's encode (tests/rle_oracle.py).

Box-cropped masks of yolo11s-seg (synthetic weights, bench.py's seeded batch), repeated cyclically up to n planes, at
three points: 40 and 300 planes of 640 x 640 (default predict()), 40 planes of the native 853 x 1280 of an image source
(retina_masks=True).  Per point, in `--repeats` alternated windows:

  rle_device    device events around `--launches` back-to-back ym_mask_rle calls with fitting capacities, per call
  rle_call      Engine.mask_rle(planes) by the host clock: the call, the offsets / areas read, the counts and bytes read
  copy_pinned   the planes into a pinned buffer allocated once, by the host clock, synchronised
  copy          planes.cpu() (pageable destination), by the host clock
  host_encode   the oracle's encode of all planes, already on the host
Medians with min and max, and the bytes that cross to the host on either path.  The back-to-back calls of rle_device
read the same planes again and again, so 16 - 123 MB of input may come from the last-level cache: a cache-warm figure.

    python tools/rle_timing.py [--repeats 15 --launches 50 --out profiles/rle_timing.json]
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


def spread(v):
    return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}


def point(eng, planes, a, dev):
    from tests.rle_oracle import encode
    n, H, W = planes.shape
    enc = eng.mask_rle(planes)
    runs, nbytes = sum(len(c) for c, _, _ in enc), sum(len(s) for _, s, _ in enc)
    host = planes.cpu().numpy()
    assert all(np.array_equal(c, r[0]) and s == r[1] and ar == r[2] for (c, s, ar), r in zip(enc[:8], map(encode, host[:8])))
    pinned = torch.empty(planes.shape, dtype=planes.dtype, pin_memory=True)
    bufs = eng.mask_rle_device(planes, runs, nbytes)
    st = torch.cuda.current_stream(dev).cuda_stream
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def rle_device():
        e0.record()
        for _ in range(a.launches):
            eng.rt.mask_rle(planes.data_ptr(), n, H, W, H * W, bufs[0].data_ptr(), runs, bufs[1].data_ptr(), nbytes,
                            bufs[2].data_ptr(), bufs[3].data_ptr(), bufs[4].data_ptr(), st)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / a.launches

    def clocked(f):
        def run():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            f()
            torch.cuda.synchronize(dev)
            return (time.perf_counter() - t0) * 1e6
        return run

    what = {"rle_device": rle_device, "rle_call": clocked(lambda: eng.mask_rle(planes, runs, nbytes)),
            "copy_pinned": clocked(lambda: pinned.copy_(planes, non_blocking=True)), "copy": clocked(lambda: planes.cpu()),
            "host_encode": clocked(lambda: [encode(p) for p in host])}
    for f in what.values():
        f()
    us = {k: [] for k in what}
    for _ in range(a.repeats):  # alternating: a drift of the machine hits all alike
        for k, f in what.items():
            us[k].append(f())
    out = {"planes": n, "H": H, "W": W, "runs": runs, "string_bytes": nbytes, "set_fraction": float(host.mean()),
           "bytes_to_host_copy": int(planes.numel()), "bytes_to_host_rle": 4 * runs + nbytes + 8 * (3 * n + 2)}
    out.update({k + "_us": spread(v) for k, v in us.items()})
    out["copy_pinned_plus_encode_us"] = out["copy_pinned_us"]["median"] + out["host_encode_us"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=15)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--dtype", default="x3")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rle_timing.json"))
    a = ap.parse_args()
    from bench import synthetic_batch
    from core.model import YOLO11Model
    dev = torch.device("cuda", 0)
    m = YOLO11Model(task="segment", size="s", device="cuda:0", dtype=a.dtype)
    eng = m.model.engine

    def planes_of(res, n):
        p = torch.cat([r.masks.data for r in res])
        assert len(p) > 0, "no detections"
        p = p[torch.arange(n, device=p.device) % len(p)].contiguous()
        return p.view(torch.uint8) if p.dtype == torch.bool else p

    square = m.predict(synthetic_batch(4, 640, 1000, dev))
    image = (synthetic_batch(1, 1280, 1000, dev)[0, :, :853] * 255).permute(1, 2, 0).to(torch.uint8).cpu().numpy()
    native = m.predict([np.ascontiguousarray(image)], retina_masks=True, conf=0.1)
    result = {"model": f"yolo11s-seg {a.dtype}", "repeats": a.repeats, "launches": a.launches, "points": []}
    for planes in (planes_of(square, 40), planes_of(square, 300), planes_of(native, 40)):
        result["points"].append(point(eng, planes, a, dev))
        print(json.dumps(result["points"][-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
