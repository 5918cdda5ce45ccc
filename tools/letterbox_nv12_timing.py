"""Time of the NV12 letterbox (one ym_letterbox_nv12 launch, csrc/ym_letterbox_nv12.hip) next to the route NV12 frames
had before it (convert every frame to packed BGR, then one ym_letterbox_batch launch), DESIGN §24.

Batches of 8 seeded random NV12 surfaces at 720 x 1280 and 1080 x 1920, letterboxed to imgsz 640.  Four variants, from one
process, alternating, `--repeats` times each, every one timed with device events around `--launches` back-to-back calls
after a warm-up:
  nv12_launch         the new launch alone, surfaces and descriptor table resident
  nv12_call           yolomi.preprocess.letterbox_nv12: table upload through pinned memory + the launch
  convert_then_batch  eight ym_nv12_to_bgr launches into packed BGR frames, then one ym_letterbox_batch launch
  batch_launch        ym_letterbox_batch alone on the BGR frames already converted (the floor that ignores the conversion)
The outputs of the variants are compared first: they must be the same bits.

    python tools/letterbox_nv12_timing.py [--repeats 10 --launches 100 --out profiles/letterbox_nv12_timing.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=10, help="at least 10")
    ap.add_argument("--launches", type=int, default=100, help="calls between the two device events, at least 100")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "letterbox_nv12_timing.json"))
    a = ap.parse_args()
    if a.repeats < 10 or a.launches < 100:
        ap.error("--repeats must be at least 10 and --launches at least 100")
    from yolomi.engine import Engine
    from yolomi.preprocess import NV12Frames, batch_geometry, frames_desc, letterbox_nv12, nv12_desc
    from yolomi.synth import synth_weights
    dev = torch.device("cuda", 0)
    rt = Engine("n", "detect", synth_weights("n", "detect", 0), dev, "x3").rt
    st = torch.cuda.current_stream(dev).cuda_stream
    B, S = 8, 640
    result = {"B": B, "imgsz": S, "repeats": a.repeats, "launches_timed": a.launches, "sizes": {}}
    for h, w in ((720, 1280), (1080, 1920)):
        surf = torch.from_numpy(np.random.default_rng(h).integers(0, 256, (B, 3 * h // 2, w), dtype=np.uint8)).to(dev)
        frames = NV12Frames.from_surface(surf)
        geo = batch_geometry(frames.y, S)
        uh, uw, t, b, l, r = geo[0]
        Hn, Wn = uh + t + b, uw + l + r
        desc = nv12_desc(frames, geo)
        dtab = torch.from_numpy(desc.view(np.uint8)).to(dev)
        bgr = torch.empty((B, h, w, 3), dtype=torch.uint8, device=dev)
        bl = list(bgr.unbind(0))
        bdesc = frames_desc(bl, geo)
        btab = torch.from_numpy(bdesc.view(np.uint8)).to(dev)
        out = torch.empty((B, 3, Hn, Wn), dtype=torch.float32, device=dev)
        old = torch.empty_like(out)

        def nv12_launch():
            rt.letterbox_nv12(dtab.data_ptr(), desc.ctypes.data, B, frames.coef, out.data_ptr(), Hn, Wn, st)

        def nv12_call():
            letterbox_nv12(rt, frames, dev, S, 32, st, geo=geo)

        def batch_launch():
            rt.letterbox_batch(btab.data_ptr(), bdesc.ctypes.data, B, old.data_ptr(), Hn, Wn, st)

        def convert_then_batch():
            for y, uv, f in zip(frames.y, frames.uv, bl):
                rt.nv12_to_bgr(y.data_ptr(), uv.data_ptr(), h, w, y.stride(0), uv.stride(0), frames.coef, f.data_ptr(),
                               3 * w, st)
            batch_launch()

        nv12_launch()
        convert_then_batch()
        same = torch.equal(out, old) and torch.equal(letterbox_nv12(rt, frames, dev, S, 32, st)[0], old)
        if not same:
            raise SystemExit(f"{h}x{w}: the NV12 launch and convert + ym_letterbox_batch differ")
        what = {"nv12_launch": nv12_launch, "nv12_call": nv12_call, "convert_then_batch": convert_then_batch,
                "batch_launch": batch_launch}
        for f in what.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize(dev)
        us = {k: [] for k in what}
        for _ in range(a.repeats):  # alternating: a drift of the machine hits all alike
            for k, f in what.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    f()
                e1.record()
                e1.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / a.launches)
        rec = {"canvas": [Hn, Wn], "nv12_bytes": int(surf.numel()), "bgr_bytes": int(bgr.numel()), "same_bits": same}
        for k, v in us.items():
            rec[f"{k}_us_median"], rec[f"{k}_us_min"], rec[f"{k}_us_max"] = float(np.median(v)), float(min(v)), float(max(v))
        rec["nv12_launch_below_convert_then_batch"] = bool(rec["nv12_launch_us_median"] < rec["convert_then_batch_us_median"])
        result["sizes"][f"{h}x{w}"] = rec
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
