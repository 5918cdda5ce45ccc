"""Time of the frame-batch letterbox (one ym_letterbox_batch launch, csrc/ym_letterbox_batch.hip) next to the path it
stands beside (one ym_letterbox launch per image), DESIGN §23.

Batches of 8 seeded random HWC uint8 frames at 720 x 1280 and 1080 x 1920, letterboxed to imgsz 640.  Four variants, from
one process, alternating, `--repeats` times each, every one timed with device events around `--launches` back-to-back
calls (the variant with host copies: a tenth of that) after a warm-up:
  batch_launch     the new launch alone, frames and descriptor table resident
  frames_call      yolomi.preprocess.letterbox_frames: table upload through pinned memory + the launch
  eight_launches   eight ym_letterbox launches on resident frames
  eight_with_h2d   yolomi.preprocess.letterbox_batch: eight blocking host-to-device copies + eight launches
The outputs of the variants are compared first: they must be the same bits.

    python tools/letterbox_batch_timing.py [--repeats 10 --launches 100 --out profiles/letterbox_batch_timing.json]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "letterbox_batch_timing.json"))
    a = ap.parse_args()
    if a.repeats < 10 or a.launches < 100:
        ap.error("--repeats must be at least 10 and --launches at least 100")
    from yolomi.engine import Engine
    from yolomi.preprocess import batch_geometry, frames_desc, letterbox_batch, letterbox_frames
    from yolomi.synth import synth_weights
    dev = torch.device("cuda", 0)
    rt = Engine("n", "detect", synth_weights("n", "detect", 0), dev, "x3").rt
    st = torch.cuda.current_stream(dev).cuda_stream
    B, S = 8, 640
    result = {"B": B, "imgsz": S, "repeats": a.repeats, "launches_timed": a.launches, "sizes": {}}
    for h, w in ((720, 1280), (1080, 1920)):
        rng = np.random.default_rng(h)
        imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for _ in range(B)]
        frames = torch.from_numpy(np.stack(imgs)).to(dev)
        fl = list(frames.unbind(0))
        geo = batch_geometry(imgs, S)
        uh, uw, t, b, l, r = geo[0]
        Hn, Wn = uh + t + b, uw + l + r
        desc = frames_desc(fl, geo)
        dtab = torch.from_numpy(desc.view(np.uint8)).to(dev)
        out = torch.empty((B, 3, Hn, Wn), dtype=torch.float32, device=dev)
        old = torch.empty_like(out)

        def batch_launch():
            rt.letterbox_batch(dtab.data_ptr(), desc.ctypes.data, B, out.data_ptr(), Hn, Wn, st)

        def frames_call():
            letterbox_frames(rt, frames, dev, S, 32, st, geo=geo)

        def eight_launches():
            for i, g in enumerate(geo):
                rt.letterbox(fl[i].data_ptr(), h, w, 3 * w, True, g[0], g[1], g[2], g[4], old[i].data_ptr(), Hn, Wn, st)

        def eight_with_h2d():
            letterbox_batch(rt, imgs, dev, S, 32, st, geo=geo)

        batch_launch()
        eight_launches()
        same = torch.equal(out, old) and torch.equal(letterbox_frames(rt, frames, dev, S, 32, st)[0], old)
        if not same:
            raise SystemExit(f"{h}x{w}: the batch launch and the per-image launches differ")
        what = {"batch_launch": (batch_launch, a.launches), "frames_call": (frames_call, a.launches),
                "eight_launches": (eight_launches, a.launches), "eight_with_h2d": (eight_with_h2d, a.launches // 10)}
        for f, _ in what.values():
            for _ in range(3):
                f()
        torch.cuda.synchronize(dev)
        us = {k: [] for k in what}
        for _ in range(a.repeats):  # alternating: a drift of the machine hits all alike
            for k, (f, n) in what.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(n):
                    f()
                e1.record()
                e1.synchronize()
                us[k].append(e0.elapsed_time(e1) * 1e3 / n)
        rec = {"canvas": [Hn, Wn], "frame_bytes": int(frames.numel()), "same_bits": same}
        for k, v in us.items():
            rec[f"{k}_us_median"], rec[f"{k}_us_min"], rec[f"{k}_us_max"] = float(np.median(v)), float(min(v)), float(max(v))
        rec["batch_launch_not_slower_than_eight_launches"] = bool(
            rec["batch_launch_us_median"] <= rec["eight_launches_us_median"])
        result["sizes"][f"{h}x{w}"] = rec
    print(json.dumps(result))
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
