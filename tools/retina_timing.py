"""Device time of the native-resolution mask stage alone (ym_masks_native: the flag memset + mask_native), DESIGN §13.

yolo11s-seg (synthetic weights), B=4 at 640², conf 0.25, every image's native shape (1080, 1920) by default: one
forward, its rows scaled to the native shape, then the stage timed with device events over preallocated buffers (so
no allocation or upload sits between the events), after warm-up.  Prints one JSON line: the detection counts, the mask
bytes, the median / min time and the time those bytes take at the store rate of profiles/r03g_store_probe.txt
(contiguous 1 KiB per instruction, the pattern of this kernel's 16-byte stores: 6.39 TB/s).

    python tools/retina_timing.py [--h0 1080 --w0 1920 --reps 30 --dtype x3] [--empty]

--empty gives every detection a zero-area box, so the stage stores the same bytes and evaluates no pixel: what is left
is the stores and the per-workgroup chain in front of them.
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

STORE_TBPS = 6.39


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--h0", type=int, default=1080)
    ap.add_argument("--w0", type=int, default=1920)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--dtype", default="x3")
    ap.add_argument("--empty", action="store_true", help="zero-area boxes: every byte stored as zero without evaluation")
    a = ap.parse_args()
    from core.model import YOLO11Model
    from tests.golden.make_golden import make_input
    from yolomi.preprocess import scale_boxes
    dev = torch.device("cuda", 0)
    m = YOLO11Model(task="segment", size="s", device="cuda:0", dtype=a.dtype)
    eng = m.model.engine
    x = make_input("uniform", (6001, 6002, 6003, 6004), 640).to(dev)
    B, H, W = 4, 640, 640
    dets, counts = eng.run(x, conf=0.25)
    n = counts[:B].tolist()
    rows = dets[:B].clone()
    shape = (a.h0, a.w0)
    for b in range(B):
        if n[b]:
            scale_boxes((H, W), rows[b, : n[b], :4], shape)
    if a.empty:
        rows[:, :, 2:4] = rows[:, :, 0:2]
    shapes = [shape] * B
    offs = [0]
    for k in n:
        offs.append(offs[-1] + k)
    total, px = offs[-1], a.h0 * a.w0
    masks = torch.empty((total * px,), dtype=torch.uint8, device=dev)
    flags = torch.empty((total,), dtype=torch.int32, device=dev)
    off_t = torch.tensor(offs, dtype=torch.int32, device=dev)
    shp_t = torch.tensor(shapes, dtype=torch.int32, device=dev)
    boff_t = torch.tensor([o * px for o in offs[:B]], dtype=torch.int64, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def stage():
        eng.rt.masks_native(rows.data_ptr(), rows.stride(1), B, rows.shape[1], off_t.data_ptr(), total, H, W, shapes,
                            shp_t.data_ptr(), boff_t.data_ptr(), masks.data_ptr(), flags.data_ptr(), stream)

    for _ in range(5):
        stage()
    torch.cuda.synchronize(dev)
    ms = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        stage()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    in_box = int(masks.view(total, -1).sum().item())
    bx = torch.cat([rows[b, : n[b], :4] for b in range(B)]).ceil().cpu()
    box_px = int(((bx[:, 2] - bx[:, 0]).clamp(min=0) * (bx[:, 3] - bx[:, 1]).clamp(min=0)).sum().item())
    us = np.asarray(ms) * 1e3
    store_us = total * px / (STORE_TBPS * 1e12) * 1e6
    print(json.dumps({"model": f"yolo11s-seg {a.dtype}", "B": B, "native": shape, "empty_boxes": a.empty, "counts": n,
                      "mask_bytes": total * px, "box_pixels": box_px, "set_pixels": in_box,
                      "nonempty": int(flags.sum().item()), "stage_us_median": float(np.median(us)),
                      "stage_us_min": float(us.min()), "store_us_at_6.39TBps": store_us,
                      "ratio_median_over_store": float(np.median(us)) / store_us}))


if __name__ == "__main__":
    main()
