"""Tracker configuration for `YOLO11Model.track` (Ultralytics `model.track(tracker=...)`): only ByteTrack is offered;
its state and its update run on the GPU (csrc/ym_track.hip through `yolomi.lib.Tracker`)."""
from __future__ import annotations

import os
from typing import Dict, Union

from .lib import TRACK_DEFAULTS

_FLOATS = ("track_high_thresh", "track_low_thresh", "new_track_thresh", "match_thresh")


def tracker_config(tracker: Union[str, os.PathLike, Dict, None] = "bytetrack.yaml") -> Dict:
    """The six ByteTrack parameters of `tracker`: the name ("bytetrack.yaml" / "bytetrack": trackers/cfg/bytetrack.yaml's
    values), a YAML file with the same keys, or a dict.  Missing keys take the defaults; `tracker_type`, when given,
    must be "bytetrack".  NotImplementedError for BoT-SORT (it needs optical-flow global motion compensation);
    ValueError for an unknown key, a threshold outside [0, 1] or a negative track_buffer."""
    if tracker is None:
        tracker = "bytetrack.yaml"
    if isinstance(tracker, dict):
        raw = dict(tracker)
    else:
        name = os.fspath(tracker)
        stem = os.path.splitext(os.path.basename(name))[0].lower()
        if os.path.isfile(name):
            import yaml
            with open(name) as f:
                raw = yaml.safe_load(f) or {}
            if not isinstance(raw, dict):
                raise ValueError(f"{name}: a tracker file holds `key: value` lines")
        elif stem == "bytetrack":
            raw = {}
        elif stem == "botsort":
            raw = {"tracker_type": "botsort"}
        else:
            raise ValueError(f"unknown tracker {name!r}: 'bytetrack.yaml', a YAML file with its keys, or a dict")
    kind = str(raw.pop("tracker_type", "bytetrack")).lower()
    if kind == "botsort":
        raise NotImplementedError("tracker 'botsort' is not offered: it needs optical-flow global motion compensation "
                                  "(GMC); use 'bytetrack.yaml'")
    if kind != "bytetrack":
        raise ValueError(f"unknown tracker_type {kind!r} (only 'bytetrack')")
    unknown = sorted(set(raw) - set(TRACK_DEFAULTS))
    if unknown:
        raise ValueError(f"unknown tracker keys {unknown} (ByteTrack has {sorted(TRACK_DEFAULTS)})")
    cfg = dict(TRACK_DEFAULTS, **raw)
    for k in _FLOATS:
        cfg[k] = float(cfg[k])
        if not 0.0 <= cfg[k] <= 1.0:
            raise ValueError(f"tracker {k} = {cfg[k]} outside [0, 1]")
    cfg["track_buffer"] = int(cfg["track_buffer"])
    if cfg["track_buffer"] < 0:
        raise ValueError(f"tracker track_buffer = {cfg['track_buffer']} is negative")
    cfg["fuse_score"] = bool(cfg["fuse_score"])
    return cfg
