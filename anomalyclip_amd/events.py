"""Anomaly events of unlabeled videos: the step from the per-frame decision of the reference (anomaly_clip_module.py:537-547: a frame
is normal when abnormal_score < threshold, else it takes the arg-max class) to events -- runs of such frames with hysteresis
(`lo`), gap merging (`max_gap`) and a length filter (`min_len`).  The scores stay on the device (ops.score_events, include/acx.h
acx_score_events has the exact rules); only the event tables reach the host, and `write_events` leaves them as events.json."""
from __future__ import annotations

import json
import math
import os
from typing import Any, Dict, List, Optional, Sequence

import numpy as np
import torch

from . import ops

EVENT_FIELDS = ("start", "end", "class", "votes", "hot_frames", "peak_frame")
STAT_FIELDS = ("peak", "mean")


class EventList(list):
    """one video's events (dicts, ascending start); `total`: every kept event of the video, `truncated`: total > max_events"""
    total: int = 0
    truncated: bool = False


def find_events(scores: torch.Tensor, probs: torch.Tensor, row_off, normal_idx: int, hi: float, lo: Optional[float] = None,
                max_gap: int = 0, min_len: int = 1, max_events: int = 1024) -> List[EventList]:
    """scores f32 [n] and probs f32 [n, C - 1] (class_probs without the normal column) of V videos laid end to end on the device,
    video v = rows row_off[v] .. row_off[v + 1] - 1 -> one EventList per video of dicts {start, end, class, votes, hot_frames,
    peak_frame, peak, mean} (frames relative to the video, inclusive).  `lo=None`: lo = hi, and with max_gap = 0, min_len = 1 the
    events are the maximal runs of the reference's y_pred != normal_idx.  One launch sequence; ONE copy to the host of
    V + 8 * (events found) doubles."""
    dev = scores.device
    row_off = torch.as_tensor(row_off, dtype=torch.int64).to(dev).contiguous()
    V, E = row_off.numel() - 1, int(max_events)
    lo = hi if lo is None else lo
    count, events, stats = ops.score_events(scores.contiguous(), probs.contiguous(), row_off, normal_idx, hi, lo, max_gap,
                                            min_len, E)
    have = count.clamp(0, E)
    mask = torch.arange(E, device=dev)[None, :] < have[:, None]
    host = torch.cat([count.double(), events[mask].double().reshape(-1), stats[mask].reshape(-1)]).cpu().numpy()
    cnt = host[:V].astype(np.int64)
    if (cnt < 0).any():
        bad = int(np.nonzero(cnt < 0)[0][0])
        raise ValueError(f"find_events: row_off is not a monotone partition of the {scores.numel()} rows at video {bad}")
    K = int(np.minimum(cnt, E).sum())
    ev = host[V:V + 6 * K].astype(np.int64).reshape(K, 6)
    st = host[V + 6 * K:].reshape(K, 2)
    out, k = [], 0
    for v in range(V):
        lst = EventList()
        lst.total, lst.truncated = int(cnt[v]), bool(cnt[v] > E)
        for _ in range(min(int(cnt[v]), E)):
            d: Dict[str, Any] = {f: int(x) for f, x in zip(EVENT_FIELDS, ev[k])}
            d.update({f: float(x) for f, x in zip(STAT_FIELDS, st[k])})
            lst.append(d)
            k += 1
        out.append(lst)
    return out


def _json_number(x: float):
    return None if isinstance(x, float) and not math.isfinite(x) else x      # (json has no NaN: an all-NaN event's peak / mean)


def write_events(path, videos: Sequence[str], events: Sequence[Sequence[dict]], params: dict,
                 class_names: Optional[Sequence[str]] = None) -> dict:
    """events.json: {"params": the parameters and the threshold as given, "videos": [{"video", "count", "truncated", "events":
    [...]}]}, sorted keys, indent 4; each event carries `class_name` where `class_names` has one for its class."""
    if len(videos) != len(events):
        raise ValueError(f"write_events: {len(videos)} videos, {len(events)} event lists")
    recs = []
    for name, lst in zip(videos, events):
        evs = []
        for e in lst:
            d = {k: _json_number(v) for k, v in e.items()}
            if class_names is not None and 0 <= int(e["class"]) < len(class_names):
                d["class_name"] = str(class_names[int(e["class"])])
            evs.append(d)
        recs.append({"video": str(name), "count": int(getattr(lst, "total", len(lst))),
                     "truncated": bool(getattr(lst, "truncated", False)), "events": evs})
    doc = {"params": {k: _json_number(v) for k, v in dict(params).items()}, "videos": recs}
    os.makedirs(os.path.dirname(os.path.abspath(str(path))), exist_ok=True)
    with open(path, "w") as fp:
        json.dump(doc, fp, indent=4, sort_keys=True)
    return doc
