"""Times events.find_events at the scale of UCF-Crime's test list -- 290 videos, 1.1 M frames, 13 classes without the normal column --
against the device-to-host copy of `scores` + `probs`, which is what a host implementation of the same rules would need before it
could start.  One process, one device, the arms interleaved round by round; every window ends in a device synchronise.  Arms:
  find_events        the launch sequence, the gather of the filled slots and the one copy of the tables (host clock)
  score_events       the two launches alone (device events, mean of back-to-back calls)
  to_host_pageable   scores.cpu(), probs.cpu()
  to_host_pinned     copies into page-locked buffers allocated once
Prints one JSON line.  Usage: python tools/bench_events.py [--videos V] [--frames N] [--classes C1] [--rounds R]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anomalyclip_amd import events as EV, ops


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events_ms(fn, reps):
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def synthetic(V, n, C1, seed=0):
    """video lengths log-normal like a surveillance set (a few videos hold a large part of the frames), scores low with bursts of
    a few hundred frames, probabilities a scaled softmax-like row"""
    rng = np.random.default_rng(seed)
    w = rng.lognormal(0.0, 1.1, V)
    T = np.maximum(1, np.floor(w / w.sum() * n)).astype(np.int64)
    T[np.argmax(T)] += n - T.sum()
    s = 0.25 * rng.random(n, dtype=np.float32)
    for _ in range(max(1, n // 4000)):
        a = int(rng.integers(0, n))
        s[a:a + int(rng.integers(20, 600))] += np.float32(0.5)
    s = np.clip(s + 0.1 * rng.standard_normal(n).astype(np.float32), 0, 1).astype(np.float32)
    p = rng.random((n, C1), dtype=np.float32)
    p = (p / p.sum(1, keepdims=True) * s[:, None]).astype(np.float32)
    return s, p, np.concatenate([[0], np.cumsum(T)]).astype(np.int64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=290)
    ap.add_argument("--frames", type=int, default=1_111_808)      # UCF-Crime test split
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    V, n, C1 = a.videos, a.frames, a.classes
    dev = torch.device("cuda", 0)
    s, p, off = synthetic(V, n, C1)
    ds, dp, doff = (torch.from_numpy(x).to(dev) for x in (s, p, off))
    kw = dict(hi=0.5, lo=0.35, max_gap=16, min_len=8, max_events=1024)
    normal = C1 // 2
    find = lambda: EV.find_events(ds, dp, doff, normal, **kw)
    launches = lambda: ops.score_events(ds, dp, doff, normal, kw["hi"], kw["lo"], kw["max_gap"], kw["min_len"], kw["max_events"])
    pageable = lambda: (ds.cpu(), dp.cpu())
    hs, hp = torch.empty(s.shape, dtype=torch.float32).pin_memory(), torch.empty(p.shape, dtype=torch.float32).pin_memory()
    pinned = lambda: (hs.copy_(ds, non_blocking=True), hp.copy_(dp, non_blocking=True))
    for _ in range(3):
        find(), launches(), pageable(), pinned()
    t = {"find_events": [], "score_events": [], "to_host_pageable": [], "to_host_pinned": []}
    for _ in range(a.rounds):                                     # interleaved: drift of the clocks hits every arm alike
        t["find_events"].append(wall_ms(find))
        t["score_events"].append(events_ms(launches, 10))
        t["to_host_pageable"].append(wall_ms(pageable))
        t["to_host_pinned"].append(wall_ms(pinned))
    found = find()
    nev = sum(len(f) for f in found)
    out = {"videos": V, "n_frames": n, "classes_without_normal": C1, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
           "params": kw, "longest_video_frames": int(np.diff(off).max()), "events_found": nev,
           "videos_truncated": sum(bool(f.truncated) for f in found), "launches": 2,
           "scores_probs_bytes": int(s.nbytes + p.nbytes), "tables_bytes_to_host": 8 * (V + 8 * nev)}
    for k, v in t.items():
        out[k + "_ms"] = round(median(v), 4)
        out[k + "_ms_min_max"] = [round(min(v), 4), round(max(v), 4)]
    out["pinned_copy_over_find_events"] = round(median(t["to_host_pinned"]) / median(t["find_events"]), 2)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
