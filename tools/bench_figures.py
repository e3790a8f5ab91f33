"""Times what the evaluation figures add to the metrics epilogue, in one process on one device: `evaluate` without figures and
`evaluate(figure_columns=W)` interleaved; the decimation launches alone (both modes) on a curve whose points spread evenly over the
columns and on the worst case, every point in one column; a device-to-device copy of the curve's bytes as the yardstick; and the
host's drawing of the four files.  Prints one JSON line.
Usage: python tools/bench_figures.py [--frames N] [--classes C] [--columns W] [--rounds R]"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from anomalyclip_amd import _lib as L, figures as F, metrics as M, ops


def median(v):
    return float(np.median(np.asarray(v, dtype=np.float64)))


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def events_ms(fn, reps):
    """mean per call of `reps` back-to-back calls, between two HIP events"""
    fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def record(P, N, k, dev):
    r = L.CurveResult()
    r.n_pos, r.n_neg, r.n_distinct, r.opt_index, r.opt_threshold = int(P), int(N), int(k), -1, 1.0
    return torch.frombuffer(bytearray(bytes(r)), dtype=torch.uint8).to(dev)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1_111_808)      # UCF-Crime test split
    ap.add_argument("--classes", type=int, default=14)
    ap.add_argument("--columns", type=int, default=F.DEFAULT_COLUMNS)
    ap.add_argument("--rounds", type=int, default=15)
    a = ap.parse_args()
    n, C, W, nid = a.frames, a.classes, a.columns, a.classes // 2
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    labels = rng.integers(0, C, n)
    labels[rng.random(n) < 0.9] = nid
    s = np.clip(0.4 * (labels != nid) + 0.6 * rng.random(n), 0, 1).astype(np.float32)
    p = rng.random((n, C - 1)).astype(np.float32)
    p = (p / p.sum(1, keepdims=True) * s[:, None]).astype(np.float32)
    ds, dl, dp = (torch.from_numpy(x).to(dev) for x in (s, labels, p))
    plain = lambda: M.evaluate(ds, dl, dp, nid, C)
    figs = lambda: M.evaluate(ds, dl, dp, nid, C, figure_columns=W)
    for _ in range(3):
        plain(), figs()
    t_plain, t_figs = [], []
    for _ in range(a.rounds):                                     # interleaved: drift of the clocks hits both alike
        t_plain.append(wall_ms(plain))
        t_figs.append(wall_ms(figs))
    r = figs()
    k = len(r["roc_points"][0])

    # the launches alone: a curve of n points (every score distinct) spread evenly, and all in one column (N == 0 / huge P)
    idx = torch.arange(1, n + 1, dtype=torch.int32, device=dev)
    tps_u, fps_u = idx // 2, idx - idx // 2
    out = torch.empty(2, W, 4, 3, dtype=torch.int32, device=dev)
    rec_u = record(n // 2, n - n // 2, n, dev)
    rec_w = record(2 ** 31 - 1, 0, n, dev)                        # ROC: N == 0; PR: tps * W < P
    both = lambda rec: [ops.curve_decimate(tps_u, fps_u, rec, m, W, out=out[m]) for m in (0, 1)]
    dec_u = [events_ms(lambda: both(rec_u), 20) for _ in range(a.rounds)]
    dec_w = [events_ms(lambda: both(rec_w), 20) for _ in range(a.rounds)]
    filled = int((out[:, :, 0, 0] >= 0).sum().item())
    dst = torch.empty(2, n, dtype=torch.int32, device=dev)
    src = torch.stack([tps_u, fps_u])
    copy = [events_ms(lambda: dst.copy_(src), 20) for _ in range(a.rounds)]
    # what a host plotter would be handed instead: the curve's arrays over the bus
    full = [wall_ms(lambda: (tps_u.cpu(), fps_u.cpu())) for _ in range(5)]

    draw = []
    with tempfile.TemporaryDirectory() as d:
        for _ in range(5):
            t0 = time.perf_counter()
            F.write_all(d, r, None, W)
            draw.append((time.perf_counter() - t0) * 1e3)
    print(json.dumps({
        "n_frames": n, "classes": C, "columns": W, "rounds": a.rounds, "device": torch.cuda.get_device_name(0),
        "evaluate_ms": round(median(t_plain), 4), "evaluate_with_figures_ms": round(median(t_figs), 4),
        "figures_add_ms": round(median(t_figs) - median(t_plain), 4),
        "figures_add_fraction": round(median(t_figs) / median(t_plain) - 1.0, 4),
        "evaluate_ms_min_max": [round(min(t_plain), 4), round(max(t_plain), 4)],
        "evaluate_with_figures_ms_min_max": [round(min(t_figs), 4), round(max(t_figs), 4)],
        "polyline_points_roc": k, "polyline_points_pr": len(r["pr_points"][0]),
        "decimate_points": n, "decimate_both_modes_uniform_ms": round(median(dec_u), 5),
        "decimate_both_modes_one_column_ms": round(median(dec_w), 5),
        "one_column_over_uniform": round(median(dec_w) / median(dec_u), 3), "one_column_filled_columns": filled,
        "launches_per_mode": 3, "curve_bytes": 8 * n, "copy_d2d_curve_bytes_ms": round(median(copy), 5),
        "curve_arrays_to_host_ms": round(median(full), 4), "table_bytes_to_host": 2 * W * 48,
        "draw_four_files_ms": round(median(draw), 3), "auc_roc": r["auc_roc"], "auc_pr": r["auc_pr"]}))


if __name__ == "__main__":
    main()
