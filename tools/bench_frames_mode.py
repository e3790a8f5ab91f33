#!/usr/bin/env python
"""Frame folders without feature files (`data.load_from_features: false`): the two device-side pieces it adds.

  (a) acx_tile_videos: the test-mode tiles of a group of 8 videos of 2,000 frames (D = 512, one crop, 32 x 16 grid: 16,384 rows,
      33.5 MB) in one launch, against `Tensor.copy_` of the same bytes and against the only way to fill that buffer without the
      kernel: 8 acx_sample_segments launches and a torch.cat.  HIP-event medians over --reps timings of each, the three
      alternating in one loop.  The bank (--videos videos, 0.5 GB by default) is larger than the Infinity Cache and every timing
      takes another group of videos, so the rows come out of HBM each time.  The Python wrappers take longer than these
      kernels run, so every round of three is preceded by two device copies of the whole bank (about 0.4 ms): the host enqueues
      the round while they run and the events then bracket device time, not the enqueue ("queued"); the same loop without them
      is reported as "as_issued".
  (b) the bank fill (FeatureBank.fill_video: extract.encode_video + a device-to-device copy per launch) on pre-decoded pinned
      frames against the encoder alone on the same launches: rows/s, --runs runs of each, alternating.
One JSON line per run, appended to --out.   python tools/bench_frames_mode.py [--reps 60] [--frames 2048] [--runs 2]"""
import argparse, json, os, sys, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch


def median(v):
    v = sorted(v)
    return v[len(v) // 2]


def bench_tile_videos(dev, args):
    from anomalyclip_amd import ops
    from anomalyclip_amd import feature_index as FI
    V, T, D, N, L, G = args.videos, 2000, 512, 32, 16, 8
    assert V % G == 0 and V // G >= 4, "--videos: a multiple of 8, at least 32"
    bank = torch.randn(V * T, D, device=dev)
    row_off = torch.arange(V, dtype=torch.int64, device=dev) * T
    frames = torch.full((V,), T, dtype=torch.int32, device=dev)
    starts, S = FI.test_start_indices(T, N, L, 1)
    rows = N * L * S
    starts_d = torch.from_numpy(starts.astype(np.int32)).to(dev)
    vid_d = [torch.tensor([v], dtype=torch.int32, device=dev) for v in range(V)]
    out = torch.empty(G * rows, D, device=dev)
    parts = [torch.empty(1, 1, rows, D, device=dev) for _ in range(G)]
    groups = [list(range(g * G, (g + 1) * G)) for g in range(V // G)]
    flat, n = bank.view(-1), out.numel()

    def tile(g):
        ops.tile_videos(bank, row_off, frames, groups[g], [S] * G, N, L, 1, 1, out=out)

    def copy(g):
        off = min(g * G * T * D, flat.numel() - n)             # the group's own rows (the last group: the bank's last n floats)
        out.view(-1).copy_(flat[off:off + n])

    def eight(g):
        for k, v in enumerate(groups[g]):
            ops.sample_segments(bank, row_off, frames, vid_d[v], starts_d, N * S, L, 1, 1, out=parts[k])
        return torch.cat([p.view(rows, D) for p in parts], 0)

    variants = (tile, copy, eight)
    for g in range(3):                                         # warm-up: tables built, allocator primed
        for f in variants:
            f(g)
    want = eight(1)
    tile(1)
    assert torch.equal(out, want)
    scratch = torch.empty_like(bank)

    def measure(queued):
        ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in variants] for _ in range(args.reps)]
        for r in range(args.reps):
            if queued:                                         # the device is busy while the host enqueues this round
                scratch.copy_(bank)
                scratch.copy_(bank)
            for k, f in enumerate(variants):
                g = (3 * r + k) % len(groups)                  # another group for every timing: no variant reads what the last one cached
                ev[r][k][0].record()
                f(g)
                ev[r][k][1].record()
        torch.cuda.synchronize()
        return [[ev[r][k][0].elapsed_time(ev[r][k][1]) for r in range(args.reps)] for k in range(3)]
    for g in range(len(groups)):                               # every group's tables are on the device before anything is timed
        tile(g)
    issued = measure(False)
    ms = measure(True)
    moved = 2 * n * 4
    res = {"videos_per_group": G, "frames_per_video": T, "D": D, "rows": G * rows, "bytes_read_plus_written": moved,
           "bank_bytes": bank.numel() * 4, "timings_each": args.reps}
    for name, m in zip(("tile_videos", "copy_same_bytes", "eight_sample_segments_plus_cat"), ms):
        res[name] = {"ms_median": round(median(m), 4), "ms_min": round(min(m), 4), "GBps": round(moved / median(m) / 1e6, 1)}
    res["as_issued_ms_median"] = {name: round(median(m), 4) for name, m in zip(("tile_videos", "copy_same_bytes",
                                                                               "eight_sample_segments_plus_cat"), issued)}
    res["tile_over_copy_rate"] = round(median(ms[1]) / median(ms[0]), 3)
    res["tile_over_eight_plus_cat_time"] = round(median(ms[0]) / median(ms[2]), 3)
    return res


def bench_bank_fill(dev, args):
    from anomalyclip_amd import extract as X
    from anomalyclip_amd import init_weights as IW
    from anomalyclip_amd.components.anomaly_clip import geometry_of_arch
    from anomalyclip_amd.feature_bank import FeatureBank
    from bench_extract import synthetic_frames
    geom = geometry_of_arch(args.arch)
    with torch.device(dev):
        enc = X.build_image_encoder(args.arch, args.precision)
    enc.load_state_dict(IW.init_vit_state_dict(geom, 1, prefix=""), strict=True)
    enc.eval()
    F, crop = args.frames, enc.input_resolution
    nb = X.batch_frames(enc, 1)
    pinned = torch.from_numpy(synthetic_frames(F, 240, 320)).pin_memory()
    x = torch.randn(nb, 3, crop, crop, device=dev)
    spans = [min(nb, F - i) for i in range(0, F, nb)]
    bank = FeatureBank.__new__(FeatureBank)                    # one video of F frames, filled again and again
    bank.paths, bank.ncrops, bank.D, bank.offsets = ["pinned"], 1, int(enc.output_dim), np.asarray([0, F], dtype=np.int64)
    bank.bank = torch.empty(F, bank.D, device=dev)

    def alone():
        with torch.no_grad():
            for n in spans:
                enc(x[:n])

    def fill():
        bank.fill_video(enc, 0, pinned)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    alone(), fill()
    torch.cuda.synchronize()
    a, b = [], []
    for _ in range(args.runs):
        a.append(timed(alone))
        b.append(timed(fill))
    return {"arch": args.arch, "precision": args.precision, "ncrops": 1, "rows": F, "rows_per_launch": nb, "runs_each": args.runs,
            "encoder_alone_rows_per_s": [round(F / t, 1) for t in a], "bank_fill_rows_per_s": [round(F / t, 1) for t in b],
            "fill_over_alone": round(min(a) / min(b), 4), "fill_over_alone_per_run": [round(x_ / y_, 4) for x_, y_ in zip(a, b)]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=60, help="(a): timings of each variant (at least 50)")
    ap.add_argument("--videos", type=int, default=128, help="(a): videos of 2,000 frames in the bank")
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--precision", default="auto")
    ap.add_argument("--frames", type=int, default=2048, help="(b): rows per run")
    ap.add_argument("--runs", type=int, default=2)
    ap.add_argument("--skip-fill", action="store_true")
    ap.add_argument("--skip-tile", action="store_true")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "frames_mode_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_frames_mode.py measures on the GPU"
    assert args.reps >= 50
    sys.path.insert(0, os.path.join(REPO, "tools"))
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"tool": "bench_frames_mode", "gpu": torch.cuda.get_device_name(dev)}
    if not args.skip_tile:
        res["a_tile_videos"] = bench_tile_videos(dev, args)
    torch.cuda.empty_cache()
    if not args.skip_fill:
        res["b_bank_fill"] = bench_bank_fill(dev, args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
