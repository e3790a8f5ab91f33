#!/usr/bin/env python
"""Half-precision feature files against float32 files, both in ONE process on one device, the two alternating:

  gather   one 64-video training batch out of a resident bank (ops.sample_segments), HIP-event time per launch;
  tiles    the test-mode tiles of 8 videos in one launch (ops.tile_videos);
  stream   FeatureStream.batched() over the files, features/s of a consumer that reads every row once;
  load     FeatureBank over the files (page cache -> pinned slots -> device), seconds and GB/s of file bytes;
  extract  extract_video over pre-decoded frames (ViT-B/16 unless --arch), frames/s and bytes written.

Synthetic files in a temporary directory (page cache: the numbers are the loaders', not the disk's).  One JSON document.
    python tools/bench_feature_f16.py [--videos 128] [--frames 2000] [--rounds 5] [--out profiles/feature_f16_bench.json]"""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

DTYPES = ("float32", "float16")


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(ms):
    return {"median": round(med(ms), 4), "min": round(min(ms), 4), "max": round(max(ms), 4)}


def event_ms(fns, reps, warm=5):
    """HIP-event times of the callables, alternating: {name: [ms] * reps}"""
    for _ in range(warm):
        for f in fns.values():
            f()
    ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for k in fns}
    for r in range(reps):
        for k, f in fns.items():
            ev[k][r][0].record()
            f()
            ev[k][r][1].record()
    torch.cuda.synchronize()
    return {k: [a.elapsed_time(b) for a, b in ev[k]] for k in fns}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=128)
    ap.add_argument("--frames", type=int, default=2000, help="mean frames per video (lengths are drawn in [frames/2, 3 frames/2])")
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50, help="timed launches per dtype (gather, tiles)")
    ap.add_argument("--rounds", type=int, default=5, help="timed passes per dtype (stream, load, extract)")
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--extract-frames", type=int, default=512)
    ap.add_argument("--skip-extract", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_feature_f16.py measures on the GPU"
    from anomalyclip_amd import extract as X
    from anomalyclip_amd import feature_index as FI
    from anomalyclip_amd import init_weights as IW
    from anomalyclip_amd import ops
    from anomalyclip_amd.components.anomaly_clip import geometry_of_arch
    from anomalyclip_amd.feature_bank import FeatureBank, ResidentTrainLoader
    from anomalyclip_amd.feature_stream import FeatureStream
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    V, D, N, L = args.videos, args.width, 32, 16
    res = {"tool": "bench_feature_f16", "gpu": torch.cuda.get_device_name(dev), "videos": V, "frames_mean": args.frames, "width": D,
           "note": "float32 and float16 alternate inside one process on one device; times in ms unless named otherwise"}
    with tempfile.TemporaryDirectory() as td:
        lengths = [int(t) for t in rng.integers(args.frames // 2, args.frames * 3 // 2 + 1, size=V)]
        paths = {k: [] for k in DTYPES}
        for i, T in enumerate(lengths):
            h = (rng.standard_normal((T, D)) * 0.3).astype(np.float16)
            for k in DTYPES:
                paths[k].append(os.path.join(td, f"{k}_{i}.npy"))
                np.save(paths[k][-1], h.astype(k))
        file_bytes = {k: sum(os.path.getsize(p) for p in paths[k]) for k in DTYPES}

        # ---- load
        load_s = {k: [] for k in DTYPES}
        banks = {}
        for r in range(args.rounds + 1):                               # (the first pass warms the page cache and the allocator)
            for k in DTYPES:
                banks.pop(k, None)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                banks[k] = FeatureBank(paths[k], lengths, [0] * V, 1, dev)
                torch.cuda.synchronize()
                if r:
                    load_s[k].append(time.perf_counter() - t0)
        res["load"] = {k: {"bank_bytes": banks[k].nbytes, "file_bytes": file_bytes[k], "s": stats(load_s[k]),
                           "file_GBps_median": round(file_bytes[k] / med(load_s[k]) / 1e9, 2)} for k in DTYPES}
        assert torch.equal(banks["float16"].bank.float(), banks["float32"].bank)

        # ---- gather: one training batch
        b32 = banks["float32"]
        plan = ResidentTrainLoader(b32, range(V), args.batch, N, L, 1, rng=np.random.RandomState(1), generator=torch.Generator().manual_seed(1))
        vid, starts, _ = next(plan.host_batches())
        vid_d, starts_d = torch.from_numpy(vid).to(dev), torch.from_numpy(starts).to(dev)
        outs = {k: torch.empty(args.batch, 1, N * L, D, device=dev) for k in DTYPES}
        ms = event_ms({k: (lambda k=k: ops.sample_segments(banks[k].bank, b32.row_off, b32.frames, vid_d, starts_d, N, L, 1, 1, out=outs[k]))
                       for k in DTYPES}, args.reps)
        assert torch.equal(outs["float16"], outs["float32"])
        n = outs["float32"].numel()
        res["gather_one_batch"] = {k: dict(stats(ms[k]), bytes_moved=n * (4 + banks[k].bank.element_size()),
                                           GBps_median=round(n * (4 + banks[k].bank.element_size()) / med(ms[k]) / 1e6, 1)) for k in DTYPES}

        # ---- tiles: eight videos' test-mode tiles in one launch
        vids = list(range(8))
        S = [FI.test_start_indices(lengths[v], N, L, 1)[1] for v in vids]
        touts = {k: torch.empty(N * L * sum(S), D, device=dev) for k in DTYPES}
        ms = event_ms({k: (lambda k=k: ops.tile_videos(banks[k].bank, b32.row_off, b32.frames, vids, S, N, L, 1, 1, out=touts[k]))
                       for k in DTYPES}, args.reps)
        assert torch.equal(touts["float16"], touts["float32"])
        n = touts["float32"].numel()
        res["tile_eight_videos"] = {k: dict(stats(ms[k]), bytes_moved=n * (4 + banks[k].bank.element_size()),
                                            GBps_median=round(n * (4 + banks[k].bank.element_size()) / med(ms[k]) / 1e6, 1)) for k in DTYPES}
        banks.clear()

        # ---- stream
        feats = sum(lengths)
        rate = {k: [] for k in DTYPES}
        acc = torch.zeros(D, device=dev)
        for r in range(args.rounds + 1):
            for k in DTYPES:
                stream = FeatureStream(paths[k], N, L, 1, 1, dev)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for x, meta in stream.batched():
                    acc += x.sum(0)                                    # a consumer that reads every row once
                torch.cuda.synchronize()
                if r:
                    rate[k].append(feats / (time.perf_counter() - t0))
        res["stream_batched"] = {k: {"features_per_s": stats(rate[k]), "file_GBps_median": round(med(rate[k]) * D * np.dtype(k).itemsize / 1e9, 2)}
                                 for k in DTYPES}

    # ---- extract
    if not args.skip_extract:
        geom = geometry_of_arch(args.arch)
        with torch.device(dev):
            enc = X.build_image_encoder(args.arch, "auto")
        init = IW.init_resnet_state_dict if geom.is_resnet else IW.init_vit_state_dict
        enc.load_state_dict(init(geom, 1, prefix=""), strict=True)
        enc.eval()
        T = args.extract_frames
        frames = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (T, 240, 320, 3), dtype=np.uint8)).pin_memory()
        fps, size = {k: [] for k in DTYPES}, {}
        with tempfile.TemporaryDirectory() as td:
            for r in range(args.rounds + 1):
                for k in DTYPES:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    X.extract_video(enc, frames, os.path.join(td, k), 1, overwrite=True, dtype=k)
                    if r:
                        fps[k].append(T / (time.perf_counter() - t0))
                    size[k] = os.path.getsize(os.path.join(td, k + ".npy"))
            a, b = np.load(os.path.join(td, "float32.npy")), np.load(os.path.join(td, "float16.npy"))
            assert np.array_equal(a.astype(np.float16), b)
        res["extract_predecoded"] = {"arch": args.arch, "frames": T, **{k: {"frames_per_s": stats(fps[k]), "file_bytes": size[k]} for k in DTYPES}}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
