#!/usr/bin/env python
"""The qualitative-video pipeline (anomalyclip_amd/visualizer.py), stage by stage, in frames per second on one synthetic video:
  compose_frames_per_s        acx_viz_compose on resident frames (HIP events, batches of --batch);
  forward_frames_per_s        acx_jpeg_forward on resident canvases (HIP events);
  d2h_frames_per_s            the coefficients of a batch to pinned memory (HIP events);
  entropy_frames_per_s        acx_jpeg_entropy_encode of a batch on --threads workers (host clock);
  end_to_end_frames_per_s     Visualizer.process_video from the frame folder to the finished .avi (host clock around work that ends
                              in the file's rename), with --decode as the frame reader.
The folder is written by Pillow (4:2:0, quality 75) into a temporary directory.  One JSON line; nothing is asserted.
  python tools/bench_visualize.py --frames 512 --source 240x320 --decode gpu --quality 90 --threads 8
With --entropy host,gpu the two Huffman coders are compared in this one process, on the same folder, canvas and thread count:
  entropy_dev_frames_per_s    acx_jpeg_entropy_encode_dev's launches on the batch entropy_frames_per_s codes (HIP events);
  end_to_end                  per mode the --reps repetitions of Visualizer.process_video, the modes alternating (host, gpu, host,
                              gpu ...), and the bytes copied to the host per frame;
  gpu_not_slower              the condition stated before the run: the gpu mode's mean is not below the host mode's by more than
                              the spread (largest - smallest) of the repetitions of either mode;
  files_identical             the modes' .avi files are the same bytes.
The line is also written to --out (default profiles/visualize_entropy_bench.json)."""
import argparse, json, os, shutil, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch


def event_rate(fn, frames, iters):
    """frames per second of fn() (device work on the current stream), by HIP events, after two warm-up calls"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return frames * iters / (e0.elapsed_time(e1) * 1e-3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--source", default="240x320", help="HxW of the frames")
    ap.add_argument("--decode", default="pil", choices=["pil", "gpu", "gpu_entropy"])
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--threads", type=int, default=8)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--canvas", default="1200x800", help="WxH of the picture")
    ap.add_argument("--classes", type=int, default=13)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--entropy", default=None, help="host,gpu: compare the two Huffman coders end to end")
    ap.add_argument("--reps", type=int, default=2, help="repetitions per mode of the comparison")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "visualize_entropy_bench.json"))
    args = ap.parse_args()
    from PIL import Image
    from anomalyclip_amd import ops
    from anomalyclip_amd import visualizer as V
    if not torch.cuda.is_available():
        raise SystemExit("bench_visualize measures the GPU pipeline: no GPU, no number")
    dev = torch.device("cuda", torch.cuda.current_device())
    H, W = (int(v) for v in args.source.split("x"))
    canvas = tuple(int(v) for v in args.canvas.split("x"))
    T, C1, B = args.frames, args.classes, args.batch
    rng = np.random.default_rng(0)
    root = tempfile.mkdtemp(prefix="bench_visualize_")
    try:
        folder = os.path.join(root, "frames", "Test", "video0")
        os.makedirs(folder)
        yy, xx = np.mgrid[0:H, 0:W]
        for i in range(T):                                 # a moving smooth field with some noise: frames that compress like video
            a = np.stack([128 + 100 * np.sin((xx + 3 * i) / 37.0) * np.cos(yy / 29.0), 128 + 90 * np.cos((xx - yy + i) / 53.0),
                          128 + 110 * np.sin(yy / 41.0 + i / 17.0)], -1) + rng.normal(0, 6, (H, W, 3))
            Image.fromarray(np.clip(a, 0, 255).astype(np.uint8)).save(os.path.join(folder, f"{i:06d}.jpg"), quality=75, subsampling=2)
        scores = torch.from_numpy((0.5 + 0.45 * np.sin(np.arange(T) / 40.0)).astype(np.float32)).to(dev)
        softmax = torch.softmax(torch.from_numpy(rng.standard_normal((T, C1)).astype(np.float32)), 1).to(dev)
        labels = torch.from_numpy(np.where((np.arange(T) // 100) % 2 == 1, 3, 7))
        viz = V.Visualizer(7, None, "{:06d}.jpg", os.path.join(root, "out"), dev, decode=args.decode, quality=args.quality,
                           canvas=canvas, frames_root=os.path.join(root, "frames"), batch=B, threads=args.threads)
        # ---- the stages on their own, on one resident batch
        lay = V.layout(canvas, C1, (H, W), T)
        geom, tables = V.geom_of(lay, 0.5), V.resize_tables(lay, dev)
        static = torch.from_numpy(V.static_layer(lay, scores.cpu().numpy(), labels.numpy(), 7, None, "video0")).to(dev)
        frames = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
        idx = torch.arange(B, dtype=torch.int32, device=dev)
        viz._ensure(dev)
        canv = torch.empty(B, canvas[1], canvas[0], 3, dtype=torch.uint8, device=dev)
        coef = torch.empty(B, canvas[0] * canvas[1] * 3 // 2, dtype=torch.int16, device=dev)
        res = {"frames": T, "source": args.source, "canvas": args.canvas, "decode": args.decode, "quality": args.quality,
               "threads": args.threads, "batch": B, "classes": C1}
        res["compose_frames_per_s"] = event_rate(lambda: ops.viz_compose(static, frames, scores[:B], softmax[:B], idx, tables, geom, out=canv), B, args.iters)
        res["forward_frames_per_s"] = event_rate(lambda: ops.jpeg_forward(canv, viz._qt_dev, out=coef), B, args.iters)
        res["d2h_frames_per_s"] = event_rate(lambda: viz._pin[0][:B].copy_(coef, non_blocking=True), B, args.iters)
        torch.cuda.synchronize()
        nbytes = []
        t0 = time.perf_counter()
        for _ in range(args.iters):
            nbytes = [len(d) for d in viz._pool.map(lambda j: viz._encode_one(0, j), range(B))]
        res["entropy_frames_per_s"] = B * args.iters / (time.perf_counter() - t0)
        res["mean_frame_bytes"] = float(np.mean(nbytes))
        # ---- the whole path: folder -> .avi
        path = [os.path.join(root, "features", "Test", "video0.npy")]
        torch.cuda.synchronize()                           # (the kernels are warm from the stages above)
        t0 = time.perf_counter()
        viz.process_video(scores, None, softmax, labels, path)
        res["end_to_end_frames_per_s"] = T / (time.perf_counter() - t0)
        out = os.path.join(root, "out", "qualitatives_var", "video0.avi")
        res["avi_bytes"] = os.path.getsize(out)
        viz.close()
        if args.entropy:
            modes = [V.check_entropy(m, "--entropy") for m in args.entropy.split(",")]
            head = torch.from_numpy(ops.jpeg_encode_header(viz.qtabs, canvas[1], canvas[0])).to(dev)
            ws = torch.empty(ops.jpeg_entropy_encode_dev_workspace_bytes(canvas[1], canvas[0], B), dtype=torch.uint8, device=dev)
            files = torch.empty(B, viz.cap, dtype=torch.uint8, device=dev)
            nb, st = torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev)
            res["entropy_dev_frames_per_s"] = event_rate(lambda: ops.jpeg_entropy_encode_dev(
                coef, head, canvas[1], canvas[0], cap=viz.cap, files=files, nbytes=nb, status=st, workspace=ws), B, args.iters)
            res["entropy_dev_status"] = sorted(set(st.cpu().tolist()))
            res["entropy_dev_workspace_bytes"] = ws.numel()
            del ws, files
            vs = {m: V.Visualizer(7, None, "{:06d}.jpg", os.path.join(root, "out_" + m), dev, decode=args.decode, quality=args.quality,
                                  canvas=canvas, frames_root=os.path.join(root, "frames"), batch=B, threads=args.threads, entropy=m)
                  for m in modes}
            rates, data = {m: [] for m in modes}, {}
            for r in range(args.reps + 1):                 # (the first round warms each mode's buffers up and is not counted)
                for m in modes:
                    avi = os.path.join(root, "out_" + m, "qualitatives_var", "video0.avi")
                    if os.path.exists(avi):
                        os.remove(avi)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    vs[m].process_video(scores, None, softmax, labels, path)
                    dt = time.perf_counter() - t0
                    if r:
                        rates[m].append(T / dt)
                    with open(avi, "rb") as fh:
                        data[m] = fh.read()
            res["end_to_end"] = {m: {"frames_per_s": rates[m], "mean_frames_per_s": float(np.mean(rates[m])),
                                     "bytes_to_host_per_frame": vs[m].bytes_to_host / vs[m].frames_written} for m in modes}
            for v in vs.values():
                v.close()
            res["files_identical"] = len({d for d in data.values()}) == 1
            if "host" in rates and "gpu" in rates:
                spread = max(max(v) - min(v) for v in rates.values())
                res["spread_frames_per_s"] = spread
                res["gpu_not_slower"] = bool(np.mean(rates["gpu"]) >= np.mean(rates["host"]) - spread)
            with open(args.out, "w") as fh:
                fh.write(json.dumps(res) + "\n")
        print(json.dumps(res))
    finally:
        shutil.rmtree(root, ignore_errors=True)


if __name__ == "__main__":
    main()
