#!/usr/bin/env python
"""The two frame readers of anomalyclip_amd on the same JPEG folders, alternating in one process: extract.FrameFolderReader
(Pillow on the pool) and jpeg.JpegFolderReader (Huffman decoding on the pool, the rest on the device).  Per frame size:
  host_frames_per_s   the host stage alone: batches of 512 decoded into the pinned buffers, nothing consumed on the device;
  reconstruct_ms_per_512_frames   acx_jpeg_reconstruct on resident coefficients (HIP events);
  c_frames_per_s      extract_dataset from the folder through the image encoder (one crop), per reader and repetition.
The folders are written by Pillow (4:2:0, quality 75) into a temporary directory.  One JSON document, written to --out.
  python tools/bench_jpeg_decode.py --arch ViT-B/16 --precision auto --frames 1024 --sizes 240x320,480x856 --decode-threads 8"""
import argparse, json, os, shutil, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch


def host_rate(reader, batch):
    """frames per second of the reader's host stage: every batch decoded into its pinned buffers, no device work"""
    T = len(reader)
    reader.frame_size
    t0 = time.perf_counter()
    for k, i in enumerate(range(0, T, batch)):
        reader.decode_batch(i, min(T, i + batch), k & 1)
    dt = time.perf_counter() - t0
    reader.close()
    return T / dt


def reconstruct_ms(reader, n, iters=10):
    """acx_jpeg_reconstruct on n resident frames, ms per 512 frames"""
    from anomalyclip_amd import ops
    n = min(n, len(reader))
    coef, qt, ok = reader.decode_batch(0, n, 0)
    reader.close()
    assert all(ok), "the folder holds frames the host decoder does not take"
    dev = torch.device("cuda", torch.cuda.current_device())
    coef, qt = coef.to(dev), qt.to(dev)
    out = torch.empty(n, *reader.frame_size, 3, dtype=torch.uint8, device=dev)
    for _ in range(2):
        ops.jpeg_reconstruct(coef, qt, *reader.geometry, out=out)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ops.jpeg_reconstruct(coef, qt, *reader.geometry, out=out)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 512 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--precision", default="auto")
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--sizes", default="240x320,480x856")
    ap.add_argument("--decode-threads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_decode_bench.json"))
    args = ap.parse_args()
    from PIL import Image
    from anomalyclip_amd import extract as X
    from anomalyclip_amd import init_weights as IW
    from anomalyclip_amd.components.anomaly_clip import geometry_of_arch
    from anomalyclip_amd.jpeg import JpegFolderReader
    from bench_extract import cpu_model, synthetic_frames
    dev = torch.device("cuda", torch.cuda.current_device())
    geom = geometry_of_arch(args.arch)
    with torch.device(dev):
        enc = X.build_image_encoder(args.arch, args.precision)
    init = IW.init_resnet_state_dict if geom.is_resnet else IW.init_vit_state_dict
    enc.load_state_dict(init(geom, 1, prefix=""), strict=True)
    enc.eval()
    res = {"tool": "bench_jpeg_decode", "arch": args.arch, "precision": args.precision, "frames": args.frames,
           "decode_threads": args.decode_threads, "reps": args.reps, "gpu": torch.cuda.get_device_name(dev), "cpu": cpu_model(),
           "jpeg": "Pillow, 4:2:0, quality 75", "sizes": {}}
    with torch.no_grad():                                          # the encoder alone, launches of `chunk` rows
        x = torch.randn(enc.chunk, 3, enc.input_resolution, enc.input_resolution, device=dev)
        enc(x)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(4):
            enc(x)
        torch.cuda.synchronize()
        res["encoder_rows_per_s"] = round(4 * enc.chunk / (time.perf_counter() - t0), 1)
    tmp = tempfile.mkdtemp(prefix="acx_jpeg_bench_")
    try:
        for size in args.sizes.split(","):
            H, W = (int(v) for v in size.split("x"))
            root = os.path.join(tmp, size)
            vdir = os.path.join(root, "v")
            os.makedirs(vdir)
            base = synthetic_frames(min(args.frames, 64), H, W)
            nbytes = 0
            for t in range(args.frames):
                p = os.path.join(vdir, X.TEMPLATE.format(t))
                Image.fromarray(np.roll(base[t % len(base)], t // len(base), axis=1)).save(p, quality=75, subsampling=2)
                nbytes += os.path.getsize(p)
            r = {"file_bytes_mean": round(nbytes / args.frames), "host_frames_per_s": {"pil": [], "gpu": []},
                 "c_frames_per_s": {"pil": [], "gpu": []}}
            mk = {"pil": lambda: X.FrameFolderReader(root, "v", threads=args.decode_threads),
                  "gpu": lambda: JpegFolderReader(root, "v", threads=args.decode_threads)}
            host_rate(mk["pil"](), 512), host_rate(mk["gpu"](), 512)                      # page cache, pools, pinned allocations
            for _ in range(args.reps):
                for kind in ("pil", "gpu"):
                    r["host_frames_per_s"][kind].append(round(host_rate(mk[kind](), 512), 1))
            r["reconstruct_ms_per_512_frames"] = round(reconstruct_ms(mk["gpu"](), 512), 4)
            for kind in ("pil", "gpu"):                                                    # warm: tables, workspaces
                X.extract_dataset(enc, None, root, os.path.join(tmp, "warm"), 1, overwrite=True, decode_threads=args.decode_threads,
                                  decode=kind)
            for _ in range(args.reps):
                for kind in ("pil", "gpu"):
                    t0 = time.perf_counter()
                    counts = X.extract_dataset(enc, None, root, os.path.join(tmp, "feats_" + kind), 1, overwrite=True,
                                               decode_threads=args.decode_threads, decode=kind)
                    dt = time.perf_counter() - t0
                    assert counts["frames"] == args.frames, counts
                    r["c_frames_per_s"][kind].append(round(args.frames / dt, 1))
            a, b = (np.load(os.path.join(tmp, "feats_" + k, "v.npy")) for k in ("pil", "gpu"))
            r["files_equal"] = bool(np.array_equal(a, b))
            res["sizes"][size] = r
            shutil.rmtree(root, ignore_errors=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
