#!/usr/bin/env python
"""The two device JPEG readers of anomalyclip_amd on the same folders, alternating in one process: jpeg.JpegFolderReader
(`decode="gpu"`: Huffman decoding on the pool) and jpeg.JpegEntropyFolderReader (`decode="gpu_entropy"`: on the device).  The
setting of tools/bench_jpeg_decode.py: Pillow-written 4:2:0 frames at quality 75, 8 decode threads.  Per frame size:
  host_frames_per_s          the host stage alone, batches of 512 into the pinned buffers (entropy decoding / read + parse + pack);
  entropy_ms_per_512_frames  acx_jpeg_entropy_decode_dev on resident scans, HIP events around `iters` launches after two warm-up
                             launches (the coefficients are zeroed outside the timed region: the kernel stores only non-zeros and
                             the DCs, which a second launch over the same buffer repeats);
  h2d_bytes_per_frame        bytes copied to the device per frame;
  c_frames_per_s             extract_dataset from the folder through the image encoder (one crop), per reader and repetition,
                             beside the encoder alone in the same process.
One JSON document, written to --out.
  python tools/bench_jpeg_entropy.py --arch ViT-B/16 --precision auto --frames 2048 --sizes 240x320,480x856 --decode-threads 8"""
import argparse, json, os, shutil, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tools"))
import numpy as np
import torch

from bench_jpeg_decode import host_rate


def entropy_ms(reader, n, iters=10):
    """-> (ms per 512 frames of the entropy kernel on n resident frames, sub_bits of the longest scan, its bytes)"""
    from anomalyclip_amd import ops
    n = min(n, len(reader))
    scans, (off, bits, huff), how = reader.decode_batch(0, n, 0)
    reader.close()
    assert all(h == 1 for h in how), "the folder holds frames the device decoder does not take"
    dev = torch.device("cuda", torch.cuda.current_device())
    longest = int(bits.max())
    scans, off, bits, huff = (t.to(dev) for t in (scans, off, bits, huff))
    geom = reader.geometry
    coef = torch.zeros(n, ops.jpeg_coef_elems(*geom), dtype=torch.int16, device=dev)
    status = torch.empty(n, dtype=torch.int32, device=dev)
    run = lambda: ops.jpeg_entropy_decode(scans, off, bits, huff, *geom, max_scan_bits=longest, coef=coef, status=status)
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    assert not status.any()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        run()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 512 / n, ops.jpeg_min_sub_bits(longest // 8), longest // 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--precision", default="auto")
    ap.add_argument("--frames", type=int, default=2048)
    ap.add_argument("--sizes", default="240x320,480x856")
    ap.add_argument("--decode-threads", type=int, default=8)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_entropy_bench.json"))
    args = ap.parse_args()
    from PIL import Image
    from anomalyclip_amd import _build
    from anomalyclip_amd import extract as X
    from anomalyclip_amd import init_weights as IW
    from anomalyclip_amd import ops
    from anomalyclip_amd.components.anomaly_clip import geometry_of_arch
    from anomalyclip_amd.jpeg import JpegEntropyFolderReader, JpegFolderReader
    from bench_extract import cpu_model, synthetic_frames
    dev = torch.device("cuda", torch.cuda.current_device())
    geom = geometry_of_arch(args.arch)
    with torch.device(dev):
        enc = X.build_image_encoder(args.arch, args.precision)
    init = IW.init_resnet_state_dict if geom.is_resnet else IW.init_vit_state_dict
    enc.load_state_dict(init(geom, 1, prefix=""), strict=True)
    enc.eval()
    kinds = ("gpu", "gpu_entropy")
    res = {"tool": "bench_jpeg_entropy", "arch": args.arch, "precision": args.precision, "frames": args.frames,
           "decode_threads": args.decode_threads, "reps": args.reps, "gpu": torch.cuda.get_device_name(dev), "cpu": cpu_model(),
           "jpeg": "Pillow, 4:2:0, quality 75", "sizes": {}}
    res["entropy_kernel_resources"] = next(v for k, v in _build.kernel_resources().items() if "jpeg_entropy_kernel" in k)
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
            r = {"file_bytes_mean": round(nbytes / args.frames), "host_frames_per_s": {k: [] for k in kinds},
                 "c_frames_per_s": {k: [] for k in kinds}}
            mk = {"gpu": lambda: JpegFolderReader(root, "v", threads=args.decode_threads),
                  "gpu_entropy": lambda: JpegEntropyFolderReader(root, "v", threads=args.decode_threads)}
            for kind in kinds:                                                             # page cache, pools, pinned allocations
                host_rate(mk[kind](), 512)
            for _ in range(args.reps):
                for kind in kinds:
                    r["host_frames_per_s"][kind].append(round(host_rate(mk[kind](), 512), 1))
            ms, sub, longest = entropy_ms(mk["gpu_entropy"](), 512)
            r["entropy_ms_per_512_frames"] = round(ms, 4)
            r["sub_bits_of_the_longest_scan"], r["longest_scan_bytes"] = sub, longest
            elems = ops.jpeg_coef_elems(H, W, 3, 2, 2)
            rd = mk["gpu_entropy"]()
            n = sum(b.shape[0] for _, b in rd.batches(512))
            torch.cuda.synchronize()
            assert n == args.frames and rd.fallbacks == 0
            r["h2d_bytes_per_frame"] = {"gpu": elems * 2 + 3 * 64 * 2, "gpu_entropy": round(rd.h2d_bytes / n)}
            for kind in kinds:                                                             # warm: tables, workspaces
                X.extract_dataset(enc, None, root, os.path.join(tmp, "warm"), 1, overwrite=True, decode_threads=args.decode_threads,
                                  decode=kind)
            for _ in range(args.reps):
                for kind in kinds:
                    t0 = time.perf_counter()
                    counts = X.extract_dataset(enc, None, root, os.path.join(tmp, "feats_" + kind), 1, overwrite=True,
                                               decode_threads=args.decode_threads, decode=kind)
                    dt = time.perf_counter() - t0
                    assert counts["frames"] == args.frames, counts
                    r["c_frames_per_s"][kind].append(round(args.frames / dt, 1))
            a, b = (np.load(os.path.join(tmp, "feats_" + k, "v.npy")) for k in kinds)
            r["files_equal"] = bool(np.array_equal(a, b))
            r["c_over_encoder"] = {k: [round(v / res["encoder_rows_per_s"], 3) for v in r["c_frames_per_s"][k]] for k in kinds}
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
