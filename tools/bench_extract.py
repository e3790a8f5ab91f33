#!/usr/bin/env python
"""Feature extraction from frames (anomalyclip_amd/extract.py) against its encoder, in encoder rows per second:
  (a) the encoder alone on resident f32 input, launches of `chunk` rows;
  (b) extract_video on pre-decoded uint8 frames in pinned memory (copy, crops, encoder, rows back, file written);
  (c) extract_dataset from JPEG folders this tool writes to a temporary directory (host decode included).
Also the crop kernel's own time per 512 rows (HIP events).  One JSON line, appended to profiles/extract_bench.jsonl.
`--pack`: extract_dataset over many short clips (64 folders of 40 ... 300 frames, two frame sizes) with pack off and on, alternating in
one process, for 1 and 10 crops and decode pil / gpu_entropy: rows/s and encoder launches per arm, one JSON line per pair, appended
to profiles/extract_pack_bench.jsonl.
  python tools/bench_extract.py --arch ViT-B/16 --precision auto --ncrops 10 --frames 512 --hw 240x320
  python tools/bench_extract.py --kernel-only --crop-size 336 --ncrops 10 --hw 240x320        (no encoder: the kernel alone)
  python tools/bench_extract.py --pack --arch ViT-B/16 --precision auto"""
import argparse, json, os, platform, shutil, sys, tempfile, time
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import numpy as np
import torch


def cpu_model():
    try:
        with open("/proc/cpuinfo") as fh:
            for line in fh:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor() or platform.machine()


def synthetic_frames(F, H, W, seed=0):
    """moving gradients + noise: JPEG-compressible, not flat"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.empty((F, H, W, 3), dtype=np.uint8)
    for t in range(F):
        a = np.stack([(xx * 2 + t * 5) % 256, (yy * 3 + t * 3) % 256, ((xx + yy) + t * 7) % 256], -1).astype(np.int64)
        out[t] = np.clip(a + rng.integers(-24, 25, a.shape), 0, 255)
    return out


def crop_kernel_ms(frames_dev, crop, scale, ncrops, iters=20):
    from anomalyclip_amd.preprocess import preprocess_crops
    for _ in range(2):
        preprocess_crops(frames_dev, crop, scale, ncrops)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        preprocess_crops(frames_dev, crop, scale, ncrops)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


PACK_FOLDERS, PACK_SIZES, PACK_REPS = 64, ((240, 320), (360, 480)), 2


def pack_lengths():
    """64 clip lengths between 40 and 300 frames, the same at every run"""
    return [40 + (v * 97) % 261 for v in range(PACK_FOLDERS)]


def write_short_clips(root):
    """the frames root of the --pack leg: folder v holds pack_lengths()[v] JPEG frames of PACK_SIZES[v % 2].  300 frames per size are
    synthesised and compressed once; folder v starts v frames into them (its files are copies of those bytes)"""
    import io
    from PIL import Image
    lens = pack_lengths()
    for k, (H, W) in enumerate(PACK_SIZES):
        blobs = []
        for a in synthetic_frames(300, H, W, seed=k):
            fh = io.BytesIO()
            Image.fromarray(a).save(fh, "JPEG", quality=90)
            blobs.append(fh.getvalue())
        for v in range(k, PACK_FOLDERS, 2):
            d = os.path.join(root, f"clip{v:03d}")
            os.makedirs(d)
            for t in range(lens[v]):
                with open(os.path.join(d, "{:06d}.jpg".format(t)), "wb") as fh:
                    fh.write(blobs[(t + v) % 300])
    return lens


def pack_leg(args):
    """pack off against pack on over the short clips: per (ncrops, decode) PACK_REPS repetitions of each arm, alternating.  The
    condition (fixed before the first run): the slower packed repetition is faster than the faster unpacked one by more than the
    spread of the unpacked repetitions.  boundary_ms: the time one video boundary costs the unpacked run -- the difference of the
    arms' mean times over the 64 boundaries (the ragged last launch of every video is part of it)."""
    from anomalyclip_amd import extract as X
    from anomalyclip_amd import init_weights as IW
    from anomalyclip_amd.components.anomaly_clip import geometry_of_arch
    dev = torch.device("cuda", torch.cuda.current_device())
    geom = geometry_of_arch(args.arch)
    with torch.device(dev):
        enc = X.build_image_encoder(args.arch, args.precision)
    init = IW.init_resnet_state_dict if geom.is_resnet else IW.init_vit_state_dict
    enc.load_state_dict(init(geom, 1, prefix=""), strict=True)
    enc.eval()
    launches = [0]
    fwd = enc.forward

    def counted(x):
        launches[0] += 1
        return fwd(x)

    enc.forward = counted
    tmp = tempfile.mkdtemp(prefix="acx_extract_pack_")
    lines = []
    try:
        root = os.path.join(tmp, "frames")
        t0 = time.perf_counter()
        lens = write_short_clips(root)
        print(f"{sum(lens)} frames in {len(lens)} folders written in {time.perf_counter() - t0:.1f} s", file=sys.stderr)
        warm = os.path.join(tmp, "warm.txt")
        with open(warm, "w") as fh:
            fh.write("".join(f"clip{v:03d} 0 {lens[v] - 1} 0\n" for v in range(4)))
        for ncrops in (1, 10):
            for decode in ("pil", "gpu_entropy"):
                rows = sum(lens) * ncrops
                for pack in (False, True):                                     # both arms once on four clips, untimed
                    X.extract_dataset(enc, warm, root, os.path.join(tmp, "w"), ncrops, overwrite=True, decode=decode, pack=pack,
                                      decode_threads=args.decode_threads)
                torch.cuda.synchronize()
                secs, calls = {False: [], True: []}, {}
                for rep in range(PACK_REPS):
                    for pack in (False, True):
                        out = os.path.join(tmp, f"o_{ncrops}_{decode}_{int(pack)}_{rep}")
                        launches[0] = 0
                        t0 = time.perf_counter()
                        counts = X.extract_dataset(enc, None, root, out, ncrops, decode=decode, pack=pack,
                                                   decode_threads=args.decode_threads)
                        torch.cuda.synchronize()
                        secs[pack].append(time.perf_counter() - t0)
                        assert counts["written"] == len(lens) and counts["rows"] == rows, counts
                        calls[pack] = launches[0]
                        shutil.rmtree(out, ignore_errors=True)
                spread = abs(secs[False][0] - secs[False][1])
                gain = min(secs[False]) - max(secs[True])
                res = {"tool": "bench_extract --pack", "arch": args.arch, "precision": args.precision, "ncrops": ncrops, "decode": decode,
                       "folders": len(lens), "frames": sum(lens), "rows": rows, "sizes": [list(s) for s in PACK_SIZES],
                       "decode_threads": args.decode_threads, "rows_per_launch": X.batch_frames(enc, ncrops) * ncrops,
                       "unpacked_s": [round(t, 3) for t in secs[False]], "packed_s": [round(t, 3) for t in secs[True]],
                       "unpacked_rows_per_s": [round(rows / t, 1) for t in secs[False]],
                       "packed_rows_per_s": [round(rows / t, 1) for t in secs[True]],
                       "unpacked_launches": calls[False], "packed_launches": calls[True],
                       "unpacked_spread_s": round(spread, 3), "slower_packed_minus_faster_unpacked_s": round(-gain, 3),
                       "condition_met": bool(gain > spread),
                       "boundary_ms": round((sum(secs[False]) - sum(secs[True])) / PACK_REPS / len(lens) * 1e3, 2),
                       "gpu": torch.cuda.get_device_name(dev), "cpu": cpu_model()}
                lines.append(json.dumps(res))
                print(lines[-1], flush=True)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "a") as fh:
                        fh.write(lines[-1] + "\n")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="ViT-B/16")
    ap.add_argument("--precision", default="auto")
    ap.add_argument("--ncrops", type=int, default=10, choices=(1, 5, 10))
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--hw", default="240x320")
    ap.add_argument("--scale-size", type=int, default=None)
    ap.add_argument("--decode-threads", type=int, default=8)
    ap.add_argument("--kernel-only", action="store_true", help="time the crop kernel alone (no encoder is built)")
    ap.add_argument("--crop-size", type=int, default=224, help="--kernel-only: the crop size")
    ap.add_argument("--dtype", default="float32", choices=("float32", "float16"),
                    help="element type of the files written (legs b and c; not with --pack or --kernel-only)")
    ap.add_argument("--pack", action="store_true", help="pack off against pack on over 64 short clips (extract_pack_bench.jsonl)")
    ap.add_argument("--out", default=None, help="default: profiles/extract_bench.jsonl, with --pack profiles/extract_pack_bench.jsonl")
    args = ap.parse_args()
    if args.out is None:
        args.out = os.path.join(REPO, "profiles", "extract_pack_bench.jsonl" if args.pack else "extract_bench.jsonl")
    if args.pack:
        pack_leg(args)
        return
    H, W = (int(v) for v in args.hw.split("x"))
    from anomalyclip_amd import extract as X
    from anomalyclip_amd import init_weights as IW
    from anomalyclip_amd.components.anomaly_clip import geometry_of_arch
    from anomalyclip_amd.preprocess import default_scale_size
    dev = torch.device("cuda", torch.cuda.current_device())
    res = {"tool": "bench_extract", "ncrops": args.ncrops, "hw": [H, W], "gpu": torch.cuda.get_device_name(dev), "cpu": cpu_model()}

    if args.kernel_only:
        crop = args.crop_size
        scale = args.scale_size or default_scale_size(crop, args.ncrops)
        nf = max(1, 512 // args.ncrops)
        fr = torch.from_numpy(synthetic_frames(nf, H, W)).to(dev)
        ms = crop_kernel_ms(fr, crop, scale, args.ncrops)
        rows = nf * args.ncrops
        res.update({"kernel_only": True, "crop": crop, "scale": scale, "rows": rows, "crop_kernel_ms": round(ms, 4),
                    "crop_kernel_ms_per_512_rows": round(ms * 512 / rows, 4),
                    "write_GBps": round(rows * 3 * crop * crop * 4 / ms / 1e6, 1)})
    else:
        geom = geometry_of_arch(args.arch)
        with torch.device(dev):
            enc = X.build_image_encoder(args.arch, args.precision)
        init = IW.init_resnet_state_dict if geom.is_resnet else IW.init_vit_state_dict
        enc.load_state_dict(init(geom, 1, prefix=""), strict=True)
        enc.eval()
        crop, chunk = enc.input_resolution, enc.chunk
        scale = args.scale_size or default_scale_size(crop, args.ncrops)
        nb = X.batch_frames(enc, args.ncrops)
        rows_total = args.frames * args.ncrops
        res.update({"arch": args.arch, "precision": args.precision, "frames": args.frames, "rows": rows_total, "crop": crop,
                    "scale": scale, "rows_per_launch": nb * args.ncrops, "decode_threads": args.decode_threads, "dtype": args.dtype})
        host = synthetic_frames(args.frames, H, W)
        # (a) the encoder alone: the launches extract_video makes (nb * ncrops rows each, the ragged last one included)
        x = torch.randn(nb * args.ncrops, 3, crop, crop, device=dev)
        spans = [min(nb, args.frames - i) * args.ncrops for i in range(0, args.frames, nb)]
        with torch.no_grad():
            enc(x)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for n in spans:
                enc(x[:n])
            torch.cuda.synchronize()
            dt_a = time.perf_counter() - t0
        res["a_encoder_rows_per_s"] = round(rows_total / dt_a, 1)
        res["a_ms_per_launch"] = round(dt_a / len(spans) * 1e3, 3)
        res["crop_kernel_ms_per_512_rows"] = round(crop_kernel_ms(torch.from_numpy(host[:nb]).to(dev), crop, scale, args.ncrops)
                                                   * 512 / (nb * args.ncrops), 4)
        tmp = tempfile.mkdtemp(prefix="acx_extract_bench_")
        try:
            # (b) pre-decoded frames in pinned memory
            pinned = torch.from_numpy(host).pin_memory()
            X.extract_video(enc, pinned[:nb], os.path.join(tmp, "warm.npy"), args.ncrops, scale, overwrite=True, dtype=args.dtype)
            t0 = time.perf_counter()
            X.extract_video(enc, pinned, os.path.join(tmp, "b.npy"), args.ncrops, scale, overwrite=True, dtype=args.dtype)
            dt_b = time.perf_counter() - t0
            res["b_file_bytes"] = os.path.getsize(os.path.join(tmp, "b.npy"))
            res["b_predecoded_rows_per_s"] = round(rows_total / dt_b, 1)
            res["b_over_a"] = round(dt_a / dt_b, 4)
            # (c) from JPEG folders
            from PIL import Image
            vdir = os.path.join(tmp, "frames", "v")
            os.makedirs(vdir)
            for t in range(args.frames):
                Image.fromarray(host[t]).save(os.path.join(vdir, X.TEMPLATE.format(t)), quality=90)
            t0 = time.perf_counter()
            counts = X.extract_dataset(enc, None, os.path.join(tmp, "frames"), os.path.join(tmp, "feats"), args.ncrops, scale,
                                       decode_threads=args.decode_threads, dtype=args.dtype)
            dt_c = time.perf_counter() - t0
            assert counts["rows"] == rows_total, counts
            res["c_jpeg_rows_per_s"] = round(rows_total / dt_c, 1)
            res["c_jpeg_frames_per_s"] = round(args.frames / dt_c, 1)
            res["c_over_a"] = round(dt_a / dt_c, 4)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
