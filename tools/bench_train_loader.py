#!/usr/bin/env python
"""Training batches from feature files: the resident feature set (anomalyclip_amd.feature_bank) against a host loader.

Synthetic `.npy` files in a temporary directory (page cache, so the numbers are the loaders', not the disk's), then
  1. the gather of ONE batch (acx_sample_segments): HIP-event time, and its GB/s (bytes read + bytes written) next to a
     device-to-device copy of the same bytes timed in the same run, the two alternating;
  2. steps/s of Trainer.fit on the UCF head fed (a) by AnomalyCLIPDataModule's resident loaders and (b) by a host loader --
     the files held in RAM, one numpy gather per video (feature_index) straight into pinned memory, `.to(device)` -- in the
     same run.  (b) is the best a user can write without the bank; the reference's per-frame Python loop is slower still.
--dtype float16 writes half-precision files: the bank holds halves and the gather widens them (part 2 then times the resident
loaders only: the host loader of (b) gathers float32 rows).  tools/bench_feature_f16.py times both dtypes in one process.
One JSON line.   python tools/bench_train_loader.py [--videos 256] [--frames 2000] [--batch 64] [--steps 40] [--dtype float16]"""
import argparse, json, os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch


class HostTrainLoader:
    """the same index stream as ResidentTrainLoader (same samplers, same draws); rows gathered on the host"""

    def __init__(self, arrays, plan, N, L, stride):
        self.arrays, self.plan, self.N, self.L, self.stride = arrays, plan, N, L, stride
        self.pinned = None

    def __len__(self):
        return len(self.plan)

    def __iter__(self):
        from anomalyclip_amd import feature_index as FI
        for vid, starts, labels in self.plan.host_batches():
            b, D = len(vid), self.arrays[0].shape[1]
            if self.pinned is None:
                self.pinned = [torch.empty(b, 1, self.N * self.L, D).pin_memory() for _ in range(2)]
                self.turn = 0
            buf = self.pinned[self.turn]
            self.turn ^= 1
            host = buf.numpy()
            for i, v in enumerate(vid):
                a = self.arrays[v]
                idx = FI.frame_index_table(starts[i * self.N:(i + 1) * self.N].astype(np.int64), self.L, self.stride, a.shape[0])
                np.take(a, idx, axis=0, out=host[i, 0])
            # Trainer.fit moves the batch with .to(device, non_blocking=True); the pinned buffer is reused two batches later, after
            # the step that consumed it has been enqueued and the copy before it has long finished
            yield buf, torch.from_numpy(labels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, default=256)
    ap.add_argument("--frames", type=int, default=2000, help="mean frames per video (lengths are drawn in [frames/2, 3 frames/2])")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--steps", type=int, default=40, help="timed training steps per loader")
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--gather-reps", type=int, default=50)
    ap.add_argument("--dtype", default="float32", choices=("float32", "float16"), help="element type of the feature files")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_train_loader.py measures on the GPU"
    import bench as B
    from anomalyclip_amd import ops
    from anomalyclip_amd.anomaly_clip_module import AnomalyCLIPModule
    from anomalyclip_amd.components.loss import ComputeLoss
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    from anomalyclip_amd.feature_bank import ResidentTrainLoader
    from anomalyclip_amd.trainer import Trainer
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    rng = np.random.default_rng(0)
    V, D, N, L = args.videos, 512, 32, 16
    half = args.batch // 2
    steps_per_epoch = (V // 2) // half
    assert steps_per_epoch >= 1, "--videos must be at least --batch"
    epochs = -(-(args.steps + args.warmup) // steps_per_epoch)
    with tempfile.TemporaryDirectory() as td:
        lengths = [int(t) for t in rng.integers(args.frames // 2, args.frames * 3 // 2 + 1, size=V)]
        lists = {k: os.path.join(td, k + ".txt") for k in ("normal", "anomaly")}
        with open(lists["normal"], "w") as fn, open(lists["anomaly"], "w") as fa:
            for i, T in enumerate(lengths):
                np.save(os.path.join(td, f"v{i}.npy"), (rng.standard_normal((T, D)) * 0.3).astype(args.dtype))
                (fn if i < V // 2 else fa).write(f"v{i} 0 {T - 1} {7 if i < V // 2 else i % 7}\n")
        hp = dict(frames_root=td, annotation_file_normal=lists["normal"], annotation_file_anomaly=lists["anomaly"],
                  annotation_file_test=lists["anomaly"], normal_id=7, num_classes=14, num_segments=N, seg_length=L, batch_size=args.batch,
                  device=dev)
        dm = AnomalyCLIPDataModule(**hp)
        t0 = time.perf_counter()
        dm.setup("fit")
        torch.cuda.synchronize()
        load_s = time.perf_counter() - t0
        bank = dm.bank

        # ---- 1. one batch's gather against a device-to-device copy of the same bytes
        plan = ResidentTrainLoader(bank, range(V), args.batch, N, L, 1, rng=np.random.RandomState(1),
                                   generator=torch.Generator().manual_seed(1))
        vid, starts, _ = next(plan.host_batches())
        vid_d, starts_d = torch.from_numpy(vid).to(dev), torch.from_numpy(starts).to(dev)
        out = torch.empty(args.batch, 1, N * L, D, device=dev)
        dst = torch.empty_like(out)
        moved = 2 * out.numel() * 4                                    # bytes read + bytes written by the copy ...
        moved_g = out.numel() * (4 + bank.bank.element_size())         # ... and by the gather (a float16 bank: 2 read, 4 written)
        ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(2 * args.gather_reps)]
        for _ in range(5):
            ops.sample_segments(bank.bank, bank.row_off, bank.frames, vid_d, starts_d, N, L, 1, 1, out=out)
            dst.copy_(out)
        for r in range(args.gather_reps):
            ev[2 * r][0].record()
            ops.sample_segments(bank.bank, bank.row_off, bank.frames, vid_d, starts_d, N, L, 1, 1, out=out)
            ev[2 * r][1].record()
            ev[2 * r + 1][0].record()
            dst.copy_(out)
            ev[2 * r + 1][1].record()
        torch.cuda.synchronize()
        g_ms = sorted(ev[2 * r][0].elapsed_time(ev[2 * r][1]) for r in range(args.gather_reps))
        c_ms = sorted(ev[2 * r + 1][0].elapsed_time(ev[2 * r + 1][1]) for r in range(args.gather_reps))
        med = lambda v: v[len(v) // 2]
        assert torch.equal(dst, out)

        # ---- 2. Trainer.fit: resident loaders against the host loader
        def module():
            net, sd, eot, hc = B.build_net("auto", dev)
            net.load_from_features = True
            crit = ComputeLoss(hc.normal_id, 3, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, L, N)
            mod = AnomalyCLIPModule(net, None, None, crit, num_classes=hc.num_classes, solver={"lr": 1e-5},
                                    save_dir=os.path.join(td, "run")).to(dev)
            return mod

        def timed_fit(mod, datamodule):
            stamps, step = [], mod.train_batch

            def stamped(batch, opt, i=0):
                if len(stamps) == args.warmup:
                    torch.cuda.synchronize()
                    stamps.append(time.perf_counter())
                else:
                    stamps.append(None)
                return step(batch, opt, i)
            mod.train_batch = stamped
            Trainer(max_epochs=epochs, check_val_every_n_epoch=epochs + 1).fit(mod, datamodule)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            del mod.train_batch
            n = len(stamps) - args.warmup
            return n, t1 - stamps[args.warmup]

        mod = module()
        n_res, s_res = timed_fit(mod, dm)
        if args.dtype != "float32":
            print(json.dumps({
                "row": "training batches from a resident feature set", "dtype": args.dtype, "videos": V, "frames_mean": args.frames,
                "batch": args.batch, "bank": {"bytes": bank.nbytes, "load_s": round(load_s, 3), "GBps": round(bank.nbytes / load_s / 1e9, 2)},
                "gather_one_batch": {"bytes_moved": moved_g, "ms_median": round(med(g_ms), 4), "ms_min": round(g_ms[0], 4),
                                     "GBps": round(moved_g / med(g_ms) / 1e6, 1)},
                "d2d_copy_same_rows_f32": {"ms_median": round(med(c_ms), 4), "ms_min": round(c_ms[0], 4)},
                "fit_resident": {"steps": n_res, "steps_per_s": round(n_res / s_res, 2), "ms_per_step": round(s_res / n_res * 1e3, 3)}}))
            return
        arrays = [np.load(r.path) for r in dm.normal + dm.anomaly]
        kw = dict(batch_size=half, num_segments=N, seg_length=L, stride=1)
        host_loaders = [HostTrainLoader(arrays, ResidentTrainLoader(bank, ids, **kw), N, L, 1) for ids in (range(V // 2), range(V // 2, V))]
        from types import SimpleNamespace
        dm_host = SimpleNamespace(hparams=dm.hparams, num_classes=14, setup=lambda stage: None, train_dataloader=lambda: host_loaders,
                                  train_dataloader_test_mode=dm.train_dataloader_test_mode)
        n_host, s_host = timed_fit(mod, dm_host)                       # (same module: graphs captured, ncentroid.pt on disk)
    print(json.dumps({
        "row": "training batches from a resident feature set", "videos": V, "frames_mean": args.frames, "batch": args.batch,
        "bank": {"bytes": bank.nbytes, "load_s": round(load_s, 3), "GBps": round(bank.nbytes / load_s / 1e9, 2)},
        "gather_one_batch": {"bytes_moved": moved, "ms_median": round(med(g_ms), 4), "ms_min": round(g_ms[0], 4),
                             "GBps": round(moved / med(g_ms) / 1e6, 1)},
        "d2d_copy_same_bytes": {"ms_median": round(med(c_ms), 4), "ms_min": round(c_ms[0], 4), "GBps": round(moved / med(c_ms) / 1e6, 1)},
        "fit_resident": {"steps": n_res, "steps_per_s": round(n_res / s_res, 2), "ms_per_step": round(s_res / n_res * 1e3, 3)},
        "fit_host_loader": {"steps": n_host, "steps_per_s": round(n_host / s_host, 2), "ms_per_step": round(s_host / n_host * 1e3, 3)}}))


if __name__ == "__main__":
    main()
