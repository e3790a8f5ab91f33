"""Wall time of the end-of-epoch `Trainer.save_checkpoint` at the UCF-Crime config (ViT-B/16 towers in the state_dict, 256-wide
head, AcxAdamW moments allocated by two training steps; without a GPU the module stays on the host, the moments are filled with
noise and the numbers are the host side of the save alone): median of `--saves` saves of the resumable file against the same number of
saves of the weights-only layout (the keys written before resume existed: the same call without an optimizer), alternating in
one process.  Prints one JSON line.

    python tools/bench_checkpoint_save.py [--saves 5] [--dir DIR]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from functools import partial

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

import torch  # noqa: E402

import bench  # noqa: E402
from anomalyclip_amd.anomaly_clip_module import AnomalyCLIPModule  # noqa: E402
from anomalyclip_amd.components.loss import ComputeLoss  # noqa: E402
from anomalyclip_amd.components.scheduler import WarmupCosineAnnealingLR  # noqa: E402
from anomalyclip_amd.optim import AcxAdamW  # noqa: E402
from anomalyclip_amd.trainer import Trainer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--saves", type=int, default=5)
    ap.add_argument("--dir", default=None, help="where the files are written (default: the system's temporary directory)")
    args = ap.parse_args()
    dev = torch.device("cuda", 0) if torch.cuda.is_available() else torch.device("cpu")
    net, _, _, _ = bench.build_net("auto", dev)
    net.load_from_features = True
    crit = ComputeLoss(7, 3, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, 16, 32)
    mod = AnomalyCLIPModule(net, partial(AcxAdamW, weight_decay=0.2), partial(WarmupCosineAnnealingLR, warmup_epochs=5, total_epoch=50),
                            crit, num_classes=14, solver={"lr": 1e-5}).to(dev)
    mod.ncentroid = torch.zeros(512, device=dev)
    net.train()
    trainers = {"weights_only": Trainer(max_epochs=50), "resumable": Trainer(max_epochs=50)}
    object.__setattr__(mod, "trainer", trainers["resumable"])
    cfg = mod.configure_optimizers()
    opt = cfg["optimizer"]
    if dev.type == "cuda":
        batch, _ = bench.head_batch(8, 1, 0, dev)
        for i in range(2):
            mod.train_batch(batch, opt, i)
    else:
        for p in mod.trainable_parameters():
            if p is not net.selector_model.logit_scale:
                opt.state[p].update(step=2, exp_avg=torch.randn_like(p), exp_avg_sq=torch.rand_like(p))
    sync = torch.cuda.synchronize if dev.type == "cuda" else (lambda: None)
    sync()
    trainers["resumable"]._optimizer, trainers["resumable"]._scheduler = opt, cfg["lr_scheduler"]["scheduler"]
    times, sizes = {k: [] for k in trainers}, {}
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        for rep in range(args.saves + 1):                      # the first round warms up
            for name, tr in trainers.items():
                path = os.path.join(d, name, "checkpoints", "last.ckpt")
                sync()
                t0 = time.perf_counter()
                tr.save_checkpoint(mod, path)
                dt = time.perf_counter() - t0
                if rep:
                    times[name].append(dt)
                sizes[name] = os.path.getsize(path)
    med = {k: statistics.median(v) for k, v in times.items()}
    print(json.dumps({"device": dev.type, "median_s": med, "all_s": times, "bytes": sizes, "ratio_time": med["resumable"] / med["weights_only"],
                      "ratio_bytes": sizes["resumable"] / sizes["weights_only"]}))


if __name__ == "__main__":
    main()
