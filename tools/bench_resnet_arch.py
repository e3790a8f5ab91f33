"""Frames/s of the CLIP ResNet image encoders (RN50, RN101, RN50x4, RN50x16, RN50x64) per precision, with the library's per-kind
kernel times.

    python tools/bench_resnet_arch.py --arch RN50 --precision auto --frames 512 [--steps 5 --warmup 2]
    python tools/bench_resnet_arch.py --arch RN50 --precision f32,bf16x6 --reps 2 --frames 512     (A/B in one process)

One call of `--frames` frames (seeded random weights and frames) is timed with HIP events after the warm-up; a separate profiled
pass (acx_prof_*: HIP-event pairs around every kernel, summed by kind) gives GEMM / attention / other times.  `gmac_per_frame`
counts the multiply-adds of every convolution (unpadded channels), the attention pool's projections and its attention, from the
shapes; `gemm_tflops` is what the profiled GEMMs executed (padded channels included) over their time, against the f32 MFMA roof
(157.3 TFLOP/s: "auto" runs the f32 kernels for the ResNets; "bf16x6" runs most products on the bf16 matrix cores, so its fraction
of that roof can exceed 1).  `--precision a,b --reps R`: the precisions ALTERNATE on one module in one process (a b a b ...), R
repetitions each.  Prints one JSON line per measurement."""
import argparse
import ctypes
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from anomalyclip_amd import _lib as L  # noqa: E402
from anomalyclip_amd import init_weights as IW  # noqa: E402
from anomalyclip_amd.components.anomaly_clip import geometry_of_arch  # noqa: E402
from anomalyclip_amd.components.clip_resnet import ModifiedResNet  # noqa: E402

F32_ROOF_TFLOPS = 157.3


def macs_per_frame(g):
    w, G = g.vision_width, g.image_resolution // 2
    m = G * G * (27 * (w // 2) + 9 * (w // 2) * (w // 2) + 9 * (w // 2) * w)
    H, inpl = G // 2, w
    for li, blocks in enumerate(g.vision_layers):
        planes = w * 2 ** li
        for j in range(blocks):
            m += H * H * (inpl * planes + 9 * planes * planes)
            if li > 0 and j == 0:
                H //= 2
            m += H * H * planes * 4 * planes
            if j == 0:
                m += H * H * inpl * 4 * planes
            inpl = 4 * planes
    E, Lt = 32 * w, H * H + 1
    return m + Lt * 2 * E * E + E * E + 2 * Lt * E + E * g.embed_dim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="RN50", choices=["RN50", "RN101", "RN50x4", "RN50x16", "RN50x64"])
    ap.add_argument("--precision", default="auto", help="auto, f32 or bf16x6; two or more separated by commas alternate in this process")
    ap.add_argument("--reps", type=int, default=1, help="repetitions of every precision")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    a = ap.parse_args()
    precisions = a.precision.split(",")
    for p in precisions:
        if p not in ("auto", "f32", "bf16x6"):
            ap.error(f"--precision {p}: one of auto, f32, bf16x6")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = geometry_of_arch(a.arch)
    with torch.device(dev):
        m = ModifiedResNet(g.vision_layers, g.embed_dim, g.resnet_heads, g.image_resolution, g.vision_width,
                           precision=precisions[0], chunk=a.frames, arch=a.arch)
    m.load_state_dict(IW.init_resnet_state_dict(g, 0, prefix=""), strict=True)
    m.eval()
    x = torch.randn(a.frames, 3, g.image_resolution, g.image_resolution, generator=torch.Generator().manual_seed(1)).to(dev)
    for rep in range(a.reps):
        for p in precisions:
            m.precision = p
            res = measure(a, g, m, x)
            res["precision"], res["rep"] = p, rep
            print(json.dumps(res), flush=True)


def measure(a, g, m, x):
    t0 = time.time()
    for _ in range(a.warmup):
        m(x)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(a.steps):
        out = m(x)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / a.steps
    lib, h = L.lib(), L.ctx(0)
    lib.acx_prof_enable(h, 1)
    m(x)
    torch.cuda.synchronize()
    lib.acx_prof_enable(h, 0)
    gf = ctypes.c_double(0.0)
    L.check(lib.acx_prof_gemm_flops(h, ctypes.byref(gf)), h)
    counts, tot = (ctypes.c_int32 * 4)(), (ctypes.c_double * 4)()
    L.check(lib.acx_prof_collect(h, counts, tot), h)
    kinds = ["gemm", "attention", "norm", "other"]
    kt = {k: round(tot[i], 3) for i, k in enumerate(kinds)}
    gemm_tflops = gf.value / 1e9 / tot[0] if tot[0] > 0 else None
    macs = macs_per_frame(g)
    res = {"arch": a.arch, "precision": m.precision, "frames": a.frames, "steps": a.steps, "warmup": a.warmup, "frames_per_s": round(a.frames / (ms / 1e3), 1),
           "ms_per_call": round(ms, 3), "gmac_per_frame": round(macs / 1e9, 2),
           "model_tflops": round(2 * macs * a.frames / (ms / 1e3) / 1e12, 1),
           "kernel_ms": {"gemm": kt["gemm"], "attention": kt["attention"], "other": round(kt["norm"] + kt["other"], 3)},
           "kernel_launches": {k: int(counts[i]) for i, k in enumerate(kinds)},
           "gemm_tflops": round(gemm_tflops, 1) if gemm_tflops else None, "gemm_roof_tflops": F32_ROOF_TFLOPS,
           "gemm_frac_of_roof": round(gemm_tflops / F32_ROOF_TFLOPS, 4) if gemm_tflops else None,
           "finite": bool(torch.isfinite(out).all()), "wall_s": round(time.time() - t0, 1)}
    return res


if __name__ == "__main__":
    main()
