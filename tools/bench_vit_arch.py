"""Frames/s of the CLIP image encoder per `net.arch` backbone and precision, with the library's per-kind kernel times.

    python tools/bench_vit_arch.py --arch ViT-L/14 --precision auto --frames 512 [--steps 5 --warmup 2]
    python tools/bench_vit_arch.py --arch ViT-B/16 --frames 512 --precision auto --act quick_gelu,gelu --reps 2
    python tools/bench_vit_arch.py --arch ViT-L/14 --frames 512 --precision auto,f16x3s --reps 2

`--act A[,B]` names the MLP's activation (quick_gelu, gelu) and `--precision P[,Q...]` the precision (auto, f32, bf16, f32x6, f16x3,
f16x3s); several activations or precisions and / or `--reps N` time the legs ALTERNATELY in one process (A B A B ...: clock and
thermal drift hit both alike), one JSON line with every leg's frames/s and the spread of each arm's legs -- the run-to-run spread a
difference has to exceed.  With several precisions the line also carries every precision's feature distance from the "f32" run of
the same frames (max |a - f32| / max |f32|, and the mean absolute difference).

One launch of `--frames` frames (seeded random weights and frames) is timed with HIP events after the warm-up; a separate profiled
pass (acx_prof_*: HIP-event pairs around every kernel, summed by kind) gives attention / GEMM / other times and the GEMMs'
throughput.  `gemm_tflops` counts 2 M N K once per product (f32-equivalent, as bench.py does); `gemm_frac_of_roof` divides it by
the precision's roof, as bench.py's roofline does: f32 157.3 TFLOP/s, bf16 2.5 PFLOP/s dense, auto 2.5 / 6 PFLOP/s (a pairs = 6
product is six bf16 products -- gemm_frac_of_roof is then also the fraction of the bf16 matrix cores' roof the planes keep busy).
Prints one JSON line."""
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
from anomalyclip_amd.components.clip_vit import VisionTransformer  # noqa: E402

PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0, "auto": 2500.0 / 6, "f32x6": 2500.0 / 6, "f16x3": 2500.0 / 3, "f16x3s": 2500.0 / 3}   # MI355X dense MFMA (bench.py's roofs)


def macs_per_frame(g):
    T = g.grid ** 2
    Lt, W = T + 1, g.vision_width
    patch = T * 3 * g.vision_patch_size ** 2 * W
    layer = Lt * 12 * W * W + 2 * Lt * Lt * W       # in/out projections + MLP, QK^T + PV
    return patch + g.vision_layers * layer + W * g.embed_dim


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="ViT-L/14", choices=["ViT-B/16", "ViT-B/32", "ViT-L/14", "ViT-L/14@336px", "ViT-H-14"])
    ap.add_argument("--precision", default="auto", help="auto | f32 | bf16 | f32x6 | f16x3 | f16x3s, or several separated by commas: alternating legs")
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--act", default=None, help="quick_gelu | gelu, or both separated by a comma: alternating legs (default: the arch's own)")
    ap.add_argument("--reps", type=int, default=1, help="legs per activation")
    a = ap.parse_args()
    g = geometry_of_arch(a.arch)
    acts = (a.act or g.act).split(",")
    if any(t not in ("quick_gelu", "gelu") for t in acts) or a.reps < 1:
        ap.error("--act takes quick_gelu, gelu or both separated by a comma; --reps >= 1")
    precs = a.precision.split(",")
    if any(t not in PEAK_TFLOPS for t in precs):
        ap.error("--precision takes " + ", ".join(PEAK_TFLOPS) + " or several of them separated by commas")
    a.precision = precs[0]
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    vit = VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim,
                            precision=a.precision, chunk=a.frames, arch=a.arch, act=acts[0])
    vit.load_state_dict(IW.init_vit_state_dict(g, 0, prefix=""), strict=True)
    vit = vit.to(dev)
    x = torch.randn(a.frames, 3, g.image_resolution, g.image_resolution, generator=torch.Generator().manual_seed(1)).to(dev)
    t0 = time.time()
    for _ in range(a.warmup):
        vit(x)
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(a.steps):
        out = vit(x)
    ev[1].record()
    torch.cuda.synchronize()
    ms = ev[0].elapsed_time(ev[1]) / a.steps
    if len(acts) > 1 or len(precs) > 1 or a.reps > 1:
        return alternate(a, vit, x, acts, precs, t0)
    # profiled pass: per-kind kernel times
    lib, h = L.lib(), L.ctx(0)
    lib.acx_prof_enable(h, 1)
    vit(x)
    torch.cuda.synchronize()
    lib.acx_prof_enable(h, 0)
    gf = ctypes.c_double(0.0)
    L.check(lib.acx_prof_gemm_flops(h, ctypes.byref(gf)), h)
    counts, tot = (ctypes.c_int32 * 4)(), (ctypes.c_double * 4)()
    L.check(lib.acx_prof_collect(h, counts, tot), h)
    kinds = ["gemm", "attention", "norm", "other"]
    kt = {k: round(tot[i], 3) for i, k in enumerate(kinds)}
    gemm_tflops = gf.value / 1e9 / tot[0] if tot[0] > 0 else None
    res = {"arch": a.arch, "precision": a.precision, "frames": a.frames, "tokens": g.grid ** 2 + 1,
           "frames_per_s": round(a.frames / (ms / 1e3), 1), "ms_per_launch": round(ms, 3),
           "gmac_per_frame": round(macs_per_frame(g) / 1e9, 2),
           "kernel_ms": {"attention": kt["attention"], "gemm": kt["gemm"], "other": round(kt["norm"] + kt["other"], 3)},
           "kernel_launches": {k: int(counts[i]) for i, k in enumerate(kinds)},
           "gemm_tflops": round(gemm_tflops, 1) if gemm_tflops else None,
           "gemm_roof_tflops": round(PEAK_TFLOPS[a.precision], 1),
           "gemm_frac_of_roof": round(gemm_tflops / PEAK_TFLOPS[a.precision], 4) if gemm_tflops else None,
           "finite": bool(torch.isfinite(out).all()), "wall_s": round(time.time() - t0, 1)}
    print(json.dumps(res))


def alternate(a, vit, x, acts, precs, t0):
    """legs of a.steps launches each, the arms (precision x activation) in turn, a.reps rounds; every leg behind a.warmup launches of
    its own"""
    arms = [(p, act) for p in precs for act in acts]
    name = (lambda p, act: act) if len(precs) == 1 else (lambda p, act: p) if len(acts) == 1 else (lambda p, act: f"{p}/{act}")
    legs = []
    for r in range(a.reps):
        for p, act in arms:
            vit.precision = p
            vit.act = vit.transformer.act = act
            for _ in range(a.warmup):
                vit(x)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(a.steps):
                out = vit(x)
            ev[1].record()
            torch.cuda.synchronize()
            ms = ev[0].elapsed_time(ev[1]) / a.steps
            legs.append({"arm": name(p, act), "precision": p, "act": act, "rep": r, "ms_per_launch": round(ms, 3),
                         "frames_per_s": round(a.frames / (ms / 1e3), 1), "finite": bool(torch.isfinite(out).all())})
    names = [name(p, act) for p, act in arms]
    by = {n: [l["frames_per_s"] for l in legs if l["arm"] == n] for n in names}
    res = {"arch": a.arch, "precision": ",".join(precs), "frames": a.frames, "steps": a.steps, "legs": legs,
           "frames_per_s": {n: round(sum(v) / len(v), 1) for n, v in by.items()},
           "spread": {n: round((max(v) - min(v)) / (sum(v) / len(v)), 5) for n, v in by.items()}}
    if len(names) == 2:
        m = res["frames_per_s"]
        res["ratio"] = {f"{names[1]}/{names[0]}": round(m[names[1]] / m[names[0]], 5)}
    if len(precs) > 1:                                   # the features' distance from the f32 MFMA kernels' on the same frames
        vit.act = vit.transformer.act = acts[0]
        vit.precision = "f32"
        ref = vit(x).double()
        dist = {}
        for p in precs:
            vit.precision = p
            d = (vit(x).double() - ref).abs()
            dist[p] = {"max_rel": float(d.max() / ref.abs().max()), "mean_abs": float(d.mean())}
        res["distance_from_f32"] = dist
    res["wall_s"] = round(time.time() - t0, 1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
