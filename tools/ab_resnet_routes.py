"""A/B of the ResNet encoder's routing rule at precision "bf16x6" (csrc/acx_resnet.hip rn_routed), one product class at a time, both
arms ALTERNATING in one process on one device, with the split launches each arm needs:

    conv1 (1x1, K = 4 planes or the block's input, N = planes; its input is the block input, f32):
        plane arm   acx_split_bf16x3(x [M, K])  +  pairs = 6 product, ReLU -> planes (conv2's A operand)
        f32 arm     f32 product, ReLU -> f32     +  acx_split_bf16x3(t1 [M, N])      (conv2 runs on planes either way)
    conv3 (1x1, K = planes, N = 4 planes, + identity, ReLU; its input comes from conv2):
        plane arm   pairs = 6 product on conv2's planes, ReLU after the residual -> f32
        f32 arm     f32 product on conv2's f32 rows (conv2 writes f32 instead of planes: no extra launch)

    python tools/ab_resnet_routes.py --arch RN50 --frames 512 [--reps 2 --steps 5]

Prints one JSON line per (layer, class, arm, repetition): the rows, K, N and the time per call of the arm's launches (HIP events)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from anomalyclip_amd import _lib as L  # noqa: E402
from anomalyclip_amd import ops  # noqa: E402
from anomalyclip_amd.components.anomaly_clip import geometry_of_arch  # noqa: E402


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    for _ in range(steps):
        fn()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1]) / steps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", default="RN50", choices=["RN50", "RN101", "RN50x4", "RN50x16", "RN50x64"])
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--steps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    g = geometry_of_arch(a.arch)
    w = g.vision_width
    H = g.image_resolution // 4
    gen = torch.Generator(device=dev).manual_seed(0)
    for li in range(4):
        planes = w << li
        pp = (planes + 31) // 32 * 32
        if li > 0:
            H //= 2                                               # (the blocks after the layer's first: the common case)
        frames = a.frames
        while frames * H * H * 4 * planes * 4 >= 1 << 31:         # the driver's internal batches
            frames = (frames + 1) // 2
        M, K1, N3 = frames * H * H, 4 * planes, 4 * planes
        x = torch.randn(M, K1, generator=gen, device=dev)
        w1 = torch.randn(pp, K1, generator=gen, device=dev) * K1 ** -0.5
        w3 = torch.randn(N3, pp, generator=gen, device=dev) * pp ** -0.5
        b1, b3 = torch.zeros(pp, device=dev), torch.zeros(N3, device=dev)
        w1p, w3p = ops.split_bf16x3(w1), ops.split_bf16x3(w3)
        xp = torch.empty(3, M, K1, dtype=torch.bfloat16, device=dev)
        t1 = torch.empty(M, pp, device=dev)
        t1p = torch.empty(3, M, pp, dtype=torch.bfloat16, device=dev)
        out = torch.empty(M, N3, device=dev)

        def conv1_planes():
            ops.split_bf16x3(x, out=xp)
            ops.gemm_x6(xp, w1p, bias=b1, act=L.ACT_RELU, planes_out=True, out=t1p, split_k=False)

        def conv1_f32():
            ops.gemm(x, w1, bias=b1, act=L.ACT_RELU, out=t1)
            ops.split_bf16x3(t1, out=t1p)

        def conv3_planes():
            ops.gemm_x6(t1p, w3p, bias=b3, act=L.ACT_RESRELU, residual=x, out=out, split_k=False)

        def conv3_f32():
            ops.gemm(t1, w3, bias=b3, act=L.ACT_RESRELU, residual=x, out=out)

        for rep in range(a.reps):
            for cls, arm, fn, K, N in (("conv1", "planes", conv1_planes, K1, pp), ("conv1", "f32", conv1_f32, K1, pp),
                                       ("conv3", "planes", conv3_planes, pp, N3), ("conv3", "f32", conv3_f32, pp, N3)):
                print(json.dumps({"arch": a.arch, "layer": li + 1, "class": cls, "arm": arm, "rep": rep, "rows": M, "K": K, "N": N,
                                  "ms": round(timed(fn, a.steps), 4)}), flush=True)
        del x, xp, t1, t1p, out
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
