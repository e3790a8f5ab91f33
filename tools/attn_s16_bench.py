"""acx_attention_s16 (the streaming fp16 planes attention) alone, against what "auto" launches for the same sequences.

    python tools/attn_s16_bench.py --L 257 --heads 16 [--batch 512 --reps 3 --steps 20 --warmup 3]

Arm "s16": ops.attention_s16 on the two fp16 planes of q | k | v.  Arm "auto": for 128 < L the f32 attention that writes the
out-projection's three bf16 planes (acx_attention_x3_panel on f32 rows); for L <= 128 acx_attention followed by
acx_split_bf16x3_panel.  The legs alternate in one process (s16 auto s16 auto ...), `--steps` launches per leg behind `--warmup`
launches of the leg's own, timed with HIP events; one JSON line with every leg, each arm's mean and the spread of its legs -- the
run-to-run spread a difference has to exceed.  `tflops` counts 4 batch heads L L 64 flops once (f32-equivalent)."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from anomalyclip_amd import _lib as L  # noqa: E402
from anomalyclip_amd import ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=257)
    ap.add_argument("--heads", type=int, default=16)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    W = a.heads * 64
    qkv = torch.randn(a.batch * a.L, 3 * W, generator=torch.Generator().manual_seed(1)).to(dev)
    planes = ops.split_f16x2(qkv, panel=True)
    out3 = torch.empty(3, a.batch * a.L, W, dtype=torch.bfloat16, device=dev)
    lib, h, s = L.lib(), ops._h(qkv), ops._stream()

    def auto():
        if a.L > 128:
            L.check(lib.acx_attention_x3_panel(h, qkv.data_ptr(), 3 * W, out3.data_ptr(), W, a.batch, a.L, a.heads, s), h)
        else:
            ops.split_bf16x3(ops.attention(qkv, a.batch, a.L, a.heads, False), out=out3, panel=True)

    arms = {"s16": lambda: ops.attention_s16(planes, a.batch, a.L, a.heads), "auto": auto}
    legs = []
    for r in range(a.reps):
        for name, fn in arms.items():
            for _ in range(a.warmup):
                fn()
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            ev[0].record()
            for _ in range(a.steps):
                fn()
            ev[1].record()
            torch.cuda.synchronize()
            legs.append({"arm": name, "rep": r, "ms": round(ev[0].elapsed_time(ev[1]) / a.steps, 4)})
    by = {n: [l["ms"] for l in legs if l["arm"] == n] for n in arms}
    mean = {n: sum(v) / len(v) for n, v in by.items()}
    flops = 4.0 * a.batch * a.heads * a.L * a.L * 64
    o = ops.unpanel(ops.attention_s16(planes, a.batch, a.L, a.heads)).float().sum(0)
    ref = ops.attention(qkv, a.batch, a.L, a.heads, False)
    print(json.dumps({"L": a.L, "heads": a.heads, "batch": a.batch, "steps": a.steps, "legs": legs,
                      "ms": {n: round(v, 4) for n, v in mean.items()},
                      "spread": {n: round((max(v) - min(v)) / mean[n], 5) for n, v in by.items()},
                      "tflops": {n: round(flops / v / 1e9, 1) for n, v in mean.items()},
                      "auto/s16": round(mean["auto"] / mean["s16"], 3),
                      "max_abs_diff_vs_f32_attention": float((o - ref).abs().max())}))


if __name__ == "__main__":
    main()
