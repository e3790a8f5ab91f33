"""Time of the f32 ViT attention: `python tools/attn_bench.py [L] [--head-dim 64|80] [--batch F] [--heads H] [--planes]`.

--head-dim 64 (default): acx_attention (acx_attention_x3_panel with --planes); 80: acx_attention_hd (acx_attention_x3_hd, K-panel planes).
--compare: both head dimensions at one width (H heads of 80 against 5 H / 4 heads of 64: the same FLOPs and bytes), timed ALTERNATELY in
one process, medians over --reps legs, f32 rows and panel planes; prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from anomalyclip_amd import _lib as Lb  # noqa: E402
from anomalyclip_amd import ops  # noqa: E402


def runner(qkv, F, L, H, hd, planes):
    W = H * hd
    if hd == 64 and not planes:
        return lambda: ops.attention(qkv, F, L, H, False)
    if hd == 64:
        out = torch.empty(3, F * L, W, dtype=torch.bfloat16, device=qkv.device)
        lib, h = Lb.lib(), ops._h(qkv)
        return lambda: Lb.check(lib.acx_attention_x3_panel(h, qkv.data_ptr(), 3 * W, out.data_ptr(), W, F, L, H, ops._stream()), h)
    out = torch.empty((3, F * L, W) if planes else (F * L, W), dtype=torch.bfloat16 if planes else torch.float32, device=qkv.device)
    return lambda: ops.attention_hd(qkv, F, L, H, hd, planes_out=planes, panel_out=planes, out=out)


def time_ms(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("L", nargs="?", type=int, default=197)
    ap.add_argument("--head-dim", type=int, default=64, choices=(64, 80))
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--heads", type=int, default=None, help="default 12 (head dim 64) / 16 (80)")
    ap.add_argument("--planes", action="store_true")
    ap.add_argument("--compare", action="store_true")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    F, L = a.batch, a.L
    Lp = (L + 15) // 16 * 16
    if not a.compare:
        hd = a.head_dim
        H = a.heads or (16 if hd == 80 else 12)
        qkv = torch.randn(F * L, 3 * H * hd, device="cuda")
        fn = runner(qkv, F, L, H, hd, a.planes)
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = time_ms(fn, a.iters)
        print(f"attention F={F} L={L} H={H} head_dim={hd}{' planes' if a.planes else ''}: {ms:.4f} ms  "
              f"{4.0 * F * H * L * L * hd / ms / 1e9:.1f} TFLOP/s (algorithmic)  "
              f"{4.0 * F * H * Lp * Lp * hd / ms / 1e9:.1f} TFLOP/s (16-padded MFMA work)")
        return
    H80 = a.heads or 16
    H64 = H80 * 5 // 4
    assert H64 * 64 == H80 * 80, "--compare needs a number of heads divisible by 4"
    qkv = torch.randn(F * L, 3 * H80 * 80, device="cuda")
    res = {"L": L, "batch": F, "width": H80 * 80, "heads": {"hd80": H80, "hd64": H64}, "reps": a.reps, "iters": a.iters}
    for planes in (False, True):
        arms = {"hd64": runner(qkv, F, L, H64, 64, planes), "hd80": runner(qkv, F, L, H80, 80, planes)}
        for fn in arms.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        legs = {k: [] for k in arms}
        for _ in range(a.reps):
            for k, fn in arms.items():
                legs[k].append(time_ms(fn, a.iters))
        med = {k: statistics.median(v) for k, v in legs.items()}
        res["panel_planes" if planes else "f32_rows"] = {
            "median_ms": {k: round(v, 4) for k, v in med.items()}, "legs_ms": {k: [round(t, 4) for t in v] for k, v in legs.items()},
            "hd80_over_hd64": round(med["hd80"] / med["hd64"], 4),
            "tflops_algorithmic": {k: round(4.0 * F * L * L * H80 * 80 / v / 1e9, 1) for k, v in med.items()}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
