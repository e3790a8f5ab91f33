"""Gate for the LayerNorm rider of the residual bf16 x 6 products (acx_gemm_ln; acx_gemm_x6.h, RIDE): the ViT-B/16 shapes of a
512-frame launch, M = 100,864, N = 768, K = 768 (out-proj) and K = 3072 (c_proj), residual in place, random data, every arm
INTERLEAVED in one process on one device, several rounds:
    (a)  product, then LayerNorm                        (ACX_OPT_LN_RIDER = 0: what the drivers did before)
    (b)  product with riders, then the remainder LayerNorm, rows by the library's cost model (ACX_OPT_LN_RIDER = 1)
    (r)  the same with 1/8 .. 8/8 of the completed rows forced to ride: where the time stops falling is what the riders finish
         within the tail -- the rate constant beside x6_strip_cost (rows of 768 columns per us and rider CU)
    (g)  the product alone, (l) the LayerNorm alone
GATE: (b) must beat (a) at K = 3072 by more than the arms' own repeat spread.
    python tools/probes/ln_rider_gate.py [--rounds 5] [--iters 20] [--out FILE]"""
import argparse
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import torch
from anomalyclip_amd import ops
from bench import _event_time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--iters", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


DEV = torch.device("cuda:0")
dev = 0
ncu = ops.x6_workgroups(dev)
M, N = 512 * 197, 768
say(f"device: {torch.cuda.get_device_name(0)}   {ncu} workgroups   M = {M}, N = {N}, residual in place; {args.rounds} rounds x {args.iters} calls per arm, interleaved")
verdict = {}
for K in (768, 3072):
    g = torch.Generator(device=DEV).manual_seed(K)
    a = torch.randn(M, K, generator=g, device=DEV)
    w = torch.randn(N, K, generator=g, device=DEV) * (0.02 / K ** 0.5)    # (x grows by ~2 % of its scale per call: no overflow over the run)
    a3, w3 = ops.split_bf16x3(a, panel=True), ops.split_bf16x3(w, panel=True)
    del a, w
    bias = torch.randn(N, generator=g, device=DEV) * 0.01
    x = torch.randn(M, N, generator=g, device=DEV)
    lw, lb = torch.randn(N, generator=g, device=DEV), torch.randn(N, generator=g, device=DEV)
    y = torch.empty(3, M, N, dtype=torch.bfloat16, device=DEV)
    ride, ready = ops.ln_rider_plan(M, N, K, ncu)
    say(f"K = {K}: plan {ride} of {ready} completed rows ride")

    def both():
        ops.gemm_x6(a3, w3, panels=3, bias=bias, residual=x, out=x, ln=(lw, lb, y))

    def prod():
        ops.gemm_x6(a3, w3, panels=3, bias=bias, residual=x, out=x)

    def norm():
        ops.layernorm(x, lw, lb, planes_out=True, panel_out=True)

    arms = [("a", 0, both), ("b", 1, both)] + [(f"r{e}/8", max(2, ready * e // 8), both) for e in range(1, 9)] + [("g", 0, prod), ("l", 0, norm)]
    t = {n: [] for n, _, _ in arms}
    try:
        for rnd in range(args.rounds):
            for n, mode, fn in arms:
                ops.set_ln_rider(dev, mode)
                t[n].append(_event_time(fn, args.iters, 3) * 1e3)
            say(f"  round {rnd}: ms  " + "  ".join(f"{n} {t[n][-1]:.4f}" for n, _, _ in arms))
    finally:
        ops.set_ln_rider(dev, 1)
    med = {n: statistics.median(v) for n, v in t.items()}
    spread = {n: max(v) - min(v) for n, v in t.items()}
    for n, mode, _ in arms:
        say(f"  {n:5s} rows {mode if mode > 1 else (ride if mode == 1 else 0):6d}: median {med[n]:.4f} ms  min {min(t[n]):.4f}  max {max(t[n]):.4f}")
    best = min((n for n, _, _ in arms if n.startswith("r")), key=lambda n: med[n])
    say(f"  product alone + LayerNorm alone = {med['g'] + med['l']:.4f} ms;  (a) {med['a']:.4f}  (b) {med['b']:.4f}  best forced arm {best} {med[best]:.4f}")
    gain, s = med["a"] - med["b"], max(spread["a"], spread["b"])
    verdict[K] = gain > s
    say(f"  (a) - (b) = {gain * 1e3:.1f} us ({100 * gain / med['a']:.2f} % of the pair), repeat spread of the arms {s * 1e3:.1f} us  ->  {'faster' if gain > s else 'NOT faster'}")
    del a3, w3, x, y
    torch.cuda.synchronize()
say(f"GATE (K = 3072): {'PASS' if verdict[3072] else 'STOP'}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
