"""Gate for moving the plane-reuse GEMM (acx_gemm_x6.h) from v_mfma_f32_32x32x16_bf16 to v_mfma_f32_16x16x32_bf16: where the chip
holds its clock down under load, the clock it holds can depend on the MFMA shape.  Four loops of acx_probe_mfma on random operands,
INTERLEAVED in one process, several rounds, ~0.2 s sustained each:
    mode 2 / 3: register-only 32x32x16 / 16x16x32 (64 accumulator registers, one wave per SIMD)
    mode 4 / 5: the kernel's half-step without DMA and barriers -- 128 x 128 outputs per wave, every fragment re-read from LDS
then the headline of bench.py (fresh child processes, the form the driver uses) a few times for the run-to-run spread s of ms_per_step
on the same device.  The rewrite is worth starting only if the LDS-fed ratio r promises 0.875 x (1 - 1/r) >= 2 s.
    python tools/probes/x6_mfma_shape_gate.py [--rounds 5] [--bench-runs 3] [--out FILE]"""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, REPO)
import torch
from anomalyclip_amd import _lib as L
from bench import _event_time

ap = argparse.ArgumentParser()
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--bench-runs", type=int, default=3)
ap.add_argument("--out", default=None)
args = ap.parse_args()

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


dev = torch.device("cuda:0")
lib, h = L.lib(), L.ctx(0)
st = torch.cuda.current_stream().cuda_stream
sink = torch.zeros(4, device=dev)
# ~25.6 M MFMA cycles per launch (~15 ms), 12 launches back to back per measurement
MODES = ((2, "reg 32x32x16", 200000), (3, "reg 16x16x32", 100000), (4, "lds 32x32x16", 8334), (5, "lds 16x16x32", 8334))
tf = {m: [] for m, _, _ in MODES}
say(f"device: {torch.cuda.get_device_name(0)}   rounds {args.rounds}, 12 launches of ~15 ms per loop and round, one wave per SIMD, random bf16 operands")
for rnd in range(args.rounds):
    row = []
    for m, name, iters in MODES:
        fl = ctypes.c_double(0.0)

        def run(m=m, iters=iters, fl=fl):
            L.check(lib.acx_probe_mfma(h, m, iters, 1, sink.data_ptr(), ctypes.byref(fl), st), h)
        dt = _event_time(run, 12, 2)
        tf[m].append(fl.value / dt / 1e12)
        row.append(f"{name} {tf[m][-1]:7.1f}")
    say(f"round {rnd}: TFLOP/s  " + " | ".join(row))
med = {m: statistics.median(v) for m, v in tf.items()}
for m, name, _ in MODES:
    say(f"{name}: median {med[m]:7.1f} TFLOP/s  min {min(tf[m]):7.1f}  max {max(tf[m]):7.1f}")
r_reg, r_lds = med[3] / med[2], med[5] / med[4]
per_round = [b / a for a, b in zip(tf[4], tf[5])]
say(f"ratio 16x16x32 / 32x32x16: register-only {r_reg:.4f}   LDS-fed r = {r_lds:.4f} (per round: {' '.join(f'{x:.4f}' for x in per_round)})")
gain = 0.875 * (1.0 - 1.0 / r_lds)
say(f"expected step gain 0.875 x (1 - 1/r) = {100 * gain:.2f} %")
torch.cuda.synchronize()

ms = []
for i in range(args.bench_runs):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"], cwd=REPO,
                       stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=300)
    if p.returncode != 0:
        say(f"bench.py run {i}: exit status {p.returncode}; stopping")
        break
    rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
    ms.append(rec["ms_per_step"])
    say(f"bench.py run {i}: ms_per_step {rec['ms_per_step']}  value {rec.get('value')}")
if len(ms) >= 2:
    s = (max(ms) - min(ms)) / statistics.median(ms)
    say(f"headline: median {statistics.median(ms):.3f} ms, min-max spread s = {100 * s:.2f} %   2 s = {200 * s:.2f} %")
    say(f"GATE: expected gain {100 * gain:.2f} % {'>=' if gain >= 2 * s else '<'} 2 s = {200 * s:.2f} %  ->  {'PASS' if gain >= 2 * s else 'STOP'}")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
