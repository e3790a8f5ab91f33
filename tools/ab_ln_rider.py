"""Headline A/B of the LayerNorm rider (acx_gemm_ln): the PARENT commit's libacx.so (ACX_LIB_PATH, as tools/ab_x6.sh does: build it from
a checkout of the parent with `python -m anomalyclip_amd._build` and copy it to tools/ab_libs/) against this tree's, `python
bench.py --gpus 1 --steps 20 --warmup 5`, arms ALTERNATING, fresh processes, one call on one device.
    accepted: this tree's slowest run is faster than the parent's fastest AND the median gain is >= 3 x the parent arm's spread
    --dump-outputs of both arms must be equal bit for bit
    --prof: one `rocprofv3 --kernel-trace --stats` pass per arm (the profiler alone), LayerNorm and GEMM-family time per step
    python tools/ab_ln_rider.py --parent tools/ab_libs/libacx_parent.so [--runs 6] [--prof] [--out FILE]"""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True)
ap.add_argument("--runs", type=int, default=6)
ap.add_argument("--prof", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
parent = os.path.abspath(args.parent)
assert os.path.exists(parent), parent
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def env_of(arm):
    e = dict(os.environ)
    e.pop("ACX_LIB_PATH", None)
    if arm == "parent":
        e["ACX_LIB_PATH"] = parent
    return e


tmp = tempfile.mkdtemp(prefix="ab_ln_rider_")
ms = {"parent": [], "rider": []}
ok = True
for i in range(args.runs):
    for arm in ("parent", "rider"):
        dump = os.path.join(tmp, arm)
        p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", dump],
                           cwd=REPO, env=env_of(arm), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, text=True, timeout=400)
        if p.returncode != 0:
            say(f"{arm} run {i}: exit status {p.returncode}; stopping")
            ok = False
            break
        rec = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])
        ms[arm].append(rec["ms_per_step"])
        say(f"run {i} {arm:6s}: ms_per_step {rec['ms_per_step']}  value {rec.get('value')}")
    if not ok:
        break
if ok:
    med = {a: statistics.median(v) for a, v in ms.items()}
    sp = (max(ms["parent"]) - min(ms["parent"])) / med["parent"]
    gain = (med["parent"] - med["rider"]) / med["parent"]
    say(f"parent: median {med['parent']:.3f} ms  min {min(ms['parent']):.3f}  max {max(ms['parent']):.3f}  spread {100 * sp:.2f} %")
    say(f"rider : median {med['rider']:.3f} ms  min {min(ms['rider']):.3f}  max {max(ms['rider']):.3f}  spread {100 * (max(ms['rider']) - min(ms['rider'])) / med['rider']:.2f} %")
    c1, c2 = max(ms["rider"]) < min(ms["parent"]), gain >= 3 * sp
    say(f"median gain {100 * gain:.2f} %;  slowest rider run < fastest parent run: {c1};  gain >= 3 x parent spread ({300 * sp:.2f} %): {c2}  ->  {'ACCEPTED' if c1 and c2 else 'NOT accepted'}")
    same = True
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, "parent", "*.npy")))
    for n in names:
        a, b = np.load(os.path.join(tmp, "parent", n)), np.load(os.path.join(tmp, "rider", n))
        eq = a.shape == b.shape and a.tobytes() == b.tobytes()
        same = same and eq
        say(f"--dump-outputs {n}: {a.shape} {'equal bit for bit' if eq else 'DIFFERENT'}")
    say(f"outputs of both arms: {'EQUAL' if same and names else 'NOT EQUAL'}")

if ok and args.prof:
    for arm in ("parent", "rider"):
        d = os.path.join(tmp, "prof_" + arm)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bench", "--",
               sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1"]
        p = subprocess.run(cmd, cwd=tmp, env=env_of(arm), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
        st = glob.glob(os.path.join(d, "**", "bench_kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not st:
            say(f"rocprofv3 {arm}: exit status {p.returncode}, stats file {'found' if st else 'missing'}; stopping")
            break
        fam = {}
        for r in csv.DictReader(open(st[0])):
            n = r["Name"]
            m = re.search(r"gemm_x6_p4_kernel<([^>]*)>", n)
            targs = [int(v) for v in m.group(1).split(",")] if m else []
            key = ("gemm_x6_p4_kernel (other)" if m and not (targs[0] == 0 and targs[2] == 1)
                   else "gemm_x6_p4_kernel (residual, riders)" if m and len(targs) > 9 and targs[9] == 1
                   else "gemm_x6_p4_kernel (residual)" if m
                   else "layernorm_panel2_kernel" if "layernorm_panel2_kernel" in n
                   else "attn_p3_kernel" if "attn_p3_kernel" in n else "everything else")
            c, t = fam.get(key, (0, 0.0))
            fam[key] = (c + int(r["Calls"]), t + float(r["TotalDurationNs"]) * 1e-6)
        steps = max(1, fam.get("attn_p3_kernel", (11, 0))[0] // 11)      # eleven whole layers per encode
        say(f"rocprofv3 --kernel-trace --stats, {arm}: {steps} encodes profiled; per encode:")
        for k in sorted(fam):
            say(f"    {k:40s} {fam[k][0] / steps:7.1f} launches  {fam[k][1] / steps:8.3f} ms")
        gsum = sum(t for k, (c, t) in fam.items() if k.startswith("gemm_x6"))
        say(f"    gemm_x6_p4_kernel family {gsum / steps:.3f} ms, + layernorm_panel2 {(gsum + fam.get('layernorm_panel2_kernel', (0, 0.0))[1]) / steps:.3f} ms")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
