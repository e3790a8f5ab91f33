"""Headline A/B of the f32-fed plane attention (acx_attention_p3f, ACX_OPT_ATTN_F32IN): the PARENT commit's libacx.so (ACX_LIB_PATH:
build it from a checkout of the parent with `python -m anomalyclip_amd._build` and copy it to tools/ab_libs/) against this tree's,
`python bench.py --gpus 1 --steps 20 --warmup 5`, arms ALTERNATING, fresh processes, one call on one device.
    accepted (the rule of profiles/ln_rider_ab.txt): this tree's slowest run is faster than the parent's fastest AND the median gain
    is >= 3 x the parent arm's spread
    --dump-outputs of both arms must be equal bit for bit
    --prof: one `rocprofv3 --kernel-trace --stats` pass per arm (the profiler alone) over `bench.py --steps 4 --warmup 1`; per encode:
            every gemm_x6_p4_kernel instantiation on a line of its own (template arguments: the in-projection is the one whose
            launches move between the plane and the f32 epilogue), the family total, the attention, LayerNorm, the rest
    --lib: the library of the new arm where it is not this tree's build (a build with another default of the option, say)
    python tools/ab_attn_f32in.py --parent tools/ab_libs/libacx_parent.so [--lib FILE] [--runs 6] [--prof] [--out FILE]"""
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
ap.add_argument("--lib", default=None)
ap.add_argument("--runs", type=int, default=6)
ap.add_argument("--prof", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
parent = os.path.abspath(args.parent)
assert os.path.exists(parent), parent
lines = []
ARMS = ("parent", "f32in")


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:                                   # kept current: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def env_of(arm):
    e = dict(os.environ)
    e.pop("ACX_LIB_PATH", None)
    if arm == "parent":
        e["ACX_LIB_PATH"] = parent
    elif args.lib:
        e["ACX_LIB_PATH"] = os.path.abspath(args.lib)
    return e


tmp = tempfile.mkdtemp(prefix="ab_attn_f32in_")
ms = {a: [] for a in ARMS}
ok = True
for i in range(args.runs):
    for arm in ARMS:
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
    gain = (med["parent"] - med["f32in"]) / med["parent"]
    for a in ARMS:
        say(f"{a:6s}: median {med[a]:.3f} ms  min {min(ms[a]):.3f}  max {max(ms[a]):.3f}  spread {100 * (max(ms[a]) - min(ms[a])) / med[a]:.2f} %")
    c1, c2 = max(ms["f32in"]) < min(ms["parent"]), gain >= 3 * sp
    say(f"median gain {100 * gain:.2f} % ({med['parent'] - med['f32in']:.3f} ms);  slowest f32in run < fastest parent run: {c1};  "
        f"gain >= 3 x parent spread ({300 * sp:.2f} %): {c2}  ->  {'ACCEPTED' if c1 and c2 else 'NOT accepted'}")
    same = True
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, "parent", "*.npy")))
    for n in names:
        a, b = np.load(os.path.join(tmp, "parent", n)), np.load(os.path.join(tmp, "f32in", n))
        eq = a.shape == b.shape and a.tobytes() == b.tobytes()
        same = same and eq
        say(f"--dump-outputs {n}: {a.shape} {'equal bit for bit' if eq else 'DIFFERENT'}")
    say(f"outputs of both arms: {'EQUAL' if same and names else 'NOT EQUAL'}")

if ok and args.prof:
    for arm in ARMS:
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
            a = re.search(r"attn_p3_kernel<([^>]*)>", n)
            key = (f"gemm_x6_p4_kernel<{m.group(1).replace(' ', '')}>" if m else f"attn_p3_kernel<{a.group(1).replace(' ', '')}>" if a
                   else "layernorm_panel2_kernel" if "layernorm_panel2_kernel" in n else "everything else")
            c, t = fam.get(key, (0, 0.0))
            fam[key] = (c + int(r["Calls"]), t + float(r["TotalDurationNs"]) * 1e-6)
        nattn = sum(c for k, (c, t) in fam.items() if k.startswith("attn_p3"))
        steps = max(1, nattn // 11)                    # eleven whole layers per encode
        say(f"rocprofv3 --kernel-trace --stats, {arm}: {steps} encodes profiled; per encode:")
        for k in sorted(fam):
            say(f"    {k:56s} {fam[k][0] / steps:7.1f} launches  {fam[k][1] / steps:8.3f} ms")
        gsum = sum(t for k, (c, t) in fam.items() if k.startswith("gemm_x6"))
        asum = sum(t for k, (c, t) in fam.items() if k.startswith("attn_p3"))
        say(f"    gemm_x6_p4_kernel family {gsum / steps:.3f} ms, attn_p3_kernel {asum / steps:.3f} ms, together {(gsum + asum) / steps:.3f} ms")
