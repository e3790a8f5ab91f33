"""Headline A/B of precision "auto"'s third resolution step (ACX_PREC_F32X6_QKV16: q | k | v as fp16 planes into the three-product planes
attention); tools/ab_r16.py's method.  Arms, each a libacx.so handed to this tree's Python through ACX_LIB_PATH,
`python bench.py --gpus 1 --steps 20 --warmup 5`, ALTERNATING, fresh processes, one call on one device:
    parent   the parent commit's library (build it from a checkout of the parent with `python -m anomalyclip_amd._build`): it has no
             acx_vit_encode_qkv16, so "auto" resolves to ACX_PREC_F32X6_R16 -- the parent's launches
    NAME     any number of --arm NAME=PATH: this tree built with a build constant changed (acx_api.hip only), e.g.
             off = -DACX_QKV16_DEFAULT=0 (the new entry point with ACX_PREC_F32X6_R16's records)
    new      this tree's library as built
  accepted (per arm against parent): the arm's slowest run is faster than the parent's fastest AND the median gain is >= 3 x the parent
  arm's spread.  --dump-outputs: max |arm - parent| on class_probs.npy / scores.npy against the yardstick max |parent auto - parent f32|.
  --prof: one `rocprofv3 --kernel-trace --stats` pass per arm (the profiler alone; --steps 5 --warmup 1 --no-extra-legs
  --no-cpu-baseline: the headline step's encodes and nothing else under the tracer), per-encode time by kernel;
  --runs 0 --prof: the profile passes alone, in a call of their own.
    python tools/ab_qkv16.py --parent tools/ab_libs/libacx_parent.so [--arm off=tools/ab_libs/libacx_qkv16off.so] [--runs 6] [--prof] [--out FILE]"""
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
ap.add_argument("--arm", action="append", default=[], help="NAME=PATH of a variant library")
ap.add_argument("--runs", type=int, default=6)
ap.add_argument("--prof", action="store_true")
ap.add_argument("--headline-only", action="store_true",
                help="timed runs with --no-extra-legs --no-cpu-baseline: the same headline step, without bench.py's other legs (a short call)")
ap.add_argument("--out", default=None)
args = ap.parse_args()
libs = {"parent": os.path.abspath(args.parent)}
for spec in args.arm:
    name, path = spec.split("=", 1)
    libs[name] = os.path.abspath(path)
libs["new"] = None
arms = list(libs)
width = max(len(a) for a in arms)
for p in libs.values():
    assert p is None or os.path.exists(p), p
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def env_of(arm):
    e = dict(os.environ)
    e.pop("ACX_LIB_PATH", None)
    if libs[arm]:
        e["ACX_LIB_PATH"] = libs[arm]
    return e


def bench(arm, extra, timeout=400):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", *extra], cwd=REPO, env=env_of(arm),
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)
    if p.returncode != 0:
        say(f"{arm}: bench.py {' '.join(extra)} failed; the end of its stderr:\n" + "\n".join(p.stderr.splitlines()[-15:]))
        return p.returncode, None
    return 0, json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


say(f"tools/ab_qkv16.py: arms {', '.join(arms)}; {args.runs} alternating runs of bench.py --gpus 1 --steps 20 --warmup 5 each")
tmp = tempfile.mkdtemp(prefix="ab_qkv16_")
ms = {a: [] for a in arms}
short = ["--no-extra-legs", "--no-cpu-baseline"] if args.headline_only else []
if short:
    say("timed runs with " + " ".join(short) + ": the headline step alone")
ok = True
for i in range(args.runs):
    for arm in arms:
        rc, rec = bench(arm, ["--steps", "20", "--warmup", "5", *short, "--dump-outputs", os.path.join(tmp, arm)])
        if rc:
            say(f"{arm} run {i}: exit status {rc}; stopping")      # (nothing more is started on the device after a failed run)
            ok = False
            break
        ms[arm].append(rec["ms_per_step"])
        say(f"run {i} {arm:{width}s}: ms_per_step {rec['ms_per_step']}  value {rec.get('value')}")
    if not ok:
        break
if ok and args.runs:
    med = {a: statistics.median(v) for a, v in ms.items()}
    sp = (max(ms["parent"]) - min(ms["parent"])) / med["parent"]
    for a in arms:
        say(f"{a:{width}s}: median {med[a]:.3f} ms  min {min(ms[a]):.3f}  max {max(ms[a]):.3f}  spread {100 * (max(ms[a]) - min(ms[a])) / med[a]:.2f} %")
    for a in arms[1:]:
        gain = (med["parent"] - med[a]) / med["parent"]
        c1, c2 = max(ms[a]) < min(ms["parent"]), gain >= 3 * sp
        say(f"{a}: median gain {100 * gain:.2f} %;  slowest run < fastest parent run: {c1};  gain >= 3 x parent spread ({300 * sp:.2f} %): {c2}"
            f"  ->  {'ACCEPTED' if c1 and c2 else 'NOT accepted'}")
    # the outputs' yardstick: the parent's own distance between its default and its f32 MFMA path
    rc, _ = bench("parent", ["--steps", "1", "--warmup", "0", "--precision", "f32", "--no-extra-legs", "--no-cpu-baseline", "--dump-outputs",
                             os.path.join(tmp, "parent_f32")])
    if rc:
        say(f"parent --precision f32: exit status {rc}; stopping")
        ok = False
    else:
        for n in sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, "parent", "*.npy"))):
            ref = np.load(os.path.join(tmp, "parent", n)).astype(np.float64)
            yard = float(np.abs(ref - np.load(os.path.join(tmp, "parent_f32", n))).max())
            for a in arms[1:]:
                d = float(np.abs(np.load(os.path.join(tmp, a, n)) - ref).max())
                say(f"--dump-outputs {n}: max |{a} - parent| = {d:.3e};  yardstick max |parent auto - parent f32| = {yard:.3e}  ->  "
                    f"{'within' if d <= yard else 'ABOVE'}")

if ok and args.prof:
    for arm in arms:
        d = os.path.join(tmp, "prof_" + arm)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bench", "--",
               sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "1", "--no-extra-legs", "--no-cpu-baseline"]
        p = subprocess.run(cmd, cwd=tmp, env=env_of(arm), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=240)   # (a headline-only run takes under 20 s untraced)
        st = glob.glob(os.path.join(d, "**", "bench_kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not st:
            say(f"rocprofv3 {arm}: exit status {p.returncode}, stats file {'found' if st else 'missing'}; stopping")
            break
        fam = {}
        for r in csv.DictReader(open(st[0])):
            n = r["Name"]
            m = re.search(r"gemm_x6_(p4|h3|r16)_kernel<([^>]*)>", n)
            if m:
                t = [int(v) for v in m.group(2).split(",")]
                cm, act, res, x3, ride = t[0], t[1], t[2], t[8], t[9] if len(t) > 9 else 0
                what = ("residual products, riders" if ride else "residual products (out-proj, c_proj)" if res
                        else "c_fc -> planes (QuickGELU)" if cm == 2 and act == 1 else "in-proj -> fp16 planes" if cm == 2 and act == 0
                        else "in-proj -> f32 rows" if cm == 0 and act == 0 else "other")
                key = f"gemm_x6_{m.group(1)}_kernel {'fp16 x3' if x3 == 2 else 'bf16 x6'}: {what}"
            else:
                key = ("layernorm_panel2_kernel" if "layernorm_panel2_kernel" in n else "attn_p3_o16_kernel" if "attn_p3_o16" in n
                       else "attn_p3_h16_kernel" if "attn_p3_h16" in n else "attn_p3_kernel" if "attn_p3" in n else "everything else")
            c, tt = fam.get(key, (0, 0.0))
            fam[key] = (c + int(r["Calls"]), tt + float(r["TotalDurationNs"]) * 1e-6)
        natt = sum(fam.get(k, (0, 0))[0] for k in ("attn_p3_kernel", "attn_p3_o16_kernel", "attn_p3_h16_kernel"))
        steps = max(1, natt // 11)                                       # eleven whole layers per encode
        say(f"rocprofv3 --kernel-trace --stats, {arm}: {steps} encodes profiled; per encode:")
        for k in sorted(fam):
            say(f"    {k:62s} {fam[k][0] / steps:7.1f} launches  {fam[k][1] / steps:8.3f} ms")
        say(f"    all kernels {sum(t for c, t in fam.values()) / steps:.3f} ms")
