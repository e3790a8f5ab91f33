"""Headline A/B of the CLS fold of the pruned last ViT layer (acx_attention_cls_fold, ACX_OPT_CLS_FOLD).  Three arms, fresh processes,
ALTERNATING, `python bench.py --gpus 1 --steps 20 --warmup 5` each, one call on one device:
    parent  the PARENT commit's libacx.so (ACX_LIB_PATH: build it from a checkout of the parent with `python -m anomalyclip_amd._build`
            and copy it to tools/ab_libs/)
    off     this tree's sources with the option's default off (acx_api.hip compiled with -DACX_CLS_FOLD_DEFAULT=0, linked with this
            tree's other objects): must equal the parent, in time and bit for bit in --dump-outputs
    fold    this tree's build
    accepted (the rule of DESIGN.md section 6): the fold arm's slowest run is faster than the parent's fastest AND the median gain is
    >= 3 x the parent arm's spread
    outputs: max |fold - parent| of class_probs / scores against the parent's own `--precision auto` versus `--precision f32` difference
    (one extra parent run in f32)
    A step that fails (any non-zero exit of a bench, profiler or timing process) ends the tool: nothing more is started on the device.
    --prof: one `rocprofv3 --kernel-trace --stats` pass per arm (parent, fold; the profiler alone) over `bench.py --steps 4 --warmup 1`;
            per encode: every gemm_x6_p4_kernel instantiation, attn_cls_kernel, the cls_fold kernels, the LayerNorms, the rest
    --kernels: stand-alone HIP-event timings of what the fold replaces (plane LayerNorm of all rows, the K | V product on the plane
            kernel, acx_attention_cls) against the fold's three launches, ViT-B/16 at 512 and 256 frames (this tree's library)
    python tools/ab_cls_fold.py --parent tools/ab_libs/libacx_parent.so --off tools/ab_libs/libacx_foldoff.so [--runs 6] [--prof]
                                [--kernels] [--out FILE]"""
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
ap.add_argument("--parent", default=None)
ap.add_argument("--off", default=None)
ap.add_argument("--runs", type=int, default=6)
ap.add_argument("--prof", action="store_true")
ap.add_argument("--kernels", action="store_true")
ap.add_argument("--out", default=None)
args = ap.parse_args()
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)
    if args.out:                                   # kept current: a run cut short still leaves what it measured
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


def kernels():
    """stand-alone: the launches the fold replaces against its own, same inputs (in-process, HIP events, median of 20 after 3)"""
    import torch
    sys.path.insert(0, REPO)
    from anomalyclip_amd import _lib as L, ops
    dev, Lt, W, H = "cuda", 197, 768, 12
    g = torch.Generator().manual_seed(1)
    ln_w, ln_b = (1 + 0.2 * torch.randn(W, generator=g)).to(dev), (0.1 * torch.randn(W, generator=g)).to(dev)
    in_w, in_b = (torch.randn(3 * W, W, generator=g) * W ** -0.5).to(dev), (0.2 * torch.randn(3 * W, generator=g)).to(dev)
    w3 = ops.split_bf16x3(in_w[W:].contiguous(), panel=True)
    bkv = in_b[W:].contiguous()
    lib, h = L.lib(), L.ctx(torch.cuda.current_device())

    def timed(fn):
        ts = []
        for i in range(23):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        return statistics.median(ts[3:])

    for frames in (512, 256):
        rows = frames * Lt
        x = torch.randn(rows, W, device=dev) * 1.3
        q = torch.randn(frames, W, device=dev)
        qkv = torch.zeros(rows, 3 * W, device=dev)
        qkv[::Lt, :W] = q
        planes = torch.empty(3, rows, W, dtype=torch.bfloat16, device=dev)
        out = torch.empty(frames, W, device=dev)

        def ln():
            L.check(lib.acx_layernorm(h, x.data_ptr(), W, ln_w.data_ptr(), ln_b.data_ptr(), planes.data_ptr(), W, L.BF16X3P, rows, W, 1e-5,
                                      L.NORM_LAYER, ops._stream()), h)

        def kv():
            ops.gemm_x6(planes, w3, out=qkv[:, W:], bias=bkv, panels=3)

        def att():
            L.check(lib.acx_attention_cls(h, qkv.data_ptr(), 3 * W, out.data_ptr(), W, frames, Lt, H, ops._stream()), h)

        def old():
            ln(); kv(); att()

        nws = lib.acx_attention_cls_fold_workspace_bytes(frames, H)
        fws = torch.empty(nws, dtype=torch.uint8, device=dev)                     # (allocated once: the timing is the three launches)

        def new():
            L.check(lib.acx_attention_cls_fold(h, x.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), 1e-5, in_w.data_ptr(), in_b.data_ptr(),
                                               q.data_ptr(), W, out.data_ptr(), W, frames, Lt, W, H, fws.data_ptr(), nws, ops._stream()), h)

        t = {n: timed(f) for n, f in (("plane LayerNorm, all rows", ln), ("K | V product (plane kernel)", kv), ("acx_attention_cls", att),
                                       ("the three together", old), ("acx_attention_cls_fold (u, fold, o)", new))}
        say(f"stand-alone, ViT-B/16, {frames} frames ({rows} rows):")
        for n, v in t.items():
            say(f"    {n:40s} {v:8.3f} ms")
    return 0


if args.kernels and not args.parent:
    sys.exit(kernels())

parent = os.path.abspath(args.parent)
assert os.path.exists(parent), parent
ARMS = ("parent", "off", "fold") if args.off else ("parent", "fold")
LIBS = {"parent": parent, "off": os.path.abspath(args.off) if args.off else None, "fold": None}


def env_of(arm):
    e = dict(os.environ)
    e.pop("ACX_LIB_PATH", None)
    if LIBS[arm]:
        e["ACX_LIB_PATH"] = LIBS[arm]
    return e


def bench(arm, dump, extra=(), steps=20, warmup=5):
    p = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
                        "--dump-outputs", dump, *extra], cwd=REPO, env=env_of(arm), stdout=subprocess.PIPE, stderr=subprocess.DEVNULL,
                       text=True, timeout=400)
    if p.returncode != 0:
        return None, p.returncode
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1]), 0


tmp = tempfile.mkdtemp(prefix="ab_cls_fold_")
ms = {a: [] for a in ARMS}
ok = True
for i in range(args.runs):
    for arm in ARMS:
        rec, rc = bench(arm, os.path.join(tmp, arm))
        if rec is None:
            say(f"{arm} run {i}: exit status {rc}; stopping")
            ok = False
            break
        ms[arm].append(rec["ms_per_step"])
        say(f"run {i} {arm:6s}: ms_per_step {rec['ms_per_step']}  value {rec.get('value')}")
    if not ok:
        break
if ok:
    med = {a: statistics.median(v) for a, v in ms.items()}
    sp = (max(ms["parent"]) - min(ms["parent"])) / med["parent"]
    for a in ARMS:
        say(f"{a:6s}: median {med[a]:.3f} ms  min {min(ms[a]):.3f}  max {max(ms[a]):.3f}  spread {100 * (max(ms[a]) - min(ms[a])) / med[a]:.2f} %")
    if "off" in ARMS:
        say(f"off against parent: median {100 * (med['off'] - med['parent']) / med['parent']:+.2f} % (parent spread {100 * sp:.2f} %)")
    gain = (med["parent"] - med["fold"]) / med["parent"]
    c1, c2 = max(ms["fold"]) < min(ms["parent"]), gain >= 3 * sp
    say(f"median gain {100 * gain:.2f} % ({med['parent'] - med['fold']:.3f} ms);  slowest fold run < fastest parent run: {c1};  "
        f"gain >= 3 x parent spread ({300 * sp:.2f} %): {c2}  ->  {'ACCEPTED' if c1 and c2 else 'NOT accepted'}")
    # the parent's own auto - f32 difference: the yardstick of the fold's output change
    rec, rc = bench("parent", os.path.join(tmp, "parent_f32"), ("--precision", "f32"), steps=2, warmup=1)
    if rec is None:
        say(f"parent --precision f32: exit status {rc}; stopping (no further GPU step)")
        ok = False
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(tmp, "parent", "*.npy")))
    for n in names:
        a = np.load(os.path.join(tmp, "parent", n))
        if "off" in ARMS:
            b = np.load(os.path.join(tmp, "off", n))
            say(f"--dump-outputs {n}: off against parent {'equal bit for bit' if a.shape == b.shape and a.tobytes() == b.tobytes() else 'DIFFERENT'}")
        d = float(np.abs(np.load(os.path.join(tmp, "fold", n)).astype(np.float64) - a).max())
        line = f"--dump-outputs {n}: {a.shape} max |fold - parent| {d:.3e}"
        if rec is not None:
            y = float(np.abs(np.load(os.path.join(tmp, "parent_f32", n)).astype(np.float64) - a).max())
            line += f";  parent max |auto - f32| {y:.3e}  ->  {'within' if d <= y else 'ABOVE'} the yardstick"
        say(line)

if ok and args.prof:
    for arm in ("parent", "fold"):
        d = os.path.join(tmp, "prof_" + arm)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "bench", "--",
               sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1"]
        p = subprocess.run(cmd, cwd=tmp, env=env_of(arm), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=400)
        st = glob.glob(os.path.join(d, "**", "bench_kernel_stats.csv"), recursive=True)
        if p.returncode != 0 or not st:
            say(f"rocprofv3 {arm}: exit status {p.returncode}, stats file {'found' if st else 'missing'}; stopping (no further GPU step)")
            ok = False
            break
        fam = {}
        for r in csv.DictReader(open(st[0])):
            n = r["Name"]
            m = re.search(r"gemm_x6_p4_kernel<([^>]*)>", n)
            c = re.search(r"(cls_fold_[a-z_]*kernel|attn_cls_kernel|attn_p3_kernel|layernorm_panel2_kernel|layernorm_kernel)", n)
            key = f"gemm_x6_p4_kernel<{m.group(1).replace(' ', '')}>" if m else c.group(1) if c else "everything else"
            cnt, t = fam.get(key, (0, 0.0))
            fam[key] = (cnt + int(r["Calls"]), t + float(r["TotalDurationNs"]) * 1e-6)
        nattn = sum(cnt for k, (cnt, t) in fam.items() if k.startswith("attn_p3"))
        steps = max(1, nattn // 11)                    # eleven whole layers per encode
        say(f"rocprofv3 --kernel-trace --stats, {arm}: {steps} encodes profiled; per encode:")
        for k in sorted(fam):
            say(f"    {k:56s} {fam[k][0] / steps:7.1f} launches  {fam[k][1] / steps:8.3f} ms")
        say(f"    all kernels {sum(t for c_, t in fam.values()) / steps:.3f} ms")

if ok and args.kernels:
    p = subprocess.run([sys.executable, os.path.abspath(__file__), "--kernels"], cwd=REPO, env=env_of("fold"), stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=300)
    for ln in p.stdout.splitlines():
        say(ln)
    if p.returncode != 0:
        say(f"--kernels: exit status {p.returncode}")
        ok = False

sys.exit(0 if ok else 1)
