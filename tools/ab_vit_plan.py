"""A/B of the transformer driver's plan / executor split against the PARENT commit's libacx.so (ACX_LIB_PATH: build it from a checkout
of the parent with `python -m anomalyclip_amd._build` and copy it to tools/ab_libs/).  A refactor: nothing may change.  Fresh
processes, arms ALTERNATING, every step under its own timeout, stop at the first failure, one call on one device.
    bits   one process per arm: ViT-B/16 features in its six precisions at 3, 8 and 512 frames, "auto" on the other three vision
           geometries at 8 frames, the text tower (causal, 14 x 77 rows, width 512); with every call its acx_prof_collect launch
           counts per kind.  Features and counts of both arms must be EQUAL, bit for bit; so must `bench.py --dump-outputs`.
    time   `python bench.py --gpus 1 --steps 20 --warmup 5`, --runs per arm.  No speed-up to claim: this tree's median ms_per_step
           must not exceed the parent arm's median by more than the parent arm's own spread (max - min) in this call.
    python tools/ab_vit_plan.py --parent tools/ab_libs/libacx_parent.so [--runs 6] [--out FILE]"""
import argparse
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARMS = ("parent", "plan")


def child(out_dir):
    """this process's library (ACX_LIB_PATH or the tree's): features and launch counts of every call into out_dir"""
    import ctypes as C
    import torch
    sys.path.insert(0, REPO)
    from anomalyclip_amd import _lib as L
    from anomalyclip_amd import init_weights as IW
    from anomalyclip_amd import ops
    from anomalyclip_amd.components.clip_vit import Transformer, VisionTransformer
    os.makedirs(out_dir, exist_ok=True)
    lib, h = L.lib(), L.ctx(0)
    counts_of = {}

    def record(name, fn):
        try:
            fn()                                           # (weights' planes and workspaces exist before the recording)
        except L.AcxError as e:                            # a refusal (f16x3 where no planes attention runs): its text is the result
            counts_of[name] = str(e)
            return
        counts, ms = (C.c_int32 * 4)(), (C.c_double * 4)()
        L.check(lib.acx_prof_enable(h, 1), h)
        y = fn()
        torch.cuda.synchronize()
        L.check(lib.acx_prof_collect(h, counts, ms), h)
        lib.acx_prof_enable(h, 0)
        np.save(os.path.join(out_dir, name + ".npy"), y.float().cpu().numpy())
        counts_of[name] = list(counts)

    def vit(geom, precision):
        v = VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers, geom.vision_heads,
                              geom.embed_dim, precision=precision)
        v.load_state_dict(IW.init_vit_state_dict(geom, 3, prefix=""), strict=True)
        return v.to("cuda")

    def frames(n, res):
        return torch.randn(n, 3, res, res, generator=torch.Generator().manual_seed(n)).to("cuda")

    with torch.no_grad():
        for precision in ("auto", "f32", "bf16", "f32x6", "bf16x3", "f16x3"):
            v = vit(IW.VIT_B16, precision)
            for n in (3, 8, 512):
                x = frames(n, 224)
                v.chunk = n
                record(f"vit_b16-{precision}-{n}f", lambda: v(x).clone())
        for name in ("VIT_B32", "VIT_L14", "VIT_L14_336"):
            geom = getattr(IW, name)
            v, x = vit(geom, "auto"), frames(8, geom.image_resolution)
            v.chunk = 8
            record(f"{name.lower()}-auto-8f", lambda: v(x).clone())
        torch.manual_seed(7)
        t = Transformer(512, 12, 8, causal=True).to("cuda")
        x = torch.randn(14 * 77, 512, generator=torch.Generator().manual_seed(77)).to("cuda")
        record("text-512-14", lambda: t.forward_(x.clone(), 14, 77))
    with open(os.path.join(out_dir, "counts.json"), "w") as fh:
        json.dump(counts_of, fh, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent")
    ap.add_argument("--runs", type=int, default=6)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args.child)
    parent = os.path.abspath(args.parent)
    assert os.path.exists(parent), parent
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)
        if args.out:                                   # kept current: a run cut short still leaves what it measured
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as fh:
                fh.write("\n".join(lines) + "\n")

    def run(arm, cmd, limit):
        e = dict(os.environ)
        e.pop("ACX_LIB_PATH", None)
        if arm == "parent":
            e["ACX_LIB_PATH"] = parent
        try:
            p = subprocess.run([sys.executable] + cmd, cwd=REPO, env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            say(f"{arm}: {' '.join(cmd[:2])} ran into its {limit} s limit; stopping")
            return None
        if p.returncode != 0:
            say(f"{arm}: {' '.join(cmd[:2])} exit status {p.returncode}; stopping\n{p.stderr[-2000:]}")
            return None
        return p.stdout

    def same_files(what, a_dir, b_dir):
        names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(a_dir, "*.npy")))
        same = bool(names) and names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(b_dir, "*.npy")))
        for n in names if same else ():
            a, b = np.load(os.path.join(a_dir, n)), np.load(os.path.join(b_dir, n))
            eq = a.shape == b.shape and a.tobytes() == b.tobytes() and bool(np.isfinite(a).all())
            same = same and eq
            say(f"{what} {n}: {a.shape} {'equal bit for bit' if eq else 'DIFFERENT'}")
        return same

    tmp = tempfile.mkdtemp(prefix="ab_vit_plan_")
    say(f"A/B of the transformer layer plan: parent library {os.path.basename(parent)} against this tree's")
    for arm in ARMS:
        if run(arm, [os.path.abspath(__file__), "--child", os.path.join(tmp, "bits_" + arm)], 600) is None:
            return 1
    bits = same_files("features", os.path.join(tmp, "bits_parent"), os.path.join(tmp, "bits_plan"))
    ca, cb = (json.load(open(os.path.join(tmp, "bits_" + arm, "counts.json"))) for arm in ARMS)
    for n in sorted(ca):
        say(f"launches (gemm, attention, norm, other) {n}: parent {ca[n]}  plan {cb.get(n)}  {'equal' if ca[n] == cb.get(n) else 'DIFFERENT'}")
    counts = ca == cb
    ms = {a: [] for a in ARMS}
    for i in range(args.runs):
        for arm in ARMS:
            out = run(arm, [os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs",
                            os.path.join(tmp, "bench_" + arm)], 400)
            if out is None:
                return 1
            rec = json.loads([ln for ln in out.splitlines() if ln.startswith("{")][-1])
            ms[arm].append(rec["ms_per_step"])
            say(f"run {i} {arm:6s}: ms_per_step {rec['ms_per_step']}  value {rec.get('value')}")
    bench = same_files("bench.py --dump-outputs", os.path.join(tmp, "bench_parent"), os.path.join(tmp, "bench_plan"))
    med = {a: statistics.median(v) for a, v in ms.items()}
    for a in ARMS:
        say(f"{a:6s}: median {med[a]:.3f} ms  min {min(ms[a]):.3f}  max {max(ms[a]):.3f}  spread {100 * (max(ms[a]) - min(ms[a])) / med[a]:.2f} %")
    spread = max(ms["parent"]) - min(ms["parent"])
    t_ok = med["plan"] <= med["parent"] + spread
    say(f"bits: features {'EQUAL' if bits else 'NOT EQUAL'}, launch counts {'EQUAL' if counts else 'NOT EQUAL'}, "
        f"bench outputs {'EQUAL' if bench else 'NOT EQUAL'}")
    say(f"time: plan median - parent median = {med['plan'] - med['parent']:+.3f} ms ({100 * (med['plan'] - med['parent']) / med['parent']:+.2f} %), "
        f"parent spread (max - min) {spread:.3f} ms ({100 * spread / med['parent']:.2f} %): {'within' if t_ok else 'OUTSIDE'} the spread")
    ok = bits and counts and bench and t_ok
    say("verdict: " + ("NO CHANGE in bits, launches or time" if ok else "FAILED"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
