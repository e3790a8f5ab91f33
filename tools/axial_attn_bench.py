#!/usr/bin/env python
"""Micro-benchmark of acx_axial_attention and acx_seq_attention_bwd per shape, HIP-event timed, the shapes ALTERNATING inside one
process (round r times every shape once, so clock and cache state are shared by the arms).  Per shape: median / min / max time per
launch over the rounds, time per row, and for the forward the achieved bytes/s from 16 * heads * e bytes per row (q, k, v read,
out written).  A shape is `T[xO]:e:heads[:axis]` -- T the attended axis length, O the other axis (default 16), axis 0 attends
along num_segments (rows gl apart), axis 1 along seg_length (contiguous rows).

    python tools/axial_attn_bench.py                       # the default sweep at 32 768 rows (64 videos of 32 x 16)
    python tools/axial_attn_bench.py --shapes 32:32:8 64:32:8 24x10:64:4:0 --rows 32768 --json out.json

A shape the build does not take (ACX_E_UNSUPPORTED) is reported as such and skipped."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from anomalyclip_amd import _lib as L  # noqa: E402
from anomalyclip_amd import ops  # noqa: E402

DEFAULT = ["32:32:8", "32:16:8", "16x32:32:8:1", "64:32:8", "24x10:32:8", "10x24:32:8:1", "48x8:32:8", "8x48:32:8:1", "128x4:32:8",
           "20x20:32:8", "64:16:8", "96:16:8", "32:64:4", "64:64:4", "24x10:64:4", "128x4:64:4"]


def parse(spec):
    f = spec.split(":")
    t = f[0].split("x")
    T, other = int(t[0]), int(t[1]) if len(t) > 1 else 16
    e, heads = int(f[1]), int(f[2])
    axis = int(f[3]) if len(f) > 3 else 0
    return dict(spec=spec, T=T, other=other, e=e, heads=heads, axis=axis)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="*", default=DEFAULT)
    ap.add_argument("--rows", type=int, default=32768, help="token rows per launch (rounded down to whole tiles, at least one)")
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--inner", type=int, default=10, help="launches per timed interval")
    ap.add_argument("--label", default="", help="tag printed with every line (e.g. the build under test)")
    ap.add_argument("--json", default="")
    args = ap.parse_args()
    dev = "cuda"
    arms = []
    g = torch.Generator().manual_seed(0)
    for sh in map(parse, args.shapes):
        gn, gl = (sh["T"], sh["other"]) if sh["axis"] == 0 else (sh["other"], sh["T"])
        tiles = max(1, args.rows // (gn * gl))
        rows, He = tiles * gn * gl, sh["heads"] * sh["e"]
        qkv = torch.randn(rows, 3 * He, generator=g).to(dev)
        dout = torch.randn(rows, He, generator=g).to(dev)
        a = (tiles, gn, gl, sh["heads"], sh["e"], sh["axis"])
        sh.update(rows=rows, fwd=[], bwd=[], fwd_fn=lambda qkv=qkv, a=a: ops.axial_attention(qkv, *a),
                  bwd_fn=lambda qkv=qkv, dout=dout, a=a: ops.seq_attention_bwd(qkv, dout, *a))
        for k in ("fwd", "bwd"):
            try:
                sh[k + "_fn"]()
                torch.cuda.synchronize()
            except L.AcxError as ex:
                sh[k] = None
                sh[k + "_error"] = str(ex).splitlines()[0][:120]
        arms.append(sh)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rnd in range(args.rounds + 1):                      # round 0 warms up
        for sh in arms:
            for k in ("fwd", "bwd"):
                if sh[k] is None:
                    continue
                fn = sh[k + "_fn"]
                e0.record()
                for _ in range(args.inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rnd:
                    sh[k].append(e0.elapsed_time(e1) * 1e3 / args.inner)
    out = []
    print(f"# {args.label or 'axial_attn_bench'}: {torch.cuda.get_device_name(0)}, {args.rounds} rounds x {args.inner} launches, us per launch")
    for sh in arms:
        rec = {k: sh[k] for k in ("spec", "T", "other", "e", "heads", "axis", "rows")}
        line = f"{args.label:8s} {sh['spec']:>14s} rows {sh['rows']:6d}"
        for k in ("fwd", "bwd"):
            if sh[k] is None:
                line += f" | {k} unsupported ({sh[k + '_error']})"
                rec[k] = None
                continue
            med, lo, hi = statistics.median(sh[k]), min(sh[k]), max(sh[k])
            rec[k] = dict(us_median=round(med, 2), us_min=round(lo, 2), us_max=round(hi, 2), ns_per_row=round(med * 1e3 / sh["rows"], 3))
            line += f" | {k} {med:8.2f} us (min {lo:.2f} max {hi:.2f}) {med * 1e3 / sh['rows']:7.3f} ns/row"
            if k == "fwd":
                gbs = 16.0 * sh["heads"] * sh["e"] * sh["rows"] / (med * 1e-6) / 1e9
                rec[k]["gbytes_per_s"] = round(gbs, 1)
                line += f" {gbs:7.1f} GB/s"
        print(line)
        out.append(rec)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(dict(label=args.label, device=torch.cuda.get_device_name(0), rounds=args.rounds, inner=args.inner, shapes=out), f,
                      indent=1)


if __name__ == "__main__":
    main()
