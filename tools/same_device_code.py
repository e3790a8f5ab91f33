#!/usr/bin/env python3
"""python tools/same_device_code.py <rev>: is the device code of this tree the device code of <rev>?

Every file of _build.SOURCES is compiled to gfx950 assembly (the build's compiler and flags + --cuda-device-only -S) twice: from a
`git archive` of <rev> (csrc/ and include/ in their places) and from the working tree.  Lines with the __hip_cuid_<hash> symbol (a hash
of the source text) are dropped, the rest is compared.  One line per source: `same`, or the mangled names of the functions whose text
differs.  A function inserted in front of others renumbers their local labels (.LBB<function ordinal>_<block>, .Lfunc_end<ordinal>) and shifts the
column of the comments behind them, so functions whose text differs are compared once more with the labels' function ordinal
and the comments dropped: `... in labels and comments only` then means the instructions, their order and the kernel descriptors are the
same.  Exit status 1 if any function differs beyond that.  The tool only diffs -- it never looks at what the assembly holds -- and needs
no GPU."""
import io
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from anomalyclip_amd import _build  # noqa: E402

CSRC_REL = os.path.relpath(_build.CSRC, ROOT)


def device_asm(root: str, src: str, out: str) -> list:
    cmd = [_build.HIPCC, *_build.FLAGS, "--cuda-device-only", "-S", os.path.join(root, CSRC_REL, src), "-o", out]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f"hipcc failed on {os.path.join(root, CSRC_REL, src)}:\n{r.stdout}")
    with open(out) as fh:
        return [line for line in fh if "__hip_cuid_" not in line]


def functions(lines: list) -> dict:
    """{name: text}: a function's code from its label to the next function's, and its .amdhsa_kernel ... .end_amdhsa_kernel section"""
    out, cur = {}, "(outside any function)"
    for line in lines:
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line) or re.match(r"([A-Za-z_][\w$.]*):", line)
        if m and not m.group(1).startswith(".L"):
            cur = m.group(1)
        out[cur] = out.get(cur, "") + line
        if line.strip() == ".end_amdhsa_kernel":
            cur = "(outside any function)"
    return out


def code_only(text: str) -> list:
    """a function's lines without comments, the function ordinal of its block labels replaced"""
    out = []
    for line in text.split("\n"):
        line = re.sub(r"(\.L)?(BB|func_begin|func_end|tmp)\d+", r"\2", line.split(";")[0]).rstrip()
        if line:
            out.append(line)
    return out


def metadata_grew_only(a: str, b: str) -> bool:
    """amdhsa.kernels (one YAML entry per kernel): every entry of <rev> is in the tree unchanged"""
    def entries(text):
        out = {}
        for e in re.split(r"\n(?=  - \.)", text):
            m = re.search(r"\.name:\s+(\S+)", e)
            if m:
                out[m.group(1)] = e.rstrip()
        return out
    ea, eb = entries(a), entries(b)
    return bool(ea) and all(eb.get(k) == v for k, v in ea.items())


def main() -> int:
    if len(sys.argv) != 2:
        print(__doc__, file=sys.stderr)
        return 2
    rev = sys.argv[1]
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "-C", ROOT, "archive", rev, "--", CSRC_REL, "include"], stdout=subprocess.PIPE, check=True).stdout
        tarfile.open(fileobj=io.BytesIO(tar)).extractall(os.path.join(tmp, "rev"))
        with ThreadPoolExecutor(max_workers=min(16, os.cpu_count() or 1)) as pool:
            jobs = [(src, pool.submit(device_asm, os.path.join(tmp, "rev"), src, os.path.join(tmp, src + ".rev.s")),
                     pool.submit(device_asm, ROOT, src, os.path.join(tmp, src + ".tree.s"))) for src in _build.SOURCES]
            differ = 0
            for src, a, b in jobs:
                a, b = a.result(), b.result()
                if a == b:
                    print(f"{src}: same")
                    continue
                fa, fb = functions(a), functions(b)
                names = sorted(k for k in fa.keys() | fb.keys() if fa.get(k) != fb.get(k))
                new = [k for k in names if k not in fa]
                gone = [k for k in names if k not in fb]
                real = [k for k in names if k in fa and k in fb and k != "(outside any function)" and code_only(fa[k]) != code_only(fb[k])
                        and not (k == "amdhsa.kernels" and metadata_grew_only(fa[k], fb[k]))]
                if not real and not gone and names:
                    print(f"{src}: {len(fa) - 1} functions of <rev> present, same in labels and comments only "
                          f"({len(names) - len(new)} texts renumbered); new: " + (" ".join(new) if new else "none"))
                    continue
                differ += 1
                print(f"{src}: DIFFERENT in " + (" ".join(real + gone) if names else "the order of its functions only") +
                      ("; new: " + " ".join(new) if new else ""))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
