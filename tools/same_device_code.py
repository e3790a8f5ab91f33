#!/usr/bin/env python3
"""python tools/same_device_code.py <rev>: is the device code of this tree the device code of <rev>?

Every file of _build.SOURCES is compiled to gfx950 assembly (the build's compiler and flags + --cuda-device-only -S) twice: from a
`git archive` of <rev> (csrc/ and include/ in their places) and from the working tree.  Lines with the __hip_cuid_<hash> symbol (a hash
of the source text) are dropped, the rest is compared.  One line per source: `same`, or the mangled names of the functions whose text
differs.  Exit status 1 if anything differs.  The tool only diffs -- it never looks at what the assembly holds -- and needs no GPU."""
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
                differ += 1
                fa, fb = functions(a), functions(b)
                names = sorted(k for k in fa.keys() | fb.keys() if fa.get(k) != fb.get(k))
                print(f"{src}: DIFFERENT in " + (" ".join(names) if names else "the order of its functions only"))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
