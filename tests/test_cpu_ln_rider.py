"""No device: the host-side plan of acx_gemm_ln (how many LayerNorm rows ride in a residual product's partly filled last round of
tiles) and the register table of the plane-reuse kernel, whose pre-existing instantiations the rider must not touch."""
import os
import re

import pytest

from anomalyclip_amd import _build
from anomalyclip_amd import ops

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (M, N, K): the ViT-B/16 residual products at 512 / 256 / 230 / 160 frames, ViT-L/14 (257-token rows, N = 1024), an exact multiple
# of the CU count (768 tiles), fewer tiles than CUs, M not a multiple of 256
SHAPES = [(100864, 768, 768), (100864, 768, 3072), (50432, 768, 768), (50432, 768, 3072), (45310, 768, 768), (31520, 768, 3072),
          (77100, 1024, 1024), (77100, 1024, 4096), (65536, 768, 768), (2048, 768, 768), (100000, 768, 3072)]


@pytest.mark.parametrize("M,N,K", SHAPES)
@pytest.mark.parametrize("ncu", [256, 240, 64])
def test_plan_invariants(M, N, K, ncu):
    ride, ready = ops.ln_rider_plan(M, N, K, ncu)
    tiles_n, tiles = N // 256, (M + 255) // 256 * (N // 256)
    rounds, rem = divmod(tiles, ncu)
    assert 0 <= ride <= ready <= M
    assert ride % 2 == 0
    if rounds < 1 or rem == 0:
        assert ride == 0 and ready == 0                                  # no partial round (or fewer tiles than workgroups)
    else:
        assert ready <= rounds * ncu // tiles_n * 256                    # only rows whose every column tile lies in the full rounds
    assert ops.ln_rider_plan(M, N, K, ncu, ksplit=2) == (0, 0)           # a K split never rides
    # monotone in the rate constant, saturating at the completed rows
    last = 0
    for rate in (1e-3, 0.1, 0.5, 1.0, 2.0, 8.0, 1e6):
        r, rd = ops.ln_rider_plan(M, N, K, ncu, rate=rate)
        assert rd == ready and r % 2 == 0 and last <= r <= ready
        last = r
    assert last == ready - (ready & 1)


def test_plan_bench_shape():
    """512 frames of ViT-B/16 on 256 CUs: 1,182 tiles = 4 full rounds + 158; row blocks 0 .. 340 are complete before the last round"""
    for K in (768, 3072):
        ride, ready = ops.ln_rider_plan(100864, 768, K, 256)
        assert ready == 341 * 256 and 0 < ride <= ready
    assert ops.ln_rider_plan(100864, 768, 3072, 256)[0] >= ops.ln_rider_plan(100864, 768, 768, 256)[0]    # the longer tail takes more
    # 256 frames: 591 tiles = 2 rounds + 79, the last round as 158 strips of 128 columns: 98 riders, row blocks 0 .. 169 complete
    assert ops.ln_rider_plan(50432, 768, 768, 256)[1] == 170 * 256


def test_existing_x6_instantiations_keep_their_registers():
    """Every gemm_x6_p4_kernel instantiation that existed before the rider flag (tests/golden/x6_kernel_registers.tsv: the table of
    the commit before it, by template arguments) keeps its VGPR / AGPR counts and uses no scratch in the library as built; the
    rider instantiations exist, for the f32 residual epilogue only, and use no scratch either."""
    from anomalyclip_amd import _lib
    _lib.lib()
    rows = _build.kernel_resources()
    now = {}
    for k, v in rows.items():
        if "gemm_x6_p4_kernel" in k:
            now[tuple(int(x) for x in re.findall(r"Li(\d+)E", k.split("gemm_x6_p4_kernelI")[1]))] = v
    assert all(len(t) == 10 for t in now), sorted(now)[:3]
    with open(os.path.join(REPO, "tests", "golden", "x6_kernel_registers.tsv")) as fh:
        fh.readline()
        before = [ln.rstrip("\n").split("\t") for ln in fh if ln.strip()]
    assert len(before) == 68
    for targs, vgpr, agpr, scratch in before:
        t = tuple(int(x) for x in targs.split(",")) + (0,)
        assert t in now, t
        v = now[t]
        assert (v["VGPRs"], v["AGPRs"], v["ScratchSize [bytes/lane]"]) == (int(vgpr), int(agpr), int(scratch)), (t, v)
    riders = sorted(t for t in now if t[9] == 1)
    assert riders == [(0, 0, 1, 0, 0, 0, ni, 0, 0, 1) for ni in (1, 2, 4)], riders
    for t in riders:
        assert now[t]["ScratchSize [bytes/lane]"] == 0 and now[t]["VGPRs Spill"] == 0 and now[t]["AGPRs"] == now[t[:9] + (0,)]["AGPRs"]
    assert len(now) == len(before) + len(riders)
