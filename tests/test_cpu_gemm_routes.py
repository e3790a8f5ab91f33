"""acx_gemm_route (host arithmetic: no device, NULL context, dummy operand addresses) on every row of tests/gemm_ref.py's table, and
the table's own reference: ref() against independent fp64 evaluations, and torch fp32 inside the bound the GPU kernels are held
to -- the bound can be met by a plain f32 evaluation, so a kernel that misses it is wrong."""
import ctypes as C

import pytest
import torch

from anomalyclip_amd import _lib as L

import gemm_ref as G
import gemm_scratch_ref as GS


def _null_ctx_expectation(c):
    return c.default_ctx if c.default_ctx is not None else c.expect


@pytest.mark.parametrize("c", G.RUN_CASES, ids=[c.name for c in G.RUN_CASES])
def test_route_of_every_row(c):
    rc, got = G.query(None, G.desc(c))
    assert rc == 0, L.lib().acx_last_error(None)
    want = _null_ctx_expectation(c)
    assert got == want, (c.name, "got", G.ROUTE_NAMES[got[0]], got[1:], "want", G.ROUTE_NAMES[want[0]], want[1:])


@pytest.mark.parametrize("c", G.REFUSALS, ids=[c.name for c in G.REFUSALS])
def test_refusals(c):
    rc, got = G.query(None, G.desc(c))
    assert rc == c.refuse and got == (G.R_NONE, 1, 0, 0), (rc, got)
    assert c.text.encode() in L.lib().acx_last_error(None), L.lib().acx_last_error(None)


def test_query_arguments():
    d = G.desc(G.RUN_CASES[0])
    assert L.lib().acx_gemm_route(None, C.byref(d), None) == G.E_BADARG
    out = L.GemmRoute()
    assert L.lib().acx_gemm_route(None, None, C.byref(out)) == G.E_BADARG and out.route == G.R_NONE


def test_every_route_has_a_neighbour_on_the_other_side():
    """for every route and every split mechanism in scope there are rows that report it, and rows of the same M or N (the neighbouring
    shape) that report another route or another split"""
    by_route = {}
    for c in G.RUN_CASES:
        by_route.setdefault(c.expect[0], []).append(c)
    in_scope = {G.R_SK, G.R_S64, G.R_P256, G.R_W8, G.R_W8C, G.R_RING, G.R_P8, G.R_DMAC, G.R_DMA, G.R_GEN}
    assert set(by_route) == in_scope
    for route, rows in by_route.items():
        others = [c for c in G.RUN_CASES if c.expect[0] != route]
        near = [(a.name, b.name) for a in rows for b in others
                if a.prec == b.prec and a.amap == b.amap and (abs(a.M - b.M) <= 128 or a.M == b.M) and abs(a.N - b.N) <= 64]
        assert near, G.ROUTE_NAMES[route]
    for route in (G.R_SK, G.R_S64, G.R_W8C, G.R_GEN):                  # the routes that split: split and unsplit rows of one shape
        rows = by_route[route]
        assert any(a.expect[1] > 1 and b.expect[1] == 1 and (a.M, a.N) == (b.M, b.N) for a in rows for b in rows), G.ROUTE_NAMES[route]
    reduces = {(c.expect[0], c.expect[2]) for c in G.RUN_CASES}
    assert {(G.R_SK, 2), (G.R_S64, 1), (G.R_W8C, 1), (G.R_W8C, 2), (G.R_GEN, 1)} <= reduces
    # the 8-XCD remaps: fewer than 8 workgroups, nwg % 8 in 1 .. 7, for both w8 kernels
    for route in (G.R_W8, G.R_W8C):
        counts = {c.expect[3] for c in by_route[route] if c.expect[1] == 1}
        assert min(counts) < 8 and len({n % 8 for n in counts}) >= 4, counts


def _sample(rows, amap, n=3):
    return [c for c in rows if c.amap == amap and c.M <= 4096][:n]


@pytest.mark.parametrize("c", _sample(G.RUN_CASES, G.CONV, 6) + _sample(G.RUN_CASES, G.TESTTILE) + _sample(G.RUN_CASES, G.TILETABLE)
                         + _sample(G.RUN_CASES, G.IDENT, 4), ids=lambda c: c.name)
def test_ref_against_an_independent_evaluation(c):
    t = G.operands(c)
    r, S = G.ref(c, t)
    a, w = t["a"].double(), t["w"].double()
    if c.prec == G.BF16:
        a = t["a"].bfloat16().double()
    if c.a_sub:
        a = a - t["a_sub"].double()
    if c.amap == G.CONV:
        x = a.view(-1, c.gn, c.gl, c.cin).permute(0, 3, 1, 2)
        w4 = w.view(c.N, 3, 3, c.cin).permute(0, 3, 1, 2)
        y = torch.nn.functional.conv2d(x, w4, padding=1).permute(0, 2, 3, 1).reshape(c.M, c.N)
    else:
        y = torch.empty(c.M, c.N, dtype=torch.float64)
        for m in range(c.M):                              # an explicit gather, row by row
            if c.amap == G.TESTTILE:
                per = c.gn * c.gl * c.seg
                b_, rem = divmod(m, per)
                s_, rem = divmod(rem, c.gn * c.gl)
                n_, l_ = divmod(rem, c.gl)
                src = b_ * per + (n_ * c.seg + s_) * c.gl + l_
            elif c.amap == G.TILETABLE:
                tile, rem = divmod(m, c.gn * c.gl)
                n_, l_ = divmod(rem, c.gl)
                src = c.table[tile][0] + n_ * c.table[tile][1] + l_
            else:
                src = m
            y[m] = (w * a[src]).sum(1)
    if c.bias:
        y = y + t["bias"].double()
    y = {G.NONE: y, G.GELU: y / (1 + torch.exp(-1.702 * y)), G.LEAKY: torch.nn.functional.leaky_relu(y, 0.01), G.RELU: torch.relu(y),
         G.RESRELU: y}[c.act]
    if c.pos:
        y = (y.view(-1, c.gn, c.gl, c.N) + t["pos0"].double().view(1, c.gn, 1, c.N) + t["pos1"].double().view(1, 1, c.gl, c.N)).reshape(c.M, c.N)
    if c.res:
        y = y + t["res"].double()
    if c.act == G.RESRELU:
        y = torch.relu(y)
    assert bool(((y - r).abs() <= 1e-12 * S).all())
    assert bool((S >= r.abs() * (1 - 1e-12)).all()) or c.act in (G.GELU,)      # S bounds the value it is the magnitude of


WORST = {}


@pytest.mark.parametrize("c", G.RUN_CASES, ids=[c.name for c in G.RUN_CASES])
def test_torch_fp32_meets_the_bound(c):
    """torch fp32 on the CPU, rounded to bf16 where C is: inside bound() on every row (worst ratio: DESIGN.md)"""
    t = G.operands(c)
    r, S = G.ref(c, t)
    y = G.evaluate(c, t, torch.float32)
    if c.c_bf16:
        y = y.bfloat16()
    ratio = ((y.double() - r).abs() / G.bound(c, r, S)).max().item()
    WORST[c.name] = ratio
    print(f"fp32/bound {c.name}: {ratio:.3f}")
    assert torch.isfinite(y.float()).all() and ratio <= 1.0, ratio


def test_torch_fp32_worst_ratio_is_recorded():
    if len(WORST) == len(G.RUN_CASES):                    # (the whole table ran in this process)
        name = max(WORST, key=WORST.get)
        print(f"worst torch fp32 |err| / bound over {len(WORST)} rows: {WORST[name]:.3f} ({name})")
        assert WORST[name] <= 1.0


def test_operand_buffers_are_poisoned():
    c = next(c for c in G.RUN_CASES if c.name == "gen-k60")
    t = G.operands(c)
    assert t["a_buf"].shape == (c.M + 2, c.K + 4) and t["a_buf"].isnan().sum() == 2 * (c.K + 4) + 4 * c.M
    assert G.guards_intact(t["c_buf"], 0, 0) and G.guards_intact(t["res_buf"], c.M, c.N) and G.guards_intact(t["a_buf"], c.M, c.K)
    t["c"][:] = 1.0
    assert G.guards_intact(t["c_buf"], c.M, c.N)
    t["c_buf"][c.M, 0] = 1.0
    assert not G.guards_intact(t["c_buf"], c.M, c.N)


def test_x6_cases_report_the_plane_routes():
    picks = [("x6-256x768x768", G.R_X6, True), ("x6-256x768x352", G.R_X6, False), ("x6-65536x768x768", G.R_X6, False),
             ("x3-256x768x768", G.R_X6, True), ("x6-conv-256x128", G.R_X6, True), ("x6-ln-21760x768x768", G.R_X6, False)]
    cases = dict(GS.x6_cases())
    for name, route, splits in picks:
        d = GS.desc(**cases[name])
        nbytes, _ = GS.scratch_ref(d)
        if nbytes:
            d.workspace, d.workspace_bytes = 11 * 0x10000, nbytes
        rc, got = G.query(None, d)
        assert rc == 0 and got[0] == route and (got[1] > 1) == splits and got[2] == (1 if splits else 0), (name, got)
        assert got[3] == ((d.M + 255) // 256) * (1 if name.startswith("x6-conv-256x128") else (d.N + 255) // 256), (name, got)


# descriptors of gemm_scratch_ref.f32_cases() that the caller's (looser) rules hand scratch to and no route splits, and why
SCRATCH_UNUSED = {
    # the 64 x 64-tile kernel splits from K = 1024 and up to 256 of its tiles
    "f32-1281x512x768": "s64", "f32-2048x1024x256": "s64", "f32-2048x2048x1024": "s64",
    # bf16 pieces keep >= 8 K-steps of 64 (generic_ksplit)
    "bf16-77x512x512": "dma", "bf16-77x2048x512": "dma", "bf16-320x768x768": "dma", "bf16-321x768x768": "dma",
    "bf16-1280x512x768": "dma", "bf16-1281x512x768": "dma", "bf16-2048x1024x256": "dma",
    # few rows by the caller's rule but N % 4 != 0: not the few-row kernel's, and its pieces' scratch is smaller than the two partial
    # images the 128 x 128-tile split would need
    "f32-n510": "w8",
    # LeakyReLU on identity rows and the bf16 convolutions never split; an f32 convolution with a bf16 output is not the 8-wave kernel's
    "f32-leaky": "generic", "f32-leaky-tiles": "generic", "bf16-conv-256x64": "dma_conv", "bf16-conv-256x512": "dma_conv",
    "bf16-conv-4096x64": "dma_conv", "bf16-conv-4096x512": "dma_conv", "f32-conv-bf16out": "generic",
}


def test_split_exactly_where_the_scratch_rules_hand_out_scratch():
    """with the scratch acx_gemm_scratch recommends, the query reports a K split exactly where the frozen rules of gemm_scratch_ref
    hand out scratch that a route uses: everywhere but on SCRATCH_UNUSED, and never without scratch"""
    lib = L.lib()
    seen, unused = 0, {}
    for name, kw in GS.f32_cases():
        d = GS.desc(**kw)
        need = L.GemmScratch()
        assert lib.acx_gemm_scratch(None, C.byref(d), 1, C.byref(need)) == 0
        assert (need.workspace_bytes, need.counters) == GS.scratch_ref(d), name
        if need.workspace_bytes:
            d.workspace, d.workspace_bytes = 11 * 0x10000, need.workspace_bytes
        if need.counters:
            d.counters, d.n_counters = 12 * 0x10000, 4095
        rc, got = G.query(None, d)
        if rc:                                            # (bf16 with K = 252 or with a_sub: acx_gemm refuses them, so does the query)
            assert rc == G.E_BADARG and d.prec == G.BF16 and (d.K % 8 or d.a_sub), name
            continue
        splits = got[1] > 1
        assert not (splits and not need.workspace_bytes), (name, got)
        if need.workspace_bytes and not splits:
            unused[name] = G.ROUTE_NAMES[got[0]]
        if splits and need.counters:
            assert got[2] == G.RED_COUNTERS, (name, got)
        seen += splits
    assert unused == SCRATCH_UNUSED
    assert seen >= 20
