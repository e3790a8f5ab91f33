"""-m gpu: acx_gemm on every row of tests/gemm_ref.py's table -- the route asserted with acx_gemm_route on the live context, then
EVERY element of [0, M) x [0, N) finite and within bound() of the fp64 reference (no norm, no allowance for outliers), every guard
element of C still its NaN pattern bit for bit, split rows run twice and torch.equal, arrival counters zero afterwards.  Descriptors
are filled by hand (tests/test_gpu_gemm_scratch.py's _direct): padded leading dimensions, scratch brought or withheld per row.
Refusal rows: the query and acx_gemm answer the same code and nothing is written."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L

import gemm_ref as G
import gemm_scratch_ref as GS

DEV = "cuda"
WORST = {}                                               # route -> (worst |err| / bound, row): printed by the last test


@pytest.fixture(scope="module")
def own_ctx():
    """a context of the file's own: the options the ring / p8 rows set never reach the one the package works with"""
    lib, h = L.lib(), C.c_void_p()
    assert lib.acx_create(C.byref(h), torch.cuda.current_device()) == 0
    assert torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count == G.NCU
    try:
        yield h
    finally:
        lib.acx_destroy(h)


class _Options:
    def __init__(self, h, opts):
        self.h, self.opts, self.before = h, opts, {}

    def __enter__(self):
        lib = L.lib()
        for opt, value in self.opts.items():
            v = C.c_int64(-1)
            assert lib.acx_get_option(self.h, opt, C.byref(v)) == 0
            self.before[opt] = int(v.value)
            assert lib.acx_set_option(self.h, opt, value) == 0

    def __exit__(self, *exc):
        for opt, value in self.before.items():
            assert L.lib().acx_set_option(self.h, opt, value) == 0


def _scratch(c, d, t):
    """what the row's caller brings: a poisoned workspace (a partial image that is summed without having been written shows as NaN),
    zeroed counters, the zero page, the tile table"""
    if c.ws:
        t["ws"] = torch.full((c.ws_bytes // 4,), G.NAN32, dtype=torch.int32, device=DEV)
        d.workspace, d.workspace_bytes = t["ws"].data_ptr(), c.ws_bytes
    if c.ctr:
        t["ctr"] = torch.zeros(c.ctr, dtype=torch.int32, device=DEV)
        d.counters, d.n_counters = t["ctr"].data_ptr(), c.ctr
    if c.amap == G.CONV:
        t["zero"] = torch.zeros(256, dtype=torch.float32, device=DEV)
        d.zero_page = t["zero"].data_ptr()
    if c.amap == G.TILETABLE:
        d.tile_table = t["table"].data_ptr()


def _run(h, c):
    """-> (output [M, N] as stored, fp64 reference, S, the operands)"""
    t = G.operands(c, DEV)
    r, S = G.ref(c, t)
    d = G.desc(c, t)
    _scratch(c, d, t)
    rc, got = G.query(h, d)
    assert rc == 0 and got == c.expect, (c.name, "got", G.ROUTE_NAMES[got[0]], got[1:], "want", G.ROUTE_NAMES[c.expect[0]], c.expect[1:])
    rc = L.lib().acx_gemm(h, C.byref(d), torch.cuda.current_stream().cuda_stream)
    assert rc not in (G.E_BADARG, G.E_UNSUPPORTED), (c.name, L.lib().acx_last_error(h))
    try:
        L.check(rc, h)
        torch.cuda.synchronize()
    except Exception as e:                                # a launch or device error: nothing more is started on this GPU
        pytest.exit(f"device error in acx_gemm on row {c.name}, the session ends here: {e}", returncode=3)
    return t["c"], r, S, t


@pytest.mark.parametrize("c", G.RUN_CASES, ids=[c.name for c in G.RUN_CASES])
def test_every_element_against_fp64(c, own_ctx):
    with _Options(own_ctx, c.opts):
        out, r, S, t = _run(own_ctx, c)
        assert bool(torch.isfinite(out.float()).all()), c.name
        ratio = ((out.double() - r).abs() / G.bound(c, r, S)).max().item()
        print(f"gemm-route-ratio {G.ROUTE_NAMES[c.expect[0]]} {c.name} {ratio:.4f}")
        if ratio > WORST.get(c.expect[0], (0.0, ""))[0]:
            WORST[c.expect[0]] = (ratio, c.name)
        assert ratio <= 1.0, (c.name, ratio)
        assert G.guards_intact(t["c_buf"], c.M, c.N), c.name
        for k in ("a_buf", "w_buf"):                      # (the operands are read only)
            assert G.guards_intact(t[k], t[k].shape[0] - 2, t[k[0]].shape[1])
        if c.res == "own":
            assert G.guards_intact(t["res_buf"], c.M, c.N)
        if c.ctr:
            assert int(t["ctr"].abs().sum()) == 0, c.name  # the arrival counters are zero at rest
        if c.expect[1] > 1:                               # a K split sums in a fixed order
            again, _, _, t2 = _run(own_ctx, c)
            assert torch.equal(out, again), c.name
            if c.ctr:
                assert int(t2["ctr"].abs().sum()) == 0, c.name


@pytest.mark.parametrize("c", G.REFUSALS, ids=[c.name for c in G.REFUSALS])
def test_refusals_write_nothing(c, own_ctx):
    lib = L.lib()
    with _Options(own_ctx, c.opts):
        t = G.operands(c, DEV)
        d = G.desc(c, t)
        if c.amap == G.TILETABLE:
            d.tile_table = t["table"].data_ptr()
        if c.amap == G.CONV:
            t["zero"] = torch.zeros(256, dtype=torch.float32, device=DEV)
            d.zero_page = t["zero"].data_ptr()
        for k, v in c.raw.items():
            setattr(d, k, v)
        rc, got = G.query(own_ctx, d)
        assert rc == c.refuse and got == (G.R_NONE, 1, 0, 0), (rc, got)
        assert c.text.encode() in lib.acx_last_error(own_ctx)
        assert lib.acx_gemm(own_ctx, C.byref(d), torch.cuda.current_stream().cuda_stream) == c.refuse
        assert c.text.encode() in lib.acx_last_error(own_ctx)
        torch.cuda.synchronize()
        assert G.guards_intact(t["c_buf"], 0, 0)


def test_x6_tail_split_is_reported(own_ctx):
    """280 tiles of 256 x 256 on 256 CUs with the opt-in tail split: the 24 tiles of the last round as a K-split problem of 4 pieces"""
    lib = L.lib()
    d = GS.desc(256 * 70, 1024, 768, pairs=6, residual=True)
    answers = []
    for on in (0, 1):
        with _Options(own_ctx, {L.OPT_X6_TAIL_SPLIT: on}):
            need = L.GemmScratch()
            assert lib.acx_gemm_scratch(own_ctx, C.byref(d), 1, C.byref(need)) == 0
            d.workspace, d.workspace_bytes = (11 * 0x10000, need.workspace_bytes) if need.workspace_bytes else (None, 0)
            answers.append(G.query(own_ctx, d))
    assert answers[0] == (0, (G.R_X6, 1, 0, 280)) and answers[1] == (0, (G.R_TAIL, 4, G.RED_LAUNCH, 280)), answers


def test_worst_ratio_per_route():
    for route, (ratio, name) in sorted(WORST.items()):
        print(f"gemm-route-worst {G.ROUTE_NAMES[route]} {ratio:.4f} {name}")
    assert all(ratio <= 1.0 for ratio, _ in WORST.values())
