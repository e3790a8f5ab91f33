"""acx_gemm_tn_route / acx_gemm_tn_x6_route (host arithmetic: no device, NULL context, no operands) on every row of tests/tn_ref.py's
table, and the table's own reference: ref() against independent fp64 evaluations, and torch fp32 inside the bound the GPU kernels
are held to -- the bound can be met by a plain f32 evaluation, so a kernel that misses it is wrong."""
import ctypes as C

import pytest
import torch

from anomalyclip_amd import _lib as L

import tn_ref as T


def _null_ctx_expectation(c):
    return c.default_ctx if c.default_ctx is not None else c.expect


@pytest.mark.parametrize("c", T.RUN_CASES, ids=[c.name for c in T.RUN_CASES])
def test_route_of_every_row(c):
    rc, got, clears = T.query(None, c)
    assert rc == 0, L.lib().acx_last_error(None)
    want = _null_ctx_expectation(c)
    assert got == want, (c.name, "got", T.KERNEL_NAMES[got[0]], got[1:], "want", T.KERNEL_NAMES[want[0]], want[1:])
    assert clears == int(want[0] == T.K_P256 and not c.zp)
    if got[1] > 1:                                        # the row ranges cover M, and only the 256 x 256 kernel leaves one empty
        assert got[1] * got[2] >= c.M
        assert (got[1] - 1) * got[2] < c.M or (got[0] == T.K_P256 and c.name == "p256-empty-split")


@pytest.mark.parametrize("c", [c for c in T.REFUSALS if not c.call_only], ids=lambda c: c.name)
def test_refusals(c):
    rc, got, clears = T.query(None, c)
    assert rc == c.refuse and got == T.NO_ROUTE and clears == 0, (rc, got)
    assert c.text.encode() in L.lib().acx_last_error(None), L.lib().acx_last_error(None)


def test_query_arguments():
    lib = L.lib()
    assert lib.acx_gemm_tn_route(None, 256, 128, 128, 128, 128, 128, 0, 0, 0, 0, 0, 0, 0, 0, 0, None) == T.E_BADARG
    assert lib.acx_gemm_tn_x6_route(None, 256, 256, 256, 256, 256, 256, 0, 0, 0, 0, 0, 0, 1, None) == T.E_BADARG
    out = L.GemmTnRoute()
    assert lib.acx_gemm_tn_route(None, 0, 128, 128, 128, 128, 128, 0, 0, 0, 0, 0, 0, 0, 0, 0, C.byref(out)) == T.E_BADARG
    assert b"empty shape" in lib.acx_last_error(None) and out.kernel == T.K_NONE and out.splits == 1


def test_every_kernel_and_both_sides_of_every_gate():
    """every route constant is reported by a run row; every gate of tn_takes_p256, of the workspace fallbacks and of tn_x6_mode has
    a row on each side (the neighbour differs in the one quantity the gate reads)"""
    rows = {c.name: c for c in T.RUN_CASES}
    assert {c.expect[0] for c in T.RUN_CASES} == {T.K_W8, T.K_P256, T.K_X6_256x256, T.K_X6_256x128, T.K_X6_128x256}
    assert {(c.expect[0], c.expect[4]) for c in T.RUN_CASES} >= {(T.K_W8, 0), (T.K_W8, 1), (T.K_W8, 2), (T.K_P256, 0), (T.K_P256, 1),
                                                                (T.K_P256, 2), (T.K_X6_256x256, 0), (T.K_X6_256x256, 1)}
    sides = [("p256-4096x256x2048", "w8-rows-4095"), ("p256-n1-192", "w8-n1-188"), ("p256-n2-256", "w8-n2-252"),
             ("p256-n2-1796-8-tiles", "w8-n2-1792-7-tiles"), ("p256-4096x256x2048", "w8-p256-shape-bsub"),
             ("p256-ragged", "w8-p256-withheld"), ("p256-4096x256x2048", "p256-min-rows-4097-w8"),
             ("p256-three-images", "p256-three-images-less-1"), ("p256-ragged-own-zero-page", "p256-one-image-own-zero-page"),
             ("x6_256x256-m1000", "x6_256x128-m1000"), ("x6_256x256-m1000", "x6_128x256-m1000"),
             ("x6c_256x256-4x4", "x6c_256x128-4x4"), ("x6c_256x256-8x32", "x6c_128x256-8x32"),
             ("x6_256x256-m1000", "x6_256x256-m1000-no-workspace"), ("x6_256x256-m1000-two-images", "x6_256x256-m1000-two-images-less-1")]
    for a, b in sides:
        assert rows[a].expect != rows[b].expect or rows[a].default_ctx != rows[b].default_ctx, (a, b)
    refused = {c.name for c in T.REFUSALS}
    assert {"w8-p256-shape-no-workspace-refused", "p256-512-bytes-w8-refused", "x6-128x128", "x6-conv-cin128-n1-128"} <= refused
    # the three row-map branches of the 8-wave kernel and the two of the 256 x 256 kernel
    convs = [c for c in T.RUN_CASES if c.conv and not c.x6]
    pow2 = lambda v: v & (v - 1) == 0                     # noqa: E731
    for kern in (T.K_W8, T.K_P256):
        mine = [c for c in convs if c.expect[0] == kern]
        assert any(pow2(c.gl) and pow2(c.gn * c.gl) and c.gl > 16 for c in mine)             # shifts
        assert any(not pow2(c.gl) for c in mine) and (kern == T.K_P256 or any(pow2(c.gl) and not pow2(c.gn) for c in mine))
    assert any(pow2(c.gn * c.gl) and c.gl <= 16 for c in convs if c.expect[0] == T.K_W8)    # fastconv
    assert any(c.expect[1] > 1 and c.M % (c.gn * c.gl) == 0 and c.expect[2] % (c.gn * c.gl) for c in convs)   # splits cut grid tiles
    assert len(T.GROUP) == 10 and sum(rows[n].b_sub for n in T.GROUP) == 2 and any(rows[n].pad_a for n in T.GROUP)
    assert {rows[n].expect[1] > 1 for n in T.GROUP} == {False, True} and not any(rows[n].conv or rows[n].x6 for n in T.GROUP)


def _conv_sample():
    return [c for c in T.RUN_CASES if c.conv and c.M * c.N1 * c.N2 <= 1 << 28]


@pytest.mark.parametrize("c", _conv_sample(), ids=lambda c: c.name)
def test_ref_against_conv2d_weight_gradient(c):
    """the row map of ref() against torch's own convolution: the weight gradient of conv2d(padding = 1) in fp64"""
    t = T.operands(c)
    r, S = T.ref(c, t)
    x = t["b"].double().view(-1, c.gn, c.gl, c.cin).permute(0, 3, 1, 2)
    dy = t["a"].double().view(-1, c.gn, c.gl, c.N1).permute(0, 3, 1, 2)
    gw = torch.nn.grad.conv2d_weight(x, (c.N1, c.cin, 3, 3), dy, padding=1)          # [N1, cin, 3, 3]
    y = gw.permute(0, 2, 3, 1).reshape(c.N1, 9 * c.cin)                              # [N1][tap][cin]
    assert bool(((y - r).abs() <= 1e-12 * S + 1e-300).all())
    assert bool((S >= r.abs() * (1 - 1e-12)).all())


def test_ref_identity_rows_with_b_sub():
    c = T.by_name("w8-33-padded-bsub")
    t = T.operands(c)
    r, S = T.ref(c, t)
    y = torch.zeros(c.N1, c.N2, dtype=torch.float64)
    for m in range(c.M):                                  # one outer product per row
        y += torch.outer(t["a"][m].double(), t["b"][m].double() - t["b_sub"].double())
    assert bool(((y - r).abs() <= 1e-12 * S).all())


WORST = {}


@pytest.mark.parametrize("c", T.RUN_CASES, ids=[c.name for c in T.RUN_CASES])
def test_torch_fp32_meets_the_bound(c):
    """torch fp32 on the CPU from the same operands with the same row map: inside bound() on every row (worst ratio: DESIGN.md)"""
    t = T.operands(c)
    r, S = T.ref(c, t)
    y = T.evaluate(c, t, torch.float32)
    ratio = ((y.double() - r).abs() / T.bound(c, S).clamp_min(1e-300)).max().item()
    WORST[c.name] = ratio
    print(f"fp32/bound {c.name}: {ratio:.3f}")
    assert torch.isfinite(y).all() and ratio <= 0.5, ratio


def test_torch_fp32_worst_ratio_is_recorded():
    if len(WORST) == len(T.RUN_CASES):                    # (the whole table ran in this process)
        name = max(WORST, key=WORST.get)
        print(f"worst torch fp32 |err| / bound over {len(WORST)} rows: {WORST[name]:.3f} ({name})")
        assert WORST[name] <= 0.5


def test_operand_buffers_are_poisoned():
    c = T.by_name("w8-700-padded")
    t = T.operands(c)
    assert t["a_buf"].shape == (c.M + 2, c.N1 + 4) and t["a_buf"].isnan().sum() == 2 * (c.N1 + 4) + 4 * c.M
    assert t["b_buf"].shape == (c.M + 2, c.N2 + 12) and t["c_buf"].shape == (c.N1 + 2, c.N2)
    assert T.guards_intact(t["c_buf"], 0, 0) and T.guards_intact(t["a_buf"], c.M, c.N1) and T.guards_intact(t["b_buf"], c.M, c.N2)
    t["c"][:] = 1.0
    assert T.guards_intact(t["c_buf"], c.N1, c.N2)
    t["c_buf"][c.N1, 0] = 1.0
    assert not T.guards_intact(t["c_buf"], c.N1, c.N2)
