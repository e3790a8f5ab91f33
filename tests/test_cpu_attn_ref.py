"""No device: the reference of the attention route sweep (tests/attn_ref.py) and the library's two route queries.

  - the closed forms equal fp64 autograd of the plain softmax-attention expression to 1e-12 * S;
  - torch's fp32 CPU evaluation of that expression, autograd included, stays below 1e-6 * S on every case of the GPU table --
    the condition that makes 2e-6 * S a bound a correct fp32 kernel can meet, measured on the reference and never on the kernels;
  - acx_seq_attention_bwd_route / acx_axial_attention_route, through the C ABI with a null context, at every boundary of the
    dispatch rules and on every case of the table: the table's route tags are the library's own answers."""
import pytest
import torch

from anomalyclip_amd import _lib as L

import attn_ref as AR

C = AR.Case
# both axes, causal and not, T = 1, e in {16, 32, 64}
FORM_CASES = [C("-", 1, 3, 16, 2, 0, 0, 2, None, True), C("-", 1, 3, 64, 2, 1, 1, 2, None, True), C("-", 7, 3, 16, 2, 0, 0, 2, None, True),
              C("-", 7, 3, 32, 3, 1, 0, 2, None, True), C("-", 7, 3, 64, 1, 0, 1, 2, None, True), C("-", 16, 5, 32, 3, 1, 1, 3, None, True),
              C("-", 33, 2, 16, 3, 0, 1, 2, None, True), C("-", 33, 2, 64, 2, 1, 0, 2, None, True), C("-", 77, 1, 64, 3, 1, 1, 2, None, True),
              C("-", 77, 1, 64, 3, 1, 0, 2, None, True), C("-", 100, 2, 32, 1, 0, 0, 2, None, True), C("-", 40, 2, 64, 2, 0, 0, 2, "tile", True),
              C("-", 40, 1, 64, 2, 1, 1, 2, "last", True)]
ALL = AR.CASES + AR.GUARD_CASES


def _args(c):
    return (*AR.grid(c), c.heads, c.e, c.axis, c.causal, c.e ** -0.5)


@pytest.mark.parametrize("c", FORM_CASES, ids=AR.case_id)
def test_closed_forms_equal_fp64_autograd(c):
    qkv, dout, ref = AR.reference(c)
    auto = AR.autograd(qkv, dout, *_args(c), torch.float64)
    for name, (val, S) in ref.items():
        assert val.shape == auto[name].shape and bool((S >= 0).all())
        AR.within(auto[name], val, S, f"{name} {AR.case_id(c)}", "fp64_autograd", tol=1e-12)


def test_masked_pairs_add_nothing():
    """causal: the first query sees one key -- P = 1, dS = 0 and its dq is 0 -- and the last key's dv comes from the last query alone"""
    c = C("-", 9, 2, 16, 2, 1, 1, 2, None, True)
    qkv, dout, ref = AR.reference(c)
    first = torch.arange(0, qkv.shape[0], c.T)
    dq, s_dq = ref["dq"]
    assert bool((dq[first].abs() <= 1e-12 * s_dq[first]).all())
    q, k, v, dO = AR._split(qkv, dout, *AR.grid(c), c.heads, c.e, c.axis, torch.float64)
    dv = AR.to_lines(ref["dv"][0].contiguous(), *AR.grid(c), c.heads, c.e, c.axis)
    s = c.e ** -0.5 * (q[:, -1:] @ k.transpose(1, 2))
    assert torch.allclose(dv[:, -1], torch.softmax(s, -1)[:, 0, -1:] * dO[:, -1], rtol=1e-12, atol=0)


@pytest.mark.parametrize("c", ALL, ids=AR.case_id)
def test_torch_fp32_stays_below_half_the_bound(c):
    qkv, dout, ref = AR.reference(c)
    auto = AR.autograd(qkv, dout, *_args(c), torch.float32)
    for name, (val, S) in ref.items():
        AR.within(auto[name], val, S, f"{name} {AR.case_id(c)}", "torch_fp32", tol=1e-6)


# ------------------------------------------------------------------------------------------------------------- route queries
def bwd(gn, gl, e, axis, causal=0, has_stats=1, tiles=2, heads=3):
    return L.lib().acx_seq_attention_bwd_route(None, tiles, gn, gl, heads, e, axis, causal, has_stats)


def fwd(gn, gl, e, axis, aligned=1, heads=4):
    return L.lib().acx_axial_attention_route(None, gn, gl, heads, e, axis, aligned)


def test_backward_route_text_boundaries():
    for causal in (0, 1):
        for stats in (0, 1):
            assert bwd(1, 1, 64, 1, causal, stats) == L.SAB_ROUTE_TEXT_MFMA
            assert bwd(1, 80, 64, 1, causal, stats) == L.SAB_ROUTE_TEXT_MFMA
            assert bwd(1, 81, 64, 1, causal, stats) == L.SAB_ROUTE_TEXT_BLOCK
            assert bwd(1, 128, 64, 1, causal, stats) == L.SAB_ROUTE_TEXT_BLOCK
            assert bwd(1, 257, 64, 1, causal, stats) == L.SAB_ROUTE_UNSUPPORTED
        assert bwd(1, 129, 64, 1, causal, 1) == L.SAB_ROUTE_TEXT_ROWS
        assert bwd(1, 256, 64, 1, causal, 1) == L.SAB_ROUTE_TEXT_ROWS
        assert bwd(1, 129, 64, 1, causal, 0) == L.SAB_ROUTE_GENERIC            # no stats_ws: the thread-per-row kernel
        assert bwd(1, 256, 64, 1, causal, 0) == L.SAB_ROUTE_GENERIC
    # the text kernels take gn = 1 along axis 1 with e = 64 only
    assert bwd(2, 77, 64, 1) == L.SAB_ROUTE_GENERIC and bwd(77, 1, 64, 0) == L.SAB_ROUTE_GENERIC
    assert bwd(1, 77, 32, 1, 1) == L.SAB_ROUTE_GENERIC


def test_backward_route_axial_boundaries():
    for e in (16, 32):
        for axis in (0, 1):
            g = (lambda T: (T, 5)) if axis == 0 else (lambda T: (5, T))
            for T in (16, 32):
                assert bwd(*g(T), e, axis) == L.SAB_ROUTE_AXIAL_MFMA
                assert bwd(*g(T - 1), e, axis) == L.SAB_ROUTE_AXIAL_MFMA_PADDED
                assert bwd(*g(T + 1), e, axis) == L.SAB_ROUTE_AXIAL_MFMA_PADDED
                assert bwd(*g(T), e, axis, causal=1) == L.SAB_ROUTE_GENERIC      # causal never runs on the axial MFMA kernels
            assert bwd(*g(1), e, axis) == L.SAB_ROUTE_AXIAL_MFMA_PADDED
            assert bwd(*g(64), e, axis) == L.SAB_ROUTE_AXIAL_MFMA_PADDED
            assert bwd(*g(65), e, axis) == L.SAB_ROUTE_GENERIC
            assert bwd(*g(256), e, axis) == L.SAB_ROUTE_GENERIC
            assert bwd(*g(257), e, axis) == L.SAB_ROUTE_UNSUPPORTED
            assert bwd(*g(300), e, axis) == L.SAB_ROUTE_UNSUPPORTED
            assert bwd(*g(0), e, axis) == L.SAB_ROUTE_UNSUPPORTED
    assert bwd(24, 5, 32, 0, causal=1) == L.SAB_ROUTE_GENERIC
    for T in (16, 32, 64, 65):                                                   # e = 64 off the text shape: always generic
        assert bwd(T, 5, 64, 0) == L.SAB_ROUTE_GENERIC and bwd(5, T, 64, 1) == L.SAB_ROUTE_GENERIC
    for e in (48, 8, 128, 0):
        assert bwd(16, 5, e, 0) == L.SAB_ROUTE_UNSUPPORTED and bwd(1, 77, e, 1) == L.SAB_ROUTE_UNSUPPORTED
    # has_stats moves nothing off the text shape
    assert bwd(16, 5, 32, 0, has_stats=0) == L.SAB_ROUTE_AXIAL_MFMA and bwd(100, 5, 32, 0, has_stats=0) == L.SAB_ROUTE_GENERIC


def test_forward_route_boundaries():
    for e in (16, 32):
        for axis in (0, 1):
            g = (lambda T: (T, 5)) if axis == 0 else (lambda T: (5, T))
            for T in (16, 32):
                assert fwd(*g(T), e, axis) == L.AXF_ROUTE_EXACT_MFMA
                assert fwd(*g(T - 1), e, axis) == L.AXF_ROUTE_PADDED_MFMA
                assert fwd(*g(T + 1), e, axis) == L.AXF_ROUTE_PADDED_MFMA
                assert fwd(*g(T), e, axis, aligned=0) == L.AXF_ROUTE_THREAD_PER_ROW           # T * heads = 64, 128 | 256
                assert fwd(*g(T), e, axis, aligned=0, heads=3) == L.AXF_ROUTE_UNSUPPORTED
            assert fwd(*g(32), e, axis, aligned=0, heads=8) == L.AXF_ROUTE_THREAD_PER_ROW
            assert fwd(*g(32), e, axis, aligned=0, heads=16) == L.AXF_ROUTE_UNSUPPORTED
            assert fwd(*g(24), e, axis, aligned=0) == L.AXF_ROUTE_PADDED_MFMA               # (the call answers ACX_E_BADARG)
            assert fwd(*g(1), e, axis) == L.AXF_ROUTE_PADDED_MFMA
            assert fwd(*g(64), e, axis) == fwd(*g(65), e, axis) == fwd(*g(128), e, axis) == L.AXF_ROUTE_PADDED_MFMA
            assert fwd(*g(129), e, axis) == L.AXF_ROUTE_UNSUPPORTED
    for T in (16, 32, 77):
        assert fwd(T, 5, 64, 0) == L.AXF_ROUTE_PADDED_MFMA and fwd(1, T, 64, 1) == L.AXF_ROUTE_PADDED_MFMA
    assert fwd(16, 5, 64, 0, aligned=0) == L.AXF_ROUTE_PADDED_MFMA
    assert fwd(16, 5, 48, 0) == L.AXF_ROUTE_UNSUPPORTED and fwd(16, 5, 32, 0, heads=0) == L.AXF_ROUTE_UNSUPPORTED
    assert fwd(0, 5, 32, 1) == L.AXF_ROUTE_UNSUPPORTED and fwd(5, 0, 32, 0) == L.AXF_ROUTE_UNSUPPORTED


@pytest.mark.parametrize("c", ALL, ids=AR.case_id)
def test_table_tags_are_the_librarys_answers(c):
    assert AR.bwd_route(L.lib(), None, c) == AR.route_id(c.route)
    if c.route.startswith("text") and c.T > 128:
        assert AR.bwd_route(L.lib(), None, c, has_stats=0) == L.SAB_ROUTE_GENERIC
    if not c.causal and c.T <= 128:
        # the forward runs on these rows: the exact kernel exactly where the backward's is, the padded one everywhere else
        want = L.AXF_ROUTE_EXACT_MFMA if c.route == "axial_mfma" else L.AXF_ROUTE_PADDED_MFMA
        assert L.lib().acx_axial_attention_route(None, *AR.grid(c)[1:], c.heads, c.e, c.axis, 1) == want


def test_table_holds_what_the_sweep_promises():
    by = {r: [c for c in AR.CASES if c.route == r] for r in AR.ROUTES}
    plain = {r: [c for c in cs if not c.spike] for r, cs in by.items()}
    assert {c.T for c in plain["text_mfma"]} == {1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 77, 79, 80}
    assert {c.T for c in plain["text_block"]} == {81, 96, 100, 127, 128}
    assert {c.T for c in plain["text_rows"]} == {129, 191, 192, 193, 255, 256}
    for r in ("text_mfma", "text_block", "text_rows"):
        assert {(c.T, c.causal) for c in plain[r]} == {(c.T, z) for c in plain[r] for z in (0, 1)}
    assert {c.heads for c in plain["text_mfma"]} == {1, 3, 8}
    assert {(c.T, c.e, c.axis) for c in plain["axial_mfma"]} >= {(T, e, a) for T in (16, 32) for e in (16, 32) for a in (0, 1)}
    assert all((c.tiles * c.other * c.heads) % 4 for c in plain["axial_mfma"] if c.other != 86)
    pad = plain["axial_mfma_padded"]
    assert {c.T for c in pad} == {1, 2, 5, 15, 17, 31, 33, 47, 48, 49, 63, 64}
    assert {((c.T + 15) // 16, c.e) for c in pad} == {(tt, e) for tt in (1, 2, 3, 4) for e in (16, 32)}
    many = [c for c in AR.CASES if c.tiles * c.other * c.heads == AR.MANY_GROUPS]
    assert sorted(c.route for c in many) == ["axial_mfma", "axial_mfma_padded"] and AR.MANY_GROUPS > 8 * 256
    gen = plain["generic"]
    assert {(c.T, c.axis) for c in gen if c.e == 64 and c.other != 1} >= {(T, a) for T in (1, 3, 16, 32, 64, 65, 93, 94, 127, 128) for a in (0, 1)}
    assert {c.T for c in gen if c.e in (16, 32) and not c.causal} == {65, 85, 86, 96, 128, 129, 200, 256}
    assert {(c.T, c.e) for c in gen if c.causal and c.stats} == {(24, 32), (64, 16)}
    assert {(c.T, c.causal) for c in gen if not c.stats} == {(130, 0), (130, 1)}
    assert {(c.route, c.T) for c in AR.CASES if c.spike} == {("text_mfma", 77), ("text_block", 100), ("text_rows", 200), ("axial_mfma", 32),
                                                            ("axial_mfma_padded", 33), ("generic", 93)}
    assert [c.route for c in AR.GUARD_CASES] == list(AR.ROUTES)
    for c in AR.CASES + AR.GUARD_CASES:
        assert c.tiles in (2, 3) and c.tiles * c.T * c.other <= 4200, c
