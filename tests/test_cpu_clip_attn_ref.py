"""No device: the reference of the CLIP attention forward sweep (tests/clip_attn_ref.py) and the library's route query.

  - acx_attention_route, through the C ABI, at every boundary of the dispatch rule and on every case of the table: the table's
    route tags are the library's own answers;
  - torch's fp32 CPU evaluation stays below 1e-6 * S on every f32 case, and the CPU emulation of each reduced arithmetic (bf16
    planes with six and with three products, fp16 planes, fp16-pair and plane outputs, bf16) below HALF its derived bound on every
    case of its family -- the condition that makes each bound one a correct implementation keeps, measured on the emulations and
    never on the kernels;
  - the table holds what it promises: every NT of both block kernels, every tile count 9 .. 16 of the streaming kernel, the query
    block splits, every length and form of the planes attention."""
import ctypes as C

import pytest
import torch

from anomalyclip_amd import _lib as L

import attn_ref as AR
import clip_attn_ref as CR

ALL = CR.CASES + CR.GUARD_CASES
UNSUPPORTED = -2
# the query tests its context against NULL and dereferences nothing (include/acx.h): any non-NULL address stands for a context here
_CTX_MEM = C.create_string_buffer(64)
CTX = C.addressof(_CTX_MEM)


def route(L_, causal=0, aligned=1, ctx=CTX):
    return L.lib().acx_attention_route(ctx, L_, causal, aligned)


def test_route_boundaries():
    B, S, Q = L.ATTN_ROUTE_BLOCK32, L.ATTN_ROUTE_STREAM16, L.ATTN_ROUTE_STREAM16_QB
    assert (B, S, Q) == (1, 2, 3)
    for ctx in (CTX, None):
        assert route(0, 0, 1, ctx) == route(-1, 1, 1, ctx) == UNSUPPORTED
        for causal in (0, 1):
            for aligned in (0, 1):
                assert route(1, causal, aligned, ctx) == route(128, causal, aligned, ctx) == B                # 128 | 129
        assert route(129, 0, 1, ctx) == route(224, 0, 1, ctx) == S
        for L_ in (129, 160, 197, 224):
            assert route(L_, 0, 0, ctx) == B and route(L_, 1, 1, ctx) == B and route(L_, 1, 0, ctx) == B      # misaligned, causal: 129 .. 224
        assert route(225, 1, 1, ctx) == route(225, 1, 0, ctx) == UNSUPPORTED                                   # 224 | 225 causal
        assert route(1025, 0, 1, ctx) == route(1025, 1, 1, ctx) == UNSUPPORTED                                 # 1024 | 1025
    assert route(225, 0, 1) == route(256, 0, 1) == S and route(257, 0, 1) == route(1024, 0, 1) == Q           # 256 | 257
    for L_ in (225, 256, 257, 577, 1024):
        assert route(L_, 0, 0) == UNSUPPORTED                                                                  # misaligned above 224
        assert route(L_, 0, 1, None) == route(L_, 0, 0, None) == UNSUPPORTED                                   # NULL context above 224


def test_null_context_call_keeps_its_answer():
    """acx_attention itself with a NULL context and host memory: refused before any launch above 224 (tests/test_cpu_host.py's contract)"""
    buf = (C.c_float * 64)()
    p = (C.addressof(buf) + 15) & ~15
    lib = L.lib()
    assert lib.acx_attention(None, p, 192, p, 64, 1, 500, 1, 0, None) == UNSUPPORTED
    assert b"context" in lib.acx_last_error(None)
    assert lib.acx_attention(None, p, 192, p, 64, 1, 1025, 1, 0, None) == UNSUPPORTED
    assert b"0 < L" in lib.acx_last_error(None)
    assert lib.acx_attention(None, p, 192, p, 64, 1, 64, 0, 0, None) == UNSUPPORTED                           # heads = 0


@pytest.mark.parametrize("c", [c for c in ALL if c.route], ids=CR.case_id)
def test_route_tags_are_the_librarys(c):
    assert route(c.L, c.causal, CR.out_aligned(c)) == CR.route_id(c.route)


def test_table_holds_what_it_promises():
    att = [c for c in CR.CASES if c.entry == "attention" and not c.spike and not c.many]

    def lengths(route_, causal, out=None):
        return sorted(c.L for c in att if c.route == route_ and c.causal == causal and (out is None or c.out == out))
    assert lengths("block32", 0, "dense") == list(CR.BLOCK_L) and lengths("block32", 1) == sorted(CR.BLOCK_L + CR.BLOCK_LONG_L)
    assert lengths("block32", 0, "offset4") == lengths("block32", 0, "ldo1") == list(CR.BLOCK_LONG_L)
    nt = lambda ls: {(L_ + 31) // 32 for L_ in ls}
    assert nt(lengths("block32", 1)) == set(range(1, 8)) and nt(CR.BLOCK_LONG_L) == {5, 6, 7} and nt(CR.BF16_L) == set(range(1, 8))
    assert lengths("stream16", 0) == list(CR.STREAM_L) and {(L_ + 15) // 16 for L_ in CR.STREAM_L} == set(range(9, 17))
    for t in range(9, 17):                                                 # both sides of every tile: 16 t - 15 (or 129), 16 t
        assert 16 * t in CR.STREAM_L and (16 * (t - 1) + 1) in CR.STREAM_L
    assert lengths("stream16_qb", 0) == list(CR.QB_L) and {257, 512, 513, 577, 1024} <= set(CR.QB_L)
    for c in CR.CASES:
        assert c.batch * c.heads % 4 or c.entry == "cls", CR.case_id(c)
        assert c.many or (c.batch in (2, 3) and c.heads in (1, 2, 3)) or c.entry == "cls", CR.case_id(c)
    assert {c.batch * c.heads for c in CR.CASES if c.entry == "cls"} == {3, 5, 8}
    assert sorted({c.L for c in CR.CASES if c.entry == "cls"}) == list(CR.CLS_L) and {c.out for c in CR.CASES if c.entry == "cls"} == {"dense", "ldo3"}
    many = [c for c in CR.CASES if c.many]
    assert [(c.entry, c.route, c.L) for c in many] == [("attention", "stream16", 129), ("attention", "stream16_qb", 257), ("p3n", None, 193)]
    forms = {(c.entry, c.products, c.in_scale, c.out_scale, c.ldpad) for c in CR.CASES}
    for L_ in CR.P3_L:
        assert {(c.entry, c.products, c.in_scale, c.out_scale, c.ldpad) for c in CR.CASES if c.L == L_ and c.entry.startswith("p3")} >= set(CR.P3_FORMS)
    assert set(CR.P3_FORMS) <= forms and CR.P3_L == tuple(range(193, 209))
    for e in ("x3", "x3_panel"):
        assert sorted(c.L for c in CR.CASES if c.entry == e) == list(CR.X3_L)
    spiked = {(CR.label(c), c.L, c.spike) for c in CR.CASES if c.spike}
    for sp in ("first", "last", "tile"):
        assert {("block32", 77, sp), ("block32_misaligned", 197, sp), ("stream16", 197, sp), ("stream16", 241, sp), ("stream16_qb", 577, sp)} <= spiked
        for lab in ("p3n6", "p3n3", "p3n103", "p3f", "p3f16", "p3h16"):
            assert (lab, 197, sp) in spiked
    guard = {CR.label(c) for c in CR.GUARD_CASES}
    assert guard >= {"block32", "block32_misaligned", "stream16", "stream16_qb", "x3_stream16", "x3_panel_stream16_qb", "bf16", "cls", "p3n6", "p3n3",
                     "p3n103", "p3f", "p3f16", "p3h16"}
    assert len({CR.case_id(c) for c in CR.CASES}) == len(CR.CASES)


def test_the_last_sequence_repeats_the_first():
    c = next(c for c in CR.CASES if c.batch == 3 and c.entry == "attention")
    qkv = CR.inputs(c)
    assert torch.equal(qkv[2 * c.L:], qkv[:c.L]) and not torch.equal(qkv[c.L:2 * c.L], qkv[:c.L])


@pytest.mark.parametrize("c", [c for c in ALL if CR.family(c) == "f32"], ids=CR.case_id)
def test_torch_fp32_stays_below_half_the_bound(c):
    qkv, o, Sx = CR.reference(c)
    AR.within(CR.emulate(c, qkv), o, Sx, CR.case_id(c), "torch_fp32", tol=0.5 * CR.TOL)


@pytest.mark.parametrize("c", [c for c in ALL if CR.family(c) != "f32"], ids=CR.case_id)
def test_emulation_stays_below_half_its_bound(c):
    qkv, o, Sx = CR.reference(c)
    AR.within(CR.emulate(c, qkv), o, Sx, CR.case_id(c), "emulated_" + CR.family(c), tol=0.5 * CR.TOL)


def test_bounds_grow_only_by_their_derived_terms():
    """Sx / S is the family's constant where the bound is purely relative, and at least it where absolute terms are added"""
    base = CR.FCase("attention", "stream16", 197, 2, 3, 0, None, "dense", 0, 1.0, 1.0, 0, False, 0)
    _, _, S = CR.reference(base)
    for entry, products, so, rel in (("x3", 0, 1.0, 2.0 ** -23), ("p3n", 6, 1.0, 2.0 ** -23), ("p3f", 6, 1.0, 2.0 ** -23), ("p3n", 3, 1.0, 2.0 ** -14)):
        _, _, Sx = CR.reference(base._replace(entry=entry, route=None, products=products, out_scale=so))
        assert torch.allclose(Sx, S * (1 + rel / CR.TOL), rtol=1e-12, atol=0)
    _, _, S16 = CR.reference(base._replace(entry="p3f16", route=None, products=6, out_scale=64.0))
    assert torch.allclose(S16, S * (1 + 2.0 ** -22 / CR.TOL) + 2.0 ** -30 / CR.TOL, rtol=1e-12, atol=0)
    _, _, Sh1 = CR.reference(base._replace(entry="p3h16", route=None, products=103))
    _, _, Sh64 = CR.reference(base._replace(entry="p3h16", route=None, products=103, in_scale=64.0, out_scale=16.0))
    assert bool((Sh1 > Sh64).all()) and bool((Sh64 > S * (1 + 2.0 ** -20 / CR.TOL)).all())
