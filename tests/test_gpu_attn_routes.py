"""-m gpu: acx_seq_attention_bwd on each of its six kernel routes and acx_axial_attention on each of its three, element by element
against the fp64 closed forms of attn_ref with the bound 2e-6 * S (S = the sum of the absolute values of the terms of the element,
with the derived term for the rounding of the scores), dq, dk and dv each on its own.  The case table (attn_ref.CASES) sits on both
sides of every length at which a kernel changes its tiling or the dispatcher its route; each row's tag is asserted against the
library's own route query, never restated here.  Per-line scales of 2^-4 .. 2^4 judge a small line on its own S.

Beside the table: spiked rows (one key 30 above the rest), calls on slices of larger buffers (sentinel rows around dqkv must keep
their bits, NaN rows around qkv / dout must not reach the result: a padded tile that read past its line turns 0 * NaN into NaN),
the forward's thread-per-row route through a view offset by 4 bytes, and the refusals.  Every comparison prints its worst
|err| / S before it asserts (pytest -s; DESIGN.md section 3 records them)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

import attn_ref as AR

DEV = "cuda"
SENTINEL = 0x7FA5A5A5                       # a NaN's bit pattern no kernel produces
GUARD = 8                                   # guard rows on each side of a slice (a multiple of 4 rows keeps the slice 16-byte aligned)


def _bwd_raw(c, qkv, dout, dqkv, stats):
    """acx_seq_attention_bwd through the C ABI on the given device tensors; stats None: no stats_ws"""
    h = ops._h(qkv)
    return L.lib().acx_seq_attention_bwd(h, qkv.data_ptr(), dout.data_ptr(), dqkv.data_ptr(), *AR.grid(c), c.heads, c.e, c.axis, c.causal,
                                         stats.data_ptr() if stats is not None else None, ops._stream())


def _bwd(c, qd, dd):
    if c.stats:
        return ops.seq_attention_bwd(qd, dd, *AR.grid(c), c.heads, c.e, c.axis, causal=bool(c.causal))
    dqkv = torch.empty_like(qd)
    assert _bwd_raw(c, qd, dd, dqkv, None) == 0
    return dqkv


def _check_bwd(c, got, ref, label=""):
    He = c.heads * c.e
    for i, name in enumerate(("dq", "dk", "dv")):
        AR.within(got[:, i * He:(i + 1) * He], *ref[name], f"{name} {AR.case_id(c)}{label}", c.route)


@pytest.mark.parametrize("c", AR.CASES, ids=AR.case_id)
def test_every_route_against_fp64(c):
    qkv, dout, ref = AR.reference(c)
    qd, dd = qkv.to(DEV), dout.to(DEV)
    h = ops._h(qd)
    assert AR.bwd_route(L.lib(), h, c) == AR.route_id(c.route)
    if c.tiles * c.other * c.heads == AR.MANY_GROUPS:
        assert AR.MANY_GROUPS > 8 * torch.cuda.get_device_properties(qd.device).multi_processor_count
    got = _bwd(c, qd, dd)
    again = _bwd(c, qd, dd)
    failures = []
    try:
        _check_bwd(c, got, ref)
    except AssertionError as err:
        failures.append(str(err))
    if not torch.equal(got, again):
        failures.append("backward differs run to run")
    if not c.causal and c.T <= 128:
        fwd_route = L.lib().acx_axial_attention_route(h, *AR.grid(c)[1:], c.heads, c.e, c.axis, 1)
        assert fwd_route in (L.AXF_ROUTE_PADDED_MFMA, L.AXF_ROUTE_EXACT_MFMA)
        assert (fwd_route == L.AXF_ROUTE_EXACT_MFMA) == (c.route == "axial_mfma")
        o = ops.axial_attention(qd, *AR.grid(c), c.heads, c.e, c.axis)
        try:
            AR.within(o, *ref["o"], f"o {AR.case_id(c)}", "fwd_exact_mfma" if fwd_route == L.AXF_ROUTE_EXACT_MFMA else "fwd_padded_mfma")
        except AssertionError as err:
            failures.append(str(err))
        if not torch.equal(o, ops.axial_attention(qd, *AR.grid(c), c.heads, c.e, c.axis)):
            failures.append("forward differs run to run")
    assert not failures, failures


def _guarded(x, fill_nan):
    """x's rows inside a larger device buffer: GUARD rows of NaN (inputs) or of the sentinel (outputs) on both sides"""
    rows, W = x.shape
    if fill_nan:
        big = torch.full((rows + 2 * GUARD, W), float("nan"), device=DEV)
    else:
        big = torch.full((rows + 2 * GUARD, W), SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    mid = big[GUARD:GUARD + rows]
    if fill_nan:
        mid.copy_(x)
    assert mid.is_contiguous() and mid.data_ptr() % 16 == 0
    return big, mid


def _guards_intact(big, rows):
    bits = big.view(torch.int32)
    return bool((bits[:GUARD] == SENTINEL).all()) and bool((bits[GUARD + rows:] == SENTINEL).all())


@pytest.mark.parametrize("c", AR.GUARD_CASES, ids=AR.case_id)
def test_routes_stay_inside_their_problem(c):
    """the C ABI on slices: the last group of the case ends with the slice"""
    qkv, dout, ref = AR.reference(c)
    rows = qkv.shape[0]
    _, qd = _guarded(qkv, True)
    _, dd = _guarded(dout, True)
    out_big, dqkv = _guarded(qkv, False)
    st_big, stats = _guarded(torch.empty(rows, c.heads * 3), False)
    assert AR.bwd_route(L.lib(), ops._h(qd), c) == AR.route_id(c.route)
    assert _bwd_raw(c, qd, dd, dqkv, stats) == 0
    torch.cuda.synchronize()
    assert _guards_intact(out_big, rows) and _guards_intact(st_big, rows)
    assert bool(torch.isfinite(dqkv).all())
    _check_bwd(c, dqkv, ref, " (guarded)")
    if not c.causal:
        o_big, o = _guarded(dout, False)
        assert L.lib().acx_axial_attention(ops._h(qd), qd.data_ptr(), o.data_ptr(), *AR.grid(c), c.heads, c.e, c.axis, ops._stream()) == 0
        torch.cuda.synchronize()
        assert _guards_intact(o_big, rows) and bool(torch.isfinite(o).all())
        AR.within(o, *ref["o"], f"o {AR.case_id(c)} (guarded)", "fwd_guarded")


@pytest.mark.parametrize("T,e,heads,axis", [(16, 32, 8, 0), (32, 16, 4, 1)])
def test_forward_thread_per_row_route(T, e, heads, axis):
    """a qkv view offset by 4 bytes takes the exact shapes to axial_attn_kernel (T * heads | 256)"""
    c = AR.Case("-", T, 5, e, heads, axis, 0, 3, None, True)
    qkv, dout, ref = AR.reference(c)
    flat = torch.empty(qkv.numel() + 4, device=DEV)
    view = flat[1:1 + qkv.numel()].view(qkv.shape)
    view.copy_(qkv)
    assert view.data_ptr() % 16 == 4
    h = ops._h(flat)
    assert L.lib().acx_axial_attention_route(h, *AR.grid(c)[1:], heads, e, axis, 0) == L.AXF_ROUTE_THREAD_PER_ROW
    outs = []
    for _ in range(2):
        o = torch.empty(qkv.shape[0], heads * e, device=DEV)
        assert L.lib().acx_axial_attention(h, view.data_ptr(), o.data_ptr(), *AR.grid(c), heads, e, axis, ops._stream()) == 0
        outs.append(o)
    AR.within(outs[0], *ref["o"], f"o T={T} e={e} heads={heads} axis={axis}", "fwd_thread_per_row")
    assert torch.equal(outs[0], outs[1])


def test_refusals():
    """none of these launches (the dispatchers answer from their route query before any launch): the codes, and outputs left alone"""
    lib = L.lib()
    buf = torch.zeros(300 * 3 * 3 * 64 * 2 + 4, device=DEV)
    out = torch.full((300 * 3 * 64 * 2 * 3,), SENTINEL, dtype=torch.int32, device=DEV)
    h, s = ops._h(buf), ops._stream()
    p, o = buf.data_ptr(), out.data_ptr()
    UNSUPPORTED, BADARG = -2, -1
    assert lib.acx_seq_attention_bwd(h, p, p, o, 2, 1, 257, 3, 64, 1, 1, p, s) == UNSUPPORTED          # T = 257 at the text shape
    assert lib.acx_seq_attention_bwd(h, p, p, o, 2, 16, 5, 3, 48, 0, 0, p, s) == UNSUPPORTED           # e = 48
    assert lib.acx_seq_attention_bwd(h, p, p, o, 2, 300, 1, 3, 32, 0, 0, p, s) == UNSUPPORTED          # T = 300 at e = 32
    assert lib.acx_axial_attention(h, p, o, 2, 129, 2, 3, 32, 0, s) == UNSUPPORTED                     # forward T = 129
    assert lib.acx_axial_attention(h, p, o, 2, 16, 5, 3, 48, 0, s) == UNSUPPORTED
    assert b"acx_axial_attention" in lib.acx_last_error(h)
    assert lib.acx_axial_attention(h, p + 4, o, 2, 24, 5, 4, 32, 0, s) == BADARG                       # misaligned off the exact shapes
    assert b"aligned" in lib.acx_last_error(h)
    assert lib.acx_axial_attention(h, p + 4, o, 2, 16, 5, 3, 32, 0, s) == UNSUPPORTED                  # misaligned, T * heads = 48
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
