"""-m gpu: the forward attention of the two CLIP towers on every entry point and kernel route, element by element against the fp64
closed form of attn_ref with the bound of each arithmetic (clip_attn_ref: 2e-6 * Sx, Sx = S enlarged by what the route's number
formats lose; derived there, held against CPU emulations by tests/test_cpu_clip_attn_ref.py, never fitted to a kernel).  The case table
(clip_attn_ref.CASES) sits on both sides of every length at which a kernel changes its tiling or the dispatcher its route; each
acx_attention row's tag is asserted against acx_attention_route, never restated here.  q times 3 and per-sequence scales of
2^-4 .. 2^4 judge a peaked row and a small sequence on their own S.

Every case runs twice and must be bit-identical; where batch > 2 the last sequence repeats the first and must equal it bit for bit.
Beside the table: calls through the C ABI on slices of larger buffers (NaN rows around qkv and NaN columns behind its rows must not
reach the result -- a padded key tile that read on, or multiplied 0 * NaN, shows -- and sentinel rows / columns around the output must
keep their bits), and the refusals.  Every comparison prints its worst |err| / Sx before it asserts (pytest -s, the ATTN_RATIO
lines; DESIGN.md section 3 records them)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

import attn_ref as AR
import clip_attn_ref as CR

DEV = "cuda"
SENTINEL = 0x7FA5A5A5                       # a NaN's bit pattern no kernel produces
SENTINEL16 = 0x7FA5                         # ... as bf16 / fp16
GUARD = 8                                   # guard rows on each side of a slice (a multiple of 8 rows keeps every slice 16-byte aligned)
UNSUPPORTED, BADARG = -2, -1


def _sentinel(shape, dtype):
    """a device tensor of `dtype` (4 or 2 bytes per element) holding the sentinel's bits"""
    if dtype == torch.float32:
        return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device=DEV).view(dtype)


def _is_sentinel(t):
    if t.dtype == torch.float32:
        return bool((t.view(torch.int32) == SENTINEL).all())
    return bool((t.view(torch.int16) == SENTINEL16).all())


def _out_dtype(c):
    if c.entry in ("attention", "cls"):
        return torch.float32
    return torch.float16 if CR.family(c) in ("p3f16", "f16x3") else torch.bfloat16


def _out_planes(c):
    if c.entry in ("attention", "cls", "bf16"):
        return 0
    return 2 if CR.family(c) in ("p3f16", "f16x3") else 3


def _operand(c, qd):
    """what the entry point reads, made on the device from the f32 rows qd [rows, 3 W] (a dense tensor): the rows themselves, their
    bf16 rounding, or their planes in K-panel order; p3n with three products gets NaN lo planes (it must not read them)"""
    if c.entry == "bf16":
        return qd.bfloat16()
    if c.entry == "p3n" and c.products == 103:
        return ops.split_f16x2(qd, panel=True)
    if c.entry == "p3h16":
        return ops.split_f16x2(qd, panel=True, scale=c.in_scale)
    if c.entry == "p3n":
        planes = ops.split_bf16x3(qd, panel=True)
        if c.products == 3:
            planes[2] = float("nan")
        return planes
    return qd


def _call(c, src, ldqkv, out, ldo):
    """the entry point through the C ABI on device pointers; returns its code"""
    lib, h, s = L.lib(), ops._h(src), ops._stream()
    a = (c.batch, c.L, c.heads)
    if c.entry == "attention":
        return lib.acx_attention(h, src.data_ptr(), ldqkv, out.data_ptr(), ldo, *a, c.causal, s)
    if c.entry in ("x3", "x3_panel", "cls", "bf16"):
        return getattr(lib, "acx_attention_" + c.entry)(h, src.data_ptr(), ldqkv, out.data_ptr(), ldo, *a, s)
    if c.entry == "p3n":
        return lib.acx_attention_p3n(h, src.data_ptr(), out.data_ptr(), *a, c.products, s)
    if c.entry == "p3f":
        return lib.acx_attention_p3f(h, src.data_ptr(), ldqkv, out.data_ptr(), *a, s)
    if c.entry == "p3f16":
        return lib.acx_attention_p3f16(h, src.data_ptr(), ldqkv, out.data_ptr(), c.out_scale, *a, s)
    assert c.entry == "p3h16"
    return lib.acx_attention_p3h16(h, src.data_ptr(), c.in_scale, out.data_ptr(), c.out_scale, *a, s)


def _value(c, out, ldo):
    """the fp64 value [rows, W] of an output buffer: `out` is [rows, ldo] (row-major entry points), [planes, rows, ldo] (x3) or the
    dense planes in K-panel order"""
    W = c.heads * CR.E
    if c.entry in ("attention", "cls", "bf16"):
        return out[:, :W].double()
    if c.entry == "x3":
        return out[:, :, :W].double().sum(0)
    planes = ops.unpanel(out)
    if c.entry == "p3n" and c.products == 3:
        planes = planes[:2]                                                # (the lo plane is not written)
    return planes.double().sum(0) / c.out_scale


def _bits(t):
    return t.contiguous().view(torch.int32 if t.element_size() == 4 else torch.int16)


def _row_major(c, raw):
    """the raw output as [planes (or 1), rows, W]"""
    if _out_planes(c) == 0:
        return raw[:, :c.heads * CR.E].unsqueeze(0)
    return raw if c.entry == "x3" else ops.unpanel(raw)


def _out_rows(c):
    return c.batch if c.entry == "cls" else c.batch * c.L


def _run(c, src, ldqkv):
    """(value fp64 [rows, W], the raw output tensor) of one call on an output laid out as the case says"""
    W, rows, dt, npl = c.heads * CR.E, _out_rows(c), _out_dtype(c), _out_planes(c)
    edge = None
    if c.out == "offset4":
        flat = torch.empty(rows * W + 4, dtype=dt, device=DEV)
        out, ldo = flat[1:1 + rows * W].view(rows, W), W
        assert out.data_ptr() % 16 == 4
    elif c.out in ("ldo1", "ldo3"):
        ldo = W + int(c.out[3:])
        out = _sentinel((rows, ldo), dt)
        edge = out[:, W:]
    else:
        ldo = W
        out = torch.empty((npl, rows, W) if npl else (rows, W), dtype=dt, device=DEV)
        if c.entry == "p3n" and c.products == 3:
            out[2] = 0
    assert _call(c, src, ldqkv, out, ldo) == 0
    torch.cuda.synchronize()
    assert edge is None or _is_sentinel(edge), "wrote behind an output row"
    return _value(c, out, ldo), out


def _source(c, qkv):
    """(src, ldqkv): the operand on the device; ldpad: f32 rows inside a NaN-filled matrix of leading dimension 3 W + ldpad"""
    W3 = 3 * c.heads * CR.E
    qd = qkv.to(DEV)
    if c.ldpad:
        buf = torch.full((qd.shape[0], W3 + c.ldpad), float("nan"), device=DEV)
        buf[:, :W3] = qd
        return buf[:, :W3], W3 + c.ldpad
    return _operand(c, qd), W3


def _route(c, h):
    return L.lib().acx_attention_route(h, c.L, c.causal, CR.out_aligned(c))


@pytest.mark.parametrize("c", CR.CASES, ids=CR.case_id)
def test_every_route_against_fp64(c):
    qkv, o, Sx = CR.reference(c)
    src, ldqkv = _source(c, qkv)
    if c.route:
        assert _route(c, ops._h(src)) == CR.route_id(c.route)
    if c.many:
        items = c.batch * c.heads * max(c.qblocks, 1)
        assert items > 2 * torch.cuda.get_device_properties(src.device).multi_processor_count, items
    got, raw = _run(c, src, ldqkv)
    _, raw2 = _run(c, src, ldqkv)
    failures = []
    try:
        AR.within(got, o, Sx, CR.case_id(c), CR.label(c))
    except AssertionError as err:
        failures.append(str(err))
    if not torch.equal(_bits(raw), _bits(raw2)):
        failures.append("differs run to run")
    if c.batch > 2:
        n = 1 if c.entry == "cls" else c.L
        rm = _row_major(c, raw)
        if not torch.equal(_bits(rm[:, -n:]), _bits(rm[:, :n])):
            failures.append("the last sequence differs from the first, which it repeats")
    if c.entry in ("x3", "x3_panel"):                                     # the planes are the exact split of acx_attention's f32 output
        o32 = ops.attention(qkv.to(DEV), c.batch, c.L, c.heads, False)
        planes = raw if c.entry == "x3" else ops.unpanel(raw)
        r = o32
        for p in range(3):
            want = r.bfloat16()
            if not torch.equal(planes[p].view(torch.int16), want.view(torch.int16)):
                failures.append(f"plane {p} is not the split of acx_attention's output")
            r = r - want.float()
    assert not failures, failures


# ------------------------------------------------------------------------------------------------------------- slices of larger buffers
def _guarded_rows(x, ld, nan):
    """x [rows, w] inside a [rows + 2 GUARD, ld] buffer of NaN (inputs) or of the sentinel (outputs): (buffer, the [rows, ld] middle)"""
    rows = x.shape[0]
    big = torch.full((rows + 2 * GUARD, ld), float("nan"), dtype=x.dtype, device=DEV) if nan else _sentinel((rows + 2 * GUARD, ld), x.dtype)
    mid = big[GUARD:GUARD + rows]
    if nan:
        mid[:, :x.shape[1]] = x
    assert mid.data_ptr() % 16 == 0
    return big, mid


def _guarded_flat(x, nan):
    """a dense tensor (the planes of an operand or of an output) inside a flat buffer with GUARD rows of its last dimension on both
    sides.  The plane stride is fixed by the ABI (rows * width), so the guards lie in front of the first and behind the last plane."""
    pad = GUARD * x.shape[-1]
    big = torch.full((x.numel() + 2 * pad,), float("nan"), dtype=x.dtype, device=DEV) if nan else _sentinel((x.numel() + 2 * pad,), x.dtype)
    mid = big[pad:pad + x.numel()].view(x.shape)
    if nan:
        mid.copy_(x)
    assert mid.data_ptr() % 16 == 0
    return big, mid


@pytest.mark.parametrize("c", CR.GUARD_CASES, ids=CR.case_id)
def test_routes_stay_inside_their_problem(c):
    """the C ABI on slices: the last sequence of the case ends with the slice; ldqkv = 3 W + 4 (bf16: + 8) and ldo = W + 4 (the
    misaligned block32 case: W + 1) where the entry point takes a leading dimension"""
    qkv, o, Sx = CR.reference(c)
    W, rows, dt, npl = c.heads * CR.E, _out_rows(c), _out_dtype(c), _out_planes(c)
    operand = _operand(c, qkv.to(DEV))
    if operand.dim() == 2:                                                # rows with a leading dimension
        ldqkv = 3 * W + (8 if c.entry == "bf16" else 4)
        _, src = _guarded_rows(operand, ldqkv, True)
    else:
        ldqkv = 0
        _, src = _guarded_flat(operand, True)
    if c.route:
        assert _route(c, ops._h(src)) == CR.route_id(c.route)
    if npl == 0:                                                          # [rows, ldo]
        ldo = W + (1 if c.out == "ldo1" else 4)
        big, out = _guarded_rows(torch.empty(rows, W, dtype=dt), ldo, False)
        inside = lambda b: b[GUARD:GUARD + rows, :W]
    elif c.entry == "x3":                                                 # [3, rows, ldo], plane stride rows * ldo
        ldo = W + 4
        big, out = _guarded_flat(torch.empty(3, rows, ldo, dtype=dt), False)
        inside = lambda b: b[GUARD * ldo:GUARD * ldo + 3 * rows * ldo].view(3, rows, ldo)[:, :, :W]
    else:                                                                 # dense planes in K-panel order
        ldo = W
        big, out = _guarded_flat(torch.empty(npl, rows, W, dtype=dt), False)
        written = npl - 1 if (c.entry == "p3n" and c.products == 3) else npl
        inside = lambda b: b[GUARD * W:GUARD * W + written * rows * W]
    assert _call(c, src, ldqkv, out, ldo) == 0
    torch.cuda.synchronize()
    after = big.clone()
    inside(after).view(torch.int32 if dt == torch.float32 else torch.int16).fill_(SENTINEL if dt == torch.float32 else SENTINEL16)
    assert _is_sentinel(after), "wrote outside its output"
    if c.entry == "p3n" and c.products == 3:
        out[2] = 0
    got = _value(c, out, ldo)
    assert bool(torch.isfinite(got).all())
    AR.within(got, o, Sx, CR.case_id(c) + " (guarded)", CR.label(c) + "_guarded")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    """none of these launches: the codes (acx_attention's are the route query's own negative answers), and the outputs left alone"""
    lib = L.lib()
    W = 64
    qkv = torch.zeros(1025 * 3 * W + 4, device=DEV)
    planes = torch.zeros(3 * 1025 * 3 * W, dtype=torch.bfloat16, device=DEV)
    out = _sentinel((3 * 1025 * W + 4,), torch.float32)
    h, s = ops._h(qkv), ops._stream()
    p, pp, o = qkv.data_ptr(), planes.data_ptr(), out.data_ptr()
    for L_, causal, off in ((225, 1, 0), (1025, 0, 0), (1025, 1, 0), (0, 0, 0), (225, 0, 4), (257, 0, 4), (1024, 0, 4)):
        want = lib.acx_attention_route(h, L_, causal, int(off == 0))
        assert want == UNSUPPORTED
        assert lib.acx_attention(h, p, 3 * W, o + off, W, 1, L_, 1, causal, s) == want, (L_, causal, off)
    assert lib.acx_attention(h, p, 3 * W, o, W + 1, 1, 225, 1, 0, s) == lib.acx_attention_route(h, 225, 0, 0) == UNSUPPORTED   # ldo % 4
    assert lib.acx_attention(h, p + 4, 3 * W, o, W, 1, 197, 1, 0, s) == BADARG                                               # qkv misaligned
    for fn in (lib.acx_attention_x3, lib.acx_attention_x3_panel):
        assert lib.acx_attention_route(h, 128, 0, 1) == L.ATTN_ROUTE_BLOCK32 and lib.acx_attention_route(h, 197, 0, 0) == L.ATTN_ROUTE_BLOCK32
        assert fn(h, p, 3 * W, o, W, 1, 128, 1, s) == UNSUPPORTED                                                            # below 129
        assert fn(h, p, 3 * W, o + 4, W, 1, 197, 1, s) == UNSUPPORTED                                                        # misaligned out
        assert fn(h, p, 3 * W, o + 4, W, 1, 577, 1, s) == UNSUPPORTED
    assert lib.acx_attention_x3_panel(h, p, 3 * W, o, W + 4, 1, 197, 1, s) == BADARG                                          # dense planes only
    for L_ in (192, 209):
        for products in (6, 3, 103):
            assert lib.acx_attention_p3n(h, pp, o, 1, L_, 1, products, s) == UNSUPPORTED, (L_, products)
        assert lib.acx_attention_p3(h, pp, o, 1, L_, 1, s) == UNSUPPORTED
        assert lib.acx_attention_p3f(h, p, 3 * W, o, 1, L_, 1, s) == UNSUPPORTED
        assert lib.acx_attention_p3f16(h, p, 3 * W, o, 1.0, 1, L_, 1, s) == UNSUPPORTED
        assert lib.acx_attention_p3h16(h, pp, 1.0, o, 1.0, 1, L_, 1, s) == UNSUPPORTED
    assert lib.acx_attention_p3n(h, pp, o, 1, 197, 1, 4, s) == BADARG
    assert lib.acx_attention_p3f(h, p, 3 * W + 2, o, 1, 197, 1, s) == UNSUPPORTED                                             # ldqkv % 4
    assert lib.acx_attention_p3f(h, p, 3 * W - 4, o, 1, 197, 1, s) == UNSUPPORTED                                             # ldqkv < 3 W
    assert lib.acx_attention_bf16(h, pp, 3 * W, o, W, 1, 225, 1, s) == UNSUPPORTED
    assert lib.acx_attention_cls(h, p, 3 * W, o, W, 1, 1025, 1, s) == UNSUPPORTED
    torch.cuda.synchronize()
    assert _is_sentinel(out)
