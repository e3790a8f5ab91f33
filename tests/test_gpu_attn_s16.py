"""-m gpu: acx_attention_s16, the streaming fp16 planes attention, element by element against the fp64 closed form of attn_ref with the
bound of its arithmetic (clip_attn_ref's family "f16x3": 2e-6 * Sx, derived there from the number formats, held against the CPU
emulations of the one-pass and of the chunked softmax by tests/test_cpu_attn_s16.py, never fitted to the kernel).

The lengths sit on both sides of every boundary of the kernel's tiling: the 32-query tile, the 64-key chunk (a cut last chunk, a
chunk that holds one key) and the query block (a fourth, fifth, ... block; blocks of unequal size), beside the CLIP backbones' 50,
197, 257 and 577 and the ends 1 and 1024.  Spiked keys put the dominating key of every row into the first or the last chunk: every
partial sum before it is rescaled.  Every case runs twice and must be bit-identical; where batch > 2 the last sequence repeats the
first and must equal it bit for bit.  Beside the sweep: more items than the persistent grid has workgroups, the planes as slices of
NaN-filled buffers (a padded key that read on, or multiplied 0 * NaN, shows; sentinels around the output keep their bits), and the
refusals.  Every comparison prints its worst |err| / Sx before it asserts (pytest -s, the ATTN_RATIO lines)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

import attn_ref as AR
import attn_s16_ref as SR
import clip_attn_ref as CR

DEV = "cuda"
SENTINEL16 = 0x7FA5                         # a NaN's bit pattern the kernel does not produce
GUARD = 8
UNSUPPORTED, BADARG = -2, -1

ISSUE_L = (1, 15, 16, 17, 31, 32, 33, 50, 63, 64, 65, 127, 128, 129, 197, 208, 209, 255, 256, 257, 289, 511, 512, 513, 577, 1009, 1023, 1024)
# both sides of every multiple of the query tile (32): the multiples of the chunk (64) and of the query block (128) are among them
EDGE_L = tuple(sorted({x for k in range(1, 32) for x in (SR.QTILE * k, SR.QTILE * k + 1)} - set(ISSUE_L)))
SWEEP = [SR.case(L_, CR._shape(i)) for i, L_ in enumerate(ISSUE_L + EDGE_L)]
SPIKES = [SR.case(L_, (2, 3) if L_ < 577 else (2, 1), spike) for L_ in (50, 257, 577) for spike in ("first", "last", "tile")]
SCALED = [SR.case(L_, (3, 2), None, 64.0, 16.0) for L_ in (50, 257)]
MANY = SR.case(257, CR.MANY_QB, many=True)


def test_the_sweep_holds_what_it_promises():
    Ls = {c.L for c in SWEEP}
    assert set(ISSUE_L) <= Ls and (SR.CHUNK, SR.QTILE, SR.QBLOCK) == (64, 32, 128)
    for size in (SR.QTILE, SR.CHUNK, SR.QBLOCK):
        for edge in range(size, 1024, size):
            assert edge in Ls and edge + 1 in Ls, (size, edge)
    assert {len(SR.query_blocks(L_)) for L_ in Ls} == set(range(1, 9))
    assert any(len(set(SR.query_blocks(L_))) == 2 for L_ in Ls)            # blocks of unequal size


def _sentinel(shape):
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device=DEV).view(torch.float16)


def _is_sentinel(t):
    return bool((t.view(torch.int16) == SENTINEL16).all())


def _planes(c, qkv):
    return ops.split_f16x2(qkv.to(DEV), panel=True, scale=c.in_scale)


def _value(c, out):
    return ops.unpanel(out).double().sum(0) / c.out_scale


def _check(c):
    qkv, o, Sx = CR.reference(c)
    src = _planes(c, qkv)
    out = ops.attention_s16(src, c.batch, c.L, c.heads, c.in_scale, c.out_scale)
    out2 = ops.attention_s16(src, c.batch, c.L, c.heads, c.in_scale, c.out_scale)
    torch.cuda.synchronize()
    failures = []
    try:
        AR.within(_value(c, out), o, Sx, SR.case_id(c), "s16")
    except AssertionError as err:
        failures.append(str(err))
    if not torch.equal(out.view(torch.int16), out2.view(torch.int16)):
        failures.append("differs run to run")
    if c.batch > 2:
        rm = ops.unpanel(out).view(torch.int16)
        if not torch.equal(rm[:, -c.L:], rm[:, :c.L]):
            failures.append("the last sequence differs from the first, which it repeats")
    assert not failures, failures


@pytest.mark.parametrize("c", SWEEP, ids=SR.case_id)
def test_length_sweep_against_fp64(c):
    _check(c)


@pytest.mark.parametrize("c", SPIKES, ids=SR.case_id)
def test_spiked_keys(c):
    _check(c)


@pytest.mark.parametrize("c", SCALED, ids=SR.case_id)
def test_scaled_planes(c):
    _check(c)


def test_more_items_than_workgroups():
    c = MANY
    items = c.batch * c.heads * len(SR.query_blocks(c.L))
    assert items > 2 * torch.cuda.get_device_properties(0).multi_processor_count, items
    _check(c)


def test_repeated_sequences_are_bit_identical():
    c = SR.case(257, (3, 2))
    qkv, _, _ = CR.reference(c)
    assert torch.equal(qkv[-c.L:], qkv[:c.L])
    rm = ops.unpanel(ops.attention_s16(_planes(c, qkv), c.batch, c.L, c.heads)).view(torch.int16)
    assert torch.equal(rm[:, -c.L:], rm[:, :c.L]) and not torch.equal(rm[:, c.L:2 * c.L], rm[:, :c.L])


def test_a_second_call_gives_identical_bits():
    c = SR.case(577, (2, 3))
    src = _planes(c, CR.inputs(c))
    a = ops.attention_s16(src, c.batch, c.L, c.heads)
    b = ops.attention_s16(src, c.batch, c.L, c.heads)
    assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def _guarded_flat(x, nan):
    """a dense tensor (the planes of the operand or of the output) inside a flat buffer with GUARD rows of its last dimension on both
    sides: NaN around an input, the sentinel around (and under) an output"""
    pad = GUARD * x.shape[-1]
    big = torch.full((x.numel() + 2 * pad,), float("nan"), dtype=x.dtype, device=DEV) if nan else _sentinel((x.numel() + 2 * pad,))
    mid = big[pad:pad + x.numel()].view(x.shape)
    if nan:
        mid.copy_(x)
    assert mid.data_ptr() % 16 == 0
    return big, mid


@pytest.mark.parametrize("c", [SR.case(50, (2, 3)), SR.case(257, (2, 3))], ids=SR.case_id)
def test_stays_inside_its_problem(c):
    qkv, o, Sx = CR.reference(c)
    W, rows = c.heads * CR.E, c.batch * c.L
    _, src = _guarded_flat(_planes(c, qkv), True)
    big, out = _guarded_flat(torch.empty(2, rows, W, dtype=torch.float16), False)
    h = ops._h(src)
    assert L.lib().acx_attention_s16(h, src.data_ptr(), 1.0, out.data_ptr(), 1.0, c.batch, c.L, c.heads, ops._stream()) == 0
    torch.cuda.synchronize()
    after = big.clone()
    after[GUARD * W:GUARD * W + 2 * rows * W].view(torch.int16).fill_(SENTINEL16)
    assert _is_sentinel(after), "wrote outside its output"
    assert not bool((out.view(torch.int16) == SENTINEL16).any()), "left an output element unwritten"
    got = _value(c, out)
    assert bool(torch.isfinite(got).all())
    AR.within(got, o, Sx, SR.case_id(c) + " (guarded)", "s16_guarded")


def test_refusals():
    """none of these launches: the codes, the texts, and the output left alone"""
    lib = L.lib()
    src = torch.zeros(2 * 64 * 3 * 64 + 16, dtype=torch.float16, device=DEV)
    out = _sentinel((2 * 64 * 64 + 16,))
    h, s = ops._h(src), ops._stream()
    p, o = src.data_ptr(), out.data_ptr()

    def call(L_=50, batch=1, heads=1, si=1.0, so=1.0, src_=p, dst=o):
        return lib.acx_attention_s16(h, src_, si, dst, so, batch, L_, heads, s), lib.acx_last_error(h).decode()
    for kw, code, text in (({"L_": 0}, UNSUPPORTED, "1 <= L <= 1024"), ({"L_": 1025}, UNSUPPORTED, "1 <= L <= 1024"),
                           ({"batch": 0}, BADARG, "batch >= 1"), ({"heads": 0}, BADARG, "heads >= 1"),
                           ({"si": 3.0}, BADARG, "powers of two"), ({"so": 2.0 ** 21}, BADARG, "powers of two"),
                           ({"si": 2.0 ** -21}, BADARG, "powers of two"), ({"src_": p + 2}, BADARG, "16-byte aligned"),
                           ({"dst": o + 8}, BADARG, "16-byte aligned")):
        rc, err = call(**kw)
        assert rc == code and text in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert _is_sentinel(out)
    with pytest.raises(L.AcxError):
        ops.attention_s16(torch.zeros(2, 1025, 192, dtype=torch.float16, device=DEV), 1, 1025, 1)
