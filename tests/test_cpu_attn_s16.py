"""No device: the arithmetic of acx_attention_s16 (the streaming fp16 planes attention) against the bound it is judged by on the GPU.

clip_attn_ref derives the bound of the family "f16x3" (|err| <= 2e-6 * Sx) from the number formats alone; neither the bound nor
clip_attn_ref.emulate depends on L.  Here both clip_attn_ref.emulate (one softmax over all keys) and attn_s16_ref.emulate_chunked (the
running max and sum of the kernel, in chunks of the kernel's 64 keys and of 16 and 32) are held below HALF the bound at the lengths
of the CLIP backbones the kernel exists for (50, 257, 577), at 1, 33 and 1024, with one dominating key per row in the last chunk
("last", "tile": every earlier partial sum is rescaled) and in the first, and on scaled planes.  So the bound is not fitted to the
kernel and leaves it room.  The refusals of the C entry point come before any launch: they are asked here with a NULL context and
host memory."""
import ctypes as C

import pytest
import torch

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

import attn_ref as AR
import attn_s16_ref as SR
import clip_attn_ref as CR

ATTENTION_S16 = ops.attention_s16                      # (the wrapper exists)
UNSUPPORTED, BADARG = -2, -1

CASES = [SR.case(1, (2, 3)), SR.case(33, (2, 3)), SR.case(50, (2, 3)), SR.case(257, (3, 2)), SR.case(577, (2, 1)), SR.case(1024, (2, 1)),
         SR.case(50, (2, 3), "last"), SR.case(257, (2, 3), "last"), SR.case(577, (2, 1), "tile"), SR.case(577, (2, 1), "first"),
         SR.case(257, (3, 2), None, 64.0, 16.0)]


@pytest.mark.parametrize("c", CASES, ids=SR.case_id)
def test_emulations_keep_half_the_bound(c):
    assert CR.family(c) == "f16x3"
    qkv, o, Sx = CR.reference(c)
    AR.within(CR.emulate(c, qkv), o, Sx, SR.case_id(c), "s16_emulated", tol=0.5 * CR.TOL)
    for chunk in (SR.CHUNK, 32, 16):
        AR.within(SR.emulate_chunked(c, qkv, chunk), o, Sx, SR.case_id(c) + f" chunk {chunk}", "s16_emulated_chunked", tol=0.5 * CR.TOL)


def test_chunked_emulation_of_one_chunk_is_the_unchunked_one():
    """with every key in one chunk the running form is clip_attn_ref.emulate up to the f32 rounding of the accumulator"""
    c = SR.case(50, (2, 3))
    qkv, o, Sx = CR.reference(c)
    a, b = CR.emulate(c, qkv), SR.emulate_chunked(c, qkv, 64)
    assert float(((a - b).abs() / Sx).max()) < 0.1 * CR.TOL


def test_query_blocks():
    assert SR.query_blocks(50) == [2] and SR.query_blocks(128) == [4] and SR.query_blocks(129) == [3, 2]
    assert SR.query_blocks(257) == [3, 3, 3] and SR.query_blocks(577) == [4, 4, 4, 4, 3] and SR.query_blocks(1024) == [4] * 8
    for L_ in range(1, 1025):
        qb = SR.query_blocks(L_)
        assert sum(qb) == (L_ + 31) // 32 and max(qb) <= 4 and qb == sorted(qb, reverse=True) and max(qb) - min(qb) <= 1


def test_refusals_come_before_any_launch():
    lib = L.lib()
    buf = (C.c_uint16 * 4096)()
    p = (C.addressof(buf) + 15) & ~15

    def call(L_=50, batch=1, heads=1, si=1.0, so=1.0, src=p, dst=p):
        return lib.acx_attention_s16(None, src, si, dst, so, batch, L_, heads, None), lib.acx_last_error(None).decode()
    for L_ in (0, -1, 1025, 4096):
        rc, text = call(L_=L_)
        assert rc == UNSUPPORTED and "1 <= L <= 1024" in text
    for kw in ({"batch": 0}, {"batch": -3}, {"heads": 0}, {"heads": -1}):
        rc, text = call(**kw)
        assert rc == BADARG and "batch >= 1 and heads >= 1" in text, kw
    for kw in ({"si": 3.0}, {"so": 0.75}, {"si": 0.0}, {"so": -1.0}, {"si": 2.0 ** 21}, {"so": 2.0 ** -21}, {"si": float("nan")}, {"so": float("inf")}):
        rc, text = call(**kw)
        assert rc == BADARG and "powers of two" in text, kw
    for kw in ({"src": p + 2}, {"dst": p + 8}):
        rc, text = call(**kw)
        assert rc == BADARG and "16-byte aligned" in text, kw
    for kw in ({"src": None}, {"dst": None}):
        rc, text = call(**kw)
        assert rc == BADARG and "null pointer" in text, kw
