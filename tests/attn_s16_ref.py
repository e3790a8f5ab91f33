"""Test infrastructure for acx_attention_s16 (csrc/acx_attn_s16.h), the streaming fp16 planes attention: the kernel's tiling constants,
the case constructor on clip_attn_ref's table type, and a CPU emulation of the CHUNKED arithmetic.

The arithmetic is clip_attn_ref's family "f16x3" (two fp16 planes per operand, products hi.hi, hi.lo, lo.hi, P split into an fp16 pair,
the output an fp16 pair): its bound, |err| <= 2e-6 * Sx, is derived there from the number formats alone and does not depend on L or on
how the keys are walked.  What streaming adds -- a running max m and sum per chunk of CHUNK keys, p = exp(s - m) split into an fp16
pair per chunk against the max SO FAR, the accumulator and the sum rescaled by exp(m_old - m) in f32 -- is emulated below;
tests/test_cpu_attn_s16.py holds it, like clip_attn_ref.emulate, below HALF the bound."""
import torch

import clip_attn_ref as CR

CHUNK = 64            # AS16_C: keys per chunk
QTILE = 32            # queries per wave
QBLOCK = 4 * QTILE    # AS16_NW tiles per query block (the tiles of a sequence are dealt evenly over ceil(tiles / 4) blocks)


def case(L, bh, spike=None, in_scale=1.0, out_scale=1.0, many=False):
    """a clip_attn_ref.FCase of the f16x3 family (entry "p3h16": scaled planes in, scaled planes out) at any L"""
    return CR.FCase("p3h16", None, L, bh[0], bh[1], 0, spike, "dense", 103, in_scale, out_scale, 0, many, 0)


def case_id(c):
    return CR.case_id(c).replace("p3h16", "s16")


def query_blocks(L):
    """the tiles of every query block of a sequence, as the kernel deals them"""
    nt = (L + QTILE - 1) // QTILE
    nqb = (nt + 3) // 4
    return [nt // nqb + (1 if qb < nt % nqb else 0) for qb in range(nqb)]


def emulate_chunked(c, qkv, chunk=CHUNK):
    """the streaming arithmetic on the CPU, [batch * L, heads * 64] fp64: the products of clip_attn_ref.emulate (fp64 sums of the
    retained plane products), the softmax chunk by chunk with the accumulator, the sum and the rescaling factor held in f32"""
    W, si = c.heads * CR.E, c.in_scale
    q, k, v = (CR._lines(qkv[:, i * W:(i + 1) * W].float(), c, c.batch) for i in range(3))

    def planes(x):
        return [p.double() for p in CR.split_f16(x)]
    qp, kp, vp = planes(q * si), planes(k * si), planes(v * si)
    s = sum(qp[a] @ kp[b].transpose(1, 2) for a, b in CR.PAIRS3) * (CR.SCALE / (si * si))
    m = torch.full(s.shape[:-1] + (1,), float("-inf"), dtype=torch.float64)
    l = torch.zeros_like(m)
    acc = torch.zeros(s.shape[:-1] + (CR.E,), dtype=torch.float64)
    for j0 in range(0, c.L, chunk):
        sc = s[..., j0:j0 + chunk]
        mnew = torch.maximum(m, sc.max(-1, keepdim=True).values)
        alpha = torch.exp(m - mnew).float().double()                       # exp(-inf) = 0 in front of the first chunk
        p = torch.exp(sc - mnew).float()
        pp = planes(p)
        pv = sum(pp[a] @ vp[b][:, j0:j0 + chunk] for a, b in CR.PAIRS3)
        acc = ((acc * alpha).float().double() + pv).float().double()
        l = (l * alpha + p.double().sum(-1, keepdim=True)).float().double()
        m = mnew
    o = acc / (l * si)
    return CR._unlines(CR._store(o, "f16x2", c.out_scale), c, c.batch)
