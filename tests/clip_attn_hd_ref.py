"""Test infrastructure for the attention at head dimension 80 (csrc/acx_attn_hd.h: acx_attention_hd, _x3_hd, _cls_hd): the case table
of tests/test_gpu_h14.py and its fp64 reference (tests/test_cpu_h14.py holds the table's route tags against acx_attention_hd_route
and torch's fp32 evaluation against HALF the bound).

The layout [batch * L, 3 * heads * 80] is attn_ref's (tiles = batch, gn = 1, gl = L, axis = 1, e = 80, scale = 80 ** -0.5): the fp64
closed form, its term magnitude S, the seeded inputs (q times 3, 2^-4 .. 2^4 per sequence; or one spiked key per row) and the
element-wise comparison are attn_ref's, unchanged.  The bound is attn_ref.TOL * S = 2e-6 * S for the f32 rows and the CLS row, as
clip_attn_ref holds head dimension 64 to.  The scale is no power of two here: the kernels multiply q by the f32 rounding of
80 ** -0.5 (relative 2^-24 per score term, inside the u S of clip_attn_ref's derivation with u = 2^-24 << TOL).

THE LENGTHS.  The kernel tiles keys by 16, stages them in chunks of 32 and gives every wave one 16-query tile; a sequence of
ceil(L / 16) tiles is split into ceil(tiles / 8) query blocks.  One item per (sequence, head) up to 128 (route "stream"), several
above ("stream_qb").  STREAM_L sits on both sides of every tile count 1 .. 8's ends that matter (1, 15 | 16 | 17, 31 | 32 | 33,
64 | 65, 112 | 113: 7 | 8 tiles, 127 | 128); QB_L on both sides of every length at which the number of query blocks changes
(128 | 129, 256 | 257, 384 | 385, 512 | 513, 640 | 641, 768 | 769, 896 | 897) and at the ViT lengths 197, 257, 577, with 1023 | 1024
at the end.  Every case is batch 2, heads 3: width 240, the head offsets 0, 80, 160 start on both halves of a 32-column panel."""
import functools
from collections import namedtuple

import torch

import attn_ref as AR

TOL = AR.TOL
E, SCALE = 80, 80 ** -0.5

# entry: "hd" (f32 rows), "x3" (row-major planes), "x3_panel", "cls".  route: the tag of acx_attention_hd_route's answer (None: cls).
# many: more (query block, sequence, head) items than the kernel has workgroups; qblocks: its query blocks per (sequence, head).
HCase = namedtuple("HCase", "entry route L batch heads spike many qblocks")
ROUTES = ("stream", "stream_qb")
STREAM_L = (1, 15, 16, 17, 31, 32, 33, 64, 65, 112, 113, 127, 128)
QB_L = (129, 197, 256, 257, 384, 385, 512, 513, 577, 640, 641, 768, 769, 896, 897, 1023, 1024)
PLANE_L = (1, 17, 65, 128, 129, 257, 577)
CLS_L = (1, 63, 64, 65, 257, 577, 1024)
MANY = (40, 16)                   # (batch, heads) at L = 65: 640 items, above two workgroups on each of 256 CUs


def route_of(L):
    return "stream" if L <= 128 else "stream_qb"


def route_id(name):
    from anomalyclip_amd import _lib as L
    return getattr(L, "ATTN_HD_ROUTE_" + name.upper())


def qblocks(L):
    return ((L + 15) // 16 + 7) // 8


def case_id(c):
    return f"{c.entry}-L{c.L}-b{c.batch}-h{c.heads}" + (f"-{c.route}" if c.route else "") + (f"-spike_{c.spike}" if c.spike else "") + \
        ("-many" if c.many else "")


def _cases():
    out = [HCase("hd", route_of(L), L, 2, 3, None, False, 0) for L in STREAM_L + QB_L]
    out.append(HCase("hd", "stream", 65, MANY[0], MANY[1], None, True, 1))
    # one dominating key per query row: the last key (L = 577: the last chunk holds key 576 alone) and the first key of the last tile
    out += [HCase("hd", "stream_qb", 577, 2, 3, "last", False, 0), HCase("hd", "stream_qb", 1009, 2, 3, "tile", False, 0),
            HCase("hd", "stream", 113, 2, 3, "last", False, 0)]
    for heads in (3, 16):
        out += [HCase(e, route_of(L), L, 2, heads, None, False, 0) for e in ("x3", "x3_panel") for L in PLANE_L]
    out += [HCase("cls", None, L, 2, 3, None, False, 0) for L in CLS_L]
    return out


CASES = _cases()


def _ar(c):
    return AR.Case("-", c.L, 1, E, c.heads, 1, 0, c.batch, c.spike, True)


def inputs(c):
    """qkv [batch * L, 3 * heads * 80] f32 (attn_ref.inputs of the shape)"""
    return AR.inputs(_ar(c))[0]


@functools.lru_cache(maxsize=2)
def _cached(key):
    qkv = inputs(key)
    W = key.heads * E
    os_, Ss = [], []
    for b0 in range(0, key.batch, 8):                                    # the sequences are independent: chunks of at most 8
        nb = min(8, key.batch - b0)
        x = qkv[b0 * key.L:(b0 + nb) * key.L]
        o, S = AR.attention(x, torch.zeros(nb * key.L, W), nb, 1, key.L, key.heads, E, 1, 0, SCALE)["o"]
        os_.append(o)
        Ss.append(S)
    return qkv, torch.cat(os_), torch.cat(Ss)


def reference(c):
    """(qkv, o, S) of a case in fp64 (cls: the rows of token 0); cases that differ in the entry point only share it (do not modify)"""
    qkv, o, S = _cached(c._replace(entry="hd", route=None, many=False, qblocks=0))
    if c.entry == "cls":
        rows = torch.arange(c.batch) * c.L
        return qkv, o[rows], S[rows]
    return qkv, o, S


def torch_fp32(c, qkv):
    """torch's fp32 evaluation of softmax(q k^T / sqrt 80) v on the CPU, [batch * L, heads * 80]"""
    W = c.heads * E
    q, k, v = (AR.to_lines(qkv[:, i * W:(i + 1) * W].float().contiguous(), c.batch, 1, c.L, c.heads, E, 1) for i in range(3))
    o = torch.softmax((q @ k.transpose(1, 2)) * SCALE, -1) @ v
    return AR.from_lines(o, c.batch, 1, c.L, c.heads, E, 1)
