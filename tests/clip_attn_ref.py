"""Test infrastructure for the forward attention of the two CLIP towers (csrc/acx_attn.hip: acx_attention, _x3, _x3_panel, _p3n, _p3f,
_p3f16, _p3h16, _bf16, _cls): the case table of the route sweep (tests/test_gpu_clip_attn_routes.py), the bound of each arithmetic
and a CPU emulation of each reduced arithmetic (tests/test_cpu_clip_attn_ref.py holds the table's route tags against
acx_attention_route and torch's fp32 evaluation and every emulation against HALF their bounds).

The CLIP layout [batch * L, 3 * heads * 64] is attn_ref's (tiles = batch, gn = 1, gl = L, axis = 1, e = 64, scale = 0.125): the fp64
closed form, its term magnitude S (with R, the rounding of the scores, and F, the underflow floor), the seeded inputs (q times 3,
2^-4 .. 2^4 per sequence; or one spiked key per row) and the element-wise comparison are attn_ref's, unchanged.

THE BOUNDS.  Every family is judged as |err| <= TOL * Sx, TOL = 2e-6, element by element; Sx is S enlarged by
what the family's number formats lose on top of an fp32 evaluation, so that every recorded ratio |err| / Sx reads against the same
2e-6 (and the same 1e-6 for the CPU evaluations).  With u a relative error of every product term of both contractions, the scores
move by u A_ij, P_ij by the factor 1 + u R_ij and every term P_ij v_j by u again: the error is at most u sum_j P_ij (1 + R_ij) |v_j|
<= u S.  A relative error r of the stored output adds r |o| <= r S.  So a relative unit simply adds to TOL:

  f32        acx_attention, acx_attention_cls                       Sx = S
  x3         three bf16 planes of an f32 value (acx_attention_x3, _x3_panel, and p3n products = 6, p3f: six products keep every
             cross term down to 2^-27 of the term, inside TOL): three planes hold 24 bits, the residual of hi + mid + lo is at
             most 2^-23 |o|                                         Sx = S (1 + 2^-23 / TOL)
  p3n3       products = 3 on bf16 planes: the dropped products hi.lo, lo.hi and mid.mid are each at most 2^-16 of their term (a bf16
             plane keeps 8 bits: |mid| <= 2^-8 |hi|, |lo| <= 2^-16 |hi|, with room for the roundings' signs), u = 3 * 2^-16, in the score
             terms and in the P.V terms (P is split into hi + mid: its lo is the dropped hi.lo product); the output goes out as hi + mid
             only, residual 2^-16 |o| by the same count        Sx = S (1 + 4 * 2^-16 / TOL)
  p3f16      six products, output as the two fp16 planes of out_scale * o: fp16 keeps 11 bits, so hi + lo leaves 2^-22 |o| while lo is a
             normal number and, where lo is subnormal (spacing 2^-24), half of 2^-24 absolute in the scaled value.  That half spacing
             is not an estimate but the value a correct split REACHES (a scaled output just under 2^-24 plus half a step: hi rounds
             on the subnormal grid, lo cannot repair it), and an error a correct implementation reaches must sit at half the bound
             like every other: the first derivation, with 2^-25 / out_scale, had the emulation of the spiked L = 197 case at 1.4e-6
             of its Sx, 0.70 of the bound, on an output element of 2.9e-6 at out_scale = 1.  The absolute term is therefore the whole
             spacing                                                Sx = S (1 + 2^-22 / TOL) + 2^-24 / out_scale / TOL
  f16x3      products = 103 / acx_attention_p3h16: two fp16 planes per operand, products hi.hi, hi.lo, lo.hi.  Relative: the dropped lo.lo
             and the split residual of each of the two operands, 2^-22 of the term each, u = 3 * 2^-22.  Absolute: an operand element x
             arrives as in_scale * x on a grid of 2^-24 where its lo plane is subnormal, so x carries d = 2^-25 / in_scale whatever
             its size (why in_scale exists: at in_scale = 1 a sequence of 2^-4 * randn has every lo plane in the subnormals).  Through
             the sums: the score moves by E_ij = scale (d sum_c |q_ic| + d sum_c |k_jc| + 64 d^2), P_ij by the factor
             1 + E_ij + sum_j' P_ij' E_ij' (the derivation of R with E in the place of u A), v_j by d; the un-normalised
             p_ij = exp(s_ij - max_i) <= 1 is split into fp16 pairs as well and carries a_p = 2^-25, which the normaliser
             l_i = sum_j p_ij = 1 / max_j P_ij turns into a_p max_j P_ij per key:
                 X_i = sum_j P_ij (E_ij + sum_j' P_ij' E_ij') |v_j| + d + 2^-25 max_j P_ij sum_j (|v_j| + d)
             The output is an fp16 pair as in p3f16.      Sx = S (1 + 4 * 2^-22 / TOL) + (X + 2^-24 / out_scale) / TOL
             Stated for |in_scale * x| < 2^15 and |out_scale * o| < 2^15 (finite fp16 hi planes); inputs() asserts it.
  bf16       acx_attention_bf16: the reference is fp64 on the bf16-rounded inputs; products of bf16 numbers are exact in f32, P is
             rounded to bf16 for P.V and o to bf16 for the store, half an ulp = 2^-9 each     Sx = S (1 + 2^-8 / TOL)

None of these is fitted to a kernel.  Each reduced arithmetic has a CPU emulation below (operands split in torch with the kernels'
round-to-nearest conversions, the retained products, the softmax and the split of P evaluated in fp64, the output rounded as the
route stores it); test_cpu_clip_attn_ref.py holds every emulation, and torch's own fp32 evaluation for the f32 family, below HALF the
bound on every case of the table -- the rule attn_ref follows for fp32.  The worst ratios are in DESIGN.md section 3."""
import functools
from collections import namedtuple

import torch

import attn_ref as AR

TOL = AR.TOL
E, SCALE = 64, 0.125

# entry: the C entry point ("attention", "x3", "x3_panel", "p3n", "p3f", "p3f16", "p3h16", "bf16", "cls").  route: the tag of
# acx_attention_route's answer for attention / x3 / x3_panel, else None.  out: how the output buffer lies -- "dense", "offset4" (the
# base 4 bytes off a 16-byte boundary), "ldo1" (ldo = W + 1), "ldo3" (cls: ldo = W + 3).  products: p3n's.  ldpad: ldqkv - 3 W.
# qblocks: the query blocks per (sequence, head) the many-items case counts on (257 keys = 17 tiles = 9 + 8).
FCase = namedtuple("FCase", "entry route L batch heads causal spike out products in_scale out_scale ldpad many qblocks")
ROUTES = ("block32", "stream16", "stream16_qb")
MANY_STREAM = (173, 3)            # (batch, heads) of the many-items cases: 519 (sequence, head) items at L = 129,
MANY_QB = (87, 3)                 # 261 x 2 query blocks = 522 items at L = 257,
MANY_P3 = (171, 3)                # 513 items at L = 193 on a grid of one workgroup per CU: some workgroup walks three


def route_id(name):
    from anomalyclip_amd import _lib as L
    return getattr(L, "ATTN_ROUTE_" + name.upper())


def out_aligned(c):
    return int(c.out == "dense")


def family(c):
    """the arithmetic a case is judged by (the bounds of the module docstring)"""
    if c.entry in ("attention", "cls"):
        return "f32"
    if c.entry in ("x3", "x3_panel", "p3f") or (c.entry == "p3n" and c.products == 6):
        return "x3"
    if c.entry == "p3n":
        return "p3n3" if c.products == 3 else "f16x3"
    return {"p3f16": "p3f16", "p3h16": "f16x3", "bf16": "bf16"}[c.entry]


def label(c):
    """the tag the recorded ratios are grouped by: the route for acx_attention, the entry point and form for the others"""
    if c.entry == "attention":
        return c.route + ("" if c.out == "dense" else "_misaligned")
    if c.entry == "p3n":
        return f"p3n{c.products}"
    return c.entry + (f"_{c.route}" if c.route else "")


def case_id(c):
    s = f"{c.entry}-L{c.L}-b{c.batch}-h{c.heads}" + ("-causal" if c.causal else "") + (f"-{c.route}" if c.route else "")
    s += f"-p{c.products}" if c.entry == "p3n" else ""
    s += f"-in{c.in_scale:g}-out{c.out_scale:g}" if c.entry in ("p3f16", "p3h16") else ""
    s += (f"-{c.out}" if c.out != "dense" else "") + (f"-ldpad{c.ldpad}" if c.ldpad else "")
    return s + (f"-spike_{c.spike}" if c.spike else "") + ("-many" if c.many else "")


def _shape(i):
    """(batch, heads) number i: batch 2 or 3, heads in {1, 2, 3}, batch * heads no multiple of 4"""
    return ((2, 1), (3, 2), (2, 3), (3, 1), (3, 3))[i % 5]


BLOCK_L = (1, 2, 31, 32, 33, 63, 64, 65, 77, 95, 96, 97, 127, 128)
BLOCK_LONG_L = (129, 159, 160, 161, 191, 192, 193, 197, 223, 224)
STREAM_L = (129, 143, 144, 145, 159, 160, 161, 175, 176, 177, 191, 192, 193, 197, 207, 208, 209, 223, 224, 225, 239, 240, 241, 255, 256)
QB_L = (257, 272, 273, 289, 512, 513, 577, 768, 769, 1009, 1023, 1024)
X3_L = (129, 197, 256, 257, 577, 1024)
P3_L = tuple(range(193, 209))
BF16_L = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 160, 161, 192, 193, 197, 224)
CLS_L = (1, 63, 64, 65, 197, 255, 256, 257, 512, 513, 577, 1024)
# (entry, products, in_scale, out_scale, ldpad) of every form of the planes attention
P3_FORMS = (("p3n", 6, 1.0, 1.0, 0), ("p3n", 3, 1.0, 1.0, 0), ("p3n", 103, 1.0, 1.0, 0), ("p3f", 6, 1.0, 1.0, 0), ("p3f", 6, 1.0, 1.0, 64),
            ("p3f16", 6, 1.0, 1.0, 0), ("p3f16", 6, 1.0, 64.0, 0), ("p3h16", 103, 1.0, 1.0, 0), ("p3h16", 103, 64.0, 16.0, 0))


def _stream_route(L):
    return "stream16" if L <= 256 else "stream16_qb"


def _cases():
    out = []

    def add(entry, route, L, bh, causal=0, spike=None, lie="dense", products=0, in_scale=1.0, out_scale=1.0, ldpad=0, many=False, qblocks=0):
        out.append(FCase(entry, route, L, bh[0], bh[1], int(causal), spike, lie, products, in_scale, out_scale, ldpad, many, qblocks))

    for i, L in enumerate(BLOCK_L):                                       # both sides of every 32 boundary: NT = 1 .. 4
        for causal in (0, 1):
            add("attention", "block32", L, _shape(i + causal), causal)
    for i, L in enumerate(BLOCK_LONG_L):                                  # NT = 5 .. 7, eight waves: causal, and non-causal through an
        add("attention", "block32", L, _shape(i), 1)                      # output the streaming kernel cannot store to
        add("attention", "block32", L, _shape(i + 1), 0, lie="offset4")
        add("attention", "block32", L, _shape(i + 2), 0, lie="ldo1")
    for i, L in enumerate(STREAM_L):                                      # both sides of every 16-key tile and 32-key chunk: 9 .. 16 tiles
        add("attention", "stream16", L, _shape(i))
    for i, L in enumerate(QB_L):
        add("attention", "stream16_qb", L, _shape(i))
    add("attention", "stream16", 129, MANY_STREAM, many=True)             # more items than the grid has workgroups
    add("attention", "stream16_qb", 257, MANY_QB, many=True, qblocks=2)
    add("p3n", None, 193, MANY_P3, products=6, many=True)
    for spike in ("first", "last", "tile"):                               # one dominating key per query row
        add("attention", "block32", 77, (2, 3), 1, spike)
        add("attention", "block32", 197, (2, 3), 0, spike, lie="offset4")
        add("attention", "stream16", 197, (2, 3), 0, spike)
        add("attention", "stream16", 241, (3, 1), 0, spike)
        add("attention", "stream16_qb", 577, (2, 1), 0, spike)            # "last" / "tile": key 576, the last query block's last chunk
        for entry, products, si, so, ldpad in P3_FORMS:
            if not ldpad:
                add(entry, None, 197, (2, 3), 0, spike, products=products, in_scale=si, out_scale=so)
    for i, L in enumerate(X3_L):
        add("x3", _stream_route(L), L, _shape(i))
        add("x3_panel", _stream_route(L), L, _shape(i + 1))
    for i, L in enumerate(P3_L):
        for j, (entry, products, si, so, ldpad) in enumerate(P3_FORMS):
            add(entry, None, L, _shape(i + j), products=products, in_scale=si, out_scale=so, ldpad=ldpad)
    for i, L in enumerate(BF16_L):                                        # NT = 1 .. 7 of attn_bf16_kernel
        add("bf16", None, L, _shape(i))
    for i, L in enumerate(CLS_L):                                         # batch * heads in {3, 5, 8}: four per block, the last one partial
        add("cls", None, L, ((3, 1), (5, 1), (4, 2), (1, 3))[i % 4], lie=("dense", "ldo3")[i % 2])
    return out


CASES = _cases()
# the guard cases (the C ABI on slices of larger buffers): one per route and per form of the planes attention
GUARD_CASES = [FCase("attention", "block32", 77, 2, 3, 1, None, "dense", 0, 1.0, 1.0, 0, False, 0),
               FCase("attention", "block32", 197, 2, 3, 0, None, "ldo1", 0, 1.0, 1.0, 0, False, 0),
               FCase("attention", "stream16", 197, 2, 3, 0, None, "dense", 0, 1.0, 1.0, 0, False, 0),
               FCase("attention", "stream16_qb", 257, 2, 3, 0, None, "dense", 0, 1.0, 1.0, 0, False, 0),
               FCase("x3", "stream16", 197, 2, 3, 0, None, "dense", 0, 1.0, 1.0, 0, False, 0),
               FCase("x3_panel", "stream16_qb", 257, 2, 3, 0, None, "dense", 0, 1.0, 1.0, 0, False, 0),
               FCase("bf16", None, 197, 2, 3, 0, None, "dense", 0, 1.0, 1.0, 0, False, 0),
               FCase("cls", None, 257, 5, 1, 0, None, "dense", 0, 1.0, 1.0, 0, False, 0)] + \
              [FCase(e, None, 197, 2, 3, 0, None, "dense", p, si, so, 0, False, 0) for e, p, si, so, ldpad in P3_FORMS if not ldpad]


# ------------------------------------------------------------------------------------------------------------- inputs, reference
def _ar(c, batch=None):
    return AR.Case("-", c.L, 1, E, c.heads, 1, c.causal, c.batch if batch is None else batch, c.spike, True)


def inputs(c):
    """qkv [batch * L, 3 * heads * 64] f32: attn_ref.inputs of the shape; where batch > 2 the last sequence repeats the first; for
    acx_attention_bf16 rounded to bf16 (the reference is fp64 on what the kernel is given)"""
    qkv, _ = AR.inputs(_ar(c))
    if c.batch > 2:
        qkv[(c.batch - 1) * c.L:] = qkv[:c.L]
    if c.entry == "bf16":
        qkv = qkv.bfloat16().float()
    if family(c) in ("f16x3", "p3f16"):
        assert float(qkv.abs().max()) * c.in_scale < 2.0 ** 15
        assert float(qkv[:, 2 * c.heads * E:].abs().max()) * c.out_scale < 2.0 ** 15
    return qkv


def _lines(x, c, batch):
    return AR.to_lines(x.contiguous(), batch, 1, c.L, c.heads, E, 1)


def _unlines(y, c, batch):
    return AR.from_lines(y, batch, 1, c.L, c.heads, E, 1)


def _f16_terms(c, qkv, batch):
    """X of the module docstring, [batch * L, heads * 64] (the same for the 64 columns of a head)"""
    W = c.heads * E
    q, k, v = (_lines(qkv[:, i * W:(i + 1) * W].double(), c, batch) for i in range(3))
    d = 2.0 ** -25 / c.in_scale
    P = torch.softmax(SCALE * (q @ k.transpose(1, 2)), -1)
    Eij = SCALE * (d * q.abs().sum(-1, keepdim=True) + d * k.abs().sum(-1).unsqueeze(1) + E * d * d)
    RE = Eij + (P * Eij).sum(-1, keepdim=True)
    X = (P * RE) @ v.abs() + d + 2.0 ** -25 * P.max(-1, keepdim=True).values * (v.abs() + d).sum(1, keepdim=True)
    return _unlines(X, c, batch)


def _reference(c, qkv):
    """(o, Sx) in fp64, sequence chunks of at most 16 (the sequences are independent)"""
    W, fam = c.heads * E, family(c)
    rel = {"f32": 0.0, "x3": 2.0 ** -23, "p3n3": 4 * 2.0 ** -16, "p3f16": 2.0 ** -22, "f16x3": 4 * 2.0 ** -22, "bf16": 2.0 ** -8}[fam]
    os_, Ss = [], []
    for b0 in range(0, c.batch, 16):
        nb = min(16, c.batch - b0)
        x = qkv[b0 * c.L:(b0 + nb) * c.L]
        o, S = AR.attention(x, torch.zeros(nb * c.L, W), nb, 1, c.L, c.heads, E, 1, c.causal, SCALE)["o"]
        Sx = S * (1 + rel / TOL)
        if fam in ("p3f16", "f16x3"):
            Sx = Sx + 2.0 ** -24 / c.out_scale / TOL
        if fam == "f16x3":
            Sx = Sx + _f16_terms(c, x, nb) / TOL
        os_.append(o)
        Ss.append(Sx)
    return torch.cat(os_), torch.cat(Ss)


@functools.lru_cache(maxsize=2)
def _cached(key):
    c = key
    qkv = inputs(c)
    return (qkv,) + _reference(c, qkv)


def reference(c):
    """(qkv, o, Sx) of a case; cases that differ only in how the buffers lie share it (do not modify)"""
    fam = family(c)
    key = c._replace(route=None, out="dense", ldpad=0, many=False, qblocks=0,
                     entry={"f32": "attention", "x3": "x3", "bf16": "bf16"}.get(fam, c.entry),
                     products=c.products if fam in ("p3n3", "f16x3") else 0)
    qkv, o, Sx = _cached(key)
    if c.entry == "cls":
        rows = torch.arange(c.batch) * c.L
        return qkv, o[rows], Sx[rows]
    return qkv, o, Sx


# ------------------------------------------------------------------------------------------------------------- CPU evaluations
def torch_fp32(c, qkv):
    """torch's fp32 evaluation of softmax(q k^T / 8) v on the CPU"""
    W = c.heads * E
    q, k, v = (_lines(qkv[:, i * W:(i + 1) * W].float(), c, c.batch) for i in range(3))
    s = (q @ k.transpose(1, 2)) * SCALE
    if c.causal:
        s = s + torch.full((c.L, c.L), float("-inf")).triu_(1)
    return _unlines(torch.softmax(s, -1) @ v, c, c.batch)


def split_bf16(x, n):
    """the n leading bf16 planes of an f32 tensor, each as f32: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)"""
    planes, r = [], x.float()
    for _ in range(n):
        p = r.bfloat16().float()
        planes.append(p)
        r = r - p
    return planes


def split_f16(x):
    """the two fp16 planes of an f32 tensor, each as f32: hi = fp16(x), lo = fp16(x - hi) (subnormals kept)"""
    x = x.float()
    hi = x.half().float()
    return [hi, (x - hi).half().float()]


def _store(o, how, out_scale=1.0):
    """o (fp64) rounded to f32 and then as the route stores it, read back in fp64"""
    o32 = (o * out_scale).float()
    if how == "f32":
        return o32.double()
    if how == "bf16":
        return o32.bfloat16().double()
    planes = split_f16(o32) if how == "f16x2" else split_bf16(o32, 3 if how == "bf16x3" else 2)
    return sum(p.double() for p in planes) / out_scale


PAIRS6 = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))
PAIRS3 = ((0, 1), (1, 0), (0, 0))


def emulate(c, qkv):
    """the case's reduced arithmetic on the CPU, [batch * L, heads * 64] fp64 (cls: [batch, heads * 64]); sequence chunks of at most 16"""
    return torch.cat([_emulate(c._replace(batch=min(16, c.batch - b0)), qkv[b0 * c.L:(b0 + 16) * c.L]) for b0 in range(0, c.batch, 16)])


def _emulate(c, qkv):
    fam, W = family(c), c.heads * E
    if fam == "f32":
        o = torch_fp32(c, qkv)
        return o[torch.arange(c.batch) * c.L] if c.entry == "cls" else o
    if c.entry in ("x3", "x3_panel"):                                     # the f32 kernel, then the split
        return _store(torch_fp32(c, qkv).double(), "bf16x3")
    q, k, v = (_lines(qkv[:, i * W:(i + 1) * W].float(), c, c.batch) for i in range(3))
    if fam == "bf16":
        s = SCALE * (q.double() @ k.double().transpose(1, 2))
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        o = (p.float().bfloat16().double() @ v.double()) / p.sum(-1, keepdim=True)
        return _unlines(_store(o, "bf16"), c, c.batch)
    f16 = fam == "f16x3"
    six = fam in ("x3", "p3f16")
    si = c.in_scale if c.entry == "p3h16" else 1.0

    def planes(x):
        return [p.double() for p in (split_f16(x) if f16 else split_bf16(x, 3 if six else 2))]
    pairs = PAIRS6 if six else PAIRS3
    qp, kp, vp = planes(q * si), planes(k * si), planes(v * si)
    s = sum(qp[a] @ kp[b].transpose(1, 2) for a, b in pairs) * (SCALE / (si * si))
    p = torch.exp(s - s.max(-1, keepdim=True).values)
    pp = planes(p.float())                                                # un-normalised, split as it is consumed
    o = sum(pp[a] @ vp[b] for a, b in pairs) / (p.float().double().sum(-1, keepdim=True) * si)
    how = "f16x2" if (f16 or fam == "p3f16") else ("bf16x3" if six else "bf16x2")
    return _unlines(_store(o, how, c.out_scale), c, c.batch)
