"""Test infrastructure for the axial / sequence attention forward (acx_axial_attention) and backward (acx_seq_attention_bwd):
the closed forms in fp64, each with the term magnitude S its error is judged against, the case table of the route sweep
(tests/test_gpu_attn_routes.py; tests/test_cpu_attn_ref.py holds the table's tags against the library's route queries and
the forms of S against torch's fp32 evaluation) and the seeded inputs.

The tolerance is the project's fp32 bound, element by element:  |err| <= TOL * S  with TOL = 2e-6, S = the sum
of the absolute values of the terms the element is made of.  With s_ij = scale q_i . k_j over the keys j the query i may see (all of
them, or j <= i when causal), P = softmax_j(s), dP_ij = dO_i . v_j, D_i = sum_j P_ij dP_ij, dS_ij = P_ij (dP_ij - D_i):

    o_i  = sum_j P_ij v_j                  S = sum_j W_ij |v_j|
    dv_j = sum_i P_ij dO_i                 S = sum_i W_ij |dO_i|
    dq_i = scale sum_j dS_ij k_j           S = scale sum_j M_ij |k_j|
    dk_j = scale sum_i dS_ij q_i           S = scale sum_i M_ij |q_i|

    A_ij  = scale sum_c |q_ic k_jc|                         the terms of the score s_ij
    R_ij  = A_ij + sum_j' P_ij' A_ij'                       the relative error of P_ij per unit of relative rounding of the scores
    W_ij  = P_ij (1 + R_ij) + F                             |P_ij| with its own rounding
    aP_ij = sum_c |dO_ic v_jc|                              the terms of dP_ij
    aD_i  = sum_j W_ij aP_ij                                the terms of D_i
    M_ij  = W_ij (aP_ij + aD_i) + F                         the terms of dS_ij: |dP| and |D| counted one by one, never |dP - D|
    F     = 2^-106 on the pairs the query may see           fp32 underflow, below

R is derived, not fitted: a score computed in fp32 is s_ij (1 + d_ij) with |s_ij d_ij| <= u A_ij (u: a few units of 2^-24, the
rounding of the products and of their sum); P_ij = exp(s_ij) / sum_j' exp(s_ij') then moves by the factor
exp(s_ij d_ij - sum_j' P_ij' s_ij' d_ij') to first order, which is at most 1 + u (A_ij + sum_j' P_ij' A_ij').  The subtraction of
the row maximum and the exponential's argument reduction round relative to |s_ij - max|, which the same two terms bound.  Without
R, a row whose q and k are large (scores of several hundred, a softmax that is one-hot up to near-ties) cannot be met by ANY fp32
evaluation: the near-tie's two P move by u A, far above 2^-24 of themselves.

F is the other derived term.  An exponential below 2^-126 is a denormal in fp32 -- flushed to zero on the GPU, kept with an
absolute spacing of 2^-149 on the CPU -- so a P_ij that small carries an ABSOLUTE error of up to 2^-126, whatever its size, and
so does the product dS_ij.  Where every pair of an element is that small (the gradient of a key no query attends to: dv and dk
of the second key of a causal T = 2 line with scores a few hundred apart), 2^-24 of the terms is not a bound any fp32 evaluation
keeps.  S therefore counts P_ij and dS_ij as at least F = 2^-106 >= 2^-126 / 1e-6: TOL * F covers the flush.  F is 1e-32: it moves
no S that holds an ordinary term.

A masked pair has P = 0 exactly and adds nothing to any S, F included; where S is 0 the value must be exactly 0.

torch's own fp32 CPU evaluation of the expression (autograd for the gradients) stays below HALF the bound, 1e-6 * S, on every
case of the table: test_cpu_attn_ref.py asserts it, the worst ratios it has seen are in DESIGN.md section 3 beside the kernels'.
The bound is never set from the kernels' ratios."""
from collections import namedtuple

import torch

TOL = 2e-6
UNDERFLOW = 2.0 ** -106      # 2^-126 / 1e-6 rounded up to a power of two: what S counts an unmasked P_ij and dS_ij as at least


# ------------------------------------------------------------------------------------------------------------- layout
def _geom(tiles, gn, gl, axis):
    """(T, other): the sequence length along the axis and the number of lines per tile"""
    return (gn, gl) if axis == 0 else (gl, gn)


def to_lines(x, tiles, gn, gl, heads, e, axis):
    """[tiles * gn * gl, heads * e] -> [tiles * other * heads, T, e]: one (line, head) group per batch entry, line-major"""
    x = x.view(tiles, gn, gl, heads, e)
    x = x.permute(0, 2, 3, 1, 4) if axis == 0 else x.permute(0, 1, 3, 2, 4)
    return x.reshape(-1, x.shape[3], e)


def from_lines(y, tiles, gn, gl, heads, e, axis):
    """the inverse of to_lines"""
    T, other = _geom(tiles, gn, gl, axis)
    y = y.view(tiles, other, heads, T, e)
    y = y.permute(0, 3, 1, 2, 4) if axis == 0 else y.permute(0, 1, 3, 2, 4)
    return y.reshape(tiles * gn * gl, heads * e)


def _split(qkv, dout, tiles, gn, gl, heads, e, axis, dtype):
    He = heads * e
    qkv, dout = qkv.to(dtype), dout.to(dtype)
    a = (tiles, gn, gl, heads, e, axis)
    return tuple(to_lines(t.contiguous(), *a) for t in (qkv[:, :He], qkv[:, He:2 * He], qkv[:, 2 * He:], dout))


# ------------------------------------------------------------------------------------------------------------- closed forms
def attention(qkv, dout, tiles, gn, gl, heads, e, axis, causal, scale):
    """{"o", "dq", "dk", "dv"} -> (value, S), each [tiles * gn * gl, heads * e] in fp64: the forward output and the gradients of
    sum(o * dout) with respect to q, k and v, in the closed forms of the module docstring"""
    a = (tiles, gn, gl, heads, e, axis)
    q, k, v, dO = _split(qkv, dout, *a, torch.float64)
    T = q.shape[1]
    s = scale * (q @ k.transpose(1, 2))
    A = scale * (q.abs() @ k.abs().transpose(1, 2))
    if causal:
        s = s.masked_fill(torch.ones(T, T, dtype=torch.bool).triu_(1), float("-inf"))
    P = torch.softmax(s, -1)                                              # a masked pair: exactly 0
    floor = torch.full_like(P, UNDERFLOW)
    if causal:
        floor = floor.masked_fill(torch.ones(T, T, dtype=torch.bool).triu_(1), 0.0)
    W = P * (1 + A + (P * A).sum(-1, keepdim=True)) + floor
    dP = dO @ v.transpose(1, 2)
    aP = dO.abs() @ v.abs().transpose(1, 2)
    dS = P * (dP - (P * dP).sum(-1, keepdim=True))
    M = W * (aP + (W * aP).sum(-1, keepdim=True)) + floor
    out = {"o": (P @ v, W @ v.abs()),
           "dq": (scale * (dS @ k), scale * (M @ k.abs())),
           "dk": (scale * (dS.transpose(1, 2) @ q), scale * (M.transpose(1, 2) @ q.abs())),
           "dv": (P.transpose(1, 2) @ dO, W.transpose(1, 2) @ dO.abs())}
    return {n: (from_lines(val, *a), from_lines(S, *a)) for n, (val, S) in out.items()}


def autograd(qkv, dout, tiles, gn, gl, heads, e, axis, causal, scale, dtype):
    """{"o", "dq", "dk", "dv"}: torch's own evaluation of softmax(scale q k^T) v in `dtype` on the CPU and its autograd"""
    a = (tiles, gn, gl, heads, e, axis)
    He = heads * e
    with torch.enable_grad():
        t = qkv.to(dtype).clone().requires_grad_(True)
        q, k, v = (to_lines(t[:, i * He:(i + 1) * He], *a) for i in range(3))
        s = (q @ k.transpose(1, 2)) * scale
        if causal:
            T = s.shape[-1]
            s = s + torch.full((T, T), float("-inf"), dtype=dtype).triu_(1)
        o = from_lines(torch.softmax(s, -1) @ v, *a)
        o.backward(dout.to(dtype))
    g = t.grad
    return {"o": o.detach(), "dq": g[:, :He], "dk": g[:, He:2 * He], "dv": g[:, 2 * He:]}


# ------------------------------------------------------------------------------------------------------------- comparison
def ratio(got, ref, S):
    """worst |got - ref| / S over the elements with S > 0 (an element with S == 0 must be exact: inf otherwise; so is a non-finite one)"""
    got = torch.as_tensor(got).detach().double().cpu()
    err = (got - ref.double()).abs()
    S = S.double().expand_as(err)
    inf = torch.full_like(err, float("inf"))
    r = torch.where(S > 0, err / S.clamp_min(1e-300), torch.where(err > 0, inf, torch.zeros_like(err)))
    r = torch.where(torch.isfinite(got), r, inf)
    return float(r.max()) if r.numel() else 0.0


def within(got, ref, S, label, family, tol=TOL):
    """asserts |got - ref| <= tol * S element by element; prints the worst ratio first (family: the tag the recorded ratios are
    grouped by, the route for the kernels)"""
    r = ratio(got, ref, S)
    print(f"ATTN_RATIO {family} {label} {r:.3e}")
    assert r <= tol, f"{family} {label}: worst |err| / S = {r:.3e} > {tol:.1e}"
    return r


# ------------------------------------------------------------------------------------------------------------- the case table
# route: the backward route's tag (route_id maps it to the library's enum;test_cpu_attn_ref.py holds every tag against
# acx_seq_attention_bwd_route).  The grid is (tiles, T, other) for axis 0 and (tiles, other, T) for axis 1.  spike: None, or where the
# dominating key sits ("first", "last", "tile": the first key of the last 16-key tile).  stats: the call brings stats_ws.
Case = namedtuple("Case", "route T other e heads axis causal tiles spike stats")
ROUTES = ("text_mfma", "text_block", "text_rows", "axial_mfma", "axial_mfma_padded", "generic")
MANY_GROUPS = 3 * 86 * 8          # the two many-groups cases: above 8 x 256 CUs, so every wave of the capped grid walks >= 2 groups


def route_id(name):
    """the library's enum value of a route tag (anomalyclip_amd._lib SAB_ROUTE_*)"""
    from anomalyclip_amd import _lib as L
    return getattr(L, "SAB_ROUTE_" + name.upper())


def bwd_route(lib, ctx, c, has_stats=None):
    """acx_seq_attention_bwd_route's answer for a case"""
    return lib.acx_seq_attention_bwd_route(ctx, *grid(c), c.heads, c.e, c.axis, c.causal, int(c.stats if has_stats is None else has_stats))


def case_id(c):
    return (f"{c.route}-T{c.T}-o{c.other}-e{c.e}-h{c.heads}-ax{c.axis}-{'causal' if c.causal else 'full'}-t{c.tiles}"
            + (f"-spike_{c.spike}" if c.spike else "") + ("" if c.stats else "-nostats"))


def grid(c):
    """(tiles, gn, gl) of a case"""
    return (c.tiles, c.T, c.other) if c.axis == 0 else (c.tiles, c.other, c.T)


def _cases():
    out = []

    def add(route, T, other, e, heads, axis, causal, tiles, spike=None, stats=True):
        out.append(Case(route, T, other, e, heads, axis, int(causal), tiles, spike, stats))

    # text tower shape (gn = 1, axis 1, e = 64).  MFMA kernel: the 16-key tile boundaries of its padding to 80
    for i, T in enumerate((1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 77, 79, 80)):
        for causal in (0, 1):
            add("text_mfma", T, 1, 64, (1, 3, 8)[(i + causal) % 3], 1, causal, 2 + i % 2)
    for i, T in enumerate((81, 96, 100, 127, 128)):
        for causal in (0, 1):
            add("text_block", T, 1, 64, (1, 3, 8)[(i + causal) % 3], 1, causal, 2 + i % 2)
    for i, T in enumerate((129, 191, 192, 193, 255, 256)):                # the 64-key lane boundaries of KPL = 4
        for causal in (0, 1):
            add("text_rows", T, 1, 64, (1, 3, 8)[(i + causal) % 3], 1, causal, 2)
    # axial MFMA, exact: group counts 3, 15, 9, 45 -- no multiple of the 4 waves of a workgroup
    i = 0
    for T in (16, 32):
        for e in (16, 32):
            for axis in (0, 1):
                add("axial_mfma", T, (1, 5)[i % 2], e, (1, 3)[(i // 2) % 2], axis, 0, 3)
                i += 1
    # axial MFMA, padded: both sides of every 16 boundary; each e meets each padded size 16, 32, 48, 64
    for i, T in enumerate((1, 2, 15, 17, 31, 33, 47, 48, 49, 63, 64)):
        add("axial_mfma_padded", T, (1, 5)[i % 2], (16, 32)[i % 2], (1, 3)[(i // 2) % 2], (i // 2) % 2, 0, 3)
    # more groups than the grid cap has waves: a wave re-stages its LDS slice for a second group
    add("axial_mfma_padded", 5, 86, 16, 8, 0, 0, 3)
    add("axial_mfma", 16, 86, 32, 8, 1, 0, 3)
    # generic kernel, e = 64 on a grid.  groups per block gpb = 256 / T cut to gpb * T <= 187 (96 KB of LDS at e = 64):
    # 187 at T = 1, 62 at 3, 11 at 16, 5 at 32, 3 at 62, 2 from 63 to 93, 1 from 94.  (tiles, other, heads) give group counts
    # that are no multiple of gpb wherever gpb > 1 (201 and 45, 69, 27, 10, 27)
    for T in (1, 3, 16, 32, 62, 63, 64, 65, 93, 94, 127, 128):
        for axis in (0, 1):
            tiles, other, heads = {1: ((3, 67, 1), (3, 5, 3))[axis], 3: (3, 23, 1), 62: (2, 5, 1)}.get(T, (3, 3, 3) if T < 94 else (2, 3, 1))
            add("generic", T, other, 64, heads, axis, 0, tiles)
    # generic kernel, e in {16, 32} beyond the MFMA kernels' 64: gpb = 256 / T = 3 up to 85, 2 up to 128, then 1
    for i, T in enumerate((65, 85, 86, 96, 128, 129, 200, 256)):
        for e in (16, 32):
            tiles, other, heads = (2, 5, 1) if T <= 85 else (3, 3, 1) if T <= 128 else (2, 3, 1)
            add("generic", T, other, e, heads, (i + e // 32) % 2, 0, tiles)
    add("generic", 24, 5, 32, 3, 0, 1, 3)                                  # causal never runs on the axial MFMA kernels
    add("generic", 64, 5, 16, 3, 1, 1, 3)
    for causal in (0, 1):                                                  # the text shape beyond 128 without stats_ws
        add("generic", 130, 1, 64, 3, 1, causal, 2, stats=False)
    # one dominating key per query row, one T per route
    for spike in ("first", "last", "tile"):
        add("text_mfma", 77, 1, 64, 3, 1, 1, 2, spike)
        add("text_block", 100, 1, 64, 3, 1, 1, 2, spike)
        add("text_rows", 200, 1, 64, 3, 1, 0, 2, spike)
        add("axial_mfma", 32, 5, 32, 3, 0, 0, 3, spike)
        add("axial_mfma_padded", 33, 5, 16, 3, 1, 0, 3, spike)
        add("generic", 93, 3, 64, 3, 0, 0, 3, spike)
    return out


CASES = _cases()
# the guard cases (a call through the C ABI on slices of larger buffers): one per route
GUARD_CASES = [Case("text_mfma", 77, 1, 64, 3, 1, 1, 2, None, True), Case("text_block", 100, 1, 64, 3, 1, 1, 2, None, True),
               Case("text_rows", 193, 1, 64, 3, 1, 1, 2, None, True), Case("axial_mfma", 32, 5, 32, 3, 0, 0, 3, None, True),
               Case("axial_mfma_padded", 33, 5, 16, 3, 1, 0, 3, None, True), Case("generic", 65, 3, 64, 3, 0, 0, 3, None, True)]


def spike_key(c):
    return {"first": 0, "last": c.T - 1, "tile": 16 * ((c.T - 1) // 16)}[c.spike]


def inputs(c):
    """(qkv [rows, 3 * heads * e], dout [rows, heads * e]) f32 CPU tensors of a case, seeded by it.
    Plain cases: randn, q times 3 (peaked rows), and q, k, v, dout each times 2^k per line, k uniform in -4..4, so that a small
    line is judged on its own S.  Spiked cases (after test_attention_spiked_scores): plain randn; every key loses its component
    along u = (1, ..., 1) / sqrt(e), the spiked key is sqrt(e) u and every query that may see it (all of them, or i >= the key
    when causal) gains 30 u: its score there is 30 + N(0, 1) against N(0, 1) everywhere else."""
    tiles, gn, gl = grid(c)
    a = (tiles, gn, gl, c.heads, c.e, c.axis)
    B = tiles * c.other * c.heads
    g = torch.Generator().manual_seed(1000003 * c.T + 10007 * c.other + 101 * c.e + 13 * c.heads + 7 * c.axis + 3 * c.causal + c.tiles
                                      + (0 if not c.spike else 500 + spike_key(c)))
    q, k, v, dO = (torch.randn(B, c.T, c.e, generator=g) for _ in range(4))
    if c.spike:
        u = torch.full((c.e,), c.e ** -0.5)
        p = spike_key(c)
        k = k - (k @ u).unsqueeze(-1) * u
        k[:, p] = c.e ** 0.5 * u
        q[:, (p if c.causal else 0):] += 30.0 * u
    else:
        q = q * 3.0
        def line_scale():
            s = torch.exp2(torch.randint(-4, 5, (tiles * c.other, 1, 1, 1), generator=g).float())
            return s.expand(-1, c.heads, 1, 1).reshape(B, 1, 1)
        q, k, v, dO = (t * line_scale() for t in (q, k, v, dO))
    q, k, v, dO = (from_lines(t.contiguous(), *a) for t in (q, k, v, dO))
    return torch.cat([q, k, v], 1).contiguous(), dO.contiguous()


def reference(c):
    """(qkv, dout, attention(...)) of a case"""
    qkv, dout = inputs(c)
    return qkv, dout, attention(qkv, dout, *grid(c), c.heads, c.e, c.axis, c.causal, c.e ** -0.5)
