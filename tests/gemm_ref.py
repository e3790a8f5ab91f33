"""Test infrastructure for acx_gemm, route by route and element by element (tests/test_cpu_gemm_routes.py, tests/test_gpu_gemm_routes.py):
plain torch, importable without a GPU.

evaluate(case, t, dtype) is the operation written out plainly:

    epilogue( amap(A - a_sub) . W^T + bias [+ pos0 / pos1] ) [+ residual]

with the row maps spelled out (identity; CONV3X3 as nine shifted products on a zero-padded (gn, gl) grid; TESTTILE through the
oracle's test_tile_index; TILETABLE as a gather from the table) and the five activations.  ref(case, t) is that in fp64, together
with the per-element magnitude S = sum_k |a||w| + |bias| + |pos| + |residual|; for ACX_PREC_BF16 the operands are rounded to bf16
first, as the kernel reads them.

bound(case, ref, S) = 2e-6 S -- the constant the project's element-wise GEMM tests hold (test_gemm_few_rows_kernel,
test_gemm_f32_w8_benchmark_shapes: K up to 3072) -- times 1.5 behind QuickGELU (slope <= 1.1, as those tests), plus 2^-8 |ref| for
a bf16 output (8 significand bits and one double rounding).  Nothing else.

operands(case, device) builds the buffers: asymmetric weights (+ arange(N) 1e-4), rows of A scaled by powers of two, and every
buffer over-allocated and poisoned -- lda = K + 4 (f32) / K + 8 (bf16) with NaN pad columns and NaN rows behind the last row, W
likewise, ldc = N + 4 (N + 8 for a bf16 C) with NaN pad columns and NaN guard rows.  A read past K or M that reaches a stored
element shows as NaN; a write past N or M destroys a guard (guards_intact).

CASES is the table: descriptor keywords, the scratch the caller brings, the context option a row needs, and the route, K pieces,
reduce mechanism and tile count acx_gemm_route must report -- the gates of csrc/acx_gemm.hip, both sides of each.  A row means "this
kernel, this side of this boundary": where the query disagrees the SHAPE is wrong, not the expectation."""
from dataclasses import dataclass, field
from typing import Optional

import torch

from anomalyclip_amd import _lib as L

F32, BF16 = L.PREC_F32, L.PREC_BF16
NONE, GELU, LEAKY, RELU, RESRELU = L.ACT_NONE, L.ACT_QUICKGELU, L.ACT_LEAKYRELU, L.ACT_RELU, L.ACT_RESRELU
IDENT, CONV, TESTTILE, TILETABLE = L.AMAP_IDENTITY, L.AMAP_CONV3X3, L.AMAP_TESTTILE, L.AMAP_TILETABLE
R_NONE, R_TAIL, R_SK, R_X6, R_S64, R_P256, R_W8 = (L.GEMM_ROUTE_NONE, L.GEMM_ROUTE_X6_TAIL_SPLIT, L.GEMM_ROUTE_SK, L.GEMM_ROUTE_X6,
                                                   L.GEMM_ROUTE_S64, L.GEMM_ROUTE_P256, L.GEMM_ROUTE_W8)
R_W8C, R_RING, R_P8, R_DMAC, R_DMA, R_GEN = (L.GEMM_ROUTE_W8_CONV, L.GEMM_ROUTE_RING, L.GEMM_ROUTE_P8, L.GEMM_ROUTE_DMA_CONV,
                                             L.GEMM_ROUTE_DMA, L.GEMM_ROUTE_GENERIC)
ROUTE_NAMES = {R_NONE: "none", R_TAIL: "x6_tail_split", R_SK: "sk", R_X6: "x6", R_S64: "s64", R_P256: "p256", R_W8: "w8",
               R_W8C: "w8_conv", R_RING: "ring", R_P8: "p8", R_DMAC: "dma_conv", R_DMA: "dma", R_GEN: "generic"}
RED_NONE, RED_LAUNCH, RED_COUNTERS = L.GEMM_REDUCE_NONE, L.GEMM_REDUCE_LAUNCH, L.GEMM_REDUCE_COUNTERS
E_BADARG, E_UNSUPPORTED = -1, -2                       # include/acx.h ACX_E_*
NCU = 256                                              # workgroups of a persistent launch: the MI355X's CUs, and the NULL context's

EPS = 2e-6
N_COUNTERS = 4096


@dataclass
class Case:
    name: str
    M: int
    N: int
    K: int
    prec: int = F32
    a_bf16: bool = False            # A stored as bf16 (ACX_PREC_BF16 only)
    c_bf16: bool = False
    act: int = NONE
    bias: bool = True
    res: str = ""                   # "": none, "own": a buffer of its own, "alias": the residual IS C
    a_sub: bool = False
    pos: bool = False
    amap: int = IDENT
    gn: int = 0
    gl: int = 0
    cin: int = 0
    seg: int = 0
    table: Optional[list] = None    # TILETABLE: [(base row, row stride between segments)] per output tile
    ws: bool = False                # the caller brings a split-K workspace (ws_bytes of it)
    ctr: int = 0                    # ... and this many arrival counters (0: none)
    opts: dict = field(default_factory=dict)     # context options the row needs (GPU: set on a context of the test's own)
    # what acx_gemm_route must answer: (route, ksplit, reduce, tiles) under opts on 256 CUs; default_ctx: the same for a NULL context
    # where the options move it (None: no difference)
    expect: tuple = (R_NONE, 1, 0, 0)
    default_ctx: Optional[tuple] = None
    refuse: int = 0                 # ACX_E_* the query and acx_gemm must both answer (then `text` is in acx_last_error)
    text: str = ""
    raw: dict = field(default_factory=dict)      # refusals: descriptor fields overwritten after filling (a broken descriptor)

    @property
    def ka(self):                   # columns of a row of A
        return self.cin if self.amap == CONV else self.K

    @property
    def a_rows(self):
        if self.amap == TILETABLE:
            return max(b + (self.gn - 1) * s + self.gl for b, s in self.table)
        return self.M

    @property
    def ws_bytes(self):             # enough for every split rule: 16 partial images, or the few-row kernel's 512 partial tiles
        return max(16 * self.M * self.N * 4, 512 * 4096) if self.ws else 0

    @property
    def lda(self):
        return self.ka + (8 if self.a_bf16 else 4)

    @property
    def ldw(self):
        return self.K + (8 if self.prec == BF16 else 4)

    @property
    def ldc(self):
        return self.N + (8 if self.c_bf16 else 4)


# ---------------------------------------------------------------------------------------------------------------- operands
NAN32, NAN16 = 0x7FC0BEEF, 0x7FCE                     # the poison: quiet NaNs with a payload of their own


def _poison(rows, cols, dtype, device):
    if dtype == torch.bfloat16:
        return torch.full((rows, cols), NAN16, dtype=torch.int16, device=device).view(torch.bfloat16)
    return torch.full((rows, cols), NAN32, dtype=torch.int32, device=device).view(torch.float32)


def _padded(x, ld, guard_rows=2):
    """x [r, c] inside a poisoned [r + guard_rows, ld] buffer; returns (buffer, view of x's place)"""
    buf = _poison(x.shape[0] + guard_rows, ld, x.dtype, x.device)
    buf[:x.shape[0], :x.shape[1]] = x
    return buf, buf[:x.shape[0], :x.shape[1]]


def guards_intact(buf, rows, cols):
    """every element of buf outside [0, rows) x [0, cols) still holds its poison, bit for bit"""
    bits = buf.view(torch.int16 if buf.dtype == torch.bfloat16 else torch.int32)
    want = NAN16 if buf.dtype == torch.bfloat16 else NAN32
    return bool((bits[rows:] == want).all()) and bool((bits[:rows, cols:] == want).all())


def operands(c: Case, device="cpu"):
    """the operands of a case: values (CPU generator, so both test files see the same numbers) in poisoned, over-allocated buffers"""
    g = torch.Generator().manual_seed(c.M * 31 + c.N * 7 + c.K + c.act + 17 * c.amap)
    a = torch.randn(c.a_rows, c.ka, generator=g) * torch.exp2(torch.randint(-3, 3, (c.a_rows, 1), generator=g).float())
    w = torch.randn(c.N, c.K, generator=g) * c.K ** -0.5 + torch.arange(c.N).view(-1, 1) * 1e-4
    t = {"bias": torch.randn(c.N, generator=g) if c.bias else None,
         "res": torch.randn(c.M, c.N, generator=g) if c.res else None,
         "a_sub": torch.randn(c.K, generator=g) if c.a_sub else None,
         "pos0": torch.randn(c.gn, c.N, generator=g) if c.pos else None,
         "pos1": torch.randn(c.gl, c.N, generator=g) if c.pos else None}
    a = a.to(device)
    w = w.to(device)
    if c.a_bf16:
        a = a.bfloat16()
    if c.prec == BF16:
        w = w.bfloat16()
    t = {k: (v.to(device) if v is not None else None) for k, v in t.items()}
    t["a_buf"], t["a"] = _padded(a, c.lda)
    t["w_buf"], t["w"] = _padded(w, c.ldw)
    c_dtype = torch.bfloat16 if c.c_bf16 else torch.float32
    t["c_buf"] = _poison(c.M + 2, c.ldc, c_dtype, device)
    t["c"] = t["c_buf"][:c.M, :c.N]
    if c.res == "own":
        t["res_buf"], t["res"] = _padded(t["res"], c.ldc)
    elif c.res == "alias":                              # the residual starts out in C's place (f32 C only)
        t["c"].copy_(t["res"])
        t["res_buf"] = t["c_buf"]
    if c.amap == TILETABLE:
        t["table"] = torch.tensor(c.table, dtype=torch.int32, device=device).reshape(-1, 2).contiguous()
    return t


# ---------------------------------------------------------------------------------------------------------------- reference
def quick_gelu(x):
    return x * torch.sigmoid(1.702 * x)


def source_rows(c: Case, device="cpu"):
    """TESTTILE / TILETABLE: the row of A that output row m reads"""
    if c.amap == TESTTILE:
        from oracle import anomalyclip_oracle as O
        return O.test_tile_index(c.M, c.gn, c.gl, c.seg).to(device)
    base = torch.tensor([b for b, _ in c.table], device=device).view(-1, 1, 1)
    stride = torch.tensor([s for _, s in c.table], device=device).view(-1, 1, 1)
    n = torch.arange(c.gn, device=device).view(1, -1, 1)
    l = torch.arange(c.gl, device=device).view(1, 1, -1)
    return (base + n * stride + l).reshape(-1)


def evaluate(c: Case, t, dtype=torch.float64, magnitude=False):
    """the product and its epilogue in `dtype`; magnitude: also S, the sum of the absolute values of every term"""
    a, w = t["a"].to(dtype), t["w"].to(dtype)          # (bf16 operands: already rounded)
    if c.prec == BF16 and not c.a_bf16:
        a = t["a"].bfloat16().to(dtype)                 # f32 A converted to bf16 in the loader
    if c.a_sub:
        a = a - t["a_sub"].to(dtype)
    if c.amap in (TESTTILE, TILETABLE):
        a = a[source_rows(c, a.device)]
    if c.amap == CONV:
        tiles = c.M // (c.gn * c.gl)
        xp = torch.nn.functional.pad(a.view(tiles, c.gn, c.gl, c.cin), (0, 0, 1, 1, 1, 1))      # zero halo on the (gn, gl) grid
        w9 = w.view(c.N, 9, c.cin)
        acc = torch.zeros(c.M, c.N, dtype=dtype, device=a.device)
        mag = torch.zeros_like(acc)
        for kh in range(3):
            for kw in range(3):
                x = xp[:, kh:kh + c.gn, kw:kw + c.gl, :].reshape(c.M, c.cin)
                acc += x @ w9[:, kh * 3 + kw, :].t()
                if magnitude:
                    mag += x.abs() @ w9[:, kh * 3 + kw, :].abs().t()
    else:
        acc = a[:c.M] @ w.t()
        mag = a[:c.M].abs() @ w.abs().t() if magnitude else None
    if c.bias:
        acc = acc + t["bias"].to(dtype)
        if magnitude:
            mag = mag + t["bias"].to(dtype).abs()
    if c.act == GELU:
        acc = quick_gelu(acc)
    elif c.act == LEAKY:
        acc = torch.where(acc > 0, acc, 0.01 * acc)
    elif c.act == RELU:
        acc = acc.clamp_min(0)
    if c.pos:
        m = torch.arange(c.M, device=acc.device)
        p = t["pos0"].to(dtype)[(m // c.gl) % c.gn] + t["pos1"].to(dtype)[m % c.gl]
        acc = acc + p
        if magnitude:
            mag = mag + t["pos0"].to(dtype).abs()[(m // c.gl) % c.gn] + t["pos1"].to(dtype).abs()[m % c.gl]
    if c.res:
        acc = acc + t["res"].to(dtype)
        if magnitude:
            mag = mag + t["res"].to(dtype).abs()
    if c.act == RESRELU:
        acc = acc.clamp_min(0)
    return (acc, mag) if magnitude else acc


def ref(c: Case, t):
    """(fp64 reference, S) -- computed BEFORE acx_gemm runs (an aliased residual is overwritten by it)"""
    return evaluate(c, t, torch.float64, magnitude=True)


def bound(c: Case, r, S):
    b = EPS * S * (1.5 if c.act == GELU else 1.0)
    if c.c_bf16:
        b = b + 2.0 ** -8 * r.abs()
    return b


# ---------------------------------------------------------------------------------------------------------------- descriptor
_PTR = 0x10000                                         # dummy 16-byte aligned addresses: the query dereferences nothing


def desc(c: Case, t=None):
    """the acx_gemm_desc of a case, filled by hand: operands of t (operands()), or dummy addresses for the host-only query.
    Workspace, counters, zero page and tile table: the caller sets them (scratch())."""
    d = L.GemmDesc()
    ptr = (lambda k, i: t[k].data_ptr()) if t is not None else (lambda k, i: i * _PTR)
    d.A, d.W, d.C = ptr("a_buf", 1), ptr("w_buf", 2), ptr("c_buf", 3)
    d.M, d.N, d.K = c.M, c.N, c.K
    d.lda, d.ldw, d.ldc = c.lda, c.ldw, c.ldc
    d.a_dtype = L.ACX_BF16 if c.a_bf16 else L.ACX_F32
    d.c_dtype = L.ACX_BF16 if c.c_bf16 else L.ACX_F32
    d.prec, d.act = c.prec, c.act
    if c.bias:
        d.bias = ptr("bias", 4)
    if c.res:
        d.residual, d.ldr = ptr("res_buf", 3 if c.res == "alias" else 5), c.ldc
    if c.a_sub:
        d.a_sub = ptr("a_sub", 6)
    if c.pos:
        d.pos0, d.pos1 = ptr("pos0", 7), ptr("pos1", 8)
    d.amap, d.gn, d.gl, d.cin, d.seg = c.amap, c.gn, c.gl, c.cin, c.seg
    if t is None:
        if c.amap == TILETABLE:
            d.tile_table = 9 * _PTR
        if c.amap == CONV:
            d.zero_page = 10 * _PTR
        if c.ws:
            d.workspace, d.workspace_bytes = 11 * _PTR, c.ws_bytes
        if c.ctr:
            d.counters, d.n_counters = 12 * _PTR, c.ctr
    for k, v in c.raw.items():
        setattr(d, k, v)
    return d


def query(h, d):
    """acx_gemm_route -> (return code, (route, ksplit, reduce, tiles))"""
    import ctypes as C
    out = L.GemmRoute()
    rc = L.lib().acx_gemm_route(h, C.byref(d), C.byref(out))
    return rc, (out.route, out.ksplit, out.reduce, out.tiles)


# ---------------------------------------------------------------------------------------------------------------- the table
def t128(M, N):
    return ((M + 127) // 128) * ((N + 127) // 128)


def t64(M, N):
    return ((M + 63) // 64) * ((N + 63) // 64)


def t32(M, N):
    return ((M + 31) // 32) * ((N + 31) // 32)


def t256(M, N):
    return ((M + 255) // 256) * ((N + 255) // 256)


def _cases():
    out = []

    def add(name, M, N, K, expect, **kw):
        out.append(Case(name, M, N, K, expect=expect, **kw))

    # ---- few-row kernel (32 x 32 tiles, K % 256 == 0): gemm_f32_sk_kernel
    add("sk-rows-320", 320, 768, 256, (R_SK, 1, 0, t32(320, 768)))
    add("sk-rows-321-w8", 321, 768, 256, (R_W8, 1, 0, 18))                            # behind the row limit: 72 64-tiles < 96
    add("sk-narrow-1280", 1280, 512, 256, (R_SK, 1, 0, t32(1280, 512)))
    add("sk-narrow-1281-s64", 1281, 512, 256, (R_S64, 1, 0, t64(1281, 512)))
    add("sk-pieces-4", 77, 512, 2048, (R_SK, 4, RED_COUNTERS, 48), ws=True, ctr=N_COUNTERS)
    add("sk-pieces-too-many", 77, 2048, 2048, (R_SK, 1, 0, 192), ws=True, ctr=N_COUNTERS)      # 192 tiles x 4 pieces > 512
    add("sk-pieces-k768", 77, 512, 768, (R_SK, 1, 0, 48), ws=True, ctr=N_COUNTERS)             # K % 512 != 0
    add("sk-pieces-3-k1536", 77, 512, 1536, (R_SK, 3, RED_COUNTERS, 48), ws=True, ctr=N_COUNTERS, act=GELU)
    add("sk-pieces-few-counters", 77, 512, 2048, (R_SK, 1, 0, 48), ws=True, ctr=47)            # fewer counters than tiles
    add("sk-pieces-no-counters", 77, 512, 2048, (R_SK, 1, 0, 48), ws=True)
    add("sk-pieces-no-workspace", 77, 512, 2048, (R_SK, 1, 0, 48), ctr=N_COUNTERS)
    add("sk-pieces-res-alias", 33, 100, 1024, (R_SK, 2, RED_COUNTERS, t32(33, 100)), ws=True, ctr=N_COUNTERS, res="alias")
    add("sk-long-k-768", 768, 512, 1536, (R_SK, 1, 0, t32(768, 512)), ws=True)                    # narrow outputs, long K, a workspace:
    add("sk-long-k-769-s64", 769, 512, 1536, (R_S64, 4, RED_LAUNCH, t64(769, 512)), ws=True)      # above 768 rows the 64 x 64 kernel, split
    add("sk-long-k-1280", 1078, 512, 1280, (R_SK, 1, 0, t32(1078, 512)), ws=True)                 # ... from K = 1536
    add("sk-m1-n36", 1, 36, 256, (R_SK, 1, 0, 2), act=GELU)
    add("sk-res", 154, 100, 512, (R_SK, 1, 0, t32(154, 100)), res="own")
    add("sk-gelu-res-w8", 154, 100, 512, (R_W8, 1, 0, 2), res="own", act=GELU)                 # no such few-row epilogue
    add("sk-n-mod4-w8", 154, 102, 512, (R_W8, 1, 0, 2))                                        # N % 4 != 0
    add("sk-k-mod256-w8", 154, 100, 288, (R_W8, 1, 0, 2))

    # ---- 64 x 64 tiles (128-tiles <= 256 and 64-tiles >= 96): gemm_f32_s64_kernel
    add("s64-96", 321, 1024, 32, (R_S64, 1, 0, 96))
    add("s64-90-w8", 321, 960, 32, (R_W8, 1, 0, 24))
    add("s64-256", 2048, 2048, 32, (R_S64, 1, 0, 1024))
    add("s64-257-w8", 2049, 2048, 32, (R_W8, 1, 0, 272))
    for act, res in ((NONE, ""), (NONE, "own"), (GELU, ""), (GELU, "own"), (RELU, ""), (RELU, "own"), (RESRELU, "own")):
        add(f"s64-epi-{act}{'r' if res else ''}", 641, 708, 64, (R_S64, 1, 0, t64(641, 708)), act=act, res=res)     # M % 64 = 1, N % 64 = 4
    add("s64-ragged-63", 703, 710, 96, (R_S64, 1, 0, t64(703, 710)), res="alias")               # M % 64 = 63, N % 4 = 2
    add("s64-nobias", 641, 708, 32, (R_S64, 1, 0, t64(641, 708)), bias=False)
    S = t64(513, 768)                                                                         # 108 tiles of 64 x 64
    add("s64-split8", 513, 768, 3072, (R_S64, 8, RED_LAUNCH, S), ws=True)
    add("s64-split4", 513, 768, 1536, (R_S64, 4, RED_LAUNCH, S), ws=True, act=GELU)
    add("s64-split2", 513, 768, 1024, (R_S64, 2, RED_LAUNCH, S), ws=True, res="own")
    add("s64-split-none-k992", 513, 768, 992, (R_S64, 1, 0, S), ws=True)
    add("s64-split-ragged-k1056", 513, 768, 1056, (R_S64, 2, RED_LAUNCH, S), ws=True, act=RESRELU, res="own")     # 33 K-steps: 17 + 16
    add("s64-split-no-workspace", 513, 768, 1056, (R_S64, 1, 0, S))
    add("s64-split-res-alias", 513, 768, 1024, (R_S64, 2, RED_LAUNCH, S), ws=True, res="alias")
    add("s64-split-relu-ragged-n", 577, 710, 1024, (R_S64, 2, RED_LAUNCH, t64(577, 710)), ws=True, act=RELU)
    add("s64-long-k-takes-rows", 1078, 512, 1536, (R_S64, 4, RED_LAUNCH, t64(1078, 512)), ws=True)    # (the few-row kernel without a workspace)
    add("s64-long-k-no-workspace-sk", 1078, 512, 1536, (R_SK, 1, 0, t32(1078, 512)))

    # ---- persistent strip stream (>= 1024 tiles of 128 x 128, no residual): gemm_f32_p256_kernel
    add("p256-1024", 32768, 512, 32, (R_P256, 1, 0, 1024))
    add("p256-1020-w8", 32640, 512, 32, (R_W8, 1, 0, 1020))
    add("p256-ragged-m", 32768 - 5, 512, 32, (R_P256, 1, 0, 1024), act=GELU)
    add("p256-ragged-n", 26240 - 5, 516, 64, (R_P256, 1, 0, 1025), act=RELU)
    add("p256-relu", 32768, 512, 32, (R_P256, 1, 0, 1024), act=RELU, bias=False)
    add("p256-residual-w8", 32768, 512, 32, (R_W8, 1, 0, 1024), res="own")
    add("p256-leaky-generic", 32768, 512, 32, (R_GEN, 1, 0, 1024), act=LEAKY)                   # LeakyReLU on identity rows: gemm_kernel
    cv = dict(amap=CONV, gn=16, gl=16, cin=32)
    for act in (NONE, LEAKY, RELU):
        add(f"p256-conv-{act}", 32768, 512, 288, (R_P256, 1, 0, 1024), act=act, **cv)
    add("p256-conv-residual-w8", 32768, 512, 288, (R_W8C, 1, 0, 1024), res="own", **cv)
    add("p256-conv-grid-7x9-w8", 63 * 520, 512, 288, (R_W8C, 1, 0, t128(63 * 520, 512)), amap=CONV, gn=7, gl=9, cin=32)

    # ---- 8 waves per 128 x 128 tile, identity rows: gemm_f32_w8_kernel<., ., 0> and its 8-XCD remap.  (24 .. 256 tiles of
    # 128 x 128 are >= 96 tiles of 64 x 64: the 64 x 64 kernel's; so 5, 18, 21 below and 257, 258, 261 above)
    for M, N, tiles in ((637, 128, 5), (321, 768, 18), (891, 384, 21), (32800, 128, 257), (16400, 256, 258), (11130, 384, 261)):
        add(f"w8-tiles-{tiles}", M, N, 32, (R_W8, 1, 0, tiles), act=GELU if tiles % 2 else NONE)
    for act, res in ((NONE, ""), (NONE, "own"), (GELU, ""), (GELU, "own"), (RELU, ""), (RELU, "own"), (RESRELU, "own")):
        add(f"w8-epi-{act}{'r' if res else ''}", 891, 382, 96, (R_W8, 1, 0, 21), act=act, res=res)
    add("w8-res-alias", 891, 382, 64, (R_W8, 1, 0, 21), res="alias")

    # ---- ... and the f32 3 x 3 convolutions: gemm_f32_w8_kernel<., ., 1>
    g16x8 = dict(amap=CONV, gn=16, gl=8, cin=32)
    add("w8c-tiles-5", 640, 128, 288, (R_W8C, 1, 0, 5), **g16x8)
    add("w8c-tiles-18-16x16", 2304, 128, 288, (R_W8C, 1, 0, 18), act=LEAKY, **cv)
    add("w8c-tiles-21", 896, 384, 288, (R_W8C, 1, 0, 21), **g16x8)
    add("w8c-tiles-64-32x16", 1024, 1024, 288, (R_W8C, 1, 0, 64), amap=CONV, gn=32, gl=16, cin=32)
    add("w8c-tiles-257", 32896, 128, 288, (R_W8C, 1, 0, 257), res="own", **g16x8)
    add("w8c-grid-7x9", 315, 200, 288, (R_W8C, 1, 0, 6), act=LEAKY, res="own", amap=CONV, gn=7, gl=9, cin=32)    # M % 128 = 59
    add("w8c-grid-1x8", 160, 100, 288, (R_W8C, 1, 0, 2), amap=CONV, gn=1, gl=8, cin=32)
    add("w8c-grid-8x1", 160, 100, 288, (R_W8C, 1, 0, 2), amap=CONV, gn=8, gl=1, cin=32)
    add("w8c-cin96", 315, 200, 864, (R_W8C, 1, 0, 6), amap=CONV, gn=7, gl=9, cin=96)
    for act, res in ((NONE, ""), (NONE, "own"), (GELU, ""), (GELU, "own"), (LEAKY, ""), (LEAKY, "own"), (RELU, ""), (RELU, "own"),
                     (RESRELU, "own")):
        add(f"w8c-epi-{act}{'r' if res else ''}", 512, 132, 288, (R_W8C, 1, 0, 8), act=act, res=res, **cv)
    add("w8c-split-counters", 256, 128, 288, (R_W8C, 2, RED_COUNTERS, 2), ws=True, ctr=N_COUNTERS, act=LEAKY, **cv)   # 9 K-steps: 5 + 4
    add("w8c-split-reduce-launch", 256, 128, 288, (R_W8C, 2, RED_LAUNCH, 2), ws=True, act=LEAKY, **cv)
    add("w8c-split-few-counters", 256, 128, 288, (R_W8C, 2, RED_LAUNCH, 2), ws=True, ctr=1, res="own", **cv)
    add("w8c-split-no-workspace", 256, 128, 288, (R_W8C, 1, 0, 2), ctr=N_COUNTERS, **cv)
    add("w8c-split4-cin96", 315, 200, 864, (R_W8C, 4, RED_COUNTERS, 6), ws=True, ctr=N_COUNTERS, res="alias", amap=CONV, gn=7, gl=9, cin=96)
    add("w8c-split4-cin96-launch", 315, 200, 864, (R_W8C, 4, RED_LAUNCH, 6), ws=True, act=RELU, amap=CONV, gn=7, gl=9, cin=96)
    add("w8c-split-counters-gelu", 512, 132, 576, (R_W8C, 4, RED_COUNTERS, 8), ws=True, ctr=N_COUNTERS, act=GELU, amap=CONV, gn=16, gl=16, cin=64)

    # ---- gemm_kernel, f32: what no branch-free kernel takes (K tails, a_sub, the positional epilogue, the tile maps, LeakyReLU on
    # identity rows, a bf16 C), unsplit and -- where generic_ksplit's gen_split applies -- split, the epilogue in splitk_reduce_kernel
    add("gen-k36", 130, 70, 36, (R_GEN, 1, 0, 2))                                              # K % 32 = 4, N % 4 = 2
    add("gen-k60", 130, 70, 60, (R_GEN, 1, 0, 2), act=GELU, res="own")                         # K % 32 = 28
    add("gen-k92-n5", 130, 5, 92, (R_GEN, 1, 0, 2), res="alias")
    add("gen-m1", 1, 5, 4, (R_GEN, 1, 0, 1))
    add("gen-relu-runtime", 130, 70, 36, (R_GEN, 1, 0, 2), act=RELU)
    add("gen-resrelu-runtime", 130, 70, 60, (R_GEN, 1, 0, 2), act=RESRELU, res="own")
    add("gen-relu-res-runtime", 257, 132, 36, (R_GEN, 1, 0, 6), act=RELU, res="own")
    add("gen-leaky-identity", 300, 200, 96, (R_GEN, 1, 0, 6), act=LEAKY)
    add("gen-leaky-never-splits", 300, 200, 256, (R_GEN, 1, 0, 6), act=LEAKY, ws=True)
    add("gen-asub", 300, 200, 96, (R_GEN, 1, 0, 6), a_sub=True, act=GELU, res="own")
    add("gen-asub-k-tail", 300, 200, 100, (R_GEN, 1, 0, 6), a_sub=True)
    add("gen-asub-split", 300, 200, 256, (R_GEN, 2, RED_LAUNCH, 6), a_sub=True, ws=True, act=GELU, res="own")
    add("gen-asub-no-workspace", 300, 200, 256, (R_GEN, 1, 0, 6), a_sub=True)
    add("gen-asub-split-k-tail-none", 300, 200, 260, (R_GEN, 1, 0, 6), a_sub=True, ws=True)     # K % 32 != 0: no split
    grid = dict(gn=4, gl=8)
    add("gen-pos", 320, 70, 64, (R_GEN, 1, 0, 3), pos=True, **grid)
    add("gen-pos-split", 320, 70, 288, (R_GEN, 2, RED_LAUNCH, 3), pos=True, ws=True, res="own", **grid)          # 9 K-steps: 5 + 4
    add("gen-pos-split-relu-refused", 320, 70, 288, (R_NONE, 1, 0, 0), pos=True, ws=True, act=RELU, refuse=E_UNSUPPORTED,
        text="ACX_ACT_RELU / ACX_ACT_RESRELU need an f32 or a pairs = 6 product", **grid)
    for seg in (1, 2, 3):
        add(f"gen-testtile-{seg}", 64 * seg * 2, 68, 64, (R_GEN, 1, 0, t128(128 * seg, 68)), amap=TESTTILE, seg=seg, pos=True, **grid)
        add(f"gen-testtile-{seg}-split", 64 * seg * 2, 68, 512, (R_GEN, 4, RED_LAUNCH, t128(128 * seg, 68)), amap=TESTTILE, seg=seg,
            pos=True, ws=True, act=GELU, **grid)
    # two videos in 160 source rows: rows 0 .. 96 with segment size 3 (tiles at 0, 8, 16, stride 24), rows 96 .. 160 with 2 (96, 104,
    # stride 16); the table permutes them and takes one tile twice
    table = [(104, 16), (0, 24), (16, 24), (96, 16), (8, 24), (16, 24), (0, 24)]
    add("gen-tiletable", 32 * 7, 70, 64, (R_GEN, 1, 0, 2), amap=TILETABLE, table=table, pos=True, **grid)
    add("gen-tiletable-split", 32 * 7, 70, 256, (R_GEN, 2, RED_LAUNCH, 2), amap=TILETABLE, table=table, ws=True, res="own", **grid)
    add("gen-tiletable-k-tail", 32 * 7, 70, 36, (R_GEN, 1, 0, 2), amap=TILETABLE, table=table, act=LEAKY, **grid)
    add("gen-f32-bf16-out", 300, 200, 96, (R_GEN, 1, 0, 6), c_bf16=True, act=GELU)
    add("gen-fast-split7", 400, 600, 1056, (R_GEN, 7, RED_LAUNCH, 20), ws=True, act=GELU, res="own")    # branch-free + split: 33 steps as 6 x 5 + 3
    add("gen-fast-no-workspace-w8", 400, 600, 1056, (R_W8, 1, 0, 20), act=GELU, res="own")

    # ---- gemm_kernel, bf16 MFMA
    b = dict(prec=BF16)
    add("genb-f32-a", 300, 200, 128, (R_GEN, 1, 0, 6), **b)                                     # f32 A converted in the loader
    add("genb-f32-a-k-tail", 300, 200, 72, (R_GEN, 1, 0, 6), act=GELU, res="own", **b)
    add("genb-f32-a-bf16-out", 300, 200, 128, (R_GEN, 1, 0, 6), c_bf16=True, **b)
    add("genb-k-tail", 300, 200, 40, (R_GEN, 1, 0, 6), a_bf16=True, **b)                        # K % 64 = 40: not branch-free, not DMA
    add("genb-k-tail-bf16-out", 130, 72, 104, (R_GEN, 1, 0, 2), a_bf16=True, c_bf16=True, act=LEAKY, **b)
    add("genb-split-f32-out", 300, 200, 1024, (R_GEN, 2, RED_LAUNCH, 6), a_bf16=True, ws=True, res="own", **b)    # splitk_reduce_kernel<0>
    add("genb-split-bf16-out", 300, 200, 1024, (R_GEN, 2, RED_LAUNCH, 6), a_bf16=True, c_bf16=True, ws=True, act=GELU, **b)   # <1>
    add("genb-split-f32-a", 300, 200, 2048, (R_GEN, 4, RED_LAUNCH, 6), ws=True, **b)
    add("genb-split-short-k-dma", 300, 200, 960, (R_DMA, 1, 0, 6), a_bf16=True, ws=True, **b)   # 15 K-steps: pieces would be < 8

    # ---- persistent 256 x 256 bf16 kernels (ACX_OPT_RING_MIN_TILES lowered): (K / 64) odd -> ring, even -> p8
    ring = {L.OPT_RING_MIN_TILES: 1}
    bb = dict(prec=BF16, a_bf16=True, opts=ring)
    for kern, route, K in (("ring", R_RING, 64), ("p8", R_P8, 128)):
        # (258 tiles, three tile columns: the second tile of workgroups 0 and 1 lies in another column than their first)
        for M, N, what in ((777, 1000, "16-tiles"), (256 * NCU, 256, "ncu-tiles"), (256 * (NCU + 1) - 9, 252, "ncu+1-tiles"),
                           (256 * 86 - 9, 760, "ncu+2-tiles-3-wide")):
            add(f"{kern}-{what}", M, N, K, (route, 1, 0, t256(M, N)), default_ctx=(R_DMA, 1, 0, t128(M, N)),
                res="own" if what == "ncu+1-tiles" else "", **bb)
        for act, res, cb in ((NONE, "", 0), (NONE, "", 1), (GELU, "", 0), (GELU, "", 1), (NONE, "own", 0), (NONE, "own", 1)):
            add(f"{kern}-epi-{act}{'r' if res else ''}{'b' if cb else ''}", 777, 1000, K + 128, (route, 1, 0, 16),
                default_ctx=(R_DMA, 1, 0, t128(777, 1000)), act=act, res=res, c_bf16=bool(cb), **bb)
    add("p8-k3072-gelu-bf16-out", 5000, 300, 3072, (R_P8, 1, 0, 40), default_ctx=(R_DMA, 1, 0, 120), act=GELU, c_bf16=True, **bb)   # (no workspace)
    add("ring-k64-one-tile", 256, 256, 64, (R_RING, 1, 0, 1), default_ctx=(R_DMA, 1, 0, 4), **bb)
    add("ring-gelu-res-dma", 777, 1000, 64, (R_DMA, 1, 0, t128(777, 1000)), act=GELU, res="own", **bb)    # no such ring epilogue
    add("ring-n-mod4-dma", 777, 1002, 64, (R_DMA, 1, 0, t128(777, 1002)), **bb)
    add("ring-default-512-tiles", 256 * 512, 256, 64, (R_RING, 1, 0, 512), prec=BF16, a_bf16=True)
    add("ring-default-511-tiles-dma", 256 * 511, 256, 64, (R_DMA, 1, 0, t128(256 * 511, 256)), prec=BF16, a_bf16=True)

    # ---- 128 x 128 bf16 tiles staged by LDS-DMA: gemm_bf16_dma_kernel, identity rows and the 3 x 3 convolutions
    bd = dict(prec=BF16, a_bf16=True)
    for cb in (0, 1):
        for act in (NONE, GELU):
            for res in ("", "own"):
                add(f"dma-{'b' if cb else 'f'}{act}{'r' if res else ''}", 300, 200, 64, (R_DMA, 1, 0, 6), c_bf16=bool(cb), act=act, res=res, **bd)
    add("dma-k192-ragged", 391, 260, 192, (R_DMA, 1, 0, 12), **bd)
    add("dma-leaky-generic", 300, 200, 64, (R_GEN, 1, 0, 6), act=LEAKY, **bd)
    cv64 = dict(amap=CONV, gn=16, gl=16, cin=64)
    for cb in (0, 1):
        for act, res in ((LEAKY, ""), (NONE, "own"), (NONE, "")):
            add(f"dmac-{'b' if cb else 'f'}{act}{'r' if res else ''}", 512, 136, 576, (R_DMAC, 1, 0, 8), c_bf16=bool(cb), act=act, res=res,
                **cv64, **bd)
    add("dmac-m-mod128-generic", 63 * 5, 136, 576, (R_GEN, 1, 0, 6), amap=CONV, gn=7, gl=9, cin=64, **bd)
    add("dmac-gelu-generic", 512, 136, 576, (R_GEN, 1, 0, 8), act=GELU, **cv64, **bd)
    add("dmac-leaky-res-generic", 512, 136, 576, (R_GEN, 1, 0, 8), act=LEAKY, res="own", **cv64, **bd)

    # ---- refusals: every text of gemm_validate and of the routes in this scope, once
    def refuse(name, code, text, M=130, N=72, K=64, **kw):
        out.append(Case(name, M, N, K, refuse=code, text=text, **kw))

    refuse("no-a", E_BADARG, "null pointer", raw=dict(A=0))
    refuse("no-rows", E_BADARG, "empty shape", raw=dict(M=0))
    refuse("prec", E_UNSUPPORTED, "unknown precision", raw=dict(prec=7))
    refuse("fp16-planes", E_UNSUPPORTED, "fp16 planes", prec=BF16, raw=dict(a_dtype=L.ACX_F16))
    refuse("f32-bf16-a", E_UNSUPPORTED, "PREC_F32 needs f32 A", raw=dict(a_dtype=L.ACX_BF16, lda=72))
    refuse("k-mod4", E_BADARG, "must be multiples of", raw=dict(K=66))
    refuse("lda-mod4", E_BADARG, "must be multiples of", raw=dict(lda=70))
    refuse("a-misaligned", E_BADARG, "16-byte aligned", raw=dict(A=_PTR + 8))
    refuse("asub-bf16-a", E_BADARG, "a_sub needs f32 A", prec=BF16, a_bf16=True, a_sub=True)
    refuse("conv-geometry", E_BADARG, "bad conv3x3 geometry", M=128, K=288, amap=CONV, gn=16, gl=8, cin=32, raw=dict(cin=24))
    refuse("conv-rows", E_BADARG, "bad conv3x3 geometry", M=128, K=288, amap=CONV, gn=16, gl=8, cin=32, raw=dict(M=130))
    refuse("conv-asub", E_UNSUPPORTED, "a_sub with conv3x3", M=128, K=288, amap=CONV, gn=16, gl=8, cin=32, raw=dict(a_sub=6 * _PTR))
    refuse("tiletable-none", E_BADARG, "TILETABLE needs tile_table", M=64, amap=TILETABLE, table=[(0, 8), (0, 8)], gn=4, gl=8,
           raw=dict(tile_table=0))
    refuse("testtile-geometry", E_BADARG, "bad test-tile geometry", M=128, amap=TESTTILE, gn=4, gl=8, seg=3)
    refuse("amap", E_UNSUPPORTED, "unknown amap", raw=dict(amap=9))
    refuse("pos-one", E_BADARG, "pos0/pos1 need both", M=128, pos=True, gn=4, gl=8, raw=dict(pos1=0))
    refuse("relu-bf16", E_UNSUPPORTED, "ACX_ACT_RELU / ACX_ACT_RESRELU need", prec=BF16, a_bf16=True, act=RELU)
    refuse("resrelu-no-residual", E_BADARG, "ACX_ACT_RESRELU needs a residual", act=RESRELU)
    refuse("act", E_BADARG, "unknown act", raw=dict(act=9))
    refuse("a-act-k-tail", E_UNSUPPORTED, "need the few-row f32 kernel", K=36, raw=dict(a_act=GELU))
    refuse("a-norm-k", E_UNSUPPORTED, "a_norm needs K == 512", K=256, N=72, raw=dict(a_norm_w=13 * _PTR, a_norm_b=14 * _PTR))
    refuse("bf16x3-residual", E_UNSUPPORTED, "c_dtype ACX_BF16X3 needs", M=777, N=1000, K=128, prec=BF16, a_bf16=True, res="own",
           opts=ring, raw=dict(c_dtype=L.BF16X3))
    refuse("pairs3-misfit", E_UNSUPPORTED, "pairs = 3 needs bf16 planes", M=777, N=1000, K=128, prec=BF16, a_bf16=True,
           raw=dict(pairs=3))
    refuse("pairs6-misfit", E_UNSUPPORTED, "pairs = 6 needs bf16 planes", M=777, N=1000, K=128, prec=BF16, a_bf16=True,
           raw=dict(pairs=6))
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
RUN_CASES = [c for c in CASES if not c.refuse]
REFUSALS = [c for c in CASES if c.refuse]
