"""Test infrastructure for the transposed (weight-gradient) products -- acx_gemm_tn, _zp, _parts, _group and acx_gemm_tn_x6 -- route by
route and element by element (tests/test_cpu_tn_routes.py, tests/test_gpu_tn_routes.py): plain torch, importable without a GPU.

evaluate(case, t, dtype) is the operation written out plainly:

    C[N1, N2] = A^T (bmap(B) - b_sub)

conv: column tap * cin + ci of bmap(B) at row m = tile * gn * gl + n * gl + l is B[tile * gn * gl + (n + dn) * gl + (l + dl), ci] with
(dn, dl) = (tap // 3 - 1, tap % 3 - 1), zero where (n + dn, l + dl) leaves the (gn, gl) grid -- index arithmetic on the row number,
one tap at a time, no branch of any kernel.  ref(case, t) is that in fp64 with the magnitude S = |A|^T |bmap(B) - b_sub|.

bound: every element within EPS * S, EPS = 2e-6 (gemm_ref.EPS, the figure of test_gemm_tn_256_tiles_plain); the plane kernel's
rows 2.5e-6 (what test_gemm_tn_x6_random_shapes_vs_fp64 holds it to).  Nothing else.

operands(case, device): randn, A's rows scaled by 2^randint(-3, 3), b_sub ~ randn, in poisoned buffers (gemm_ref._poison /
_padded): NaN pad columns where the row has ld > N, two NaN guard rows behind row M - 1, two behind row N1 - 1 of C.

CASES is the table: the call's arguments, the workspace and zero page the caller brings, the context option a row needs and the
(kernel, splits, rows per split, tiles, reduce) acx_gemm_tn_route / acx_gemm_tn_x6_route must report -- literals, replayed by hand
from tn_choose_splits, tn_p256_splits and x6_choose_split (csrc/acx_gemm.hip), both sides of every gate of tn_takes_p256, tn_x6_mode
and the workspace fallbacks.  A row means "this kernel, this side of this boundary": where the query disagrees the SHAPE is wrong,
not the expectation."""
from dataclasses import dataclass, field
from typing import Optional

import torch

from anomalyclip_amd import _lib as L

from gemm_ref import EPS, NAN16, NAN32, NCU, _padded, _poison, guards_intact  # noqa: F401  (shared, not copied)

EPS_X6 = 2.5e-6
K_NONE, K_W8, K_P256, K_X6_256x256, K_X6_256x128, K_X6_128x256 = (L.TN_ROUTE_NONE, L.TN_ROUTE_W8, L.TN_ROUTE_P256, L.TN_ROUTE_X6_256x256,
                                                                  L.TN_ROUTE_X6_256x128, L.TN_ROUTE_X6_128x256)
KERNEL_NAMES = {K_NONE: "none", K_W8: "w8", K_P256: "p256", K_X6_256x256: "x6_256x256", K_X6_256x128: "x6_256x128",
                K_X6_128x256: "x6_128x256"}
RED_NONE, RED_LAUNCH, RED_CALLER = 0, 1, 2
E_BADARG, E_UNSUPPORTED, E_WORKSPACE = -1, -2, -4      # include/acx.h ACX_E_*
ZERO_B = 1024                                          # the zero page the 256 x 256 kernel clears behind its images when it owns it
NO_ROUTE = (K_NONE, 1, 0, 0, 0)


@dataclass
class Case:
    name: str
    M: int
    N1: int
    N2: int
    x6: bool = False                # acx_gemm_tn_x6 (bf16 planes) instead of acx_gemm_tn_zp / _parts
    pad_a: int = 0                  # lda = N1 + pad_a, ldb = (cin or N2) + pad_b: NaN pad columns
    pad_b: int = 0
    b_sub: bool = False
    conv: bool = False
    gn: int = 0
    gl: int = 0
    cin: int = 0
    ws: object = "full"             # "full": acx_gemm_tn_workspace_bytes / acx_gemm_tn_x6_workspace_bytes; "none"; or a byte count
    zp: bool = True                 # the caller brings a zero page (acx_gemm_tn_zp); False: acx_gemm_tn's NULL
    parts: bool = False             # acx_gemm_tn_parts
    opts: dict = field(default_factory=dict)     # context options the row needs (GPU: set on a context of the test's own)
    # what the query must answer: (kernel, splits, rows_per_split, tiles, reduce) under opts on 256 CUs; default_ctx: the same for a
    # NULL context where the options move it (None: no difference)
    expect: tuple = NO_ROUTE
    default_ctx: Optional[tuple] = None
    refuse: int = 0                 # ACX_E_* the query and the call must both answer (then `text` is in acx_last_error)
    text: str = ""
    raw: dict = field(default_factory=dict)      # refusals: arguments overwritten after filling (a broken call)
    call_only: bool = False         # a refusal of the real entry alone (pointer alignment: the query has no pointers)

    @property
    def kb(self):                   # columns of a row of B
        return self.cin if self.conv else self.N2

    @property
    def lda(self):
        return self.N1 + self.pad_a

    @property
    def ldb(self):
        return self.kb + self.pad_b

    @property
    def ws_bytes(self):
        if self.ws == "none":
            return 0
        if self.ws == "full":
            f = L.lib().acx_gemm_tn_x6_workspace_bytes if self.x6 else L.lib().acx_gemm_tn_workspace_bytes
            return int(f(self.M, self.N1, self.N2))
        return int(self.ws)

    @property
    def clears(self):               # the library owns the zero page: 1 KB behind the images
        return self.expect[0] == K_P256 and not self.zp

    @property
    def ws_need(self):              # the bytes of the workspace the route may write
        k, splits = self.expect[0], self.expect[1]
        return (splits * self.N1 * self.N2 * 4 if splits > 1 else 0) + (ZERO_B if self.clears else 0)

    @property
    def eps(self):
        return EPS_X6 if self.x6 else EPS


# ---------------------------------------------------------------------------------------------------------------- operands
def operands(c: Case, device="cpu"):
    """the operands of a case: values (CPU generator, so both test files see the same numbers) in poisoned, over-allocated buffers"""
    g = torch.Generator().manual_seed(c.M * 31 + c.N1 * 7 + c.N2 + 17 * c.cin + 3 * c.gl + c.pad_a)
    a = torch.randn(c.M, c.N1, generator=g) * torch.exp2(torch.randint(-3, 3, (c.M, 1), generator=g).float())
    b = torch.randn(c.M, c.kb, generator=g)
    t = {"b_sub": torch.randn(c.N2, generator=g).to(device) if c.b_sub else None}
    t["a_buf"], t["a"] = _padded(a.to(device), c.lda)
    t["b_buf"], t["b"] = _padded(b.to(device), c.ldb)
    t["c_buf"] = _poison(c.N1 + 2, c.N2, torch.float32, device)
    t["c"] = t["c_buf"][:c.N1]
    return t


# ---------------------------------------------------------------------------------------------------------------- reference
def tap_rows(c: Case, b, tap):
    """the rows of bmap(B) under one tap: B's row at the shifted grid position, zero outside the (gn, gl) grid"""
    m = torch.arange(c.M, device=b.device)
    per = c.gn * c.gl
    tile, rem = m // per, m % per
    n, l = rem // c.gl + (tap // 3 - 1), rem % c.gl + (tap % 3 - 1)
    inside = (n >= 0) & (n < c.gn) & (l >= 0) & (l < c.gl)
    src = (tile * per + n * c.gl + l).clamp(0, c.M - 1)
    return torch.where(inside.view(-1, 1), b[src], torch.zeros((), dtype=b.dtype, device=b.device))


def evaluate(c: Case, t, dtype=torch.float64, magnitude=False):
    """A^T (bmap(B) - b_sub) in `dtype`; magnitude: also S = |A|^T |bmap(B) - b_sub|"""
    a, b = t["a"].to(dtype), t["b"].to(dtype)
    at, aat = a.t().contiguous(), (a.abs().t().contiguous() if magnitude else None)
    if c.conv:
        out = torch.empty(c.N1, c.N2, dtype=dtype, device=a.device)
        mag = torch.empty_like(out) if magnitude else None
        for tap in range(9):                            # column order [tap][cin]
            x = tap_rows(c, b, tap)
            out[:, tap * c.cin:(tap + 1) * c.cin] = at @ x
            if magnitude:
                mag[:, tap * c.cin:(tap + 1) * c.cin] = aat @ x.abs()
    else:
        x = b - t["b_sub"].to(dtype) if c.b_sub else b
        out = at @ x
        mag = aat @ x.abs() if magnitude else None
    return (out, mag) if magnitude else out


def ref(c: Case, t):
    """(fp64 reference, S)"""
    return evaluate(c, t, torch.float64, magnitude=True)


def bound(c: Case, S):
    return c.eps * S


# ---------------------------------------------------------------------------------------------------------------- the query
def call_args(c: Case):
    """the integer arguments of the call, a refusal row's overwritten"""
    a = dict(M=c.M, N1=c.N1, N2=c.N2, lda=c.lda, ldb=c.ldb, ldc=c.N2, conv=int(c.conv), gn=c.gn, gl=c.gl, cin=c.cin,
             a_off=0, bsub_off=0, ws=c.ws_bytes, has_ws=c.ws != "none" and c.ws_bytes > 0, has_zp=c.zp)
    for k, v in c.raw.items():
        assert k in a, k
        a[k] = v
    return a


def query(h, c: Case):
    """acx_gemm_tn_route / acx_gemm_tn_x6_route -> (return code, (kernel, splits, rows_per_split, tiles, reduce), clears_zero_page)"""
    import ctypes as C
    out, a = L.GemmTnRoute(), call_args(c)
    if c.x6:
        rc = L.lib().acx_gemm_tn_x6_route(h, a["M"], a["N1"], a["N2"], a["lda"], a["ldb"], a["ldc"], a["conv"], a["gn"], a["gl"], a["cin"],
                                          int(a["has_ws"]), a["ws"], int(a["has_zp"]), C.byref(out))
    else:
        rc = L.lib().acx_gemm_tn_route(h, a["M"], a["N1"], a["N2"], a["lda"], a["ldb"], a["ldc"], int(c.b_sub), a["conv"], a["gn"], a["gl"],
                                       a["cin"], int(a["has_ws"]), a["ws"], int(a["has_zp"]), int(c.parts), C.byref(out))
    return rc, (out.kernel, out.splits, out.rows_per_split, out.tiles, out.reduce), out.clears_zero_page


# ---------------------------------------------------------------------------------------------------------------- the table
def _cases():
    out = []

    def add(name, M, N1, N2, expect, **kw):
        out.append(Case(name, M, N1, N2, expect=expect, **kw))

    # ---- gemm_tn_w8_kernel, identity rows: 128 x 128 tiles, splits of tn_choose_splits (rows per split a multiple of 32, >= 256
    # when split, no empty split)
    add("w8-1x4x4", 1, 4, 4, (K_W8, 1, 32, 1, 0))
    add("w8-31x4x132", 31, 4, 132, (K_W8, 1, 32, 2, 0))
    add("w8-33x132x4", 33, 132, 4, (K_W8, 1, 64, 2, 0))
    add("w8-255", 255, 128, 128, (K_W8, 1, 256, 1, 0))
    add("w8-256", 256, 128, 128, (K_W8, 1, 256, 1, 0))
    add("w8-256-no-workspace", 256, 128, 128, (K_W8, 1, 256, 1, 0), ws="none", zp=False)
    add("w8-511-split2", 511, 128, 128, (K_W8, 2, 256, 1, RED_LAUNCH))                 # 256 + 255
    add("w8-513-split2", 513, 128, 128, (K_W8, 2, 288, 1, RED_LAUNCH))                 # 288 + 225
    add("w8-700-split3", 700, 260, 124, (K_W8, 3, 256, 3, RED_LAUNCH))                 # both ragged: N1 % 128 = 4, N2 % 128 = 124
    add("w8-1037-split4", 1037, 36, 36, (K_W8, 4, 288, 1, RED_LAUNCH))                 # the last split: 173 rows
    add("w8-2000-split8", 2000, 64, 64, (K_W8, 8, 256, 1, RED_LAUNCH))
    add("w8-1000-split4", 1000, 16, 132, (K_W8, 4, 256, 2, RED_LAUNCH))
    add("w8-1000-split4-bsub", 1000, 16, 132, (K_W8, 4, 256, 2, RED_LAUNCH), b_sub=True)
    add("w8-31-bsub", 31, 4, 132, (K_W8, 1, 32, 2, 0), b_sub=True)
    add("w8-700-padded", 700, 260, 124, (K_W8, 3, 256, 3, RED_LAUNCH), pad_a=4, pad_b=12)
    add("w8-33-padded-bsub", 33, 132, 4, (K_W8, 1, 64, 2, 0), pad_a=8, pad_b=4, b_sub=True)
    add("w8-exact-workspace", 700, 260, 124, (K_W8, 3, 256, 3, RED_LAUNCH), ws=3 * 260 * 124 * 4, zp=False)
    # the 256 x 256 kernel's shape, withheld by the option: 17 splits of 256 rows, the last with 4
    add("w8-p256-withheld", 4100, 196, 1800, (K_W8, 17, 256, 30, RED_LAUNCH), opts={L.OPT_TN_P256_MIN_ROWS: 1 << 30},
        default_ctx=(K_P256, 8, 544, 8, RED_LAUNCH))
    # one below each gate of tn_takes_p256 (the other side: the p256 rows below)
    add("w8-rows-4095", 4095, 256, 2048, (K_W8, 16, 256, 32, RED_LAUNCH))
    add("w8-n1-188", 4096, 188, 2048, (K_W8, 16, 256, 32, RED_LAUNCH))
    add("w8-n2-1792-7-tiles", 4096, 256, 1792, (K_W8, 16, 256, 28, RED_LAUNCH))
    add("w8-n2-252", 4096, 2048, 252, (K_W8, 16, 256, 32, RED_LAUNCH))
    add("w8-p256-shape-bsub", 4096, 256, 2048, (K_W8, 16, 256, 32, RED_LAUNCH), b_sub=True)
    add("w8-p256-shape-no-workspace-refused", 4096, 256, 2048, NO_ROUTE, ws="none", refuse=E_WORKSPACE, text="workspace too small")

    # ---- gemm_tn_w8_kernel, the 3 x 3 convolution's row map, its three branches; M = tiles gn gl, so splits cut grid tiles in two
    def conv(name, grid, cin, tiles, N1, expect, **kw):
        add(name, tiles * grid[0] * grid[1], N1, 9 * cin, expect, conv=True, gn=grid[0], gl=grid[1], cin=cin, **kw)

    conv("w8c-fast-32x16-cin4", (32, 16), 4, 1, 128, (K_W8, 2, 256, 1, RED_LAUNCH))            # 9 taps' chunks in one tile
    conv("w8c-fast-8x4-cin36", (8, 4), 36, 40, 36, (K_W8, 5, 256, 3, RED_LAUNCH))              # taps straddle the 128-column tiles
    conv("w8c-fast-2x4", (2, 4), 4, 5, 4, (K_W8, 1, 64, 1, 0))                                 # the grid smaller than a K-step
    conv("w8c-fast-1x1", (1, 1), 4, 100, 132, (K_W8, 1, 128, 2, 0))                            # only the centre tap is inside
    conv("w8c-fast-8x16", (8, 16), 8, 6, 36, (K_W8, 3, 256, 1, RED_LAUNCH))                    # gl = 16: the fast branch's last width
    conv("w8c-shift-8x32", (8, 32), 32, 4, 128, (K_W8, 4, 256, 3, RED_LAUNCH))                 # gl = 32: shifts, not the fast branch
    conv("w8c-shift-16x32-cin8", (16, 32), 8, 2, 36, (K_W8, 4, 256, 1, RED_LAUNCH))
    conv("w8c-div-24x10-cin8", (24, 10), 8, 3, 36, (K_W8, 3, 256, 1, RED_LAUNCH))              # not powers of two: division
    conv("w8c-div-24x10-cin36", (24, 10), 36, 5, 128, (K_W8, 5, 256, 3, RED_LAUNCH))
    conv("w8c-div-3x5", (3, 5), 4, 50, 132, (K_W8, 3, 256, 2, RED_LAUNCH))
    conv("w8c-div-24x16", (24, 16), 16, 2, 128, (K_W8, 3, 256, 2, RED_LAUNCH))                 # gl a power of two, the grid not
    conv("w8c-div-24x10-padded", (24, 10), 8, 3, 36, (K_W8, 3, 256, 1, RED_LAUNCH), pad_a=4, pad_b=8)

    # ---- gemm_tn_p256_kernel: N1 >= 192, N2 >= 256, M >= 4096, >= 8 tiles of 256 x 256, no b_sub, a workspace; splits = 256 CUs /
    # tiles while a split keeps >= 512 rows, fewer when the workspace is short
    add("p256-4096x256x2048", 4096, 256, 2048, (K_P256, 8, 512, 8, RED_LAUNCH))
    add("p256-4096x512x1024", 4096, 512, 1024, (K_P256, 8, 512, 8, RED_LAUNCH))
    add("p256-n1-192", 4096, 192, 2048, (K_P256, 8, 512, 8, RED_LAUNCH))
    add("p256-n2-256", 4096, 2048, 256, (K_P256, 8, 512, 8, RED_LAUNCH))
    add("p256-ragged", 4100, 196, 1800, (K_P256, 8, 544, 8, RED_LAUNCH))                # the last K-step of the last split: 4 rows
    add("p256-n2-1796-8-tiles", 4096, 256, 1796, (K_P256, 8, 512, 8, RED_LAUNCH))
    add("p256-5000x260x1540", 5000, 260, 1540, (K_P256, 9, 576, 14, RED_LAUNCH))
    add("p256-empty-split", 16400, 256, 2048, (K_P256, 32, 544, 8, RED_LAUNCH))         # 31 x 544 = 16864 > M: split 31 has no rows
    add("p256-ragged-padded", 4100, 196, 1800, (K_P256, 8, 544, 8, RED_LAUNCH), pad_a=4, pad_b=8)
    add("p256-ragged-own-zero-page", 4100, 196, 1800, (K_P256, 8, 544, 8, RED_LAUNCH), zp=False)
    add("p256-three-images", 4100, 196, 1800, (K_P256, 3, 1376, 8, RED_LAUNCH), ws=3 * 196 * 1800 * 4 + ZERO_B, zp=False)
    add("p256-three-images-less-1", 4100, 196, 1800, (K_P256, 2, 2080, 8, RED_LAUNCH), ws=3 * 196 * 1800 * 4 + ZERO_B - 16, zp=False)
    add("p256-one-image-own-zero-page", 4100, 196, 1800, (K_P256, 1, 4128, 8, 0), ws=196 * 1800 * 4 + ZERO_B, zp=False)
    add("p256-512-bytes-callers-zero-page", 4096, 256, 2048, (K_P256, 1, 4096, 8, 0), ws=512)
    add("p256-512-bytes-w8-refused", 4096, 256, 2048, NO_ROUTE, ws=512, zp=False, refuse=E_WORKSPACE, text="workspace too small")
    add("p256-min-rows-4097-w8", 4096, 256, 2048, (K_W8, 16, 256, 32, RED_LAUNCH), opts={L.OPT_TN_P256_MIN_ROWS: 4097},
        default_ctx=(K_P256, 8, 512, 8, RED_LAUNCH))

    # ---- ... and its convolution row map: shifts and division, taps from the zero page
    conv("p256c-div-24x10-cin228", (24, 10), 228, 18, 256, (K_P256, 8, 544, 9, RED_LAUNCH))    # N2 = 2052: tap edges off the tile edges
    conv("p256c-shift-32x16", (32, 16), 256, 8, 256, (K_P256, 8, 512, 9, RED_LAUNCH))
    conv("p256c-shift-8x32-n1-196", (8, 32), 256, 16, 196, (K_P256, 8, 512, 9, RED_LAUNCH))
    conv("p256c-1x1", (1, 1), 512, 4096, 256, (K_P256, 8, 512, 18, RED_LAUNCH))
    conv("p256c-div-24x10-own-zero-page", (24, 10), 228, 18, 256, (K_P256, 8, 544, 9, RED_LAUNCH), zp=False)

    # ---- acx_gemm_tn_parts: the images stay (test_gpu_tn_routes.py sums them in image order against _zp)
    add("parts-w8-bsub", 1000, 16, 132, (K_W8, 4, 256, 2, RED_CALLER), b_sub=True, parts=True)
    add("parts-w8-unsplit", 256, 128, 128, (K_W8, 1, 256, 1, 0), parts=True)
    add("parts-p256", 4096, 256, 2048, (K_P256, 8, 512, 8, RED_CALLER), parts=True)

    # ---- acx_gemm_tn_x6: the plane kernel's three tile geometries (tn_x6_mode), plain and convolution, K-steps of 32 rows split by
    # x6_choose_split (pieces of >= 8 K-steps that fit the workspace)
    def x6(name, M, N1, N2, expect, **kw):
        add(name, M, N1, N2, expect, x6=True, **kw)

    def x6c(name, grid, cin, tiles, N1, expect, **kw):
        conv(name, grid, cin, tiles, N1, expect, x6=True, **kw)

    for kern, N1, N2 in ((K_X6_256x256, 256, 256), (K_X6_256x128, 256, 128), (K_X6_128x256, 128, 256)):
        nm = KERNEL_NAMES[kern]
        x6(f"{nm}-m1", 1, N1, N2, (kern, 1, 32, 1, 0))
        x6(f"{nm}-m33", 33, N1, N2, (kern, 1, 64, 1, 0))
        x6(f"{nm}-m1000", 1000, N1, N2, (kern, 4, 256, 1, RED_LAUNCH))                         # 32 K-steps as 4 x 8
    x6("x6_256x256-m1000-no-workspace", 1000, 256, 256, (K_X6_256x256, 1, 1024, 1, 0), ws="none")
    x6("x6_256x256-m1000-two-images", 1000, 256, 256, (K_X6_256x256, 2, 512, 1, RED_LAUNCH), ws=2 * 256 * 256 * 4)
    x6("x6_256x256-m1000-two-images-less-1", 1000, 256, 256, (K_X6_256x256, 1, 1024, 1, 0), ws=2 * 256 * 256 * 4 - 16)
    x6("x6_256x256-m1000-padded", 1000, 256, 256, (K_X6_256x256, 4, 256, 1, RED_LAUNCH), pad_a=8, pad_b=16)
    x6("x6_256x256-4-tiles", 1000, 512, 512, (K_X6_256x256, 4, 256, 4, RED_LAUNCH))
    x6("x6_256x128-padded-6-tiles", 33, 512, 384, (K_X6_256x128, 1, 64, 6, 0), pad_a=8, pad_b=8)
    x6("x6_128x256-6-tiles", 1000, 384, 512, (K_X6_128x256, 4, 256, 6, RED_LAUNCH))
    x6("x6_256x256-37-cus", 4096, 512, 512, (K_X6_256x256, 9, 480, 4, RED_LAUNCH), opts={L.OPT_X6_CUS: 37},
       default_ctx=(K_X6_256x256, 16, 256, 4, RED_LAUNCH))
    x6c("x6c_256x256-4x4", (4, 4), 256, 63, 256, (K_X6_256x256, 4, 256, 9, RED_LAUNCH))        # M = 1008: 32 K-steps, the last 16 rows
    x6c("x6c_256x256-8x32", (8, 32), 256, 4, 256, (K_X6_256x256, 4, 256, 9, RED_LAUNCH))       # gl = 32
    x6c("x6c_256x256-1x1", (1, 1), 256, 33, 256, (K_X6_256x256, 1, 64, 9, 0))                  # only the centre tap is inside
    x6c("x6c_256x256-8x32-37-cus", (8, 32), 256, 8, 256, (K_X6_256x256, 4, 512, 9, RED_LAUNCH), opts={L.OPT_X6_CUS: 37},
        default_ctx=(K_X6_256x256, 8, 256, 9, RED_LAUNCH))
    x6c("x6c_256x128-4x4", (4, 4), 128, 63, 256, (K_X6_256x128, 4, 256, 9, RED_LAUNCH))        # cin = 128: a 128-column tile per tap
    x6c("x6c_256x128-8x32", (8, 32), 128, 1, 256, (K_X6_256x128, 1, 256, 9, 0))
    x6c("x6c_256x128-1x1-padded", (1, 1), 128, 1000, 256, (K_X6_256x128, 4, 256, 9, RED_LAUNCH), pad_a=8, pad_b=8)
    x6c("x6c_128x256-8x32", (8, 32), 256, 4, 128, (K_X6_128x256, 4, 256, 9, RED_LAUNCH))
    x6c("x6c_128x256-4x4", (4, 4), 256, 1, 128, (K_X6_128x256, 1, 32, 9, 0))
    x6c("x6c_128x256-1x1-no-workspace", (1, 1), 256, 1000, 128, (K_X6_128x256, 1, 1024, 9, 0), ws="none")

    # ---- refusals: the query and the call answer the same code and text
    T_ALIGN, T_CONV = "must be multiples of 4, C dense, 16-byte aligned", "bad conv geometry"

    def refuse(name, code, text, M=700, N1=260, N2=124, **kw):
        out.append(Case(name, M, N1, N2, refuse=code, text=text, **kw))

    cv = dict(conv=True, gn=24, gl=10, cin=8)
    refuse("n1-mod4", E_BADARG, T_ALIGN, raw=dict(N1=258))
    refuse("lda-mod4", E_BADARG, T_ALIGN, raw=dict(lda=262))
    refuse("ldc-not-n2", E_BADARG, T_ALIGN, raw=dict(ldc=128))
    refuse("a-misaligned", E_BADARG, T_ALIGN, raw=dict(a_off=4), call_only=True)
    refuse("bsub-misaligned", E_BADARG, "b_sub alignment", b_sub=True, raw=dict(bsub_off=4), call_only=True)
    refuse("conv-n2-not-9cin", E_BADARG, T_CONV, M=720, N1=36, N2=72, raw=dict(N2=76, ldc=76), **cv)
    # (cin % 4 != 0 with N2 == 9 cin cannot pass N2 % 4 == 0: the clause is implied; the nearest call answers through N2 != 9 cin)
    refuse("conv-cin-mod4", E_BADARG, T_CONV, M=720, N1=36, N2=72, raw=dict(cin=6, N2=56, ldc=56), **cv)
    refuse("conv-rows-not-whole-tiles", E_BADARG, T_CONV, M=720, N1=36, N2=72, raw=dict(M=716), **cv)
    refuse("w8-workspace-two-of-three-images", E_WORKSPACE, "workspace too small", ws=2 * 260 * 124 * 4)
    refuse("w8-workspace-withheld", E_WORKSPACE, "workspace too small", ws="none")
    T_X6 = "acx_gemm_tn_x6: N1 a multiple of 256 and N2 of 128, or N1 of 128 and N2 of 256"
    refuse("x6-128x128", E_UNSUPPORTED, T_X6, M=1000, N1=128, N2=128, x6=True)
    refuse("x6-lda-mod8", E_UNSUPPORTED, T_X6, M=1000, N1=256, N2=256, x6=True, raw=dict(lda=260))
    refuse("x6-conv-24x10", E_UNSUPPORTED, "conv needs N2 == 9 cin, a power-of-two grid, whole tiles", M=720, N1=256, N2=2304, x6=True,
           conv=True, gn=24, gl=10, cin=256)
    refuse("x6-no-zero-page", E_BADARG, "the zero page is required", M=1000, N1=256, N2=256, x6=True, zp=False)
    # cin = 128 makes N2 = 9 cin no multiple of 256; with N2 a multiple of 256 and N1 = 128 the 128 x 256 geometry wants cin % 256 == 0
    refuse("x6-conv-cin128-n1-128", E_UNSUPPORTED, T_X6, M=1024, N1=128, N2=1152, x6=True, conv=True, gn=8, gl=32, cin=128,
           raw=dict(N2=2304, ldc=2304))
    return out


CASES = _cases()
assert len({c.name for c in CASES}) == len(CASES)
RUN_CASES = [c for c in CASES if not c.refuse]
REFUSALS = [c for c in CASES if c.refuse]

# acx_gemm_tn_group: ten of the identity-row rows above (two launches of at most eight): both ragged ones, two with b_sub, padded
# leading dimensions, unsplit and split
GROUP = ["w8-31x4x132", "w8-33x132x4", "w8-700-split3", "w8-1000-split4-bsub", "w8-31-bsub", "w8-700-padded", "w8-256", "w8-513-split2",
         "w8-1037-split4", "w8-2000-split8"]


def by_name(name):
    return next(c for c in CASES if c.name == name)
