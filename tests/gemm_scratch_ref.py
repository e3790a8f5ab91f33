"""Test infrastructure for acx_gemm_scratch: the scratch rules of acx_gemm's callers as the Python wrapper evaluated them before the
library answered the question itself -- FROZEN.  ops.gemm and ops.gemm_x6 sized the split-K workspace and decided about the
arrival counters with these formulas; the library chooses its K split from the workspace size it is handed, so the formulas fix
the summation order of real products.  acx_gemm_scratch must give the same answer for every descriptor the wrapper can build
(tests/test_cpu_gemm_scratch.py, tests/test_gpu_gemm_scratch.py).

scratch_ref(d, ncu, ...) reads the fields of an acx_gemm_desc (any object with those attributes; pointers are tested for None / 0
only) and returns (workspace bytes, counters): bytes == 0 means no workspace, counters == 1 the caller's arrival-counter table.
split_k is ops.gemm_x6's argument; ops.gemm had none (always True) -- a caller that allows no split brings nothing.

desc(...) fills a descriptor with dummy operand pointers for the query, and the grids below are the shapes both test files ask
about: every rule, both sides of every threshold."""

PREC_F32, PREC_BF16 = 0, 1                            # == include/acx.h ACX_PREC_*
ACX_F32, ACX_BF16 = 0, 1
ACT_NONE, ACT_LEAKYRELU = 0, 2
AMAP_IDENTITY, AMAP_CONV3X3, AMAP_TESTTILE, AMAP_TILETABLE = 0, 1, 2, 3


def x6_workgroups(ncu, x6_cus):
    """workgroups of the persistent plane kernels: the CU count, or ACX_OPT_X6_CUS when that is lower"""
    return min(ncu, x6_cus) if x6_cus > 0 else ncu


def scratch_ref(d, ncu=256, sk_max_m=320, x6_cus=0, tail_split=False, split_k=True):
    if d.pairs in (6, 3):
        return _x6(d, x6_workgroups(ncu, x6_cus), bool(tail_split), bool(split_k))
    return _plain(d, sk_max_m) if split_k else (0, 0)


def _x6(d, wgs, tail_split, split_k):
    """ops.gemm_x6 (pairs = 6 / 3): the whole-problem K split of launches with fewer tiles than workgroups, else -- opt-in -- the K
    split of a partly filled last round of tiles"""
    M, N, K, amap, gn, gl = d.M, d.N, d.K, d.amap, d.gn, d.gl
    tm, tn = (M + 255) // 256, (N + 255) // 256
    tiles = tm * tn
    if split_k and tiles < wgs and K >= 384:
        return min(16, max(2, 2 * wgs // tiles)) * M * N * 4, 0
    if split_k and tail_split and amap in (AMAP_IDENTITY, AMAP_CONV3X3) and K >= 384 and tiles % wgs:
        tail_rows = M - min(M, (tiles // wgs * wgs) // tn * 256)
        if amap == AMAP_CONV3X3 and (gn * gl) % 256 == 0:      # (the tail begins at a token-grid boundary)
            gt = gn * gl // 256
            tail_rows = M - min(M, ((tiles // wgs * wgs) // tn) // gt * gt * 256)
        if tail_rows > 0:
            return min(8, max(4, 2 * wgs // max(1, (tail_rows + 255) // 256 * tn))) * tail_rows * N * 4, 0
    return 0, 0


def _plain(d, sk_max_m):
    """ops.gemm: the K split of the 128 x 128 / 64 x 64 tile kernels (with the counters for the f32 convolutions), else the piece
    split of the few-row kernel at long K"""
    M, N, K, amap, prec, act = d.M, d.N, d.K, d.amap, d.prec, d.act
    a_sub, pos0 = bool(d.a_sub), bool(d.pos0)
    nbytes, counters = 0, 0
    tiles = ((M + 127) // 128) * ((N + 127) // 128)
    few_rows = ((M <= sk_max_m or (N <= 512 and M <= 4 * sk_max_m and not (M > 768 and K >= 1536)))
                and K % 256 == 0 and prec == PREC_F32
                and amap == AMAP_IDENTITY and not a_sub and not pos0
                and act != ACT_LEAKYRELU)
    generic_f32 = (a_sub or pos0 or amap in (AMAP_TESTTILE, AMAP_TILETABLE)) and prec == PREC_F32 \
        and d.a_dtype == ACX_F32 and d.c_dtype == ACX_F32
    if ((tiles <= 128 and K >= 256 or tiles <= 256 and K >= 1024) and not few_rows
            and ((amap in (AMAP_IDENTITY, AMAP_CONV3X3) and not a_sub and not pos0) or generic_f32)):
        nbytes = min(16, 512 // tiles) * M * N * 4
        if amap == AMAP_CONV3X3 and prec == PREC_F32:
            counters = 1
    if few_rows and K >= 1024 and K % 512 == 0 and ((M + 31) // 32) * ((N + 31) // 32) * (K // 512) <= 512:
        tiles32 = ((M + 31) // 32) * ((N + 31) // 32)
        nbytes, counters = (K // 512) * tiles32 * 4096, 1
    return nbytes, counters


_PTR = 0x10000                                        # a dummy, 16-byte aligned operand address: the query dereferences nothing


def desc(M, N, K, *, prec=PREC_F32, act=ACT_NONE, amap=AMAP_IDENTITY, gn=0, gl=0, cin=0, seg=0, pairs=0, a_sub=False, pos=False,
         residual=False, tile_table=False, c_dtype=None):
    """an acx_gemm_desc as ops.gemm (pairs = 0) / ops.gemm_x6 (pairs = 6 / 3) fill it, operands at dummy addresses"""
    from anomalyclip_amd import _lib as L
    d = L.GemmDesc()
    d.A, d.W, d.C = _PTR, 2 * _PTR, 3 * _PTR
    d.M, d.N, d.K = M, N, K
    Ka = cin if amap == AMAP_CONV3X3 else K
    d.lda, d.ldw, d.ldc = Ka, K, N
    d.prec = PREC_BF16 if pairs else prec
    d.a_dtype = ACX_BF16 if d.prec == PREC_BF16 else ACX_F32
    d.c_dtype = ACX_F32 if c_dtype is None else c_dtype
    d.act, d.amap, d.gn, d.gl, d.cin, d.seg = act, amap, gn, gl, cin, seg
    if residual:
        d.residual, d.ldr = 4 * _PTR, N
    if a_sub:
        d.a_sub = 5 * _PTR
    if pos:
        d.pos0, d.pos1 = 6 * _PTR, 7 * _PTR
    if tile_table:
        d.tile_table = 8 * _PTR
    if amap == AMAP_CONV3X3:
        d.zero_page = 9 * _PTR
    if pairs:
        d.pairs, d.a_plane_stride, d.w_plane_stride = pairs, M * Ka * 2, N * K * 2
    return d


# f32 identity rows (M, N, K): the text tower's few-row shapes with short and long K, the narrow-output rows up to 4 x the row limit
# with the long-K exception above 768 rows, the row limit itself, 128 / 256 tiles of 128 x 128 at K = 256 / 768 / 1024, past both
F32_SHAPES = [(77, 512, 512), (77, 512, 2048), (77, 2048, 512), (539, 512, 2048), (1078, 512, 2048), (1078, 512, 1024),
              (320, 768, 768), (321, 768, 768), (1280, 512, 768), (1281, 512, 768), (2048, 1024, 256), (2048, 2048, 1024),
              (2048, 2048, 768), (4096, 2048, 1024),
              # the other side of each threshold: 129 / 257 tiles, K just below 256 / 1024, 512 / 576 piece workgroups, K = 1536 at
              # 768 / 769 rows and K = 1280 at 769, N = 516 at 1078 rows, a few-row product too wide for the piece split
              (2049, 1024, 256), (2049, 2048, 1024), (2048, 1024, 252), (2048, 2048, 1020), (256, 512, 2048), (257, 512, 2048),
              (768, 512, 1536), (769, 512, 1536), (769, 512, 1280), (1078, 516, 1024), (77, 2048, 2048), (77, 512, 1536)]
_GRID = dict(gn=32, gl=16)


def f32_cases():
    """[(name, descriptor keyword arguments)] of the ops.gemm descriptors"""
    out = [(f"f32-{M}x{N}x{K}", dict(M=M, N=N, K=K)) for M, N, K in F32_SHAPES]
    out += [(f"bf16-{M}x{N}x{K}", dict(M=M, N=N, K=K, prec=PREC_BF16)) for M, N, K in F32_SHAPES]
    out += [("f32-k1120", dict(M=200, N=512, K=1120)), ("f32-n510", dict(M=77, N=510, K=2048)),
            ("f32-leaky", dict(M=77, N=512, K=2048, act=ACT_LEAKYRELU)), ("f32-leaky-tiles", dict(M=2048, N=1024, K=512, act=ACT_LEAKYRELU)),
            ("f32-asub", dict(M=2048, N=512, K=512, a_sub=True)), ("f32-asub-few", dict(M=77, N=512, K=2048, a_sub=True)),
            ("f32-asub-bf16out", dict(M=2048, N=512, K=512, a_sub=True, c_dtype=ACX_BF16)),
            ("bf16-asub", dict(M=2048, N=512, K=512, a_sub=True, prec=PREC_BF16)),
            ("f32-pos", dict(M=4096, N=512, K=512, pos=True, **_GRID)),
            ("f32-testtile", dict(M=4096, N=512, K=512, amap=AMAP_TESTTILE, seg=2, **_GRID)),
            ("f32-tiletable", dict(M=4096, N=512, K=512, amap=AMAP_TILETABLE, tile_table=True, **_GRID)),
            ("f32-tiletable-many", dict(M=8192, N=2048, K=512, amap=AMAP_TILETABLE, tile_table=True, **_GRID))]
    for M in (256, 4096):
        for N in (64, 512):
            out.append((f"f32-conv-{M}x{N}", dict(M=M, N=N, K=288, amap=AMAP_CONV3X3, gn=16, gl=16, cin=32)))
            out.append((f"bf16-conv-{M}x{N}", dict(M=M, N=N, K=576, amap=AMAP_CONV3X3, gn=16, gl=16, cin=64, prec=PREC_BF16)))
    out.append(("f32-conv-bf16out", dict(M=4096, N=512, K=288, amap=AMAP_CONV3X3, gn=16, gl=16, cin=32, c_dtype=ACX_BF16)))
    return out


# pairs = 6 / 3, identity rows: one tile row (K = 768 and the K = 352 that is too short to split), 255 / 258 / 100 tiles around the
# 256 workgroups, whole rounds (768 tiles), the ViT's 256- and 512-frame products with a partly filled last round
X6_SHAPES = [(256, 768, 768), (256, 768, 352), (65536, 768, 768), (50432, 768, 768), (100864, 768, 3072),
             (21760, 768, 768), (22016, 768, 768), (6400, 1024, 768), (256, 768, 384)]


def x6_cases():
    """[(name, descriptor keyword arguments)] of the ops.gemm_x6 descriptors: both pairs values, with and without the residual of
    the acx_gemm_ln form, the convolutions on a 16 x 16 grid (one tile) and on a 16 x 8 grid (half a tile)"""
    out = []
    for pairs in (6, 3):
        for M, N, K in X6_SHAPES:
            out.append((f"x{pairs}-{M}x{N}x{K}", dict(M=M, N=N, K=K, pairs=pairs)))
            out.append((f"x{pairs}-ln-{M}x{N}x{K}", dict(M=M, N=N, K=K, pairs=pairs, residual=True)))
    for M in (256, 65536 + 256 * 79):
        for N in (128, 512):
            out.append((f"x6-conv-{M}x{N}", dict(M=M, N=N, K=576, pairs=6, amap=AMAP_CONV3X3, gn=16, gl=16, cin=64)))
    out.append(("x6-conv-halftile-grid", dict(M=65536 + 256 * 79, N=512, K=576, pairs=6, amap=AMAP_CONV3X3, gn=16, gl=8, cin=64)))
    out.append(("x6-conv-4tile-grid", dict(M=65536 + 1024 * 20, N=512, K=576, pairs=6, amap=AMAP_CONV3X3, gn=32, gl=32, cin=64)))
    return out
