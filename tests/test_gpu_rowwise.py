"""-m gpu: the row-wise kernels at every width the dispatch takes and in every rows-per-wave regime, element by element against the
fp64 closed forms of rowwise_ref with the bound 2e-6 * S (S = the sum of the absolute values of the terms of the element), on
inputs whose rows differ in scale by up to 2^12 -- LayerNorm / ChanLayerNorm forward and backward, the classifier head forward and
backward, acx_vit_embed -- and the small gradient and data-movement launches of the training step (pos_grad, ctx_grad,
gather / scatter_rows, prompt_embed, add_bcast, leaky_grad_planes, multi_axpy_, transpose) against torch, bit for bit where the
arithmetic is exact.  Every comparison prints its worst |err| / S before it asserts (pytest -s; DESIGN.md section 3 records them).

Rows-per-wave regimes of the two backward kernels (acx_rows_per_wave): 1 below 4096 rows, 2 below 8192, 4 below 16384, 8 below
32768, 16 from there.  4101 rows = 512 full blocks of 8 rows + one of 5: its waves walk 2, 2, 1 (the `break`) and 0 rows (an
all-zero partial); 8195, 16393 and 32785 leave 3, 9 and 17 rows to the last block in the same way."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops
from oracle import anomalyclip_oracle as O
import rowwise_ref as RR

DEV = "cuda"
MODES = [L.NORM_LAYER, L.NORM_CHAN]
DEEP_ROWS = [8195, 16393, 32785]          # rows per wave 4, 8, 16, each with a ragged last block


def _d(*ts):
    return [t.to(DEV) for t in ts]


# =============================================================================================================== LayerNorm forward
@pytest.mark.parametrize("D", RR.WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_layernorm_fwd_every_width(D, mode):
    """f32 output within 2e-6 * S_y, bf16 output within 2^-8 |ref| on top of it; one, five (a row count that is no multiple of the
    four rows of a block) and 777 rows; a source with a row stride above D; a zero-variance row."""
    for rows in (1, 5, 777):
        x, w, b, _, _ = RR.ln_inputs(rows, D, seed=11 * D + mode + rows)
        ref, S = RR.ln_fwd(x, w, b, mode)
        xd, wd, bd = _d(x, w, b)
        out = ops.layernorm(xd, wd, bd, mode=mode)
        assert out.shape == (rows, D) and RR.within(out, ref, S, f"y D={D} mode={mode} rows={rows}", "ln_fwd")
        outb = ops.layernorm(xd, wd, bd, mode=mode, out_dtype=torch.bfloat16)
        assert outb.dtype == torch.bfloat16
        assert bool(((outb.double().cpu() - ref).abs() <= 2.0 ** -8 * ref.abs() + RR.TOL * S).all())
        # rows of a wider buffer (ldx = D + 8): the pad columns hold other values and are not read
        wide = torch.full((rows, D + 8), 1e3)
        wide[:, :D] = x
        outw = ops.layernorm(wide.to(DEV), wd, bd, mode=mode, rows=rows, ldx=D + 8)
        assert torch.equal(outw, out)
    if mode == L.NORM_LAYER:
        # zero-variance rows: v == 0 gives y == b to the rounding of b alone.  v is exactly 0 for a row of zeros at every width, and
        # for a row of 0.5 where 1 / D is a power of two; at 640 and 768 the kernel's x - sum * fl(1 / D) (one fused multiply-add) keeps
        # the rounding of 1 / D, 2^-26 * 0.5, which 1 / sqrt(eps) = 316 amplifies: that row is held to the general bound there
        x, w, b, _, _ = RR.ln_inputs(5, D, seed=D)
        x[2], x[3] = 0.5, 0.0
        ref, S = RR.ln_fwd(x, w, b, mode)
        out = ops.layernorm(*_d(x, w, b), mode=mode)
        assert RR.within(out, ref, S, f"y D={D} zero-variance rows", "ln_fwd")
        for r in (2, 3) if D & (D - 1) == 0 else (3,):
            assert bool(((out[r].double().cpu() - b.double()).abs() <= RR.TOL * b.double().abs()).all()), r


# =============================================================================================================== LayerNorm backward
def _ln_bwd_case(D, mode, rows):
    x, w, _, dy, add = RR.ln_inputs(rows, D, seed=7 * D + mode + rows)
    ref = RR.ln_bwd(x, w, dy, mode)
    xd, wd, dyd, addd = _d(x, w, dy, add)
    tag = f"D={D} mode={mode} rows={rows}"
    dx, dw, db = ops.layernorm_bwd(xd, wd, dyd, mode=mode)
    for k, out in (("dx", dx), ("dw", dw), ("db", db)):
        assert RR.within(out, *ref[k], f"{k} {tag}", "ln_bwd"), k
    # the two partial calls: same arithmetic per row whatever the rows-per-wave mapping, same partials with or without the dx store
    dx1, dw1, db1 = ops.layernorm_bwd(xd, wd, dyd, mode=mode, need_params=False)
    assert dw1 is None and db1 is None and torch.equal(dx1, dx)
    dx2, dw2, db2 = ops.layernorm_bwd(xd, wd, dyd, mode=mode, need_dx=False)
    assert dx2 is None and torch.equal(dw2, dw) and torch.equal(db2, db)
    # the residual branch and the scale folded into the pass
    ref_dx, s_dx = ref["dx"]
    dxa, _, _ = ops.layernorm_bwd(xd, wd, dyd, mode=mode, add=addd)
    assert RR.within(dxa, add.double() + ref_dx, add.double().abs() + s_dx, f"add+dx {tag}", "ln_bwd")
    dxh, _, _ = ops.layernorm_bwd(xd, wd, dyd, mode=mode, dx_scale=0.5)
    assert torch.equal(dxh, 0.5 * dx)                                # a power of two: the scaling is exact
    sc = float(np.float32(0.3))                                      # (the C ABI takes a float)
    dxs, dws, dbs = ops.layernorm_bwd(xd, wd, dyd, mode=mode, dx_scale=0.3, add=addd)
    assert RR.within(dxs, add.double() + sc * ref_dx, add.double().abs() + sc * s_dx, f"add+0.3dx {tag}", "ln_bwd")
    assert torch.equal(dws, dw) and torch.equal(dbs, db)             # the parameter gradients do not see dx_scale / add
    # what the step graph calls: the partials left to the caller, fixed order, run-to-run identical
    dxp, part = ops.layernorm_bwd_parts(xd, wd, dyd, mode=mode)
    assert part.shape == (ops.row_parts(rows), 2 * D) and torch.equal(dxp, dx)
    assert torch.equal(ops.reduce_rows(part), torch.cat([dw, db]))
    dxq, part2 = ops.layernorm_bwd_parts(xd, wd, dyd, mode=mode)
    assert torch.equal(dxq, dxp) and torch.equal(part2, part)
    dxr, part3 = ops.layernorm_bwd_parts(xd, wd, dyd, mode=mode, dx_scale=0.3, add=addd)
    assert torch.equal(dxr, dxs) and torch.equal(part3, part)


@pytest.mark.parametrize("rows", [1, 3, 777, 4101])
@pytest.mark.parametrize("D", RR.WIDTHS)
@pytest.mark.parametrize("mode", MODES)
def test_layernorm_bwd_every_width(D, mode, rows):
    """every width (float4 rows with the permuted element layout: 256, 512, 768, 1024; scalar rows: 64, 128, 640) at one row, three
    rows (one block, one idle wave), 777 rows (one row per wave) and 4101 (two rows per wave, ragged last block)"""
    _ln_bwd_case(D, mode, rows)


@pytest.mark.parametrize("rows", DEEP_ROWS)
@pytest.mark.parametrize("D", [64, 256, 640])
@pytest.mark.parametrize("mode", MODES)
def test_layernorm_bwd_deeper_row_regimes(D, mode, rows):
    """4, 8 and 16 rows per wave; the row loop does not depend on the width: one float4 width and both kinds of scalar ones"""
    _ln_bwd_case(D, mode, rows)


@pytest.mark.parametrize("D", [64, 256])
@pytest.mark.parametrize("mode", MODES)
def test_layernorm_bwd_zero_variance_row(D, mode):
    """a constant row among normal rows.  LAYER: the closed form holds there as everywhere.  CHAN: 1 / std does not exist, the
    kernel drops that term -- the row must come out finite, the other rows and the parameter gradients keep their bound."""
    rows, z = 9, 4
    x, w, _, dy, _ = RR.ln_inputs(rows, D, seed=D + mode)
    x[z] = 0.5
    ref = RR.ln_bwd(x, w, dy, mode)
    dx, dw, db = ops.layernorm_bwd(*_d(x, w, dy), mode=mode)
    assert bool(torch.isfinite(dx).all())
    keep = torch.arange(rows) != z if mode == L.NORM_CHAN else torch.ones(rows, dtype=torch.bool)
    assert RR.within(dx.cpu()[keep], ref["dx"][0][keep], ref["dx"][1][keep], f"dx D={D} mode={mode} zero-variance", "ln_bwd")
    assert RR.within(dw, *ref["dw"]) and RR.within(db, *ref["db"])


# =============================================================================================================== classifier head
def _scores_ok(out, ref, bound, what):
    err = (out.double().cpu() - ref).abs()
    print(f"ROWWISE_RATIO head_fwd {what} {float((err / bound).max()) * RR.TOL:.3e}")
    return bool((err <= bound).all())


@pytest.mark.parametrize("E", RR.WIDTHS)
def test_cls_head_fwd_every_width(E):
    """270 rows (no multiple of the four rows of a block) on a (6, 5) grid: plain order, and the inverse test-mode tiling of the
    store for segment sizes 1 and 3 ("(b s) n l -> b n s l")"""
    gn, gl, rows = 6, 5, 270
    x1, x2, lw, lb, w, b, _ = RR.head_inputs(rows, E, seed=3 * E)
    ref, bound = RR.head_fwd(x1, x2, lw, lb, w, b)
    dev = _d(x1, x2, lw, lb, w, b)
    plain = ops.cls_head(*dev, gn, gl, 0)
    assert plain.shape == (rows,) and _scores_ok(plain, ref, bound, f"E={E} seg=0")
    for seg in (1, 3):
        src = O.test_tile_index(rows, gn, gl, seg)
        out = ops.cls_head(*dev, gn, gl, seg)
        assert _scores_ok(out.cpu()[src], ref, bound, f"E={E} seg={seg}")
        assert torch.equal(out.cpu()[src], plain.cpu())              # the same arithmetic, another store address


@pytest.mark.parametrize("E", [64, 256])
def test_cls_head_tile_table_store(E):
    """acx_cls_head_tiles: row (tile, n, l) is stored at base[tile] + n * stride[tile] + l.  Three tiles with their own base and
    stride into a buffer with gaps: the scores are the plain call's, bit for bit, and nothing else is written."""
    gn, gl, tiles = 6, 5, 3
    rows = tiles * gn * gl
    table = [(0, 5), (40, 7), (100, 11)]                             # last element written: 100 + 5 * 11 + 4 = 159
    size = 160
    x1, x2, lw, lb, w, b, _ = RR.head_inputs(rows, E, seed=E + 1)
    dev = _d(x1, x2, lw, lb, w, b)
    plain = ops.cls_head(*dev, gn, gl, 0)
    dst = torch.tensor([base + n * stride + l for base, stride in table for n in range(gn) for l in range(gl)])
    assert int(dst.max()) < size and dst.unique().numel() == rows
    exp = torch.full((size,), -7.0)
    exp[dst] = plain.cpu()
    out = torch.full((size,), -7.0, device=DEV)
    tab = torch.tensor(table, dtype=torch.int32).reshape(-1).to(DEV)
    h = L.ctx(torch.cuda.current_device())
    L.check(L.lib().acx_cls_head_tiles(h, *[t.data_ptr() for t in dev], out.data_ptr(), rows, E, gn, gl, tab.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), h)
    assert torch.equal(out.cpu(), exp)
    # through the wrapper (its buffer has `rows` elements): a video of segment size 2 and one of segment size 1
    tab2 = torch.tensor([(0, 10), (5, 10), (60, 5)], dtype=torch.int32).reshape(-1).to(DEV)
    dst2 = torch.tensor([base + n * stride + l for base, stride in ((0, 10), (5, 10), (60, 5)) for n in range(gn) for l in range(gl)])
    assert sorted(dst2.tolist()) == list(range(rows))
    out2 = ops.cls_head(*dev, gn, gl, 0, tile_table=tab2)
    assert torch.equal(out2.cpu()[dst2], plain.cpu())


def _head_bwd_case(E, rows):
    x1, x2, lw, lb, w, b, ds = RR.head_inputs(rows, E, seed=5 * E + rows)
    dev = _d(x1, x2, lw, lb, w)
    dsd = ds.to(DEV)
    scores = ops.cls_head(*dev, b.to(DEV), 1, 1, 0)                  # the kernel's own f32 scores: an INPUT of the backward
    ref = RR.head_bwd(x1, x2, lw, lb, w, scores.cpu(), ds)
    outs = dict(zip(("dx", "dlw", "dlb", "dw", "db"), ops.cls_head_bwd(*dev, scores, dsd)))
    for k in ("dx", "dlw", "dlb", "dw", "db"):
        assert RR.within(outs[k], *ref[k], f"{k} E={E} rows={rows}", "head_bwd"), k
    dxp, part = ops.cls_head_bwd_parts(*dev, scores, dsd)
    assert part.shape == (ops.row_parts(rows), 3 * E + 4) and torch.equal(dxp, outs["dx"])
    red = ops.reduce_rows(part)
    assert torch.equal(red[:3 * E + 1], torch.cat([outs["dlw"], outs["dlb"], outs["dw"], outs["db"]]))
    dxq, part2 = ops.cls_head_bwd_parts(*dev, scores, dsd)
    assert torch.equal(dxq, dxp) and torch.equal(part2[:, :3 * E + 1], part[:, :3 * E + 1])     # (the pad columns are not written)


@pytest.mark.parametrize("rows", [777, 4101])
@pytest.mark.parametrize("E", RR.WIDTHS)
def test_cls_head_bwd_every_width(E, rows):
    _head_bwd_case(E, rows)


@pytest.mark.parametrize("rows", [8195, 32785])
@pytest.mark.parametrize("E", [128, 256])
def test_cls_head_bwd_deeper_row_regimes(E, rows):
    _head_bwd_case(E, rows)


# =============================================================================================================== ViT embedding
@pytest.mark.parametrize("W", RR.WIDTHS)
def test_vit_embed_every_width(W):
    """x[f, 0] = LN(cls + pos[0]), x[f, 1 + t] = LN(patch[f, t] + pos[1 + t]) for 3 frames of 7 patches, through the C ABI"""
    F_, T = 3, 7
    g = torch.Generator().manual_seed(W)
    patches = (torch.randn(F_ * T, W, generator=g) * 2 + 0.3) * RR.row_scales(F_ * T, g)
    cls, pos = torch.randn(W, generator=g), torch.randn(T + 1, W, generator=g) * 0.5
    lw, lb = torch.randn(W, generator=g), torch.randn(W, generator=g)
    xin = torch.cat([cls.double().expand(F_, 1, W), patches.double().view(F_, T, W)], 1) + pos.double()
    ref, S = RR.ln_fwd(xin.view(-1, W), lw, lb, RR.NORM_LAYER)
    dev = _d(patches, cls, pos, lw, lb)
    out = torch.full((F_ * (T + 1), W), float("nan"), device=DEV)
    h = L.ctx(torch.cuda.current_device())
    L.check(L.lib().acx_vit_embed(h, *[t.data_ptr() for t in dev], out.data_ptr(), F_, T, W, torch.cuda.current_stream().cuda_stream), h)
    assert RR.within(out, ref, S, f"W={W}", "vit_embed")


# =============================================================================================================== small gradient launches
@pytest.mark.parametrize("tiles", [1, 3])
@pytest.mark.parametrize("gn,gl", [(32, 16), (5, 17), (1, 33), (7, 1), (24, 10)])
@pytest.mark.parametrize("E", [64, 256])
def test_pos_grad(tiles, gn, gl, E):
    """d0[n] = sum over tiles and l, d1[l] = sum over tiles and n.  gl > 16 takes the second pass over l with its read-modify-write of
    the first stage's partial (17: one element in it, 33: three passes); gn % 4 != 0 leaves the last group of segment rows ragged."""
    g = torch.Generator().manual_seed(tiles + gn + gl + E)
    dx = torch.randn(tiles * gn * gl, E, generator=g) * RR.row_scales(tiles * gn * gl, g)
    v = dx.double().view(tiles, gn, gl, E)
    d0, d1 = ops.pos_grad(dx.to(DEV), tiles, gn, gl)
    assert d0.shape == (gn, E) and d1.shape == (gl, E)
    assert RR.within(d0, v.sum((0, 2)), v.abs().sum((0, 2)), f"d0 {tiles}x{gn}x{gl}x{E}", "pos_grad")
    assert RR.within(d1, v.sum((0, 1)), v.abs().sum((0, 1)), f"d1 {tiles}x{gn}x{gl}x{E}", "pos_grad")
    e0, e1 = ops.pos_grad(dx.to(DEV), tiles, gn, gl)
    assert torch.equal(e0, d0) and torch.equal(e1, d1)


def test_ctx_grad():
    g = torch.Generator().manual_seed(8)
    C_, n_ctx, Lc, W = 5, 3, 9, 68
    dx = torch.randn(C_ * Lc, W, generator=g) * RR.row_scales(C_ * Lc, g)
    v = dx.view(C_, Lc, W)[:, 1:1 + n_ctx]
    dxd = dx.to(DEV)
    assert torch.equal(ops.ctx_grad(dxd, C_, n_ctx, Lc, W, False).cpu(), v)
    shared = ops.ctx_grad(dxd, C_, n_ctx, Lc, W, True)
    assert shared.shape == (n_ctx, W) and RR.within(shared, v.double().sum(0), v.double().abs().sum(0), "shared context", "ctx_grad")
    for sh in (False, True):
        buf = torch.full((n_ctx, W) if sh else (C_, n_ctx, W), float("nan"), device=DEV)
        ret = ops.ctx_grad(dxd, C_, n_ctx, Lc, W, sh, out=buf)
        assert ret is buf and torch.equal(buf, ops.ctx_grad(dxd, C_, n_ctx, Lc, W, sh))


# =============================================================================================================== data movement
@pytest.mark.parametrize("W", [4, 512, 772])
def test_gather_scatter_rows(W):
    g = torch.Generator().manual_seed(W)
    rows, n = 301, 77
    x = torch.randn(rows, W, generator=g)
    idx = torch.randperm(rows, generator=g)[:n]                      # distinct (scatter_rows' contract), unsorted
    assert torch.equal(ops.gather_rows(x.to(DEV), idx.to(DEV)).cpu(), x.index_select(0, idx))
    rep = torch.randint(0, rows, (n,), generator=g)                  # gathering may repeat a row
    assert torch.equal(ops.gather_rows(x.to(DEV), rep.to(DEV)).cpu(), x.index_select(0, rep))
    src = torch.randn(n, W, generator=g)
    assert torch.equal(ops.scatter_rows(src.to(DEV), idx.to(DEV), rows).cpu(), torch.zeros(rows, W).index_copy(0, idx, src))


def test_gather_scatter_rows_refuse_a_width_off_four():
    x, idx = torch.randn(8, 6).to(DEV), torch.arange(3).to(DEV)
    with pytest.raises(L.AcxError):
        ops.gather_rows(x, idx)
    with pytest.raises(L.AcxError):
        ops.scatter_rows(x[:3].contiguous(), idx, 8)


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("with_pos", [True, False])
def test_prompt_embed(shared, with_pos):
    g = torch.Generator().manual_seed(int(shared) + 2 * int(with_pos))
    C_, n_ctx, Ls, W = 5, 3, 7, 68
    Lc = 1 + n_ctx + Ls
    prefix, suffix = torch.randn(C_, 1, W, generator=g), torch.randn(C_, Ls, W, generator=g)
    ctxv = torch.randn(n_ctx, W, generator=g) if shared else torch.randn(C_, n_ctx, W, generator=g)
    pos = torch.randn(Lc, W, generator=g) if with_pos else None
    full = torch.cat([prefix, ctxv.expand(C_, n_ctx, W), suffix], 1)
    for Lout in (None, 6, 2):                                        # all positions; a cut inside the suffix; inside the context
        n = Lc if Lout is None else Lout
        ref = full[:, :n] + pos[:n] if with_pos else full[:, :n]
        out = ops.prompt_embed(*_d(prefix, ctxv, suffix), None if pos is None else pos.to(DEV), n_ctx, Lout)
        assert out.shape == (C_, n, W) and torch.equal(out.cpu(), ref)


def test_add_bcast():
    g = torch.Generator().manual_seed(6)
    x, p = torch.randn(7, 11, 36, generator=g), torch.randn(11, 36, generator=g)
    assert torch.equal(ops.add_bcast(x.to(DEV), p.to(DEV)).cpu(), x + p)


def test_leaky_grad_planes():
    """out = d * (hi > 0 ? 1 : 0.01) with hi the bf16 HI plane of the saved activation, and the three bf16 planes of out -- the
    fused launch against the two single-purpose ones, bit for bit"""
    g = torch.Generator().manual_seed(12)
    rows, C_ = 37, 68
    u = torch.randn(rows, C_, generator=g)
    u[0, :8] = torch.tensor([0.0, -0.0, 1.0 + 2 ** -8 + 2 ** -10, -(1.0 + 2 ** -8 + 2 ** -10), 1e-30, -1e-30, 3.0, -3.0])
    d = torch.randn(rows, C_, generator=g)
    d[1, :6] = torch.tensor([0.0, -0.0, 1.0 + 2 ** -8 + 2 ** -10, -(1.0 + 2 ** -8 + 2 ** -10), 1.0 + 2 ** -9 + 2 ** -17, -100.0 / 3])
    d[0, :8] = torch.tensor([1.5, 1.5, -2.0, -2.0, 1.0 + 2 ** -8 + 2 ** -10, 0.7, -0.0, 0.0])
    u3 = ops.split_bf16x3(u.to(DEV))
    dd = d.to(DEV)
    out, planes = ops.leaky_grad_planes(u3, dd)
    ref = ops.act(u3[0].float(), dd, 0)
    assert torch.equal(out.view(torch.int32), ref.view(torch.int32))
    assert torch.equal(planes.view(torch.int16), ops.split_bf16x3(out).view(torch.int16))
    exp = d * torch.where(u3[0].float().cpu() > 0, 1.0, 0.01)
    assert torch.equal(out.cpu(), exp)                               # (one f32 product: torch rounds it the same way)


@pytest.mark.parametrize("a", [1.0, -0.5])
def test_multi_axpy(a):
    """one launch over tensors of 1, 1023, 1024, 1025 and 50001 elements (1024 per workgroup): y += a x, a product that is exact, so
    the fused and the unfused form agree bit for bit"""
    g = torch.Generator().manual_seed(13)
    sizes = [1, 1023, 1024, 1025, 50001]
    ys = [torch.randn(n, generator=g) for n in sizes]
    xs = [torch.randn(n, generator=g) for n in sizes]
    yd, xd = _d(*ys), _d(*xs)
    ops.multi_axpy_(yd, xd, a)
    for y, x, out, xin in zip(ys, xs, yd, xd):
        assert torch.equal(out.cpu(), y + a * x) and torch.equal(xin.cpu(), x)


@pytest.mark.parametrize("R,Cn", [(33, 65), (1, 7)])
def test_transpose(R, Cn):
    x = torch.randn(R, Cn, generator=torch.Generator().manual_seed(R))
    assert torch.equal(ops.transpose(x.to(DEV)).cpu(), x.t().contiguous())


def test_act_and_add_refuse_a_length_off_four():
    x = torch.randn(7, 3).to(DEV)
    with pytest.raises(L.AcxError):
        ops.act(x, x, 0)
    with pytest.raises(L.AcxError):
        ops.add(x, x)
