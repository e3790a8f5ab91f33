"""-m gpu: the selector / MIL chain of every training gradient -- select_idx -> gather_segments -> mil_loss / mil_loss_bn ->
scatter_segments_ -> bn_bwd_stats -> bn_bwd_apply -> gemm_tn -> text_directions_bwd -- against plain fp64, element by element with
the bound 2e-6 * S of mil_ref (S = the sum of the absolute values of the terms of the element; an element with S == 0 is exact), at
seven distinct lambdas, on grids other than 32 x 16, at C-1 of 1 and 64, K of 1, 5 and N, normal_id at either end of the class
list, scores within 1e-4 of 0 and of 1, and BatchNorm columns 500 standard deviations away from 0.  The selection is compared bit
for bit with the oracle in fp64 on logits whose sums are exact, with ties away from the mask fill; the fused launches
(selector_tail, mil_loss_bn, selector_dirs_grad) are then compared with separate launches that are themselves checked here.
Every comparison prints its worst |err| / S before it asserts (pytest -s; DESIGN.md section 3 records them)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops
from oracle import anomalyclip_oracle as O
import mil_ref as MR

DEV = "cuda"
BN_CASES = [c for c in MR.LOSS_SWEEP if c[0] * c[1] * c[2] % 256 == 0] + MR.LOSS_BN_EXTRA
LOSS_KEYS = ("sim", "sim_topk", "labels", "scores", "idx_topk_abn", "idx_topk_nor", "idx_bottomk_abn")


def _d(*ts):
    return [t.to(DEV) for t in ts]


@functools.lru_cache(maxsize=None)
def _loss_case(case, gout):
    """(CPU inputs, fp64 reference) of one case of the sweep: computed once, shared by the tests, never written to"""
    _, N, Lg, _, K, nid = case
    inp = MR.loss_inputs(case)
    return inp, MR.mil_loss(*(inp[k] for k in LOSS_KEYS), N, Lg, K, nid, MR.LAMBDAS, 1.0 if gout is None else gout)


def _gout(gout):
    return None if gout is None else torch.tensor([gout], dtype=torch.float32, device=DEV)


def _counter():
    return int(ops._colsum_counters(torch.device(DEV, torch.cuda.current_device()))[ops._CTR_N - 1])


# =============================================================================================================== the loss
@pytest.mark.parametrize("gout", [MR.GOUT, None])
@pytest.mark.parametrize("case", MR.LOSS_SWEEP, ids=MR.case_id)
def test_mil_loss_vs_fp64(case, gout):
    """all eight loss terms, dsim, dsim_topk and dscores of ops.mil_loss within 2e-6 * S; exact zeros where S == 0"""
    _, N, Lg, _, K, nid = case
    inp, ref = _loss_case(case, gout)
    losses, dsim, dtopk, dsc = ops.mil_loss(*_d(*(inp[k] for k in LOSS_KEYS)), N, Lg, K, nid, MR.LAMBDAS, gout=_gout(gout))
    tag = f"{MR.case_id(case)} gout={gout}"
    for i, name in enumerate(MR.LOSS_NAMES):
        assert MR.within(losses[i], ref["losses"][0][i], ref["losses"][1][i], f"{name} {tag}", "loss"), name
    assert MR.within(dsim, *ref["dsim"], f"dsim {tag}", "loss")
    assert MR.within(dtopk, *ref["dsim_topk"], f"dsim_topk {tag}", "loss")
    assert MR.within(dsc, *ref["dscores"], f"dscores {tag}", "loss")
    assert _counter() == 0


@pytest.mark.parametrize("case", BN_CASES, ids=MR.case_id)
def test_mil_loss_bn_vs_fp64(case):
    """ops.mil_loss_bn where B N Lg % 256 == 0: losses and dscores as above, dlogits against dsim + scatter(dsim_topk), bn_sums against
    the fp64 column sums of dl and dl * logits; meter grows by exactly the returned losses; a second call is bit-identical and the
    arrival counter is zero afterwards"""
    B, N, Lg, C1, K, nid = case
    for gout in (MR.GOUT, None):
        inp, ref = _loss_case(case, gout)
        dev = _d(*(inp[k] for k in LOSS_KEYS))
        meter0 = torch.arange(8, dtype=torch.float32, device=DEV) * 0.37
        meter = meter0.clone()
        losses, dl, dsc, sums = ops.mil_loss_bn(*dev, N, Lg, K, nid, MR.LAMBDAS, meter=meter, gout=_gout(gout))
        tag = f"{MR.case_id(case)} gout={gout}"
        for i, name in enumerate(MR.LOSS_NAMES):
            assert MR.within(losses[i], ref["losses"][0][i], ref["losses"][1][i], f"{name} {tag}", "loss_bn"), name
        assert MR.within(dsc, *ref["dscores"], f"dscores {tag}", "loss_bn")
        ref_dl, s_dl = MR.dlogits(ref, torch.cat([inp["idx_topk_abn"], inp["idx_topk_nor"]]), N, Lg)
        assert MR.within(dl, ref_dl, s_dl, f"dlogits {tag}", "loss_bn")
        # the column sums of the dlogits AS RETURNED (checked element by element above), within 2e-6 sum|dl| and 2e-6 sum|dl logits|
        assert MR.within(sums, *MR.bn_col_sums(inp["sim"], dl.cpu()), f"bn_sums {tag}", "loss_bn")
        assert torch.equal(meter, meter0 + losses)
        assert _counter() == 0
        l2, dl2, dsc2, sums2 = ops.mil_loss_bn(*dev, N, Lg, K, nid, MR.LAMBDAS, gout=_gout(gout))
        assert torch.equal(l2, losses) and torch.equal(dl2, dl) and torch.equal(dsc2, dsc) and torch.equal(sums2, sums)
        assert _counter() == 0


@pytest.mark.parametrize("case", [c for c in MR.LOSS_SWEEP if c not in BN_CASES], ids=MR.case_id)
def test_mil_loss_bn_refuses_rows_off_the_slab(case):
    _, N, Lg, _, K, nid = case
    inp, _ = _loss_case(case, None)
    with pytest.raises(L.AcxError, match=r"libacx error -2: acx_mil_loss_bn"):
        ops.mil_loss_bn(*_d(*(inp[k] for k in LOSS_KEYS)), N, Lg, K, nid, MR.LAMBDAS)
    assert _counter() == 0


def test_mil_loss_weighted_golden(golden):
    """ops.mil_loss against the REFERENCE's ComputeLoss at seven distinct weights (tests/golden/loss_weighted.npz), at 2e-6 * S"""
    g = golden("loss_weighted")
    B, N, Lg, C1, K, nid = (int(v) for v in g["shape"])
    lam = [float(v) for v in g["lambdas"]]
    inp = {k: torch.from_numpy(g[k]) for k in LOSS_KEYS}
    S = MR.mil_loss(*(inp[k] for k in LOSS_KEYS), N, Lg, K, nid, lam)
    losses, dsim, dtopk, dsc = ops.mil_loss(*_d(*(inp[k] for k in LOSS_KEYS)), N, Lg, K, nid, lam)
    T = lambda k: torch.from_numpy(g[k]).double()                                                       # noqa: E731
    assert MR.within(losses, T("losses"), S["losses"][1], "losses", "loss_golden")
    assert MR.within(dsim, T("g_sim"), S["dsim"][1], "dsim", "loss_golden")
    assert MR.within(dtopk, T("g_sim_topk"), S["dsim_topk"][1], "dsim_topk", "loss_golden")
    assert MR.within(dsc, T("g_scores"), S["dscores"][1], "dscores", "loss_golden")


# =============================================================================================================== selection, exactly
def _k_pairs(K):
    return sorted({(K, 1), (1, K)})


@pytest.mark.parametrize("case", MR.LOSS_SWEEP, ids=MR.case_id)
def test_selection_gather_scatter_exact(case):
    """logits in multiples of 2^-6: select_idx equals the oracle's fp64 selection bit for bit (ktop != kbot, different masks with
    all-zero / one-survivor / exactly-k / full rows, duplicated segments), gather_segments equals the oracle's gather and
    scatter_segments_ an fp32 index_add (one addend per destination)"""
    B, N, Lg, C1, K, nid = case
    for ktop, kbot in _k_pairs(K):
        for shift in ((0, 2) if B < 4 else (0,)):                 # two videos cannot hold four kinds of mask row: two rounds
            lg, labels, mt, mb = MR.select_inputs(B, N, Lg, C1, nid, ktop, kbot, seed=17 * ktop + kbot, shift=shift)
            lgd = lg.to(DEV)
            it, ib = ops.select_idx(lgd, *_d(labels, mt, mb), N, Lg, nid, ktop, kbot)
            ta, tn = O.select_idx(lg.double(), labels, mt, nid, N, Lg, ktop, True)
            ba, bn = O.select_idx(lg.double(), labels, mb, nid, N, Lg, kbot, False)
            assert torch.equal(it.cpu(), torch.cat([ta, tn])), (ktop, kbot, shift)
            assert torch.equal(ib.cpu(), torch.cat([ba, bn])), (ktop, kbot, shift)
            for idx in (it, ib):
                got = ops.gather_segments(lgd.view(-1, C1), idx, N, Lg)
                assert torch.equal(got.cpu(), O.gather_segments(lg, idx.cpu(), N, Lg))
                g = torch.Generator().manual_seed(ktop + 3 * kbot)
                base = torch.randn(B * N * Lg, C1, generator=g)
                dout = torch.randn(got.shape, generator=g)
                acc = base.to(DEV)
                ops.scatter_segments_(acc, dout.to(DEV), idx, N, Lg)
                assert torch.equal(acc.cpu(), base.index_add(0, MR.segment_rows(idx.cpu(), N, Lg), dout))


@pytest.mark.parametrize("case", MR.LOSS_SWEEP, ids=MR.case_id)
def test_selector_tail_equals_checked_launches(case):
    """ops.selector_tail bit-identical to selector_bn + bn_running_update_ + select_idx + gather_segments on the sweep's grids (N Lg no
    power of two, C-1 of 1 and 64, ktop != kbot) -- the separate launches are the ones checked against fp64 in this file"""
    B, N, Lg, C1, K, nid = case
    ktop, kbot = K, min(K + 1, N)
    assert (N * Lg * C1 + N * C1 + 2 * N + 2 * C1 + ktop + kbot) * 4 <= 160 * 1024
    raw, _ = MR.bn_inputs(B * N * Lg, C1, seed=B + C1)
    _, labels, mt, mb = MR.select_inputs(B, N, Lg, C1, nid, ktop, kbot, seed=23)
    rawd, labels, mt, mb = _d(raw, labels, mt, mb)
    bn_a, bn_b = torch.nn.BatchNorm1d(C1, affine=False).to(DEV), torch.nn.BatchNorm1d(C1, affine=False).to(DEV)
    for bn in (bn_a, bn_b):
        bn.running_mean.copy_(torch.linspace(-1, 1, C1))
        bn.running_var.copy_(torch.linspace(0.5, 2, C1))
    mean, var_b, var_u = ops.bn_stats(rawd)
    logits = ops.selector_bn(rawd, mean, var_b, 1e-5)
    ops.bn_running_update_(bn_a, mean, var_u)
    it, ib = ops.select_idx(logits, labels, mt, mb, N, Lg, nid, ktop, kbot)
    topk = ops.gather_segments(logits, it, N, Lg)
    l2, it2, ib2, topk2, _ = ops.selector_tail(rawd, labels, mt, mb, N, Lg, nid, ktop, kbot, 1e-5, stats=(mean, var_b, var_u), bn=bn_b)
    assert torch.equal(l2, logits) and torch.equal(it2, it) and torch.equal(ib2, ib) and torch.equal(topk2, topk)
    assert torch.equal(bn_a.running_mean, bn_b.running_mean) and torch.equal(bn_a.running_var, bn_b.running_var)
    assert int(bn_b.num_batches_tracked) == int(bn_a.num_batches_tracked) == 1


# =============================================================================================================== the BatchNorm chain
@pytest.mark.parametrize("rows,C1", MR.BN_SWEEP)
def test_bn_chain_vs_fp64(rows, C1):
    """bn_stats (mean within 2^-22 mean|x|, both variances within 1e-6 relative: f64 accumulators), selector_bn, bn_bwd_stats and
    bn_bwd_apply on columns whose mean dwarfs their spread; pad columns of draw exactly zero for pad_to 4 and 8; total_rows as a
    device scalar bit-identical to the host integer"""
    raw, dl = MR.bn_inputs(rows, C1, seed=rows + C1)
    rawd, dld = _d(raw, dl)
    x = raw.double()
    tag = f"rows={rows} C1={C1}"
    mean, var_b, var_u = ops.bn_stats(rawd)
    r_mean = ((mean.double().cpu() - x.mean(0)).abs() / x.abs().mean(0)).max()
    r_vb = ((var_b.double().cpu() - x.var(0, unbiased=False)).abs() / x.var(0, unbiased=False)).max()
    r_vu = ((var_u.double().cpu() - x.var(0, unbiased=True)).abs() / x.var(0, unbiased=True)).max()
    print(f"MIL_RATIO bn_stats {tag} mean {float(r_mean):.3e} var_b {float(r_vb):.3e} var_u {float(r_vu):.3e}")
    assert float(r_mean) <= 2.0 ** -22 and float(r_vb) <= 1e-6 and float(r_vu) <= 1e-6
    # BatchNorm of raw by the f32 statistics as given
    m, rstd = mean.double().cpu(), 1.0 / torch.sqrt(var_b.double().cpu() + 1e-5)
    logits = ops.selector_bn(rawd, mean, var_b, 1e-5)
    assert MR.within(logits, (x - m) * rstd, (x.abs() + m.abs()) * rstd, f"logits {tag}", "bn")
    # backward sums and apply, each from its inputs as given
    lc = logits.cpu()
    ref_sums, s_sums = MR.bn_col_sums(lc, dl)
    assert MR.within(ops.bn_bwd_stats(logits, dld), ref_sums, s_sums, f"sums {tag}", "bn")
    sums_in = ref_sums.float()
    ref, S = MR.bn_bwd(lc, dl, var_b.cpu(), rows, sums=sums_in)
    n_dev = torch.tensor([float(rows)], dtype=torch.float32, device=DEV)
    for pad in (4, 8):
        draw = ops.bn_bwd_apply(logits, dld, var_b, sums_in.to(DEV), rows, 1e-5, pad_to=pad)
        assert draw.shape == (rows, (C1 + pad - 1) // pad * pad) and bool((draw[:, C1:] == 0).all())
        assert MR.within(draw[:, :C1], ref, S, f"draw {tag} pad_to={pad}", "bn")
        assert torch.equal(ops.bn_bwd_apply(logits, dld, var_b, sums_in.to(DEV), n_dev, 1e-5, pad_to=pad), draw)


# =============================================================================================================== the directions
@pytest.mark.parametrize("Cc,D,nid", MR.DIRS_SWEEP)
def test_text_directions_vs_fp64(Cc, D, nid):
    """text_directions within 2e-6 (|t| + |nc|) / |v|; text_directions_bwd within 2e-6 * S with the normal_id row exactly zero
    (D = 2560: the loop past the eight register slots of text_dirs_bwd_kernel)"""
    text, nc, dd = MR.dirs_inputs(Cc, D, seed=Cc + D + nid)
    td, ncd, ddd = _d(text, nc, dd)
    tag = f"C={Cc} D={D} normal_id={nid}"
    assert MR.within(ops.text_directions(td, ncd, nid), *MR.dirs_fwd(text, nc, nid), f"dirs {tag}", "dirs")
    dtext = ops.text_directions_bwd(td, ncd, ddd, nid)
    assert MR.within(dtext, *MR.dirs_bwd(text, nc, dd, nid), f"dtext {tag}", "dirs")
    assert bool((dtext[nid] == 0).all())


@pytest.mark.parametrize("rows,C1,D,nid", [(960, 6, 512, 3), (32768, 13, 512, 7)])
def test_selector_dirs_grad_equals_checked_launches(rows, C1, D, nid):
    """selector_dirs_grad (the TN product's partial images added by the consumer; 32768 rows: the K-split case) bit-identical to
    gemm_tn(b_sub = ncentroid) + text_directions_bwd, the latter checked against fp64 above"""
    g = torch.Generator().manual_seed(rows + C1)
    draw = torch.zeros(rows, (C1 + 3) // 4 * 4)
    draw[:, :C1] = torch.randn(rows, C1, generator=g)
    x = torch.randn(rows, D, generator=g)
    text, nc, _ = MR.dirs_inputs(C1 + 1, D, seed=rows)
    draw, x, text, nc = _d(draw, x, text, nc)
    d_dirs = ops.gemm_tn(draw, x, b_sub=nc)[:C1].contiguous()
    ref = ops.text_directions_bwd(text, nc, d_dirs, nid)
    out = ops.selector_dirs_grad(draw, x, nc, text, nid, C1)
    assert torch.equal(out, ref) and bool((out[nid] == 0).all()) and bool(torch.isfinite(out).all())


# =============================================================================================================== refusals
def test_chain_refusals_raise_before_any_launch():
    """odd B, ktop > N and C-1 = 65 through the Python entry points: AcxError with ACX_E_BADARG (-1) and the entry point's name -- the
    host's argument checks, in front of the launch; the stream is healthy afterwards"""
    N, Lg, K, nid = 4, 4, 2, 0
    z = lambda *s: torch.zeros(*s, device=DEV)                                                          # noqa: E731
    zi = lambda *s: torch.zeros(*s, dtype=torch.int64, device=DEV)                                      # noqa: E731

    def loss_args(B, C1):
        Bh = max(B // 2, 1)
        return (z(B * N * Lg, C1), z(B * K * Lg, C1), zi(B), z(B * N * Lg) + 0.5, zi(Bh, K), zi(B - B // 2, K), zi(Bh, K), N, Lg, K, nid,
                MR.LAMBDAS)

    def sel_args(B, C1):
        return z(B, N * Lg, C1), zi(B), z(B, N) + 1, z(B, N) + 1

    def tail(B, C1, ktop):
        st = (z(C1), z(C1) + 1, z(C1) + 1)
        return ops.selector_tail(z(B * N * Lg, C1), zi(B), z(B, N) + 1, z(B, N) + 1, N, Lg, nid, ktop, K, 1e-5, stats=st)

    cases = [
        ("acx_select_idx", lambda: ops.select_idx(*sel_args(3, 3), N, Lg, nid, K, K)),
        ("acx_select_idx", lambda: ops.select_idx(*sel_args(2, 3), N, Lg, nid, N + 1, K)),
        ("acx_mil_loss", lambda: ops.mil_loss(*loss_args(3, 3))),
        ("acx_mil_loss", lambda: ops.mil_loss(*loss_args(2, 65))),
        ("acx_mil_loss_bn", lambda: ops.mil_loss_bn(*loss_args(3, 3))),
        ("acx_mil_loss_bn", lambda: ops.mil_loss_bn(*loss_args(2, 65))),
        ("acx_selector_tail", lambda: tail(3, 3, K)),
        ("acx_selector_tail", lambda: tail(2, 65, K)),
        ("acx_selector_tail", lambda: tail(2, 3, N + 1)),
        ("acx_bn_bwd_stats", lambda: ops.bn_bwd_stats(z(16, 65), z(16, 65))),
        ("acx_bn_combine", lambda: ops.bn_combine(z(2, 131) + 1, 65)),
    ]
    for name, call in cases:
        with pytest.raises(L.AcxError, match=rf"libacx error -1: {name}:"):
            call()
    torch.cuda.synchronize()
    assert _counter() == 0
