"""No GPU: the reference side of tests/test_gpu_mil_chain.py and the host side of the chain's entry points.  The fp64 closed forms of
mil_ref against torch's fp64 autograd of oracle.compute_loss / a plain BatchNorm expression / oracle.selector_directions (1e-12 * S);
torch's fp32 evaluation of the same inside HALF the bound the kernels are held to (so the form of S, not a kernel, is what this
file judges); the properties the seeded inputs promise; the C ABI's refusal of odd B, k > N and C-1 = 65 before any launch; and the
two shape queries the training step asks (acx_selector_tail_fits, acx_mil_loss_bn_fits) on both sides of every boundary."""
import ctypes as C

import pytest
import torch

from anomalyclip_amd import _lib as L
from oracle import anomalyclip_oracle as O
import mil_ref as MR

LOSS_CASES = MR.LOSS_SWEEP + MR.LOSS_BN_EXTRA
GRADS = ("dsim", "dsim_topk", "dscores")


def _loss_autograd(inp, case, gout, dtype):
    B, N, Lg, C1, K, nid = case
    lam = MR.LAMBDAS
    with torch.enable_grad():
        s1, s2, s3 = (inp[k].to(dtype).clone().requires_grad_(True) for k in ("sim", "sim_topk", "scores"))
        outs = O.compute_loss(s1, s2, inp["labels"], s3, inp["idx_topk_abn"], inp["idx_topk_nor"], inp["idx_bottomk_abn"],
                              normal_id=nid, num_topk=K, num_segments=N, frames_per_segment=Lg, lambda_dir_abn=lam[0],
                              lambda_dir_nor=lam[1], lambda_topk_abn=lam[2], lambda_bottomk_abn=lam[3], lambda_topk_nor=lam[4],
                              lambda_smooth=lam[5], lambda_sparse=lam[6])
        (outs[0] * gout).backward()
    return {"losses": torch.stack([o.detach() for o in outs]), "dsim": s1.grad, "dsim_topk": s2.grad, "dscores": s3.grad}


def _loss_ref(inp, case, gout):
    _, N, Lg, _, K, nid = case
    return MR.mil_loss(inp["sim"], inp["sim_topk"], inp["labels"], inp["scores"], inp["idx_topk_abn"], inp["idx_topk_nor"],
                       inp["idx_bottomk_abn"], N, Lg, K, nid, MR.LAMBDAS, gout)


@pytest.mark.parametrize("case", LOSS_CASES, ids=MR.case_id)
def test_loss_closed_forms_equal_fp64_autograd(case):
    inp = MR.loss_inputs(case)
    for gout in (MR.GOUT, 1.0):
        got, ref = _loss_autograd(inp, case, gout, torch.float64), _loss_ref(inp, case, gout)
        for k in ("losses",) + GRADS:
            assert MR.within(got[k], *ref[k], tol=1e-12), (k, gout)
    # where S is zero the closed form itself is an exact zero, and S is zero nowhere else
    for k in GRADS:
        v, S = ref[k]
        assert bool(((S == 0) == (v == 0)).all()) or case[3] == 1, k          # (C1 = 1: dsim = w (1 - 1) = 0 under S = w)


@pytest.mark.parametrize("case", LOSS_CASES, ids=MR.case_id)
def test_loss_fp32_reference_is_inside_half_the_bound(case):
    """torch's fp32 forward and autograd of the oracle's loss against the fp64 closed forms: |err| <= 1e-6 * S on every element.  A
    failure here means S leaves out a term the value is made of."""
    inp = MR.loss_inputs(case)
    got, ref = _loss_autograd(inp, case, MR.GOUT, torch.float32), _loss_ref(inp, case, MR.GOUT)
    for k in ("losses",) + GRADS:
        assert MR.within(got[k], *ref[k], what=f"{k} {MR.case_id(case)}", family="fp32-cpu-loss", tol=MR.TOL / 2), k


def test_loss_inputs_are_the_hard_ones():
    for case in LOSS_CASES:
        B, N, Lg, C1, K, nid = case
        inp = MR.loss_inputs(case)
        sc, lab = inp["scores"], inp["labels"]
        assert bool((sc >= torch.tensor(1e-6)).all()) and bool((sc <= torch.tensor(1 - 1e-6)).all())        # (the f32 roundings)
        assert int((sc < 1e-4).sum()) > 0 and int((sc > 1 - 1e-4).sum()) > 0
        assert bool((lab[B // 2:] == nid).all()) and bool((lab[:B // 2] != nid).all()) and int(lab.max()) <= C1
        if nid < C1:
            assert nid + 1 in lab.tolist()
        if B // 2 >= 2:
            assert max(c for c in range(C1 + 1) if c != nid) in lab.tolist()
        if B // 2 >= 3 and 0 < nid < C1:
            assert int(lab[:B // 2].min()) < nid < int(lab[:B // 2].max())
        for k in ("idx_topk_abn", "idx_topk_nor", "idx_bottomk_abn"):
            assert all(len(set(r)) == K for r in inp[k].tolist())
        top2 = inp["sim"].topk(min(2, C1), dim=1)[0]
        assert C1 == 1 or bool((top2[:, 0] > top2[:, 1]).all())                 # no argmax ties
    assert len(set(MR.LAMBDAS)) == 7


@pytest.mark.parametrize("rows,C1", MR.BN_SWEEP)
def test_bn_bwd_closed_form(rows, C1):
    """fp64: the closed form from (xhat, biased variance) equals autograd through (raw - mean) / sqrt(var + eps); fp32: torch's
    autograd of the same expression stays within 1e-6 * S of the closed form evaluated on ITS normalised output and variance"""
    raw, dl = MR.bn_inputs(rows, C1, seed=rows + C1)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, MR.TOL / 2)):
        with torch.enable_grad():
            x = raw.to(dtype).clone().requires_grad_(True)
            var = x.var(0, unbiased=False)
            y = (x - x.mean(0)) / torch.sqrt(var + 1e-5)
            y.backward(dl.to(dtype))
        ref, S = MR.bn_bwd(y.detach(), dl, var.detach(), rows)
        fam = None if dtype == torch.float64 else "fp32-cpu-bn"
        assert MR.within(x.grad, ref, S, what=f"draw rows={rows} C1={C1}", family=fam, tol=tol), dtype
    sums, sabs = MR.bn_col_sums(y.detach(), dl)
    assert MR.within(torch.cat([dl.sum(0), (dl * y.detach()).sum(0)]), sums, sabs, what=f"sums rows={rows} C1={C1}",
                     family="fp32-cpu-bn", tol=MR.TOL / 2)


@pytest.mark.parametrize("Cc,D,nid", MR.DIRS_SWEEP)
def test_directions_closed_forms(Cc, D, nid):
    text, nc, dd = MR.dirs_inputs(Cc, D, seed=Cc + D + nid)
    for dtype, tol in ((torch.float64, 1e-12), (torch.float32, MR.TOL / 2)):
        with torch.enable_grad():
            t = text.to(dtype).clone().requires_grad_(True)
            dirs = O.selector_directions(t, nc.to(dtype), nid)
            dirs.backward(dd.to(dtype))
        fam = None if dtype == torch.float64 else "fp32-cpu-dirs"
        tag = f"C={Cc} D={D} normal_id={nid}"
        assert MR.within(dirs.detach(), *MR.dirs_fwd(text, nc, nid), what=f"dirs {tag}", family=fam, tol=tol), dtype
        ref, S = MR.dirs_bwd(text, nc, dd, nid)
        assert MR.within(t.grad, ref, S, what=f"dtext {tag}", family=fam, tol=tol), dtype
        assert bool((t.grad[nid] == 0).all()) and bool((S[nid] == 0).all()) and bool((ref[nid] == 0).all())


def test_select_inputs_hold_what_they_promise():
    for (B, N, Lg, C1, K, nid) in MR.LOSS_SWEEP:
        kinds_t, kinds_b = set(), set()
        for shift in ((0, 2) if B < 4 else (0,)):
            lg, labels, mt, mb = MR.select_inputs(B, N, Lg, C1, nid, K, 1, seed=5, shift=shift)
            assert not torch.equal(mt, mb) and bool((lg * 64 == (lg * 64).round()).all()) and float(lg.abs().max()) <= 4
            kinds_t |= {int(r.sum()) for r in mt[:4]}
            kinds_b |= {int(r.sum()) for r in mb[:4]}
            seg = lg.view(B, N, Lg * C1)
            for v in range(B if N >= 2 else 0):
                assert any(torch.equal(seg[v, a], seg[v, b]) for a in range(N) for b in range(a + 1, N)), v
        assert {0, 1, min(K, N), N} <= kinds_t and {0, 1, N} <= kinds_b


def test_chain_refuses_bad_arguments_before_any_launch():
    """odd B, k > N and C-1 = 65: ACX_E_BADARG with the entry point's name in acx_last_error, and B N Lg % 256 != 0 is
    ACX_E_UNSUPPORTED for acx_mil_loss_bn.  No device is needed: a refusal comes before the launch (with a launch the code would be
    ACX_E_HIP here, or ACX_OK on a GPU)."""
    lib = L.lib()
    buf = (C.c_float * 8192)()
    p = C.addressof(buf)
    N, Lg, K, nid = 4, 4, 2, 0

    def select_idx(B=2, C1=3, ktop=K, kbot=K):
        return lib.acx_select_idx(None, p, p, p, p, p, p, B, N, Lg, C1, nid, ktop, kbot, None)

    def mil_loss_one(B=2, C1=3, counter=p):
        return lib.acx_mil_loss_one(None, *[p] * 12, 8192, B, N, Lg, C1, K, nid, p, None, counter, None)

    def mil_loss_bn(B=2, C1=3, N_=N):
        return lib.acx_mil_loss_bn(None, *[p] * 13, 8192, p, 8192 * 4, B, N_, Lg, C1, K, nid, p, None, p, None)

    def selector_tail(B=2, C1=3, ktop=K, kbot=K):
        return lib.acx_selector_tail(None, p, None, 0, p, p, p, None, None, None, None, 0.1, 0.9, p, C1, p, p, p, p, p, p, B, N, Lg, C1,
                                     nid, ktop, kbot, 1e-5, None)

    BADARG, UNSUPPORTED = -1, -2
    cases = [
        ("acx_select_idx", lambda: select_idx(B=3), BADARG), ("acx_select_idx", lambda: select_idx(ktop=N + 1), BADARG),
        ("acx_select_idx", lambda: select_idx(kbot=N + 1), BADARG),
        ("acx_mil_loss", lambda: mil_loss_one(B=3), BADARG), ("acx_mil_loss", lambda: mil_loss_one(C1=65), BADARG),
        ("acx_mil_loss", lambda: mil_loss_one(counter=None), BADARG),
        ("acx_mil_loss_bn", lambda: mil_loss_bn(B=3), BADARG), ("acx_mil_loss_bn", lambda: mil_loss_bn(C1=65), BADARG),
        ("acx_mil_loss_bn", lambda: mil_loss_bn(), UNSUPPORTED), ("acx_mil_loss_bn", lambda: mil_loss_bn(N_=513 * 32), UNSUPPORTED),
        ("acx_selector_tail", lambda: selector_tail(B=3), BADARG), ("acx_selector_tail", lambda: selector_tail(C1=65), BADARG),
        ("acx_selector_tail", lambda: selector_tail(ktop=N + 1), BADARG),
        ("acx_bn_bwd_stats", lambda: lib.acx_bn_bwd_stats(None, p, p, p, 16, 65, p, 1 << 20, None), BADARG),
        ("acx_bn_combine", lambda: lib.acx_bn_combine(None, p, 2, 65, p, p, p, p, None), BADARG),
    ]
    for name, call, code in cases:
        lib.acx_layernorm(None, None, 0, None, None, None, 0, 0, 4, 64, 1e-5, 0, None)        # another text in the error slot
        assert b"null" in lib.acx_last_error(None)
        assert call() == code, name
        assert lib.acx_last_error(None).startswith(name.encode() + b":"), (name, lib.acx_last_error(None))


OK, BADARG, UNSUPPORTED = 0, -1, -2
# (B, N, Lg, C1, ktop, kbot) -> the code of acx_selector_tail_fits and of acx_selector_tail's shape checks
TAIL_BOUNDARIES = [
    ((2, 2559, 13, 1, 7, 7), OK),                  # exactly 163,840 bytes of LDS
    ((2, 2559, 13, 1, 7, 8), UNSUPPORTED),         # 163,844
    ((2, 37, 16, 64, 3, 3), OK), ((2, 38, 16, 64, 3, 3), UNSUPPORTED),
    ((2, 4, 4, 64, 2, 2), OK), ((2, 4, 4, 65, 2, 2), BADARG), ((2, 4, 4, 0, 2, 2), BADARG),
    ((3, 4, 4, 3, 2, 2), BADARG),
    ((2, 4, 4, 3, 5, 2), BADARG),                  # ktop = N + 1
]
# (B, N, Lg, C1, K) -> the code of acx_mil_loss_bn_fits and of acx_mil_loss_bn's shape checks
LOSS_BN_BOUNDARIES = [
    ((2, 8, 16, 3, 1), OK), ((2, 8, 15, 3, 1), UNSUPPORTED),                    # 256 rows, 240
    ((2, 4096, 16, 3, 1), OK), ((2, 4104, 16, 3, 1), UNSUPPORTED),              # 131072 rows (512 slabs), 131328
    ((2, 8, 16, 64, 1), OK), ((2, 8, 16, 65, 1), BADARG), ((2, 8, 16, 0, 1), BADARG),
    ((3, 8, 16, 3, 1), BADARG),
]


def test_shape_queries_agree_with_the_gates_and_the_entry_points():
    """acx_selector_tail_fits / acx_mil_loss_bn_fits through the C ABI with a null context: `== ACX_OK` equals the gate the training
    step evaluated itself (mil_ref) over the loss sweep; the expected code on both sides of every boundary; and for every refused
    shape the entry point (dummy pointers: it returns before any launch) gives the query's code."""
    lib = L.lib()
    for (B, N, Lg, C1, K, _) in LOSS_CASES:
        assert (lib.acx_selector_tail_fits(None, B, N, Lg, C1, K, K) == OK) == MR.selector_tail_gate(B, N, Lg, C1, K, K), (B, N, Lg, C1, K)
        assert (lib.acx_mil_loss_bn_fits(None, B, N, Lg, C1, K) == OK) == MR.mil_loss_bn_gate(B, N, Lg, C1, K), (B, N, Lg, C1, K)
    gates = [MR.mil_loss_bn_gate(*c[:5]) for c in LOSS_CASES]
    assert any(gates) and not all(gates)
    buf = (C.c_float * 8192)()
    p = C.addressof(buf)
    for shape, code in TAIL_BOUNDARIES:
        B, N, Lg, C1, ktop, kbot = shape
        assert lib.acx_selector_tail_fits(None, *shape) == code, shape
        assert code == BADARG or MR.selector_tail_gate(*shape) == (code == OK), shape      # (the gates never judged B or k)
        if code != OK:
            assert lib.acx_selector_tail(None, p, None, 0, p, p, p, None, None, None, None, 0.1, 0.9, p, C1, p, p, p, p, p, p, B, N, Lg,
                                         C1, 0, ktop, kbot, 1e-5, None) == code, shape
            assert lib.acx_last_error(None).startswith(b"acx_selector_tail:"), shape
    for shape, code in LOSS_BN_BOUNDARIES:
        B, N, Lg, C1, K = shape
        assert lib.acx_mil_loss_bn_fits(None, *shape) == code, shape
        assert code == BADARG or MR.mil_loss_bn_gate(*shape) == (code == OK), shape
        if code != OK:
            assert lib.acx_mil_loss_bn(None, *[p] * 13, 8192, p, 8192 * 4, B, N, Lg, C1, K, 0, p, None, p, None) == code, shape
            assert lib.acx_last_error(None).startswith(b"acx_mil_loss_bn:"), shape
