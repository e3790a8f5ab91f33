"""No GPU: the reference side of tests/test_gpu_rowwise.py and the host side of the row-wise entry points.  The fp64 closed forms
of rowwise_ref against torch's fp64 autograd; torch's fp32 evaluation of the same cases inside HALF the bound the kernels are held
to (so the form of S, not the kernel, is what this file judges); acx_row_parts against the rows-per-wave rule restated; and the
C ABI's refusal of row widths outside {64, 128, 256, 512, 640, 768, 1024}, before any launch."""
import ctypes as C

import pytest
import torch

from anomalyclip_amd import _lib as L
from oracle import anomalyclip_oracle as O
import rowwise_ref as RR

LN_CASES = [(D, mode) for D in (64, 640) for mode in (RR.NORM_LAYER, RR.NORM_CHAN)]
ROWS = 37
FEW_ROWS = (1, 3, ROWS)        # one and three rows: a sum over rows hides nothing there (S must hold term by term)


def _ln_autograd(x, w, b, dy, mode, dtype):
    with torch.enable_grad():
        xr, wr, br = (t.to(dtype).clone().requires_grad_(True) for t in (x, w, b))
        y = O.layer_norm(xr, wr, br) if mode == RR.NORM_LAYER else O.chan_layer_norm_last(xr, wr, br)
        y.backward(dy.to(dtype))
    return y.detach(), {"dx": xr.grad, "dw": wr.grad, "db": br.grad}


def _head_autograd(x1, x2, lw, lb, w, b, ddot, dtype):
    """the pre-sigmoid sum and the five gradients for a given d(loss)/d(sum)"""
    with torch.enable_grad():
        ps = [t.to(dtype).clone().requires_grad_(True) for t in (x1, x2, lw, lb, w, b)]
        dot = (O.layer_norm((ps[0] + ps[1]) / 2, ps[2], ps[3]) @ ps[4].t() + ps[5]).view(-1)
        dot.backward(ddot.to(dtype))
    return dot.detach(), {"dx": ps[0].grad, "dx2": ps[1].grad, "dlw": ps[2].grad, "dlb": ps[3].grad, "dw": ps[4].grad.view(-1),
                          "db": ps[5].grad}


def _head_case(E, rows=ROWS):
    x1, x2, lw, lb, w, b, ds = RR.head_inputs(rows, E, seed=100 + E + rows)
    scores = torch.sigmoid((O.layer_norm((x1 + x2) / 2, lw, lb) @ w.t() + b).view(-1))           # f32, as the kernel would save them
    return x1, x2, lw, lb, w, b, ds, scores


@pytest.mark.parametrize("D,mode", LN_CASES)
def test_layernorm_closed_forms_equal_fp64_autograd(D, mode):
    x, w, b, dy, _ = RR.ln_inputs(ROWS, D, seed=D + mode)
    y, grads = _ln_autograd(x, w, b, dy, mode, torch.float64)
    ref_y, s_y = RR.ln_fwd(x, w, b, mode)
    assert RR.within(y, ref_y, s_y, tol=1e-12)
    ref = RR.ln_bwd(x, w, dy, mode)
    for k in ("dx", "dw", "db"):
        assert RR.within(grads[k], *ref[k], tol=1e-12), k


@pytest.mark.parametrize("E", [64, 256])
def test_head_closed_forms_equal_fp64_autograd(E):
    x1, x2, lw, lb, w, b, ds, scores = _head_case(E)
    ddot = ds.double() * scores.double() * (1 - scores.double())
    dot, grads = _head_autograd(x1, x2, lw, lb, w, b, ddot, torch.float64)
    ref_dot, s_dot = RR.head_dot(x1, x2, lw, lb, w, b)
    assert RR.within(dot, ref_dot, s_dot, tol=1e-12)
    s, bound = RR.head_fwd(x1, x2, lw, lb, w, b)
    assert torch.equal(s, torch.sigmoid(ref_dot)) and bool((bound >= 1e-7).all())
    ref = RR.head_bwd(x1, x2, lw, lb, w, scores, ds)
    for k in ("dx", "dlw", "dlb", "dw", "db"):
        assert RR.within(grads[k], *ref[k], tol=1e-12), k
    assert RR.within(grads["dx2"], *ref["dx"], tol=1e-12)


@pytest.mark.parametrize("D,mode", LN_CASES)
def test_layernorm_fp32_reference_is_inside_half_the_bound(D, mode):
    """torch's fp32 forward and autograd against the fp64 closed forms: |err| <= 1e-6 * S.  A failure here means S leaves out a
    term the value is made of."""
    for rows in FEW_ROWS:
        x, w, b, dy, _ = RR.ln_inputs(rows, D, seed=D + mode + rows)
        y, grads = _ln_autograd(x, w, b, dy, mode, torch.float32)
        tag = f"D={D} mode={mode} rows={rows}"
        assert RR.within(y, *RR.ln_fwd(x, w, b, mode), what=f"y {tag}", family="fp32-cpu-layernorm", tol=RR.TOL / 2)
        ref = RR.ln_bwd(x, w, dy, mode)
        for k in ("dx", "dw", "db"):
            assert RR.within(grads[k], *ref[k], what=f"{k} {tag}", family="fp32-cpu-layernorm", tol=RR.TOL / 2), k


@pytest.mark.parametrize("E", [64, 256])
def test_head_fp32_reference_is_inside_half_the_bound(E):
    """the same for the head, with the saved scores as an input of the backward (rowwise_ref's docstring says why)"""
    for rows in FEW_ROWS:
        x1, x2, lw, lb, w, b, ds, scores = _head_case(E, rows)
        dot, grads = _head_autograd(x1, x2, lw, lb, w, b, ds * scores * (1 - scores), torch.float32)
        tag = f"E={E} rows={rows}"
        assert RR.within(dot, *RR.head_dot(x1, x2, lw, lb, w, b), what=f"dot {tag}", family="fp32-cpu-head", tol=RR.TOL / 2)
        s, bound = RR.head_fwd(x1, x2, lw, lb, w, b)
        assert bool(((scores.double() - s).abs() <= bound).all())    # (1e-7 of it is the score's own rounding: not halved)
        ref = RR.head_bwd(x1, x2, lw, lb, w, scores, ds)
        for k in ("dx", "dlw", "dlb", "dw", "db"):
            assert RR.within(grads[k], *ref[k], what=f"{k} {tag}", family="fp32-cpu-head", tol=RR.TOL / 2), k


def test_zero_variance_rows_of_the_closed_forms():
    """LAYER: y == b and dx = (g - mean g) / sqrt(eps) on a constant row; CHAN: the dx term with 1 / std is dropped there (the
    kernel's guard), every value finite."""
    x, w, b, dy, _ = RR.ln_inputs(9, 64, seed=3)
    x[4] = 0.5
    y, _ = RR.ln_fwd(x, w, b, RR.NORM_LAYER)
    assert torch.equal(y[4], b.double())
    dx, s_dx = RR.ln_bwd(x, w, dy, RR.NORM_LAYER)["dx"]
    g = dy[4].double() * w.double()
    assert RR.within(dx[4], (g - g.mean()) / 1e-5 ** 0.5, s_dx[4], tol=1e-12)
    for k, (v, s) in RR.ln_bwd(x, w, dy, RR.NORM_CHAN).items():
        assert bool(torch.isfinite(v).all()) and bool(torch.isfinite(s).all()), k


def _rows_per_wave(rows):
    """acx_rows_per_wave of acx_train.hip restated: 16, halved while rows < 2048 * rpw (1 below 4096 rows, 2 below 8192, 4 below
    16384, 8 below 32768)"""
    rpw = 16
    while rpw > 1 and rows < 2048 * rpw:
        rpw //= 2
    return rpw


def test_row_parts_follows_the_rows_per_wave_rule():
    lib = L.lib()
    assert lib.acx_row_parts(0) == 0
    regimes = {}
    for rows in (1, 4095, 4096, 4097, 8191, 8192, 16383, 16384, 32767, 32768, 32785):
        rpw = _rows_per_wave(rows)
        regimes[rows] = rpw
        assert lib.acx_row_parts(rows) == -(-rows // (4 * rpw)), rows
    assert regimes == {1: 1, 4095: 1, 4096: 2, 4097: 2, 8191: 2, 8192: 4, 16383: 4, 16384: 8, 32767: 8, 32768: 16, 32785: 16}


@pytest.mark.parametrize("width", [96, 130, 1000, 192])
def test_row_width_outside_the_dispatch_is_refused_before_any_launch(width):
    """The five entry points that dispatch on the row width alone (acx_layernorm checks D % 64 itself): a width the kernels are not
    instantiated for is ACX_E_UNSUPPORTED with the width in acx_last_error -- 96 and 130 used to run the 64- and 128-wide kernels
    on rows of the wrong stride and return ACX_OK.  No device is needed: the refusal comes before the launch (with a launch the
    code would be ACX_E_HIP here, or ACX_OK on a GPU)."""
    lib = L.lib()
    buf = (C.c_float * 8192)()
    tab = (C.c_int32 * 8)()
    p, t = C.addressof(buf), C.addressof(tab)
    rows = 4
    calls = {
        "acx_layernorm_bwd": lambda: lib.acx_layernorm_bwd(None, p, p, p, p, p, rows, width, 1e-5, 0, 1.0, None, None),
        "acx_cls_head_bwd": lambda: lib.acx_cls_head_bwd(None, p, p, p, p, p, p, p, p, p, rows, width, None),
        "acx_cls_head": lambda: lib.acx_cls_head(None, p, p, p, p, p, p, p, rows, width, 1, 4, 0, None),
        "acx_cls_head_tiles": lambda: lib.acx_cls_head_tiles(None, p, p, p, p, p, p, p, rows, width, 1, 4, t, None),
        "acx_vit_embed": lambda: lib.acx_vit_embed(None, p, p, p, p, p, p, 1, 3, width, None),
    }
    for name, call in calls.items():
        lib.acx_layernorm(None, None, 0, None, None, None, 0, 0, 4, 64, 1e-5, 0, None)        # another text in the error slot
        assert b"null" in lib.acx_last_error(None)
        assert call() == -2, name                                                             # ACX_E_UNSUPPORTED
        msg = lib.acx_last_error(None)
        assert b"row width %d not in {64,128,256,512,640,768,1024}" % width in msg, (name, msg)
