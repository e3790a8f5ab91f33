"""Test infrastructure for the row-wise kernels (LayerNorm / ChanLayerNorm forward and backward, the classifier head forward and
backward, the ViT embedding): their closed forms in fp64, each with the term magnitude S its error is judged against, and the
seeded inputs of the sweeps (per-row scales 2^k, so that an error in a small row is not hidden by the tensor's largest).

The tolerance is the project's fp32 bound, element by element:  |err| <= TOL * S  with TOL = 2e-6, S = the sum of the absolute
values of the terms the element is made of.

Where TOL comes from: torch's own fp32 CPU evaluation of the same operations on these inputs, measured against the fp64 closed
forms below (tests/test_cpu_rowwise.py repeats the measurement on small shapes and asserts half the bound):

    worst |err| / S of an fp32 CPU evaluation, rows in {777, 8195}
      LayerNorm / ChanLayerNorm backward (autograd), widths 64, 640, 1024:    dx 2.8e-7   dw 4.5e-8   db 4.8e-8
        the same at 1 and 3 rows, all seven widths:                           dx 1.8e-7   dw 2.6e-7   db 1.1e-7
      LayerNorm / ChanLayerNorm forward, widths 64, 640, 1024:                y  4.9e-7
      classifier head backward (scores as an input), widths 64, 256, 640, 1024:
                                                                              dx 3.0e-7   dlw 6.7e-8   dlb 5.1e-8   dw 1.6e-7   db 1.9e-8
      classifier head forward (pre-sigmoid sum), same shapes:                 1.1e-7

so 2e-6 leaves 4x to 7x over a correct fp32 evaluation.  The kernels' own ratios are recorded in DESIGN.md section 3; the bound
is never set from them.

The head's backward takes the saved fp32 scores as an INPUT (ddot = dscores * s * (1 - s) with s as handed to the kernel): 1 - s
of a saturated s carries a relative error of eps / (1 - s), so a reference that differentiates through its own sigmoid disagrees
with any fp32 evaluation by far more than the bound without either being wrong."""
import torch

TOL = 2e-6
WIDTHS = (64, 128, 256, 512, 640, 768, 1024)          # the widths the dispatch takes
NORM_LAYER, NORM_CHAN = 0, 1                          # == include/acx.h ACX_NORM_LAYER / ACX_NORM_CHAN
HEAD_EPS = 1e-5                                       # the classifier head's LayerNorm (nn.LayerNorm default)


# ------------------------------------------------------------------------------------------------------------- inputs
def row_scales(rows, g):
    """2^k per row, k uniform in -6..6"""
    return torch.exp2(torch.randint(-6, 7, (rows, 1), generator=g).float())


def ln_inputs(rows, D, seed):
    """x (offset 0.3, spread 2, per-row scale), w, b, dy (per-row scale), add -- f32 CPU tensors"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(rows, D, generator=g) * 2 + 0.3) * row_scales(rows, g)
    w, b = torch.randn(D, generator=g), torch.randn(D, generator=g)
    dy = torch.randn(rows, D, generator=g) * row_scales(rows, g)
    add = torch.randn(rows, D, generator=g)
    return x, w, b, dy, add


def head_inputs(rows, E, seed):
    """x1, x2 (per-row scale), LayerNorm weight / bias, the Linear(E, 1) weight [1, E] scaled by E^-0.5 and bias [1],
    dscores (per-row scale) -- f32 CPU tensors"""
    g = torch.Generator().manual_seed(seed)
    sc = row_scales(rows, g)
    x1 = (torch.randn(rows, E, generator=g) * 2 + 0.3) * sc
    x2 = (torch.randn(rows, E, generator=g) * 2 + 0.3) * sc
    lw, lb = torch.randn(E, generator=g), torch.randn(E, generator=g)
    w, b = torch.randn(1, E, generator=g) * E ** -0.5, torch.randn(1, generator=g)
    ds = torch.randn(rows, generator=g) * row_scales(rows, g).view(-1)
    return x1, x2, lw, lb, w, b, ds


# ------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_stats(x, eps, mode):
    """v = x - mean, av = |x| + |mean| (the terms of v, see ln_fwd), sc (y = v * sc * w + b), c2 (the factor of mean(g v) v in dx);
    zero-variance rows: c2 = sc^3 (LAYER), 0 (CHAN: the kernel's guard, the limit does not exist)"""
    mean = x.mean(-1, keepdim=True)
    v = x - mean
    av = x.abs() + mean.abs()
    var = (v * v).mean(-1, keepdim=True)
    if mode == NORM_LAYER:
        sc = 1.0 / torch.sqrt(var + eps)
        c2 = sc ** 3
    else:
        sd = var.sqrt()
        sc = 1.0 / (sd + eps)
        c2 = torch.where(sd > 0, sc * sc / sd, torch.zeros_like(sd))
    return v, av, sc, c2


def ln_fwd(x, w, b, mode, eps=1e-5, dtype=torch.float64):
    """(y, S_y):  y = (x - mean) * sc * w + b,  S_y = (|x| + |mean|) * sc * |w| + |b|.
    The terms of v = x - mean are counted one by one (av = |x| + |mean| stands where |v| would): |v * sc * w| + |b| is NOT a bound a
    correct fp32 evaluation keeps -- the mean carries its own rounding (about 2^-24 |mean|), so an element with x close to the mean
    and a small b has an error far above 2^-24 |v|.  torch's fp32 CPU LayerNorm misses 1e-6 * (|v sc w| + |b|) by up to 29x on
    these inputs (777 rows of 1024) and keeps the form used here with the margin quoted in the module docstring.  The same holds
    for every S below that multiplies by v without summing many rows: dw of one row is dy * v * sc, and torch's fp32 autograd misses
    1e-6 * |dy v sc| by 113x there (tests/test_cpu_rowwise.py holds the forms at 1 and 3 rows)."""
    x, w, b = x.to(dtype), w.to(dtype), b.to(dtype)
    v, av, sc, _ = _ln_stats(x, eps, mode)
    return v * sc * w + b, av * sc * w.abs() + b.abs()


def ln_bwd(x, w, dy, mode, eps=1e-5, dtype=torch.float64):
    """{"dx": (dx, S_dx), "dw": (dw, S_dw), "db": (db, S_db)} with g = dy * w:
    dx = sc (g - mean g) - c2 mean(g v) v       S_dx = sc (|g| + mean|g|) + c2 mean|g v| |v|
    dw = sum_rows dy v sc                       S_dw = sum_rows |dy| av sc          (av = |x| + |mean|: the terms of v)
    db = sum_rows dy                            S_db = sum_rows |dy|"""
    x, w, dy = x.to(dtype), w.to(dtype), dy.to(dtype)
    v, av, sc, c2 = _ln_stats(x, eps, mode)
    dw, s_dw = (dy * v * sc).sum(0), (dy.abs() * av * sc).sum(0)
    db, s_db = dy.sum(0), dy.abs().sum(0)
    del av
    g = dy * w
    gv = g * v
    dx = sc * (g - g.mean(-1, keepdim=True)) - c2 * gv.mean(-1, keepdim=True) * v
    s_dx = sc * (g.abs() + g.abs().mean(-1, keepdim=True)) + c2 * gv.abs().mean(-1, keepdim=True) * v.abs()
    return {"dx": (dx, s_dx), "dw": (dw, s_dw), "db": (db, s_db)}


# ------------------------------------------------------------------------------------------------------------- classifier head
def _head_rows(x1, x2, lw, lb):
    """v, rstd, xh = v rstd, z = xh lw + lb, and the magnitudes of the terms of xh and of z (|a| + |mean| stands where |v| would)"""
    a = (x1 + x2) * 0.5
    mean = a.mean(-1, keepdim=True)
    v = a - mean
    rstd = 1.0 / torch.sqrt((v * v).mean(-1, keepdim=True) + HEAD_EPS)
    xh = v * rstd
    s_xh = (a.abs() + mean.abs()) * rstd
    return v, rstd, xh, xh * lw + lb, s_xh, s_xh * lw.abs() + lb.abs()


def head_fwd(x1, x2, lw, lb, w, b, dtype=torch.float64):
    """(scores, bound) of s = sigmoid(sum_e z_e w_e + b), z = LN((x1 + x2) / 2) lw + lb; the error of the pre-sigmoid sum is at most
    TOL * (sum_e |z_e w_e| + |b|), the sigmoid's slope s (1 - s) carries it to the score, 1e-7 is the score's own rounding."""
    x1, x2, lw, lb, w, b = (t.to(dtype) for t in (x1, x2, lw, lb, w, b))
    zw = _head_rows(x1, x2, lw, lb)[3] * w.view(-1)
    s = torch.sigmoid(zw.sum(-1) + b)
    return s, TOL * (zw.abs().sum(-1) + b.abs()) * s * (1 - s) + 1e-7


def head_dot(x1, x2, lw, lb, w, b, dtype=torch.float64):
    """(pre-sigmoid sum, S): what the 1e-6 * S reference check is made on"""
    x1, x2, lw, lb, w, b = (t.to(dtype) for t in (x1, x2, lw, lb, w, b))
    zw = _head_rows(x1, x2, lw, lb)[3] * w.view(-1)
    return zw.sum(-1) + b, zw.abs().sum(-1) + b.abs()


def head_bwd(x1, x2, lw, lb, w, scores, dscores, dtype=torch.float64):
    """{"dx", "dlw", "dlb", "dw", "db"} -> (value, S) from the scores AS GIVEN: ddot = dscores s (1 - s), dz = ddot w,
    xh = v rstd, z = xh lw + lb, g = dz lw:
    dx  = (rstd (g - mean g) - rstd^3 mean(g v) v) / 2  (of x1 and of x2)
    dlw = sum_rows dz xh  (S: |dz| S_xh)    dlb = sum_rows dz    dw = sum_rows ddot z  (S: |ddot| (S_xh |lw| + |lb|))    db = sum_rows ddot
    with S_xh = (|a| + |mean|) rstd, a = (x1 + x2) / 2"""
    x1, x2, lw, lb, w, s, ds = (t.to(dtype) for t in (x1, x2, lw, lb, w, scores, dscores))
    w = w.view(-1)
    v, rstd, xh, z, s_xh, s_z = _head_rows(x1, x2, lw, lb)
    ddot = (ds * s * (1 - s)).view(-1, 1)
    dz = ddot * w
    g = dz * lw
    gv = g * v
    dx = 0.5 * (rstd * (g - g.mean(-1, keepdim=True)) - rstd ** 3 * gv.mean(-1, keepdim=True) * v)
    s_dx = 0.5 * (rstd * (g.abs() + g.abs().mean(-1, keepdim=True)) + rstd ** 3 * gv.abs().mean(-1, keepdim=True) * v.abs())
    return {"dx": (dx, s_dx),
            "dlw": ((dz * xh).sum(0), (dz.abs() * s_xh).sum(0)),
            "dlb": (dz.sum(0), dz.abs().sum(0)),
            "dw": ((ddot * z).sum(0), (ddot.abs() * s_z).sum(0)),
            "db": (ddot.sum(0), ddot.abs().sum(0))}


# ------------------------------------------------------------------------------------------------------------- comparison
def ratio(out, ref, S):
    """worst |out - ref| / S over the elements with S > 0 (an element with S == 0 must be exact: reported as inf otherwise)"""
    err = (torch.as_tensor(out).detach().double().cpu() - ref.double()).abs()
    S = S.double().expand_as(err)
    r = torch.where(S > 0, err / S.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, float("inf")), torch.zeros_like(err)))
    return float(r.max()) if r.numel() else 0.0


def within(out, ref, S, what="", family=None, tol=TOL):
    """|out - ref| <= tol * S element by element; prints the worst ratio first (family: the tag the recorded ratios are grouped by)"""
    r = ratio(out, ref, S)
    if family:
        print(f"ROWWISE_RATIO {family} {what} {r:.3e}")
    return bool(torch.isfinite(torch.as_tensor(out)).all()) and r <= tol
