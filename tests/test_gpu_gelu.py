"""-m gpu: the exact GELU (ACX_ACT_GELU = 5, nn.GELU) -- the device function itself, then every acx_gemm route that carries it,
element-wise against fp64.

A. acx_act modes 4 (forward) and 3 (derivative) on gelu_ref.sweep(), against F.gelu / its autograd derivative in fp64.  The yardstick
   is torch's own float32 CPU F.gelu on the same sweep (gelu_ref.yardstick, computed, not hard-coded); the device function may have
   at most twice its error: forward |err| <= 2 y_f max(|x|, 1), derivative |err| <= 2 y_g.
B. the route asserted with acx_gemm_route, then the product in poisoned, guarded buffers (tests/gemm_ref.py's operands).  Bound per
   element: gemm_ref.bound (2e-6 S for the f32-accurate products, no slope factor) plus the function-error term of A at the fp64
   pre-activation, 2 y_f max(|pre|, 1).
     gelu_grad_of:  C = acc * gelu'(p): |acc| 2 y_g for the function, and the product's 2e-6 S times max |gelu'| <= 1.13
     a_act:         every A element carries 2 y_f max(|a|, 1) into the product: sum_k (that) |w_k|
     plane outputs: the planes recombine to the f32 value within the split's round-off, 2^-22 |r| (bf16 triples: 24 bits; fp16
                    pairs: 22 bits) plus 2^-24 / c_scale for an fp16 lo plane that went subnormal
     pairs = 3 on bf16 planes is not f32-accurate: 3e-5 S, the bound of test_gemm_x6_three_products
   The K-panel plane layouts (ACX_BF16X3P, ACX_F16X2P: [N / 32][M][32]) exist for N % 32 == 0 only, so those two outputs run at
   (300, 288, 96) -- the last tile row still ends behind M, the second tile column is still ragged -- and (300, 264, 96) writes
   f32, bf16 rows and the row-major planes ACX_BF16X3."""
import ctypes as C
import dataclasses

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

import gelu_ref as R
import gemm_ref as G

DEV = "cuda"
ACT = L.ACT_GELU


def _h():
    return L.ctx(torch.cuda.current_device())


# ------------------------------------------------------------------------------------------------------------------ A. the function
@pytest.fixture(scope="module")
def device_sweep():
    x = R.sweep()
    pad = (-x.numel()) % 4
    xd = torch.cat([x, torch.zeros(pad)]).to(DEV)
    fwd = ops.act(xd, None, 4)[:x.numel()].cpu()
    grad = ops.act(xd, None, 3)[:x.numel()].cpu()
    return x, fwd, grad


def test_function_forward_within_twice_torch_cpu(device_sweep):
    x, y, _ = device_sweep
    yf, _ = R.yardstick()
    assert bool(torch.isfinite(y).all())
    ratio = ((y.double() - R.gelu64(x)).abs() / (yf * R.fwd_scale(x))).max().item()
    print(f"gelu forward: yardstick {yf * 2 ** 24:.2f} * 2^-24 * max(|x|, 1); device / yardstick = {ratio:.3f}")
    assert ratio <= R.MARGIN, ratio
    at = {float(v): y[x == v] for v in (-30.0, 1e4, 0.0)}
    assert bool((at[1e4] == 1e4).all())
    m30 = at[-30.0]
    assert bool(torch.signbit(m30).all()) and bool((m30.abs() < 2.0 ** -126).all()), m30       # -0.0 or a negative denormal
    assert bool((at[0.0] == 0.0).all())


def test_function_derivative_within_twice_torch_cpu(device_sweep):
    x, _, g = device_sweep
    _, yg = R.yardstick()
    assert bool(torch.isfinite(g).all())
    ratio = ((g.double() - R.gelu64_grad(x)).abs() / yg).max().item()
    print(f"gelu derivative: yardstick {yg * 2 ** 24:.2f} * 2^-24; device / yardstick = {ratio:.3f}")
    assert ratio <= R.MARGIN, ratio


def test_function_is_not_quickgelu(device_sweep):
    """the two activations differ by up to 2e-2: the sweep tells them apart by four orders of magnitude more than the bound"""
    x, y, _ = device_sweep
    assert ((y.double() - R.quick_gelu64(x)).abs().max().item()) > 1e-2
    with pytest.raises(L.AcxError, match="unknown mode"):
        ops.act(torch.zeros(4, device=DEV), None, 5)


# ------------------------------------------------------------------------------------------------------------------ B. f32 routes
def _scratch(c, d, t):
    if c.ws:
        t["ws"] = torch.full((c.ws_bytes // 4,), G.NAN32, dtype=torch.int32, device=DEV)
        d.workspace, d.workspace_bytes = t["ws"].data_ptr(), c.ws_bytes
    if c.ctr:
        t["ctr"] = torch.zeros(c.ctr, dtype=torch.int32, device=DEV)
        d.counters, d.n_counters = t["ctr"].data_ptr(), c.ctr


def _reference(c, t, mode):
    """(fp64 reference, per-element bound) of case c; mode: "act" (epilogue), "a_act" (A prologue), "grad" (gelu_grad_of)"""
    base = dataclasses.replace(c, act=G.NONE, res="")
    tt = dict(t)
    extra = 0.0
    if mode == "a_act":
        a64 = t["a"].double()
        tt["a"] = R.gelu64(a64)
        extra = R.fwd_term(a64)[:c.M] @ t["w"].double().abs().t()
    pre, S = G.evaluate(base, tt, torch.float64, magnitude=True)
    if mode == "grad":
        gp = R.gelu64_grad(t["p"])
        return pre * gp, G.EPS * S * 1.13 + pre.abs() * R.grad_term()
    r = R.gelu64(pre) if mode == "act" else pre
    b = G.EPS * S + (R.fwd_term(pre) if mode == "act" else extra)
    if c.res:
        r = r + t["res"].double()
        b = b + G.EPS * t["res"].double().abs()
    return r, b


def _f32_cases():
    S = G.t64(513, 768)
    return [
        ("sk-m1-n36", "act", G.Case("g", 1, 36, 256, act=ACT, expect=(G.R_SK, 1, 0, 2))),
        ("sk-pieces-3", "act", G.Case("g", 77, 512, 1536, act=ACT, ws=True, ctr=G.N_COUNTERS, expect=(G.R_SK, 3, G.RED_COUNTERS, 48))),
        ("sk-a-act-res", "a_act", G.Case("g", 154, 100, 512, res="own", expect=(G.R_SK, 1, 0, G.t32(154, 100)))),
        ("sk-gelu-grad", "grad", G.Case("g", 77, 512, 2048, act=ACT, expect=(G.R_SK, 1, 0, 48))),
        ("s64", "act", G.Case("g", 641, 708, 64, act=ACT, expect=(G.R_S64, 1, 0, G.t64(641, 708)))),
        ("s64-res", "act", G.Case("g", 641, 708, 64, act=ACT, res="own", expect=(G.R_S64, 1, 0, G.t64(641, 708)))),
        ("s64-split4", "act", G.Case("g", 513, 768, 1536, act=ACT, ws=True, expect=(G.R_S64, 4, G.RED_LAUNCH, S))),
        ("w8", "act", G.Case("g", 891, 382, 96, act=ACT, expect=(G.R_W8, 1, 0, 21))),
        ("w8-res", "act", G.Case("g", 891, 382, 96, act=ACT, res="own", expect=(G.R_W8, 1, 0, 21))),
        ("p256", "act", G.Case("g", 32763, 512, 32, act=ACT, expect=(G.R_P256, 1, 0, 1024))),
        ("generic-k60-res", "act", G.Case("g", 130, 70, 60, act=ACT, res="own", expect=(G.R_GEN, 1, 0, 2))),
        ("generic-asub-split2", "act", G.Case("g", 300, 200, 256, act=ACT, a_sub=True, ws=True, expect=(G.R_GEN, 2, G.RED_LAUNCH, 6))),
    ]


def _run_f32(c, mode):
    h = _h()
    t = G.operands(c, DEV)
    if mode == "grad":
        g = torch.Generator().manual_seed(5)
        t["p"] = (2.0 * torch.randn(c.M, c.N, generator=g)).to(DEV)
    r, b = _reference(c, t, mode)
    d = G.desc(c, t)
    if mode == "a_act":
        d.a_act = ACT
    if mode == "grad":
        d.gelu_grad_of, d.ldg = t["p"].data_ptr(), c.N
    _scratch(c, d, t)
    rc, got = G.query(h, d)
    assert rc == 0 and got == c.expect, ("got", G.ROUTE_NAMES[got[0]], got[1:], "want", G.ROUTE_NAMES[c.expect[0]], c.expect[1:])
    L.check(L.lib().acx_gemm(h, C.byref(d), torch.cuda.current_stream().cuda_stream), h)
    torch.cuda.synchronize()
    return t, r, b


@pytest.mark.parametrize("name,mode,c", _f32_cases(), ids=[n for n, _, _ in _f32_cases()])
def test_f32_routes_against_fp64(name, mode, c):
    assert torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count == G.NCU
    t, r, b = _run_f32(c, mode)
    out = t["c"]
    assert bool(torch.isfinite(out).all())
    ratio = ((out.double() - r).abs() / b).max().item()
    print(f"gelu-route-ratio {name} {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)
    assert G.guards_intact(t["c_buf"], c.M, c.N)
    if c.res == "own":
        assert G.guards_intact(t["res_buf"], c.M, c.N)
    if mode == "act":                                     # ... and it is this activation, not the other one
        other = dataclasses.replace(c, act=G.GELU)
        assert ((out.double() - G.evaluate(other, t)).abs() > b).any()
    if c.ctr:
        assert int(t["ctr"].abs().sum()) == 0
    if c.expect[1] > 1:                                   # a K split sums in a fixed order
        t2, _, _ = _run_f32(c, mode)
        assert torch.equal(out, t2["c"])


def test_gelu_grad_of_keeps_meaning_quickgelu_without_act():
    """act = 0 with gelu_grad_of: QuickGELU's derivative, as before; act = ACX_ACT_GELU: the exact one"""
    g = torch.Generator().manual_seed(3)
    a, w = torch.randn(77, 256, generator=g).to(DEV), (torch.randn(512, 256, generator=g) / 16).to(DEV)
    p = (2.0 * torch.randn(77, 512, generator=g)).to(DEV)
    acc = a.double() @ w.double().t()
    sg = torch.sigmoid(1.702 * p.double())
    quick = acc * sg * (1.0 + 1.702 * p.double() * (1.0 - sg))
    exact = acc * R.gelu64_grad(p)
    assert (ops.gemm(a, w, gelu_grad_of=p).double() - quick).abs().max() < 1e-4
    assert (ops.gemm(a, w, gelu_grad_of=p, act=ACT).double() - exact).abs().max() < 1e-4
    assert (quick - exact).abs().max() > 1e-2
    with pytest.raises(L.AcxError):
        ops.gemm(a, w, gelu_grad_of=p, act=L.ACT_QUICKGELU)


# ------------------------------------------------------------------------------------------------------------------ B. the plane kernel
def _x6_problem(M, N, K, seed=0):
    g = torch.Generator().manual_seed(1000 + M + 3 * N + 7 * K + seed)
    a = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 3, (M, 1), generator=g).float())
    w = torch.randn(N, K, generator=g) * K ** -0.5 + torch.arange(N).view(-1, 1) * 1e-4
    bias = torch.randn(N, generator=g)
    a, w, bias = a.to(DEV), w.to(DEV), bias.to(DEV)
    pre = a.double() @ w.double().t() + bias.double()
    S = a.double().abs() @ w.double().abs().t() + bias.double().abs()
    return a, w, bias, pre, S


def _guarded(M, N, dtype=torch.float32):
    buf = G._poison(M + 2, N, dtype, DEV)
    return buf, buf[:M]


def _route(rt):
    return (rt.route, rt.ksplit, rt.reduce, rt.tiles)


def _check(name, got64, pre, b):
    r = R.gelu64(pre)
    assert bool(torch.isfinite(got64).all()), name
    ratio = ((got64 - r).abs() / b).max().item()
    print(f"gelu-route-ratio x6-{name} {ratio:.4f}")
    assert ratio <= 1.0, (name, ratio)
    assert ((got64 - R.quick_gelu64(pre)).abs() > b).any(), name


def test_x6_pairs6_every_output():
    M, N, K = 300, 264, 96                                # the last tile of 256 rows ends behind M, the second tile column is ragged
    a, w, bias, pre, S = _x6_problem(M, N, K)
    a3, w3 = ops.split_bf16x3(a), ops.split_bf16x3(w)
    f = R.fwd_term(pre)
    rt = L.GemmRoute()
    buf, out = _guarded(M, N)
    ops.gemm_x6(a3, w3, out=out, bias=bias, act=ACT, route=rt)
    assert _route(rt) == (G.R_X6, 1, 0, 4)
    _check("f32", out.double(), pre, G.EPS * S + f)
    assert G.guards_intact(buf, M, N)
    bufb, outb = _guarded(M, N, torch.bfloat16)
    ops.gemm_x6(a3, w3, out=outb, bias=bias, act=ACT, route=rt)
    assert _route(rt) == (G.R_X6, 1, 0, 4)
    _check("bf16", outb.double(), pre, G.EPS * S + f + 2.0 ** -8 * R.gelu64(pre).abs())
    assert G.guards_intact(bufb, M, N)
    assert torch.equal(outb, out.bfloat16())              # the same f32 epilogue value, rounded once
    p3 = ops.gemm_x6(a3, w3, bias=bias, act=ACT, planes_out=True, route=rt)          # ACX_BF16X3: row-major planes
    assert _route(rt) == (G.R_X6, 1, 0, 4) and p3.shape == (3, M, N)
    assert torch.equal(p3.float().sum(0), out) and torch.equal(p3[0], out.bfloat16())   # the planes ARE the f32 value, hi first
    # ACX_BF16X3P: K-panel planes, N % 32 == 0
    M, N, K = 300, 288, 96
    a, w, bias, pre, S = _x6_problem(M, N, K)
    a3, w3 = ops.split_bf16x3(a), ops.split_bf16x3(w)
    pp = G._poison(3 * M, N, torch.bfloat16, DEV).view(3, M, N)
    ops.gemm_x6(a3, w3, out=pp, bias=bias, act=ACT, planes_out=True, panel_out=True, route=rt)
    assert _route(rt) == (G.R_X6, 1, 0, 4)
    rec = ops.unpanel(pp).double().sum(0)
    _check("bf16x3p", rec, pre, G.EPS * S + R.fwd_term(pre) + 2.0 ** -22 * R.gelu64(pre).abs())
    assert torch.equal(rec.float(), ops.gemm_x6(a3, w3, bias=bias, act=ACT))


def test_x6_pairs3_bf16_and_fp16_planes():
    M, N, K = 300, 264, 96
    a, w, bias, pre, S = _x6_problem(M, N, K, seed=1)
    rt = L.GemmRoute()
    buf, out = _guarded(M, N)
    ops.gemm_x6(ops.split_bf16x3(a), ops.split_bf16x3(w), out=out, bias=bias, act=ACT, pairs=3, route=rt)
    assert _route(rt) == (G.R_X6, 1, 0, 4)
    _check("pairs3-bf16", out.double(), pre, 3e-5 * S + R.fwd_term(pre))
    assert G.guards_intact(buf, M, N)
    # fp16 pair planes of s a and of 2^10 w; out_scale undoes both
    s, ws = 64.0, 1024.0
    a2, w2 = ops.split_f16x2(a, panel=True, scale=s), ops.split_f16x2(w, panel=True, scale=ws)
    buf, out = _guarded(M, N)
    ops.gemm_x6(a2, w2, out=out, bias=bias, act=ACT, pairs=3, out_scale=1.0 / (s * ws), panels=3, route=rt)
    assert _route(rt) == (G.R_X6, 1, 0, 4)
    _check("pairs3-f16", out.double(), pre, G.EPS * S + R.fwd_term(pre))
    assert G.guards_intact(buf, M, N)
    # ... to fp16 pair planes of c_scale * gelu(.) (ACX_F16X2P: K-panel layout, N % 32 == 0)
    M, N, K = 300, 288, 96
    a, w, bias, pre, S = _x6_problem(M, N, K, seed=1)
    a2, w2 = ops.split_f16x2(a, panel=True, scale=s), ops.split_f16x2(w, panel=True, scale=ws)
    cs = 2.0 ** -3
    kw = dict(bias=bias, act=ACT, pairs=3, out_scale=1.0 / (s * ws), panels=3)
    hp = ops.gemm_x6(a2, w2, planes_out=True, panel_out=True, c_scale=cs, route=rt, **kw)
    assert _route(rt) == (G.R_X6, 1, 0, 4) and hp.dtype == torch.float16 and hp.shape == (2, M, N)
    rec = ops.unpanel(hp).double().sum(0) / cs
    r = R.gelu64(pre)
    _check("pairs3-f16x2p", rec, pre, G.EPS * S + R.fwd_term(pre) + 2.0 ** -22 * r.abs() + 2.0 ** -24 / cs)
    hf = ops.gemm_x6(a2, w2, split_k=False, **kw)
    want = ops.split_f16x2(hf, panel=True, scale=cs)      # the planes are the split of c_scale * (the f32 epilogue value)
    assert torch.equal(hp[0], want[0]) and torch.equal(hp[1], want[1])


def test_x6_strips_bit_identical_to_whole_tiles():
    """130 x 2 tiles on 256 CUs: a last round of 4 tiles goes out as strips (64 columns by the cost model, 128 forced)"""
    assert torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count == G.NCU
    M, N, K = 256 * 130, 512, 32
    a, w, bias, pre, S = _x6_problem(M, N, K, seed=2)
    a3, w3 = ops.split_bf16x3(a), ops.split_bf16x3(w)
    dev = torch.cuda.current_device()
    before = ops.get_option(dev, L.OPT_X6_STRIP_TAIL)
    res = {}
    rt = L.GemmRoute()
    try:
        for mode in (0, 1, 2):
            ops.set_x6_strip_tail(dev, mode)
            res[mode] = (ops.gemm_x6(a3, w3, bias=bias, act=ACT, route=rt),
                         ops.gemm_x6(a3, w3, bias=bias, act=ACT, planes_out=True, panel_out=True))
            assert _route(rt) == (G.R_X6, 1, 0, 260)
    finally:
        ops.set_x6_strip_tail(dev, before)
    _check("strips", res[1][0].double(), pre, G.EPS * S + R.fwd_term(pre))
    for mode in (1, 2):
        assert torch.equal(res[mode][0], res[0][0]) and torch.equal(res[mode][1], res[0][1]), mode
    assert torch.equal(ops.unpanel(res[1][1]).float().sum(0), res[1][0])


def test_x6_k_split_epilogue_in_the_reduce_launch():
    M, N, K = 256, 256, 3072
    a, w, bias, pre, S = _x6_problem(M, N, K, seed=3)
    a3, w3 = ops.split_bf16x3(a), ops.split_bf16x3(w)
    rt = L.GemmRoute()
    buf, out = _guarded(M, N)
    ops.gemm_x6(a3, w3, out=out, bias=bias, act=ACT, route=rt)      # (brings the workspace acx_gemm_scratch asks for)
    assert rt.route == G.R_X6 and rt.ksplit > 1 and rt.reduce == G.RED_LAUNCH and rt.tiles == 1, _route(rt)
    _check("ksplit", out.double(), pre, G.EPS * S + R.fwd_term(pre))
    assert G.guards_intact(buf, M, N)
    again = ops.gemm_x6(a3, w3, bias=bias, act=ACT)
    assert torch.equal(again, out)
    p3 = ops.gemm_x6(a3, w3, bias=bias, act=ACT, planes_out=True, panel_out=True, route=rt)
    assert rt.ksplit > 1
    assert torch.equal(ops.unpanel(p3).float().sum(0), out)
    ob = ops.gemm_x6(a3, w3, bias=bias, act=ACT, out_dtype=torch.bfloat16, route=rt)
    assert rt.ksplit > 1 and torch.equal(ob, out.bfloat16())


# ------------------------------------------------------------------------------------------------------------------ B. refusals
@pytest.mark.parametrize("c,text", [
    (G.Case("bf16-mfma", 130, 72, 64, prec=G.BF16, a_bf16=True, act=ACT, refuse=G.E_UNSUPPORTED), "ACX_ACT_GELU needs an f32 product"),
    (G.Case("conv3x3", 128, 72, 288, amap=G.CONV, gn=16, gl=8, cin=32, act=ACT, refuse=G.E_UNSUPPORTED), "ACX_ACT_GELU runs on identity rows"),
], ids=["bf16-mfma", "conv3x3"])
def test_gemm_refusals_write_nothing(c, text):
    h, lib = _h(), L.lib()
    t = G.operands(c, DEV)
    d = G.desc(c, t)
    if c.amap == G.CONV:
        t["zero"] = torch.zeros(256, dtype=torch.float32, device=DEV)
        d.zero_page = t["zero"].data_ptr()
    rc, got = G.query(h, d)
    assert rc == c.refuse and got == (G.R_NONE, 1, 0, 0), (rc, got)
    assert text.encode() in lib.acx_last_error(h)
    assert lib.acx_gemm(h, C.byref(d), torch.cuda.current_stream().cuda_stream) == c.refuse
    assert text.encode() in lib.acx_last_error(h)
    torch.cuda.synchronize()
    assert G.guards_intact(t["c_buf"], 0, 0)


def test_vit_desc_unknown_act_is_refused():
    from anomalyclip_amd import init_weights as IW
    from anomalyclip_amd.components.clip_vit import VisionTransformer
    g = IW.TINY
    enc = VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim,
                            precision="f32").to(DEV).eval()
    w, _keep = enc._weights(L.PREC_F32)
    h, lib = _h(), L.lib()
    frames = torch.randn(2, 3, g.image_resolution, g.image_resolution, device=DEV)
    out = G._poison(2, g.embed_dim, torch.float32, DEV)
    for act, prec, code, text in ((9, L.PREC_F32, G.E_BADARG, b"act must be"), (ACT, L.PREC_BF16, G.E_UNSUPPORTED, b"ACX_ACT_GELU with ACX_PREC_BF16")):
        d = L.VitDesc(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim, prec, act)
        nbytes = lib.acx_vit_workspace_bytes(C.byref(d), 2)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        rc = lib.acx_vit_encode(h, C.byref(d), C.byref(w), frames.data_ptr(), 2, out.data_ptr(), ws.data_ptr(), nbytes,
                                torch.cuda.current_stream().cuda_stream)
        assert rc == code and text in lib.acx_last_error(h), (rc, lib.acx_last_error(h))
    torch.cuda.synchronize()
    assert G.guards_intact(out, 0, 0)
