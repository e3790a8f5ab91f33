"""-m gpu: precision "auto"'s mixed mode (ACX_PREC_F32X6_LN16) -- the ViT's LayerNorm-fed products as three-product GEMMs of fp16
planes.  Kernel level against fp64 (LayerNorm -> scaled fp16 planes -> in-projection to f32 rows, c_fc + QuickGELU to bf16 planes), the
planes' bits, the LayerNorm rider's fp16 store against the stand-alone kernel's, and the model against precision "f32x6"."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components import clip_vit as V
import gemm_ref as G

DEV = "cuda"
WSCALE = 1024.0

# (M, N, K): an edge tile with one K-step pair; strips; the in-projection of an 8-frame ViT-B/16 launch
SHAPES = [(300, 256, 64), (520, 768, 768), (8 * 197, 2304, 768)]


def _inputs(M, N, K, wild):
    """x rows of mixed scale; wild: gamma columns spanning 2^-12 ... 2^3 and one massive-activation column in x"""
    g = torch.Generator().manual_seed(1000 * M + N + K + int(wild))
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())
    gamma = 1.0 + 0.2 * torch.randn(K, generator=g)
    beta = 0.3 * torch.randn(K, generator=g)
    if wild:
        gamma = torch.exp2(torch.randint(-12, 4, (K,), generator=g).float()) * torch.where(torch.rand(K, generator=g) < 0.5, -1.0, 1.0)
        x[:, K // 3] += 400.0
    w1, w2 = torch.randn(N, K, generator=g) * K ** -0.5, torch.randn(N, K, generator=g) * K ** -0.5
    b1, b2 = torch.randn(N, generator=g) * 0.5, torch.randn(N, generator=g) * 0.5
    return x, gamma, beta, w1, b1, w2, b2


def _reference(x, gamma, beta, w1, b1, w2, b2, dtype):
    """(in-projection, QuickGELU(c_fc), their magnitudes S = sum_k |a||w| + |bias|) in `dtype`"""
    y = torch.nn.functional.layer_norm(x.to(dtype), (x.shape[1],), gamma.to(dtype), beta.to(dtype), 1e-5)
    o1 = y @ w1.to(dtype).t() + b1.to(dtype)
    o2 = G.quick_gelu(y @ w2.to(dtype).t() + b2.to(dtype))
    return o1, o2, y.abs() @ w1.to(dtype).abs().t() + b1.to(dtype).abs(), y.abs() @ w2.to(dtype).abs().t() + b2.to(dtype).abs()


_REF = {}


def _ref(M, N, K, wild):
    key = (M, N, K, wild)
    if key not in _REF:
        t = _inputs(M, N, K, wild)
        _REF[key] = (t, _reference(*t, torch.float64), _reference(*t, torch.float32)[:2])
    return _REF[key]


@pytest.mark.parametrize("wild", [False, True], ids=["plain", "wild-gamma"])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_chain_against_fp64(M, N, K, wild):
    """|err| <= 2e-6 S (x 1.5 behind QuickGELU; tests/gemm_ref.py), S = sum_k |a||w| + |bias| with a the fp64 LayerNorm output -- first for
    torch's fp32 evaluation on the CPU, then for the kernels.  K = 768: acx_layernorm_scaled writes the planes (the LayerNorm's fp16 store is
    built for the ViT width); K = 64: the f32 LayerNorm rows times s through acx_split_f16x2, the same two planes.  The bf16 output planes
    sum to the f32 value of the epilogue: hi + mid + lo is exact, checked bit for bit against the f32-output launch of the same product."""
    (x, gamma, beta, w1, b1, w2, b2), (r1, r2, S1, S2), (f1, f2) = _ref(M, N, K, wild)
    bd1, bd2 = G.EPS * S1, 1.5 * G.EPS * S2
    assert ((f1.double() - r1).abs() <= bd1).all() and ((f2.double() - r2).abs() <= bd2).all()      # torch fp32 stays inside
    s = V.ln16_scale(float((gamma.abs() * (K - 1) ** 0.5 + beta.abs()).max()))
    assert s is not None
    xd, gd, bed = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    if K == 768:
        a2 = ops.layernorm_f16x2(xd, gd, bed, s)
    else:
        a2 = ops.split_f16x2(ops.layernorm(xd, gd, bed) * s, panel=True)
    assert torch.isfinite(a2.float()).all() and float(a2[0].float().abs().max()) <= 2.0 ** 14 * (1 + 2.0 ** -10)
    w1p, w2p = ops.split_f16x2(w1.to(DEV), panel=True, scale=WSCALE), ops.split_f16x2(w2.to(DEV), panel=True, scale=WSCALE)
    osc = 1.0 / (WSCALE * s)
    o1 = ops.gemm_x6(a2, w1p, panels=3, pairs=3, out_scale=osc, bias=b1.to(DEV))
    e1 = (o1.double().cpu() - r1).abs()
    print(f"in-proj {M}x{N}x{K} wild={wild} s={s}: max err / bound = {float((e1 / bd1).max()):.3f}")
    assert (e1 <= bd1).all()
    p3 = ops.gemm_x6(a2, w2p, panels=3, pairs=3, out_scale=osc, bias=b2.to(DEV), act=L.ACT_QUICKGELU, planes_out=True, panel_out=True,
                     planes_bf16=True)
    assert p3.dtype == torch.bfloat16 and p3.shape == (3, M, N)
    o2 = ops.unpanel(p3).float().sum(0)                    # (three bf16 planes of one f32 value: the sum is exact)
    e2 = (o2.double().cpu() - r2).abs()
    print(f"c_fc {M}x{N}x{K} wild={wild}: max err / bound = {float((e2 / bd2).max()):.3f}")
    assert (e2 <= bd2).all()
    o2f = ops.gemm_x6(a2, w2p, panels=3, pairs=3, out_scale=osc, bias=b2.to(DEV), act=L.ACT_QUICKGELU)
    assert torch.equal(o2, o2f)                           # the planes ARE the f32 epilogue value, bit for bit
    hi = ops.unpanel(p3)[0].float()
    assert torch.equal(hi, o2f.bfloat16().float())        # ... split hi first: hi = bf16(value)


@pytest.mark.parametrize("D", [768, 1024])
def test_layernorm_planes_are_the_split_of_the_scaled_rows(D):
    """acx_layernorm_scaled's planes hold s * y to max(2^-22 |y|, 2^-25 / s) per element (the fp16 pair's 22 bits; the lo plane's smallest
    step) -- judged against acx_layernorm's f32 rows, which may differ from the plane kernel's y by one f32 rounding (2^-23 |y|: another
    kernel, another contraction); s = 1 is acx_layernorm's own ACX_F16X2P output bit for bit.  Odd row count:
    the last row pair is half empty."""
    g = torch.Generator(device=DEV).manual_seed(3 + D)
    x = torch.randn(1001, D, generator=g, device=DEV) * 3.0
    lw, lb = torch.randn(D, generator=g, device=DEV), torch.randn(D, generator=g, device=DEV)
    y = ops.layernorm(x, lw, lb).double()
    for s in (2.0 ** -3, 1.0, 64.0, 512.0):
        pl = ops.unpanel(ops.layernorm_f16x2(x, lw, lb, s)).double()
        err = ((pl[0] + pl[1]) / s - y).abs()
        assert (err <= torch.maximum(2.0 ** -22 * y.abs(), torch.full_like(y, 2.0 ** -25 / s)) + 2.0 ** -23 * y.abs()).all(), s
    y1 = torch.empty(2, 1001, D, dtype=torch.float16, device=DEV)
    hh = ops._h(x)
    L.check(L.lib().acx_layernorm(hh, x.data_ptr(), D, lw.data_ptr(), lb.data_ptr(), y1.data_ptr(), D, L.F16X2P, 1001, D, 1e-5, 0,
                                  ops._stream()), hh)
    assert torch.equal(y1, ops.layernorm_f16x2(x, lw, lb, 1.0))
    h = ops._h(x)
    assert L.lib().acx_layernorm_scaled(h, x.data_ptr(), D, lw.data_ptr(), lb.data_ptr(), x.data_ptr(), 8, D, 1e-5, 0, 3.0, None) != 0


# (name, M, N, K, rides): the shapes of tests/test_gpu_ln_rider.py
RIDER_CASES = [("bench out-proj", 512 * 197, 768, 768, True), ("bench c_proj", 512 * 197, 768, 3072, True),
               ("256 frames", 256 * 197, 768, 768, True), ("ViT-L/14", 300 * 257, 1024, 1024, True),
               ("exact rounds", 256 * 256, 768, 768, False), ("few tiles", 2048, 768, 768, False),
               ("edge tile", 100000, 768, 768, True)]


@pytest.mark.parametrize("name,M,N,K,rides", RIDER_CASES, ids=[c[0] for c in RIDER_CASES])
def test_rider_fp16_planes_bit_identical(name, M, N, K, rides):
    """acx_gemm_ln with an ACX_F16X2P job (the planes of s * LayerNorm riding in the residual product's last round) against acx_gemm followed by
    acx_layernorm_scaled: torch.equal on x and on both planes, with the cost model's rows, with every completed row riding, and switched off.
    The host plan lets rows ride on the shapes where it does for bf16 jobs (that fp16 jobs take the riding launch shows in the kernel table
    of profiles/ln16_ab.txt; the bits are the same either way, which is what this test holds).  Where N == K the fp16 planes are written INTO the product's A planes (the hi and mid planes of the
    bf16 triple, as ln_2 does behind out-proj in the model: the riders write plane rows the last round's tiles do not read)."""
    dev = torch.cuda.current_device()
    ncu = ops.x6_workgroups(dev)
    ride, ready = ops.ln_rider_plan(M, N, K, ncu)
    print(f"{name}: {M} x {N} x {K} on {ncu} workgroups: {ride} of {ready} completed rows ride")
    if ncu == 256:
        assert (ride > 0) == rides and (ready > 0) == rides, (name, ride, ready)
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g, device=DEV) * torch.exp2(torch.randint(-4, 4, (M, 1), generator=g, device=DEV).float())
    a3 = ops.split_bf16x3(a, panel=True)
    del a
    w3 = ops.split_bf16x3(torch.randn(N, K, generator=g, device=DEV) * 0.05, panel=True)
    bias = torch.randn(N, generator=g, device=DEV)
    x = torch.randn(M, N, generator=g, device=DEV) * 3.0
    lw, lb = torch.randn(N, generator=g, device=DEV), torch.randn(N, generator=g, device=DEV)
    s = 128.0
    x_ref = x.clone()
    ops.gemm_x6(a3, w3, panels=3, bias=bias, residual=x_ref, out=x_ref)
    y_ref = ops.layernorm_f16x2(x_ref, lw, lb, s)
    try:
        for mode in (1, 10 ** 9, 0):
            ops.set_ln_rider(dev, mode)
            x2 = x.clone()
            if N == K:                                        # the job's planes alias the product's A planes (their hi and mid plane)
                a3c = a3.clone()
                y2 = a3c.view(torch.float16)[:2]
                ops.gemm_x6(a3c, w3, panels=3, bias=bias, residual=x2, out=x2, ln=(lw, lb, y2, s))
            else:
                y2 = torch.full((2, M, N), 7.0, dtype=torch.float16, device=DEV)
                ops.gemm_x6(a3, w3, panels=3, bias=bias, residual=x2, out=x2, ln=(lw, lb, y2, s))
            assert torch.equal(x2, x_ref), (name, mode, "x")
            for p, pl in enumerate(("hi", "lo")):
                assert torch.equal(y2[p], y_ref[p]), (name, mode, pl)
    finally:
        ops.set_ln_rider(dev, 1)


def _vit(sd, precision):
    geom = IW.VIT_B16
    vit = V.VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers, geom.vision_heads,
                              geom.embed_dim, precision=precision)
    vit.load_state_dict(sd, strict=True)
    return vit.to(DEV)


def _relerr(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _state(kind):
    sd = IW.init_vit_state_dict(IW.VIT_B16, 11, prefix="")
    if kind == "affine":                                    # gamma / beta drawn in 0.1 ... 5 (random signs on beta)
        g = torch.Generator().manual_seed(12)
        for k in sd:
            if ".ln_1." in k or ".ln_2." in k:
                v = 0.1 + 4.9 * torch.rand(sd[k].shape, generator=g)
                sd[k] = v if k.endswith("weight") else v * torch.where(torch.rand(v.shape, generator=g) < 0.5, -1.0, 1.0)
    if kind == "gate-fails":
        sd["transformer.resblocks.4.mlp.c_fc.weight"][7, 9] = 100.0
    return sd


@pytest.mark.parametrize("kind", ["init", "affine"])
def test_model_mixed_against_f32x6(kind):
    """ViT-B/16, 8 and 32 frames: "auto" resolves to the mixed mode and stays within 5e-6 (relative to the largest feature) of "f32x6" --
    the bound the f16x3 mode is held to; identical frames give bit-identical rows in every slot."""
    sd = _state(kind)
    mixed, six = _vit(sd, "auto"), _vit(sd, "f32x6")
    assert mixed.ln16_resolution() is not None and len(mixed.ln16_resolution()) == 24
    frames = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(5)) * 0.8
    idx = torch.arange(32) % 8
    idx[20:] = torch.tensor([7, 3, 0, 1, 5, 5, 2, 6, 4, 0, 1, 7])
    for x in (frames, frames[idx]):
        xd = x.to(DEV)
        om, o6 = mixed(xd), six(xd)
        e = _relerr(om, o6)
        print(f"{kind}, {len(x)} frames: relerr(mixed, f32x6) = {e:.3e}")
        assert torch.isfinite(om).all() and e < 5e-6
    for k in range(8):
        rows = om[idx == k]
        assert torch.equal(rows, rows[:1].expand_as(rows)), k


def test_model_that_fails_the_gate_is_f32x6():
    sd = _state("gate-fails")
    auto, six = _vit(sd, "auto"), _vit(sd, "f32x6")
    assert auto.ln16_resolution() is None
    x = (torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(6)) * 0.8).to(DEV)
    assert torch.equal(auto(x), six(x))
