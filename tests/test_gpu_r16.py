"""-m gpu: precision "auto"'s widest mode (ACX_PREC_F32X6_R16) -- the ViT's two residual products as three-product GEMMs of fp16 planes
too.  The attention's fp16 planes bit for bit against the split of its f32 value, the c_fc -> c_proj chain against fp64 (c_fc's scaled
fp16 planes bit for bit against the split of the f32-output launch), the LayerNorm rider behind a residual product of fp16 operands
against the two stand-alone calls, and the model against precision "f32x6" with its two-step fall-back."""
import ctypes as C

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


@pytest.mark.parametrize("frames,heads", [(2, 12), (3, 16)], ids=["2x197x12", "3x197x16"])
def test_attention_planes_are_the_split_of_the_scaled_output(frames, heads):
    """acx_attention_p3f16's two planes == acx_split_f16x2(s * o, panel) with o the exact sum of the three bf16 planes acx_attention_p3f
    writes for the same q | k | v (hi + mid + lo of one f32 value: exact), s in {2^-3, 1, 64}"""
    Ltok, W = 197, heads * 64
    g = torch.Generator(device=DEV).manual_seed(100 * frames + heads)
    qkv = torch.randn(frames * Ltok, 3 * W, generator=g, device=DEV) * torch.exp2(torch.randint(-2, 3, (frames * Ltok, 1), generator=g, device=DEV).float())
    o = ops.unpanel(ops.attention_p3_f32(qkv, frames, Ltok, heads)).float().sum(0)
    assert torch.isfinite(o).all() and float(o.abs().max()) > 0.1
    for s in (2.0 ** -3, 1.0, 64.0):
        got = ops.attention_p3_f32_f16(qkv, frames, Ltok, heads, s)
        want = ops.split_f16x2(o, panel=True, scale=s)
        assert got.shape == want.shape == (2, frames * Ltok, W)
        for p, name in enumerate(("hi", "lo")):
            assert torch.equal(got[p], want[p]), (s, name)
    h = ops._h(qkv)
    out = torch.empty(2, frames * Ltok, W, dtype=torch.float16, device=DEV)
    assert L.lib().acx_attention_p3f16(h, qkv.data_ptr(), 3 * W, out.data_ptr(), 3.0, frames, Ltok, heads, ops._stream()) != 0   # not a power of two


# (M, D, H, N): LayerNorm rows of D -> c_fc + QuickGELU to H hidden columns -> c_proj (+ residual) to N.  c_fc (300, 256, 64): an edge tile;
# (520, 768, 768): strips; c_proj (520, 768, 3072): its K in the model
CHAINS = [(300, 64, 256, 256), (520, 768, 768, 768), (520, 768, 3072, 768)]


def _chain_inputs(M, D, H, N, wild):
    """wild: one hidden column 2^10 above the rest (its c_fc row and bias lifted) while nine tenths of the hidden sit at QuickGELU's
    vanishing negative tail (bias -6): elements of s * hidden far below 2^-3, where the fp16 pair keeps an ABSOLUTE 2^-25"""
    g = torch.Generator().manual_seed(1000 * M + D + H + N + int(wild))
    x = torch.randn(M, D, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())
    gamma = 1.0 + 0.2 * torch.randn(D, generator=g)
    beta = 0.3 * torch.randn(D, generator=g)
    w2 = torch.randn(H, D, generator=g) * D ** -0.5
    b2 = torch.randn(H, generator=g) * 0.5
    if wild:
        low = torch.randperm(H, generator=g)[: (92 * H) // 100]
        b2[low] = -6.0 + 0.2 * torch.randn(len(low), generator=g)
        w2[low] *= 0.25
        j0 = int(torch.tensor([j for j in range(H) if j not in set(low.tolist())])[0])
        w2[j0] *= 0.25
        scale_j0 = j0
        b2[j0] = 2.0 ** 12                                # (the other columns' medians reach ~1.5: 2^12 keeps a factor 2^10 over every one)
    w3 = torch.randn(N, H, generator=g) * H ** -0.5
    if wild:
        # the column's c_proj weights are 2^-10 of the rest: its terms are of the size of the others.  The bound is relative to S; an output
        # that IS one term of size S puts fp32 accumulation itself at the bound (a running sum of that size rounds K times: torch's fp32
        # on the CPU misses 2e-6 S there), and would let S hide the pair format's absolute floor, K 2^-25 / s |w|, which this case is about
        w3[:, scale_j0] *= 2.0 ** -10
    b3 = torch.randn(N, generator=g) * 0.5
    res = torch.randn(M, N, generator=g)
    return x, gamma, beta, w2, b2, w3, b3, res


def _chain_reference(x, gamma, beta, w2, b2, w3, b3, res, dtype):
    """(hidden, output, S of c_fc, S of c_proj) in `dtype`; S = sum_k |a||w| + |bias| (+ |residual|), a the operand in this dtype"""
    t = lambda v: v.to(dtype)
    y = torch.nn.functional.layer_norm(t(x), (x.shape[1],), t(gamma), t(beta), 1e-5)
    hid = G.quick_gelu(y @ t(w2).t() + t(b2))
    out = hid @ t(w3).t() + t(b3) + t(res)
    return hid, out, y.abs() @ t(w2).abs().t() + t(b2).abs(), hid.abs() @ t(w3).abs().t() + t(b3).abs() + t(res).abs()


_REF = {}


def _chain(M, D, H, N, wild):
    key = (M, D, H, N, wild)
    if key not in _REF:
        t = _chain_inputs(M, D, H, N, wild)
        _REF[key] = (t, _chain_reference(*t, torch.float64), _chain_reference(*t, torch.float32)[:2])
    return _REF[key]


@pytest.mark.parametrize("wild", [False, True], ids=["plain", "wild-hidden"])
@pytest.mark.parametrize("M,D,H,N", CHAINS)
def test_mlp_chain_against_fp64(M, D, H, N, wild):
    """The protocol and bounds of tests/test_gpu_ln16.py::test_chain_against_fp64: |err| <= 2e-6 S (x 1.5 behind QuickGELU), first for torch's
    fp32 on the CPU, then for the kernels.  c_fc's fp16 planes are split_f16x2(c_scale * value) of the f32-output launch bit for bit; fed
    through the residual product with out_scale = 2^-10 / c_scale the output stays inside 2e-6 S of the fp64 chain.  The scales are the
    gate's: ln16_scale of the LayerNorm bound, and of max_j min(L1_j, L2_j) (r16_bounds) for the hidden."""
    (x, gamma, beta, w2, b2, w3, b3, res), (rh, ro, S2, S3), (fh, fo) = _chain(M, D, H, N, wild)
    bd2, bd3 = 1.5 * G.EPS * S2, G.EPS * S3
    assert ((fh.double() - rh).abs() <= bd2).all() and ((fo.double() - ro).abs() <= bd3).all()      # torch fp32 stays inside
    s = V.ln16_scale(float((gamma.abs() * (D - 1) ** 0.5 + beta.abs()).max()))
    l1, l2 = V.r16_bounds(gamma, beta, w2, b2)
    hb = float(torch.minimum(l1, l2).max())
    cs = V.ln16_scale(hb)
    assert s is not None and cs is not None and float(rh.abs().max()) <= hb
    if wild:
        small = float((rh.abs() < 2.0 ** -3 / cs).double().mean())
        col = rh.abs().median(0).values
        j0 = int(col.argmax())
        rest = torch.cat([col[:j0], col[j0 + 1:]])
        print(f"wild {M}x{D}x{H}: c_scale {cs}, {100 * small:.1f} % of the hidden below 2^-3 / s, column {j0} at {float(col[j0] / rest.max()):.0f} x the next")
        assert small >= 0.9 and float(col[j0]) >= 2.0 ** 10 * float(rest.max())
    xd, gd, bed = x.to(DEV), gamma.to(DEV), beta.to(DEV)
    a2 = ops.layernorm_f16x2(xd, gd, bed, s) if D == 768 else ops.split_f16x2(ops.layernorm(xd, gd, bed) * s, panel=True)
    w2p, w3p = ops.split_f16x2(w2.to(DEV), panel=True, scale=WSCALE), ops.split_f16x2(w3.to(DEV), panel=True, scale=WSCALE)
    osc = 1.0 / (WSCALE * s)
    kw = dict(panels=3, pairs=3, out_scale=osc, bias=b2.to(DEV), act=L.ACT_QUICKGELU)
    # the f32-output launch; whole K per tile, as every launch with fp16 plane output (no reduce launch writes those planes: a launch of
    # few tiles would otherwise split K across workgroups and sum in another order)
    hf = ops.gemm_x6(a2, w2p, split_k=False, **kw)
    e2 = (hf.double().cpu() - rh).abs()
    print(f"c_fc {M}x{H}x{D} wild={wild} s={s}: max err / bound = {float((e2 / bd2).max()):.3f}")
    assert (e2 <= bd2).all()
    hp = ops.gemm_x6(a2, w2p, planes_out=True, panel_out=True, c_scale=cs, **kw)
    assert hp.dtype == torch.float16 and hp.shape == (2, M, H)
    want = ops.split_f16x2(hf, panel=True, scale=cs)
    assert torch.equal(hp[0], want[0]) and torch.equal(hp[1], want[1])
    assert torch.isfinite(hp.float()).all() and float(hp[0].float().abs().max()) <= 2.0 ** 14 * (1 + 2.0 ** -10)
    if cs != 1.0:                                                                     # c_scale = 0 / 1: the planes of the value itself
        assert torch.equal(ops.gemm_x6(a2, w2p, planes_out=True, panel_out=True, **kw), ops.split_f16x2(hf, panel=True))
    out = ops.gemm_x6(hp, w3p, panels=3, pairs=3, out_scale=1.0 / (WSCALE * cs), bias=b3.to(DEV), residual=res.to(DEV))
    e3 = (out.double().cpu() - ro).abs()
    print(f"c_proj {M}x{N}x{H} wild={wild} c_scale={cs}: max err / bound = {float((e3 / bd3).max()):.3f}")
    assert (e3 <= bd3).all()


def _rider_m(N, K, ncu):
    """the smallest multiple of 256 above one full round of tiles for which the host plan lets rows ride"""
    M = (ncu // (N // 256) + 1) * 256
    while ops.ln_rider_plan(M, N, K, ncu)[0] == 0:
        M += 256
        assert M < 64 * 256 * ncu
    return M


RIDER_CASES = [("out-proj", 768, 768, 0), ("c_proj", 768, 3072, 0), ("out-proj edge", 768, 768, 130), ("c_proj edge", 768, 3072, 130),
               ("width 1024", 1024, 1024, 0)]


@pytest.mark.parametrize("name,N,K,extra", RIDER_CASES, ids=[c[0] for c in RIDER_CASES])
def test_rider_behind_fp16_operands_bit_identical(name, N, K, extra):
    """tests/test_gpu_ln16.py::test_rider_fp16_planes_bit_identical with A as fp16 pair planes and pairs = 3 (gemm_x6_r16_kernel's RIDE
    instantiations): x and both planes of s * LayerNorm torch.equal to acx_gemm followed by acx_layernorm_scaled, with the cost model's
    rows, with every completed row riding, and switched off.  N == K: the job's planes ARE the product's A planes (ln_2 behind out-proj
    in the model: same two-plane geometry, the riders write plane rows the last round's tiles do not read)."""
    dev = torch.cuda.current_device()
    ncu = ops.x6_workgroups(dev)
    M = _rider_m(N, K, ncu) + extra
    ride, ready = ops.ln_rider_plan(M, N, K, ncu)
    print(f"{name}: {M} x {N} x {K} on {ncu} workgroups: the six-product plan rides {ride} of {ready} completed rows")
    assert ride > 0 and M % 2 == 0
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g, device=DEV) * torch.exp2(torch.randint(-4, 4, (M, 1), generator=g, device=DEV).float())
    sa = 64.0
    a2 = ops.split_f16x2(a, panel=True, scale=sa)
    del a
    w2 = ops.split_f16x2(torch.randn(N, K, generator=g, device=DEV) * 0.05, panel=True, scale=WSCALE)
    bias = torch.randn(N, generator=g, device=DEV)
    x = torch.randn(M, N, generator=g, device=DEV) * 3.0
    lw, lb = torch.randn(N, generator=g, device=DEV), torch.randn(N, generator=g, device=DEV)
    s = 128.0
    kw = dict(panels=3, pairs=3, out_scale=1.0 / (WSCALE * sa), bias=bias)
    x_ref = x.clone()
    ops.gemm_x6(a2, w2, residual=x_ref, out=x_ref, **kw)
    y_ref = ops.layernorm_f16x2(x_ref, lw, lb, s)
    try:
        for mode in (1, 10 ** 9, 0):
            ops.set_ln_rider(dev, mode)
            x2 = x.clone()
            if N == K:
                y2 = a2c = a2.clone()
                ops.gemm_x6(a2c, w2, residual=x2, out=x2, ln=(lw, lb, y2, s), **kw)
            else:
                y2 = torch.full((2, M, N), 7.0, dtype=torch.float16, device=DEV)
                ops.gemm_x6(a2, w2, residual=x2, out=x2, ln=(lw, lb, y2, s), **kw)
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
    if kind == "wide-fails":
        sd["transformer.resblocks.4.mlp.c_proj.weight"][7, 9] = 100.0
    if kind == "ln16-fails":
        sd["transformer.resblocks.4.mlp.c_fc.weight"][7, 9] = 100.0
    return sd


@pytest.mark.parametrize("kind", ["init", "affine"])
def test_model_wide_against_f32x6(kind):
    """ViT-B/16, 8 and 32 frames: "auto" resolves to the wide mode, stays finite and within 5e-6 (relative to the largest feature) of
    "f32x6" -- the bound tests/test_gpu_ln16.py holds the mixed mode to; identical frames give bit-identical rows in every slot."""
    sd = _state(kind)
    wide, six = _vit(sd, "auto"), _vit(sd, "f32x6")
    sc = wide.r16_resolution()
    assert sc is not None and len(sc) == 48 and len(wide.ln16_resolution()) == 24
    frames = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(5)) * 0.8
    idx = torch.arange(32) % 8
    idx[20:] = torch.tensor([7, 3, 0, 1, 5, 5, 2, 6, 4, 0, 1, 7])
    for x in (frames, frames[idx]):
        xd = x.to(DEV)
        ow, o6 = wide(xd), six(xd)
        e = _relerr(ow, o6)
        print(f"{kind}, {len(x)} frames: relerr(wide, f32x6) = {e:.3e}")
        assert torch.isfinite(ow).all() and e < 5e-6
    for k in range(8):
        rows = ow[idx == k]
        assert torch.equal(rows, rows[:1].expand_as(rows)), k


def _encode_ln16(vit, x):
    """acx_vit_encode_ln16 called directly with the model's weights and LayerNorm scales"""
    scales, sc, fc16, _ = vit._ln16_bound()
    d = L.VitDesc(vit.input_resolution, vit.patch_size, vit.width, vit.layers, vit.heads, vit.output_dim, L.PREC_F32X6_LN16)
    w, _keep = vit._weights(L.PREC_F32X6_LN16, fc16)
    lib = L.lib()
    n = x.shape[0]
    out = torch.empty(n, vit.output_dim, dtype=torch.float32, device=x.device)
    nbytes = lib.acx_vit_workspace_bytes(C.byref(d), n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    h = ops._h(x)
    L.check(lib.acx_vit_encode_ln16(h, C.byref(d), C.byref(w), sc, x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), nbytes, ops._stream()), h)
    return out


def test_model_falls_back_in_two_steps():
    """a weight failing only the new conditions: "auto" is the ACX_PREC_F32X6_LN16 result bit for bit (that arm: acx_vit_encode_ln16 called
    directly); a weight failing LN16's conditions: "f32x6" bit for bit"""
    x = (torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(6)) * 0.8).to(DEV)
    auto = _vit(_state("wide-fails"), "auto")
    assert auto.r16_resolution() is None and auto.ln16_resolution() is not None
    assert torch.equal(auto(x), _encode_ln16(auto, x))
    sd = _state("ln16-fails")
    auto, six = _vit(sd, "auto"), _vit(sd, "f32x6")
    assert auto.r16_resolution() is None and auto.ln16_resolution() is None
    assert torch.equal(auto(x), six(x))
    # ... and on weights passing everything the direct LN16 arm is NOT what "auto" runs (the wide mode is taken)
    wide = _vit(_state("init"), "auto")
    assert wide.r16_resolution() is not None
    assert not torch.equal(wide(x), _encode_ln16(wide, x))
