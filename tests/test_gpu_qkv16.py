"""-m gpu: precision "auto"'s third resolution step (ACX_PREC_F32X6_QKV16) -- q | k | v as fp16 planes from the in-projection into the
three-product planes attention.  The attention kernel on scaled planes against fp64 (bounded by the f32 MFMA attention's own error) and
its output planes bit for bit, the in-projection that produces the planes against fp64, and the model against precision "f32x6" with its
fall-back to ACX_PREC_F32X6_R16."""
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
DATA = ("plain", "large-logits", "one-column-x40", "small-v")


def _two_item_frames(heads=12):
    """a frame count whose (frame, head) items exceed the workgroups (one per CU) by less than a factor of two: some workgroups run two
    items and stage K(next) during phase B.  24 on 256 CUs."""
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    frames = 24 if ncu < 24 * heads < 2 * ncu else ncu // heads + 2
    assert ncu < frames * heads < 2 * ncu, (ncu, frames)
    return frames


def _qkv(frames, heads, Ltok, kind):
    W = heads * 64
    g = torch.Generator(device=DEV).manual_seed(1000 * frames + 10 * heads + Ltok + DATA.index(kind))
    qkv = torch.randn(frames * Ltok, 3 * W, generator=g, device=DEV) * 1.3
    if kind == "large-logits":
        qkv[:, :2 * W] *= 6.0
    if kind == "one-column-x40":
        for t in range(3):
            qkv[:, t * W + 37 + 64 * (t % heads)] *= 40.0
    if kind == "small-v":
        qkv[:, 2 * W:] *= 2.0 ** -12
    return qkv


def _fp64(qkv, frames, Ltok, heads):
    x = qkv.double().view(frames, Ltok, 3, heads, 64)
    q_, k_, v_ = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    return (torch.softmax(q_ @ k_.transpose(-1, -2) / 8.0, dim=-1) @ v_).transpose(1, 2).reshape(frames * Ltok, heads * 64)


@pytest.mark.parametrize("Ltok", [193, 197, 208])
@pytest.mark.parametrize("frames,heads", [(2, 12), (3, 16), (0, 12)], ids=["2x12", "3x16", "two-items-x12"])
def test_attention_on_scaled_planes_against_fp64(frames, heads, Ltok):
    """acx_attention_p3h16 on split_f16x2(s * qkv, panel) with the gate's scales (s: the largest power of two with s * max|q, k, v| <= 2^14,
    s_att the same for max|v|): the reassembled (hi + lo) / s_att is finite and its max err / max|ref| against fp64 is at most 4 x that of
    the f32 MFMA attention (acx_attention) on the same inputs -- a two-plane fp16 operand holds 22 of f32's 24 significand bits.  Four
    data sets: plain; q and k scaled by 6 (large logits); one q / k / v column scaled by 40; V scaled by 2^-12 (lo planes in the
    subnormals: one scale serves the three thirds)."""
    frames = frames or _two_item_frames(heads)
    for kind in DATA:
        qkv = _qkv(frames, heads, Ltok, kind)
        ref = _fp64(qkv, frames, Ltok, heads)
        s = V.ln16_scale(float(qkv.abs().max()))
        s_att = V.ln16_scale(max(float(qkv[:, 2 * heads * 64:].abs().max()), 2.0 ** -6))   # (at most 2^20: the entry point's range)
        planes = ops.attention_p3_h16(ops.split_f16x2(qkv, panel=True, scale=s), frames, Ltok, heads, s, s_att)
        out = ops.unpanel(planes).float().sum(0) / s_att
        o32 = ops.attention(qkv, frames, Ltok, heads, False)
        mx = float(ref.abs().max())
        e, e32 = float((out.double() - ref).abs().max()) / mx, float((o32.double() - ref).abs().max()) / mx
        print(f"{frames}x{Ltok}x{heads} {kind}: s {s} s_att {s_att}: max err / max|ref| {e:.3e}, f32 MFMA attention {e32:.3e}, ratio {e / e32:.2f}")
        assert torch.isfinite(out).all(), kind
        assert e <= 4.0 * e32, (kind, e, e32)


@pytest.mark.parametrize("frames,heads", [(2, 12), (3, 16)], ids=["2x197x12", "3x197x16"])
def test_attention_planes_are_the_split_of_the_scaled_output(frames, heads):
    """The f32 output o never leaves this kernel whole (its two planes hold 22 bits of it), so acx_split_f16x2(out_scale * o) cannot be
    formed outside it as tests/test_gpu_r16.py forms it for the f32-rows arm.  The planes are pinned bit for bit in two steps instead:
    at in_scale = out_scale = 1 they are acx_attention_p3n(products = 103)'s -- the tested form this kernel shares its body with, whose
    planes are that split; and with in_scale fixed, out_scale only multiplies o by a power of two in front of the split, so wherever an
    fp16 number and its multiple are both normal (above 2^-14) the planes at out_scale = t are the planes at out_scale = 1024 times t / 1024, exactly,
    hi and lo.  Across in_scales the value agrees to the pair format's 2^-21 |o| + 2^-24 / out_scale.  Scales that are no powers of two
    in 2^-20 ... 2^20 are refused."""
    Ltok, W = 197, heads * 64
    g = torch.Generator(device=DEV).manual_seed(100 * frames + heads)
    qkv = torch.randn(frames * Ltok, 3 * W, generator=g, device=DEV) * torch.exp2(torch.randint(-2, 3, (frames * Ltok, 1), generator=g, device=DEV).float())
    q1 = ops.split_f16x2(qkv, panel=True)
    base = ops.attention_p3(q1, frames, Ltok, heads, products=103)
    assert torch.equal(ops.attention_p3_h16(q1, frames, Ltok, heads, 1.0, 1.0), base)
    tiny = 2.0 ** -14                                           # fp16's smallest normal number
    for s in (1.0, 64.0):
        qs = q1 if s == 1.0 else ops.split_f16x2(qkv, panel=True, scale=s)
        big = ops.attention_p3_h16(qs, frames, Ltok, heads, s, 1024.0).float()
        assert torch.isfinite(big).all() and float(big[0].abs().max()) > 100.0
        for t in (2.0 ** -3, 1.0, 64.0):
            got = ops.attention_p3_h16(qs, frames, Ltok, heads, s, t)
            assert got.shape == (2, frames * Ltok, W) and got.dtype == torch.float16
            if s == 1.0 and t == 1.0:
                assert torch.equal(got, base)
            got = got.float()
            r = 1024.0 / t
            # (strictly above 2^-14: a value rounded UP to 2^-14 was rounded on the subnormals' grid, twice as coarse as its multiple's)
            hi_ok = got[0].abs() > tiny
            lo_ok = hi_ok & ((got[1].abs() > tiny) | ((got[1] == 0) & (big[1] == 0)))
            bad = [int(((got[p] * r)[m] != big[p][m]).sum()) for p, m in ((0, hi_ok), (1, lo_ok))]
            print(f"in_scale {s} out_scale {t}: hi normal on {float(hi_ok.float().mean()):.4f}, lo normal on {float(lo_ok.float().mean()):.4f} of the "
                  f"elements; elements that differ there: hi {bad[0]}, lo {bad[1]}")
            assert torch.equal((got[0] * r)[hi_ok], big[0][hi_ok]), (s, t, "hi")
            assert torch.equal((got[1] * r)[lo_ok], big[1][lo_ok]), (s, t, "lo")
            assert float(hi_ok.float().mean()) > 0.99 and (t < 64.0 or float(lo_ok.float().mean()) > 0.9)
            o, ob = (got[0].double() + got[1].double()) / t, (big[0].double() + big[1].double()) / 1024.0
            assert ((o - ob).abs() <= 2.0 ** -21 * ob.abs() + 2.0 ** -24 / t).all(), (s, t)
    o1 = ops.unpanel(ops.attention_p3_h16(q1, frames, Ltok, heads, 1.0, 1024.0)).double().sum(0)
    o64 = ops.unpanel(ops.attention_p3_h16(ops.split_f16x2(qkv, panel=True, scale=64.0), frames, Ltok, heads, 64.0, 1024.0)).double().sum(0)
    ref = _fp64(qkv, frames, Ltok, heads) * 1024.0
    assert float((o1 - o64).abs().max()) <= 4e-6 * float(ref.abs().max())      # (in_scale = 1 leaves small operands' lo planes subnormal)
    h = ops._h(qkv)
    out = torch.empty(2, frames * Ltok, W, dtype=torch.float16, device=DEV)
    for bad in ((3.0, 1.0), (1.0, 3.0), (2.0 ** 21, 1.0), (1.0, 2.0 ** -21), (0.0, 1.0)):
        assert L.lib().acx_attention_p3h16(h, q1.data_ptr(), bad[0], out.data_ptr(), bad[1], frames, Ltok, heads, ops._stream()) != 0, bad


# (M, K, N): test_gpu_r16.CHAINS' M and K (an edge tile; the model's K), N = 3 K as the in-projection, N % 32 == 0
PRODUCER = [(300, 64, 192), (520, 768, 2304)]


@pytest.mark.parametrize("M,K,N", PRODUCER)
def test_in_projection_planes_against_fp64(M, K, N):
    """The in-projection as ACX_PREC_F32X6_QKV16 runs it: fp16 A planes of s_a * LayerNorm, the weight's fp16 planes, bias, no activation,
    c_scale = s, ACX_F16X2P output.  The bound test_gpu_r16.py::test_mlp_chain_against_fp64 holds c_fc's planes to: the f32-output launch
    within 2e-6 S of fp64 (S = sum |a||w| + |bias|; no activation, so no factor 1.5), the planes split_f16x2(s * value) of that launch bit
    for bit, inside 2^14.  One third of the columns is 2^-12 of the others (one scale for the three thirds)."""
    g = torch.Generator().manual_seed(M + K + N)
    x = torch.randn(M, K, generator=g) * torch.exp2(torch.randint(-3, 4, (M, 1), generator=g).float())
    gamma, beta = 1.0 + 0.2 * torch.randn(K, generator=g), 0.3 * torch.randn(K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.5
    w[2 * N // 3:] *= 2.0 ** -12
    b[2 * N // 3:] *= 2.0 ** -12
    y64 = torch.nn.functional.layer_norm(x.double(), (K,), gamma.double(), beta.double(), 1e-5)
    ref = y64 @ w.double().t() + b.double()
    S = y64.abs() @ w.double().abs().t() + b.double().abs()
    sa = V.ln16_scale(float((gamma.abs() * (K - 1) ** 0.5 + beta.abs()).max()))
    l1, l2 = V.r16_bounds(gamma, beta, w, b)
    bound = float(torch.minimum(l1, l2).max())
    cs = V.ln16_scale(bound)
    assert sa is not None and cs is not None and float(ref.abs().max()) <= bound
    xd = x.to(DEV)
    a2 = ops.layernorm_f16x2(xd, gamma.to(DEV), beta.to(DEV), sa) if K == 768 else ops.split_f16x2(ops.layernorm(xd, gamma.to(DEV), beta.to(DEV)) * sa, panel=True)
    w2 = ops.split_f16x2(w.to(DEV), panel=True, scale=WSCALE)
    kw = dict(panels=3, pairs=3, out_scale=1.0 / (WSCALE * sa), bias=b.to(DEV))
    vf = ops.gemm_x6(a2, w2, split_k=False, **kw)
    e = (vf.double().cpu() - ref).abs()
    print(f"in-projection {M}x{N}x{K} s_a={sa} c_scale={cs}: max err / bound = {float((e / (G.EPS * S)).max()):.3f}")
    assert (e <= G.EPS * S).all()
    vp = ops.gemm_x6(a2, w2, planes_out=True, panel_out=True, c_scale=cs, **kw)
    assert vp.dtype == torch.float16 and vp.shape == (2, M, N)
    want = ops.split_f16x2(vf, panel=True, scale=cs)
    assert torch.equal(vp[0], want[0]) and torch.equal(vp[1], want[1])
    assert torch.isfinite(vp.float()).all() and float(vp[0].float().abs().max()) <= 2.0 ** 14 * (1 + 2.0 ** -10)


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
    if kind == "qk-fails":
        sd["transformer.resblocks.4.attn.in_proj_bias"][9] = 2.0 ** 35  # a Q bias: the Q | K | V bound's scale falls below 2^-20
    return sd


def _new_path_frames():
    """the smallest launch of (8, 16, 32, 64) frames whose body layers the plan moves to the new path"""
    for n in (8, 16, 32, 64):
        rec = ops.transformer_plan(n, 197, 768, 12, 12, prec=L.PREC_F32X6_QKV16, prune_last=True, device_index=torch.cuda.current_device())[1]
        if rec["att"] == L.TF_ATT_P3N and rec["att_products"] == 103 and rec["in_proj"]["c_dtype"] == L.F16X2P:
            return n
    return None


@pytest.mark.parametrize("kind", ["init", "affine"])
def test_model_against_f32x6(kind):
    """ViT-B/16 at the smallest launch the plan moves: "auto" resolves to the new mode, stays finite and within 5e-6 (relative to the
    largest feature) of "f32x6" -- the bound test_gpu_r16.py::test_model_wide_against_f32x6 uses; identical frames give bit-identical rows."""
    n = _new_path_frames()
    assert n is not None and n <= 64
    sd = _state(kind)
    new, six = _vit(sd, "auto"), _vit(sd, "f32x6")
    s5 = new.qkv16_resolution()
    assert s5 is not None and len(s5) == 60 and len(new.r16_resolution()) == 48
    frames = torch.randn(4, 3, 224, 224, generator=torch.Generator().manual_seed(5)) * 0.8
    idx = torch.arange(n) % 4
    idx[n // 2:] = idx[n // 2:].flip(0)
    xd = frames[idx].to(DEV)
    on, o6 = new(xd), six(xd)
    e = _relerr(on, o6)
    print(f"{kind}, {n} frames: relerr(qkv16, f32x6) = {e:.3e}; s_qkv per layer {s5[4::5]}")
    assert torch.isfinite(on).all() and e < 5e-6
    for k in range(4):
        rows = on[idx == k]
        assert torch.equal(rows, rows[:1].expand_as(rows)), k


def _encode_r16(vit, x):
    """acx_vit_encode_r16 called directly with the model's weights and scales"""
    _scales, _sc, fc16, r16 = vit._ln16_bound()
    _s4, sc4, fmt = r16
    d = L.VitDesc(vit.input_resolution, vit.patch_size, vit.width, vit.layers, vit.heads, vit.output_dim, L.PREC_F32X6_R16)
    w, _keep = vit._weights(L.PREC_F32X6_R16, fc16, fmt)
    lib = L.lib()
    n = x.shape[0]
    out = torch.empty(n, vit.output_dim, dtype=torch.float32, device=x.device)
    nbytes = lib.acx_vit_workspace_bytes(C.byref(d), n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    h = ops._h(x)
    L.check(lib.acx_vit_encode_r16(h, C.byref(d), C.byref(w), sc4, x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), nbytes, ops._stream()), h)
    return out


def test_model_falls_back_to_r16():
    """weights failing only the Q / K condition: "auto" is the ACX_PREC_F32X6_R16 result bit for bit (acx_vit_encode_r16 called directly);
    on weights passing everything that direct call is NOT what "auto" returns (the new mode is taken)"""
    n = _new_path_frames()
    assert n is not None and n <= 64
    x = (torch.randn(n, 3, 224, 224, generator=torch.Generator().manual_seed(6)) * 0.8).to(DEV)
    auto = _vit(_state("qk-fails"), "auto")
    assert auto.qkv16_resolution() is None and auto.r16_resolution() is not None
    out, direct = auto(x), _encode_r16(auto, x)
    print(f"Q bias 2^35: {float(torch.isfinite(out).float().mean()):.3f} of the features finite")
    assert torch.equal(out.view(torch.int32), direct.view(torch.int32))     # bit for bit, whatever such a bias makes of the features
    new = _vit(_state("init"), "auto")
    assert new.qkv16_resolution() is not None
    assert not torch.equal(new(x), _encode_r16(new, x))
