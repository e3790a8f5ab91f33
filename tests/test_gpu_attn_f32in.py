"""-m gpu: acx_attention_p3f -- the six-product plane attention fed with the in-projection's f32 rows, splitting q | k | v into the
three bf16 planes as it stages them -- gives the bits of acx_attention_p3 on the split planes: at kernel level on all three output
planes, at model level with ACX_OPT_ATTN_F32IN on and off (the in-projection's plane epilogue against the attention's own split)."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.clip_vit import VisionTransformer
import recipes as R

DEV = "cuda"


def _qkv(batch, L_, heads, ld=None):
    """the input of test_attention_p3_vs_fp64: randn * 1.7, q scaled by 1.5, the last sequence a copy of the first where batch > 2"""
    W = heads * 64
    g = torch.Generator().manual_seed(batch * 1000 + L_)
    qkv = torch.randn(batch * L_, 3 * W, generator=g) * 1.7
    qkv[:, :W] *= 1.5
    if batch > 2:
        qkv[(batch - 1) * L_:] = qkv[:L_]
    if ld is None:
        return qkv.to(DEV)
    buf = torch.full((batch * L_, ld), float("nan"), device=DEV)      # the padding columns must never be read
    buf[:, :3 * W] = qkv.to(DEV)
    return buf[:, :3 * W]


# (1, 193, 1): shortest L of the gate, one item; (2, 208, 2): no padded key row; (3, 197, 12): equal sequences; (24, 197, 12): 288
# items, more than one per workgroup -- the persistent loop, K of the next item staged under phase B
@pytest.mark.parametrize("batch,L_,heads,pad", [(1, 193, 1, 0), (2, 208, 2, 0), (3, 197, 12, 0), (24, 197, 12, 0), (3, 197, 12, 64)])
def test_f32_input_gives_the_plane_kernels_bits(batch, L_, heads, pad):
    W = heads * 64
    qd = _qkv(batch, L_, heads, 3 * W + pad if pad else None)
    assert qd.stride(0) == 3 * W + pad
    ref = ops.attention_p3(ops.split_bf16x3(qd.contiguous(), panel=True), batch, L_, heads)
    out = ops.attention_p3_f32(qd, batch, L_, heads)
    for p, pl in enumerate(("hi", "mid", "lo")):
        assert torch.equal(out[p].view(torch.int16), ref[p].view(torch.int16)), (pl, int((out[p] != ref[p]).sum()))
    if batch > 2:
        o = ops.unpanel(out)
        assert torch.equal(o[:, (batch - 1) * L_:], o[:, :L_])


@pytest.mark.parametrize("batch,L_,heads", [(3, 197, 12), (3, 200, 3)])
def test_f32_input_vs_fp64(batch, L_, heads):
    """the bound of test_attention_p3_vs_fp64: no worse than 1.5 x the f32 MFMA kernel's maximum error on the same input, and within
    2e-6 of max |ref|"""
    W = heads * 64
    qd = _qkv(batch, L_, heads)
    out = ops.unpanel(ops.attention_p3_f32(qd, batch, L_, heads)).float().sum(0)
    ref32 = ops.attention(qd, batch, L_, heads, False)
    x = qd.double().view(batch, L_, 3, heads, 64)
    q_, k_, v_ = x[:, :, 0].transpose(1, 2), x[:, :, 1].transpose(1, 2), x[:, :, 2].transpose(1, 2)
    ref = (torch.softmax(q_ @ k_.transpose(-1, -2) / 8.0, dim=-1) @ v_).transpose(1, 2).reshape(batch * L_, W)
    e3, e32 = (out.double() - ref).abs().max().item(), (ref32.double() - ref).abs().max().item()
    print("max |err| vs fp64: f32-input planes kernel", e3, " f32 MFMA", e32)
    assert torch.isfinite(out).all() and e3 <= 1.5 * e32 and e3 <= 2e-6 * ref.abs().max().item()


@functools.lru_cache(maxsize=None)
def _weights(name, seed):
    return IW.init_vit_state_dict(getattr(IW, name), seed, prefix="")


def _vit(name, precision, seed=3):
    geom = getattr(IW, name)
    vit = VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers,
                            geom.vision_heads, geom.embed_dim, precision=precision)
    vit.load_state_dict(_weights(name, seed), strict=True)
    return vit.to(DEV)


def _on_off(vit, x):
    dev = torch.cuda.current_device()
    vit.chunk = x.shape[0]
    before = ops.get_option(dev, L.OPT_ATTN_F32IN)
    try:
        ops.set_attn_f32in(dev, True)
        on = vit(x).clone()
        ops.set_attn_f32in(dev, False)
        off = vit(x).clone()
    finally:
        ops.set_attn_f32in(dev, before)
    assert on.shape[0] == x.shape[0] and torch.isfinite(on).all()
    return on, off


# 8 frames: the smallest launch whose in- and out-projection both take the plane kernels (63 and 21 tiles, ACX_OPT_X6_MIN_TILES = 18);
# 9 frames: an edge row tile; a frame scaled by 1e4: the split of large magnitudes through the real epilogue
@pytest.mark.parametrize("frames,scale", [(8, 1.0), (9, 1.0), (8, 1e4)])
def test_vit_features_equal_with_f32_qkv_on_and_off(frames, scale):
    vit = _vit("VIT_B16", "auto")
    x = R.vit_frames(3, frames, 224)
    x[1] *= scale
    on, off = _on_off(vit, x.to(DEV))
    assert torch.equal(on, off), (frames, scale, int((on != off).any(1).sum()))


@pytest.mark.parametrize("name,precision", [("VIT_B16", "f16x3"), ("VIT_B16", "bf16x3"), ("VIT_B32", "auto")])
def test_other_routes_do_not_change(name, precision):
    """the three-product precisions keep the plane route, a 50-token geometry never had the plane attention: equal with the option on
    and off"""
    vit = _vit(name, precision)
    on, off = _on_off(vit, R.vit_frames(3, 8, 224).to(DEV))
    assert torch.equal(on, off), (name, precision)
