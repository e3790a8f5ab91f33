"""-m gpu: precision "f16x3s" on the CLIP ViT backbones beside ViT-B/16 -- ViT-B/32 (50 tokens), ViT-L/14 (257), ViT-L/14@336px (577):
the whole f16x3 arithmetic (two fp16 planes per operand, three products) with the streaming planes attention.

64 frames in ONE launch (enough rows for every product of a body layer to take the plane kernel; fewer rows put some of them there
and the mode, like "f16x3", wants all four or none), the two golden frames at the front and repeated at the end: the golden rows at
the bounds of test_vit_arch_golden (relerr < 1e-4 and the element-wise bound against the REFERENCE's output), all rows at the bounds
of test_vit_l14_small_launches_auto_vs_f32 against the same module at "f32" (relerr < 5e-6 and the element-wise bound), repeated
frames bit-identical, and the plan the launch executed names the streaming attention in its body layers.  On the ViT-B/16 geometry
"f16x3s" is "f16x3", bit for bit.  One act="gelu" case meets the f32 comparison."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.clip_vit import VisionTransformer
import recipes as R

DEV = "cuda"
TOL = 1e-4                                   # test_vit_arch_golden
TOL_F32 = 5e-6                               # test_vit_l14_small_launches_auto_vs_f32
FRAMES = 64
GEOMS = {"vit_b32": ("ViT-B/32", IW.VIT_B32), "vit_l14": ("ViT-L/14", IW.VIT_L14), "vit_l14_336": ("ViT-L/14@336px", IW.VIT_L14_336)}


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def elem_ok(a, b):
    return R.elem_excess(a, b) <= 1.0


def _vit(geom, arch, seed, act="quick_gelu"):
    vit = VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers, geom.vision_heads,
                            geom.embed_dim, precision="f32", arch=arch, act=act)
    vit.load_state_dict(IW.init_vit_state_dict(geom, seed, prefix=""), strict=True)
    vit.chunk = FRAMES
    return vit.to(DEV)


def _launch(base, resolution, seed):
    """FRAMES frames: the golden ones at the front and again at the end"""
    more = torch.randn(FRAMES - 4, 3, resolution, resolution, generator=torch.Generator().manual_seed(seed))
    return torch.cat([base, more, base], 0).to(DEV)


def _run(vit, x, precision):
    vit.precision = precision
    out = vit(x)
    assert out.shape[0] == x.shape[0] and bool(torch.isfinite(out).all())
    return out


def _body_plan(geom, frames=FRAMES):
    L_ = geom.grid ** 2 + 1
    recs = ops.transformer_plan(frames, L_, geom.vision_width, geom.vision_heads, geom.vision_layers, prec=L.PREC_F16X3S, prune_last=True,
                                device_index=torch.cuda.current_device())
    assert recs[-1]["pruned"] == 1
    return recs[:-1]


@pytest.mark.parametrize("tag", list(GEOMS))
def test_backbones_beside_b16(golden, tag):
    g = golden(tag)
    arch, geom = GEOMS[tag]
    base = R.vit_frames(int(g["seed"]), 2, geom.image_resolution)
    assert abs(float(base.double().sum()) - float(g["frames_checksum"])) < 1e-6
    vit = _vit(geom, arch, int(g["seed"]))
    x = _launch(base, geom.image_resolution, 11)
    o32 = _run(vit, x, "f32")
    out = _run(vit, x, "f16x3s")
    again = _run(vit, x, "f16x3s")
    print(f"F16X3S {tag}: vs golden {relerr(out[:2], g['out']):.3e}  vs f32 {relerr(out, o32):.3e}  f32 vs golden {relerr(o32[:2], g['out']):.3e}")
    body = _body_plan(geom)
    assert body and all(r["att"] == L.TF_ATT_S16 and r["in_proj"]["c_dtype"] == L.F16X2P and r["split_att"] == 0 for r in body)
    assert relerr(out[:2], g["out"]) < TOL and elem_ok(out[:2], g["out"])
    assert relerr(out, o32) < TOL_F32 and elem_ok(out, o32)
    assert torch.equal(out[-2:], out[:2]), "repeated frames differ"
    assert torch.equal(out, again), "differs run to run"


def test_b16_geometry_is_f16x3_bit_for_bit():
    geom = IW.VIT_B16
    vit = _vit(geom, "ViT-B/16", 3)
    x = torch.randn(FRAMES, 3, 224, 224, generator=torch.Generator().manual_seed(12)).to(DEV)
    a = _run(vit, x, "f16x3")
    b = _run(vit, x, "f16x3s")
    assert all(r["att"] == L.TF_ATT_P3N and r["att_products"] == 103 for r in _body_plan(geom))
    assert torch.equal(a, b)


def test_exact_gelu_meets_the_f32_comparison():
    geom = IW.VIT_B32
    vit = _vit(geom, "ViT-B/32", 5, act="gelu")
    x = torch.randn(FRAMES, 3, 224, 224, generator=torch.Generator().manual_seed(13)).to(DEV)
    o32 = _run(vit, x, "f32")
    out = _run(vit, x, "f16x3s")
    quick = _vit(geom, "ViT-B/32", 5)
    oq = _run(quick, x, "f16x3s")
    print(f"F16X3S vit_b32 gelu: vs f32 {relerr(out, o32):.3e}")
    assert relerr(out, o32) < TOL_F32 and elem_ok(out, o32)
    assert relerr(oq, out) > 1e-3                                           # (the activation reached the kernels)
