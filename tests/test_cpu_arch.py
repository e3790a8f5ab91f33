"""The CLIP ViT backbones selected by `net.arch` (ViT-B/16, ViT-B/32, ViT-L/14, ViT-L/14@336px): geometry registry, the mirrors'
parameter names and shapes against the reference's CLIP(**geometry) (tests/golden/arch_shapes.json, make_golden_arch.py), and
the errors raised before any GPU work.  No GPU needed: modules are built on the meta device where they would be large."""
import json
import os

import pytest
import torch

from anomalyclip_amd import init_weights as IW
from anomalyclip_amd.components import anomaly_clip as AC
from anomalyclip_amd.components.clip_vit import VisionTransformer
from anomalyclip_amd.components.text_encoder import TextEncoder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VIT_ARCHS = ("ViT-B/16", "ViT-B/32", "ViT-L/14", "ViT-L/14@336px")


def _shapes():
    with open(os.path.join(GOLDEN, "arch_shapes.json")) as f:
        return json.load(f)


def _net_kw(**kw):
    base = dict(labels_key="ucf", emb_size=64, depth=1, heads=2, dim_heads=None, num_segments=32, seg_length=16,
                concat_features=False, normal_id=7, stride=1, load_from_features=True, select_idx_dropout_topk=0.7,
                select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3)
    base.update(kw)
    return base


def test_arch_registry_has_the_four_vit_backbones():
    for a in VIT_ARCHS:
        assert a in AC._ARCH
    assert AC._ARCH["ViT-B/32"] == IW.VIT_B32 and AC._ARCH["ViT-L/14"] == IW.VIT_L14
    assert AC._ARCH["ViT-L/14@336px"] == IW.VIT_L14_336
    # CLIP's published shapes (clip/model.py:294-308 arguments as clip.build_model derives them)
    assert (IW.VIT_B32.vision_patch_size, IW.VIT_B32.grid ** 2 + 1, IW.VIT_B32.embed_dim) == (32, 50, 512)
    assert (IW.VIT_L14.vision_width, IW.VIT_L14.vision_layers, IW.VIT_L14.grid ** 2 + 1, IW.VIT_L14.embed_dim) == (1024, 24, 257, 768)
    assert (IW.VIT_L14.transformer_width, IW.VIT_L14.transformer_heads, IW.VIT_L14.transformer_layers) == (768, 12, 12)
    assert (IW.VIT_L14_336.image_resolution, IW.VIT_L14_336.grid ** 2 + 1) == (336, 577)


@pytest.mark.parametrize("arch", VIT_ARCHS)
def test_mirror_state_dict_matches_reference_clip(arch):
    """Every name and shape of the reference CLIP(**geometry) that the mirrors hold: visual.* = the image encoder,
    transformer.* / positional_embedding / ln_final.* / text_projection = the text encoder, token_embedding.weight."""
    ref = _shapes()[arch]
    g = AC._ARCH[arch]
    with torch.device("meta"):
        vit = VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads,
                                g.embed_dim, arch=arch)
        te = TextEncoder(g.context_length, g.transformer_width, g.transformer_heads, g.transformer_layers, g.embed_dim)
        tok = AC._TokenEmbedding(g.vocab_size, g.transformer_width)
    mine = {"visual." + k: list(v.shape) for k, v in vit.state_dict().items()}
    mine.update({k: list(v.shape) for k, v in te.state_dict().items()})
    mine["token_embedding.weight"] = list(tok.weight.shape)
    want = {k: v for k, v in ref.items() if k != "logit_scale"}            # (logit_scale lives in the selector)
    assert mine == want


@pytest.mark.parametrize("arch", VIT_ARCHS)
def test_init_weights_match_reference_shapes(arch):
    """init_weights draws exactly the reference's image-encoder tensors for every arch (the GPU goldens load them strictly)."""
    ref = _shapes()[arch]
    g = AC._ARCH[arch]
    with torch.device("meta"):
        sd = IW.init_vit_state_dict(g, 0, prefix="visual.")
    assert {k: list(v.shape) for k, v in sd.items()} == {k: v for k, v in ref.items() if k.startswith("visual.")}


def test_unknown_arch_lists_the_supported_names():
    with pytest.raises(ValueError) as e:
        AC.AnomalyCLIP(**_net_kw(arch="ViT-H/14"))
    msg = str(e.value)
    assert "ViT-H/14" in msg and all(a in msg for a in VIT_ARCHS)


def _meta_checkpoint(arch):
    """A state_dict with the reference ViT-L/14 (etc.) image / text encoder shapes, on the meta device (shapes only)."""
    out = {}
    for k, shape in _shapes()[arch].items():
        if k.startswith("visual."):
            out["image_encoder." + k[len("visual."):]] = torch.empty(shape, device="meta")
        elif k.startswith(("transformer.", "positional_embedding", "ln_final.", "text_projection")):
            out["text_encoder." + k] = torch.empty(shape, device="meta")
    return out


def test_mismatched_checkpoint_names_both_geometries():
    net = AC.AnomalyCLIP(**_net_kw(arch="tiny"))
    with pytest.raises(ValueError) as e:
        net.load_state_dict(_meta_checkpoint("ViT-L/14"), strict=False)
    msg = str(e.value)
    assert "ViT-L/14" in msg and "'tiny'" in msg and "width 1024" in msg and "width 128" in msg
    # a checkpoint of the module's own geometry still loads
    sd = {k: v.clone() for k, v in net.state_dict().items()}
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not missing and not unexpected


def test_geometry_from_state_dict_recognises_every_arch():
    for arch in VIT_ARCHS:
        assert AC.geometry_from_state_dict(_meta_checkpoint(arch)) == AC._ARCH[arch], arch


@pytest.mark.parametrize("arch", ["ViT-L/14", "ViT-L/14@336px", "ViT-B/32"])
@pytest.mark.parametrize("precision", ["f16x3", "bf16x3"])
def test_three_product_modes_refused_off_the_b16_geometry(arch, precision):
    """f16x3 / bf16x3 need the planes attention (192 < L <= 208) of ViT-B/16: refused with the arch named, before any allocation
    or launch (the model is not even built)."""
    with pytest.raises(ValueError) as e:
        AC.AnomalyCLIP(**_net_kw(arch=arch, precision=precision))
    assert arch in str(e.value) and precision in str(e.value)
    g = AC._ARCH[arch]
    with torch.device("meta"), pytest.raises(ValueError, match="not available"):
        VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim,
                          precision=precision, arch=arch)


def test_vit_refuses_a_precision_switched_after_construction():
    g = IW.VIT_L14
    with torch.device("meta"):
        vit = VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads,
                                g.embed_dim, precision="auto", arch="ViT-L/14")
    vit.precision = "f16x3"
    with pytest.raises(ValueError, match="ViT-L/14"):
        vit(torch.zeros(1, 3, 224, 224))


@pytest.mark.parametrize("geom", [IW.VIT_B16, IW.TINY, IW.ClipGeometry(image_resolution=192, vision_patch_size=16)])
def test_other_geometries_keep_their_three_product_modes(geom):
    """Only the new backbones' geometries (and sequences above 224 tokens, which never ran) refuse f16x3 / bf16x3: ViT-B/16, the
    test geometry and a custom one construct as before."""
    g = geom
    with torch.device("meta"):
        for p in ("f16x3", "bf16x3", "auto", "f32", "bf16"):
            VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads,
                              g.embed_dim, precision=p)
    AC.AnomalyCLIP(**_net_kw(arch="tiny", precision="bf16x3"))


def test_three_product_modes_refused_above_224_tokens():
    g = IW.ClipGeometry(image_resolution=240, vision_patch_size=16)            # 226 tokens at ViT-B/16's width
    with torch.device("meta"), pytest.raises(ValueError, match="not available"):
        VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim,
                          precision="f16x3")
