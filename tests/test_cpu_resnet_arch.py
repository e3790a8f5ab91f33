"""The CLIP ResNet backbones selected by `net.arch` (RN50, RN101, RN50x4, RN50x16, RN50x64): geometry registry, the mirror's
parameter and buffer names and shapes against the reference's CLIP(**geometry) (tests/golden/rn_shapes.json,
make_golden_resnet.py), the seeded weights, checkpoint geometry detection and the errors raised before any GPU work.  No GPU
needed: modules are built on the meta device where they would be large."""
import json
import os

import pytest
import torch

from anomalyclip_amd import init_weights as IW
from anomalyclip_amd.components import anomaly_clip as AC
from anomalyclip_amd.components.clip_resnet import ModifiedResNet, check_resnet_precision
from anomalyclip_amd.components.text_encoder import TextEncoder

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RN_ARCHS = ("RN50", "RN101", "RN50x4", "RN50x16", "RN50x64")
PUBLISHED = {   # layers, width, resolution, attnpool tokens, heads, embed, text width / heads (CLIP's released models)
    "RN50": ((3, 4, 6, 3), 64, 224, 50, 32, 1024, 512, 8),
    "RN101": ((3, 4, 23, 3), 64, 224, 50, 32, 512, 512, 8),
    "RN50x4": ((4, 6, 10, 6), 80, 288, 82, 40, 640, 640, 10),
    "RN50x16": ((6, 8, 18, 8), 96, 384, 145, 48, 768, 768, 12),
    "RN50x64": ((3, 15, 36, 10), 128, 448, 197, 64, 1024, 1024, 16),
}


def _shapes():
    with open(os.path.join(GOLDEN, "rn_shapes.json")) as f:
        return json.load(f)


def _net_kw(**kw):
    base = dict(labels_key="ucf", emb_size=64, depth=1, heads=2, dim_heads=None, num_segments=32, seg_length=16,
                concat_features=False, normal_id=7, stride=1, load_from_features=True, select_idx_dropout_topk=0.7,
                select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3)
    base.update(kw)
    return base


def _mirror(g, arch):
    return ModifiedResNet(g.vision_layers, g.embed_dim, g.resnet_heads, g.image_resolution, g.vision_width, arch=arch)


@pytest.mark.parametrize("arch", RN_ARCHS)
def test_registry_and_published_shapes(arch):
    g = AC.geometry_of_arch(arch)
    layers, w, res, tokens, heads, embed, tw, th = PUBLISHED[arch]
    assert g.is_resnet and tuple(g.vision_layers) == layers and g.vision_width == w and g.image_resolution == res
    assert (g.image_resolution // 32) ** 2 + 1 == tokens and g.resnet_heads == heads and g.embed_dim == embed
    assert (g.transformer_width, g.transformer_heads, g.transformer_layers) == (tw, th, 12)
    with pytest.raises(ValueError):
        g.grid
    with pytest.raises(ValueError):
        g.vision_heads
    assert not IW.VIT_B16.is_resnet and IW.VIT_B16.grid == 14 and IW.VIT_B16.vision_heads == 12


@pytest.mark.parametrize("arch", RN_ARCHS)
def test_mirror_state_dict_matches_reference_clip(arch):
    """Every name and shape of the reference CLIP(**geometry), BatchNorm buffers included: visual.* = the ResNet mirror,
    the rest = the text encoder and the token embedding."""
    ref = _shapes()[arch]
    g = AC._ARCH[arch]
    with torch.device("meta"):
        rn = _mirror(g, arch)
        te = TextEncoder(g.context_length, g.transformer_width, g.transformer_heads, g.transformer_layers, g.embed_dim)
        tok = AC._TokenEmbedding(g.vocab_size, g.transformer_width)
    mine = {"visual." + k: list(v.shape) for k, v in rn.state_dict().items()}
    mine.update({k: list(v.shape) for k, v in te.state_dict().items()})
    mine["token_embedding.weight"] = list(tok.weight.shape)
    want = {k: v for k, v in ref.items() if k != "logit_scale"}
    assert mine == want
    assert any(k.endswith("downsample.1.num_batches_tracked") for k in mine)


@pytest.mark.parametrize("arch", ["RN50", "RN50x4"])
def test_init_resnet_state_dict_loads_strictly(arch):
    g = AC._ARCH[arch]
    sd = IW.init_resnet_state_dict(g, 3, prefix="")
    with torch.device("meta"):
        rn = _mirror(g, arch)
    want = {k: tuple(v.shape) for k, v in rn.state_dict().items()}
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    # BatchNorms perturbed away from their defaults; bn3 not zero (a dead residual branch would hide a wrong epilogue)
    for k, v in sd.items():
        if k.endswith(".weight") and ".bn" in k:
            assert (v - 1).abs().max() > 0 and v.abs().min() > 0.1, k
        if k.endswith("running_mean"):
            assert v.abs().max() > 0, k
        if k.endswith("running_var"):
            assert (v - 1).abs().max() > 0 and v.min() > 0, k


@pytest.mark.parametrize("arch", RN_ARCHS)
def test_geometry_from_state_dict(arch):
    g = AC._ARCH[arch]
    with torch.device("meta"):
        rn = _mirror(g, arch)
    sd = {"image_encoder." + k: v for k, v in rn.state_dict().items()}
    sd["text_encoder.positional_embedding"] = torch.empty(77, g.transformer_width, device="meta")
    for i in range(12):
        sd[f"text_encoder.transformer.resblocks.{i}.ln_1.weight"] = torch.empty(g.transformer_width, device="meta")
    assert AC.geometry_from_state_dict(sd) == g


def test_cross_family_checkpoints_are_refused():
    """ViT-B/16 weights into an RN101 module and RN101 weights into a ViT-B/16 module: the "do not match arch" ValueError
    naming both geometries."""
    vit_sd = {"image_encoder." + k: v for k, v in IW.init_vit_state_dict(IW.VIT_B16, 1, prefix="").items()}
    rn_sd = IW.init_resnet_state_dict(IW.RN101, 1)
    net = AC.AnomalyCLIP(arch="RN101", **_net_kw())
    with pytest.raises(ValueError, match="do not match arch 'RN101'.*ViT-B/16.*RN101"):
        net.load_state_dict(vit_sd, strict=False)
    net = AC.AnomalyCLIP(arch="ViT-B/16", **_net_kw())
    with pytest.raises(ValueError, match="do not match arch 'ViT-B/16'.*ResNet width 64.*ViT-B/16"):
        net.load_state_dict(rn_sd, strict=False)


@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "f16x3"])
def test_precision_refusals(precision):
    with pytest.raises(ValueError, match="not available for RN50x16"):
        check_resnet_precision(precision, "RN50x16")
    with pytest.raises(ValueError, match="not available for RN101"):
        AC.AnomalyCLIP(arch="RN101", precision=precision, **_net_kw())
    check_resnet_precision("auto", "RN50x16")
    check_resnet_precision("f32", "RN50x16")


def test_rn50_in_anomalyclip_names_both_widths():
    """The reference cannot run AnomalyCLIP(arch="RN50") (rn_shapes.json records its own exception): 1024-wide image features
    against the 512-wide text tower.  The mirror refuses it at construction."""
    assert _shapes()["_reference_rn50_anomalyclip_raised"] is True
    with pytest.raises(ValueError, match="1024.*512"):
        AC.AnomalyCLIP(arch="RN50", **_net_kw())


def test_resnet_width_must_be_a_multiple_of_8():
    with pytest.raises(ValueError, match="multiple of 8"):
        with torch.device("meta"):
            ModifiedResNet((1, 1, 1, 1), 64, 2, 64, 36)


def test_unknown_arch_lists_the_resnets():
    with pytest.raises(ValueError) as e:
        AC.geometry_of_arch("RN152")
    for a in RN_ARCHS + ("ViT-B/16", "ViT-L/14@336px"):
        assert repr(a) in str(e.value)
