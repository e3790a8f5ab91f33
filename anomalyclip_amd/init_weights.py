"""Seeded random initialisation of an AnomalyCLIP state_dict with the REFERENCE's key names.

There is no network in the build/bench environment, hence no CLIP checkpoint and no published
AnomalyCLIP `.ckpt`.  Benchmarks, parity tests and golden fixtures therefore use random weights
drawn with CLIP's own initialisation scales (reference clip/model.py:352-384 and :254-264) so
activations have realistic magnitudes.  Biases / LayerNorm affines are perturbed away from their
0/1 defaults so that a kernel that drops a bias or a gain cannot pass parity.

Key layout == `AnomalyCLIP.state_dict()` of the reference (checkpoint row):
  image_encoder.*, text_encoder.*, token_embedding.weight, prompt_learner.{ctx,token_prefix,
  token_suffix}, selector_model.{logit_scale,bn_layer.*}, temporal_model.{projection,axial_attn,
  classifier}.*
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Tuple, Union

import torch


@dataclass
class ClipGeometry:
    """Constructor arguments of the reference CLIP (clip/model.py:294-308).  `vision_layers` is a tuple of four block counts for
    the ResNet image encoders (clip/model.py:313-321, vision_patch_size None), an int for the ViTs."""
    embed_dim: int = 512
    image_resolution: int = 224
    vision_layers: Union[int, Tuple[int, int, int, int]] = 12
    vision_width: int = 768
    vision_patch_size: Optional[int] = 16
    context_length: int = 77
    vocab_size: int = 49408
    transformer_width: int = 512
    transformer_heads: int = 8
    transformer_layers: int = 12
    act: str = "quick_gelu"     # the MLPs' activation: "quick_gelu" (OpenAI's checkpoints) or "gelu" (open_clip configs without quick_gelu);
                                # not a constructor argument of the reference's CLIP: as_kwargs() leaves it out
    vision_head_dim: int = 64   # the ViT image tower's head dimension: 64 for every CLIP of clip.load, 80 for open_clip's ViT-H-14 (its
                                # `head_width`).  The reference's CLIP always divides by 64: as_kwargs() leaves this out too

    @property
    def is_resnet(self) -> bool:
        return isinstance(self.vision_layers, (tuple, list))

    @property
    def vision_heads(self) -> int:
        if self.is_resnet:
            raise ValueError("vision_heads is a ViT field: a ResNet's attention pool has resnet_heads = vision_width * 32 // 64")
        return self.vision_width // self.vision_head_dim

    @property
    def grid(self) -> int:
        if self.is_resnet:
            raise ValueError("grid is a ViT field: a ResNet has no patch grid (its attention pool sees resolution // 32 squared)")
        return self.image_resolution // self.vision_patch_size

    @property
    def resnet_heads(self) -> int:
        """AttentionPool2d heads (clip/model.py:314): head dim 64 over the 32 * width features."""
        return self.vision_width * 32 // 64

    def as_kwargs(self) -> dict:
        return dict(embed_dim=self.embed_dim, image_resolution=self.image_resolution,
                    vision_layers=self.vision_layers, vision_width=self.vision_width,
                    vision_patch_size=self.vision_patch_size, context_length=self.context_length,
                    vocab_size=self.vocab_size, transformer_width=self.transformer_width,
                    transformer_heads=self.transformer_heads,
                    transformer_layers=self.transformer_layers)


VIT_B16 = ClipGeometry()
# the other ViT backbones of clip.load (clip/clip.py:31-41), with CLIP's published shapes
VIT_B32 = ClipGeometry(embed_dim=512, image_resolution=224, vision_layers=12, vision_width=768, vision_patch_size=32,
                       transformer_width=512, transformer_heads=8, transformer_layers=12)
VIT_L14 = ClipGeometry(embed_dim=768, image_resolution=224, vision_layers=24, vision_width=1024, vision_patch_size=14,
                       transformer_width=768, transformer_heads=12, transformer_layers=12)
VIT_L14_336 = ClipGeometry(embed_dim=768, image_resolution=336, vision_layers=24, vision_width=1024, vision_patch_size=14,
                           transformer_width=768, transformer_heads=12, transformer_layers=12)
# open_clip's ViT-H-14 (LAION-2B): 16 heads of 80 in the image tower, a 24-layer text tower of 16 heads of 64, exact GELU
VIT_H14 = ClipGeometry(embed_dim=1024, image_resolution=224, vision_layers=32, vision_width=1280, vision_patch_size=14, vision_head_dim=80,
                       transformer_width=1024, transformer_heads=16, transformer_layers=24, act="gelu")
# the ResNet backbones of clip.load (clip/clip.py:31-41), CLIP's published shapes (vision_layers: blocks of layer1..4)
RN50 = ClipGeometry(embed_dim=1024, image_resolution=224, vision_layers=(3, 4, 6, 3), vision_width=64, vision_patch_size=None,
                    transformer_width=512, transformer_heads=8, transformer_layers=12)
RN101 = ClipGeometry(embed_dim=512, image_resolution=224, vision_layers=(3, 4, 23, 3), vision_width=64, vision_patch_size=None,
                     transformer_width=512, transformer_heads=8, transformer_layers=12)
RN50X4 = ClipGeometry(embed_dim=640, image_resolution=288, vision_layers=(4, 6, 10, 6), vision_width=80, vision_patch_size=None,
                      transformer_width=640, transformer_heads=10, transformer_layers=12)
RN50X16 = ClipGeometry(embed_dim=768, image_resolution=384, vision_layers=(6, 8, 18, 8), vision_width=96, vision_patch_size=None,
                       transformer_width=768, transformer_heads=12, transformer_layers=12)
RN50X64 = ClipGeometry(embed_dim=1024, image_resolution=448, vision_layers=(3, 15, 36, 10), vision_width=128, vision_patch_size=None,
                       transformer_width=1024, transformer_heads=16, transformer_layers=12)
# tiny geometry used by fixtures (head dim stays 64 like every CLIP ViT of clip.load)
TINY = ClipGeometry(embed_dim=128, image_resolution=32, vision_layers=2, vision_width=128,
                    vision_patch_size=16, context_length=77, vocab_size=49408,
                    transformer_width=128, transformer_heads=2, transformer_layers=2)


@dataclass
class HeadConfig:
    """`net.*` keys of configs/model/anomaly_clip_*.yaml that shape the head."""
    num_classes: int = 14
    normal_id: int = 7
    n_ctx: int = 8
    shared_context: bool = False
    num_segments: int = 32
    seg_length: int = 16
    emb_size: int = 256
    depth: int = 1
    heads: int = 8
    dim_heads: Optional[int] = None
    concat_features: bool = False
    num_topk: int = 3
    num_bottomk: int = 3
    select_idx_dropout_topk: float = 0.7
    select_idx_dropout_bottomk: float = 0.7
    stride: int = 1
    ncrops: int = 1

    @property
    def e(self) -> int:
        return self.dim_heads if self.dim_heads else self.emb_size // self.heads


UCF_HEAD = HeadConfig()
SHT_HEAD = HeadConfig(num_classes=18, normal_id=8, depth=2, concat_features=True)
XD_HEAD = HeadConfig(num_classes=7, normal_id=4, emb_size=128, ncrops=5)


def _n(gen, *shape, std=1.0, mean=0.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float32) * std + mean


def _resblocks(sd: Dict[str, torch.Tensor], prefix: str, width: int, layers: int, gen):
    proj_std = (width ** -0.5) * ((2 * layers) ** -0.5)
    attn_std = width ** -0.5
    fc_std = (2 * width) ** -0.5
    for i in range(layers):
        p = f"{prefix}.resblocks.{i}."
        sd[p + "attn.in_proj_weight"] = _n(gen, 3 * width, width, std=attn_std)
        sd[p + "attn.in_proj_bias"] = _n(gen, 3 * width, std=0.02)
        sd[p + "attn.out_proj.weight"] = _n(gen, width, width, std=proj_std)
        sd[p + "attn.out_proj.bias"] = _n(gen, width, std=0.02)
        sd[p + "ln_1.weight"] = _n(gen, width, std=0.05, mean=1.0)
        sd[p + "ln_1.bias"] = _n(gen, width, std=0.02)
        sd[p + "mlp.c_fc.weight"] = _n(gen, 4 * width, width, std=fc_std)
        sd[p + "mlp.c_fc.bias"] = _n(gen, 4 * width, std=0.02)
        sd[p + "mlp.c_proj.weight"] = _n(gen, width, 4 * width, std=proj_std)
        sd[p + "mlp.c_proj.bias"] = _n(gen, width, std=0.02)
        sd[p + "ln_2.weight"] = _n(gen, width, std=0.05, mean=1.0)
        sd[p + "ln_2.bias"] = _n(gen, width, std=0.02)


def init_vit_state_dict(geom: ClipGeometry, seed: int, prefix: str = "image_encoder.") -> Dict[str, torch.Tensor]:
    gen = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    w = geom.vision_width
    scale = w ** -0.5
    ps = geom.vision_patch_size
    fan_in = 3 * ps * ps
    sd[prefix + "conv1.weight"] = _n(gen, w, 3, ps, ps, std=fan_in ** -0.5)
    sd[prefix + "class_embedding"] = _n(gen, w, std=scale)
    sd[prefix + "positional_embedding"] = _n(gen, geom.grid ** 2 + 1, w, std=scale)
    sd[prefix + "ln_pre.weight"] = _n(gen, w, std=0.05, mean=1.0)
    sd[prefix + "ln_pre.bias"] = _n(gen, w, std=0.02)
    _resblocks(sd, prefix + "transformer", w, geom.vision_layers, gen)
    sd[prefix + "ln_post.weight"] = _n(gen, w, std=0.05, mean=1.0)
    sd[prefix + "ln_post.bias"] = _n(gen, w, std=0.02)
    sd[prefix + "proj"] = _n(gen, w, geom.embed_dim, std=scale)
    return sd


def _bn(sd: Dict[str, torch.Tensor], p: str, c: int, gen, gamma: float = 1.0):
    """BatchNorm2d affine and running statistics, all perturbed away from 1 / 0 / 0 / 1 (a dropped or mis-folded BN fails)."""
    sd[p + "weight"] = _n(gen, c, std=0.05, mean=gamma)
    sd[p + "bias"] = _n(gen, c, std=0.05)
    sd[p + "running_mean"] = _n(gen, c, std=0.1)
    sd[p + "running_var"] = _n(gen, c, std=0.1, mean=1.0).abs() + 0.05
    sd[p + "num_batches_tracked"] = torch.tensor(0, dtype=torch.long)


def init_resnet_state_dict(geom: ClipGeometry, seed: int, prefix: str = "image_encoder.") -> Dict[str, torch.Tensor]:
    """Seeded weights of the reference ModifiedResNet (clip/model.py:111-171) under its own key names.  Convolutions at std
    sqrt(1.5 / fan_in); bn3 (and downsample.1) start at gamma ~0.5 instead of CLIP's zero (clip/model.py:364-372), which would
    make every residual branch dead in the tests.  With these scales 50-200 convolutions in eval mode keep the features at
    O(0.1-10) (reference outputs: std 0.22 for RN50 up to 5.0 for RN50x64)."""
    if not geom.is_resnet:
        raise ValueError("init_resnet_state_dict needs a ResNet geometry (vision_layers a tuple)")
    gen = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    w = geom.vision_width

    def conv(p, cout, cin, k):
        sd[p + "weight"] = _n(gen, cout, cin, k, k, std=(1.5 / (cin * k * k)) ** 0.5)
    conv(prefix + "conv1.", w // 2, 3, 3)
    _bn(sd, prefix + "bn1.", w // 2, gen)
    conv(prefix + "conv2.", w // 2, w // 2, 3)
    _bn(sd, prefix + "bn2.", w // 2, gen)
    conv(prefix + "conv3.", w, w // 2, 3)
    _bn(sd, prefix + "bn3.", w, gen)
    inplanes = w
    for li, blocks in enumerate(geom.vision_layers):
        planes = w * 2 ** li
        for j in range(blocks):
            p = f"{prefix}layer{li + 1}.{j}."
            conv(p + "conv1.", planes, inplanes, 1)
            _bn(sd, p + "bn1.", planes, gen)
            conv(p + "conv2.", planes, planes, 3)
            _bn(sd, p + "bn2.", planes, gen)
            conv(p + "conv3.", 4 * planes, planes, 1)
            _bn(sd, p + "bn3.", 4 * planes, gen, gamma=0.5)
            if j == 0 and (li > 0 or inplanes != 4 * planes):
                conv(p + "downsample.0.", 4 * planes, inplanes, 1)
                _bn(sd, p + "downsample.1.", 4 * planes, gen, gamma=0.5)
            inplanes = 4 * planes
    E = w * 32
    a = prefix + "attnpool."
    sd[a + "positional_embedding"] = _n(gen, (geom.image_resolution // 32) ** 2 + 1, E, std=E ** -0.5)
    for name in ("k_proj", "q_proj", "v_proj"):
        sd[a + name + ".weight"] = _n(gen, E, E, std=E ** -0.5)
        sd[a + name + ".bias"] = _n(gen, E, std=0.02)
    sd[a + "c_proj.weight"] = _n(gen, geom.embed_dim, E, std=E ** -0.5)
    sd[a + "c_proj.bias"] = _n(gen, geom.embed_dim, std=0.02)
    return sd


def init_text_state_dict(geom: ClipGeometry, seed: int) -> Dict[str, torch.Tensor]:
    gen = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    w = geom.transformer_width
    sd["token_embedding.weight"] = _n(gen, geom.vocab_size, w, std=0.02)
    sd["text_encoder.positional_embedding"] = _n(gen, geom.context_length, w, std=0.01)
    _resblocks(sd, "text_encoder.transformer", w, geom.transformer_layers, gen)
    sd["text_encoder.ln_final.weight"] = _n(gen, w, std=0.05, mean=1.0)
    sd["text_encoder.ln_final.bias"] = _n(gen, w, std=0.02)
    sd["text_encoder.text_projection"] = _n(gen, w, geom.embed_dim, std=w ** -0.5)
    return sd


def init_temporal_state_dict(in_size: int, hc: HeadConfig, seed: int,
                             prefix: str = "temporal_model.") -> Dict[str, torch.Tensor]:
    """Shapes follow temporal_model.py:31-40 and the restated axial_attention (oracle/)."""
    gen = torch.Generator().manual_seed(seed)
    sd: Dict[str, torch.Tensor] = {}
    E, H, e = hc.emb_size, hc.heads, hc.e
    he = H * e
    sd[prefix + "projection.weight"] = _n(gen, E, in_size, std=in_size ** -0.5)
    sd[prefix + "projection.bias"] = _n(gen, E, std=0.02)
    ax = prefix + "axial_attn."
    # upstream uses randn (std 1) for the axial positional embedding; keep that
    sd[ax + "pos_emb.param_0"] = _n(gen, 1, E, hc.num_segments, 1)
    sd[ax + "pos_emb.param_1"] = _n(gen, 1, E, 1, hc.seg_length)
    for d in range(hc.depth):
        for fg in ("f", "g"):
            a = f"{ax}layers.blocks.{2 * d}.{fg}.net.fn."
            sd[a + "norm.weight"] = _n(gen, E, std=0.05, mean=1.0)
            sd[a + "norm.bias"] = _n(gen, E, std=0.02)
            sd[a + "fn.to_q.weight"] = _n(gen, he, E, std=E ** -0.5)
            sd[a + "fn.to_kv.weight"] = _n(gen, 2 * he, E, std=E ** -0.5)
            sd[a + "fn.to_out.weight"] = _n(gen, E, he, std=he ** -0.5)
            sd[a + "fn.to_out.bias"] = _n(gen, E, std=0.02)
            c = f"{ax}layers.blocks.{2 * d + 1}.{fg}.net."
            sd[c + "0.g"] = _n(gen, 1, E, 1, 1, std=0.05, mean=1.0)
            sd[c + "0.b"] = _n(gen, 1, E, 1, 1, std=0.02)
            sd[c + "1.weight"] = _n(gen, 4 * E, E, 3, 3, std=(9 * E) ** -0.5)
            sd[c + "1.bias"] = _n(gen, 4 * E, std=0.02)
            sd[c + "3.weight"] = _n(gen, E, 4 * E, 3, 3, std=(36 * E) ** -0.5)
            sd[c + "3.bias"] = _n(gen, E, std=0.02)
    sd[prefix + "classifier.layer_norm.weight"] = _n(gen, E, std=0.05, mean=1.0)
    sd[prefix + "classifier.layer_norm.bias"] = _n(gen, E, std=0.02)
    sd[prefix + "classifier.linear.weight"] = _n(gen, 1, E, std=E ** -0.5)
    sd[prefix + "classifier.linear.bias"] = _n(gen, 1, std=0.02)
    return sd


def init_anomalyclip_state_dict(geom: ClipGeometry, hc: HeadConfig, tokenized_prompts: torch.Tensor,
                                seed: int, with_image_encoder: bool = True) -> Dict[str, torch.Tensor]:
    """Full `AnomalyCLIP.state_dict()`-shaped dict.  `tokenized_prompts`: (C, 77) int token ids of
    "X X X X X X X X <classname>." (reference coop.py:53-56)."""
    sd: Dict[str, torch.Tensor] = {}
    if with_image_encoder:
        sd.update(init_resnet_state_dict(geom, seed + 1) if geom.is_resnet else init_vit_state_dict(geom, seed + 1))
    sd.update(init_text_state_dict(geom, seed + 2))
    gen = torch.Generator().manual_seed(seed + 3)
    C, w = hc.num_classes, geom.transformer_width
    if hc.shared_context:
        sd["prompt_learner.ctx"] = _n(gen, hc.n_ctx, w, std=0.02)
    else:
        sd["prompt_learner.ctx"] = _n(gen, C, hc.n_ctx, w, std=0.02)
    emb = sd["token_embedding.weight"][tokenized_prompts.long()]  # (C, 77, w) coop.py:57-60
    sd["prompt_learner.token_prefix"] = emb[:, :1, :].clone()           # coop.py:65
    sd["prompt_learner.token_suffix"] = emb[:, 1 + hc.n_ctx:, :].clone()  # coop.py:66
    sd["selector_model.logit_scale"] = torch.tensor(math.log(1 / 0.07), dtype=torch.float32)
    sd["selector_model.bn_layer.running_mean"] = _n(gen, C - 1, std=0.05)
    sd["selector_model.bn_layer.running_var"] = _n(gen, C - 1, std=0.02).abs() + 0.05
    sd["selector_model.bn_layer.num_batches_tracked"] = torch.tensor(0, dtype=torch.long)
    in_size = geom.embed_dim + (C - 1) * int(hc.concat_features)
    sd.update(init_temporal_state_dict(in_size, hc, seed + 4))
    return sd
