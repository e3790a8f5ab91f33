"""Generates the ViT-H-14 fixtures by EXECUTING THE REFERENCE's modules at open_clip's ViT-H-14 geometry with nn.GELU.

Run in the development container only (needs the reference tree, see ref_harness.py):
    python tests/golden/make_golden_h14.py [shapes] [vit] [text]

The reference's CLIP class derives the image tower's head count as vision_width // 64 = 20; ViT-H-14 has 16 heads of 80.  The image
fixture therefore comes from the reference's VisionTransformer, built directly with 16 heads (make_golden_arch.gen_vit, which reads
geom.vision_heads); there is no end-to-end fixture through CLIP.  The text tower (width 1024, 16 heads of 64, 24 layers) is the
reference's own TextEncoder.  As in make_golden_gelu.py the activation is switched by replacing clip_model.QuickGELU before any module
is constructed, and only DATA is stored: seeds and outputs for weights drawn by anomalyclip_amd.init_weights and inputs drawn by
recipes.py.
    vit_h14.npz       the reference VisionTransformer(224, 14, 1280, 32, 16, 1024) with nn.GELU on 2 frames (recipes.vit_frames)
    text_h14.npz      the reference TextEncoder with nn.GELU at the ViT-H-14 text geometry (UCF prompts)
    h14_shapes.json   {"ViT-H-14": {name: shape}} in arch_shapes.json's format: `visual.*` from that VisionTransformer, everything
                      else from CLIP(**geometry) (whose own `visual.*`, the 20-head tower, is dropped: the shapes are the same, the
                      head count is not a shape)
"""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_arch as A  # noqa: E402  (ref_modules(), save, gen_vit, gen_text)
from anomalyclip_amd import init_weights as IW  # noqa: E402

A.ns.clip_model.QuickGELU = torch.nn.GELU           # before any module is constructed
G = IW.VIT_H14


def gen_shapes():
    with torch.device("meta"):
        vit = A.ns.clip_model.VisionTransformer(G.image_resolution, G.vision_patch_size, G.vision_width, G.vision_layers, G.vision_heads,
                                                G.embed_dim)
        clip = A.ns.clip_model.CLIP(**G.as_kwargs())
    out = {"visual." + k: list(v.shape) for k, v in vit.state_dict().items()}
    out.update({k: list(v.shape) for k, v in clip.state_dict().items() if not k.startswith("visual.")})
    path = os.path.join(A.OUT, "h14_shapes.json")
    with open(path, "w") as f:
        json.dump({"ViT-H-14": out}, f, indent=0, sort_keys=True)
    print(f"h14_shapes.json  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    probe = A.ns.clip_model.ResidualAttentionBlock(64, 1)
    assert isinstance(probe.mlp.gelu, torch.nn.GELU), "the reference no longer takes its activation from clip_model.QuickGELU"
    assert G.vision_heads == 16 and G.vision_width // G.vision_heads == 80
    which = set(sys.argv[1:]) or {"shapes", "vit", "text"}
    if "shapes" in which:
        gen_shapes()
    if "vit" in which:
        A.gen_vit("vit_h14", G, seed=81)
    if "text" in which:
        A.gen_text("text_h14", G, seed=82)
