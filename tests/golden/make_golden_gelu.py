"""Generates the exact-GELU fixtures by EXECUTING THE REFERENCE with its MLP activation switched to nn.GELU.

Run in the development container only (needs the reference tree, see ref_harness.py):
    python tests/golden/make_golden_gelu.py

The reference's ResidualAttentionBlock looks `QuickGELU` up in its module when it is constructed; replacing that attribute by
torch.nn.GELU before construction is exactly what open_clip's config switch (`quick_gelu: false`) does.  Like make_golden_arch.py,
only DATA is stored: seeds and the outputs of the reference's own modules for weights drawn by anomalyclip_amd.init_weights and
inputs drawn by recipes.py (the GPU tests regenerate both from the seeds).
    vit_b16_gelu.npz, vit_l14_gelu.npz   the reference VisionTransformer with nn.GELU on 2 frames (recipes.vit_frames)
    text_gelu.npz                        the reference TextEncoder with nn.GELU at the ViT-B/16 text geometry (UCF prompts)
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_arch as A  # noqa: E402  (ref_modules(), save, gen_vit, gen_text)
from anomalyclip_amd import init_weights as IW  # noqa: E402

A.ns.clip_model.QuickGELU = torch.nn.GELU           # before any module is constructed

if __name__ == "__main__":
    probe = A.ns.clip_model.ResidualAttentionBlock(64, 1)
    assert isinstance(probe.mlp.gelu, torch.nn.GELU), "the reference no longer takes its activation from clip_model.QuickGELU"
    A.gen_vit("vit_b16_gelu", IW.VIT_B16, seed=71)
    A.gen_vit("vit_l14_gelu", IW.VIT_L14, seed=72)
    A.gen_text("text_gelu", IW.VIT_B16, seed=73)
