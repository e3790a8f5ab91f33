"""Generates the fixtures of the other CLIP ViT backbones (ViT-B/32, ViT-L/14, ViT-L/14@336px) by EXECUTING THE REFERENCE.

Run in the development container only (needs the reference tree, see ref_harness.py):
    python tests/golden/make_golden_arch.py

Like make_golden.py, only DATA is stored: seeds and the outputs of the reference's own modules for weights drawn by
anomalyclip_amd.init_weights and inputs drawn by recipes.py (the GPU tests regenerate both from the seeds).
    vit_b32.npz, vit_l14.npz, vit_l14_336.npz   the reference VisionTransformer on 2 frames (recipes.vit_frames)
    text_l14.npz                                the reference TextEncoder at the ViT-L/14 text geometry (UCF prompts)
    e2e_l14.npz                                 the reference AnomalyCLIP(arch = "ViT-L/14") on 768-wide seeded features,
                                                test and train forward (UCF head)
    arch_shapes.json                            every parameter / buffer name and shape of the reference CLIP(**geometry)
"""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, REPO)

import ref_harness as H  # noqa: E402
import recipes as R  # noqa: E402
from anomalyclip_amd import init_weights as IW  # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(16)
ns = H.ref_modules()
OUT = HERE
ARCHS = {"ViT-B/16": IW.VIT_B16, "ViT-B/32": IW.VIT_B32, "ViT-L/14": IW.VIT_L14, "ViT-L/14@336px": IW.VIT_L14_336}
E2E_HEAD = dict(emb_size=256, heads=8, depth=1)     # the UCF head of configs/model/anomaly_clip_ucf.yaml


def save(name, **arrs):
    arrs = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def prompts(key="ucf"):
    with open(os.path.join(REPO, "anomalyclip_amd", "data", "prompts.json")) as f:
        return json.load(f)[key]


def gen_vit(tag, geom, seed, nframes=2):
    sd = IW.init_vit_state_dict(geom, seed, prefix="")
    vit = ns.clip_model.VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width,
                                          geom.vision_layers, geom.vision_heads, geom.embed_dim)
    vit.load_state_dict(sd, strict=True)
    vit.eval()
    frames = R.vit_frames(seed, nframes, geom.image_resolution)
    save(tag, seed=seed, frames_seed=seed + 100, frames_checksum=frames.double().sum(), out=vit(frames))


def gen_text(tag, geom, seed, key="ucf"):
    p = prompts(key)
    toks = torch.tensor(p["tokenized_prompts"], dtype=torch.int32)
    hc = IW.HeadConfig(num_classes=toks.shape[0], normal_id=p["normal_id"])
    sd = IW.init_anomalyclip_state_dict(geom, hc, toks, seed, with_image_encoder=False)
    torch.manual_seed(0)
    clip_model = ns.clip_model.CLIP(**geom.as_kwargs()).float()
    te = ns.text_encoder.TextEncoder(clip_model)
    te.load_state_dict({k[len("text_encoder."):]: v for k, v in sd.items() if k.startswith("text_encoder.")}, strict=True)
    pr = torch.cat([sd["prompt_learner.token_prefix"], sd["prompt_learner.ctx"], sd["prompt_learner.token_suffix"]], dim=1)
    save(tag, seed=seed, out=te(pr, toks), eot=toks.argmax(-1))


def gen_e2e(tag, arch, seed):
    geom = ARCHS[arch]
    p = prompts("ucf")
    toks = torch.tensor(p["tokenized_prompts"], dtype=torch.int32)
    hc = IW.HeadConfig(num_classes=14, normal_id=7, **E2E_HEAD)
    sd = IW.init_anomalyclip_state_dict(geom, hc, toks, seed)
    H.patch_clip_load(ns, geom.as_kwargs(), seed)
    cfgs = dict(arch=arch, labels_file=os.path.join(H.REF_ROOT, "data/ucf_labels.csv"), emb_size=hc.emb_size,
                depth=hc.depth, heads=hc.heads, dim_heads=None, num_segments=32, seg_length=16,
                concat_features=False, normal_id=7, stride=1, load_from_features=True,
                select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3,
                num_bottomk=3, n_ctx=8, shared_context=False, ctx_init="")
    with contextlib.redirect_stdout(io.StringIO()):
        net = ns.anomaly_clip.AnomalyCLIP(**cfgs)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    assert torch.equal(net.tokenized_prompts, toks)
    inp = R.e2e_inputs(seed, geom.embed_dim)
    nc = inp["nc"]
    arrs = dict(seed=seed, emb_size=hc.emb_size, heads=hc.heads, depth=hc.depth)
    net.eval()
    sim, sc = net(inp["test_feats"], torch.zeros(1000), nc, 2, True)
    arrs.update(test_sim=sim, test_scores=sc)
    net.train()
    m1 = inp["mask"]
    net.selector_model.generate_mask = lambda logits: (
        m1.unsqueeze(2).expand(-1, -1, logits.shape[-1]), m1.unsqueeze(2).expand(-1, -1, logits.shape[-1]))
    lg, lt, sc, ia, in_, ba = net(inp["train_feats"], inp["labels"], nc)
    arrs.update(train_logits=lg, train_logits_topk=lt, train_scores=sc, idx_topk_abn=ia, idx_topk_nor=in_, idx_bottomk_abn=ba,
                rm1=net.selector_model.bn_layer.running_mean, rv1=net.selector_model.bn_layer.running_var)
    arrs["axial_source"] = H.AXIAL_SOURCE
    save(tag, **arrs)


def gen_shapes():
    out = {}
    for arch, geom in ARCHS.items():
        torch.manual_seed(0)
        with torch.device("meta"):
            m = ns.clip_model.CLIP(**geom.as_kwargs())
        out[arch] = {k: list(v.shape) for k, v in m.state_dict().items()}
    path = os.path.join(OUT, "arch_shapes.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(f"arch_shapes.json  {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    which = set(sys.argv[1:]) or {"shapes", "vit", "text", "e2e"}
    if "shapes" in which:
        gen_shapes()
    if "vit" in which:
        gen_vit("vit_b32", IW.VIT_B32, seed=61)
        gen_vit("vit_l14", IW.VIT_L14, seed=62)
        gen_vit("vit_l14_336", IW.VIT_L14_336, seed=63)
    if "text" in which:
        gen_text("text_l14", IW.VIT_L14, seed=64)
    if "e2e" in which:
        gen_e2e("e2e_l14", "ViT-L/14", seed=65)
