"""Generates the fixtures of the CLIP ResNet backbones (RN50, RN101, RN50x4, RN50x16, RN50x64) by EXECUTING THE REFERENCE.

Run in the development container only (needs the reference tree, see ref_harness.py):
    python tests/golden/make_golden_resnet.py

Like make_golden_arch.py, only DATA is stored: seeds and the outputs of the reference's own modules for weights drawn by
anomalyclip_amd.init_weights.init_resnet_state_dict and frames drawn by recipes.vit_frames (the GPU tests regenerate both).
    rn50.npz, rn101.npz, rn50x4.npz, rn50x16.npz, rn50x64.npz   the reference ModifiedResNet.eval() on 2 frames
    rn_train.npz                                                the reference RN50 encoder in .train() on 4 frames: output, running
                                                                statistics of named BatchNorms, checksums over all running buffers,
                                                                num_batches_tracked, and .eval() on 2 frames afterwards
    e2e_rn50x4.npz                                              the reference AnomalyCLIP(arch = "RN50x4") on 640-wide seeded
                                                                features, test and train forward (UCF head)
    text_rn50x64.npz                                            the reference TextEncoder at width 1024 (UCF prompts)
    rn_shapes.json                                              every parameter / buffer name and shape of CLIP(**geometry),
                                                                and whether the reference AnomalyCLIP(arch="RN50") forward raised
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
ARCHS = {"RN50": IW.RN50, "RN101": IW.RN101, "RN50x4": IW.RN50X4, "RN50x16": IW.RN50X16, "RN50x64": IW.RN50X64}
SEEDS = {"RN50": 71, "RN101": 72, "RN50x4": 73, "RN50x16": 74, "RN50x64": 75}


def save(name, **arrs):
    arrs = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print(f"{name}.npz  {os.path.getsize(path) / 1024:.1f} KiB")


def prompts(key="ucf"):
    with open(os.path.join(REPO, "anomalyclip_amd", "data", "prompts.json")) as f:
        return json.load(f)[key]


def gen_resnet(arch, nframes=2):
    geom, seed = ARCHS[arch], SEEDS[arch]
    sd = IW.init_resnet_state_dict(geom, seed, prefix="")
    m = ns.clip_model.ModifiedResNet(geom.vision_layers, geom.embed_dim, geom.resnet_heads, geom.image_resolution, geom.vision_width)
    m.load_state_dict(sd, strict=True)
    m.eval()
    frames = R.vit_frames(seed, nframes, geom.image_resolution)
    out = m(frames)
    print(arch, "output |max|", float(out.abs().max()), "std", float(out.std()))
    save(arch.lower(), seed=seed, frames_checksum=frames.double().sum(), out=out)


TRAIN_BNS = ("bn1", "bn2", "bn3", "layer1.0.downsample.1", "layer4.2.bn3")


def gen_train(seed=78, nframes=4):
    geom = IW.RN50
    sd = IW.init_resnet_state_dict(geom, seed, prefix="")
    m = ns.clip_model.ModifiedResNet(geom.vision_layers, geom.embed_dim, geom.resnet_heads, geom.image_resolution, geom.vision_width)
    m.load_state_dict(sd, strict=True)
    m.train()
    frames = R.vit_frames(seed, nframes, geom.image_resolution)
    out = m(frames)
    msd = m.state_dict()
    arrs = dict(seed=seed, frames_checksum=frames.double().sum(), out=out)
    for name in TRAIN_BNS:
        arrs[f"{name}.running_mean"] = msd[name + ".running_mean"]
        arrs[f"{name}.running_var"] = msd[name + ".running_var"]
    run = [v.double() for k, v in msd.items() if k.endswith(("running_mean", "running_var"))]
    arrs["running_sum"] = sum(float(v.sum()) for v in run)
    arrs["running_abs_sum"] = sum(float(v.abs().sum()) for v in run)
    arrs["num_batches_tracked"] = np.array([int(v) for k, v in msd.items() if k.endswith("num_batches_tracked")])
    m.eval()
    arrs["eval_after"] = m(frames[:2])
    save("rn_train", **arrs)


E2E_HEAD = dict(emb_size=256, heads=8, depth=1)     # the UCF head of configs/model/anomaly_clip_ucf.yaml


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


def rn50_in_anomalyclip_raises():
    """The reference's AnomalyCLIP(arch="RN50"): embedding_dim (512, ln_final) against 1024-wide image features."""
    geom = IW.RN50
    H.patch_clip_load(ns, geom.as_kwargs(), 76)
    cfgs = dict(arch="RN50", labels_file=os.path.join(H.REF_ROOT, "data/ucf_labels.csv"), emb_size=256, depth=1, heads=8,
                dim_heads=None, num_segments=32, seg_length=16, concat_features=False, normal_id=7, stride=1,
                load_from_features=True, select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3,
                num_bottomk=3, n_ctx=8, shared_context=False, ctx_init="")
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            net = ns.anomaly_clip.AnomalyCLIP(**cfgs)
            net.eval()
            feats = torch.randn(1, 1, 32 * 16 * 2, geom.embed_dim)
            net(feats, torch.zeros(1000), torch.zeros(geom.embed_dim), 2, True)
    except Exception as e:                           # noqa: BLE001 -- the reference's own exception is what is recorded
        return True, f"{type(e).__name__}: {e}"[:300]
    return False, ""


def gen_shapes():
    out = {}
    for arch, geom in ARCHS.items():
        torch.manual_seed(0)
        with torch.device("meta"):
            m = ns.clip_model.CLIP(**geom.as_kwargs())
        out[arch] = {k: list(v.shape) for k, v in m.state_dict().items()}
    raised, msg = rn50_in_anomalyclip_raises()
    out["_reference_rn50_anomalyclip_raised"] = raised
    out["_reference_rn50_anomalyclip_error"] = msg
    path = os.path.join(OUT, "rn_shapes.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
    print(f"rn_shapes.json  {os.path.getsize(path) / 1024:.1f} KiB  (RN50 in AnomalyCLIP raised: {raised} {msg})")


if __name__ == "__main__":
    which = set(sys.argv[1:]) or {"shapes", "resnet", "text", "train", "e2e"}
    if "shapes" in which:
        gen_shapes()
    if "resnet" in which:
        for a in ARCHS:
            gen_resnet(a)
    if "text" in which:
        gen_text("text_rn50x64", IW.RN50X64, seed=77)
    if "train" in which:
        gen_train()
    if "e2e" in which:
        gen_e2e("e2e_rn50x4", "RN50x4", seed=79)
