"""Generates the segment-grid fixtures e2e_grid_<N>x<L>.npz by EXECUTING THE REFERENCE at grids other than 32 x 16.

Run in the development container only (needs the reference tree, see ref_harness.py):
    python tests/golden/make_golden_grid.py

Like make_golden.py, only DATA is stored: seeds and the outputs of the reference's own AnomalyCLIP (tiny CLIP geometry) and
ComputeLoss for weights drawn by anomalyclip_amd.init_weights and inputs drawn by recipes_grid.py (the tests regenerate both
from the seeds).  Per grid of recipes_grid.GRIDS: test-mode similarity / scores at segment size S, the train-forward outputs
of four videos (logits, logits_topk, scores, the three index tensors, BatchNorm running statistics) and the eight loss terms.
Before a file is written the oracle's segment indices are asserted equal to the reference's (a tie would make the fixture
depend on torch.topk's tie order)."""
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
import recipes_grid as RG  # noqa: E402
from anomalyclip_amd import init_weights as IW  # noqa: E402
from oracle import anomalyclip_oracle as O  # noqa: E402

torch.set_grad_enabled(False)
torch.set_num_threads(16)
ns = H.ref_modules()
OUT = HERE
MAX_BYTES = 341 * 1024          # e2e_tiny.npz, the largest fixture present


def gen_grid(tag, hc, S, seed):
    geom = IW.TINY
    with open(os.path.join(REPO, "anomalyclip_amd", "data", "prompts.json")) as f:
        toks = torch.tensor(json.load(f)["ucf"]["tokenized_prompts"], dtype=torch.int32)
    sd = IW.init_anomalyclip_state_dict(geom, hc, toks, seed)
    H.patch_clip_load(ns, geom.as_kwargs(), seed)
    cfgs = dict(arch="ViT-B/16", labels_file=os.path.join(H.REF_ROOT, "data/ucf_labels.csv"), emb_size=hc.emb_size,
                depth=hc.depth, heads=hc.heads, dim_heads=hc.dim_heads, num_segments=hc.num_segments, seg_length=hc.seg_length,
                concat_features=hc.concat_features, normal_id=hc.normal_id, stride=1, load_from_features=True,
                select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=hc.num_topk,
                num_bottomk=hc.num_bottomk, n_ctx=8, shared_context=False, ctx_init="")
    with contextlib.redirect_stdout(io.StringIO()):
        net = ns.anomaly_clip.AnomalyCLIP(**cfgs)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and not missing, (missing, unexpected)
    assert torch.equal(net.tokenized_prompts, toks)
    inp = RG.grid_inputs(seed, geom.embed_dim, hc, S)
    nc = inp["nc"]
    arrs = dict(seed=seed, S=S, num_segments=hc.num_segments, seg_length=hc.seg_length, emb_size=hc.emb_size, heads=hc.heads,
                dim_heads=hc.dim_heads or 0, depth=hc.depth, concat_features=int(hc.concat_features))
    net.eval()
    sim, sc = net(inp["test_feats"], torch.zeros(inp["test_feats"].shape[2]), nc, S, True)
    arrs.update(test_sim=sim, test_scores=sc)
    net.train()
    m1 = inp["mask"]
    net.selector_model.generate_mask = lambda logits: (
        m1.unsqueeze(2).expand(-1, -1, logits.shape[-1]), m1.unsqueeze(2).expand(-1, -1, logits.shape[-1]))
    lg, lt, scr, ia, in_, ba = net(inp["train_feats"], inp["labels"], nc)
    crit = ns.loss.ComputeLoss(hc.normal_id, hc.num_topk, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, hc.seg_length, hc.num_segments)
    outs = crit(lg, lt, inp["labels"].clone(), scr, ia, in_, ba)
    arrs.update(train_logits=lg, train_logits_topk=lt, train_scores=scr, idx_topk_abn=ia, idx_topk_nor=in_, idx_bottomk_abn=ba,
                losses=torch.stack([o.detach() for o in outs]),
                rm1=net.selector_model.bn_layer.running_mean, rv1=net.selector_model.bn_layer.running_var)
    arrs["axial_source"] = H.AXIAL_SOURCE
    # the oracle must pick the same segments
    eot = toks.argmax(-1)
    o = O.anomaly_clip_forward_train(sd, hc, inp["train_feats"], inp["labels"], nc, eot, geom.transformer_heads, m1, m1)
    assert torch.equal(o[3], ia) and torch.equal(o[4], in_) and torch.equal(o[5], ba), f"{tag}: oracle and reference indices differ"
    arrs = {k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v)) for k, v in arrs.items()}
    path = os.path.join(OUT, f"e2e_grid_{tag}.npz")
    np.savez_compressed(path, **arrs)
    size = os.path.getsize(path)
    print(f"e2e_grid_{tag}.npz  {size / 1024:.1f} KiB")
    assert size < MAX_BYTES, f"{path}: {size} bytes, above the largest fixture present"


if __name__ == "__main__":
    which = set(sys.argv[1:]) or set(RG.GRIDS)
    for tag, (hc, S, seed) in RG.GRIDS.items():
        if tag in which:
            gen_grid(tag, hc, S, seed)
