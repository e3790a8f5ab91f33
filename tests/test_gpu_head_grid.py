"""-m gpu: the temporal head on segment grids other than 32 x 16 -- the axial attention kernels across their domain (axis length
1 ... 128, head dimension 16 / 32 / 64) against the fp64 formula, the assembled head against fixtures the REFERENCE produced at three
other grids (e2e_grid_*.npz) and against the oracle at head widths the real kernels run, one training step against the fp64 oracle,
the whole-step graph against the autograd path, and a feature file through FeatureStream at a 24 x 10 grid.  Every bound is the
bound of the 32 x 16 test it restates (named per test)."""
import functools
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.loss import ComputeLoss
from oracle import anomalyclip_oracle as O
import recipes as R
import recipes_grid as RG
from test_gpu_model import TOL, elem_ok, relerr
from test_gpu_train import _check_leaky_report, _leaky_sides

DEV = "cuda"


def HC(N, L, E, heads, dim_heads=None, depth=1, concat=False):
    return IW.HeadConfig(num_classes=14, normal_id=7, num_segments=N, seg_length=L, emb_size=E, heads=heads, dim_heads=dim_heads,
                         depth=depth, concat_features=concat)


# head widths the real kernels run, on ViT-B/16 features (512 wide)
FULL = {"64x16": HC(64, 16, 256, 8),                       # power-of-two grid: plane convolutions under "auto"
        "16x32": HC(16, 32, 128, 8),                       # gl = 32: the non-fastconv branch of the weight-gradient kernel
        "24x10": HC(24, 10, 256, 4),                       # e = 64, f32 convolutions
        "40x12": HC(40, 12, 128, 8, depth=2, concat=True)}


@functools.lru_cache(maxsize=None)
def _toks():
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anomalyclip_amd", "data", "prompts.json")) as f:
        return torch.tensor(json.load(f)["ucf"]["tokenized_prompts"], dtype=torch.int32)


def build_grid_net(geom_name, hc, seed, **kw):
    """test_gpu_model.build_net with the head configuration's own grid"""
    geom = IW.TINY if geom_name == "tiny" else IW.VIT_B16
    toks = _toks()
    net = AnomalyCLIP(arch=geom_name, labels_key="ucf", emb_size=hc.emb_size, depth=hc.depth, heads=hc.heads, dim_heads=hc.dim_heads,
                      num_segments=hc.num_segments, seg_length=hc.seg_length, concat_features=hc.concat_features,
                      normal_id=hc.normal_id, stride=1, load_from_features=True, select_idx_dropout_topk=0.7,
                      select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=hc.num_topk, num_bottomk=hc.num_bottomk, n_ctx=8,
                      shared_context=False, ctx_init="", **kw)
    sd = IW.init_anomalyclip_state_dict(geom, hc, toks, seed)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not missing and not unexpected, (missing, unexpected)
    return net.to(DEV), sd, toks.argmax(-1)


# ====================================================================================================== kernel level
def _axial_ref(qkv, tiles, N, Lg, heads, e, axis):
    """the fp64 formula of test_gpu_kernels.test_axial_attention; returns (qkv leaf, out) with autograd on"""
    He = heads * e
    t = qkv.clone().double().requires_grad_(True)
    q, k, v = t.view(tiles, N, Lg, 3, heads, e).permute(3, 0, 1, 2, 4, 5)
    if axis == 0:
        q, k, v = (z.transpose(1, 2) for z in (q, k, v))
    q, k, v = (z.transpose(2, 3) for z in (q, k, v))
    o = (torch.softmax(q @ k.transpose(-1, -2) * e ** -0.5, -1) @ v).transpose(2, 3)
    if axis == 0:
        o = o.transpose(1, 2)
    return t, o.reshape(tiles * N * Lg, He)


# (T, other axis): every T of {1, 4, 5, 7, 8, 10, 12, 20, 24, 40, 48, 64, 96, 128}, the other axis mostly not a multiple of 16
FWD_T = [(1, 7), (4, 128), (5, 7), (7, 5), (8, 48), (10, 24), (12, 40), (20, 20), (24, 10), (40, 12), (48, 8), (64, 16), (96, 3),
         (128, 4)]
# e and heads rotate over the sweep (each of e in {16, 32, 64} x heads in {1, 2, 8} appears; both axes for every T)
FWD_CASES = [(T, oth, (16, 32, 64)[(i + a) % 3], (1, 2, 8)[(i // 3 + a) % 3], a) for i, (T, oth) in enumerate(FWD_T) for a in (0, 1)]
FWD_CASES += [(64, 64, 64, 1, 0), (128, 5, 64, 8, 1), (20, 20, 64, 4, 0), (96, 6, 16, 8, 0), (7, 5, 64, 2, 1), (16, 10, 64, 2, 0),
              (32, 12, 64, 2, 1)]


@pytest.mark.parametrize("T,other,e,heads,axis", FWD_CASES)
def test_axial_attention_grid(T, other, e, heads, axis):
    """ops.axial_attention across the domain against the fp64 formula, at test_axial_attention's bound"""
    N, Lg = (T, other) if axis == 0 else (other, T)
    tiles = 3
    g = torch.Generator().manual_seed(1000 * T + 10 * e + heads + axis)
    qkv = torch.randn(tiles * N * Lg, 3 * heads * e, generator=g)
    with torch.no_grad():
        ref = _axial_ref(qkv, tiles, N, Lg, heads, e, axis)[1]
    out = ops.axial_attention(qkv.to(DEV), tiles, N, Lg, heads, e, axis)
    err = relerr(out, ref)
    print(f"axial fwd T={T} other={other} e={e} heads={heads} axis={axis}: relerr {err:.2e}")
    assert torch.isfinite(out).all() and err < 3e-6


def test_axial_attention_outside_the_domain_is_refused():
    from anomalyclip_amd import _lib as L
    for N, Lg, e, axis in ((129, 4, 32, 0), (4, 129, 32, 1), (24, 10, 24, 0)):
        qkv = torch.zeros(N * Lg, 3 * 2 * e, device=DEV)
        with pytest.raises(L.AcxError, match="axis length <= 128"):
            ops.axial_attention(qkv, 1, N, Lg, 2, e, axis)


# matrix-core shapes (T <= 64 padded to 16, e in {16, 32}) and two on the general kernel (T = 96 with e = 32, T = 40 with e = 64)
BWD_CASES = [(5, 7, 16, 2, 0), (5, 7, 32, 8, 1), (24, 10, 32, 8, 0), (24, 10, 16, 1, 1), (48, 8, 16, 2, 0), (48, 8, 32, 2, 1),
             (64, 16, 32, 8, 0), (64, 5, 16, 8, 1), (96, 3, 32, 2, 0), (40, 12, 64, 2, 1)]


@pytest.mark.parametrize("T,other,e,heads,axis", BWD_CASES)
def test_axial_attention_bwd_grid(T, other, e, heads, axis):
    """ops.seq_attention_bwd against fp64 autograd, at test_axial_attention_bwd's bound"""
    N, Lg = (T, other) if axis == 0 else (other, T)
    tiles = 2
    g = torch.Generator().manual_seed(1000 * T + e + axis)
    qkv = torch.randn(tiles * N * Lg, 3 * heads * e, generator=g)
    dout = torch.randn(tiles * N * Lg, heads * e, generator=g)
    with torch.enable_grad():
        t, o = _axial_ref(qkv, tiles, N, Lg, heads, e, axis)
        o.backward(dout.double())
    dq = ops.seq_attention_bwd(qkv.to(DEV), dout.to(DEV), tiles, N, Lg, heads, e, axis)
    err = relerr(dq, t.grad)
    print(f"axial bwd T={T} other={other} e={e} heads={heads} axis={axis}: relerr {err:.2e}")
    assert torch.isfinite(dq).all() and err < 1e-5


# ====================================================================================================== model level
@pytest.mark.parametrize("tag", list(RG.GRIDS))
def test_e2e_grid_golden(golden, tag):
    """the three fixture grids (tiny CLIP geometry) against what the REFERENCE produced: test mode and the train forward + losses.
    Bounds: TOL / elem_ok of test_e2e_tiny_golden_test_mode; indices bit-exact."""
    hc, S, seed = RG.GRIDS[tag]
    g = golden("e2e_grid_" + tag)
    net, sd, eot = build_grid_net("tiny", hc, seed)
    inp = RG.grid_inputs(seed, IW.TINY.embed_dim, hc, S)
    net.eval()
    with torch.no_grad():
        sim, sc = net(inp["test_feats"].to(DEV), None, inp["nc"], S, True)
    print(f"{tag} test mode: sim {relerr(sim, g['test_sim']):.2e} scores {relerr(sc, g['test_scores']):.2e}")
    assert relerr(sim, g["test_sim"]) < TOL and relerr(sc, g["test_scores"]) < TOL
    assert elem_ok(sim, g["test_sim"]) and elem_ok(sc, g["test_scores"])
    net.train()
    mask = inp["mask"]
    net.selector_model.generate_mask = lambda b: (mask, mask)
    crit = ComputeLoss(hc.normal_id, hc.num_topk, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, hc.seg_length, hc.num_segments)
    labels = inp["labels"].to(DEV)
    with torch.no_grad():
        lg, lt, scr, ia, in_, ba = net(inp["train_feats"].to(DEV), labels, inp["nc"])
        losses = torch.stack(crit(lg, lt, labels, scr, ia, in_, ba))
    assert torch.equal(ia.cpu(), torch.from_numpy(g["idx_topk_abn"])) and torch.equal(in_.cpu(), torch.from_numpy(g["idx_topk_nor"]))
    assert torch.equal(ba.cpu(), torch.from_numpy(g["idx_bottomk_abn"]))
    for name, a in (("train_logits", lg), ("train_logits_topk", lt), ("train_scores", scr), ("losses", losses)):
        print(f"{tag} {name}: {relerr(a, g[name]):.2e}")
        assert relerr(a, g[name]) < TOL and elem_ok(a, g[name]), name
    bn = net.selector_model.bn_layer
    assert relerr(bn.running_mean, g["rm1"]) < TOL and relerr(bn.running_var, g["rv1"]) < TOL


def _full_inputs(hc, S=2):
    g = torch.Generator().manual_seed(1)
    feats = torch.randn(1, 1, hc.num_segments * hc.seg_length * S, 512, generator=g) * 0.3
    nc = torch.randn(512, generator=g) * 0.05
    return feats, nc


@functools.lru_cache(maxsize=None)
def _full_oracle_test_mode(name):
    """the oracle's test-mode result of one grid, once per module (shared by the precisions)"""
    hc = FULL[name]
    toks = _toks()
    sd = IW.init_anomalyclip_state_dict(IW.VIT_B16, hc, toks, 7)
    feats, nc = _full_inputs(hc)
    with torch.no_grad():
        return O.anomaly_clip_forward_test(sd, hc, feats, nc, toks.argmax(-1), 8, 2)


@pytest.mark.parametrize("name,precision", [(n, p) for n in FULL for p in ("auto", "f32")] + [("24x10", "bf16")])
def test_head_grid_vs_oracle(name, precision):
    """full-width heads on other grids against the oracle, test mode with S = 2: TOL / elem_ok of test_head_vs_oracle_full_configs;
    "bf16" at the bound of test_xd_long_segments_bf16_head (scores within 2e-2 absolute, similarity within 2e-2 relative)."""
    hc = FULL[name]
    net, sd, eot = build_grid_net("ViT-B/16", hc, 7, precision=precision)
    N, Lg = hc.num_segments, hc.seg_length
    assert net.temporal_model.x6_convs() == (precision == "auto" and N & (N - 1) == 0 and Lg & (Lg - 1) == 0)
    feats, nc = _full_inputs(hc)
    net.eval()
    with torch.no_grad():
        sim, sc = net(feats.to(DEV), None, nc, 2, True)
    rs, rc = _full_oracle_test_mode(name)
    print(f"{name} {precision}: sim {relerr(sim, rs):.2e} scores {relerr(sc, rc):.2e}")
    assert sim.shape == rs.shape and sc.shape == rc.shape
    if precision == "bf16":
        assert (sc.double().cpu() - rc.double()).abs().max().item() < 2e-2 and relerr(sim, rs) < 2e-2
    else:
        assert relerr(sim, rs) < TOL and relerr(sc, rc) < TOL
        assert elem_ok(sim, rs) and elem_ok(sc, rc)


# ====================================================================================================== training
def _train_batch_inputs(hc, B, seed):
    g = torch.Generator().manual_seed(seed)
    abn = [c for c in range(hc.num_classes) if c != hc.normal_id]
    labels = torch.tensor(([1, hc.num_classes - 1] + abn * 3)[:B // 2] + [hc.normal_id] * (B // 2))
    feats = torch.randn(B, 1, hc.num_segments * hc.seg_length, 512, generator=g) * 0.3
    nc = torch.randn(512, generator=g) * 0.05
    masks = [torch.bernoulli(torch.ones(B, hc.num_segments) * 0.3, generator=g) for _ in range(2)]
    for m in masks:
        m[:, :hc.num_topk] = 1
    return feats, labels, nc, masks


@pytest.mark.parametrize("name,precision", [("64x16", "auto"), ("24x10", "auto"), ("16x32", "auto"), ("16x32", "f32")])
def test_grid_train_step_vs_oracle(name, precision):
    """the method and bounds of test_full_config_train_step_vs_oracle at B = 4: indices bit-exact, losses relerr < 1e-4, every
    gradient element within 1e-3 |g64| + 1e-5 max|g64| of the fp64 oracle on the library's side of every LeakyReLU."""
    hc, B = FULL[name], 4
    net, sd, eot = build_grid_net("ViT-B/16", hc, 11, precision=precision)
    N, Lg = hc.num_segments, hc.seg_length
    assert net.temporal_model.x6_convs() == (precision == "auto" and name != "24x10")
    feats, labels, nc, masks = _train_batch_inputs(hc, B, 5)
    mask = masks[0]
    kw = dict(normal_id=hc.normal_id, num_topk=hc.num_topk, num_segments=N, frames_per_segment=Lg)
    crit = ComputeLoss(hc.normal_id, hc.num_topk, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, Lg, N)
    for p in net.image_encoder.parameters():
        p.requires_grad = False
    for p in net.text_encoder.parameters():
        p.requires_grad = False
    net.text_encoder.text_projection.requires_grad = True
    net.token_embedding.weight.requires_grad = False
    net.train()
    net.selector_model.generate_mask = lambda b: (mask, mask)
    tap = net.temporal_model.__dict__["_act_tap"] = {}
    with torch.enable_grad():
        lg, lt, sc, ia, in_, ba = net(feats.to(DEV), labels.to(DEV), nc)
        losses = crit(lg, lt, labels.to(DEV), sc, ia, in_, ba)
        losses[0].backward()
    sides = _leaky_sides(tap, net.temporal_model, B)
    del net.temporal_model.__dict__["_act_tap"]
    names = [n for n, p in net.named_parameters() if p.requires_grad and n != "selector_model.logit_scale"]
    with torch.no_grad():
        o = O.anomaly_clip_forward_train(sd, hc, feats, labels, nc, eot, 8, mask, mask)
        ol = O.compute_loss(o[0], o[1], labels, o[2], o[3], o[4], o[5], **kw)
    sd64 = {k: (v.double() if v.is_floating_point() else v) for k, v in sd.items()}
    O.LEAKY_SIDE, O.LEAKY_REPORT = sides, {}
    try:
        with torch.enable_grad():
            for n in names:
                sd64[n] = sd64[n].clone().requires_grad_(True)
            o64 = O.anomaly_clip_forward_train(sd64, hc, feats.double(), labels, nc.double(), eot, 8, mask.double(), mask.double())
            O.compute_loss(o64[0], o64[1], labels, o64[2], o[3], o[4], o[5], **kw)[0].backward()
        _check_leaky_report(2 * hc.depth)
    finally:
        O.LEAKY_SIDE = None
    assert torch.equal(ia.cpu(), o[3]) and torch.equal(in_.cpu(), o[4]) and torch.equal(ba.cpu(), o[5])
    print(f"{name} {precision}: losses relerr {relerr(torch.stack(losses), torch.stack(ol)):.2e}")
    assert relerr(torch.stack(losses), torch.stack(ol)) < 1e-4
    assert R.elem_excess(lg, o[0]) <= 1 and R.elem_excess(lt, o[1]) <= 1 and R.elem_excess(sc, o[2]) <= 1
    params = dict(net.named_parameters())
    ex = {n: R.elem_excess(params[n].grad, sd64[n].grad, rtol=1e-3, afrac=1e-5) for n in names}
    print("elem_excess(1e-3, 1e-5), worst:", sorted(((round(v, 2), n) for n, v in ex.items()), reverse=True)[:4])
    for n in names:
        assert ex[n] <= 1, (n, ex[n])


def _grid_module(hc, seed=23):
    from anomalyclip_amd.anomaly_clip_module import AnomalyCLIPModule
    net, sd, eot = build_grid_net("ViT-B/16", hc, seed)
    crit = ComputeLoss(hc.normal_id, hc.num_topk, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, hc.seg_length, hc.num_segments)
    mod = AnomalyCLIPModule(net, None, None, crit, num_classes=hc.num_classes, solver={"lr": 1e-3}).to(DEV)
    net.train()
    return mod, net


def _run_steps(mod, net, opt, hc, B, steps, seed0):
    for step in range(steps):
        feats, labels, nc, masks = _train_batch_inputs(hc, B, seed0 + step)
        f, l = feats.to(DEV), labels.to(DEV)
        if mod.ncentroid is None:
            mod.ncentroid = (torch.randn(512, generator=torch.Generator().manual_seed(3)) * 0.05).to(DEV)
        net.selector_model.generate_mask = lambda b, m=masks: (m[0], m[1])
        mod.train_batch(((f[B // 2:], l[B // 2:]), (f[:B // 2], l[:B // 2])), opt)
    torch.cuda.synchronize()


@pytest.mark.parametrize("name", ["64x16", "24x10"])
def test_grid_step_graph_bit_identical_to_autograd(name):
    """the check of test_step_graph_full_configs_bit_identical_to_autograd: train_batch's whole-step graph against the eager autograd
    path, three steps, bit-identical losses, gradients, parameters, AdamW moments and BatchNorm running statistics."""
    hc, B = FULL[name], 4
    mods = [_grid_module(hc) for _ in range(2)]
    mods[1][1].step_graph = False
    opts = [m.configure_optimizers()["optimizer"] for m, _ in mods]
    for step in range(3):
        for (mod, net), opt in zip(mods, opts):
            _run_steps(mod, net, opt, hc, B, 1, 900 + step)
        pa, pb = dict(mods[0][1].named_parameters()), dict(mods[1][1].named_parameters())
        for a_, b_ in zip(mods[0][0].last_losses, mods[1][0].last_losses):
            assert torch.equal(a_, b_), step
        for n in pa:
            if pa[n].requires_grad:
                assert (pa[n].grad is None) == (pb[n].grad is None), (step, n)
                if pb[n].grad is not None:
                    assert torch.equal(pa[n].grad, pb[n].grad), (step, n)
                    sa, sb = opts[0].state[pa[n]], opts[1].state[pb[n]]
                    assert torch.equal(sa["exp_avg"], sb["exp_avg"]) and torch.equal(sa["exp_avg_sq"], sb["exp_avg_sq"]), (step, n)
                assert torch.equal(pa[n], pb[n]), (step, n)
        bn_a, bn_b = mods[0][1].selector_model.bn_layer, mods[1][1].selector_model.bn_layer
        assert torch.equal(bn_a.running_mean, bn_b.running_mean) and torch.equal(bn_a.running_var, bn_b.running_var)
    sgs = mods[0][0].__dict__.get("_step_graphs", {})
    assert len(sgs) == 1 and all(v is not None for v in sgs.values()), getattr(mods[0][0], "step_graph_error", None)


def test_grid_step_graph_replay_is_deterministic():
    """ten steps through the whole-step graph at 24 x 10, twice from the same state: identical parameters"""
    hc, B = FULL["24x10"], 4
    finals = []
    for _ in range(2):
        mod, net = _grid_module(hc)
        opt = mod.configure_optimizers()["optimizer"]
        _run_steps(mod, net, opt, hc, B, 10, 300)
        sgs = mod.__dict__.get("_step_graphs", {})
        assert len(sgs) == 1 and all(v is not None for v in sgs.values()), getattr(mod, "step_graph_error", None)
        finals.append({n: p.detach().clone() for n, p in net.named_parameters() if p.requires_grad})
        del mod, net, opt
    for n in finals[0]:
        assert torch.equal(finals[0][n], finals[1][n]), n


# ====================================================================================================== feature files
def test_feature_file_through_a_24x10_grid(tmp_path):
    """a .npy of 700 frames -> FeatureStream(num_segments=24, seg_length=10) (S = 3 tiles of 240 rows) -> the head; the scores of
    the 700 real frames against the oracle on the same gathered rows (bounds of test_feature_stream's scores check)."""
    from anomalyclip_amd.feature_stream import FeatureStream
    from anomalyclip_amd import feature_index as FI
    hc, S_want, seed = RG.GRIDS["24x10"]
    T_ = 700
    raw = (np.random.default_rng(0).standard_normal((T_, IW.TINY.embed_dim)) * 0.3).astype(np.float32)
    path = str(tmp_path / "v.npy")
    np.save(path, raw)
    net, sd, eot = build_grid_net("tiny", hc, seed)
    net.eval()
    nc = torch.zeros(IW.TINY.embed_dim)
    ref, S_ref = FI.gather_test_features(raw, 24, 10, 1, 1)
    (feats, T, S, p), = list(FeatureStream([path], num_segments=24, seg_length=10, device=torch.device(DEV)))
    assert (T, S, S_ref) == (T_, 3, 3) and feats.shape == (1, 1, 240 * S, IW.TINY.embed_dim)
    assert np.array_equal(feats[0].cpu().numpy(), ref)
    with torch.no_grad():
        sim, sc = net(feats, None, nc, S, True)
        rs, rc = O.anomaly_clip_forward_test(sd, hc, torch.from_numpy(ref).unsqueeze(0), nc, eot, IW.TINY.transformer_heads, S)
    assert relerr(sc[:T_], rc[:T_]) < TOL and elem_ok(sc[:T_], rc[:T_])
