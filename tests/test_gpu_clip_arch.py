"""-m gpu: the other CLIP ViT backbones of `net.arch` -- ViT-B/32 (50 tokens), ViT-L/14 (257) and ViT-L/14@336px (577) -- from the
kernels up: the streaming attention beyond 256 keys (query blocks), the CLS-row attention beyond 256 keys, the patch im2col at
P = 14, the encoders against the REFERENCE's outputs (tests/golden/make_golden_arch.py), launch sizes past 2^32-byte buffers, and
the 768-wide head (text tower, test / train forward, the whole-step graph) at the ViT-L/14 geometry."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.clip_vit import VisionTransformer
from anomalyclip_amd.components.loss import ComputeLoss
from oracle import anomalyclip_oracle as O
import recipes as R

DEV = "cuda"
TOL = 1e-4                                   # the bounds of test_gpu_model.test_vit_b16_golden
GEOMS = {"vit_b32": ("ViT-B/32", IW.VIT_B32), "vit_l14": ("ViT-L/14", IW.VIT_L14), "vit_l14_336": ("ViT-L/14@336px", IW.VIT_L14_336)}
E2E_HEAD = IW.HeadConfig(num_classes=14, normal_id=7, emb_size=256, heads=8, depth=1)      # make_golden_arch.E2E_HEAD


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def elem_ok(a, b):
    return R.elem_excess(a, b) <= 1.0


def _attn_ref(qkv, batch, L_, heads, causal=False):
    q, k, v = qkv.view(batch, L_, 3, heads, 64).permute(2, 0, 3, 1, 4).double()
    s = (q * 0.125) @ k.transpose(-1, -2)
    if causal:
        s = s + torch.full((L_, L_), float("-inf"), dtype=torch.float64).triu_(1)
    return (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(batch * L_, heads * 64)


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("L_,heads,batch", [(225, 3, 2), (256, 2, 3), (257, 3, 2), (289, 2, 2), (577, 2, 2), (1024, 1, 2),
                                            (257, 16, 5), (577, 16, 3)])
def test_attention_long_sequences_vs_fp64(L_, heads, batch):
    """acx_attention non-causal beyond 224 keys: 225 / 256 one query block per (sequence, head), 257 (9 + 8 tiles), 289 (10 + 9),
    577 (13 + 12 + 12), 1024 (4 x 16): against fp64 at the 3e-6 level of the short-sequence tests."""
    g = torch.Generator().manual_seed(L_ + heads)
    qkv = torch.randn(batch * L_, 3 * heads * 64, generator=g)
    out = ops.attention(qkv.to(DEV), batch, L_, heads, False)
    assert relerr(out, _attn_ref(qkv, batch, L_, heads)) < 3e-6


@pytest.mark.parametrize("L_", [257, 577])
def test_attention_long_many_items_per_workgroup(L_):
    """More (query block, sequence, head) items than the 2 x CUs persistent workgroups (32 sequences x 16 heads: 1024 items at 257,
    1536 at 577): every workgroup walks several items, switches from the larger blocks' tile deal to the smaller ones' once,
    and prefetches the next item's first K / V chunk across that switch -- against fp64 on every row."""
    heads, batch = 16, 32
    g = torch.Generator().manual_seed(7 * L_)
    qkv = torch.randn(batch * L_, 3 * heads * 64, generator=g)
    out = ops.attention(qkv.to(DEV), batch, L_, heads, False)
    ref = torch.cat([_attn_ref(qkv[b0 * L_:(b0 + 8) * L_], 8, L_, heads) for b0 in range(0, batch, 8)])
    assert relerr(out, ref) < 3e-6
    # row-wise as well: a wrong query block of one item would hide in a norm-wise bound over 32 x 16 heads
    e = ((out.cpu().double() - ref).abs().amax(1) / ref.abs().amax(1)).max().item()
    assert e < 3e-5, e


def test_attention_long_spiked_score_in_a_late_block():
    """one key dominating a query of the LAST query block, the key in the last chunk: the running max jumps at the end."""
    L_, heads = 577, 1
    g = torch.Generator().manual_seed(1)
    qkv = torch.randn(L_, 192, generator=g)
    qkv[560, :64] *= 30.0
    qkv[570, 64:128] = qkv[560, :64] / 30.0 * 3
    out = ops.attention(qkv.to(DEV), 1, L_, heads, False)
    assert relerr(out, _attn_ref(qkv, 1, L_, heads)) < 3e-6


@pytest.mark.parametrize("L_,heads,batch", [(257, 4, 3), (577, 2, 2), (1024, 1, 2)])
def test_attention_x3_panel_recombines_to_f32(L_, heads, batch):
    """acx_attention_x3_panel (the out-projection's three bf16 planes in K-panel layout, written by every query block): hi + mid + lo
    is the f32 output of acx_attention (same kernel, same arithmetic) to the split's round-off."""
    g = torch.Generator().manual_seed(L_)
    W = heads * 64
    qkv = torch.randn(batch * L_, 3 * W, generator=g).to(DEV)
    ref = ops.attention(qkv, batch, L_, heads, False)
    planes = torch.zeros(3, batch * L_, W, dtype=torch.bfloat16, device=DEV)
    h = ops._h(qkv)
    L.check(L.lib().acx_attention_x3_panel(h, qkv.data_ptr(), 3 * W, planes.data_ptr(), W, batch, L_, heads, ops._stream()), h)
    p = ops.unpanel(planes).double()
    rec = p[0] + p[1] + p[2]
    assert relerr(rec, ref) < 1e-7
    assert (rec - ref.double()).abs().max().item() <= 2 ** -20 * ref.abs().max().item()


@pytest.mark.parametrize("L_,heads,batch", [(197, 12, 3), (257, 16, 3), (577, 16, 2), (1024, 2, 2)])
def test_attention_cls_equals_row0(L_, heads, batch):
    """acx_attention_cls (the pruned last ViT layer) beyond 256 keys: blocks of 256 keys with a running max and sum; equals row 0
    of the full attention and fp64."""
    g = torch.Generator().manual_seed(L_ * 3)
    W = heads * 64
    qkv = torch.randn(batch * L_, 3 * W, generator=g)
    qd = qkv.to(DEV)
    out = torch.empty(batch, W, device=DEV)
    h = ops._h(qd)
    L.check(L.lib().acx_attention_cls(h, qd.data_ptr(), 3 * W, out.data_ptr(), W, batch, L_, heads, ops._stream()), h)
    ref = _attn_ref(qkv, batch, L_, heads).view(batch, L_, W)[:, 0]
    assert relerr(out, ref) < 3e-6
    full = ops.attention(qd, batch, L_, heads, False).view(batch, L_, W)[:, 0]
    assert relerr(out, full) < 3e-6


def test_attention_limits_are_unsupported():
    h = L.ctx(torch.cuda.current_device())
    lib = L.lib()
    for L_, causal in ((1025, 0), (225, 1)):
        qkv = torch.zeros(L_, 192, device=DEV)
        out = torch.empty(L_, 64, device=DEV)
        rc = lib.acx_attention(h, qkv.data_ptr(), 192, out.data_ptr(), 64, 1, L_, 1, causal, ops._stream())
        assert rc == -2, (L_, causal, rc)                                  # ACX_E_UNSUPPORTED
    qkv = torch.zeros(1025, 192, device=DEV)
    out = torch.empty(1, 64, device=DEV)
    assert lib.acx_attention_cls(h, qkv.data_ptr(), 192, out.data_ptr(), 64, 1, 1025, 1, ops._stream()) == -2
    torch.cuda.synchronize()


def _unfold_ref(frames, P):
    Fn, _, R_, _ = frames.shape
    g = R_ // P
    return frames.reshape(Fn, 3, g, P, g, P).permute(0, 2, 4, 1, 3, 5).reshape(Fn * g * g, 3 * P * P)


@pytest.mark.parametrize("R_,P", [(224, 14), (336, 14), (224, 16), (224, 32)])
def test_vit_patches_even_patch_bit_exact(R_, P):
    """acx_vit_patches at P = 14 (two float2 loads per four k: a run of four may cross a patch row) and the P % 4 == 0 sizes:
    bit-exact against torch's unfold, f32 and bf16; the K-panel plane outputs need 3 P P % 32 == 0 and refuse P = 14."""
    g = torch.Generator().manual_seed(R_ + P)
    frames = torch.randn(3, 3, R_, R_, generator=g)
    fd = frames.to(DEV)
    ref = _unfold_ref(frames, P)
    K = 3 * P * P
    h = ops._h(fd)
    lib = L.lib()
    out = torch.empty(ref.shape[0], K, device=DEV)
    L.check(lib.acx_vit_patches(h, fd.data_ptr(), out.data_ptr(), L.ACX_F32, 3, R_, P, ops._stream()), h)
    assert torch.equal(out.cpu(), ref)
    ob = torch.empty(ref.shape[0], K, dtype=torch.bfloat16, device=DEV)
    L.check(lib.acx_vit_patches(h, fd.data_ptr(), ob.data_ptr(), L.ACX_BF16, 3, R_, P, ops._stream()), h)
    assert torch.equal(ob.cpu(), ref.to(torch.bfloat16))
    if K % 32:
        for dt in (L.BF16X3P, L.BF16X2P, L.F16X2P):
            pl = torch.empty(3, ref.shape[0], K, dtype=torch.bfloat16, device=DEV)
            assert lib.acx_vit_patches(h, fd.data_ptr(), pl.data_ptr(), dt, 3, R_, P, ops._stream()) == -1     # ACX_E_BADARG
    else:
        pl = torch.empty(3, ref.shape[0], K, dtype=torch.bfloat16, device=DEV)
        L.check(lib.acx_vit_patches(h, fd.data_ptr(), pl.data_ptr(), L.BF16X3P, 3, R_, P, ops._stream()), h)
        p = ops.unpanel(pl).double()
        assert torch.equal((p[0] + p[1] + p[2]).float().cpu(), ref)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------------------------ encoders
_VITS = {}


def _vit(tag, golden):
    """one encoder per fixture for the whole module (ViT-L/14: 304 M parameters drawn on the host once)"""
    if tag not in _VITS:
        g = golden(tag)
        arch, geom = GEOMS[tag]
        vit = VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers,
                                geom.vision_heads, geom.embed_dim, precision="f32", arch=arch)
        vit.load_state_dict(IW.init_vit_state_dict(geom, int(g["seed"]), prefix=""), strict=True)
        _VITS[tag] = vit.to(DEV)
    return _VITS[tag]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _VITS.clear()
    torch.cuda.empty_cache()


def _frames(tag, golden, n=2):
    g = golden(tag)
    f = R.vit_frames(int(g["seed"]), n, GEOMS[tag][1].image_resolution)
    assert abs(float(f[:2].double().sum()) - float(g["frames_checksum"])) < 1e-6
    return f


@pytest.mark.parametrize("precision", ["f32", "auto", "bf16"])
@pytest.mark.parametrize("tag", list(GEOMS))
def test_vit_arch_golden(golden, tag, precision):
    """The encoder against the reference's output for 2 frames: f32 and auto at the bounds of test_vit_b16_golden, bf16 at the bound
    of test_vit_b16_bf16_mode (bf16 runs the f32 attention above 224 tokens and the f32 patch embedding at P = 14)."""
    g = golden(tag)
    vit = _vit(tag, golden)
    vit.precision = precision
    vit.chunk = 512
    out = vit(_frames(tag, golden).to(DEV))
    if precision == "bf16":
        e = relerr(out, g["out"])
        print(tag, "bf16 rel err vs reference:", e)
        assert e < 5e-2
    else:
        assert relerr(out, g["out"]) < TOL and elem_ok(out, g["out"])


@pytest.mark.parametrize("precision", ["f32", "auto"])
@pytest.mark.parametrize("tag,nframes", [("vit_l14", 512), ("vit_l14_336", 512), ("vit_b32", 512)])
def test_vit_arch_full_launch_properties(golden, tag, precision, nframes):
    """512 frames in ONE launch (ViT-L/14@336px: 295 424 token rows; the f32 c_fc output is 4.8 GB and each of its bf16 planes
    2.4 GB -- past 2^32 bytes): identical frames give bit-identical rows wherever they sit -- the last frames included, whose rows
    the GEMMs' tail launch computes (512 rows at K = 1024 / 4096 for ViT-L) -- and the rows agree with the golden-pinned 2-frame
    launch (other kernels) to round-off and with the reference."""
    g = golden(tag)
    vit = _vit(tag, golden)
    vit.precision = precision
    vit.chunk = nframes
    R_ = GEOMS[tag][1].image_resolution
    base = _frames(tag, golden)
    extra = torch.randn(6, 3, R_, R_, generator=torch.Generator().manual_seed(5))
    eight = torch.cat([base, extra], 0)
    idx = torch.arange(nframes) % 8
    idx[-12:] = torch.tensor([7, 3, 0, 1, 5, 5, 2, 6, 4, 0, 1, 7])
    x = eight[idx].to(DEV)
    out = vit(x)
    del x
    assert out.shape == (nframes, GEOMS[tag][1].embed_dim) and torch.isfinite(out).all()
    for k in range(8):
        rows = out[idx.to(DEV) == k]
        assert torch.equal(rows, rows[:1].expand_as(rows)), k               # bit-identical across ALL slots
    small = vit(base.to(DEV))
    assert relerr(out[:2], small) < 2e-6
    assert relerr(out[:2], g["out"]) < TOL and elem_ok(out[:2], g["out"])
    vit.chunk = 512
    torch.cuda.empty_cache()


@pytest.mark.parametrize("nframes", [1, 8, 64])
def test_vit_l14_small_launches_auto_vs_f32(golden, nframes):
    """auto at 1 / 8 / 64 frames: the x6 products take the launches with enough 256 x 256 tiles, the rest run the f32 kernels --
    either way round-off away from the f32 MFMA path, and the golden frames meet the reference bound."""
    g = golden("vit_l14")
    vit = _vit("vit_l14", golden)
    base = _frames("vit_l14", golden)
    more = torch.randn(max(nframes - 2, 0), 3, 224, 224, generator=torch.Generator().manual_seed(nframes))
    x = torch.cat([base, more], 0)[:nframes].to(DEV)
    vit.precision = "f32"
    o32 = vit(x)
    vit.precision = "auto"
    o6 = vit(x)
    assert torch.isfinite(o6).all() and relerr(o6, o32) < 5e-6 and elem_ok(o6, o32)
    assert relerr(o6[:min(nframes, 2)], g["out"][:min(nframes, 2)]) < TOL


# ------------------------------------------------------------------------------------------------------------------ head
def _net(prompts_table, seed, arch="ViT-L/14", with_image_encoder=True, **kw):
    geom = dict((a, g_) for a, g_ in GEOMS.values())[arch]
    toks = torch.tensor(prompts_table["ucf"]["tokenized_prompts"], dtype=torch.int32)
    hc = E2E_HEAD
    net = AnomalyCLIP(arch=arch, labels_key="ucf", emb_size=hc.emb_size, depth=hc.depth, heads=hc.heads, dim_heads=None,
                      num_segments=32, seg_length=16, concat_features=False, normal_id=7, stride=1, load_from_features=True,
                      select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3,
                      n_ctx=8, shared_context=False, ctx_init="", **kw)
    sd = IW.init_anomalyclip_state_dict(geom, hc, toks, seed, with_image_encoder=with_image_encoder)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("image_encoder.") for k in missing) and (missing == [] or not with_image_encoder)
    return net.to(DEV), sd, toks.argmax(-1)


def test_text_tower_l14_golden(golden, prompts_table):
    g = golden("text_l14")
    net, _, _ = _net(prompts_table, int(g["seed"]), with_image_encoder=False)
    with torch.no_grad():
        tf = net.get_text_features()
    assert tf.shape == (14, 768)
    assert relerr(tf, g["out"]) < TOL and elem_ok(tf, g["out"])
    with torch.no_grad():
        tf2 = net.text_encoder(net.prompt_learner(), net.tokenized_prompts)
    assert relerr(tf2, g["out"]) < TOL and elem_ok(tf2, g["out"])


def test_e2e_l14_golden_test_and_train_forward(golden, prompts_table):
    """AnomalyCLIP(arch = "ViT-L/14") from 768-wide features against the reference's AnomalyCLIP: test mode (S = 2) and the train
    forward (B = 4, fixed selection masks): logits, scores, MIL indices (exact), BatchNorm running statistics."""
    g = golden("e2e_l14")
    seed = int(g["seed"])
    net, sd, _ = _net(prompts_table, seed, with_image_encoder=False)
    inp = R.e2e_inputs(seed, 768)
    net.eval()
    with torch.no_grad():
        sim, sc = net(inp["test_feats"].to(DEV), torch.zeros(1000), inp["nc"], 2, True)
    assert relerr(sim, g["test_sim"]) < TOL and relerr(sc, g["test_scores"]) < TOL
    assert elem_ok(sim, g["test_sim"]) and elem_ok(sc, g["test_scores"])
    net.train()
    net.selector_model.generate_mask = lambda b: (inp["mask"], inp["mask"])
    with torch.enable_grad():
        lg, lt, sc, ia, in_, ba = net(inp["train_feats"].to(DEV), inp["labels"].to(DEV), inp["nc"])
    assert torch.equal(ia.cpu(), torch.from_numpy(g["idx_topk_abn"])) and torch.equal(in_.cpu(), torch.from_numpy(g["idx_topk_nor"]))
    assert torch.equal(ba.cpu(), torch.from_numpy(g["idx_bottomk_abn"]))
    for a, k in ((lg, "train_logits"), (lt, "train_logits_topk"), (sc, "train_scores")):
        assert relerr(a, g[k]) < TOL and R.elem_excess(a, g[k]) <= 1, k
    bn = net.selector_model.bn_layer
    assert relerr(bn.running_mean, g["rm1"]) < TOL and relerr(bn.running_var, g["rv1"]) < TOL


def test_step_graph_d768_bit_identical_to_autograd(prompts_table):
    """One train_batch at D = 768 (ViT-L/14 head: 768-wide selector, temporal projection 768 -> 256, text tower width 768 with 12
    heads): the whole-step graph path is bit-identical to the eager autograd path -- losses, gradients, parameters."""
    from anomalyclip_amd.anomaly_clip_module import AnomalyCLIPModule
    D, B = 768, 8
    mods = []
    for _ in range(2):
        net, _, _ = _net(prompts_table, 23, with_image_encoder=False)
        crit = ComputeLoss(7, 3, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, 16, 32)
        mod = AnomalyCLIPModule(net, None, None, crit, num_classes=14, solver={"lr": 1e-3}).to(DEV)
        net.train()
        mods.append((mod, net))
    mods[1][1].step_graph = False
    opts = [m.configure_optimizers()["optimizer"] for m, _ in mods]
    gen = torch.Generator().manual_seed(900)
    for step in range(2):
        feats = torch.randn(B, 1, 512, D, generator=gen) * 0.3
        labels = torch.tensor([1, 2, 3, 4] + [7] * 4)
        masks = [torch.bernoulli(torch.ones(B, 32) * 0.3, generator=gen) for _ in range(2)]
        for mk in masks:
            mk[:, :3] = 1
        f, l = feats.to(DEV), labels.to(DEV)
        batch = ((f[B // 2:], l[B // 2:]), (f[:B // 2], l[:B // 2]))
        for (mod, net), opt in zip(mods, opts):
            if mod.ncentroid is None:
                mod.ncentroid = (torch.randn(D, generator=torch.Generator().manual_seed(3)) * 0.05).to(DEV)
            net.selector_model.generate_mask = lambda b, m=masks: (m[0], m[1])
            mod.train_batch(batch, opt)
        torch.cuda.synchronize()
        pa, pb = dict(mods[0][1].named_parameters()), dict(mods[1][1].named_parameters())
        for a_, b_ in zip(mods[0][0].last_losses, mods[1][0].last_losses):
            assert torch.isfinite(a_).all() and torch.equal(a_, b_), step
        for n in pa:
            if pa[n].requires_grad:
                assert (pa[n].grad is None) == (pb[n].grad is None), (step, n)
                if pb[n].grad is not None:
                    assert torch.equal(pa[n].grad, pb[n].grad), (step, n)
                assert torch.equal(pa[n], pb[n]), (step, n)
    sgs = mods[0][0].__dict__.get("_step_graphs", {})
    assert len(sgs) == 1 and all(v is not None for v in sgs.values()), getattr(mods[0][0], "step_graph_error", None)


def test_frames_path_l14_vs_oracle_chain(golden, prompts_table):
    """test mode from FRAMES with the ViT-L/14 encoder (one 512-frame tile, S = 1) against the oracle chain: oracle.vit_forward
    (torch f32 on the device) -> oracle head on the host."""
    seed = 71
    net, sd, eot = _net(prompts_table, seed)
    net.load_from_features = False
    g = torch.Generator().manual_seed(4)
    frames = torch.randn(1, 512, 3, 224, 224, generator=g)
    nc = torch.randn(768, generator=g) * 0.1
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):       # (the oracle's conv2d: torch's own kernels)
        sim, sc = net(frames.to(DEV), None, nc, 1, True)
        sdg = {k: v.to(DEV) for k, v in sd.items() if k.startswith("image_encoder.")}
        feats = torch.cat([O.vit_forward(sdg, frames[0, i:i + 64].to(DEV)) for i in range(0, 512, 64)]).cpu()
        rs, rc = O.anomaly_clip_forward_test(sd, E2E_HEAD, feats.view(1, 1, 512, 768), nc, eot, 12, 1)
    assert relerr(sim, rs) < TOL and relerr(sc, rc) < TOL
    assert elem_ok(sim, rs) and elem_ok(sc, rc)


@pytest.mark.parametrize("hw", [(240, 320), (480, 360), (720, 1280)])
def test_frame_preprocessing_336_matches_pil(hw):
    """`data.input_size: 336` (ViT-L/14@336px): the 8-bit resample stages bit-exact with Pillow as at 224."""
    from anomalyclip_amd.preprocess import preprocess_frames, CLIP_MEAN, CLIP_STD
    g = torch.Generator().manual_seed(hw[1])
    frames = torch.randint(0, 256, (3, hw[0], hw[1], 3), generator=g, dtype=torch.uint8)
    frames[0, : hw[0] // 2] = 255
    frames[1, :, : hw[1] // 3] = 0
    ref = O.preprocess_frames_ref(frames.numpy(), size=336)
    out = preprocess_frames(frames.to(DEV), size=336)
    assert out.shape == (3, 3, 336, 336)
    assert (out.cpu() - ref).abs().max().item() < 2e-6
    m, s = torch.tensor(CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(CLIP_STD).view(1, 3, 1, 1)
    assert torch.equal(((out.cpu() * s + m) * 255).round(), ((ref * s + m) * 255).round())
