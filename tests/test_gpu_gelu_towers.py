"""-m gpu: the two CLIP towers with act="gelu" (nn.GELU: open_clip's LAION-2B / DataComp checkpoints) against the REFERENCE's outputs
with its QuickGELU replaced by torch.nn.GELU (tests/golden/make_golden_gelu.py): the image encoder in every f32-accurate precision
and launch size, the text tower forward and backward on both of its branches, the whole-step graph, and extract --act gelu.

Bounds: the image and text features at test_vit_b16_golden's / test_text_golden's -- 1e-4 of the output's maximum and
recipes.elem_excess -- the gradients at the project's gradient bound, 1e-3 relative + 1e-5 of the tensor's maximum per element.
The same weights under the default activation must miss the fixture by more than ten times the bound.
precision "f16x3" is stated for the ViT-B/16 geometry only (check_vit_precision refuses it for ViT-L/14): it runs there alone, and
from 8 frames (at 2 frames the driver refuses its partly-plane plan under either activation)."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import extract as X
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components import functional as Fn
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.clip_vit import VisionTransformer
from anomalyclip_amd.components.loss import ComputeLoss
from anomalyclip_amd.preprocess import preprocess_crops
import recipes as R

DEV = "cuda"
TOL = 1e-4
GEOMS = {"vit_b16_gelu": ("ViT-B/16", IW.VIT_B16), "vit_l14_gelu": ("ViT-L/14", IW.VIT_L14)}
_VITS = {}


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def ok(a, b):
    return relerr(a, b) < TOL and R.elem_excess(a, b) <= 1.0


def _vit(tag, golden, act="gelu"):
    """one encoder per (fixture, activation) for the whole module (ViT-L/14: 304 M parameters drawn on the host once)"""
    if (tag, act) not in _VITS:
        arch, geom = GEOMS[tag]
        vit = VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers,
                                geom.vision_heads, geom.embed_dim, precision="f32", arch=arch, act=act)
        vit.load_state_dict(IW.init_vit_state_dict(geom, int(golden(tag)["seed"]), prefix=""), strict=True)
        _VITS[(tag, act)] = vit.to(DEV)
    return _VITS[(tag, act)]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _VITS.clear()
    torch.cuda.empty_cache()


def _frames(tag, golden):
    g = golden(tag)
    f = R.vit_frames(int(g["seed"]), 2, GEOMS[tag][1].image_resolution)
    assert abs(float(f.double().sum()) - float(g["frames_checksum"])) < 1e-6
    return f


# ------------------------------------------------------------------------------------------------------------------ image encoder
@pytest.mark.parametrize("precision", ["f32", "f32x6", "auto", "f16x3"])
@pytest.mark.parametrize("tag", list(GEOMS))
def test_vit_gelu_golden(golden, tag, precision):
    """2 frames (the f32 routes), then tiled to 8 and 32 (the plane kernels: from 18 tiles of 256 x 256): every row against the
    reference with nn.GELU; repeated frames give bit-identical rows"""
    if precision == "f16x3" and tag != "vit_b16_gelu":
        with pytest.raises(ValueError, match="f16x3"):
            VisionTransformer(224, 14, 1024, 2, 16, 768, precision="f16x3", arch="ViT-L/14", act="gelu")
        return
    g = golden(tag)
    vit = _vit(tag, golden)
    vit.precision = precision
    try:
        base = _frames(tag, golden)
        want = torch.from_numpy(g["out"])
        if precision == "auto":
            assert vit.ln16_resolution() is not None and len(vit.ln16_resolution()) == 2 * vit.layers
            assert vit.r16_resolution() is not None and len(vit.r16_resolution()) == 4 * vit.layers       # "auto" = ACX_PREC_F32X6_R16
        if precision == "f16x3":
            # 2 frames of ViT-B/16 put the in-projection alone on the plane kernel (18 tiles): ACX_PREC_F16X3 wants all four products
            # there or none and the driver refuses, whatever the activation -- this precision starts at 8 frames
            with pytest.raises(L.AcxError, match="all four products"):
                vit(base.to(DEV))
        for n in (8, 32) if precision == "f16x3" else (2, 8, 32):
            out = vit(base.repeat(n // 2, 1, 1, 1).to(DEV))
            assert out.shape[0] == n and bool(torch.isfinite(out).all())
            assert ok(out[:2], want), (n, relerr(out[:2], want))
            ev, od = out[0::2], out[1::2]
            assert torch.equal(ev, ev[:1].expand_as(ev)) and torch.equal(od, od[:1].expand_as(od)), n
    finally:
        vit.precision = "f32"


@pytest.mark.parametrize("tag", list(GEOMS))
def test_vit_default_activation_misses_the_gelu_fixture(golden, tag):
    """the fixture tells the two activations apart: QuickGELU on the same weights is more than 10 x the bound away"""
    quick = _vit(tag, golden, act="quick_gelu")
    assert quick.act == "quick_gelu" and VisionTransformer(32, 16, 128, 1, 2, 64).act == "quick_gelu"
    e = relerr(quick(_frames(tag, golden).to(DEV)), golden(tag)["out"])
    print(tag, "QuickGELU against the nn.GELU fixture:", e)
    assert e > 10 * TOL
    del _VITS[(tag, "quick_gelu")]


def _encode_direct(vit, x, prec):
    """acx_vit_encode_ln16 / _r16 called directly with the model's weights, scales and activation"""
    scales, sc, fc16, r16 = vit._ln16_bound()
    d = L.VitDesc(vit.input_resolution, vit.patch_size, vit.width, vit.layers, vit.heads, vit.output_dim, prec, L.ACT_GELU)
    lib = L.lib()
    if prec == L.PREC_F32X6_R16:
        w, _keep = vit._weights(prec, fc16, r16[2])
        fn, sc = lib.acx_vit_encode_r16, r16[1]
    else:
        w, _keep = vit._weights(prec, fc16)
        fn = lib.acx_vit_encode_ln16
    n = x.shape[0]
    out = torch.empty(n, vit.output_dim, dtype=torch.float32, device=x.device)
    nbytes = lib.acx_vit_workspace_bytes(C.byref(d), n)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
    h = ops._h(x)
    L.check(fn(h, C.byref(d), C.byref(w), sc, x.data_ptr(), n, out.data_ptr(), ws.data_ptr(), nbytes, ops._stream()), h)
    return out


def test_vit_b16_gelu_ln16_and_r16_plans(golden):
    """8 frames of ViT-B/16: the LN16-only plan (acx_vit_encode_ln16 called directly: c_fc's fp16-plane GELU epilogue to bf16 x 3
    planes) and the R16 plan (c_fc's epilogue to fp16 planes of s_hid * hidden: what "auto" runs) against the fixture; the plan
    records say c_fc is the plane product they are about"""
    tag = "vit_b16_gelu"
    vit = _vit(tag, golden)
    x = _frames(tag, golden).repeat(4, 1, 1, 1).to(DEV)
    want = torch.from_numpy(golden(tag)["out"])
    recs = {p: ops.transformer_plan(8, 197, 768, 12, 12, prec=p, prune_last=True)[0] for p in (L.PREC_F32X6_LN16, L.PREC_F32X6_R16)}
    assert recs[L.PREC_F32X6_LN16]["fc"]["kernel"] == L.TF_GEMM_X6 and recs[L.PREC_F32X6_LN16]["ln2_dtype"] == L.F16X2P
    assert recs[L.PREC_F32X6_LN16]["fc"]["c_dtype"] == L.BF16X3P and recs[L.PREC_F32X6_R16]["fc"]["c_dtype"] == L.F16X2P
    o_ln16 = _encode_direct(vit, x, L.PREC_F32X6_LN16)
    o_r16 = _encode_direct(vit, x, L.PREC_F32X6_R16)
    assert ok(o_ln16[:2], want) and ok(o_r16[:2], want)
    vit.precision = "auto"
    try:
        assert torch.equal(vit(x), o_r16) and not torch.equal(o_r16, o_ln16)
    finally:
        vit.precision = "f32"


# ------------------------------------------------------------------------------------------------------------------ text tower
def _net(prompts_table, seed, act="gelu", arch="ViT-B/16", hc=None, **kw):
    toks = torch.tensor(prompts_table["ucf"]["tokenized_prompts"], dtype=torch.int32)
    hc = hc or IW.HeadConfig(num_classes=14, normal_id=7)
    geom = IW.TINY if arch == "tiny" else IW.VIT_B16
    net = AnomalyCLIP(arch=arch, labels_key="ucf", emb_size=hc.emb_size, depth=hc.depth, heads=hc.heads, dim_heads=None, num_segments=32,
                      seg_length=16, concat_features=False, normal_id=7, stride=1, load_from_features=True, select_idx_dropout_topk=0.7,
                      select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3, act=act, **kw)
    sd = IW.init_anomalyclip_state_dict(geom, hc, toks, seed, with_image_encoder=False)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("image_encoder.") for k in missing)
    return net.to(DEV), sd


class _FewRows:
    """ACX_OPT_SK_MAX_M of the device's context for the block, put back afterwards"""

    def __init__(self, rows):
        self.rows = rows

    def __enter__(self):
        self.dev = torch.cuda.current_device()
        self.before = ops.get_option(self.dev, L.OPT_SK_MAX_M)
        if self.rows is not None:
            ops.set_few_row_limit(self.dev, self.rows)

    def __exit__(self, *exc):
        ops.set_few_row_limit(self.dev, self.before)


@pytest.fixture(scope="module")
def text_net(golden, prompts_table):
    return _net(prompts_table, int(golden("text_gelu")["seed"]))


@pytest.mark.parametrize("branch", ["few-row", "many-row"])
def test_text_gelu_golden(golden, text_net, branch):
    """14 classes x 16 positions = 224 rows: the few-row branch (activation in c_proj's A prologue); ACX_OPT_SK_MAX_M = 0: the many-row
    branch (acx_act mode 4).  The driver (acx_transformer_forward_act: evaluation) and the training forward, both against the fixture"""
    g = golden("text_gelu")
    net, _ = text_net
    assert net.text_encoder.transformer.act == "gelu" and net.image_encoder.act == "gelu"
    with _FewRows(0 if branch == "many-row" else None):
        rows = 14 * net.text_len
        assert (rows <= ops.get_option(torch.cuda.current_device(), L.OPT_SK_MAX_M)) == (branch == "few-row")
        with torch.no_grad():
            net._text_cache = None
            tf = net.get_text_features()
            tf2 = net.text_encoder(net.prompt_learner(), net.tokenized_prompts)
        with torch.enable_grad():
            tf3 = Fn.text_features_train(net)
    assert tf.shape == (14, 512) and tf3.requires_grad
    for t in (tf, tf2, tf3.detach()):
        assert ok(t, g["out"]), relerr(t, g["out"])


def test_text_default_activation_misses_the_gelu_fixture(golden, prompts_table):
    g = golden("text_gelu")
    net, _ = _net(prompts_table, int(g["seed"]), act="quick_gelu")
    with torch.no_grad():
        e = relerr(net.get_text_features(), g["out"])
    print("text tower, QuickGELU against the nn.GELU fixture:", e)
    assert e > 10 * TOL


def _text_tower_fp64(sd, ctx, proj, eot, heads, n_ctx=8):
    """the reference's text path restated in fp64 with nn.GELU: prompts = prefix | ctx | suffix (+ positional embedding), 12 causal
    pre-LN blocks, the EOT row, ln_final, @ text_projection (coop.py:74-90, text_encoder.py:14-25, clip/model.py:188-230)"""
    p = {k: v.double() for k, v in sd.items() if torch.is_tensor(v) and v.is_floating_point()}
    x = torch.cat([p["prompt_learner.token_prefix"], ctx, p["prompt_learner.token_suffix"]], 1) + p["text_encoder.positional_embedding"]
    Cn, Ln, W = x.shape
    mask = torch.full((Ln, Ln), float("-inf"), dtype=torch.float64).triu_(1)
    ln = torch.nn.functional.layer_norm
    gelu = torch.nn.GELU()
    layers = len({k.split(".")[3] for k in sd if k.startswith("text_encoder.transformer.resblocks.")})
    for i in range(layers):
        b = f"text_encoder.transformer.resblocks.{i}."
        h = ln(x, (W,), p[b + "ln_1.weight"], p[b + "ln_1.bias"], 1e-5)
        q, k, v = (h @ p[b + "attn.in_proj_weight"].t() + p[b + "attn.in_proj_bias"]).view(Cn, Ln, 3, heads, W // heads).permute(2, 0, 3, 1, 4)
        s = (q / math.sqrt(W // heads)) @ k.transpose(-1, -2) + mask
        a = (torch.softmax(s, -1) @ v).transpose(1, 2).reshape(Cn, Ln, W)
        x = x + a @ p[b + "attn.out_proj.weight"].t() + p[b + "attn.out_proj.bias"]
        h = ln(x, (W,), p[b + "ln_2.weight"], p[b + "ln_2.bias"], 1e-5)
        h = gelu(h @ p[b + "mlp.c_fc.weight"].t() + p[b + "mlp.c_fc.bias"])
        x = x + h @ p[b + "mlp.c_proj.weight"].t() + p[b + "mlp.c_proj.bias"]
    e = x[torch.arange(Cn), eot]
    return ln(e, (W,), p["text_encoder.ln_final.weight"], p["text_encoder.ln_final.bias"], 1e-5) @ proj


@pytest.fixture(scope="module")
def text_grads_fp64(golden, text_net, prompts_table):
    """computed once: (d_features, d ctx, d text_projection) of the fp64 restatement"""
    _, sd = text_net
    toks = torch.tensor(prompts_table["ucf"]["tokenized_prompts"], dtype=torch.int32)
    ctx = sd["prompt_learner.ctx"].double().requires_grad_(True)
    proj = sd["text_encoder.text_projection"].double().requires_grad_(True)
    d_tf = torch.randn(14, 512, generator=torch.Generator().manual_seed(77))
    with torch.enable_grad():
        tf = _text_tower_fp64(sd, ctx, proj, toks.argmax(-1).long(), 8)
        assert relerr(tf.detach(), golden("text_gelu")["out"]) < 1e-5      # the restatement IS the reference's tower
        tf.backward(d_tf.double())
    return d_tf, ctx.grad, proj.grad


@pytest.mark.parametrize("branch", ["few-row", "many-row"])
def test_text_gelu_backward_against_fp64(text_net, text_grads_fp64, branch):
    net, _ = text_net
    d_tf, g_ctx, g_proj = text_grads_fp64
    with _FewRows(0 if branch == "many-row" else None), torch.enable_grad():
        net.zero_grad(set_to_none=True)
        tf = Fn.text_features_train(net)
        tf.backward(d_tf.to(DEV))
        torch.cuda.synchronize()
    for name, got, want in (("ctx", net.prompt_learner.ctx.grad, g_ctx), ("text_projection", net.text_encoder.text_projection.grad, g_proj)):
        err = (got.double().cpu() - want).abs()
        bound = 1e-3 * want.abs() + 1e-5 * want.abs().max()
        print(f"text backward {branch} d {name}: max err / bound = {float((err / bound).max()):.3f}")
        assert bool((err <= bound).all()), (branch, name)


# ------------------------------------------------------------------------------------------------------------------ the step graph
def test_step_graph_gelu_bit_identical_to_autograd(prompts_table):
    """the smallest head of tests/test_gpu_train.py (tiny geometry, emb 64, 2 heads, depth 1) with act="gelu": two steps through the
    whole-step graph leave the losses, gradients and parameters of the autograd path, bit for bit"""
    from anomalyclip_amd.anomaly_clip_module import AnomalyCLIPModule
    hc = IW.HeadConfig(num_classes=14, normal_id=7, emb_size=64, heads=2, depth=1)
    toks = torch.tensor(prompts_table["ucf"]["tokenized_prompts"], dtype=torch.int32)
    mods = []
    for _ in range(2):
        net = AnomalyCLIP(arch="tiny", labels_key="ucf", emb_size=64, depth=1, heads=2, dim_heads=None, num_segments=32, seg_length=16,
                          concat_features=False, normal_id=7, stride=1, load_from_features=True, select_idx_dropout_topk=0.7,
                          select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3, n_ctx=8, shared_context=False, ctx_init="",
                          act="gelu")
        missing, unexpected = net.load_state_dict(IW.init_anomalyclip_state_dict(IW.TINY, hc, toks, 21), strict=False)
        assert not missing and not unexpected
        net = net.to(DEV)
        crit = ComputeLoss(7, 3, 1.0, 1.0, 1.0, 1.0, 1.0, 8e-4, 8e-3, 16, 32)
        mod = AnomalyCLIPModule(net, None, None, crit, num_classes=14, solver={"lr": 1e-3}).to(DEV)
        net.train()
        mods.append((mod, net))
    mods[1][1].step_graph = False
    opts = [m.configure_optimizers()["optimizer"] for m, _ in mods]
    B, D = 4, IW.TINY.embed_dim
    for step in range(2):
        g = torch.Generator().manual_seed(500 + step)
        feats = torch.randn(B, 1, 512, D, generator=g) * 0.3
        labels = torch.tensor([1, 2, 7, 7])
        masks = [torch.bernoulli(torch.ones(B, 32) * 0.3, generator=g) for _ in range(2)]
        for m in masks:
            m[:, :3] = 1
        f, l = feats.to(DEV), labels.to(DEV)
        batch = ((f[B // 2:], l[B // 2:]), (f[:B // 2], l[:B // 2]))
        for (mod, net), opt in zip(mods, opts):
            if mod.ncentroid is None:
                mod.ncentroid = torch.zeros(D, device=DEV)
            net.selector_model.generate_mask = lambda b, m=masks: (m[0], m[1])
            mod.train_batch(batch, opt)
        torch.cuda.synchronize()
        pa, pb = dict(mods[0][1].named_parameters()), dict(mods[1][1].named_parameters())
        for a_, b_ in zip(mods[0][0].last_losses, mods[1][0].last_losses):
            assert torch.equal(a_, b_), step
        for n in pa:
            if pa[n].requires_grad:
                assert (pa[n].grad is None) == (pb[n].grad is None), (step, n)
                if pb[n].grad is not None:
                    assert torch.equal(pa[n].grad, pb[n].grad), (step, n)
                assert torch.equal(pa[n], pb[n]), (step, n)
    sgs = mods[0][0].__dict__.get("_step_graphs", {})
    assert len(sgs) == 1 and all(v is not None for v in sgs.values()), getattr(mods[0][0], "step_graph_error", None)
    # ... and the activation is on the path: the same two steps under QuickGELU end somewhere else
    assert mods[0][1].text_encoder.transformer.act == "gelu"


# ------------------------------------------------------------------------------------------------------------------ extract
def test_extract_act_gelu_end_to_end(tmp_path):
    """extract --act gelu on a 3-frame folder with tiny weights: the file is the encoder's direct output, bit for bit, and not the
    default activation's; contradictions exit with status 2"""
    sd = IW.init_vit_state_dict(IW.TINY, 13, prefix="")
    weights = str(tmp_path / "w.pt")
    torch.save({"image_encoder." + k: v for k, v in sd.items()}, weights)
    root, out = tmp_path / "frames", tmp_path / "feats"
    folder = root / "v"
    os.makedirs(folder)
    rng = np.random.default_rng(3)
    for t in range(3):
        Image.fromarray(rng.integers(0, 256, (48, 64, 3), dtype=np.uint8)).save(str(folder / f"{t:06d}.jpg"), quality=90)
    dec = np.stack([np.asarray(Image.open(str(folder / f"{t:06d}.jpg")).convert("RGB")) for t in range(3)])
    args = ["--arch", "tiny", "--weights", weights, "--frames-root", str(root), "--precision", "f32"]
    res = {}
    for act in ("gelu", "quick_gelu"):
        assert X.main(args + ["--out-root", str(out / act)] + (["--act", act] if act == "gelu" else [])) == 0
        res[act] = np.load(str(out / act / "v.npy"))
        enc = X.build_image_encoder("tiny", "f32", act=act)
        enc.load_state_dict(sd, strict=True)
        enc = enc.to(DEV).eval()
        with torch.no_grad():
            direct = enc(preprocess_crops(torch.from_numpy(dec).to(DEV), 32, None, 1).view(-1, 3, 32, 32)).cpu().numpy()
        assert res[act].shape == (3, 128) and np.array_equal(res[act], direct), act
    assert not np.array_equal(res["gelu"], res["quick_gelu"])
    for bad in (["--act", "gelu", "--precision", "bf16"], ["--act", "gelu", "--arch", "RN50"]):
        with pytest.raises(SystemExit) as e:
            X.parse_args(args + ["--out-root", str(out)] + bad)
        assert e.value.code == 2
