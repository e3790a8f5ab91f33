"""-m gpu: the CLIP ResNet backbones of `net.arch` -- RN50, RN101, RN50x4, RN50x16, RN50x64 -- from the kernels up: the stem
im2col, the NHWC 2x2 average pool, the ReLU and residual-then-ReLU GEMM epilogues, the implicit 3x3 convolution on the ResNets'
non-power-of-two grids and padded channel counts, the attention pool's tokens and single-query attention, the five encoders
against the REFERENCE's outputs (tests/golden/make_golden_resnet.py), 512-frame launches, the 1024-wide text tower and the
frames path of AnomalyCLIP; training-mode BatchNorm (wide batch statistics, running statistics) against the reference; the
640-wide head of RN50x4 (test / train forward, the whole-step graph) and frame preprocessing at 288 / 384 / 448."""
import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.clip_resnet import ModifiedResNet
from anomalyclip_amd.components.loss import ComputeLoss
from oracle import anomalyclip_oracle as O
import recipes as R

DEV = "cuda"
TOL = 1e-4                                   # the bounds of the ViT goldens (test_gpu_clip_arch.test_vit_arch_golden)
GEOMS = {"rn50": ("RN50", IW.RN50), "rn101": ("RN101", IW.RN101), "rn50x4": ("RN50x4", IW.RN50X4),
         "rn50x16": ("RN50x16", IW.RN50X16), "rn50x64": ("RN50x64", IW.RN50X64)}
E2E_HEAD = IW.HeadConfig(num_classes=14, normal_id=7, emb_size=256, heads=8, depth=1)


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def elem_ok(a, b):
    return R.elem_excess(a, b) <= 1.0


# ------------------------------------------------------------------------------------------------------------------ kernels
@pytest.mark.parametrize("R_", [224, 288])
def test_stem_im2col_bit_exact_vs_unfold(R_):
    x = torch.randn(2, 3, R_, R_, generator=torch.Generator().manual_seed(R_))
    cols = ops.resnet_stem_im2col(x.to(DEV)).cpu()
    ref = Fnn.unfold(x, 3, padding=1, stride=2)                       # [2, 27, G*G], rows (c, ky, kx)
    ref = ref.transpose(1, 2).reshape(-1, 27)
    assert cols.shape == (2 * (R_ // 2) ** 2, 32)
    assert torch.equal(cols[:, :27], ref) and not cols[:, 27:].any()


@pytest.mark.parametrize("F_,H,C", [(2, 112, 64), (3, 18, 96), (2, 14, 2048)])
def test_avgpool2_nhwc(F_, H, C):
    x = torch.randn(F_, H, H, C, generator=torch.Generator().manual_seed(H))
    out = ops.avgpool2_nhwc(x.to(DEV)).cpu()
    ref = Fnn.avg_pool2d(x.permute(0, 3, 1, 2).double(), 2).permute(0, 2, 3, 1)
    assert (out.double() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


def _conv_ref(x, w, b, relu=True):
    """x [F, H, W, cin] NHWC, w [N, cin, 3, 3]: relu(conv2d(x, w, pad 1) + b) in fp64, NHWC rows"""
    y = Fnn.conv2d(x.permute(0, 3, 1, 2).double(), w.double(), b.double(), padding=1).permute(0, 2, 3, 1)
    return (y.clamp_min(0) if relu else y).reshape(-1, w.shape[0])


@pytest.mark.parametrize("F_,H,cin,cin_p,N", [(3, 7, 64, 64, 512), (2, 9, 640, 640, 640), (1, 56, 64, 64, 64),
                                               (1, 144, 40, 64, 40), (2, 96, 48, 64, 48), (1, 72, 80, 96, 80)])
def test_conv3x3_relu_grids_and_padded_channels(F_, H, cin, cin_p, N):
    """ACX_AMAP_CONV3X3 + ACX_ACT_RELU on the ResNets' grids (7, 9, 56, 144 ...) and the zero-padded channel counts of RN50x4
    (40 -> 64, 80 -> 96) and RN50x16 (48 -> 64): the layout acx_resnet_encode runs, against fp64."""
    g = torch.Generator().manual_seed(H * cin)
    x = torch.randn(F_, H, H, cin, generator=g)
    w = torch.randn(N, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    b = torch.randn(N, generator=g) * 0.1
    xp = torch.zeros(F_, H, H, cin_p)
    xp[..., :cin] = x
    Np = (N + 31) // 32 * 32
    wp = torch.zeros(Np, 9, cin_p)
    wp[:N, :, :cin] = w.permute(0, 2, 3, 1).reshape(N, 9, cin)
    bp = torch.zeros(Np)
    bp[:N] = b
    out = ops.gemm(xp.reshape(-1, cin_p).to(DEV), wp.reshape(Np, 9 * cin_p).to(DEV), bias=bp.to(DEV), act=L.ACT_RELU,
                   amap=L.AMAP_CONV3X3, gn=H, gl=H, cin=cin_p).cpu()
    ref = _conv_ref(x, w, b)
    assert relerr(out[:, :N], ref) < 3e-6 and not out[:, N:].any()


@pytest.mark.parametrize("M,N,K", [(49, 2048, 512), (800, 256, 64), (6272, 1024, 256), (50176, 512, 1024)])
def test_relu_and_residual_relu_epilogues(M, N, K):
    """ACX_ACT_RELU (max(acc + b, 0)) and ACX_ACT_RESRELU (max(residual + acc + b, 0), Bottleneck's add-then-ReLU) over the row
    counts that reach the 64x64, 8-wave and strip-stream kernels, against fp64."""
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.2
    r = torch.randn(M, N, generator=g)
    lin = a.double() @ w.double().T + b.double()
    o1 = ops.gemm(a.to(DEV), w.to(DEV), bias=b.to(DEV), act=L.ACT_RELU).cpu()
    assert relerr(o1, lin.clamp_min(0)) < 3e-6 and (o1 >= 0).all()
    o2 = ops.gemm(a.to(DEV), w.to(DEV), bias=b.to(DEV), act=L.ACT_RESRELU, residual=r.to(DEV)).cpu()
    assert relerr(o2, (lin + r.double()).clamp_min(0)) < 3e-6 and (o2 >= 0).all()


def test_residual_relu_needs_a_residual():
    a = torch.randn(64, 64, device=DEV)
    with pytest.raises(L.AcxError, match="RESRELU needs a residual"):
        ops.gemm(a, a, act=L.ACT_RESRELU)


def _attnpool_ref(x, pos, wq, bq, wk, bk, wv, bv, wc, bc, heads):
    """AttentionPool2d (clip/model.py:81-108) on NHWC tokens x [F, HW, E], fp64"""
    x = x.double()
    t = torch.cat([x.mean(1, keepdim=True), x], 1) + pos.double()
    q = t[:, :1] @ wq.double().T + bq.double()
    k = t @ wk.double().T + bk.double()
    v = t @ wv.double().T + bv.double()
    Fr, L_, E = t.shape
    q = q.view(Fr, 1, heads, 64).transpose(1, 2) * 0.125
    k = k.view(Fr, L_, heads, 64).transpose(1, 2)
    v = v.view(Fr, L_, heads, 64).transpose(1, 2)
    o = (torch.softmax(q @ k.transpose(-1, -2), -1) @ v).transpose(1, 2).reshape(Fr, E)
    return o @ wc.double().T + bc.double()


@pytest.mark.parametrize("HW,heads", [(49, 32), (81, 40), (144, 48), (196, 64)])
def test_attention_pool_pieces_vs_fp64(HW, heads):
    """The attention pool as acx_resnet_encode runs it: tokens (mean + positional), k | v of every token and q of token 0 into one
    q | k | v buffer, acx_attention_cls (50 / 82 / 145 / 197 keys, 32-64 heads), c_proj."""
    E, Fr, out_dim = heads * 64, 3, 512
    g = torch.Generator().manual_seed(HW)
    x = torch.randn(Fr, HW, E, generator=g)
    pos = torch.randn(HW + 1, E, generator=g) * E ** -0.5
    ws = [torch.randn(E, E, generator=g) * E ** -0.5 for _ in range(3)]
    bs = [torch.randn(E, generator=g) * 0.02 for _ in range(3)]
    wc, bc = torch.randn(out_dim, E, generator=g) * E ** -0.5, torch.randn(out_dim, generator=g) * 0.02
    d = lambda t: t.to(DEV).contiguous()                                   # noqa: E731
    tok = ops.attnpool_tokens(d(x.reshape(-1, E)), d(pos), Fr, HW)
    t_ref = torch.cat([x.double().mean(1, keepdim=True), x.double()], 1) + pos.double()
    assert relerr(tok.cpu(), t_ref.reshape(-1, E)) < 1e-6
    L_ = HW + 1
    qkv = torch.zeros(Fr * L_, 3 * E, device=DEV)
    ops.gemm(tok, d(torch.cat([ws[1], ws[2]])), bias=d(torch.cat([bs[1], bs[2]])), out=qkv[:, E:])
    q = ops.gemm(tok.view(Fr, L_ * E)[:, :E].contiguous(), d(ws[0]), bias=d(bs[0]))
    qkv.view(Fr, L_, 3 * E)[:, 0, :E] = q
    o = torch.empty(Fr, E, device=DEV)
    h = ops._h(qkv)
    L.check(L.lib().acx_attention_cls(h, qkv.data_ptr(), 3 * E, o.data_ptr(), E, Fr, L_, heads, ops._stream()), h)
    out = ops.gemm(o, d(wc), bias=d(bc)).cpu()
    ref = _attnpool_ref(x, pos, ws[0], bs[0], ws[1], bs[1], ws[2], bs[2], wc, bc, heads)
    assert relerr(out, ref) < 1e-5


# ----------------------------------------------------------------------------------------------------------------- encoders
_RNS = {}


def _rn(tag, golden):
    """one encoder per fixture for the whole module (RN50x64: 421 M parameters drawn on the host once)"""
    if tag not in _RNS:
        g = golden(tag)
        arch, geom = GEOMS[tag]
        with torch.device(DEV):
            m = ModifiedResNet(geom.vision_layers, geom.embed_dim, geom.resnet_heads, geom.image_resolution, geom.vision_width,
                               precision="f32", arch=arch)
        m.load_state_dict(IW.init_resnet_state_dict(geom, int(g["seed"]), prefix=""), strict=True)
        _RNS[tag] = m.eval()
    return _RNS[tag]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _RNS.clear()
    torch.cuda.empty_cache()


def _frames(tag, golden, n=2):
    g = golden(tag)
    f = R.vit_frames(int(g["seed"]), n, GEOMS[tag][1].image_resolution)
    assert abs(float(f[:2].double().sum()) - float(g["frames_checksum"])) < 1e-6
    return f


@pytest.mark.parametrize("tag", list(GEOMS))
def test_resnet_golden(golden, tag):
    """The encoder (every BatchNorm folded, padded channels for RN50x4 / RN50x16) against the reference ModifiedResNet.eval() on
    2 frames, at the ViT goldens' bounds ("auto" runs these same f32 kernels for the ResNets: test_resnet_auto_is_f32)."""
    g = golden(tag)
    m = _rn(tag, golden)
    m.precision = "f32"
    out = m(_frames(tag, golden).to(DEV))
    assert out.shape == g["out"].shape
    assert relerr(out, g["out"]) < TOL and elem_ok(out, g["out"])


@pytest.mark.parametrize("tag", ["rn50", "rn50x16"])
def test_resnet_full_launch_properties(golden, tag):
    """512 frames in ONE call (RN50x16: the layer1 activations of the whole launch are 7.2 GB; acx_resnet_encode runs them in
    internal batches below 2^31 bytes): identical frames give bit-identical rows wherever they sit, and the rows agree with the
    2-frame launch and the reference."""
    g = golden(tag)
    m = _rn(tag, golden)
    m.precision = "auto"
    m.chunk = 512
    R_ = GEOMS[tag][1].image_resolution
    base = _frames(tag, golden)
    extra = torch.randn(6, 3, R_, R_, generator=torch.Generator().manual_seed(5))
    eight = torch.cat([base, extra], 0)
    idx = torch.arange(512) % 8
    idx[-12:] = torch.tensor([7, 3, 0, 1, 5, 5, 2, 6, 4, 0, 1, 7])
    x = eight[idx].to(DEV)
    out = m(x)
    del x
    assert out.shape == (512, GEOMS[tag][1].embed_dim) and torch.isfinite(out).all()
    for k in range(8):
        rows = out[idx.to(DEV) == k]
        assert torch.equal(rows, rows[:1].expand_as(rows)), k
    small = m(base.to(DEV))
    assert relerr(out[:2], small) < 1e-5
    assert relerr(out[:2], g["out"]) < TOL and elem_ok(out[:2], g["out"])


def test_resnet_auto_is_f32(golden):
    """ "auto" routes the ResNets' products to the f32 kernels ("Other backbones: ResNets"): bit-identical to "f32"."""
    m = _rn("rn101", golden)
    x = torch.randn(8, 3, 224, 224, generator=torch.Generator().manual_seed(8)).to(DEV)
    m.precision = "f32"
    o32 = m(x)
    m.precision = "auto"
    assert torch.equal(m(x), o32)


# ----------------------------------------------------------------------------------------------------------- training mode
@pytest.mark.parametrize("rows,C", [(262144, 4096), (1048576, 96), (100003, 2048)])
def test_wide_bn_stats_vs_fp64(rows, C):
    """acx_bn_stats beyond 64 columns (its wide decomposition): mean, biased and unbiased variance against fp64, run-to-run
    identical."""
    g = torch.Generator(device=DEV).manual_seed(C)
    x = torch.randn(rows, C, generator=g, device=DEV) * 2.0 + torch.linspace(-1, 3, C, device=DEV)
    nb = int(L.lib().acx_bn_workspace_bytes(rows, C))
    ws = torch.empty(nb, dtype=torch.uint8, device=DEV)
    outs = []
    for _ in range(2):
        m, vb, vu = (torch.empty(C, device=DEV) for _ in range(3))
        h = ops._h(x)
        L.check(L.lib().acx_bn_stats(h, x.data_ptr(), rows, C, m.data_ptr(), vb.data_ptr(), vu.data_ptr(), ws.data_ptr(), nb,
                                     ops._stream()), h)
        outs.append((m, vb, vu))
    xd = x.double()
    rm = xd.mean(0)
    rvb = ((xd - rm) ** 2).mean(0)
    del xd
    assert relerr(outs[0][0], rm) < 1e-6 and relerr(outs[0][1], rvb) < 1e-6
    assert relerr(outs[0][2], rvb * rows / (rows - 1)) < 1e-6
    for a, b in zip(outs[0], outs[1]):
        assert torch.equal(a, b)


TRAIN_BNS = ("bn1", "bn2", "bn3", "layer1.0.downsample.1", "layer4.2.bn3")


def _rn50_train(golden):
    g = golden("rn_train")
    geom = IW.RN50
    with torch.device(DEV):
        m = ModifiedResNet(geom.vision_layers, geom.embed_dim, geom.resnet_heads, geom.image_resolution, geom.vision_width,
                           precision="f32", arch="RN50")
    m.load_state_dict(IW.init_resnet_state_dict(geom, int(g["seed"]), prefix=""), strict=True)
    frames = R.vit_frames(int(g["seed"]), 4, geom.image_resolution)
    assert abs(float(frames.double().sum()) - float(g["frames_checksum"])) < 1e-6
    return g, m, frames.to(DEV)


def test_resnet_training_mode_vs_reference(golden):
    """RN50 in .train() on 4 frames: every BatchNorm on the batch statistics of all frames, H and W (the wide acx_bn_stats above 64
    channels), running statistics updated with momentum 0.1 and the unbiased variance, num_batches_tracked + 1 -- output and
    buffers against the reference's .train() forward; a rerun from the same state is bit-identical; .eval() afterwards folds the
    UPDATED running statistics (the reference's .eval() output after its training call)."""
    g, m, x = _rn50_train(golden)
    m.train()
    out = m(x)
    assert relerr(out, g["out"]) < TOL and elem_ok(out, g["out"])
    sd = m.state_dict()
    for name in TRAIN_BNS:
        for buf in ("running_mean", "running_var"):
            assert relerr(sd[f"{name}.{buf}"], g[f"{name}.{buf}"]) < 1e-5, (name, buf)
    run = [v.double().cpu() for k, v in sd.items() if k.endswith(("running_mean", "running_var"))]
    assert abs(sum(float(v.sum()) for v in run) - float(g["running_sum"])) < 1e-5 * float(g["running_abs_sum"])
    assert abs(sum(float(v.abs().sum()) for v in run) - float(g["running_abs_sum"])) < 1e-5 * float(g["running_abs_sum"])
    nbt = np.array([int(v) for k, v in sd.items() if k.endswith("num_batches_tracked")])
    assert np.array_equal(nbt, g["num_batches_tracked"]) and (nbt == 1).all()
    # rerun from the same initial state: bit-identical output and buffers
    _, m2, _ = _rn50_train(golden)
    out2 = m2.train()(x)
    assert torch.equal(out, out2)
    sd2 = m2.state_dict()
    assert all(torch.equal(sd[k], sd2[k]) for k in sd)
    # eval afterwards: the running statistics the training call left
    m.eval()
    ev = m(x[:2])
    assert relerr(ev, g["eval_after"]) < TOL and elem_ok(ev, g["eval_after"])


# --------------------------------------------------------------------------------------------------------------------- head
def _net(prompts_table, seed, arch, with_image_encoder=True, **kw):
    geom = dict((a, g_) for a, g_ in GEOMS.values())[arch]
    toks = torch.tensor(prompts_table["ucf"]["tokenized_prompts"], dtype=torch.int32)
    hc = E2E_HEAD
    net = AnomalyCLIP(arch=arch, labels_key="ucf", emb_size=hc.emb_size, depth=hc.depth, heads=hc.heads, dim_heads=None,
                      num_segments=32, seg_length=16, concat_features=False, normal_id=7, stride=1,
                      select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3,
                      n_ctx=8, shared_context=False, ctx_init="", **kw)
    sd = IW.init_anomalyclip_state_dict(geom, hc, toks, seed, with_image_encoder=with_image_encoder)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("image_encoder.") for k in missing) and (missing == [] or not with_image_encoder)
    return net.to(DEV)


def test_e2e_rn50x4_golden_test_and_train_forward(golden, prompts_table):
    """AnomalyCLIP(arch = "RN50x4") from 640-wide features against the reference's AnomalyCLIP: the head at D = 640 (text tower
    640 / 10 heads, selector, temporal projection 640 -> 256) in test mode (S = 2) and the train forward (fixed selection masks)."""
    g = golden("e2e_rn50x4")
    seed = int(g["seed"])
    net = _net(prompts_table, seed, "RN50x4", with_image_encoder=False)
    inp = R.e2e_inputs(seed, 640)
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


def test_step_graph_d640_bit_identical_to_autograd(prompts_table):
    """One train_batch at D = 640 (RN50x4 head): the whole-step graph path is bit-identical to the eager autograd path -- losses,
    gradients, parameters."""
    from anomalyclip_amd.anomaly_clip_module import AnomalyCLIPModule
    D, B = 640, 8
    mods = []
    for _ in range(2):
        net = _net(prompts_table, 23, "RN50x4", with_image_encoder=False)
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
        f, l_ = feats.to(DEV), labels.to(DEV)
        batch = ((f[B // 2:], l_[B // 2:]), (f[:B // 2], l_[:B // 2]))
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


@pytest.mark.parametrize("size", [288, 384, 448])
def test_frame_preprocessing_resnet_sizes_match_pil(size):
    """`data.input_size` 288 / 384 / 448 (RN50x4 / RN50x16 / RN50x64): the 8-bit resample stages bit-exact with Pillow."""
    from anomalyclip_amd.preprocess import preprocess_frames, CLIP_MEAN, CLIP_STD
    g = torch.Generator().manual_seed(size)
    frames = torch.randint(0, 256, (2, 480, 640, 3), generator=g, dtype=torch.uint8)
    frames[0, :240] = 255
    ref = O.preprocess_frames_ref(frames.numpy(), size=size)
    out = preprocess_frames(frames.to(DEV), size=size)
    assert out.shape == (2, 3, size, size)
    assert (out.cpu() - ref).abs().max().item() < 2e-6
    m, s_ = torch.tensor(CLIP_MEAN).view(1, 3, 1, 1), torch.tensor(CLIP_STD).view(1, 3, 1, 1)
    assert torch.equal(((out.cpu() * s_ + m) * 255).round(), ((ref * s_ + m) * 255).round())


def test_text_tower_1024_golden(golden, prompts_table):
    """RN50x64's text tower (width 1024, 16 heads) against the reference TextEncoder."""
    g = golden("text_rn50x64")
    net = _net(prompts_table, int(g["seed"]), "RN50x64", with_image_encoder=False)
    with torch.no_grad():
        tf = net.get_text_features()
    assert tf.shape == (14, 1024)
    assert relerr(tf, g["out"]) < TOL and elem_ok(tf, g["out"])


def test_rn101_frames_path_equals_features_path(prompts_table):
    """AnomalyCLIP(arch="RN101", load_from_features=False) in test mode: the encoder runs inside forward (anomaly_clip.py:119-123)
    and gives bit-identically what encoding first and passing the features gives."""
    net = _net(prompts_table, 81, "RN101", load_from_features=False).eval()
    frames = torch.randn(1, 512, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
    nc = torch.randn(512, generator=torch.Generator().manual_seed(4)).to(DEV) * 0.1
    with torch.no_grad():
        sim_f, sc_f = net(frames, torch.zeros(1000), nc, 1, True)
        feats = net.image_encoder(frames.view(-1, 3, 224, 224)).view(1, 1, 512, 512)
        net.load_from_features = True
        sim_x, sc_x = net(feats, torch.zeros(1000), nc, 1, True)
    assert torch.equal(sim_f, sim_x) and torch.equal(sc_f, sc_x) and torch.isfinite(sc_f).all()
