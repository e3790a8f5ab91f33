"""-m gpu: the ResNet encoders on the bf16 matrix cores, precision "bf16x6" (ACX_PREC_BF16X6) -- the plane kernel's 3x3 convolution
on any grid and row count (acx_gemm_x6.h CONV = 2) and its ReLU / residual-then-ReLU epilogues against fp64, the encoders against
the reference's goldens and against their own "f32" runs, identical frames in one launch, the head of AnomalyCLIP(arch="RN50x4",
precision="bf16x6") and a feature file written by the extractor's command line.  Bounds: the project's own -- element-wise
2e-6 * (sum |a||w| + |b|) of test_gemm_bf16x6_is_f32_accurate, relerr < 3e-6 of test_conv3x3_relu_grids_and_padded_channels, TOL /
elem_ok of test_gpu_clip_resnet.py."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as Fnn
from PIL import Image

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import extract as X
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.clip_resnet import ModifiedResNet
from anomalyclip_amd.preprocess import preprocess_crops
import recipes as R

DEV = "cuda"
TOL = 1e-4                                   # tests/test_gpu_clip_resnet.py
GEOMS = {"rn50": ("RN50", IW.RN50), "rn50x4": ("RN50x4", IW.RN50X4), "rn50x16": ("RN50x16", IW.RN50X16)}
E2E_HEAD = IW.HeadConfig(num_classes=14, normal_id=7, emb_size=256, heads=8, depth=1)


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def elem_ok(a, b):
    return R.elem_excess(a, b) <= 1.0


def within(out, ref, mag, what):
    """element-wise |out - fp64| <= 2e-6 * (sum |a||w| + |b|)"""
    e = (out.double().cpu() - ref).abs()
    bound = 2e-6 * mag + 1e-30
    worst = float((e / bound).max())
    print(f"{what}: max error / bound = {worst:.3g}, relerr = {relerr(out, ref):.3g}")
    assert bool((e <= bound).all()), (what, worst)


# --------------------------------------------------------------------------------------------------------------- convolution
def _conv_problem(F_, H, W, cin, cin_p, N, Np, seed):
    """NHWC rows with zero padding channels, weights [Np][9][cin_p] with zero rows / columns, fp64 relu(conv + b) and the
    magnitudes sum |x||w| + |b|"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(F_, H, W, cin, generator=g)
    w = torch.randn(N, cin, 3, 3, generator=g) * (9 * cin) ** -0.5
    b = torch.randn(N, generator=g) * 0.1
    xp = torch.zeros(F_, H, W, cin_p)
    xp[..., :cin] = x
    wp = torch.zeros(Np, 9, cin_p)
    wp[:N, :, :cin] = w.permute(0, 2, 3, 1).reshape(N, 9, cin)
    bp = torch.zeros(Np)
    bp[:N] = b
    nchw = x.permute(0, 3, 1, 2).double()
    ref = Fnn.conv2d(nchw, w.double(), b.double(), padding=1).permute(0, 2, 3, 1).reshape(-1, N).clamp_min(0)
    mag = Fnn.conv2d(nchw.abs(), w.double().abs(), b.double().abs(), padding=1).permute(0, 2, 3, 1).reshape(-1, N)
    a3 = ops.split_bf16x3(xp.reshape(-1, cin_p).to(DEV))
    w3 = ops.split_bf16x3(wp.reshape(Np, 9 * cin_p).to(DEV))
    return a3, w3, bp.to(DEV), ref, mag


def _conv(a3, w3, b, H, W, cin_p, act=L.ACT_RELU, planes_out=False, split_k=True):
    return ops.gemm_x6(a3, w3, bias=b, act=act, amap=L.AMAP_CONV3X3, gn=H, gl=W, cin=cin_p, planes_out=planes_out, split_k=split_k)


@pytest.mark.parametrize("F_,H,W,cin,cin_p,N,Np", [(3, 7, 7, 64, 64, 64, 64),        # 147 rows: one partial tile over three frames
                                                   (2, 9, 9, 32, 32, 96, 96),
                                                   (1, 56, 56, 64, 64, 64, 64),      # 12.25 tiles
                                                   (2, 5, 12, 64, 64, 128, 128),     # rectangular: gn and gl, rows and columns
                                                   (3, 18, 18, 96, 96, 96, 96),      # 972 rows: frame boundaries at three phases
                                                   (1, 16, 16, 40, 64, 40, 64)])     # padded channels, the power-of-two route
def test_conv3x3_relu_any_grid(F_, H, W, cin, cin_p, N, Np):
    """ACX_AMAP_CONV3X3 + ACX_ACT_RELU with pairs = 6 on the ResNets' grids, to f32 and to planes, against fp64 conv2d"""
    a3, w3, b, ref, mag = _conv_problem(F_, H, W, cin, cin_p, N, Np, seed=H * W * cin + F_)
    out = _conv(a3, w3, b, H, W, cin_p)
    assert out.shape == (F_ * H * W, Np)
    within(out[:, :N], ref, mag, f"conv {F_} x {H} x {W}, cin {cin}, N {N}")
    assert relerr(out[:, :N], ref) < 3e-6 and (out >= 0).all()
    assert not out[:, N:].any()                                            # padded output columns stay exactly 0
    pl = _conv(a3, w3, b, H, W, cin_p, planes_out=True)
    assert pl.shape == (3, F_ * H * W, Np) and torch.equal(pl.float().sum(0), out)     # hi + mid + lo == the f32 output exactly
    # a frame's rows do not depend on the frames beside it: the first frame alone (another tile phase for every later row)
    one = _conv(a3[:, :H * W].contiguous(), w3, b, H, W, cin_p)
    assert torch.equal(one, out[:H * W])


def test_conv3x3_power_of_two_grid_is_the_existing_route():
    """16 x 16 at M = 256 (one whole tile on a power-of-two grid): the ReLU epilogue on the shift row map gives, bit for bit, the
    ReLU of what the existing route (no activation) gives; and the general map on the same image, zero-padded into an 18 x 18
    frame, gives the same bits in the interior (a tap outside the 16 x 16 frame reads the zero page there and a zero pixel here)"""
    a3, w3, b, ref, mag = _conv_problem(1, 16, 16, 40, 64, 40, 64, seed=16)
    plain = _conv(a3, w3, b, 16, 16, 64, act=L.ACT_NONE, split_k=False)     # (whole K per tile, as the ReLU epilogue always runs)
    out = _conv(a3, w3, b, 16, 16, 64)
    assert torch.equal(out, plain.clamp_min(0))
    big = torch.zeros(3, 18, 18, 64, dtype=a3.dtype, device=DEV)
    big[:, 1:17, 1:17] = a3.view(3, 16, 16, 64)
    gen = _conv(big.view(3, 324, 64).contiguous(), w3, b, 18, 18, 64)
    assert torch.equal(gen.view(18, 18, 64)[1:17, 1:17].reshape(256, 64), out)


def test_conv3x3_refusals():
    a3, w3, b, _, _ = _conv_problem(1, 7, 7, 64, 64, 64, 64, seed=1)
    with pytest.raises(L.AcxError):                                        # pairs = 3 keeps refusing convolutions
        ops.gemm_x6(a3, w3, bias=b, amap=L.AMAP_CONV3X3, gn=7, gl=7, cin=64, pairs=3)
    r = torch.zeros(49, 64, device=DEV)
    with pytest.raises(L.AcxError, match="no residual"):                   # the general map: no residual epilogue
        ops.gemm_x6(a3, w3, bias=b, residual=r, amap=L.AMAP_CONV3X3, gn=7, gl=7, cin=64)
    # an A plane of 4 GiB or more is beyond the per-lane 32-bit byte offsets: refused on the host, before any launch (the descriptor
    # only CLAIMS that many rows: 49 x 700,000 rows of 64 channels = 4.39e9 bytes per plane; nothing is read)
    d = L.GemmDesc()
    d.A, d.W, d.C = a3.data_ptr(), w3.data_ptr(), r.data_ptr()
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc = 49 * 700000, 64, 576, 64, 576, 64
    d.a_dtype, d.c_dtype, d.prec, d.pairs, d.act = L.ACX_BF16, L.ACX_F32, L.PREC_BF16, 6, L.ACT_RELU
    d.a_plane_stride, d.w_plane_stride = 49 * 700000 * 64 * 2, 64 * 576 * 2
    d.amap, d.gn, d.gl, d.cin, d.bias, d.zero_page = L.AMAP_CONV3X3, 7, 7, 64, b.data_ptr(), ops._zero_page(a3.device).data_ptr()
    h = ops._h(a3)
    assert L.lib().acx_gemm(h, ctypes.byref(d), ops._stream()) == -2
    assert b"32-bit byte offsets" in L.lib().acx_last_error(h)


# ----------------------------------------------------------------------------------------------------------------- epilogues
@pytest.mark.parametrize("M,N,K", [(49, 2048, 512), (800, 256, 64), (6272, 1024, 256)])
def test_relu_and_residual_relu_epilogues_x6(M, N, K):
    """pairs = 6 on identity rows: ACX_ACT_RELU to f32 and to planes, ACX_ACT_RESRELU with a residual (once aliasing the output)"""
    g = torch.Generator().manual_seed(M + N)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    b = torch.randn(N, generator=g) * 0.2
    r = torch.randn(M, N, generator=g)
    lin = a.double() @ w.double().T + b.double()
    mag = a.double().abs() @ w.double().abs().T + b.double().abs()
    a3, w3, bd, rd = ops.split_bf16x3(a.to(DEV)), ops.split_bf16x3(w.to(DEV)), b.to(DEV), r.to(DEV)
    o1 = ops.gemm_x6(a3, w3, bias=bd, act=L.ACT_RELU)
    within(o1, lin.clamp_min(0), mag, f"relu {M} x {N} x {K}")
    assert relerr(o1, lin.clamp_min(0)) < 3e-6 and (o1 >= 0).all()
    p1 = ops.gemm_x6(a3, w3, bias=bd, act=L.ACT_RELU, planes_out=True)
    assert torch.equal(p1.float().sum(0), o1)
    o2 = ops.gemm_x6(a3, w3, bias=bd, act=L.ACT_RESRELU, residual=rd)
    within(o2, (lin + r.double()).clamp_min(0), mag, f"resrelu {M} x {N} x {K}")
    assert relerr(o2, (lin + r.double()).clamp_min(0)) < 3e-6 and (o2 >= 0).all()
    alias = rd.clone()
    o3 = ops.gemm_x6(a3, w3, bias=bd, act=L.ACT_RESRELU, residual=alias, out=alias)
    assert o3.data_ptr() == alias.data_ptr() and torch.equal(o3, o2)


def test_relu_epilogue_refusals_x6():
    a3 = ops.split_bf16x3(torch.randn(64, 64, device=DEV))
    with pytest.raises(L.AcxError, match="RESRELU needs a residual"):
        ops.gemm_x6(a3, a3, act=L.ACT_RESRELU)
    r = torch.zeros(64, 64, device=DEV)
    for act, res in ((L.ACT_RELU, None), (L.ACT_RESRELU, r)):              # pairs = 3 takes neither
        with pytest.raises(L.AcxError):
            ops.gemm_x6(a3, a3, act=act, residual=res, pairs=3)


# ------------------------------------------------------------------------------------------------------------------ encoders
_RNS = {}


def _rn(tag, golden):
    if tag not in _RNS:
        g = golden(tag)
        arch, geom = GEOMS[tag]
        with torch.device(DEV):
            m = ModifiedResNet(geom.vision_layers, geom.embed_dim, geom.resnet_heads, geom.image_resolution, geom.vision_width,
                               precision="bf16x6", arch=arch)
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
def test_resnet_bf16x6_golden_and_f32(golden, tag):
    """2 frames at "bf16x6": within the golden bounds of the reference's output, within 1e-5 of the same module at "f32" -- and
    "auto" afterwards is still bit-identical to "f32" (the derived weights of one precision never reach another)"""
    g = golden(tag)
    m = _rn(tag, golden)
    x = _frames(tag, golden).to(DEV)
    m.precision = "bf16x6"
    out = m(x)
    assert out.shape == g["out"].shape
    print(f"{tag}: relerr vs golden = {relerr(out, g['out']):.3g}")
    assert relerr(out, g["out"]) < TOL and elem_ok(out, g["out"])
    m.precision = "f32"
    o32 = m(x)
    print(f"{tag}: relerr vs f32 = {relerr(out, o32):.3g}")
    assert relerr(out, o32) < 1e-5
    m.precision = "auto"
    assert torch.equal(m(x), o32)
    m.precision = "bf16x6"
    assert torch.equal(m(x), out)


def test_resnet_bf16x6_identical_frames_in_one_launch(golden):
    """RN50, 16 frames made of 4 distinct ones in scrambled order, one call: equal frames give bit-identical rows wherever they
    sit (no product's arithmetic depends on the launch's rows), and the rows agree with a 4-frame call"""
    m = _rn("rn50", golden)
    m.precision = "bf16x6"
    four = torch.cat([_frames("rn50", golden), torch.randn(2, 3, 224, 224, generator=torch.Generator().manual_seed(5))], 0)
    idx = torch.tensor([2, 0, 3, 1, 1, 3, 0, 2, 0, 0, 3, 2, 1, 2, 3, 1])
    out = m(four[idx].to(DEV))
    assert out.shape == (16, 1024) and torch.isfinite(out).all()
    for k in range(4):
        rows = out[idx.to(DEV) == k]
        assert rows.shape[0] == 4 and torch.equal(rows, rows[:1].expand_as(rows)), k
    small = m(four.to(DEV))
    assert relerr(out[[1, 3, 0, 2]], small) < 1e-5


def test_resnet_bf16x6_training_mode_runs_the_f32_kernels(golden):
    """the training-mode BatchNorm pass is a correctness path on the f32 kernels for every precision: bit-identical to "f32" """
    geom = IW.RN50
    outs = []
    x = _frames("rn50", golden).to(DEV)
    for prec in ("bf16x6", "f32"):
        with torch.device(DEV):
            m = ModifiedResNet(geom.vision_layers, geom.embed_dim, geom.resnet_heads, geom.image_resolution, geom.vision_width,
                               precision=prec, arch="RN50")
        m.load_state_dict(IW.init_resnet_state_dict(geom, 3, prefix=""), strict=True)
        outs.append(m.train()(x))
    assert torch.equal(outs[0], outs[1])


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_e2e_rn50x4_bf16x6_head_golden(golden, prompts_table):
    """AnomalyCLIP(arch="RN50x4", precision="bf16x6") in test mode on the fixture of test_e2e_rn50x4_golden_test_and_train_forward,
    at that test's bounds: the image encoder takes the precision, the rest runs "auto" """
    g = golden("e2e_rn50x4")
    seed = int(g["seed"])
    toks = torch.tensor(prompts_table["ucf"]["tokenized_prompts"], dtype=torch.int32)
    hc = E2E_HEAD
    net = AnomalyCLIP(arch="RN50x4", labels_key="ucf", emb_size=hc.emb_size, depth=hc.depth, heads=hc.heads, dim_heads=None,
                      num_segments=32, seg_length=16, concat_features=False, normal_id=7, stride=1,
                      select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3,
                      n_ctx=8, shared_context=False, ctx_init="", precision="bf16x6")
    assert net.image_encoder.precision == "bf16x6" and net.precision == "auto"
    sd = IW.init_anomalyclip_state_dict(IW.RN50X4, hc, toks, seed, with_image_encoder=False)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("image_encoder.") for k in missing)
    net = net.to(DEV).eval()
    inp = R.e2e_inputs(seed, 640)
    with torch.no_grad():
        sim, sc = net(inp["test_feats"].to(DEV), torch.zeros(1000), inp["nc"], 2, True)
    assert relerr(sim, g["test_sim"]) < TOL and relerr(sc, g["test_scores"]) < TOL
    assert elem_ok(sim, g["test_sim"]) and elem_ok(sc, g["test_scores"])


def test_extract_command_line_bf16x6(tmp_path, golden, capsys):
    """python -m anomalyclip_amd.extract --arch RN50 --precision bf16x6 on one folder of 6 frames: the file's rows are the
    module's rows at that precision, bit for bit"""
    m = _rn("rn50", golden)
    m.precision = "bf16x6"
    weights = str(tmp_path / "rn50.pt")
    torch.save({k: v.cpu() for k, v in m.state_dict().items()}, weights)
    folder = tmp_path / "frames" / "v"
    os.makedirs(folder)
    rng = np.random.default_rng(7)
    for t in range(6):
        Image.fromarray(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(str(folder / f"{t:06d}.jpg"), quality=90)
    dec = np.stack([np.asarray(Image.open(str(folder / f"{t:06d}.jpg")).convert("RGB")) for t in range(6)])
    rc = X.main(["--arch", "RN50", "--weights", weights, "--frames-root", str(tmp_path / "frames"), "--out-root",
                 str(tmp_path / "feats"), "--precision", "bf16x6"])
    assert rc == 0
    got = np.load(str(tmp_path / "feats" / "v.npy"), allow_pickle=False)
    with torch.no_grad():
        want = m(preprocess_crops(torch.from_numpy(dec).to(DEV), 224, None, 1).view(-1, 3, 224, 224)).cpu().numpy()
    assert got.shape == (6, 1024) and np.array_equal(got, want)
