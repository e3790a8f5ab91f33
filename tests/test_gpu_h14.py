"""-m gpu: open_clip's ViT-H-14 (image tower: width 1280, 16 heads of 80).

  - the attention at head dimension 80 (acx_attention_hd, _x3_hd, _cls_hd) on every case of clip_attn_hd_ref.CASES, element by element
    against the fp64 closed form of attn_ref at 2e-6 * S; every route tag asserted against acx_attention_hd_route; the output poisoned
    before the launch; every comparison prints its worst |err| / S first (pytest -s, the ATTN_RATIO lines);
  - the row-wise kernels at width 1280 with rowwise_ref's forms and bounds;
  - the encoder against the reference's VisionTransformer(224, 14, 1280, 32, 16, 1024) with nn.GELU (tests/golden/vit_h14.npz,
    make_golden_h14.py) at the bound of test_vit_arch_golden, its launch sizes, the text tower, AnomalyCLIP(arch="ViT-H-14") and extract.
The full-geometry encoder (632 M parameters) is drawn once for the module."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import extract as X
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.clip_vit import VisionTransformer
from anomalyclip_amd.preprocess import preprocess_crops

import attn_ref as AR
import clip_attn_hd_ref as HR
import recipes as R
import rowwise_ref as RR

DEV = "cuda"
ARCH = "ViT-H-14"
TOL = 1e-4                                   # test_vit_arch_golden's bound (from test_gpu_model.test_vit_b16_golden)
SENTINEL, SENTINEL16 = 0x7FA5A5A5, 0x7FA5    # a NaN's bit pattern no kernel produces


def relerr(a, b):
    a, b = torch.as_tensor(a).double().cpu(), torch.as_tensor(b).double().cpu()
    return ((a - b).abs().max() / (b.abs().max() + 1e-30)).item()


def elem_ok(a, b):
    return R.elem_excess(a, b) <= 1.0


def _poison(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, SENTINEL, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full(shape, SENTINEL16, dtype=torch.int16, device=DEV).view(dtype)


def _is_poison(t):
    if t.dtype == torch.float32:
        return bool((t.contiguous().view(torch.int32) == SENTINEL).all())
    return bool((t.contiguous().view(torch.int16) == SENTINEL16).all())


# =============================================================================================================== attention
def _hd(c, qd, tail_rows=0):
    """acx_attention_hd on a poisoned output of batch * L + tail_rows rows: (the rows of the problem, the rows behind them)"""
    rows, W = c.batch * c.L, c.heads * HR.E
    buf = _poison((rows + tail_rows, W), torch.float32)
    ops.attention_hd(qd, c.batch, c.L, c.heads, out=buf[:rows])
    torch.cuda.synchronize()
    return buf[:rows], buf[rows:]


@pytest.mark.parametrize("c", [c for c in HR.CASES if c.entry == "hd"], ids=HR.case_id)
def test_attention_hd_every_route_against_fp64(c):
    qkv, o, S = HR.reference(c)
    qd = qkv.to(DEV)
    assert L.lib().acx_attention_hd_route(ops._h(qd), c.L, HR.E, 1) == HR.route_id(c.route)
    if c.many:
        items = c.batch * c.heads * c.qblocks
        assert items > 2 * torch.cuda.get_device_properties(qd.device).multi_processor_count, items
    got, tail = _hd(c, qd, tail_rows=16 if c.L < 16 else 0)
    assert _is_poison(tail), "wrote rows beyond batch * L"
    assert bool(torch.isfinite(got).all()), "left poison in (or wrote a non-finite value to) its output"
    got2, _ = _hd(c, qd)
    failures = []
    for b0 in range(0, c.batch, 8):                                       # row-wise, in chunks of sequences
        r = slice(b0 * c.L, min(b0 + 8, c.batch) * c.L)
        try:
            AR.within(got[r], o[r], S[r], HR.case_id(c), "hd80_" + c.route + ("_many" if c.many else ""))
        except AssertionError as err:
            failures.append(str(err))
    if not torch.equal(got.view(torch.int32), got2.view(torch.int32)):
        failures.append("differs run to run")
    assert not failures, failures


@pytest.mark.parametrize("c", [c for c in HR.CASES if c.entry in ("x3", "x3_panel")], ids=HR.case_id)
def test_attention_hd_planes_recombine_to_the_f32_output(c):
    """hi + mid + lo of the planes, row-major and (through ops.unpanel) K-panel, against the f32 rows of the same launch shape within
    2^-20 * max |ref| (the existing plane tests' bound); they are in fact the exact split of those rows, plane by plane; and the f32
    rows meet the fp64 bound.  heads = 3: ldo = 256 for the panels, the columns 240 .. 255 keep the poison."""
    qkv, o, S = HR.reference(c)
    qd = qkv.to(DEV)
    rows, W = c.batch * c.L, c.heads * HR.E
    o32 = ops.attention_hd(qd, c.batch, c.L, c.heads)
    AR.within(o32, o, S, HR.case_id(c), "hd80_" + c.route)
    panel = c.entry == "x3_panel"
    ldo = (W + 31) // 32 * 32 if panel else W
    raw = _poison((3, rows, ldo), torch.bfloat16)
    ops.attention_hd(qd, c.batch, c.L, c.heads, planes_out=True, panel_out=panel, out=raw)
    torch.cuda.synchronize()
    planes = ops.unpanel(raw) if panel else raw
    assert _is_poison(planes[:, :, W:]), "wrote behind the heads' columns"
    planes = planes[:, :, :W]
    s = planes.double().sum(0)
    bound = 2.0 ** -20 * float(o.abs().max())
    err = float((s.cpu() - o32.double().cpu()).abs().max())
    print(f"ATTN_RATIO hd80_{c.entry} {HR.case_id(c)} planes - f32: {err:.3e} (bound {bound:.3e})")
    assert err <= bound
    r = o32
    for p in range(3):
        want = r.bfloat16()
        assert torch.equal(planes[p].contiguous().view(torch.int16), want.view(torch.int16)), f"plane {p} is not the split of the f32 output"
        r = r - want.float()


@pytest.mark.parametrize("c", [c for c in HR.CASES if c.entry == "cls"], ids=HR.case_id)
def test_attention_cls_hd_against_fp64_and_row_0(c):
    qkv, o, S = HR.reference(c)
    qd = qkv.to(DEV)
    W = c.heads * HR.E
    out = _poison((c.batch, W + 3), torch.float32)                         # ldo = W + 3: no alignment is asked of out
    h = ops._h(qd)
    L.check(L.lib().acx_attention_cls_hd(h, qd.data_ptr(), 3 * W, out.data_ptr(), W + 3, c.batch, c.L, c.heads, HR.E, ops._stream()), h)
    torch.cuda.synchronize()
    assert _is_poison(out[:, W:]), "wrote behind an output row"
    got = out[:, :W]
    AR.within(got, o, S, HR.case_id(c), "hd80_cls")
    full = ops.attention_hd(qd, c.batch, c.L, c.heads)[torch.arange(c.batch, device=DEV) * c.L]
    AR.within(full, o, S, HR.case_id(c) + " (row 0 of acx_attention_hd)", "hd80_" + HR.route_of(c.L))
    AR.within(got, full.double().cpu(), 2 * S, HR.case_id(c) + " (cls - row 0)", "hd80_cls_vs_row0")     # both within TOL * S of fp64
    assert torch.equal(got, ops.attention_hd(qd, c.batch, c.L, c.heads, cls=True))


def test_attention_hd_refusals_leave_the_output_alone():
    lib = L.lib()
    W = 80
    qkv = torch.zeros(1025 * 3 * W + 4, device=DEV)
    out = _poison((3 * 1025 * W + 4,), torch.float32)
    h, s, p, o = ops._h(qkv), ops._stream(), qkv.data_ptr(), out.data_ptr()
    assert lib.acx_attention_hd(h, p, 3 * W, o, W, 1, 1025, 1, 80, s) == lib.acx_attention_hd(h, p, 3 * W, o, W, 1, 0, 1, 80, s) == -2
    for hd in (48, 64, 96):
        assert lib.acx_attention_hd(h, p, 3 * hd, o, hd, 1, 197, 1, hd, s) == -2
        assert lib.acx_attention_cls_hd(h, p, 3 * hd, o, hd, 1, 197, 1, hd, s) == -2
        assert lib.acx_attention_x3_hd(h, p, 3 * hd, o, hd, 1, 197, 1, hd, 0, s) == -2
    assert lib.acx_attention_hd(h, p, 3 * W, o + 4, W, 1, 197, 1, 80, s) == lib.acx_attention_hd_route(h, 197, 80, 0) == -2
    assert lib.acx_attention_hd(h, p + 4, 3 * W, o, W, 1, 197, 1, 80, s) == -1
    assert lib.acx_attention_x3_hd(h, p, 3 * W, o, W, 1, 197, 1, 80, 1, s) == -1                      # panels: ldo % 32
    torch.cuda.synchronize()
    assert _is_poison(out)


# =============================================================================================================== row-wise at 1280
ROWS_1280 = (1, 2, 3, 257, 514)


@pytest.mark.parametrize("rows", ROWS_1280)
def test_layernorm_1280_every_output_type(rows):
    """f32 within 2e-6 * S_y; bf16 within 2^-8 |ref| on top of it (test_layernorm_fwd_every_width's bounds); the row-major and the
    K-panel planes recombine to the f32 result within the split's round-off (three bf16 planes hold 24 bits: 2^-23 |y|) -- they are
    the exact split of the f32 rows, plane by plane.  Odd row counts take the one-row-per-wave panel kernel or the two-row one by the
    planes' alignment (rows * 1280 * 2 bytes is a multiple of 16 for every row count here: the two-row kernel, whose last pair is
    half empty at 1, 3 and 257 rows)."""
    D = 1280
    x, w, b, _, _ = RR.ln_inputs(rows, D, seed=11 * D + rows)
    ref, S = RR.ln_fwd(x, w, b, RR.NORM_LAYER)
    xd, wd, bd = x.to(DEV), w.to(DEV), b.to(DEV)
    out = ops.layernorm(xd, wd, bd)
    assert out.shape == (rows, D) and RR.within(out, ref, S, f"y D={D} rows={rows}", "ln_fwd_1280")
    outb = ops.layernorm(xd, wd, bd, out_dtype=torch.bfloat16)
    assert bool(((outb.double().cpu() - ref).abs() <= 2.0 ** -8 * ref.abs() + RR.TOL * S).all())
    wide = torch.full((rows, D + 8), 1e3)
    wide[:, :D] = x
    assert torch.equal(ops.layernorm(wide.to(DEV), wd, bd, rows=rows, ldx=D + 8), out)
    for panel in (False, True):
        raw = ops.layernorm(xd, wd, bd, planes_out=True, panel_out=panel)
        planes = ops.unpanel(raw) if panel else raw
        s = planes.double().sum(0)
        assert bool(((s - out.double()).abs() <= 2.0 ** -23 * out.double().abs()).all()), panel
        r = out
        for p in range(3):
            want = r.bfloat16()
            assert torch.equal(planes[p].contiguous().view(torch.int16), want.view(torch.int16)), (panel, p)
            r = r - want.float()


def test_layernorm_1280_f16_planes_stay_refused():
    x = torch.zeros(4, 1280, device=DEV)
    w = torch.ones(1280, device=DEV)
    with pytest.raises(L.AcxError, match="768 or 1024"):
        ops.layernorm_f16x2(x, w, w)


def test_vit_embed_1280():
    """test_vit_embed_every_width at W = 1280, and ViT-H-14's own 256 patches: within rowwise_ref's LayerNorm bound of the f32
    LayerNorm of (patch + pos)"""
    W = 1280
    for F_, T in ((3, 7), (2, 256)):
        g = torch.Generator().manual_seed(W + T)
        patches = (torch.randn(F_ * T, W, generator=g) * 2 + 0.3) * RR.row_scales(F_ * T, g)
        cls, pos = torch.randn(W, generator=g), torch.randn(T + 1, W, generator=g) * 0.5
        lw, lb = torch.randn(W, generator=g), torch.randn(W, generator=g)
        xin = torch.cat([cls.double().expand(F_, 1, W), patches.double().view(F_, T, W)], 1) + pos.double()
        ref, S = RR.ln_fwd(xin.view(-1, W), lw, lb, RR.NORM_LAYER)
        dev = [t.to(DEV) for t in (patches, cls, pos, lw, lb)]
        out = torch.full((F_ * (T + 1), W), float("nan"), device=DEV)
        h = L.ctx(torch.cuda.current_device())
        L.check(L.lib().acx_vit_embed(h, *[t.data_ptr() for t in dev], out.data_ptr(), F_, T, W, torch.cuda.current_stream().cuda_stream), h)
        assert RR.within(out, ref, S, f"W={W} T={T}", "vit_embed_1280")


# =============================================================================================================== the encoder
@pytest.fixture(scope="module")
def h14(golden):
    g = golden("vit_h14")
    geom = IW.VIT_H14
    with torch.device(DEV):
        vit = VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers, geom.vision_heads,
                                geom.embed_dim, precision="f32", arch=ARCH, act=geom.act)
    vit.load_state_dict(IW.init_vit_state_dict(geom, int(g["seed"]), prefix=""), strict=True)
    yield vit.eval()
    del vit
    torch.cuda.empty_cache()


def _frames(golden, n=2):
    g = golden("vit_h14")
    f = R.vit_frames(int(g["seed"]), n, 224)
    assert abs(float(f[:2].double().sum()) - float(g["frames_checksum"])) < 1e-6
    return f


@pytest.mark.parametrize("precision", ["f32", "auto", "f32x6"])
def test_vit_h14_golden(golden, h14, precision):
    g = golden("vit_h14")
    h14.precision, h14.chunk = precision, 512
    out = h14(_frames(golden).to(DEV))
    e = relerr(out, g["out"])
    print(f"ViT-H-14 {precision}: rel err vs the reference {e:.3e}, element excess {R.elem_excess(out, g['out']):.3f}")
    assert out.shape == (2, 1024) and e < TOL and elem_ok(out, g["out"])
    if precision == "auto":
        assert h14.ln16_resolution() is None                              # six bf16-plane products everywhere: the width gate


LAUNCH_SIZES = (8, 40)                       # 8 frames: the plane route's threshold (2056 token rows)
_GOLDEN_ROWS = {}                            # (precision, nframes) -> the two golden frames' rows of that launch: shared by the tests below


def _launch(golden, h14, nframes):
    base = _frames(golden)
    extra = torch.randn(6, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    eight = torch.cat([base, extra], 0)
    idx = torch.arange(nframes) % 8
    idx[-4:] = torch.tensor([1, 5, 0, 1])                                  # break the period near the tail rows
    return eight[idx].to(DEV), idx


@pytest.mark.parametrize("nframes", LAUNCH_SIZES)
def test_vit_h14_launch_sizes(golden, h14, nframes):
    """8 and 40 frames, the golden frames at several places of the launch: within one precision identical frames give bit-identical
    rows wherever they sit; the golden rows meet the reference bound; auto (= f32x6, bit for bit) is within
    test_vit_b16_launch_sizes_auto's distance of f32 (5e-6 of the largest feature, element-wise by recipes.elem_excess)."""
    g = golden("vit_h14")
    x, idx = _launch(golden, h14, nframes)
    outs = {}
    for precision in ("f32", "auto", "f32x6"):
        h14.precision, h14.chunk = precision, nframes
        out = outs[precision] = h14(x)
        assert out.shape == (nframes, 1024) and bool(torch.isfinite(out).all())
        for k in range(8):
            rows = out[idx.to(DEV) == k]
            assert torch.equal(rows, rows[:1].expand_as(rows)), (precision, k)
        first = [int((idx == k).nonzero()[0]) for k in (0, 1)]
        assert relerr(out[first], g["out"]) < TOL and elem_ok(out[first], g["out"]), precision
        _GOLDEN_ROWS[(precision, nframes)] = out[first].clone()
    assert torch.equal(outs["auto"], outs["f32x6"])
    e = relerr(outs["auto"], outs["f32"])
    print(f"ViT-H-14 auto vs f32 at {nframes} frames: {e:.3e}")
    assert e < 5e-6 and elem_ok(outs["auto"], outs["f32"])
    h14.chunk = 512


@pytest.mark.parametrize("precision", ["f32", "auto", "f32x6"])
def test_vit_h14_golden_rows_do_not_depend_on_the_launch_size(golden, h14, precision):
    """the golden rows of the 8-frame and of the 40-frame launch are the same bits within one precision.  (The 2-frame launch of
    test_vit_h14_golden is not part of the comparison: below the plane route's threshold auto / f32x6 run the f32 kernels.)"""
    rows = []
    for nframes in LAUNCH_SIZES:
        if (precision, nframes) not in _GOLDEN_ROWS:                         # (run on its own: the launch of test_vit_h14_launch_sizes)
            x, idx = _launch(golden, h14, nframes)
            h14.precision, h14.chunk = precision, nframes
            _GOLDEN_ROWS[(precision, nframes)] = h14(x)[[int((idx == k).nonzero()[0]) for k in (0, 1)]].clone()
            h14.chunk = 512
        rows.append(_GOLDEN_ROWS[(precision, nframes)])
    diff = (rows[0].double() - rows[1].double()).abs()
    print(f"ViT-H-14 {precision}: 8- vs 40-frame launch: {int((diff > 0).sum())} of {diff.numel()} elements differ, max {float(diff.max()):.3e} "
          f"({float(diff.max() / rows[0].abs().max()):.3e} of the largest feature)")
    assert torch.equal(rows[0], rows[1]), precision


def test_vit_h14_refuses_a_precision_switched_after_construction(h14):
    for precision in ("bf16", "f16x3s"):
        h14.precision = precision
        with pytest.raises(ValueError, match=ARCH):
            h14(torch.zeros(1, 3, 224, 224, device=DEV))
    h14.precision = "f32"


# =============================================================================================================== the model
def _net(prompts_table, seed, **kw):
    toks = torch.tensor(prompts_table["ucf"]["tokenized_prompts"], dtype=torch.int32)
    hc = IW.HeadConfig(emb_size=256, heads=8, depth=1)
    with torch.device(DEV):
        net = AnomalyCLIP(arch=ARCH, labels_key="ucf", emb_size=hc.emb_size, depth=hc.depth, heads=hc.heads, dim_heads=None,
                          num_segments=2, seg_length=16, concat_features=False, normal_id=7, stride=1,
                          select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=2, num_bottomk=2,
                          n_ctx=8, shared_context=False, ctx_init="", tokenized_prompts=toks.to(DEV), **kw)
    hc = IW.HeadConfig(emb_size=256, heads=8, depth=1, num_segments=2, seg_length=16)
    sd = IW.init_anomalyclip_state_dict(IW.VIT_H14, hc, toks, seed, with_image_encoder=False)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    assert not unexpected and all(k.startswith("image_encoder.") for k in missing)
    return net.eval()


@pytest.fixture(scope="module")
def net14(prompts_table, golden):
    net = _net(prompts_table, int(golden("text_h14")["seed"]), load_from_features=False)
    yield net
    del net
    torch.cuda.empty_cache()


def test_text_tower_h14_golden(golden, net14):
    """the 24-layer text tower (width 1024, 16 heads of 64, exact GELU) against the reference's TextEncoder: test_text_tower_l14_golden's bound"""
    g = golden("text_h14")
    assert net14.act == "gelu" and net14.text_encoder.transformer.act == "gelu"
    with torch.no_grad():
        tf = net14.get_text_features()
    assert tf.shape == (14, 1024)
    assert relerr(tf, g["out"]) < TOL and elem_ok(tf, g["out"])
    with torch.no_grad():
        tf2 = net14.text_encoder(net14.prompt_learner(), net14.tokenized_prompts)
    assert relerr(tf2, g["out"]) < TOL and elem_ok(tf2, g["out"])


def test_anomalyclip_h14_frames_path_equals_features_path(net14, h14):
    """AnomalyCLIP(arch="ViT-H-14", emb_size=256) on a 2 x 16 grid, 32 frames in test mode: the encoder runs inside forward and gives
    bit-identically what encoding first and passing the features gives"""
    h14.precision = "auto"
    net14.image_encoder.load_state_dict(h14.state_dict(), strict=True)
    assert (net14.image_encoder.heads, net14.image_encoder.width, net14.image_encoder.act, net14.image_encoder.precision) == (16, 1280, "gelu", "auto")
    frames = torch.randn(1, 32, 3, 224, 224, generator=torch.Generator().manual_seed(3)).to(DEV)
    nc = (torch.randn(1024, generator=torch.Generator().manual_seed(4)) * 0.1).to(DEV)
    with torch.no_grad():
        net14.load_from_features = False
        sim_f, sc_f = net14(frames, torch.zeros(1000), nc, 1, True)
        feats = net14.image_encoder(frames.view(-1, 3, 224, 224)).view(1, 1, 32, 1024)
        net14.load_from_features = True
        sim_x, sc_x = net14(feats, torch.zeros(1000), nc, 1, True)
        net14.load_from_features = False
    assert torch.equal(sim_f, sim_x) and torch.equal(sc_f, sc_x) and bool(torch.isfinite(sc_f).all()) and sc_f.numel() == 32


def test_extract_arch_vit_h14(tmp_path, h14):
    """the steps of `python -m anomalyclip_amd.extract --arch ViT-H-14` on two folders of 16 frames: the parsed command line, the
    encoder it builds, the weights loaded by arch (from the module's encoder: a 2.5 GB file would add nothing), extract_dataset.
    The files are [16, 1024] and equal the encoder's rows bit for bit."""
    from PIL import Image
    root, out = tmp_path / "frames", tmp_path / "feats"
    rng = np.random.default_rng(7)
    for v in ("a", "b"):
        os.makedirs(root / v)
        for t in range(16):
            Image.fromarray(rng.integers(0, 256, (240, 320, 3), dtype=np.uint8)).save(str(root / v / f"{t:06d}.jpg"), quality=90)
    weights = tmp_path / "present.pt"
    weights.write_bytes(b"")
    a = X.parse_args(["--arch", ARCH, "--weights", str(weights), "--frames-root", str(root), "--out-root", str(out)])
    assert (a.arch, a.act, a.precision) == (ARCH, "gelu", "auto")
    with torch.device(DEV):
        enc = X.build_image_encoder(a.arch, a.precision, act=a.act)
    X.load_encoder_weights(enc, a.arch, {"image_encoder." + k: v for k, v in h14.state_dict().items()})
    enc = enc.eval()
    counts = X.extract_dataset(enc, None, str(root), str(out), a.ncrops, a.scale_size, a.overwrite)
    assert counts["written"] == 2 and counts["rows"] == 32
    for v in ("a", "b"):
        got = np.load(str(out / f"{v}.npy"), allow_pickle=False)
        dec = np.stack([np.asarray(Image.open(str(root / v / f"{t:06d}.jpg")).convert("RGB")) for t in range(16)])
        with torch.no_grad():
            want = enc(preprocess_crops(torch.from_numpy(dec).to(DEV), 224, None, 1).view(-1, 3, 224, 224)).cpu().numpy()
        assert got.shape == (16, 1024) and np.isfinite(got).all() and np.array_equal(got, want), v
    del enc
    torch.cuda.empty_cache()
