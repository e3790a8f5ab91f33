"""-m gpu: acx_attention_cls_fold -- the CLS-row attention of the pruned last ViT layer without the K | V product -- against the fp64
reference of tests/cls_fold_ref.py, with the path it replaces (acx_layernorm -> f32 acx_gemm K | V -> acx_attention_cls) on the same
inputs as the yardstick; its independence of the batch; the ViT with ACX_OPT_CLS_FOLD on and off; argument errors."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.clip_vit import VisionTransformer
from oracle import anomalyclip_oracle as O
import cls_fold_ref as CF
import recipes as R

DEV = "cuda"


@functools.lru_cache(maxsize=None)
def _case(shape, col_scale=None, q_scale=None):
    """inputs and the fp64 reference of one case, computed once and never written to"""
    c = CF.make_inputs(*shape, col_scale=col_scale, q_scale=q_scale)
    return c, CF.straight(c)


def _fold(c, x=None, q=None, batch=None):
    d = {k: c[k].to(DEV) for k in ("ln_w", "ln_b", "in_w", "in_b")}
    x = c["x"].to(DEV) if x is None else x
    q = c["q"].to(DEV) if q is None else q
    return ops.attention_cls_fold(x, d["ln_w"], d["ln_b"], d["in_w"], d["in_b"], q, c["batch"] if batch is None else batch, c["L"], c["heads"])


def _old_path(c):
    """what the fold replaces: LayerNorm of every row, the f32 K | V product, acx_attention_cls"""
    B, L_, W, H = c["batch"], c["L"], c["W"], c["heads"]
    x, in_w, in_b = c["x"].to(DEV), c["in_w"].to(DEV), c["in_b"].to(DEV)
    y = ops.layernorm(x, c["ln_w"].to(DEV), c["ln_b"].to(DEV))
    kv = ops.gemm(y, in_w[W:].contiguous(), bias=in_b[W:].contiguous())
    qkv = torch.zeros(B * L_, 3 * W, device=DEV)
    qkv[:, W:] = kv
    qkv[::L_, :W] = c["q"].to(DEV)
    out = torch.empty(B, W, device=DEV)
    h = L.ctx(torch.cuda.current_device())
    L.check(L.lib().acx_attention_cls(h, qkv.data_ptr(), 3 * W, out.data_ptr(), W, B, L_, H, ops._stream()), h)
    return out


CASES = [(s, None, None) for s in CF.SHAPES] + [((3, 197, 768), 40.0, None), ((3, 197, 768), None, 20.0)]


@pytest.mark.parametrize("shape,col_scale,q_scale", CASES)
def test_fold_vs_fp64_no_worse_than_twice_the_path_it_replaces(shape, col_scale, q_scale):
    """max |out - ref| / max |ref| against the fp64 straightforward form: at most 2 x the error of acx_layernorm -> acx_gemm (f32) ->
    acx_attention_cls on the same inputs (the margin covers another summation order of the same f32 work).  One x column scaled by 40
    and scores spanning more than 80 included: finite results."""
    c, ref = _case(shape, col_scale, q_scale)
    scale = ref.abs().max().item()
    out = _fold(c)
    old = _old_path(c)
    e_fold = (out.double().cpu() - ref).abs().max().item() / scale
    e_old = (old.double().cpu() - ref).abs().max().item() / scale
    print(f"cls_fold {shape} col_scale={col_scale} q_scale={q_scale}: err/max|ref| fold {e_fold:.3e}  old path {e_old:.3e}")
    assert out.shape == (shape[0], shape[2]) and torch.isfinite(out).all()
    assert e_fold <= 2.0 * e_old, (e_fold, e_old)


def test_a_frame_does_not_depend_on_the_batch():
    """frame k alone == frame k at positions 0 and 4 of a batch of five (bit for bit); two calls give equal results"""
    c, _ = _case((5, 197, 768))
    L_, W = c["L"], c["W"]
    x, q = c["x"].to(DEV), c["q"].to(DEV)
    k = 2
    xk, qk = x[k * L_:(k + 1) * L_].contiguous(), q[k:k + 1].contiguous()
    alone = _fold(c, xk, qk, batch=1)
    x5, q5 = x.clone(), q.clone()
    for pos in (0, 4):
        x5[pos * L_:(pos + 1) * L_] = xk
        q5[pos] = qk[0]
    five = _fold(c, x5, q5)
    assert torch.equal(five[0:1], alone) and torch.equal(five[4:5], alone)
    assert torch.equal(_fold(c, x5, q5), five)
    assert torch.equal(_fold(c)[k:k + 1], alone)


def test_argument_errors_come_back_before_any_launch():
    c, _ = _case((3, 2, 128))
    d = {k: c[k].to(DEV) for k in ("x", "ln_w", "ln_b", "in_w", "in_b", "q")}
    out = torch.empty(3, 128, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    lib, h = L.lib(), L.ctx(torch.cuda.current_device())
    ptr = {k: v.data_ptr() for k, v in d.items()}

    def call(L_=2, W=128, heads=2, ws_bytes=ws.numel(), **nul):
        p = dict(ptr, out=out.data_ptr(), ws=ws.data_ptr())
        p.update(nul)
        return lib.acx_attention_cls_fold(h, p["x"], p["ln_w"], p["ln_b"], 1e-5, p["in_w"], p["in_b"], p["q"], 128, p["out"], 128, 3, L_, W,
                                          heads, p["ws"], ws_bytes, ops._stream())

    assert call() == 0
    for name in ("x", "ln_w", "ln_b", "in_w", "in_b", "q", "out", "ws"):
        assert call(**{name: None}) == -1, name                                   # ACX_E_BADARG
    assert call(L_=0) == -2 and call(L_=1025) == -2                               # ACX_E_UNSUPPORTED
    assert call(W=128, heads=3) == -2 and call(W=192, heads=2) == -2
    assert call(W=192, heads=3) == -2                                             # 64 heads, but no LayerNorm width
    assert call(ws_bytes=lib.acx_attention_cls_fold_workspace_bytes(3, 2) - 1) == -4   # ACX_E_WORKSPACE
    assert lib.acx_attention_cls_fold_workspace_bytes(3, 2) == 2 * 3 * 2 * 128 * 4
    torch.cuda.synchronize()


@functools.lru_cache(maxsize=None)
def _weights(name, seed):
    return IW.init_vit_state_dict(getattr(IW, name), seed, prefix="")


def _vit(name, precision, seed=3):
    geom = getattr(IW, name)
    vit = VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers,
                            geom.vision_heads, geom.embed_dim, precision=precision)
    vit.load_state_dict(_weights(name, seed), strict=True)
    return vit.to(DEV)


def _encode(vit, x, fold):
    dev = torch.cuda.current_device()
    vit.chunk = x.shape[0]
    before = ops.get_option(dev, L.OPT_CLS_FOLD)
    try:
        ops.set_cls_fold(dev, fold)
        out = vit(x).clone()
    finally:
        ops.set_cls_fold(dev, before)
    assert out.shape[0] == x.shape[0] and torch.isfinite(out).all()
    return out


def test_vit_b16_features_with_the_fold_on_and_off():
    """ViT-B/16, 8 frames (the smallest launch on the plane kernels), precisions "auto" and "f32": max |features(fold on) -
    features(fold off)| is at most 2 x max |auto - f32| of the same frames with the fold off -- two accepted f32-level paths."""
    x = R.vit_frames(3, 8, 224).to(DEV)
    off = {p: _encode(_vit("VIT_B16", p), x, False) for p in ("auto", "f32")}
    yard = (off["auto"] - off["f32"]).abs().max().item()
    assert yard > 0.0
    for p in ("auto", "f32"):
        d = (_encode(_vit("VIT_B16", p), x, True) - off[p]).abs().max().item()
        print(f"ViT-B/16 {p}: max |fold on - off| {d:.3e}   yardstick max |auto - f32| (fold off) {yard:.3e}")
        assert 0.0 < d <= 2.0 * yard, (p, d, yard)                                  # (0: the option did nothing)


def test_vit_tiny_features_with_the_fold_on_and_off():
    """The tiny geometry (5 tokens, width 128), "auto" and "f32".  Here the auto - f32 yardstick of the ViT-B/16 test is identically 0:
    width 128 never reaches the plane kernels, both precisions run the same launches (asserted).  The yardstick that exists at this
    geometry is the kernel-level one: against the fp64 evaluation of the same weights and frames, the features with the fold on
    may be at most 2 x as far off as the features with the fold off."""
    x = R.vit_frames(3, 8, 32)
    sd64 = {k: v.double() for k, v in _weights("TINY", 3).items()}
    ref = O.vit_forward(sd64, x.double(), prefix="")
    xd = x.to(DEV)
    off = {p: _encode(_vit("TINY", p), xd, False) for p in ("auto", "f32")}
    assert torch.equal(off["auto"], off["f32"])
    e_off = (off["f32"].double().cpu() - ref).abs().max().item()
    for p in ("auto", "f32"):
        on = _encode(_vit("TINY", p), xd, True)
        d, e_on = (on - off[p]).abs().max().item(), (on.double().cpu() - ref).abs().max().item()
        print(f"tiny {p}: max |fold on - off| {d:.3e}   error vs fp64: on {e_on:.3e} off {e_off:.3e}   max |ref| {ref.abs().max().item():.3e}")
        assert d > 0.0 and e_on <= 2.0 * e_off, (p, e_on, e_off)


@pytest.mark.parametrize("precision", ["f32", "auto"])
def test_vit_three_frames_equal_the_first_three_of_eight(precision):
    """with the fold on, a 3-frame encode equals rows 0..2 of an 8-frame encode of the same frames bit for bit.  The tiny geometry: 15
    and 40 rows both run every product on the few-row kernel, whose rows do not depend on the row count.  ViT-B/16 at 3 and 8 frames
    does not qualify: `generic_ksplit` (csrc/acx_gemm.hip) doubles the K split of an f32 product while tiles * split * 2 <= 512 and
    a piece keeps 4 K-steps, with tiles = ceil(M / 128) * ceil(N / 128) -- c_fc (N = 3072) is split in 2 at 591 rows (120 tiles) and
    not at all at 1576 rows (312 tiles), c_proj (N = 768, K = 3072) in 8 at 30 tiles and in 2 at 78: other summation orders.  The
    fold kernels' own independence of the batch at ViT-B/16's shape is test_a_frame_does_not_depend_on_the_batch."""
    x = R.vit_frames(5, 8, 32).to(DEV)
    vit = _vit("TINY", precision)
    eight, three = _encode(vit, x, True), _encode(vit, x[:3].contiguous(), True)
    assert torch.equal(three, eight[:3]), int((three != eight[:3]).any(1).sum())
