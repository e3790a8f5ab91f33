"""-m gpu: acx_gemm_ln -- a residual bf16 x 6 product whose partly filled last round of tiles carries LayerNorm rows on the workgroups
that have no tile (acx_gemm_x6.h, RIDE) -- gives the bits of acx_gemm followed by acx_layernorm: on x and on all three planes, at
kernel level over the shapes of the ViT launches and at model level with the switch on and off."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components.clip_vit import VisionTransformer
import recipes as R

DEV = "cuda"

# (name, M, N, K, rides): the bench shape's two residual products, a 256-frame launch (strip tail), ViT-L/14 (257-token rows, N = 1024;
# M not a multiple of 256), a tile count that is an exact multiple of the CU count, fewer tiles than CUs, an edge tile at N = 768
CASES = [("bench out-proj", 512 * 197, 768, 768, True), ("bench c_proj", 512 * 197, 768, 3072, True),
         ("256 frames", 256 * 197, 768, 768, True), ("ViT-L/14", 300 * 257, 1024, 1024, True),
         ("exact rounds", 256 * 256, 768, 768, False), ("few tiles", 2048, 768, 768, False),
         ("edge tile", 100000, 768, 768, True)]


def _operands(M, N, K):
    g = torch.Generator(device=DEV).manual_seed(M + N + K)
    a = torch.randn(M, K, generator=g, device=DEV) * torch.exp2(torch.randint(-4, 4, (M, 1), generator=g, device=DEV).float())
    w = torch.randn(N, K, generator=g, device=DEV) * 0.05
    bias = torch.randn(N, generator=g, device=DEV)
    x = torch.randn(M, N, generator=g, device=DEV) * 3.0
    lw, lb = torch.randn(N, generator=g, device=DEV), torch.randn(N, generator=g, device=DEV)
    return ops.split_bf16x3(a, panel=True), ops.split_bf16x3(w, panel=True), bias, x, lw, lb


@pytest.mark.parametrize("name,M,N,K,rides", CASES, ids=[c[0] for c in CASES])
def test_gemm_ln_bit_identical(name, M, N, K, rides):
    """The riding entry against acx_gemm followed by acx_layernorm, residual IN PLACE (x is the product's residual and its output):
    torch.equal on x and on each of the three planes -- with the rows the cost model picks, with every completed row forced to
    ride, and with the switch off.  Where N == K the LayerNorm's planes are written INTO the product's A planes, as ln_2 does
    behind out-proj in the ViT (the riders write plane rows the last round's tiles do not read)."""
    dev = torch.cuda.current_device()
    ncu = ops.x6_workgroups(dev)
    a3, w3, bias, x, lw, lb = _operands(M, N, K)
    ride, ready = ops.ln_rider_plan(M, N, K, ncu)
    print(f"{name}: {M} x {N} x {K} on {ncu} workgroups: {ride} of {ready} completed rows ride")
    if ncu == 256:
        assert (ride > 0) == rides and (ready > 0) == rides, (name, ride, ready)
    x_ref = x.clone()
    ops.gemm_x6(a3, w3, panels=3, bias=bias, residual=x_ref, out=x_ref)
    y_ref = ops.layernorm(x_ref, lw, lb, planes_out=True, panel_out=True)
    try:
        for mode in (1, 10 ** 9, 0):
            ops.set_ln_rider(dev, mode)
            x2 = x.clone()
            alias = N == K
            y2 = a3.clone() if alias else torch.full((3, M, N), 7.0, dtype=torch.bfloat16, device=DEV)
            ops.gemm_x6(y2 if alias else a3, w3, panels=3, bias=bias, residual=x2, out=x2, ln=(lw, lb, y2))
            assert torch.equal(x2, x_ref), (name, mode, "x")
            for p, pl in enumerate(("hi", "mid", "lo")):
                assert torch.equal(y2[p], y_ref[p]), (name, mode, pl, int((y2[p] != y_ref[p]).any(1).nonzero()[0]))
    finally:
        ops.set_ln_rider(dev, 1)


def _vit(seed):
    geom = IW.VIT_B16
    vit = VisionTransformer(geom.image_resolution, geom.vision_patch_size, geom.vision_width, geom.vision_layers,
                            geom.vision_heads, geom.embed_dim, precision="auto")
    vit.load_state_dict(IW.init_vit_state_dict(geom, seed, prefix=""), strict=True)
    return vit.to(DEV)


@pytest.mark.parametrize("frames", [3, 256, 512])
def test_vit_features_equal_with_rider_on_and_off(golden, frames):
    """acx_vit_encode (ViT-B/16, the default precision) with ACX_OPT_LN_RIDER on and off: the features of a 3-, 256- and 512-frame
    launch are equal bit for bit."""
    g = golden("vit_b16")
    dev = torch.cuda.current_device()
    vit = _vit(int(g["seed"]))
    vit.chunk = frames
    base = R.vit_frames(int(g["seed"]), 2, 224)
    extra = torch.randn(6, 3, 224, 224, generator=torch.Generator().manual_seed(5))
    x = torch.cat([base, extra], 0)[torch.arange(frames) % 8].to(DEV)
    try:
        ops.set_ln_rider(dev, 1)
        on = vit(x).clone()
        ops.set_ln_rider(dev, 0)
        off = vit(x).clone()
    finally:
        ops.set_ln_rider(dev, 1)
    assert on.shape == (frames, 512) and torch.isfinite(on).all()
    assert torch.equal(on, off), (frames, int((on != off).any(1).sum()))
