"""-m gpu: the plane-reuse product (acx_gemm_x6.h) on 16 x 16 x 32 MFMAs -- the operand map of its fragments (every position of a
K-step, a tile and a strip, named when wrong) and the ViT-B/16 products of a 512-frame clip against fp64."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

DEV = "cuda"


def _first_bad(y, ref):
    bad = (y != ref).nonzero()
    return None if bad.numel() == 0 else (tuple(int(v) for v in bad[0]), float(y[tuple(bad[0])]), float(ref[tuple(bad[0])]), int(bad.shape[0]))


def _variants(a, w, ref, tag, **kw):
    """every route of one product: f32, bf16 (skipped when the values need more than 8 bits), planes row-major / K-panel, operand
    planes row-major / K-panel; all must equal `ref` exactly"""
    a3, w3 = ops.split_bf16x3(a), ops.split_bf16x3(w)
    conv = "amap" in kw
    y = ops.gemm_x6(a3, w3, **kw)
    assert torch.equal(y, ref), (tag, "f32", _first_bad(y, ref))
    if ref.shape[1] % 8 == 0:
        yp = ops.gemm_x6(a3, w3, planes_out=True, **kw).float().sum(0)
        assert torch.equal(yp, ref), (tag, "planes", _first_bad(yp, ref))
    if not conv and a.shape[1] % 32 == 0 and ref.shape[1] % 32 == 0:
        a3p, w3p = ops.split_bf16x3(a, panel=True), ops.split_bf16x3(w, panel=True)
        y = ops.gemm_x6(a3p, w3p, panels=3, **kw)
        assert torch.equal(y, ref), (tag, "panel operands", _first_bad(y, ref))
        y = ops.gemm_x6(a3, w3p, panels=2, **kw)
        assert torch.equal(y, ref), (tag, "panel W", _first_bad(y, ref))
        ypp = ops.unpanel(ops.gemm_x6(a3p, w3p, panels=3, planes_out=True, panel_out=True, **kw)).float().sum(0)
        assert torch.equal(ypp, ref), (tag, "panel planes out", _first_bad(ypp, ref))


@pytest.mark.parametrize("strip", [0, 2, 3])
@pytest.mark.parametrize("M,N,K,split", [(512, 256, 64, False), (300, 512, 96, False), (512, 256, 2304, True), (256, 256, 2304, False)])
def test_x6_operand_map_one_hot(M, N, K, split, strip):
    """One-hot operands select single entries of the other operand, which must come out EXACTLY (x = hi + mid + lo is exact, every
    other product is with zero): A one-hot / W distinct per (n, k) walks the W.lo / W.mid / W.hi fragments against A.hi, W one-hot /
    A distinct per (m, k) the A.hi / A.mid / A.lo fragments against W.hi -- for every k position of a 32-wide K-step (the one-hot
    position moves through all of them), every row and column of a tile, whole tiles and 128- / 64-column strips (NI = 4 / 2 / 1),
    K split on and off, row-major and K-panel planes on both sides.  A swapped pair of 16-byte chunks or of row blocks reads wrong
    data without a fault; the assertion names the first wrong element."""
    dev = torch.device(DEV).index or 0
    m_i, n_i, k_i = torch.arange(M, device=DEV), torch.arange(N, device=DEV), torch.arange(K, device=DEV)
    wd = (n_i.view(-1, 1) * K + k_i.view(1, -1) + 1).float()             # distinct integers < 2^24: exact in three bf16 planes
    ad = (m_i.view(-1, 1) * K + k_i.view(1, -1) + 1).float()
    ops.set_x6_strip_tail(dev, strip)
    try:
        for s in range(32):
            kpos_m = (m_i * 5 + s + 32 * (m_i // 32)) % K               # every k position of a K-step at every row position over s
            a = torch.zeros(M, K, device=DEV)
            a[m_i, kpos_m] = 2.0
            _variants(a, wd, 2.0 * wd[:, kpos_m].t().contiguous(), ("A one-hot", s), split_k=split)
            kpos_n = (n_i * 3 + s + 32 * (n_i // 16)) % K
            w = torch.zeros(N, K, device=DEV)
            w[n_i, kpos_n] = 0.5
            _variants(ad, w, 0.5 * ad[:, kpos_n].contiguous(), ("W one-hot", s), split_k=split)
    finally:
        ops.set_x6_strip_tail(dev, 1)


@pytest.mark.parametrize("cout", [256, 128])
def test_x6_operand_map_conv_centre_tap(cout):
    """The implicit 3x3 convolution differs from the identity rows in the DMA source only: with weights in the CENTRE tap alone a
    one-hot channel per row selects single weights exactly (256-column tiles, and the 128-column tiles of narrow outputs)."""
    gn, gl, cin, tiles = 8, 4, 64, 16
    M, K = tiles * gn * gl, 9 * cin
    m_i, n_i, c_i = torch.arange(M, device=DEV), torch.arange(cout, device=DEV), torch.arange(cin, device=DEV)
    w = torch.zeros(cout, 9, cin, device=DEV)
    w[:, 4] = (n_i.view(-1, 1) * cin + c_i.view(1, -1) + 1).float()
    for s in range(32):
        cpos = (m_i * 5 + s + 32 * (m_i // 32)) % cin
        x = torch.zeros(M, cin, device=DEV)
        x[m_i, cpos] = 2.0
        ref = 2.0 * w[:, 4][:, cpos].t().contiguous()
        for split in (False, True):
            _variants(x, w.view(cout, K), ref, ("conv", cout, s, split), split_k=split, amap=L.AMAP_CONV3X3, gn=gn, gl=gl, cin=cin)


@pytest.mark.parametrize("name,N,K,act,res,planes", [("qkv", 2304, 768, 0, 0, 1), ("out", 768, 768, 0, 1, 0), ("fc", 3072, 768, 1, 0, 1),
                                                     ("proj", 768, 3072, 0, 1, 0)])
def test_x6_vit_shapes_512_frames_vs_fp64(name, N, K, act, res, planes):
    """The ViT-B/16 products of a 512-frame clip (M = 512 x 197 = 100,864 rows: 394 row tiles, strips in the last round) with the
    epilogues the ViT uses (residual in f32; QuickGELU and K-panel plane outputs), operands spanning 12 binades and a
    massive-activation column, against fp64 on the GPU: element-wise within 2e-6 x sum |a||w|, and the maximum error no worse than
    1.5 x the f32 MFMA kernel's on the same operands."""
    M = 512 * 197
    g = torch.Generator(device=DEV).manual_seed(N + K)
    a = torch.randn(M, K, generator=g, device=DEV) * torch.exp2(torch.randint(-6, 6, (M, 1), generator=g, device=DEV).float())
    a[:, 3] *= 60.0
    w = torch.randn(N, K, generator=g, device=DEV) * 0.05
    b = torch.randn(N, generator=g, device=DEV)
    x = torch.randn(M, N, generator=g, device=DEV) if res else None
    a3, w3 = ops.split_bf16x3(a, panel=True), ops.split_bf16x3(w, panel=True)
    kw = dict(bias=b, act=L.ACT_QUICKGELU if act else L.ACT_NONE, residual=x)
    if planes:
        y6 = ops.unpanel(ops.gemm_x6(a3, w3, panels=3, planes_out=True, panel_out=True, **kw)).float().sum(0)
    else:
        y6 = ops.gemm_x6(a3, w3, panels=3, **kw)
    y32 = ops.gemm(a, w, **kw)
    w64, wabs = w.double().t().contiguous(), w.double().abs().t().contiguous()
    worst, e6max, e32max = 0.0, 0.0, 0.0
    for r0 in range(0, M, 8192):                                       # (fp64 reference in row blocks: 8192 x N doubles at a time)
        sl = slice(r0, min(r0 + 8192, M))
        a64 = a[sl].double()
        pre = a64 @ w64 + b.double()
        ref = pre * torch.sigmoid(1.702 * pre) if act else pre
        if res:
            ref = ref + x[sl].double()
        bound = 2e-6 * (a64.abs() @ wabs + b.double().abs()) + 1e-30
        e6, e32 = (y6[sl].double() - ref).abs(), (y32[sl].double() - ref).abs()
        worst = max(worst, float((e6 / bound).max()))
        e6max, e32max = max(e6max, float(e6.max())), max(e32max, float(e32.max()))
    print(f"{name}: max err / bound {worst:.3f}; max |err| x6 {e6max:.3e}, f32 MFMA {e32max:.3e}")
    assert worst <= 1.0, (name, worst)
    assert e6max <= 1.5 * e32max + 1e-12, (name, e6max, e32max)
