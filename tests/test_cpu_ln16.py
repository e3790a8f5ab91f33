"""No device: precision "auto"'s mixed mode (ACX_PREC_F32X6_LN16: the ViT's LayerNorm-fed products on fp16 planes) where it needs no
GPU -- the weight-only gate on synthetic weights, the driver's plan against ACX_PREC_F32X6's, and the register table of the kernel that
writes c_fc's bf16 planes from fp16 operands (gemm_x6_h3_kernel)."""
import math
import re

import pytest
import torch

from anomalyclip_amd import _build
from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops
from anomalyclip_amd.components import clip_vit as V

W = 768


def _blocks(n=3, seed=0):
    torch.manual_seed(seed)
    return [V.ResidualAttentionBlock(W, W // 64) for _ in range(n)]


def _fill(p, v):
    with torch.no_grad():
        p.fill_(v)


def test_gate_default_weights_resolve():
    """gamma = 1, beta = 0: bound = sqrt(767) = 27.7, the largest power of two s with 27.7 s <= 2^14 is 512"""
    sc = V.ln16_scales(_blocks(), W)
    assert sc == [512.0] * 6
    assert all(s * math.sqrt(W - 1) <= V.LN16_TARGET < 2 * s * math.sqrt(W - 1) for s in sc)


def test_gate_large_gamma_resolves_with_smaller_scale():
    bl = _blocks()
    _fill(bl[1].ln_2.weight.data, 1e4)
    sc = V.ln16_scales(bl, W)
    assert sc is not None and sc[3] < 512.0 and sc[:3] + sc[4:] == [512.0] * 5
    bound = 1e4 * math.sqrt(W - 1)
    assert sc[3] * bound <= V.LN16_TARGET < 2 * sc[3] * bound and math.frexp(sc[3])[0] == 0.5


def test_gate_refusals():
    bl = _blocks()
    _fill(bl[0].mlp.c_fc.weight.data[5, 7:8], 100.0)               # 2^10 * 100 > 2^15
    assert V.ln16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[2].attn.in_proj_weight.data[0, 0:1], 32.5)
    assert V.ln16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[2].attn.in_proj_weight.data[0, 0:1], 32.0)            # 2^10 * 32 == 2^15: still inside
    assert V.ln16_scales(bl, W) is not None
    bl = _blocks()
    _fill(bl[1].ln_1.bias.data[3:4], float("nan"))
    assert V.ln16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[1].ln_1.weight.data[3:4], float("inf"))
    assert V.ln16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[0].mlp.c_fc.weight.data[0, 0:1], float("nan"))
    assert V.ln16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[0].ln_2.weight.data, 0.0)                             # gamma = 0 everywhere (beta = 0): the bound is not > 0
    assert V.ln16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[0].ln_2.weight.data, 1e-12)                           # a scale above 2^20
    assert V.ln16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[0].ln_2.bias.data, 1e12)                              # ... below 2^-20
    assert V.ln16_scales(bl, W) is None


def test_scale_is_the_largest_power_of_two():
    for bound in (0.02, 0.5, 1.0, 27.69, 2.0 ** 14, 2.0 ** 14 * (1 + 2 ** -20), 12345.678, 3e9):
        s = V.ln16_scale(bound)
        assert s is not None and math.frexp(s)[0] == 0.5 and s * bound <= V.LN16_TARGET < 2 * s * bound, (bound, s)
    for bad in (0.0, -1.0, float("nan"), float("inf"), 1e-30, 1e-3, 1e30):        # (1e-3: s = 2^23, 1e30: s far below 2^-20)
        assert V.ln16_scale(bad) is None


def test_auto_resolves_on_the_clip_vit_widths():
    """every CLIP ViT width (768: B/16, B/32; 1024: L/14, L/14@336px) resolves the same way; a width the fp16 LayerNorm store is not
    built for (the test geometry) and a one-layer model (its only layer is the pruned one) stay f32x6"""
    for res, patch, width, layers, want in ((224, 16, 768, 2, True), (224, 32, 768, 2, True), (224, 14, 1024, 2, True),
                                            (336, 14, 1024, 2, True), (32, 16, 128, 2, False), (224, 16, 768, 1, False)):
        vit = V.VisionTransformer(res, patch, width, layers, width // 64, 64)
        sc = vit.ln16_resolution()
        assert (sc is not None) == want, (res, patch, width, layers)
        if want:
            assert len(sc) == 2 * layers and sc == vit.ln16_resolution()          # (cached with the weights)
            s = V.ln16_scale(math.sqrt(width - 1))
            assert sc == [s] * (2 * layers)


GRID = [(b, Ltok, width, layers, prune) for b in (1, 2, 4, 7, 8, 16, 64, 512) for Ltok, width in ((50, 768), (193, 768), (197, 768), (208, 768),
                                                                                                 (209, 768), (257, 1024), (577, 1024))
        for layers in (1, 2, 12) for prune in (0, 1)]


def _flat(rec):
    out = {}
    for k, v in rec.items():
        if isinstance(v, dict):
            out.update({f"{k}.{kk}": vv for kk, vv in v.items()})
        else:
            out[k] = v
    return out


def test_plan_equals_f32x6_but_for_the_layernorm_dtypes():
    """acx_transformer_plan(ACX_PREC_F32X6_LN16) is ACX_PREC_F32X6's plan record for record; the only fields that differ are ln1_dtype /
    ln2_dtype = ACX_F16X2P where the in-projection / c_fc of that layer is a plane product.  A geometry that sends neither to the
    plane kernel has equal plans.  The bench shape: launch for launch the same records (same counts)."""
    seen = {"mixed": 0, "same": 0}
    for b, Ltok, width, layers, prune in GRID:
        six = ops.transformer_plan(b, Ltok, width, width // 64, layers, prec=L.PREC_F32X6, prune_last=bool(prune))
        mix = ops.transformer_plan(b, Ltok, width, width // 64, layers, prec=L.PREC_F32X6_LN16, prune_last=bool(prune))
        assert len(six) == len(mix) == layers
        any_diff = False
        for r6, rm in zip(six, mix):
            f6, fm = _flat(r6), _flat(rm)
            want = dict(f6)
            if f6["in_proj.kernel"] == L.TF_GEMM_X6:
                want["ln1_dtype"] = L.F16X2P
            if f6["fc.kernel"] == L.TF_GEMM_X6 and not f6["pruned"]:
                want["ln2_dtype"] = L.F16X2P
            assert fm == want, (b, Ltok, width, layers, prune, fm, want)
            assert fm["reserved"] == 0
            any_diff |= fm != f6
        seen["mixed" if any_diff else "same"] += 1
    assert seen["mixed"] > 50 and seen["same"] > 50, seen
    body = ops.transformer_plan(512, 197, W, 12, 12, prec=L.PREC_F32X6_LN16, prune_last=True)[1]
    assert (body["ln1"], body["ln1_dtype"], body["ln2"], body["ln2_dtype"]) == (L.TF_LN_RIDDEN, L.F16X2P, L.TF_LN_RIDDEN, L.F16X2P)
    assert body["in_proj"]["c_dtype"] == L.ACX_F32 and body["fc"]["c_dtype"] == L.BF16X3P and body["att"] == L.TF_ATT_P3F


def test_plan_refuses_other_widths():
    with pytest.raises(L.AcxError, match="ACX_PREC_F32X6_LN16 is built for widths 768 and 1024"):
        ops.transformer_plan(64, 257, 512, 8, 4, prec=L.PREC_F32X6_LN16, prune_last=True)


def test_h3_kernel_registers():
    """gemm_x6_h3_kernel (fp16 operand planes, three products, bf16 x 3 output planes; with and without QuickGELU; whole tiles and the
    128- / 64-column strips): the accumulators are the AGPRs -- 256 for the whole tile, 64 NI for a strip, as the fp16-output twin of
    gemm_x6_p4_kernel -- one workgroup per CU (144 KB of LDS; whole tile and 128-column strip: one wave per SIMD by registers too), no
    scratch, no spills."""
    L.lib()
    rows = _build.kernel_resources()
    h3, p4 = {}, {}
    for k, v in rows.items():
        for name, dst in (("gemm_x6_h3_kernel", h3), ("gemm_x6_p4_kernel", p4)):
            if name in k:
                dst[tuple(int(x) for x in re.findall(r"Li(\d+)E", k.split(name + "I")[1]))] = v
    assert sorted(h3) == [(2, act, 0, 0, 0, 0, ni, 0, 2, 0) for act in (0, 1) for ni in (1, 2, 4)], sorted(h3)
    for t, v in h3.items():
        ni = t[6]
        assert v["AGPRs"] == 64 * ni == p4[t]["AGPRs"], (t, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (t, v)
        assert v["Occupancy [waves/SIMD]"] == p4[t]["Occupancy [waves/SIMD]"], (t, v)
        if ni == 4:
            assert v["AGPRs"] == 256 and v["Occupancy [waves/SIMD]"] == 1, (t, v)
