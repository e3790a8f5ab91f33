"""No device: precision "auto"'s widest mode (ACX_PREC_F32X6_R16: out-proj and c_proj on fp16 planes as well) where it needs no GPU -- the
weight-only gate and its two-step fall-back on synthetic weights, the fp64 bounds against rows built to reach them, the driver's plan
against ACX_PREC_F32X6_LN16's, and the register table of the kernels the mode adds."""
import math
import re

import pytest
import torch

from anomalyclip_amd import _build
from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops
from anomalyclip_amd.components import clip_vit as V

W = 768


def _blocks(n=3, seed=0, width=W):
    torch.manual_seed(seed)
    return [V.ResidualAttentionBlock(width, width // 64) for _ in range(n)]


def _fill(p, v):
    with torch.no_grad():
        p.fill_(v)


def _block_bound(b, which):
    ln, wt, bias = ((b.ln_1, b.attn.in_proj_weight[2 * W:], b.attn.in_proj_bias[2 * W:]) if which == 0 else
                    (b.ln_2, b.mlp.c_fc.weight, b.mlp.c_fc.bias))
    l1, l2 = V.r16_bounds(ln.weight, ln.bias, wt, bias)
    return float(torch.minimum(l1, l2).max())


def test_gate_default_weights_resolve_with_the_largest_scales():
    bl = _blocks()
    sc = V.r16_scales(bl, W)
    assert sc is not None and len(sc) == 6 and V.ln16_scales(bl, W) == [512.0] * 6
    for i, s in enumerate(sc):
        bound = _block_bound(bl[i // 2], i % 2)
        assert math.frexp(s)[0] == 0.5 and s * bound <= V.LN16_TARGET < 2 * s * bound, (i, s, bound)


def test_the_l2_bound_is_the_tighter_one_on_default_weights():
    b = _blocks(1)[0]
    for ln, wt, bias in ((b.ln_1, b.attn.in_proj_weight[2 * W:], b.attn.in_proj_bias[2 * W:]), (b.ln_2, b.mlp.c_fc.weight, b.mlp.c_fc.bias)):
        l1, l2 = V.r16_bounds(ln.weight, ln.bias, wt, bias)
        assert (l2 <= l1).all() and float(l1.max() / l2.max()) > 8.0


@pytest.mark.parametrize("what", ["out_proj", "c_proj"])
def test_new_refusals_fall_back_to_ln16_not_to_f32x6(what):
    pick = (lambda b: b.attn.out_proj.weight) if what == "out_proj" else (lambda b: b.mlp.c_proj.weight)
    for v, refused in ((32.5, True), (32.0, False), (float("nan"), True), (float("inf"), True)):
        bl = _blocks()
        _fill(pick(bl[1]).data[3, 5:6], v)
        assert (V.r16_scales(bl, W) is None) == refused, (what, v)
        assert V.ln16_scales(bl, W) == [512.0] * 6, (what, v)          # ... and LN16 still resolves


def test_an_ln16_refusal_refuses_both():
    bl = _blocks()
    _fill(bl[0].mlp.c_fc.weight.data[5, 7:8], 100.0)
    assert V.ln16_scales(bl, W) is None and V.r16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[2].ln_1.bias.data[3:4], float("nan"))
    assert V.ln16_scales(bl, W) is None and V.r16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[1].attn.in_proj_bias.data[2 * W + 4:2 * W + 5], 1e12)      # a V bias: the bound's scale falls below 2^-20
    assert V.ln16_scales(bl, W) is not None and V.r16_scales(bl, W) is None
    bl = _blocks()
    _fill(bl[1].mlp.c_fc.bias.data[4:5], float("nan"))
    assert V.ln16_scales(bl, W) is not None and V.r16_scales(bl, W) is None


def test_auto_resolves_in_two_steps():
    """every CLIP ViT geometry resolves to the wide mode on default weights (B/16: both residual products; the others, whose attention is
    not the planes attention: c_proj); a weight failing only the new conditions gives LN16, one failing LN16's gives f32x6"""
    for res, patch, width, want_out in ((224, 16, 768, True), (224, 32, 768, False), (224, 14, 1024, False)):
        vit = V.VisionTransformer(res, patch, width, 2, width // 64, 64)
        sc = vit.r16_resolution()
        assert sc is not None and len(sc) == 8 and sc == vit.r16_resolution()
        ln = vit.ln16_resolution()
        assert len(ln) == 4 and [sc[0], sc[1], sc[4], sc[5]] == ln
        rec = ops.transformer_plan(64, vit.tokens, width, width // 64, 2, prec=L.PREC_F32X6_R16, prune_last=True)[0]
        assert (rec["reserved"] == L.F16X2P) == want_out and rec["fc"]["c_dtype"] == L.F16X2P
    vit = V.VisionTransformer(224, 16, 768, 2, 12, 64)
    _fill(vit.transformer.resblocks[0].mlp.c_proj.weight[0, 0:1], 33.0)
    assert vit.r16_resolution() is None and vit.ln16_resolution() is not None
    _fill(vit.transformer.resblocks[0].mlp.c_fc.weight[0, 0:1], 33.0)
    assert vit.r16_resolution() is None and vit.ln16_resolution() is None
    for res, patch, width, layers in ((32, 16, 128, 2), (224, 16, 768, 1)):
        assert V.VisionTransformer(res, patch, width, layers, width // 64, 64).r16_resolution() is None


def test_bounds_hold_and_are_reached_on_small_blocks():
    """D = 64, gamma spanning 2^-12 ... 2^3 with random signs: for 1,000 random rows and for the rows built to maximise one output
    (z proportional to the centred W_j o gamma, ||z||_2 = sqrt(D)) the fp64 V and c_fc pre-activations stay below both bounds; the
    maximising rows reach at least half of the L2 bound -- the bound is tested, not merely obeyed."""
    D = 64
    g = torch.Generator().manual_seed(77)
    for trial in range(4):
        gamma = (torch.exp2(torch.randint(-12, 4, (D,), generator=g).double()) * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0))
        beta = 0.5 * torch.randn(D, generator=g).double()
        for N in (D, 4 * D):                                             # the V rows of the in-projection, c_fc
            w = torch.randn(N, D, generator=g).double() * D ** -0.5
            b = torch.randn(N, generator=g).double() * 0.3
            l1, l2 = V.r16_bounds(gamma, beta, w, b)
            bound = torch.minimum(l1, l2)

            def pre(x):
                y = torch.nn.functional.layer_norm(x, (D,), gamma, beta, 1e-5)
                return y @ w.t() + b
            x = torch.randn(1000, D, generator=g).double() * torch.exp2(torch.randint(-6, 7, (1000, 1), generator=g).double())
            assert (pre(x).abs() <= bound).all()
            # row j: z = +- sqrt(D) c / ||c||, c the centred W_j o gamma (LayerNorm removes the mean: only the centred part acts); scaled
            # up so that eps does not matter; the sign that adds to the constant term
            c = w * gamma
            c = c - c.mean(1, keepdim=True)
            sign = torch.where((w @ beta + b) >= 0, 1.0, -1.0).double()
            xs = 1e3 * sign[:, None] * c / c.norm(dim=1, keepdim=True)
            got = pre(xs).abs().diagonal()
            assert (got <= bound * (1 + 1e-12)).all()
            assert (got >= 0.5 * l2).all(), (trial, N, float((got / l2).min()))


def _flat(rec):
    out = {}
    for k, v in rec.items():
        if isinstance(v, dict):
            out.update({f"{k}.{kk}": vv for kk, vv in v.items()})
        else:
            out[k] = v
    return out


def _grid():
    import test_cpu_vit_plan as P                                         # the grid of that test, at this precision
    seen = set()
    for case in P.GRID:
        batch, Ltok, width, heads, layers, causal, _prec, prune, planes, sized = case[1:]
        key = (batch, Ltok, width, heads, layers, causal, prune, planes, sized)
        if key not in seen:
            seen.add(key)
            yield key


def test_plan_equals_ln16_but_for_the_two_new_formats():
    """acx_transformer_plan(ACX_PREC_F32X6_R16) is ACX_PREC_F32X6_LN16's plan record for record over the grid of tests/test_cpu_vit_plan.py;
    the only fields that differ are fc.c_dtype = ACX_F16X2P where c_fc and c_proj are plane products of a body layer, and the
    attention-output word (= ACX_F16X2P) where the attention is acx_attention_p3f.  Other widths are refused as LN16 refuses them."""
    seen = {"out": 0, "proj": 0, "same": 0, "refused": 0}
    for batch, Ltok, width, heads, layers, causal, prune, planes, sized in _grid():
        args = (batch, Ltok, width, heads, layers)
        kw = dict(causal=bool(causal), prune_last=bool(prune), has_weight_planes=bool(planes), workspace_is_prec_sized=bool(sized))
        try:
            ln = ops.transformer_plan(*args, prec=L.PREC_F32X6_LN16, **kw)
        except L.AcxError as e:
            with pytest.raises(L.AcxError) as e2:
                ops.transformer_plan(*args, prec=L.PREC_F32X6_R16, **kw)
            assert str(e2.value).replace("ACX_PREC_F32X6_R16", "ACX_PREC_F32X6_LN16") == str(e), (args, kw)
            seen["refused"] += 1
            continue
        wide = ops.transformer_plan(*args, prec=L.PREC_F32X6_R16, **kw)
        assert len(ln) == len(wide) == layers
        for rl, rw in zip(ln, wide):
            fl, fw = _flat(rl), _flat(rw)
            want = dict(fl)
            if fl["att"] == L.TF_ATT_P3F:
                want["reserved"] = L.F16X2P
                seen["out"] += 1
            if not fl["pruned"] and fl["fc.kernel"] == L.TF_GEMM_X6 and fl["proj.kernel"] == L.TF_GEMM_X6 and fl["ln2_dtype"] == L.F16X2P:
                want["fc.c_dtype"] = L.F16X2P
                seen["proj"] += 1
            assert fw == want, (args, kw, fw, want)
            seen["same"] += fw == fl
    assert seen["out"] > 20 and seen["proj"] > 20 and seen["same"] > 20 and seen["refused"] > 0, seen
    body = ops.transformer_plan(512, 197, W, 12, 12, prec=L.PREC_F32X6_R16, prune_last=True)[1]
    assert (body["att"], body["reserved"], body["fc"]["c_dtype"], body["ln1_dtype"], body["ln2_dtype"]) == \
        (L.TF_ATT_P3F, L.F16X2P, L.F16X2P, L.F16X2P, L.F16X2P)
    assert body["out_proj"]["ln_job"] == 1 and body["proj"]["ln_job"] == 1 and body["ln2"] == L.TF_LN_RIDDEN
    with pytest.raises(L.AcxError, match="ACX_PREC_F32X6_R16 is built for widths 768 and 1024"):
        ops.transformer_plan(64, 257, 512, 8, 4, prec=L.PREC_F32X6_R16, prune_last=True)


def test_r16_kernel_registers():
    """gemm_x6_r16_kernel -- scaled fp16 output planes (with and without QuickGELU) and the LayerNorm riders on fp16 operands, whole tiles
    and both strips: the accumulators are the AGPRs (64 NI, as the twins in gemm_x6_p4_kernel), no scratch, no spills, the whole tile at
    one wave per SIMD.  attn_p3_o16_kernel (the attention's fp16-output arm) keeps occupancy 2 under __launch_bounds__(512, 2), as its bf16-output twin
    does, without scratch."""
    L.lib()
    rows = _build.kernel_resources()
    r16, p4, att = {}, {}, {}
    for k, v in rows.items():
        for name, dst in (("gemm_x6_r16_kernel", r16), ("gemm_x6_p4_kernel", p4), ("attn_p3_kernel", att)):
            if name + "I" in k:
                dst[tuple(int(x) for x in re.findall(r"Li(\d+)E", k.split(name + "I")[1]))] = v
        if "attn_p3_o16_kernel" in k:
            att["o16"] = v
    want = [(2, act, 0, 0, 0, 0, ni, 0, 2, 0) for act in (0, 1) for ni in (1, 2, 4)] + [(0, 0, 1, 0, 0, 0, ni, 0, 2, 1) for ni in (1, 2, 4)]
    assert sorted(r16) == sorted(want), sorted(r16)
    for t, v in r16.items():
        twin = p4[t[:9] + (0,)]
        assert v["AGPRs"] == 64 * t[6] == twin["AGPRs"], (t, v)
        assert v["ScratchSize [bytes/lane]"] == 0 and v["VGPRs Spill"] == 0, (t, v)
        if t[9] == 0:                      # (a rider instantiation also holds ln_ride_rows' registers; 144 KB of LDS: one workgroup per CU anyway)
            assert v["Occupancy [waves/SIMD]"] == twin["Occupancy [waves/SIMD]"], (t, v)
    new, old = att["o16"], att[(6, 0, 1)]
    assert new["ScratchSize [bytes/lane]"] == 0 and new["VGPRs Spill"] == 0
    assert new["Occupancy [waves/SIMD]"] == old["Occupancy [waves/SIMD]"] == 2, (new, old)
    assert new["VGPRs"] + new["AGPRs"] <= 256, new                         # eight waves of a workgroup, two to a SIMD: 256 registers a lane
