"""No device: precision "auto"'s third resolution step (ACX_PREC_F32X6_QKV16: q | k | v as fp16 planes into the three-product planes
attention) where it needs no GPU -- the weight-only gate and its three-step fall-back on synthetic weights, the fp64 bounds of the Q and K
rows against rows built to reach them, the driver's plan against ACX_PREC_F32X6_R16's, and the register table of the kernel the mode adds."""
import ctypes as C
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


def _qkv_bound(b):
    l1, l2 = V.r16_bounds(b.ln_1.weight, b.ln_1.bias, b.attn.in_proj_weight, b.attn.in_proj_bias)
    return float(torch.minimum(l1, l2).max())


def test_gate_default_weights_resolve_with_the_largest_scale():
    bl = _blocks()
    sq = V.qkv16_scales(bl, W)
    assert sq is not None and len(sq) == 3 and V.r16_scales(bl, W) is not None
    for b, s in zip(bl, sq):
        bound = _qkv_bound(b)
        assert math.frexp(s)[0] == 0.5 and s * bound <= V.LN16_TARGET < 2 * s * bound, (s, bound)
    # one scale for the three thirds: the bound is the largest of the thirds' bounds (the V third's is r16_scales')
    b = bl[0]
    thirds = []
    for t in range(3):
        l1, l2 = V.r16_bounds(b.ln_1.weight, b.ln_1.bias, b.attn.in_proj_weight[t * W:(t + 1) * W], b.attn.in_proj_bias[t * W:(t + 1) * W])
        thirds.append(float(torch.minimum(l1, l2).max()))
    assert _qkv_bound(b) == max(thirds) and sq[0] <= V.r16_scales(bl, W)[0]


def test_q_and_k_bounds_hold_and_are_reached_on_small_blocks():
    """test_cpu_r16.py::test_bounds_hold_and_are_reached_on_small_blocks' construction (D = 64, gamma spanning 2^-12 ... 2^3 with random
    signs) for the Q and K slices of a [3 D, D] in-projection: 1,000 random rows and the rows built to maximise one output stay below
    both bounds; the maximising rows reach at least half of the L2 bound."""
    D = 64
    g = torch.Generator().manual_seed(78)
    for trial in range(4):
        gamma = (torch.exp2(torch.randint(-12, 4, (D,), generator=g).double()) * torch.where(torch.rand(D, generator=g) < 0.5, -1.0, 1.0))
        beta = 0.5 * torch.randn(D, generator=g).double()
        w_in = torch.randn(3 * D, D, generator=g).double() * D ** -0.5
        b_in = torch.randn(3 * D, generator=g).double() * 0.3
        l1_all, l2_all = V.r16_bounds(gamma, beta, w_in, b_in)
        for t in (0, 1):                                                 # the Q rows, the K rows
            w, b = w_in[t * D:(t + 1) * D], b_in[t * D:(t + 1) * D]
            l1, l2 = V.r16_bounds(gamma, beta, w, b)
            assert torch.equal(l1, l1_all[t * D:(t + 1) * D]) and torch.equal(l2, l2_all[t * D:(t + 1) * D])   # the same function on a slice
            bound = torch.minimum(l1, l2)

            def pre(x):
                y = torch.nn.functional.layer_norm(x, (D,), gamma, beta, 1e-5)
                return y @ w.t() + b
            x = torch.randn(1000, D, generator=g).double() * torch.exp2(torch.randint(-6, 7, (1000, 1), generator=g).double())
            assert (pre(x).abs() <= bound).all()
            c = w * gamma
            c = c - c.mean(1, keepdim=True)
            sign = torch.where((w @ beta + b) >= 0, 1.0, -1.0).double()
            xs = 1e3 * sign[:, None] * c / c.norm(dim=1, keepdim=True)
            got = pre(xs).abs().diagonal()
            assert (got <= bound * (1 + 1e-12)).all()
            assert (got >= 0.5 * l2).all(), (trial, t, float((got / l2).min()))


def test_gate_refuses_on_q_and_k_rows_only_then_r16_resolves():
    for where, v in ((5, 1e12), (W + 4, float("nan")), (W + 4, 1e12), (7, float("inf"))):   # a Q bias, a K bias: the V rows are left alone
        bl = _blocks()
        _fill(bl[1].attn.in_proj_bias.data[where:where + 1], v)
        assert V.qkv16_scales(bl, W) is None, (where, v)
        assert V.r16_scales(bl, W) is not None and V.ln16_scales(bl, W) == [512.0] * 6, (where, v)
    bl = _blocks()
    _fill(bl[1].mlp.c_proj.weight.data[3, 5:6], 33.0)                     # an R16 refusal refuses the new step too
    assert V.qkv16_scales(bl, W) is None and V.r16_scales(bl, W) is None and V.ln16_scales(bl, W) is not None
    bl = _blocks()
    _fill(bl[0].mlp.c_fc.weight.data[5, 7:8], 100.0)                      # ... and so does an LN16 refusal
    assert V.qkv16_scales(bl, W) is None and V.r16_scales(bl, W) is None and V.ln16_scales(bl, W) is None


def test_auto_resolves_in_three_steps():
    """ViT-B/16 on default weights resolves to the new mode, its scales R16's with s_qkv appended per layer; failing only the new
    condition gives R16, an R16 failure LN16, an LN16 failure f32x6.  Geometries whose attention is not the planes attention (B/32, L/14)
    and the ones R16 does not take stay where they were."""
    vit = V.VisionTransformer(224, 16, 768, 2, 12, 64)
    s5, s4 = vit.qkv16_resolution(), vit.r16_resolution()
    assert s5 is not None and len(s5) == 10 and s5 == vit.qkv16_resolution() and len(s4) == 8
    assert [s5[0:4], s5[5:9]] == [s4[0:4], s4[4:8]]
    assert [s5[4], s5[9]] == V.qkv16_scales(vit.transformer.resblocks, 768)
    rep = vit.f16x3_range_report()
    assert set(rep["qkv"]) == {"q", "k", "v"} and all(v > 0 for v in rep["qkv"].values())
    assert rep["qkv"]["v"] == rep["bounds"]["attention_out"] and rep["margin"] <= rep["fp16_max"] / max(rep["qkv"].values())
    _fill(vit.transformer.resblocks[0].attn.in_proj_bias[3:4], 1e12)      # a Q bias
    assert vit.qkv16_resolution() is None and vit.r16_resolution() is not None
    _fill(vit.transformer.resblocks[0].attn.in_proj_bias[3:4], 0.0)
    assert vit.qkv16_resolution() is not None
    _fill(vit.transformer.resblocks[0].attn.in_proj_bias[W + 3:W + 4], float("nan"))   # a K bias
    assert vit.qkv16_resolution() is None and vit.r16_resolution() is not None
    _fill(vit.transformer.resblocks[0].attn.in_proj_bias[W + 3:W + 4], 0.0)
    _fill(vit.transformer.resblocks[0].mlp.c_proj.weight[0, 0:1], 33.0)
    assert vit.qkv16_resolution() is None and vit.r16_resolution() is None and vit.ln16_resolution() is not None
    _fill(vit.transformer.resblocks[0].mlp.c_fc.weight[0, 0:1], 33.0)
    assert vit.qkv16_resolution() is None and vit.r16_resolution() is None and vit.ln16_resolution() is None
    for res, patch, width, layers in ((224, 32, 768, 2), (224, 14, 1024, 2), (32, 16, 128, 2), (224, 16, 768, 1)):
        assert V.VisionTransformer(res, patch, width, layers, width // 64, 64).qkv16_resolution() is None


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


def _r16_in_proj_ksplit(batch, Ltok, width):
    """1 where ACX_PREC_F32X6_R16's in-projection (fp16 A planes, f32 rows out) is no launch whose K acx_gemm may split: its split model
    asks for no scratch (acx_gemm_scratch: as many tiles as workgroups) and its route, with the f32 LayerNorm buffer as scratch, does not
    split (acx_gemm_route); 2 otherwise"""
    rows = batch * Ltok
    d = L.GemmDesc()
    d.A = d.W = d.C = d.workspace = 256
    d.M, d.N, d.K, d.lda, d.ldw, d.ldc, d.ldr = rows, 3 * width, width, width, width, 3 * width, 3 * width
    d.a_dtype, d.c_dtype, d.prec, d.pairs, d.panels = L.ACX_F16, 0, L.PREC_BF16, 3, 3
    d.out_scale = 1.0 / 1024.0
    d.a_plane_stride, d.w_plane_stride = rows * width * 2, 3 * width * width * 2
    d.workspace_bytes = rows * width * 4
    r = L.GemmRoute()
    L.check(L.lib().acx_gemm_route(None, C.byref(d), C.byref(r)), None)
    assert r.route == 3                                                   # ACX_GEMM_ROUTE_X6
    need = L.GemmScratch()
    L.check(L.lib().acx_gemm_scratch(None, C.byref(d), 1, C.byref(need)), None)
    return r.ksplit if need.workspace_bytes == 0 else 2


def test_plan_equals_r16_but_for_the_attention_and_its_producer():
    """acx_transformer_plan(ACX_PREC_F32X6_QKV16) is ACX_PREC_F32X6_R16's plan record for record over the grid of tests/test_cpu_vit_plan.py,
    but for body layers whose attention is acx_attention_p3f behind an unsplit plane-kernel in-projection: there in_proj writes ACX_F16X2P
    planes (scratch word ACX_TF_BUF_QKV), att = ACX_TF_ATT_P3N with att_products = 103, and the attention-output word stays ACX_F16X2P."""
    seen = {"new": 0, "same": 0, "refused": 0}
    for batch, Ltok, width, heads, layers, causal, prune, planes, sized in _grid():
        args = (batch, Ltok, width, heads, layers)
        kw = dict(causal=bool(causal), prune_last=bool(prune), has_weight_planes=bool(planes), workspace_is_prec_sized=bool(sized))
        try:
            r16 = ops.transformer_plan(*args, prec=L.PREC_F32X6_R16, **kw)
        except L.AcxError as e:
            with pytest.raises(L.AcxError) as e2:
                ops.transformer_plan(*args, prec=L.PREC_F32X6_QKV16, **kw)
            assert str(e2.value).replace("ACX_PREC_F32X6_QKV16", "ACX_PREC_F32X6_R16") == str(e), (args, kw)
            seen["refused"] += 1
            continue
        new = ops.transformer_plan(*args, prec=L.PREC_F32X6_QKV16, **kw)
        assert len(r16) == len(new) == layers
        for rr, rn in zip(r16, new):
            fr, fn = _flat(rr), _flat(rn)
            want = dict(fr)
            if not fr["pruned"] and fr["att"] == L.TF_ATT_P3F and fr["reserved"] == L.F16X2P and fr["in_proj.kernel"] == L.TF_GEMM_X6 and \
                    fr["ln1_dtype"] == L.F16X2P and _r16_in_proj_ksplit(batch, Ltok, width) == 1:
                want.update({"in_proj.c_dtype": L.F16X2P, "in_proj.scratch": L.TF_BUF_QKV, "att": L.TF_ATT_P3N, "att_products": 103,
                             "reserved": L.F16X2P})
                seen["new"] += 1
            assert fn == want, (args, kw, fn, want)
            seen["same"] += fn == fr
    assert seen["new"] > 20 and seen["same"] > 20 and seen["refused"] > 0, seen
    # few tiles (fewer than workgroups: 8 and 32 frames of ViT-B/16) keep R16's record, 64 frames and more move
    for n, moves in ((8, False), (32, False), (64, True), (256, True)):
        a = (n, 197, W, 12, 12)
        same = ops.transformer_plan(*a, prec=L.PREC_F32X6_QKV16, prune_last=True) == ops.transformer_plan(*a, prec=L.PREC_F32X6_R16, prune_last=True)
        assert same != moves, n
    with pytest.raises(L.AcxError, match="ACX_PREC_F32X6_QKV16 is built for widths 768 and 1024"):
        ops.transformer_plan(64, 257, 512, 8, 4, prec=L.PREC_F32X6_QKV16, prune_last=True)


def test_other_geometries_are_r16_everywhere():
    """ViT-B/32 (50 tokens), ViT-L/14 (257) and the tiny test geometry: no planes attention, so every record is ACX_PREC_F32X6_R16's"""
    for batch in (8, 64, 512):
        for Ltok, width, layers in ((50, 768, 12), (257, 1024, 24)):
            a = (batch, Ltok, width, width // 64, layers)
            assert ops.transformer_plan(*a, prec=L.PREC_F32X6_QKV16, prune_last=True) == ops.transformer_plan(*a, prec=L.PREC_F32X6_R16, prune_last=True)
    for prec in (L.PREC_F32X6_QKV16, L.PREC_F32X6_R16):
        with pytest.raises(L.AcxError, match="is built for widths 768 and 1024"):
            ops.transformer_plan(8, 5, 128, 2, 2, prec=prec, prune_last=True)


def test_the_flagship_launch_takes_the_new_path_on_every_body_layer():
    plan = ops.transformer_plan(512, 197, W, 12, 12, prec=L.PREC_F32X6_QKV16, prune_last=True)
    r16 = ops.transformer_plan(512, 197, W, 12, 12, prec=L.PREC_F32X6_R16, prune_last=True)
    for l in range(11):
        r = plan[l]
        assert (r["att"], r["att_products"], r["reserved"], r["in_proj"]["c_dtype"], r["in_proj"]["kernel"], r["ln1_dtype"]) == \
            (L.TF_ATT_P3N, 103, L.F16X2P, L.F16X2P, L.TF_GEMM_X6, L.F16X2P), l
        assert r16[l]["att"] == L.TF_ATT_P3F and r16[l]["in_proj"]["c_dtype"] == 0
        for k in ("ln1", "ln2", "ln2_dtype", "out_proj", "fc", "proj", "split_att", "split_mlp", "pruned"):
            assert r[k] == r16[l][k], (l, k)
    assert plan[11] == r16[11] and plan[11]["pruned"] == 1
    # the workspace of the new mode is R16's: the planes live where the f32 q | k | v rows live
    d5 = L.VitDesc(224, 16, W, 12, 12, 512, L.PREC_F32X6_QKV16, L.ACT_QUICKGELU)
    d4 = L.VitDesc(224, 16, W, 12, 12, 512, L.PREC_F32X6_R16, L.ACT_QUICKGELU)
    lib = L.lib()
    assert lib.acx_vit_workspace_bytes(C.byref(d5), 512) == lib.acx_vit_workspace_bytes(C.byref(d4), 512) > 0


def test_qkv16_kernel_registers():
    """attn_p3_h16_kernel: no scratch, no spills, occupancy 2 under __launch_bounds__(512, 2), VGPRs + AGPRs <= 256 (eight waves of a
    workgroup, two to a SIMD); the attention kernels that existed before keep their instantiation list, and gemm_x6_r16_kernel -- whose
    <2, 0, ...> instantiations produce the q | k | v planes -- keeps its own: no new GEMM instantiation."""
    L.lib()
    rows = _build.kernel_resources()
    r16, att = {}, {}
    for k, v in rows.items():
        for name, dst in (("gemm_x6_r16_kernel", r16), ("attn_p3_kernel", att)):
            if name + "I" in k:
                dst[tuple(int(x) for x in re.findall(r"Li(\d+)E", k.split(name + "I")[1]))] = v
    h16 = [v for k, v in rows.items() if "attn_p3_h16_kernel" in k]
    o16 = [v for k, v in rows.items() if "attn_p3_o16_kernel" in k]
    assert len(h16) == 1 and len(o16) == 1
    new = h16[0]
    assert new["ScratchSize [bytes/lane]"] == 0 and new["VGPRs Spill"] == 0
    assert new["Occupancy [waves/SIMD]"] == 2 and new["VGPRs"] + new["AGPRs"] <= 256, new
    assert sorted(att) == [(3, 0, 0), (3, 1, 0), (6, 0, 0), (6, 0, 1)], sorted(att)
    want = [(2, act, 0, 0, 0, 0, ni, 0, 2, 0) for act in (0, 1) for ni in (1, 2, 4)] + [(0, 0, 1, 0, 0, 0, ni, 0, 2, 1) for ni in (1, 2, 4)]
    assert sorted(r16) == sorted(want), sorted(r16)
