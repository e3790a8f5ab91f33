"""open_clip's ViT-H-14 (`net.arch: ViT-H-14`: image tower of 16 heads of 80) without a device: the registry, the mirrors' names and
shapes against the reference (tests/golden/h14_shapes.json, make_golden_h14.py), checkpoint recognition, the refusals raised before
anything is allocated, the route query and the error codes of the head-dimension-80 entry points, the driver's plan, and the fp64
reference of the attention sweep (tests/clip_attn_hd_ref.py) against torch's fp32 evaluation."""
import ctypes as C
import json
import os

import pytest
import torch

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components import anomaly_clip as AC
from anomalyclip_amd.components.clip_vit import Transformer, VisionTransformer, check_vit_precision
from anomalyclip_amd.components.text_encoder import TextEncoder

import attn_ref as AR
import clip_attn_hd_ref as HR
import vit_plan_ref as VP

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ARCH = "ViT-H-14"
OTHER_ARCHS = ("ViT-B/16", "ViT-B/32", "ViT-L/14", "ViT-L/14@336px", "RN50", "RN101", "RN50x4", "RN50x16", "RN50x64")
UNSUPPORTED, BADARG = -2, -1
CTX = None                                    # acx_attention_hd_route needs no device property: it is asked without a context


def _shapes():
    with open(os.path.join(GOLDEN, "h14_shapes.json")) as f:
        return json.load(f)[ARCH]


def _net_kw(**kw):
    base = dict(labels_key="ucf", emb_size=64, depth=1, heads=2, dim_heads=None, num_segments=32, seg_length=16,
                concat_features=False, normal_id=7, stride=1, load_from_features=True, select_idx_dropout_topk=0.7,
                select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3)
    base.update(kw)
    return base


# ------------------------------------------------------------------------------------------------------------- registry, shapes
def test_registry_has_vit_h14_under_open_clips_name():
    g = AC._ARCH[ARCH]
    assert g == IW.VIT_H14 and AC.geometry_of_arch(ARCH) is g
    assert (g.vision_heads, g.vision_head_dim, g.grid ** 2 + 1, g.vision_width, g.vision_layers, g.embed_dim) == (16, 80, 257, 1280, 32, 1024)
    assert (g.transformer_width, g.transformer_heads, g.transformer_layers, g.act) == (1024, 16, 24, "gelu")
    assert "vision_head_dim" not in g.as_kwargs() and "act" not in g.as_kwargs()
    assert IW.VIT_L14.vision_head_dim == 64 and IW.VIT_L14.vision_heads == 16 and IW.VIT_B16.vision_heads == 12
    with pytest.raises(ValueError) as e:
        AC.geometry_of_arch("ViT-H/14")
    assert "ViT-H/14" in str(e.value) and "'ViT-H-14'" in str(e.value)


def test_mirror_state_dict_matches_the_reference():
    g = IW.VIT_H14
    with torch.device("meta"):
        vit = VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim,
                                arch=ARCH, act=g.act)
        te = TextEncoder(g.context_length, g.transformer_width, g.transformer_heads, g.transformer_layers, g.embed_dim)
        tok = AC._TokenEmbedding(g.vocab_size, g.transformer_width)
        sd = IW.init_vit_state_dict(g, 0, prefix="visual.")
    mine = {"visual." + k: list(v.shape) for k, v in vit.state_dict().items()}
    mine.update({k: list(v.shape) for k, v in te.state_dict().items()})
    mine["token_embedding.weight"] = list(tok.weight.shape)
    ref = _shapes()
    assert mine == {k: v for k, v in ref.items() if k != "logit_scale"}
    assert {k: list(v.shape) for k, v in sd.items()} == {k: v for k, v in ref.items() if k.startswith("visual.")}
    assert vit.transformer.heads == 16 and vit.tokens == 257


def _meta_checkpoint(shapes):
    out = {}
    for k, shape in shapes.items():
        if k.startswith("visual."):
            out["image_encoder." + k[len("visual."):]] = torch.empty(shape, device="meta")
        elif k.startswith(("transformer.", "positional_embedding", "ln_final.", "text_projection")):
            out["text_encoder." + k] = torch.empty(shape, device="meta")
    return out


def test_geometry_from_state_dict_recognises_vit_h14_and_keeps_the_others():
    got = AC.geometry_from_state_dict(_meta_checkpoint(_shapes()))
    assert got == AC._ARCH[ARCH] and got.vision_heads == 16 and got.act == "gelu"
    image_only = {k: v for k, v in _meta_checkpoint(_shapes()).items() if k.startswith("image_encoder.")}
    assert AC.geometry_from_state_dict(image_only).vision_head_dim == 80
    with open(os.path.join(GOLDEN, "arch_shapes.json")) as f:
        vit_shapes = json.load(f)
    for arch in OTHER_ARCHS:
        g = AC._ARCH[arch]
        if arch in vit_shapes:
            sd = _meta_checkpoint(vit_shapes[arch])
        else:
            with torch.device("meta"):
                sd = IW.init_resnet_state_dict(g, 0)
                sd.update({k: v for k, v in IW.init_text_state_dict(g, 0).items() if k.startswith("text_encoder.")})
        got = AC.geometry_from_state_dict(sd)
        assert got == g and got.vision_head_dim == 64 and got.act == "quick_gelu", arch


def test_from_clip_state_dict_takes_an_open_clip_vit_h14():
    from anomalyclip_amd import checkpoint as K
    sd = {k: torch.empty(shape, device="meta") for k, shape in _shapes().items()}
    assert K.is_clip_state_dict(sd)
    out = K.from_clip_state_dict(sd)
    assert AC.geometry_from_state_dict(out) == AC._ARCH[ARCH]
    assert out["image_encoder.transformer.resblocks.31.attn.in_proj_weight"].shape == (3840, 1280)


# ------------------------------------------------------------------------------------------------------------- refusals
@pytest.mark.parametrize("precision", ["bf16", "bf16x3", "f16x3", "f16x3s"])
def test_refused_precisions_name_arch_and_precision(precision, monkeypatch):
    """before any allocation: no parameter of the model is created"""
    def boom(*a, **k):
        raise AssertionError("allocated before the refusal")
    monkeypatch.setattr(torch.nn.Module, "register_parameter", boom)
    with pytest.raises(ValueError) as e:
        AC.AnomalyCLIP(**_net_kw(arch=ARCH, precision=precision, act="quick_gelu" if precision == "bf16" else None))
    assert ARCH in str(e.value) and repr(precision) in str(e.value)
    g = IW.VIT_H14
    with pytest.raises(ValueError) as e:
        check_vit_precision(precision, 257, 1280, ARCH, 224, 14, g.vision_head_dim)
    assert ARCH in str(e.value) and repr(precision) in str(e.value)
    monkeypatch.undo()
    with torch.device("meta"), pytest.raises(ValueError, match="head dimension is 80"):
        VisionTransformer(224, 14, 1280, 1, 16, 1024, precision=precision, arch=ARCH)


def test_running_precisions_and_the_extract_command_line():
    from anomalyclip_amd import extract
    for precision in ("auto", "f32", "f32x6"):
        check_vit_precision(precision, 257, 1280, ARCH, 224, 14, 80)
        with torch.device("meta"):
            VisionTransformer(224, 14, 1280, 2, 16, 1024, precision=precision, arch=ARCH, act="gelu")
    with torch.device("meta"):
        enc = extract.build_image_encoder(ARCH)
    assert (enc.width, enc.heads, enc.layers, enc.act, enc.output_dim) == (1280, 16, 32, "gelu", 1024)
    p = extract._parser()
    assert p.parse_args(["--arch", ARCH, "--weights", "w", "--frames-root", "f", "--out-root", "o"]).arch == ARCH
    with pytest.raises(SystemExit):
        p.parse_args(["--arch", "ViT-H/14", "--weights", "w", "--frames-root", "f", "--out-root", "o"])


def test_transformer_head_dimensions():
    with torch.device("meta"):
        t = Transformer(1280, 2, 16)
        assert (t.width, t.heads) == (1280, 16)
        Transformer(1024, 2, 16)
        Transformer(1024, 2, 16, causal=True)
        with pytest.raises(ValueError, match="17 heads"):
            Transformer(1280, 2, 17)
        with pytest.raises(ValueError, match="non-causal"):
            Transformer(1280, 2, 16, causal=True)


# ------------------------------------------------------------------------------------------------------------- route, error codes
def hd_route(L_, head_dim=80, aligned=1, ctx=CTX):
    return L.lib().acx_attention_hd_route(ctx, L_, head_dim, aligned)


def test_route_boundaries():
    S, Q = L.ATTN_HD_ROUTE_STREAM, L.ATTN_HD_ROUTE_STREAM_QB
    assert (S, Q) == (1, 2)
    for ctx in (None,):
        assert hd_route(0, ctx=ctx) == hd_route(-1, ctx=ctx) == hd_route(1025, ctx=ctx) == UNSUPPORTED            # 0 | 1, 1024 | 1025
        assert hd_route(1, ctx=ctx) == hd_route(128, ctx=ctx) == S and hd_route(129, ctx=ctx) == hd_route(1024, ctx=ctx) == Q   # 128 | 129
        for hd in (48, 64, 96):
            assert hd_route(197, hd, ctx=ctx) == UNSUPPORTED
        for L_ in (1, 128, 129, 1024):
            assert hd_route(L_, 80, 0, ctx) == UNSUPPORTED                                                          # no misaligned route


@pytest.mark.parametrize("c", [c for c in HR.CASES if c.route], ids=HR.case_id)
def test_route_tags_are_the_librarys(c):
    assert hd_route(c.L) == HR.route_id(c.route) and HR.route_of(c.L) == c.route


def test_table_holds_what_it_promises():
    hd = [c for c in HR.CASES if c.entry == "hd" and not c.spike and not c.many]
    assert sorted(c.L for c in hd if c.route == "stream") == list(HR.STREAM_L)
    assert sorted(c.L for c in hd if c.route == "stream_qb") == list(HR.QB_L)
    assert {1, 15, 16, 17, 31, 32, 33, 64, 65, 197, 256, 257, 577, 1023, 1024} <= set(HR.STREAM_L + HR.QB_L)
    for a in (128, 256, 384, 512, 640, 768, 896):                          # both sides of every change of the query block count
        assert a in HR.STREAM_L + HR.QB_L and a + 1 in HR.QB_L and HR.qblocks(a) + 1 == HR.qblocks(a + 1)
    assert {HR.qblocks(L_) for L_ in HR.STREAM_L} == {1} and {HR.qblocks(L_) for L_ in HR.QB_L} == set(range(2, 9))
    assert all((c.batch, c.heads) == (2, 3) for c in hd)
    many = [c for c in HR.CASES if c.many]
    assert len(many) == 1 and many[0].batch * many[0].heads * many[0].qblocks > 512 and HR.qblocks(many[0].L) == many[0].qblocks
    assert {(c.L, c.spike) for c in HR.CASES if c.spike} == {(577, "last"), (1009, "tile"), (113, "last")}
    for e in ("x3", "x3_panel"):
        for heads in (3, 16):
            assert sorted(c.L for c in HR.CASES if c.entry == e and c.heads == heads) == list(HR.PLANE_L)
    assert sorted(c.L for c in HR.CASES if c.entry == "cls") == list(HR.CLS_L)
    assert len({HR.case_id(c) for c in HR.CASES}) == len(HR.CASES)


def test_hd_entry_points_refuse_with_a_null_context():
    """every code comes before any launch: host memory, no device"""
    lib = L.lib()
    buf = (C.c_float * 4096)()
    p = (C.addressof(buf) + 15) & ~15
    W = 80
    entries = {
        "acx_attention_hd": lambda q, o, L_, heads, hd: lib.acx_attention_hd(None, q, 3 * W, o, W, 1, L_, heads, hd, None),
        "acx_attention_x3_hd": lambda q, o, L_, heads, hd: lib.acx_attention_x3_hd(None, q, 3 * W, o, W, 1, L_, heads, hd, 0, None),
        "acx_attention_cls_hd": lambda q, o, L_, heads, hd: lib.acx_attention_cls_hd(None, q, 3 * W, o, W, 1, L_, heads, hd, None),
    }
    for name, call in entries.items():
        assert call(None, p, 4, 1, 80) == BADARG and call(p, None, 4, 1, 80) == BADARG, name
        assert b"null pointer" in lib.acx_last_error(None) and name.encode() in lib.acx_last_error(None)
        for hd in (48, 64, 96):
            assert call(p, p, 4, 1, hd) == UNSUPPORTED, (name, hd)
            assert b"head_dim %d" % hd in lib.acx_last_error(None), (name, lib.acx_last_error(None))
        for L_ in (0, 1025):
            assert call(p, p, L_, 1, 80) == UNSUPPORTED, (name, L_)
        assert call(p, p, 4, 0, 80) == UNSUPPORTED, name
        assert b"1 <= L <= 1024" in lib.acx_last_error(None)
        assert call(p + 4, p, 4, 1, 80) == BADARG, name                       # qkv off a 16-byte boundary
    assert lib.acx_attention_hd(None, p, 3 * W, p + 4, W, 1, 4, 1, 80, None) == UNSUPPORTED            # out misaligned: the route's answer
    assert lib.acx_attention_hd(None, p, 3 * W, p, W + 1, 1, 4, 1, 80, None) == UNSUPPORTED            # ldo % 4
    assert lib.acx_attention_x3_hd(None, p, 3 * W, p, W, 1, 4, 1, 80, 1, None) == BADARG               # K-panel planes: ldo % 32
    assert lib.acx_attention_hd(None, p, 3 * W, p, W, 0, 4, 1, 80, None) == 0                          # an empty batch is nothing to do
    for name in ("acx_attention_hd", "acx_attention_cls_hd"):                                          # leading dimensions too small
        fn = getattr(lib, name)
        assert fn(None, p, 3 * W - 4, p, W, 1, 4, 1, 80, None) == BADARG and fn(None, p, 3 * W, p, W - 4, 1, 4, 1, 80, None) == BADARG, name
        assert fn(None, p, 6 * W, p, W, 1, 4, 2, 80, None) == BADARG, name                             # ldo < 2 heads of 80
    # the head-dimension-64 entry points keep their meaning: 80 columns per head are not theirs to take
    assert lib.acx_attention(None, p, 192, p, 64, 1, 1025, 1, 0, None) == UNSUPPORTED


# ------------------------------------------------------------------------------------------------------------- the driver's plan
def test_plan_at_vit_h14():
    for prec, att, ln, dt in ((L.PREC_F32X6, L.TF_ATT_HD_X3_PANEL, L.TF_LN_PLANES, L.BF16X3P), (L.PREC_F32, L.TF_ATT_HD_F32, L.TF_LN_ROWS, L.ACX_F32)):
        for batch in (8, 64, 256):
            recs = ops.transformer_plan(batch, 257, 1280, 16, 32, prec=prec, prune_last=True)
            assert len(recs) == 32
            for r in recs[:-1]:
                assert r["att"] == att and r["pruned"] == 0 and r["split_att"] == 0 and r["att_products"] == 0
                assert (r["ln1"], r["ln2"], r["ln1_dtype"], r["ln2_dtype"]) == (ln, ln, dt, dt)
                assert r["in_proj"]["c_dtype"] == L.ACX_F32 and r["out_proj"]["ln_job"] == 0 and r["proj"]["ln_job"] == 0
                assert r["in_proj"]["kernel"] == (L.TF_GEMM_X6 if prec == L.PREC_F32X6 else L.TF_GEMM_ROWS)
            last = recs[-1]
            assert last["pruned"] == 1 and last["att"] == L.TF_ATT_HD_CLS
            for r in recs:
                assert r["att"] != L.TF_ATT_CLS_FOLD and L.TF_LN_RIDDEN not in (r["ln1"], r["ln2"])
                assert not any(r[p]["ln_job"] for p in ("in_proj", "out_proj", "fc", "proj"))
    # without the prune (acx_transformer_forward): the body attention in every layer
    assert {r["att"] for r in ops.transformer_plan(8, 257, 1280, 16, 3, prec=L.PREC_F32)} == {L.TF_ATT_HD_F32}


@pytest.mark.parametrize("prec", ["PREC_BF16", "PREC_F32X3", "PREC_F16X3", "PREC_F16X3S", "PREC_F32X6_LN16", "PREC_F32X6_R16"])
def test_plan_refuses_the_other_precisions_and_a_causal_tower(prec):
    with pytest.raises(L.AcxError, match="libacx error -2"):                 # ACX_E_UNSUPPORTED
        ops.transformer_plan(64, 257, 1280, 16, 4, prec=getattr(L, prec), prune_last=True)
    with pytest.raises(L.AcxError, match="non-causal"):
        ops.transformer_plan(14, 77, 1280, 16, 4, causal=True, prec=L.PREC_F32)


def test_plan_of_vit_l14_is_the_restated_walk():
    """head dimension 64 keeps its records: ViT-L/14 (and its text tower) against the walk restated in vit_plan_ref"""
    for batch, Ltok, W, heads, layers, causal, prec, prune in ((64, 257, 1024, 16, 24, 0, L.PREC_F32X6, 1), (256, 257, 1024, 16, 24, 0, L.PREC_F32, 1),
                                                              (64, 197, 768, 12, 12, 0, L.PREC_F32X6, 1), (14, 77, 768, 12, 12, 1, L.PREC_F32, 0)):
        code, want = VP.plan_ref(batch, Ltok, W, heads, layers, causal, prec, prune, 1, 1)
        assert code == 0
        got = ops.transformer_plan(batch, Ltok, W, heads, layers, causal=bool(causal), prec=prec, prune_last=bool(prune))
        assert [{f: r[f] for f in VP.FIELDS} for r in got] == [{f: r[f] for f in VP.FIELDS} for r in want], (Ltok, W, prec)
        assert all(r["att"] < L.TF_ATT_HD_F32 for r in got)


# ------------------------------------------------------------------------------------------------------------- the reference
def test_reference_is_attn_refs_closed_form_at_80():
    c = next(c for c in HR.CASES if c.L == 65 and c.entry == "hd" and not c.many)
    qkv, o, S = HR.reference(c)
    W = c.heads * 80
    o2, S2 = AR.attention(qkv, torch.zeros(c.batch * c.L, W), c.batch, 1, c.L, c.heads, 80, 1, 0, 80 ** -0.5)["o"]
    assert torch.equal(o, o2) and torch.equal(S, S2) and (HR.E, HR.SCALE, HR.TOL) == (80, 80 ** -0.5, AR.TOL)
    # against a plain softmax in fp64
    q, k, v = (qkv[:, i * W:(i + 1) * W].double().view(c.batch, c.L, c.heads, 80).transpose(1, 2) for i in range(3))
    plain = (torch.softmax(q @ k.transpose(-1, -2) * 80 ** -0.5, -1) @ v).transpose(1, 2).reshape(c.batch * c.L, W)
    assert float((plain - o).abs().max()) <= 1e-12 * float(o.abs().max())


@pytest.mark.parametrize("c", [c for c in HR.CASES if c.entry == "hd"], ids=HR.case_id)
def test_torch_fp32_stays_below_half_the_bound(c):
    qkv, o, S = HR.reference(c)
    AR.within(HR.torch_fp32(c, qkv), o, S, HR.case_id(c), "torch_fp32_hd80", tol=0.5 * HR.TOL)
