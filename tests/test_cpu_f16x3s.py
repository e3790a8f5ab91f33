"""No device: ACX_PREC_F16X3S / precision "f16x3s" -- the f16x3 arithmetic on every ViT sequence length.

acx_transformer_plan with a NULL context is host arithmetic.  ACX_PREC_F16X3S is ACX_PREC_F16X3 in every respect but the attention
rule: wherever the ACX_PREC_F16X3 plan exists, the ACX_PREC_F16X3S plan is that plan, record for record; where ACX_PREC_F16X3 refuses
a non-causal sequence for its length alone, ACX_PREC_F16X3S plans the streaming planes attention (ACX_TF_ATT_S16) between an
in-projection that writes fp16 planes and an out-projection that reads them; a causal sequence, a missing weight plane and an
f32-sized workspace are answered as for ACX_PREC_F16X3.  The Python side: the name in PRECISIONS, check_vit_precision and AnomalyCLIP
accept it on the four ViT backbones and refuse it on a ResNet and above 1024 tokens; "f16x3" keeps its refusals."""
import itertools

import pytest
import torch

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.components import anomaly_clip as AC
from anomalyclip_amd.components.clip_vit import PRECISIONS, VisionTransformer, check_vit_precision
from anomalyclip_amd.components.clip_resnet import check_resnet_precision

E_BADARG, E_UNSUPPORTED = -1, -2
GATE = "driver: ACX_PREC_F16X3 needs the planes attention (192 < L <= 208) and all four products on the plane kernel"
VISION = {"ViT-B/16": IW.VIT_B16, "ViT-B/32": IW.VIT_B32, "ViT-L/14": IW.VIT_L14, "ViT-L/14@336px": IW.VIT_L14_336, "TINY": IW.TINY}
FRAMES = (1, 2, 7, 8, 9, 64, 160, 222, 256, 512)
PRODUCTS = ("in_proj", "out_proj", "fc", "proj")


def vision_shape(g):
    return (g.image_resolution // g.vision_patch_size) ** 2 + 1, g.vision_width, g.vision_width // 64, g.vision_layers


def query(batch, L_, W, heads, layers, causal, prec, prune, planes, sized):
    """(rc, [record dict per layer], error text) of acx_transformer_plan"""
    out = (L.TfLayerPlan * layers)()
    rc = L.lib().acx_transformer_plan(None, batch, L_, W, heads, layers, causal, prec, prune, planes, sized, out)
    return rc, [ops._struct_dict(out[l]) for l in range(layers)], L.lib().acx_last_error(None).decode()


def grid():
    for (name, g), frames, prune, planes, sized in itertools.product(VISION.items(), FRAMES, (0, 1), (0, 1), (0, 1)):
        yield (frames,) + vision_shape(g) + (0,), (prune, planes, sized)
    for width, batch, planes, sized in itertools.product((512, 768), (14, 1), (0, 1), (0, 1)):
        yield (batch, 77, width, width // 64, 12, 1), (0, planes, sized)


def test_the_constants():
    assert L.PREC_F16X3S == 9 and L.TF_ATT_S16 == 7 and PRECISIONS["f16x3s"] == L.PREC_F16X3S and PRECISIONS["f16x3"] == L.PREC_F16X3


def test_against_the_f16x3_plan_on_the_whole_grid():
    same = new = refused = 0
    for geom, rest in grid():
        rc3, recs3, text3 = query(*geom, L.PREC_F16X3, *rest)
        rcs, recss, texts = query(*geom, L.PREC_F16X3S, *rest)
        causal, L_ = geom[5], geom[1]
        if rc3 == 0:                                                       # ... the same plan
            assert rcs == 0 and recss == recs3, (geom, rest)
            same += 1
        elif rcs != 0:                                                     # both refuse: the same code and text
            assert (rcs, texts) == (rc3, text3), (geom, rest, texts)
            assert causal or GATE not in text3 or not _all_four(geom, rest), (geom, rest)
            refused += 1
        else:                                                              # only the length stood in the way
            assert rc3 == E_UNSUPPORTED and GATE in text3 and not causal and not 192 < L_ <= 208, (geom, rest)
            assert all(r["att"] == L.TF_ATT_S16 for r in recss if not r["pruned"])
            new += 1
    assert same and new and refused, (same, new, refused)


def _all_four(geom, rest):
    """whether the six-product mode runs all four products of this geometry on the plane kernel (the rule does not look at the format)"""
    rc, recs, _ = query(*geom, L.PREC_F32X6, *rest)
    body = [r for r in recs if not r["pruned"]]
    return rc == 0 and bool(body) and all(body[0][p]["kernel"] == L.TF_GEMM_X6 for p in PRODUCTS)


@pytest.mark.parametrize("frames", [64, 512])
@pytest.mark.parametrize("arch", ["ViT-B/16", "ViT-B/32", "ViT-L/14", "ViT-L/14@336px"])
def test_the_four_backbones(arch, frames):
    geom = (frames,) + vision_shape(VISION[arch]) + (0,)
    rc3, recs3, text3 = query(*geom, L.PREC_F16X3, 1, 1, 1)
    rc, recs, text = query(*geom, L.PREC_F16X3S, 1, 1, 1)
    assert rc == 0, text
    if arch == "ViT-B/16":
        assert rc3 == 0 and recs == recs3
        assert all(r["att"] == L.TF_ATT_P3N and r["att_products"] == 103 for r in recs[:-1])
        return
    assert rc3 == E_UNSUPPORTED and GATE in text3
    assert recs[-1]["pruned"] == 1 and recs[-1]["att"] in (L.TF_ATT_CLS, L.TF_ATT_CLS_FOLD)
    for r in recs[:-1]:
        assert r["att"] == L.TF_ATT_S16 and r["att_products"] == 0 and r["split_att"] == 0 and r["reserved"] == 0
        assert r["in_proj"] == {"kernel": L.TF_GEMM_X6, "c_dtype": L.F16X2P, "scratch": L.TF_BUF_QKV, "ln_job": 0}
        assert r["out_proj"]["kernel"] == L.TF_GEMM_X6 and r["out_proj"]["c_dtype"] == L.ACX_F32
        assert r["fc"]["kernel"] == L.TF_GEMM_X6 and r["fc"]["c_dtype"] == L.F16X2P and r["proj"]["kernel"] == L.TF_GEMM_X6
        assert r["ln1_dtype"] == r["ln2_dtype"] == L.F16X2P and r["split_mlp"] == 0
    # the pruned last layer is the one the six-product mode plans
    assert recs[-1] == query(*geom, L.PREC_F32X6, 1, 1, 1)[1][-1]


@pytest.mark.parametrize("arch", ["ViT-B/32", "ViT-L/14", "ViT-L/14@336px"])
def test_a_fall_back_plan_is_the_f32_plan(arch):
    geom = (512,) + vision_shape(VISION[arch]) + (0,)
    for prune, planes in itertools.product((0, 1), (0, 1)):
        assert query(*geom, L.PREC_F16X3S, prune, planes, 0)[:2] == query(*geom, L.PREC_F32, prune, planes, 0)[:2]


def test_missing_weight_planes():
    rc, recs, text = query(512, 257, 1024, 16, 24, 0, L.PREC_F16X3S, 1, 0, 1)
    assert rc == E_BADARG and "missing" in text and "weight planes" in text
    assert all(r["att"] == 0 and r["in_proj"]["kernel"] == 0 for r in recs)


def test_a_causal_sequence_gets_the_f16x3_answer():
    for batch in (14, 512):
        a, b = query(batch, 77, 768, 12, 12, 1, L.PREC_F16X3, 0, 1, 1), query(batch, 77, 768, 12, 12, 1, L.PREC_F16X3S, 0, 1, 1)
        assert a == b
    assert query(512, 77, 768, 12, 12, 1, L.PREC_F16X3S, 0, 1, 1)[0] == E_UNSUPPORTED


def test_the_other_precisions_never_plan_the_streaming_attention():
    for geom, rest in grid():
        for prec in (L.PREC_F32, L.PREC_BF16, L.PREC_F32X6, L.PREC_F32X3, L.PREC_F16X3):
            rc, recs, _ = query(*geom, prec, *rest)
            assert all(r["att"] != L.TF_ATT_S16 for r in recs)


def test_workspace_queries_take_it():
    lib = L.lib()
    for W, rows in ((768, 512 * 50), (1024, 64 * 257)):
        assert lib.acx_transformer_workspace_bytes_prec(W, rows, L.PREC_F16X3S) == lib.acx_transformer_workspace_bytes_prec(W, rows, L.PREC_F16X3)
        assert lib.acx_transformer_workspace_bytes_prec(W, rows, L.PREC_F16X3S) > lib.acx_transformer_workspace_bytes_prec(W, rows, L.PREC_F32)


# ------------------------------------------------------------------------------------------------------------- the Python side
def _net_kw(**kw):
    base = dict(labels_key="ucf", emb_size=64, depth=1, heads=2, dim_heads=None, num_segments=32, seg_length=16,
                concat_features=False, normal_id=7, stride=1, load_from_features=True, select_idx_dropout_topk=0.7,
                select_idx_dropout_bottomk=0.7, ncrops=1, num_topk=3, num_bottomk=3)
    base.update(kw)
    return base


@pytest.mark.parametrize("arch", ["ViT-B/16", "ViT-B/32", "ViT-L/14", "ViT-L/14@336px"])
def test_accepted_on_the_four_vit_backbones(arch):
    g = AC._ARCH[arch]
    check_vit_precision("f16x3s", g.grid ** 2 + 1, g.vision_width, arch, g.image_resolution, g.vision_patch_size)
    with torch.device("meta"):
        vit = VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim,
                                precision="f16x3s", arch=arch)
    assert vit.precision == "f16x3s"
    net = AC.AnomalyCLIP(**_net_kw(arch=arch, precision="f16x3s"))
    # head and text tower keep the default's arithmetic, as for "f16x3"
    assert net.precision == "auto" and net.text_encoder.precision == "f32" and net.image_encoder.precision == "f16x3s"


def test_refused_on_a_resnet_and_above_1024_tokens():
    with pytest.raises(ValueError, match="f16x3s"):
        check_resnet_precision("f16x3s", "RN50", 64)
    with pytest.raises(ValueError, match="RN50"):
        AC.AnomalyCLIP(**_net_kw(arch="RN50", precision="f16x3s"))
    check_vit_precision("f16x3s", 1024, 768, "custom", 0, 0)
    with pytest.raises(ValueError, match="at most 1024"):
        check_vit_precision("f16x3s", 1025, 768, "custom", 0, 0)
    g = IW.ClipGeometry(image_resolution=528, vision_patch_size=16)            # 1090 tokens
    with torch.device("meta"), pytest.raises(ValueError, match="at most 1024"):
        VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim, precision="f16x3s")


def test_f16x3_keeps_its_refusals():
    g = IW.VIT_L14
    with torch.device("meta"), pytest.raises(ValueError, match="not available for ViT-L/14"):
        VisionTransformer(g.image_resolution, g.vision_patch_size, g.vision_width, g.vision_layers, g.vision_heads, g.embed_dim,
                          precision="f16x3", arch="ViT-L/14")
    with pytest.raises(ValueError, match="f16x3"):
        AC.AnomalyCLIP(**_net_kw(arch="ViT-B/32", precision="f16x3"))
    with pytest.raises(L.AcxError, match="ACX_PREC_F16X3 needs the planes attention"):
        ops.transformer_plan(512, 50, 768, 12, 12, prec=L.PREC_F16X3, prune_last=True)


def test_extract_takes_the_name(tmp_path):
    from anomalyclip_amd import extract
    w = tmp_path / "w.pt"
    w.write_bytes(b"")
    base = ["--weights", str(w), "--frames-root", str(tmp_path), "--out-root", str(tmp_path / "out"), "--precision", "f16x3s"]
    for arch in ("ViT-B/32", "ViT-L/14", "ViT-L/14@336px", "ViT-B/16"):
        assert extract.parse_args(["--arch", arch] + base).precision == "f16x3s"
    with pytest.raises(SystemExit):
        extract.parse_args(["--arch", "RN50"] + base)
    with pytest.raises(SystemExit):
        extract.parse_args(["--arch", "ViT-L/14"] + base[:-1] + ["f16x3"])
