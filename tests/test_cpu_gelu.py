"""No GPU: the host side of the exact GELU and of plain CLIP state dicts -- checkpoint.from_clip_state_dict into the image encoder and
into AnomalyCLIP for every ViT arch, the construction and command-line errors of `act`, the inequality |gelu(x)| <= |x| that
ACX_PREC_F32X6_R16's fp16 hidden planes rest on, and the kernel resource tables recorded before and after the GELU instantiations."""
import json
import os

import pytest
import torch

from anomalyclip_amd import _build
from anomalyclip_amd import checkpoint as K
from anomalyclip_amd import extract as X
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
from anomalyclip_amd.components.clip_vit import ACTS, Transformer, VisionTransformer, check_act

import gelu_ref as R

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
VIT_ARCHS = ["ViT-B/16", "ViT-B/32", "ViT-L/14", "ViT-L/14@336px"]
_DICTS = {}


def _clip_dict(arch):
    """a seeded CLIP state_dict with the reference's names and shapes (tests/golden/arch_shapes.json), every third tensor half; plus
    what a JIT archive / open_clip add.  Large tensors repeat a seeded block (the values only have to be told apart)"""
    if arch not in _DICTS:
        with open(os.path.join(HERE, "golden", "arch_shapes.json")) as f:
            shapes = json.load(f)[arch]
        g = torch.Generator().manual_seed(len(arch) + sum(map(ord, arch)))
        block = torch.randn(65537, generator=g) * 0.05
        sd = {}
        for i, (k, shp) in enumerate(sorted(shapes.items())):
            n = 1
            for s in shp:
                n *= s
            v = (block.roll(i * 131).repeat((n + block.numel() - 1) // block.numel())[:n] + 1e-3 * i).reshape(shp)
            sd[k] = v.half() if i % 3 == 0 and k != "logit_scale" else v
        sd["input_resolution"], sd["context_length"], sd["vocab_size"] = torch.tensor(224), torch.tensor(77), torch.tensor(49408)
        _DICTS[arch] = sd
    return _DICTS[arch]


@pytest.fixture(scope="module", autouse=True)
def _release():
    yield
    _DICTS.clear()


def test_from_clip_state_dict_maps_every_key():
    sd = _clip_dict("ViT-B/16")
    out = K.from_clip_state_dict(sd)
    assert K.is_clip_state_dict(sd) and not K.is_clip_state_dict(out)
    assert "image_encoder.conv1.weight" in out and "text_encoder.transformer.resblocks.0.attn.in_proj_weight" in out
    assert {"text_encoder.positional_embedding", "text_encoder.ln_final.weight", "text_encoder.text_projection", "token_embedding.weight"} <= set(out)
    assert not any(k in out for k in ("logit_scale", "input_resolution", "context_length", "vocab_size"))
    assert len(out) == len(sd) - 4
    assert all(v.dtype == torch.float32 for v in out.values())
    k16 = next(k for k, v in sd.items() if v.dtype == torch.float16 and k.startswith("visual."))
    assert torch.equal(out["image_encoder." + k16[len("visual."):]], sd[k16].float())
    with pytest.raises(ValueError, match="not a CLIP state_dict key"):
        K.from_clip_state_dict({**sd, "visual_projection_of_another_model": torch.zeros(1)})


@pytest.mark.parametrize("arch", VIT_ARCHS)
def test_clip_state_dict_into_the_image_encoder(arch):
    sd = _clip_dict(arch)
    enc = X.build_image_encoder(arch, "auto", act="gelu")
    assert enc.act == "gelu" and enc.transformer.act == "gelu"
    X.load_encoder_weights(enc, arch, sd)                 # strict: no missing, no unexpected key
    mine = enc.state_dict()
    vis = {k[len("visual."):]: v for k, v in sd.items() if k.startswith("visual.")}
    assert set(mine) == set(vis)
    for k, v in vis.items():
        assert mine[k].dtype == torch.float32 and torch.equal(mine[k], v.float()), k


@pytest.mark.parametrize("arch", VIT_ARCHS)
def test_clip_state_dict_into_anomalyclip(arch):
    sd = _clip_dict(arch)
    net = AnomalyCLIP(arch=arch, labels_key="ucf", emb_size=256, depth=1, heads=8, dim_heads=None, num_segments=32, seg_length=16,
                      concat_features=False, normal_id=7, select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, num_topk=3,
                      num_bottomk=3, act="gelu")
    assert net.act == "gelu" and net.image_encoder.act == "gelu" and net.text_encoder.transformer.act == "gelu"
    res = net.load_state_dict(sd)                          # strict for the towers: nothing of theirs missing, nothing unexpected
    assert not res.unexpected_keys
    assert res.missing_keys and not any(k.startswith(("image_encoder.", "text_encoder.", "token_embedding.")) for k in res.missing_keys)
    mine = net.state_dict()
    want = K.from_clip_state_dict(sd)
    for k, v in want.items():
        assert torch.equal(mine[k], v), k
    # the prompt learner's frozen embeddings come from the loaded table
    toks = net.tokenized_prompts.long()
    emb = want["token_embedding.weight"][toks]
    assert torch.equal(net.prompt_learner.token_prefix, emb[:, :1]) and torch.equal(net.prompt_learner.token_suffix, emb[:, 1 + 8:])
    # checkpoint.load_into takes the same dict
    missing, unexpected = K.load_into(net, sd)
    assert not unexpected and missing == list(res.missing_keys)
    broken = {k: v for k, v in sd.items() if k != "visual.proj"}
    with pytest.raises(RuntimeError, match="image_encoder.proj"):
        net.load_state_dict(broken)


def test_clip_state_dict_of_another_arch_names_both():
    sd = _clip_dict("ViT-L/14")
    enc = X.build_image_encoder("ViT-B/16")
    with pytest.raises(ValueError, match=r"ViT-B/16.*ViT-L/14|ViT-L/14.*ViT-B/16"):
        X.load_encoder_weights(enc, "ViT-B/16", sd)
    net = AnomalyCLIP(arch="ViT-B/16", labels_key="ucf", emb_size=256, depth=1, heads=8, dim_heads=None, num_segments=32, seg_length=16,
                      concat_features=False, normal_id=7, select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, num_topk=3,
                      num_bottomk=3)
    with pytest.raises(ValueError, match=r"ViT-B/16.*ViT-L/14|ViT-L/14.*ViT-B/16"):
        net.load_state_dict(sd)


# ------------------------------------------------------------------------------------------------------------------ act
def test_act_defaults_and_geometry_field():
    assert ACTS == {"quick_gelu": 1, "gelu": 5}
    assert IW.ClipGeometry().act == "quick_gelu" and "act" not in IW.VIT_B16.as_kwargs()
    assert Transformer(128, 1, 2).act == "quick_gelu" and VisionTransformer(32, 16, 128, 1, 2, 64).act == "quick_gelu"
    assert X.build_image_encoder("tiny").act == "quick_gelu"
    assert X._parser().parse_args(["--arch", "tiny", "--weights", "w", "--frames-root", "f", "--out-root", "o"]).act == "quick_gelu"
    kw = dict(labels_key="ucf", emb_size=64, depth=1, heads=2, dim_heads=None, num_segments=32, seg_length=16, concat_features=False,
              normal_id=7, select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, num_topk=3, num_bottomk=3)
    assert AnomalyCLIP(arch="tiny", **kw).act == "quick_gelu"
    import dataclasses
    net = AnomalyCLIP(arch="tiny", clip_geometry=dataclasses.replace(IW.TINY, act="gelu"), **kw)      # the geometry's field, unless net.act says otherwise
    assert net.act == "gelu" and net.text_encoder.transformer.act == "gelu"
    assert AnomalyCLIP(arch="tiny", clip_geometry=dataclasses.replace(IW.TINY, act="gelu"), act="quick_gelu", **kw).act == "quick_gelu"


def test_act_construction_errors():
    with pytest.raises(ValueError, match="act='relu'"):
        VisionTransformer(32, 16, 128, 1, 2, 64, act="relu")
    with pytest.raises(ValueError, match="act='relu'"):
        Transformer(128, 1, 2, act="relu")
    with pytest.raises(ValueError, match="act='relu'"):
        X.build_image_encoder("tiny", act="relu")
    with pytest.raises(ValueError, match="act='gelu' with precision='bf16'"):
        VisionTransformer(32, 16, 128, 1, 2, 64, precision="bf16", act="gelu")
    with pytest.raises(ValueError, match="act='gelu' with precision='bf16'"):
        X.build_image_encoder("ViT-B/16", "bf16", act="gelu")
    with pytest.raises(ValueError, match="act='gelu' with arch='RN50'"):
        X.build_image_encoder("RN50", act="gelu")
    kw = dict(labels_key="ucf", emb_size=64, depth=1, heads=2, dim_heads=None, num_segments=32, seg_length=16, concat_features=False,
              normal_id=7, select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, num_topk=3, num_bottomk=3)
    with pytest.raises(ValueError, match="net.act='silu'"):
        AnomalyCLIP(arch="tiny", act="silu", **kw)
    with pytest.raises(ValueError, match="net.act='gelu' with precision='bf16'"):
        AnomalyCLIP(arch="tiny", act="gelu", precision="bf16", **kw)
    with pytest.raises(ValueError, match="net.act='gelu' with arch='RN101'"):
        AnomalyCLIP(arch="RN101", act="gelu", **kw)
    enc = VisionTransformer(32, 16, 128, 1, 2, 64, act="gelu")
    enc.precision = "bf16"                                  # a precision set later is caught at the next forward's check
    with pytest.raises(ValueError, match="bf16"):
        enc.check_precision()
    assert check_act("gelu", "auto", "ViT-B/16") == 5 and check_act("quick_gelu", "bf16", "RN50") == 1


@pytest.mark.parametrize("argv", [["--act", "gelu", "--precision", "bf16"], ["--act", "gelu", "--arch", "RN50"], ["--act", "tanh"]])
def test_extract_act_contradictions_exit_2(tmp_path, argv):
    base = ["--arch", "ViT-B/16", "--weights", str(tmp_path), "--frames-root", str(tmp_path), "--out-root", str(tmp_path)]
    with pytest.raises(SystemExit) as e:
        X.parse_args(base + argv)
    assert e.value.code == 2
    assert X.parse_args(base + ["--act", "gelu"]).act == "gelu"


def test_gelu_magnitude_never_exceeds_the_argument():
    """|gelu(x)| <= |x| in fp64 on the function sweep: Phi(x) lies in [0, 1] -- the inequality behind r16_scales' bound on the MLP
    hidden, for the exact GELU as for QuickGELU"""
    x = R.sweep().double()
    assert bool((R.gelu64(x).abs() <= x.abs()).all()) and bool((R.quick_gelu64(x).abs() <= x.abs()).all())
    phi = 0.5 * (1.0 + torch.erf(x / 2.0 ** 0.5))
    assert float(phi.min()) >= 0.0 and float(phi.max()) <= 1.0
    assert float((R.gelu64(x) - R.quick_gelu64(x)).abs().max()) > 1.9e-2       # ... and the two are 2e-2 apart


# ------------------------------------------------------------------------------------------------------------------ resources
_RES = ("VGPRs", "AGPRs", "SGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "Occupancy [waves/SIMD]", "LDS Size [bytes/block]")


def _table(path):
    out = {}
    with open(path) as fh:
        head = fh.readline().rstrip("\n").split("\t")
        for line in fh:
            v = line.rstrip("\n").split("\t")
            out[v[0]] = dict(zip(head[1:], v[1:]))
    return out


def test_gelu_instantiations_left_every_existing_kernel_as_it_was():
    """profiles/gelu_kernel_resources_{parent,after}.txt: the build's per-kernel table before and after the exact GELU was added.
    Every kernel of the parent is in the later table with the same registers, LDS, scratch and occupancy (the GELU is a template
    value of its own, never a branch inside an existing instantiation); the new kernels have no scratch and no spills -- in the
    recorded table and, where the library has been built, in the build's own."""
    parent = _table(os.path.join(REPO, "profiles", "gelu_kernel_resources_parent.txt"))
    after = _table(os.path.join(REPO, "profiles", "gelu_kernel_resources_after.txt"))
    assert len(parent) > 500 and set(parent) <= set(after)
    for k, row in parent.items():
        assert all(row[c] == after[k][c] for c in _RES), (k, row, after[k])
    new = sorted(set(after) - set(parent))
    assert len(new) == 48
    assert not any(n in k for k in new for n in ("gemm_x6_p4_kernel", "gemm_x6_h3_kernel", "gemm_x6_r16_kernel"))     # (names of their own)
    for stem in ("gemm_x6_gelu_kernel", "gemm_x6_h3_gelu_kernel", "gemm_x6_r16_gelu_kernel", "gemm_f32_sk_kernel", "gemm_f32_s64_kernel", "gemm_f32_w8_kernel",
                 "gemm_f32_p256_kernel", "gemm_kernel", "splitk_reduce_gelu_kernel", "splitk_reduce4_gelu_kernel", "act_gelu_kernel"):
        assert any(stem in k for k in new), stem
    for k in new:
        assert after[k]["ScratchSize [bytes/lane]"] == "0" and after[k]["VGPRs Spill"] == "0", k
    if os.path.exists(_build.RESOURCES):
        built = _build.kernel_resources()
        for k in new:
            if k in built:
                assert built[k]["ScratchSize [bytes/lane]"] == 0 and built[k]["VGPRs Spill"] == 0, k
