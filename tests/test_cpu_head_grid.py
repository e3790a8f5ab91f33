"""The temporal head on segment grids other than 32 x 16, CPU side: the geometry check that runs before anything is allocated, the
oracle against what the REFERENCE produced at three other grids (fixtures e2e_grid_*.npz, tests/golden/make_golden_grid.py), and
which grids take the bf16 x 6 plane convolutions under "auto"."""
import pytest
import torch

from anomalyclip_amd import init_weights as IW
from anomalyclip_amd.components.clip_vit import check_head_geometry
from oracle import anomalyclip_oracle as O
import recipes_grid as RG
from test_oracle_golden import T, close

torch.set_grad_enabled(False)

# (N, L, E, heads, dim_heads, depth, S, concat): the tuples the reference's own AnomalyCLIP was run at
REFERENCE_TUPLES = [(24, 10, 64, 2, None, 1, 2, False), (64, 16, 64, 2, None, 1, 1, False), (16, 32, 128, 2, None, 1, 3, False),
                    (48, 8, 64, 2, 16, 2, 2, True), (20, 20, 64, 4, None, 1, 1, False), (128, 4, 64, 1, None, 1, 1, False),
                    (7, 5, 64, 2, None, 1, 2, False), (64, 64, 64, 1, None, 1, 1, False), (40, 12, 128, 2, None, 2, 2, True)]


@pytest.mark.parametrize("N,L,E,heads,dim_heads,depth,S,concat", REFERENCE_TUPLES)
def test_check_head_geometry_accepts_the_reference_tuples(N, L, E, heads, dim_heads, depth, S, concat):
    check_head_geometry(N, L, E, heads, dim_heads, 3, 3)


@pytest.mark.parametrize("hc", [IW.UCF_HEAD, IW.SHT_HEAD, IW.XD_HEAD])
def test_check_head_geometry_accepts_the_shipped_configurations(hc):
    check_head_geometry(hc.num_segments, hc.seg_length, hc.emb_size, hc.heads, hc.dim_heads, hc.num_topk, hc.num_bottomk)


@pytest.mark.parametrize("args,key", [((129, 16, 256, 8, None, 3, 3), "num_segments"), ((32, 129, 256, 8, None, 3, 3), "seg_length"),
                                      ((32, 16, 256, 8, 24, 3, 3), "dim_heads"), ((32, 16, 96, 2, 16, 3, 3), "emb_size"),
                                      ((7, 5, 64, 2, None, 8, 3), "num_topk"), ((7, 5, 64, 2, None, 3, 8), "num_bottomk"),
                                      ((32, 16, 256, 2, None, 3, 3), "heads")])
def test_check_head_geometry_names_the_offending_key(args, key):
    with pytest.raises(ValueError, match=key + "="):
        check_head_geometry(*args)


def test_constructors_check_the_geometry_before_allocating():
    from anomalyclip_amd.components.anomaly_clip import AnomalyCLIP
    from anomalyclip_amd.components.temporal_model import TemporalModel
    kw = dict(arch="tiny", labels_key="ucf", emb_size=64, depth=1, heads=2, dim_heads=None, num_segments=32, seg_length=16,
              concat_features=False, normal_id=7, select_idx_dropout_topk=0.7, select_idx_dropout_bottomk=0.7, num_topk=3,
              num_bottomk=3)
    AnomalyCLIP(**dict(kw, num_segments=24, seg_length=10))
    for bad, key in ((dict(num_segments=129), "num_segments"), (dict(dim_heads=24), "dim_heads"), (dict(emb_size=96), "emb_size"),
                     (dict(num_segments=7, num_topk=8), "num_topk")):
        with pytest.raises(ValueError, match=key + "="):
            AnomalyCLIP(**dict(kw, **bad))
    with pytest.raises(ValueError, match="seg_length="):
        TemporalModel(64, 64, 1, 2, None, 1, 32, 200)
    tm = TemporalModel(64, 96, 1, 2, None, 1, 24, 10)          # any width constructs (x6_convs() can be asked) ...
    with pytest.raises(ValueError, match="emb_size="):          # ... and is refused before the first launch
        tm(torch.zeros(240, 64), 1, False)


@pytest.mark.parametrize("tag", list(RG.GRIDS))
def test_oracle_reproduces_the_reference_on_other_grids(golden, prompts_table, tag):
    """e2e_grid_<tag>.npz: test-mode similarity / scores, the train forward of four videos, the eight loss terms -- the bounds of
    test_oracle_golden.test_e2e_tiny."""
    hc, S, seed = RG.GRIDS[tag]
    g = golden("e2e_grid_" + tag)
    assert (int(g["seed"]), int(g["S"]), int(g["num_segments"]), int(g["seg_length"])) == (seed, S, hc.num_segments, hc.seg_length)
    geom = IW.TINY
    toks = torch.tensor(prompts_table["ucf"]["tokenized_prompts"], dtype=torch.int32)
    eot = toks.argmax(-1)
    sd = IW.init_anomalyclip_state_dict(geom, hc, toks, seed)
    inp = RG.grid_inputs(seed, geom.embed_dim, hc, S)
    sim, sc = O.anomaly_clip_forward_test(sd, hc, inp["test_feats"], inp["nc"], eot, geom.transformer_heads, S)
    close(sim, g["test_sim"], rtol=1e-3, atol=1e-4)
    close(sc, g["test_scores"], rtol=1e-3, atol=1e-5)
    lg, lt, scr, ia, in_, ba, rm, rv = O.anomaly_clip_forward_train(sd, hc, inp["train_feats"], inp["labels"], inp["nc"], eot,
                                                                    geom.transformer_heads, inp["mask"], inp["mask"])
    outs = O.compute_loss(lg, lt, inp["labels"], scr, ia, in_, ba, normal_id=hc.normal_id, num_topk=hc.num_topk,
                          num_segments=hc.num_segments, frames_per_segment=hc.seg_length)
    assert torch.equal(ia, T(g["idx_topk_abn"])) and torch.equal(in_, T(g["idx_topk_nor"]))
    assert torch.equal(ba, T(g["idx_bottomk_abn"]))
    close(lg, g["train_logits"], rtol=1e-3, atol=1e-4)
    close(lt, g["train_logits_topk"], rtol=1e-3, atol=1e-4)
    close(scr, g["train_scores"], rtol=1e-3, atol=1e-5)
    close(torch.stack([o.detach() for o in outs]), g["losses"], rtol=1e-4, atol=1e-6)
    close(rm, g["rm1"])
    close(rv, g["rv1"])


@pytest.mark.parametrize("N,L,want", [(64, 16, True), (16, 32, True), (64, 64, True), (16, 16, True), (24, 10, False),
                                      (48, 8, False), (20, 20, False)])
def test_x6_convs_on_other_grids(N, L, want):
    """"auto" keeps its rule: power-of-two grids of whole 256-row tiles run the plane convolutions, every other grid the f32 MFMA
    convolutions (the plane kernels index the grid with shifts)."""
    from anomalyclip_amd.components.temporal_model import TemporalModel
    m = TemporalModel(512, 256, 1, 8, None, 1, N, L)
    m.precision = "auto"
    assert m.x6_convs() is want
