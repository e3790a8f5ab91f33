"""Seeded inputs and head configurations of the segment-grid fixtures (e2e_grid_*.npz), shared by make_golden_grid.py (which
feeds them to the REFERENCE) and by the grid tests (which feed them to the oracle and to the HIP path).  Pure torch; no reference
import.  recipes.py keeps the 32 x 16 recipes as they are."""
import torch

from anomalyclip_amd import init_weights as IW

# tag -> (HeadConfig, segment_size S of the test-mode run, seed): the reference AnomalyCLIP with the tiny CLIP geometry
GRIDS = {
    "24x10": (IW.HeadConfig(num_classes=14, normal_id=7, num_segments=24, seg_length=10, emb_size=64, heads=2, depth=1), 2, 71),
    "64x16": (IW.HeadConfig(num_classes=14, normal_id=7, num_segments=64, seg_length=16, emb_size=64, heads=2, depth=1), 1, 72),
    "48x8": (IW.HeadConfig(num_classes=14, normal_id=7, num_segments=48, seg_length=8, emb_size=64, heads=2, dim_heads=16, depth=2,
                           concat_features=True), 2, 73),
}
LABELS = (2, 11, 7, 7)


def grid_inputs(seed: int, D: int, hc, S: int):
    """nc [D]; test_feats (1, 1, N L S, D); train_feats (4, 1, N L, D) with labels LABELS; mask (4, N) ~ Bernoulli(0.3) with the first
    num_topk segments forced on (top-k and bottom-k then never meet a tie among masked-out zeros)."""
    N, L = hc.num_segments, hc.seg_length
    g = torch.Generator().manual_seed(seed + 1)
    nc = torch.randn(D, generator=g) * 0.1
    test_feats = torch.randn(1, 1, N * L * S, D, generator=g) * 0.3
    g3 = torch.Generator().manual_seed(seed + 3)
    train_feats = torch.randn(len(LABELS), 1, N * L, D, generator=g3) * 0.3
    g4 = torch.Generator().manual_seed(seed + 4)
    mask = torch.bernoulli(torch.ones(len(LABELS), N) * 0.3, generator=g4)
    mask[:, :max(hc.num_topk, hc.num_bottomk)] = 1
    return dict(nc=nc, test_feats=test_feats, train_feats=train_feats, labels=torch.tensor(LABELS), mask=mask)
