"""CPU: the algebra behind acx_attention_cls_fold in fp64 (tests/cls_fold_ref.py) -- the folded form equals the straightforward
LayerNorm -> K | V projection -> one-query attention to 1e-12 of max |ref| at every shape the GPU test runs, and the key bias
q_h . b_k, the same for every key of a (frame, head), changes nothing."""
import pytest
import torch

import cls_fold_ref as CF

CASES = [(s, None, None) for s in CF.SHAPES] + [((3, 197, 768), 40.0, None), ((3, 197, 768), None, 20.0)]


@pytest.mark.parametrize("shape,col_scale,q_scale", CASES)
def test_folded_form_equals_the_straightforward_one_fp64(shape, col_scale, q_scale):
    c = CF.make_inputs(*shape, col_scale=col_scale, q_scale=q_scale)
    ref, fold = CF.straight(c), CF.folded(c)
    assert ref.dtype == torch.float64 and torch.isfinite(ref).all()
    scale = ref.abs().max().item()
    err = (fold - ref).abs().max().item()
    print(shape, col_scale, q_scale, "fold - straight:", err / scale)
    assert err <= 1e-12 * scale
    if q_scale is not None:                                   # the wide-range case does span more than 80
        s = CF.scores_straight(c)
        assert (s.amax(-1) - s.amin(-1)).max().item() > 80.0


@pytest.mark.parametrize("shape", CF.SHAPES)
def test_key_bias_cancels_in_the_softmax(shape):
    c = CF.make_inputs(*shape)
    with_b, without_b = CF.straight(c, k_bias=True), CF.straight(c, k_bias=False)
    s1, s0 = CF.scores_straight(c, k_bias=True), CF.scores_straight(c, k_bias=False)
    shift = s1 - s0                                           # one constant per (frame, head), not zero
    assert (shift - shift[..., :1]).abs().max().item() <= 1e-12 * max(1.0, shift.abs().max().item())
    assert shift.abs().max().item() > 1e-3
    assert (with_b - without_b).abs().max().item() <= 1e-12 * with_b.abs().max().item()
