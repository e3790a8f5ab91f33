"""acx_transformer_plan (host arithmetic: no device, NULL context = the options acx_create sets) against tests/vit_plan_ref.py, the
restated gates of the walk the plan replaced, record for record; the three refusals the plan step takes over; and relations between
the fields of a plan's records that hold whatever the restatement says."""
import ctypes as C
import itertools

import pytest

from anomalyclip_amd import _lib as L
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops

import vit_plan_ref as R

PRECS = (L.PREC_F32, L.PREC_BF16, L.PREC_F32X6, L.PREC_F32X3, L.PREC_F16X3)
FRAMES = (1, 2, 7, 8, 9, 64, 160, 222, 256, 512)
VISION = {"ViT-B/16": IW.VIT_B16, "ViT-B/32": IW.VIT_B32, "ViT-L/14": IW.VIT_L14, "ViT-L/14@336": IW.VIT_L14_336, "TINY": IW.TINY}
PRODUCTS = ("in_proj", "out_proj", "fc", "proj")


def vision_shape(g):
    """(tokens, width, heads, layers) of a geometry's image encoder"""
    return (g.image_resolution // g.vision_patch_size) ** 2 + 1, g.vision_width, g.vision_width // 64, g.vision_layers


def grid():
    """(name, batch, L, W, heads, layers, causal, prec, prune, has_planes, ws_prec_sized)"""
    for (name, g), frames, prune in itertools.product(VISION.items(), FRAMES, (0, 1)):
        for prec, planes, sized in itertools.product(PRECS, (0, 1), (0, 1)):
            yield (f"{name}-{frames}f", frames) + vision_shape(g) + (0, prec, prune, planes, sized)
    for width, batch in itertools.product((512, 768), (14, 1)):
        for prec, planes, sized in itertools.product(PRECS, (0, 1), (0, 1)):
            yield (f"text-{width}-{batch}", batch, 77, width, width // 64, 12, 1, prec, 0, planes, sized)


GRID = list(grid())


def query(args, handle=None):
    """(rc, [record dict per layer], error text) of acx_transformer_plan for args = (batch, L, W, heads, layers, causal, prec, prune,
    has_planes, ws_prec_sized)"""
    layers = args[4]
    out = (L.TfLayerPlan * layers)()
    rc = L.lib().acx_transformer_plan(handle, *args, out)
    recs = [ops._struct_dict(out[l]) for l in range(layers)]
    for r in recs:
        assert r.pop("reserved") == 0
    return rc, recs, L.lib().acx_last_error(handle).decode()


_ZERO = {**dict.fromkeys(R.FIELDS, 0), **{p: {"kernel": 0, "c_dtype": 0, "scratch": 0, "ln_job": 0} for p in PRODUCTS}}
_PLANS = {}


def plan_of(case):
    if case not in _PLANS:
        _PLANS[case] = query(case[1:])
    return _PLANS[case]


def test_the_plan_is_the_restated_walk_on_the_whole_grid():
    assert len(GRID) == (5 * 10 * 2 + 4) * 5 * 2 * 2
    bad = []
    for case in GRID:
        rc, recs, text = plan_of(case)
        want_rc, want = R.plan_ref(*case[1:])
        if want_rc:
            ok = rc == want_rc and want in text and all(r == _ZERO for r in recs)
        else:
            ok = rc == 0 and recs == want
        if not ok:
            bad.append((case, rc, text if rc else [(l, k, a[k], b[k]) for l, (a, b) in enumerate(zip(recs, want)) for k in a if a[k] != b[k]][:4]))
    assert not bad, (len(bad), bad[:5])


@pytest.mark.parametrize("name,args,code,text", [
    # bf16 without the weights' bf16 copies: the in-projection's row product
    ("copy", (8, 197, 768, 12, 12, 0, L.PREC_BF16, 1, 0, 1), R.E_BADARG, "driver: missing bf16 weight copy for the requested precision"),
    # a plane mode whose products reach the plane kernel, without the weights' planes
    ("planes", (8, 197, 768, 12, 12, 0, L.PREC_F32X6, 1, 0, 1), R.E_BADARG, "driver: missing bf16 x 3 weight planes for ACX_PREC_F32X6"),
    # fp16 planes at 50 tokens (ViT-B/32, 512 frames): the products are the plane kernel's, the attention is not the planes attention
    ("f16x3", (512, 50, 768, 12, 12, 0, L.PREC_F16X3, 1, 1, 1), R.E_UNSUPPORTED,
     "driver: ACX_PREC_F16X3 needs the planes attention (192 < L <= 208) and all four products on the plane kernel"),
    # both apply: the in-projection's planes come first, then the fp16 gate, then the other products' planes
    ("planes-before-f16x3", (512, 50, 768, 12, 12, 0, L.PREC_F16X3, 1, 0, 1), R.E_BADARG, "driver: missing bf16 x 3 weight planes"),
])
def test_refusals(name, args, code, text):
    rc, recs, err = query(args)
    assert rc == code and text in err, (rc, err)
    assert all(r == _ZERO for r in recs)
    assert R.plan_ref(*args)[0] == code and R.plan_ref(*args)[1] in text


def test_query_arguments():
    assert L.lib().acx_transformer_plan(None, 8, 197, 768, 12, 12, 0, L.PREC_F32, 1, 1, 1, None) == R.E_BADARG
    out = (L.TfLayerPlan * 1)()
    assert L.lib().acx_transformer_plan(None, 0, 197, 768, 12, 1, 0, L.PREC_F32, 1, 1, 1, out) == R.E_BADARG
    assert L.lib().acx_transformer_plan(None, 8, 197, 768, 12, 0, 0, L.PREC_F32, 0, 1, 1, out) == 0       # no layers: nothing to say
    with pytest.raises(L.AcxError, match="ACX_PREC_F16X3 needs the planes attention"):
        ops.transformer_plan(512, 50, 768, 12, 12, prec=L.PREC_F16X3, prune_last=True)
    recs = ops.transformer_plan(8, 197, 768, 12, 12, prec=L.PREC_F32X6, prune_last=True)
    assert len(recs) == 12 and recs[0]["att"] == L.TF_ATT_P3F and recs[-1]["pruned"] == 1 and recs[1]["in_proj"]["kernel"] == L.TF_GEMM_X6


def _is_planes(dtype):
    return dtype in (L.BF16X3P, L.F16X2P)


def test_relations_between_the_records():
    seen = 0
    for case in GRID:
        rc, recs, _ = plan_of(case)
        if rc:
            continue
        seen += 1
        for l, r in enumerate(recs):
            last = l == len(recs) - 1
            # ln_1 rides exactly when the previous layer's c_proj runs on the plane kernel and carries the job
            prev = recs[l - 1]["proj"] if l else {"kernel": L.TF_GEMM_ROWS, "ln_job": 0}
            assert (r["ln1"] == L.TF_LN_RIDDEN) == (prev["kernel"] == L.TF_GEMM_X6 and prev["ln_job"] == 1), (case, l)
            assert not (last and r["proj"]["ln_job"]), (case, l)
            # ... and ln_2 when this layer's out-projection does
            assert (r["ln2"] == L.TF_LN_RIDDEN) == (r["out_proj"]["kernel"] == L.TF_GEMM_X6 and r["out_proj"]["ln_job"] == 1), (case, l)
            for p in PRODUCTS:                        # only the plane kernel carries a job, writes planes or borrows an f32 buffer
                if r[p]["kernel"] == L.TF_GEMM_ROWS:
                    assert r[p]["ln_job"] == 0 and not _is_planes(r[p]["c_dtype"]) and r[p]["scratch"] in (L.TF_BUF_NONE, L.TF_BUF_SPLITK), (case, l, p)
                else:
                    assert r[p]["scratch"] in (L.TF_BUF_NONE, L.TF_BUF_H, L.TF_BUF_QKV, L.TF_BUF_MLP), (case, l, p)
            # an attention that writes planes is never followed by the split of its output
            if r["att"] in (L.TF_ATT_X3_PANEL, L.TF_ATT_P3N, L.TF_ATT_P3F):
                assert r["split_att"] == 0 and r["out_proj"]["kernel"] == L.TF_GEMM_X6, (case, l)
            assert r["split_att"] == int(not r["pruned"] and r["out_proj"]["kernel"] == L.TF_GEMM_X6
                                         and r["att"] not in (L.TF_ATT_X3_PANEL, L.TF_ATT_P3N, L.TF_ATT_P3F)), (case, l)
            # the planes attention reads planes exactly when the in-projection writes them
            assert (r["att"] == L.TF_ATT_P3N) == _is_planes(r["in_proj"]["c_dtype"]), (case, l)
            assert (r["att_products"] != 0) == (r["att"] == L.TF_ATT_P3N) and r["att_products"] in (0, 3, 6, 103), (case, l)
            # c_fc writes planes exactly when c_proj reads them without a split in between
            assert _is_planes(r["fc"]["c_dtype"]) == (r["proj"]["kernel"] == L.TF_GEMM_X6 and not r["split_mlp"]), (case, l)
            assert r["split_mlp"] == int(r["proj"]["kernel"] == L.TF_GEMM_X6 and r["fc"]["kernel"] == L.TF_GEMM_ROWS), (case, l)
            # LayerNorm writes planes exactly for a product on the plane kernel
            assert (r["ln1"] in (L.TF_LN_PLANES, L.TF_LN_RIDDEN)) == (r["in_proj"]["kernel"] == L.TF_GEMM_X6), (case, l)
            assert (r["ln2"] in (L.TF_LN_PLANES, L.TF_LN_RIDDEN)) == (r["fc"]["kernel"] == L.TF_GEMM_X6), (case, l)
            # at most one pruned layer, the last, and only where asked for
            assert r["pruned"] == int(bool(case[8]) and last), (case, l)
            assert (r["att"] in (L.TF_ATT_CLS, L.TF_ATT_CLS_FOLD)) == bool(r["pruned"]) == (r["ln2"] == L.TF_LN_CLS), (case, l)
            assert r["ln1"] != L.TF_LN_CLS or r["att"] == L.TF_ATT_CLS_FOLD, (case, l)
        # one shape for every body layer but the first, the last and the one in front of a pruned last layer
        for a, b in zip(recs[1:-3], recs[2:-2]):
            assert a == b, case
    assert seen > len(GRID) // 2


def test_a_fall_back_plan_is_the_f32_plan():
    """a plane mode with an f32-sized workspace launches what ACX_PREC_F32 launches"""
    for case in GRID:
        name, *args = case
        if args[6] in (L.PREC_F32X6, L.PREC_F32X3, L.PREC_F16X3) and not args[9]:
            f32 = tuple(args[:6]) + (L.PREC_F32,) + tuple(args[7:])
            assert plan_of(case)[:2] == query(f32)[:2], case


def test_every_value_of_every_enum_is_reported():
    seen = {k: set() for k in ("ln", "kernel", "scratch", "att", "ln_dtype", "c_dtype", "products")}
    for case in GRID:
        rc, recs, _ = plan_of(case)
        for r in recs if rc == 0 else ():
            seen["ln"] |= {r["ln1"], r["ln2"]}
            seen["ln_dtype"] |= {r["ln1_dtype"], r["ln2_dtype"]}
            seen["att"].add(r["att"])
            seen["products"].add(r["att_products"])
            for p in PRODUCTS:
                seen["kernel"].add(r[p]["kernel"])
                seen["scratch"].add(r[p]["scratch"])
                seen["c_dtype"].add(r[p]["c_dtype"])
    assert seen["ln"] == {L.TF_LN_ROWS, L.TF_LN_PLANES, L.TF_LN_RIDDEN, L.TF_LN_CLS}
    assert seen["kernel"] == {L.TF_GEMM_ROWS, L.TF_GEMM_X6}
    assert seen["scratch"] == {L.TF_BUF_NONE, L.TF_BUF_SPLITK, L.TF_BUF_H, L.TF_BUF_QKV, L.TF_BUF_MLP}
    assert seen["att"] == {L.TF_ATT_F32, L.TF_ATT_BF16, L.TF_ATT_X3_PANEL, L.TF_ATT_P3N, L.TF_ATT_P3F, L.TF_ATT_CLS, L.TF_ATT_CLS_FOLD}
    assert seen["ln_dtype"] == {L.ACX_F32, L.ACX_BF16, L.BF16X3P, L.BF16X2P, L.F16X2P}
    assert seen["c_dtype"] == {L.ACX_F32, L.ACX_BF16, L.BF16X3P, L.F16X2P}
    assert seen["products"] == {0, 3, 103}          # (6: ACX_OPT_ATTN_F32IN = 0, test_gpu_vit_plan.py)
