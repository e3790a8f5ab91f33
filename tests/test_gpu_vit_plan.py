"""-m gpu: the transformer driver's plan step on a real context -- acx_transformer_plan follows the context's options as the
restated walk (tests/vit_plan_ref.py) does; a refusal of the plan precedes the first launch; a plane mode that is handed an f32-sized
workspace computes what ACX_PREC_F32 computes, bit for bit."""
import ctypes as C
import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops
from anomalyclip_amd.components.clip_vit import Transformer

import test_cpu_vit_plan as P
import vit_plan_ref as R

DEV = "cuda"
OPTS = (L.OPT_X6_MIN_TILES, L.OPT_ATTN_F32IN, L.OPT_CLS_FOLD)


class options:
    """the three options the plan reads, set for a block and put back behind it"""

    def __init__(self, min_tiles, f32in, fold):
        self.values = (min_tiles, f32in, fold)

    def __enter__(self):
        self.dev = torch.cuda.current_device()
        self.before = [ops.get_option(self.dev, o) for o in OPTS]
        self.h = L.ctx(self.dev)
        for o, v in zip(OPTS, self.values):
            L.check(L.lib().acx_set_option(self.h, o, int(v)), self.h)
        return self.h

    def __exit__(self, *exc):
        for o, v in zip(OPTS, self.before):
            L.check(L.lib().acx_set_option(self.h, o, int(v)), self.h)


CUT = [c for c in P.GRID if c[0] in ("ViT-B/16-2f", "ViT-B/16-8f", "TINY-8f", "text-512-14", "text-768-14")]


@pytest.mark.parametrize("min_tiles,f32in,fold", list(itertools.product((1, 18, 2 ** 31 - 1), (0, 1), (0, 1))))
def test_the_plan_follows_the_contexts_options(min_tiles, f32in, fold):
    assert len(CUT) == (3 * 2 + 2) * 5 * 2 * 2
    bad, products = [], set()
    with options(min_tiles, f32in, fold) as h:
        for case in CUT:
            rc, recs, text = P.query(case[1:], h)
            want_rc, want = R.plan_ref(*case[1:], x6_min_tiles=min_tiles, attn_f32in=f32in, cls_fold=fold)
            ok = (rc == want_rc and want in text and all(r == P._ZERO for r in recs)) if want_rc else (rc == 0 and recs == want)
            if not ok:
                bad.append((case, rc, text))
            products |= {r["att_products"] for r in recs}
    assert not bad, (len(bad), bad[:5])
    assert (6 in products) == (f32in == 0 and min_tiles <= 18)          # six products on planes: only without the f32-fed attention


def _transformer(width, heads, layers, seed=5):
    torch.manual_seed(seed)
    return Transformer(width, layers, heads).to(DEV)


def _forward(t, x, batch, seq, prec, nbytes):
    """acx_transformer_forward in place on a copy of x with a workspace of nbytes; (rc, output, error text)"""
    lib = L.lib()
    y = x.clone()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    arr, _keep = t.block_table(prec)
    h = ops._h(y)
    rc = lib.acx_transformer_forward(h, y.data_ptr(), batch, seq, t.width, t.heads, t.layers, 0, prec, arr, ws.data_ptr(), nbytes, ops._stream())
    torch.cuda.synchronize()
    return rc, y, lib.acx_last_error(h).decode()


def test_a_refusal_precedes_the_first_launch():
    """fp16 planes at 64 tokens with every product on the plane kernel (min tiles 1): outside the planes attention's range.  The walk
    this plan replaced refused here after ln_1 and the in-projection of layer 0 had been launched."""
    width, heads, layers, seq, batch = 256, 4, 2, 64, 8
    t = _transformer(width, heads, layers)
    x = torch.randn(batch * seq, width, device=DEV)
    lib = L.lib()
    with options(1, 1, 1) as h:
        nbytes = lib.acx_transformer_workspace_bytes_prec(width, batch * seq, L.PREC_F16X3)
        counts, ms = (C.c_int32 * 4)(), (C.c_double * 4)()
        t.block_table(L.PREC_F16X3)                # (cached: the weights' planes are split before the recording starts)
        L.check(lib.acx_prof_enable(h, 1), h)
        try:
            rc, y, text = _forward(t, x, batch, seq, L.PREC_F16X3, nbytes)
            L.check(lib.acx_prof_collect(h, counts, ms), h)
        finally:
            lib.acx_prof_enable(h, 0)
    assert rc == R.E_UNSUPPORTED, (rc, text)
    assert "driver: ACX_PREC_F16X3 needs the planes attention (192 < L <= 208) and all four products on the plane kernel" in text
    assert list(counts) == [0, 0, 0, 0], list(counts)
    assert torch.equal(y, x)


def test_a_plane_mode_on_an_f32_sized_workspace_is_the_f32_mode():
    width, heads, layers, seq, batch = 256, 4, 2, 200, 2
    t = _transformer(width, heads, layers)
    x = torch.randn(batch * seq, width, device=DEV)
    lib = L.lib()
    with options(1, 1, 1) as h:
        big = lib.acx_transformer_workspace_bytes_prec(width, batch * seq, L.PREC_F32X6)
        small = lib.acx_transformer_workspace_bytes(width, batch * seq)
        assert small < big
        plan = P.query((batch, seq, width, heads, layers, 0, L.PREC_F32X6, 0, 1, 1), h)[1]
        assert all(r[p]["kernel"] == L.TF_GEMM_X6 for r in plan for p in P.PRODUCTS) and plan[0]["att"] == L.TF_ATT_P3F
        rc6, y6, text6 = _forward(t, x, batch, seq, L.PREC_F32X6, big)
        rcs, ys, texts = _forward(t, x, batch, seq, L.PREC_F32X6, small)
        rcf, yf, textf = _forward(t, x, batch, seq, L.PREC_F32, small)
    assert (rc6, rcs, rcf) == (0, 0, 0), (text6, texts, textf)
    assert torch.isfinite(y6).all() and not torch.equal(y6, x)
    assert torch.equal(ys, yf), int((ys != yf).sum())
    assert not torch.equal(y6, yf)                                  # (the plane kernels did run with the workspace they need)
    assert (y6 - yf).abs().max().item() <= 1e-3 * yf.abs().max().item()
