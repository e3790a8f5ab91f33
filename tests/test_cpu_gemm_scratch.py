"""No device: acx_gemm_scratch -- what scratch acx_gemm's caller should bring, answered by the library beside its routes -- against
the frozen formulas the Python wrapper used to size it with (tests/gemm_scratch_ref.py), at the values a NULL context stands for
(256 workgroups, the options as acx_create sets them); and the wrapper holds no second copy of the rules any more."""
import ctypes as C
import inspect
import re

import pytest

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

import gemm_scratch_ref as GS


def query(d, allow_split=True, ctx=None):
    out = L.GemmScratch()
    out.workspace_bytes, out.counters = 12345, 7                         # (the query overwrites both)
    assert L.lib().acx_gemm_scratch(ctx, C.byref(d), int(allow_split), C.byref(out)) == 0
    return int(out.workspace_bytes), int(out.counters)


@pytest.mark.parametrize("name,kw", GS.f32_cases(), ids=[n for n, _ in GS.f32_cases()])
def test_plain_products_match_the_frozen_rules(name, kw):
    d = GS.desc(**kw)
    assert query(d) == GS.scratch_ref(d)
    assert query(d, allow_split=False) == (0, 0)


@pytest.mark.parametrize("name,kw", GS.x6_cases(), ids=[n for n, _ in GS.x6_cases()])
def test_plane_products_match_the_frozen_rules(name, kw):
    d = GS.desc(**kw)
    for split_k in (True, False):
        assert query(d, split_k) == GS.scratch_ref(d, split_k=split_k), split_k


def test_the_grid_reaches_every_rule():
    """the reference's answers over the grids: each block of the old wrapper code gives scratch somewhere and nothing somewhere"""
    plain = [GS.scratch_ref(GS.desc(**kw)) for _, kw in GS.f32_cases()]
    planes = [GS.scratch_ref(GS.desc(**kw)) for _, kw in GS.x6_cases()]
    assert any(b and c for b, c in plain) and any(b and not c for b, c in plain) and any(not b for b, _ in plain)
    assert any(b for b, _ in planes) and any(not b for b, _ in planes) and not any(c for _, c in planes)
    # the opt-in tail split (a context's option: the GPU file asks the library) answers on these grids, too
    tails = [GS.scratch_ref(GS.desc(**kw), tail_split=True) for _, kw in GS.x6_cases()]
    assert sum(1 for t, p in zip(tails, planes) if t != p) >= 4


def test_query_ignores_the_scratch_fields_and_refuses_nonsense():
    d = GS.desc(1078, 512, 2048)
    want = query(d)
    d.workspace, d.workspace_bytes, d.counters, d.n_counters = 0x20000, 64, 0x30000, 1
    assert query(d) == want and want[0] > 0
    assert d.workspace_bytes == 64                                       # (and writes nothing into the descriptor)
    out = L.GemmScratch()
    assert L.lib().acx_gemm_scratch(None, None, 1, C.byref(out)) == -1
    assert L.lib().acx_gemm_scratch(None, C.byref(d), 1, None) == -1
    d.M = 0
    assert L.lib().acx_gemm_scratch(None, C.byref(d), 1, C.byref(out)) == -1


def test_get_option_needs_a_context():
    v = C.c_int64(-5)
    assert L.lib().acx_get_option(None, L.OPT_SK_MAX_M, C.byref(v)) == -1 and v.value == -5


def test_wrapper_keeps_no_copy_of_the_rules():
    for name in ("SK_MAX_ROWS", "_X6_OPTS", "X6_MIN_TILES_DEFAULT", "ATTN_F32IN_DEFAULT", "CLS_FOLD_DEFAULT"):
        assert not hasattr(ops, name), name
    assert not [n for n in vars(ops) if n.endswith("_DEFAULT")]
    for fn in (ops.gemm, ops.gemm_x6):
        src = inspect.getsource(fn)
        assert "_bring_scratch(" in src
        assert not re.search(r"M\s*<=|tiles\s*<=?|tail_rows|few_rows|wgs|_splitk_workspace|_colsum_counters", src), fn.__name__
    src = inspect.getsource(ops._bring_scratch)
    assert "acx_gemm_scratch" in src and "_CTR_N - 1" in src and not re.search(r"<=|//|\bmin\(|\bmax\(", src)
