"""-m gpu: the context's options read back (acx_get_option), acx_gemm_scratch with a real context against the frozen rules of the old
wrapper (tests/gemm_scratch_ref.py) under the options that move its answer, and ops.gemm / ops.gemm_x6 -- which now ask the
library what scratch to bring -- bitwise equal to acx_gemm called directly with the scratch those frozen rules decide on."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

import gemm_scratch_ref as GS

DEV = "cuda"

# ACX_OPT_*: (what acx_create sets, another value the setter accepts)
OPTIONS = {L.OPT_RING_MIN_TILES: (512, 7), L.OPT_SK_MAX_M: (320, 0), L.OPT_TN_P256_MIN_ROWS: (4096, 123), L.OPT_X6_CUS: (0, 37),
           L.OPT_X6_TAIL_SPLIT: (0, 1), L.OPT_X6_STRIP_TAIL: (1, 3), L.OPT_X6_MIN_TILES: (18, 5), L.OPT_LN_RIDER: (1, 1 << 33),
           L.OPT_ATTN_F32IN: (1, 0), L.OPT_CLS_FOLD: (1, 0)}


@pytest.fixture()
def fresh_ctx():
    """a context of its own: the options of the one the package works with stay untouched"""
    lib, h = L.lib(), C.c_void_p()
    assert lib.acx_create(C.byref(h), torch.cuda.current_device()) == 0
    try:
        yield h
    finally:
        lib.acx_destroy(h)


def _get(h, opt):
    v = C.c_int64(-1)
    assert L.lib().acx_get_option(h, opt, C.byref(v)) == 0, opt
    return int(v.value)


def test_option_round_trip(fresh_ctx):
    lib, h = L.lib(), fresh_ctx
    assert len(OPTIONS) == 10
    for opt, (default, other) in OPTIONS.items():
        before = _get(h, opt)
        assert before == default, opt
        try:
            assert lib.acx_set_option(h, opt, other) == 0
            assert _get(h, opt) == other, opt
        finally:
            assert lib.acx_set_option(h, opt, before) == 0
        assert _get(h, opt) == default, opt
    v = C.c_int64(-1)
    assert lib.acx_get_option(h, 11, C.byref(v)) == -2 and lib.acx_set_option(h, 11, 1) == -2      # ACX_E_UNSUPPORTED, both
    assert b"unknown option" in lib.acx_last_error(h)
    # the package's own context through the wrapper: a setter is seen by get_option, x6_options and x6_workgroups
    dev = torch.cuda.current_device()
    ncu = torch.cuda.get_device_properties(dev).multi_processor_count
    before = ops.x6_options(dev)
    try:
        ops.set_x6_cus(dev, 7)
        ops.set_x6_tail_split(dev, True)
        assert ops.x6_options(dev) == {"cus": 7, "tail_split": True} and ops.x6_workgroups(dev) == 7
        assert ops.get_option(dev, L.OPT_X6_CUS) == 7
    finally:
        ops.set_x6_cus(dev, before["cus"])
        ops.set_x6_tail_split(dev, before["tail_split"])
    assert ops.x6_options(dev) == before and ops.x6_workgroups(dev) == (min(ncu, before["cus"]) if before["cus"] else ncu)


def _query(h, d, allow_split=True):
    out = L.GemmScratch()
    assert L.lib().acx_gemm_scratch(h, C.byref(d), int(allow_split), C.byref(out)) == 0
    return int(out.workspace_bytes), int(out.counters)


def test_query_follows_the_context_options(fresh_ctx):
    """host arithmetic only: the pairs = 6 / 3 grid and a text-tower product under the options the scratch rules read"""
    lib, h = L.lib(), fresh_ctx
    ncu = torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count
    cases = GS.x6_cases() + [("f32-539x512x2048", dict(M=539, N=512, K=2048))]
    settings = [{}, {L.OPT_X6_CUS: 7}, {L.OPT_X6_CUS: ncu - 32}, {L.OPT_X6_TAIL_SPLIT: 1}, {L.OPT_SK_MAX_M: 0}]
    answers = []
    for setting in settings:
        before = {opt: _get(h, opt) for opt in setting}
        try:
            for opt, value in setting.items():
                assert lib.acx_set_option(h, opt, value) == 0
            kw = dict(ncu=ncu, sk_max_m=_get(h, L.OPT_SK_MAX_M), x6_cus=_get(h, L.OPT_X6_CUS), tail_split=_get(h, L.OPT_X6_TAIL_SPLIT))
            got = []
            for name, dkw in cases:
                d = GS.desc(**dkw)
                for split_k in (True, False):
                    got.append(_query(h, d, split_k))
                    assert got[-1] == GS.scratch_ref(d, split_k=split_k, **kw), (setting, name, split_k)
            answers.append(got)
        finally:
            for opt, value in before.items():
                assert lib.acx_set_option(h, opt, value) == 0
    assert all(a != answers[0] for a in answers[1:])                     # every one of the settings moves some answer


def _direct(d, device, ref):
    """acx_gemm on a hand-filled descriptor with the scratch the frozen rules decide on, taken as the old wrapper took it"""
    nbytes, counters = ref
    if nbytes:
        ws = ops._splitk_workspace(device, nbytes)
        d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel()
    if counters:
        ctr = ops._colsum_counters(device)
        d.counters, d.n_counters = ctr.data_ptr(), ops._CTR_N - 1
    h = L.ctx(device.index if device.index is not None else torch.cuda.current_device())
    L.check(L.lib().acx_gemm(h, C.byref(d), torch.cuda.current_stream().cuda_stream), h)
    torch.cuda.synchronize()


CONV = dict(amap=L.AMAP_CONV3X3, gn=16, gl=16, cin=64)
# (name, M, N, K, pairs, convolution, the rule it stands for: scratch and counters the frozen rules must give)
BIT_CASES = [("few-row pieces", 77, 512, 2048, 0, False, (True, 1)), ("s64 split", 1078, 512, 2048, 0, False, (True, 0)),
             ("x6 split", 256, 768, 768, 6, False, (True, 0)), ("f32 conv split", 256, 128, 576, 0, True, (True, 1)),
             ("x6 conv split", 256, 128, 576, 6, True, (True, 0))]


@pytest.mark.parametrize("name,M,N,K,pairs,conv,rule", BIT_CASES, ids=[c[0] for c in BIT_CASES])
def test_wrapper_bit_identical_to_the_frozen_decision(name, M, N, K, pairs, conv, rule):
    dev_i = torch.cuda.current_device()
    ncu = torch.cuda.get_device_properties(dev_i).multi_processor_count
    g = torch.Generator(device=DEV).manual_seed(M + N + K + pairs)
    a = torch.randn(M, 64 if conv else K, generator=g, device=DEV) * torch.exp2(torch.randint(-3, 3, (M, 1), generator=g, device=DEV).float())
    w = torch.randn(N, K, generator=g, device=DEV) * K ** -0.5
    bias = torch.randn(N, generator=g, device=DEV)
    kw = CONV if conv else {}
    if pairs:
        a_, w_ = ops.split_bf16x3(a), ops.split_bf16x3(w)
        y = ops.gemm_x6(a_, w_, bias=bias, **kw)
    else:
        a_, w_ = a, w
        y = ops.gemm(a_, w_, bias=bias, **kw)
    d = GS.desc(M, N, K, pairs=pairs, **kw)
    opts = dict(ncu=ncu, sk_max_m=ops.get_option(dev_i, L.OPT_SK_MAX_M), x6_cus=ops.get_option(dev_i, L.OPT_X6_CUS),
                tail_split=ops.get_option(dev_i, L.OPT_X6_TAIL_SPLIT))
    ref = GS.scratch_ref(d, **opts)
    assert (ref[0] > 0, ref[1]) == rule, ref
    out = torch.full_like(y, float("nan"))
    d.A, d.W, d.C, d.bias = a_.data_ptr(), w_.data_ptr(), out.data_ptr(), bias.data_ptr()
    if conv:
        d.zero_page = ops._zero_page(a.device).data_ptr()
    _direct(d, a.device, ref)
    assert torch.equal(y, out)                                           # (out was all NaN: equal means every element was written)
