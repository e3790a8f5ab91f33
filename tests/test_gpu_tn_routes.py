"""-m gpu: acx_gemm_tn / _zp / _parts / _group and acx_gemm_tn_x6 on every row of tests/tn_ref.py's table -- the route asserted with
acx_gemm_tn_route / acx_gemm_tn_x6_route on the live context, then EVERY element of C finite and within bound() of the fp64
reference (no norm, no allowance for outliers); C's guard rows, the operands' pad columns and guard rows and the workspace beyond the
route's need still their NaN pattern bit for bit; split rows run twice and torch.equal.  The arguments are filled by hand through
ctypes: padded leading dimensions, a workspace poisoned with NaN before every call (a partial image that is summed without having
been written shows), the zero page brought or withheld per row.  Refusal rows: the query and the call answer the same code and
text, and nothing is written."""
import ctypes as C
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops

import tn_ref as T

DEV = "cuda"
WS_GUARD = 4096                                          # poisoned bytes behind workspace_bytes
WORST = {}                                               # kernel -> (worst |err| / bound, row): printed by the last test
T0 = [0.0]                                               # when the file's first test began


@pytest.fixture(scope="module")
def own_ctx():
    """a context of the file's own: the options the rows set never reach the one the package works with"""
    lib, h = L.lib(), C.c_void_p()
    T0[0] = time.time()
    assert lib.acx_create(C.byref(h), torch.cuda.current_device()) == 0
    assert torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count == T.NCU
    try:
        yield h
    finally:
        lib.acx_destroy(h)


class _Options:
    def __init__(self, h, opts):
        self.h, self.opts, self.before = h, opts, {}

    def __enter__(self):
        lib = L.lib()
        for opt, value in self.opts.items():
            v = C.c_int64(-1)
            assert lib.acx_get_option(self.h, opt, C.byref(v)) == 0
            self.before[opt] = int(v.value)
            assert lib.acx_set_option(self.h, opt, value) == 0

    def __exit__(self, *exc):
        for opt, value in self.before.items():
            assert L.lib().acx_set_option(self.h, opt, value) == 0


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _sync_or_end(rc, h, what):
    """a launch or device error: nothing more is started on this GPU"""
    try:
        L.check(rc, h)
        torch.cuda.synchronize()
    except Exception as e:
        pytest.exit(f"device error in {what}, the session ends here: {e}", returncode=3)


def _workspace(nbytes):
    """workspace_bytes + a guard, all of it the NaN pattern: (buffer as int32, pointer or None)"""
    if not nbytes:
        return None, None
    assert nbytes % 4 == 0
    ws = torch.full(((nbytes + WS_GUARD) // 4,), T.NAN32, dtype=torch.int32, device=DEV)
    return ws, ws.data_ptr()


def _intact_from(ws, nbytes):
    return ws is None or bool((ws[nbytes // 4:] == T.NAN32).all())


def _planes(x, ld):
    """the three bf16 planes of x [M, n] inside a poisoned [3, M + 2, ld] buffer -> (buffer, plane stride in bytes)"""
    p = ops.split_bf16x3(x.contiguous())
    buf = T._poison(3 * (x.shape[0] + 2), ld, torch.bfloat16, DEV).view(3, x.shape[0] + 2, ld)
    buf[:, :x.shape[0], :x.shape[1]] = p
    return buf, (x.shape[0] + 2) * ld * 2


def _planes_intact(buf, rows, cols):
    return all(T.guards_intact(buf[i], rows, cols) for i in range(3))


def _call(h, c, t, entry=None):
    """the row's call with the row's (refusal rows: overwritten) arguments -> (return code, splits_out or None)"""
    lib, a = L.lib(), T.call_args(c)
    t["ws"], wsp = _workspace(a["ws"] if a["has_ws"] else 0)
    if "zero" not in t:
        t["zero"] = torch.zeros(256, dtype=torch.float32, device=DEV)
    zp = t["zero"].data_ptr() if a["has_zp"] else None
    if c.x6:
        if "a3" not in t:
            t["a3"], t["a3_stride"] = _planes(t["a"], c.lda)
            t["b3"], t["b3_stride"] = _planes(t["b"], c.ldb)
        return lib.acx_gemm_tn_x6(h, t["a3"].data_ptr(), t["a3_stride"], a["lda"], t["b3"].data_ptr(), t["b3_stride"], a["ldb"],
                                  t["c_buf"].data_ptr(), a["ldc"], a["M"], a["N1"], a["N2"], a["conv"], a["gn"], a["gl"], a["cin"], wsp,
                                  a["ws"] if a["has_ws"] else 0, zp, _stream()), None
    bsub = t["b_sub"].data_ptr() + a["bsub_off"] if c.b_sub else None
    head = (h, t["a_buf"].data_ptr() + a["a_off"], a["lda"], t["b_buf"].data_ptr(), a["ldb"], t["c_buf"].data_ptr(), a["ldc"], a["M"],
            a["N1"], a["N2"], bsub, a["conv"], a["gn"], a["gl"], a["cin"], wsp, a["ws"] if a["has_ws"] else 0)
    if entry == "parts" or (entry is None and c.parts):
        n = C.c_int32(-1)
        return lib.acx_gemm_tn_parts(*head, zp, C.byref(n), _stream()), n
    if a["has_zp"] or entry == "zp":
        return lib.acx_gemm_tn_zp(*head, zp, _stream()), None
    return lib.acx_gemm_tn(*head, _stream()), None        # the plain entry: the library owns the zero page


def _run(h, c, entry=None):
    """-> (the operands with C written, splits_out)"""
    t = T.operands(c, DEV)
    rc, got, clears = T.query(h, c)
    assert rc == 0 and got == c.expect and clears == int(c.clears), (c.name, "got", T.KERNEL_NAMES[got[0]], got[1:], clears, "want",
                                                                    T.KERNEL_NAMES[c.expect[0]], c.expect[1:])
    rc, n = _call(h, c, t, entry)
    assert rc not in (T.E_BADARG, T.E_UNSUPPORTED, T.E_WORKSPACE), (c.name, L.lib().acx_last_error(h))
    _sync_or_end(rc, h, f"row {c.name}")
    return t, n


def _operands_intact(c, t):
    ok = T.guards_intact(t["a_buf"], c.M, c.N1) and T.guards_intact(t["b_buf"], c.M, c.kb)
    if c.x6:
        ok = ok and _planes_intact(t["a3"], c.M, c.N1) and _planes_intact(t["b3"], c.M, c.kb)
    return ok and int(t["zero"].view(torch.int32).abs().sum()) == 0


def _ratio(c, out, r, S):
    assert bool(torch.isfinite(out).all()), c.name
    return ((out.double() - r).abs() / T.bound(c, S).clamp_min(1e-300)).max().item()


@pytest.mark.parametrize("c", T.RUN_CASES, ids=[c.name for c in T.RUN_CASES])
def test_every_element_against_fp64(c, own_ctx):
    with _Options(own_ctx, c.opts):
        t, n = _run(own_ctx, c)
        r, S = T.ref(c, t)
        splits = c.expect[1]
        if c.parts:
            assert n.value == splits
        if c.parts and splits > 1:
            # the images stay in the workspace and C is not touched; their f32 sum in image order is what _zp writes, bit for bit
            assert T.guards_intact(t["c_buf"], 0, 0), c.name
            img = t["ws"][:splits * c.N1 * c.N2].view(torch.float32).view(splits, c.N1, c.N2)
            out = img[0].clone()
            for k in range(1, splits):
                out = out + img[k]
            tz, _ = _run_as_zp(own_ctx, c)
            assert torch.equal(out, tz["c"]), c.name
        else:
            out = t["c"]
        ratio = _ratio(c, out, r, S)
        print(f"tn-route-ratio {T.KERNEL_NAMES[c.expect[0]]} {c.name} {ratio:.4f}")
        if ratio > WORST.get(c.expect[0], (0.0, ""))[0]:
            WORST[c.expect[0]] = (ratio, c.name)
        assert ratio <= 1.0, (c.name, ratio)
        assert T.guards_intact(t["c_buf"], 0 if c.parts and splits > 1 else c.N1, c.N2), c.name
        assert _operands_intact(c, t), c.name
        assert _intact_from(t["ws"], c.ws_need), c.name
        if c.clears:                                      # the page the library cleared behind its images
            z0 = c.ws_need - T.ZERO_B
            assert int(t["ws"][z0 // 4:c.ws_need // 4].abs().sum()) == 0, c.name
        if splits > 1 and not c.parts:                    # the row ranges are summed in a fixed order
            again, _ = _run(own_ctx, c)
            assert torch.equal(out, again["c"]), c.name


def _run_as_zp(h, c):
    """the same problem through acx_gemm_tn_zp (the reduce launch sums the images)"""
    import dataclasses
    z = dataclasses.replace(c, parts=False, expect=c.expect[:4] + (T.RED_LAUNCH,))
    return _run(h, z, entry="zp")


@pytest.mark.parametrize("c", T.REFUSALS, ids=[c.name for c in T.REFUSALS])
def test_refusals_write_nothing(c, own_ctx):
    lib = L.lib()
    t = T.operands(c, DEV)
    if not c.call_only:
        rc, got, _ = T.query(own_ctx, c)
        assert rc == c.refuse and got == T.NO_ROUTE, (rc, got)
        assert c.text.encode() in lib.acx_last_error(own_ctx)
    rc, _ = _call(own_ctx, c, t)
    assert rc == c.refuse, (rc, lib.acx_last_error(own_ctx))
    assert c.text.encode() in lib.acx_last_error(own_ctx)
    torch.cuda.synchronize()
    assert T.guards_intact(t["c_buf"], 0, 0) and _intact_from(t["ws"], 0)


def test_parts_refuses_a_null_splits_out(own_ctx):
    lib, c = L.lib(), T.by_name("parts-w8-bsub")
    t = T.operands(c, DEV)
    ws, wsp = _workspace(c.ws_bytes)
    rc = lib.acx_gemm_tn_parts(own_ctx, t["a_buf"].data_ptr(), c.lda, t["b_buf"].data_ptr(), c.ldb, t["c_buf"].data_ptr(), c.N2, c.M, c.N1,
                               c.N2, t["b_sub"].data_ptr(), 0, 0, 0, 0, wsp, c.ws_bytes, None, None, _stream())
    assert rc == T.E_BADARG and b"null splits_out" in lib.acx_last_error(own_ctx)
    torch.cuda.synchronize()
    assert T.guards_intact(t["c_buf"], 0, 0) and _intact_from(ws, 0)


def _group_table(cases, ts):
    arr = (L.TnProblem * len(cases))()
    for i, (c, t) in enumerate(zip(cases, ts)):
        arr[i].A, arr[i].B, arr[i].C = t["a_buf"].data_ptr(), t["b_buf"].data_ptr(), t["c_buf"].data_ptr()
        arr[i].b_sub = t["b_sub"].data_ptr() if c.b_sub else None
        arr[i].M, arr[i].N1, arr[i].N2, arr[i].lda, arr[i].ldb = c.M, c.N1, c.N2, c.lda, c.ldb
    return arr


def test_group_equals_the_single_launches(own_ctx):
    """ten problems = two launches of at most eight: every output within the fp64 bound and torch.equal to its own acx_gemm_tn_zp
    launch; the workspace behind acx_gemm_tn_group_workspace_bytes untouched"""
    lib = L.lib()
    cases = [T.by_name(n) for n in T.GROUP]
    ts = [T.operands(c, DEV) for c in cases]
    arr = _group_table(cases, ts)
    pa = C.cast(arr, C.c_void_p)
    need = int(lib.acx_gemm_tn_group_workspace_bytes(len(cases), pa))
    assert need == sum((c.expect[1] * c.N1 * c.N2 * 4 + 255) // 256 * 256 for c in cases if c.expect[1] > 1)
    ws, wsp = _workspace(need)
    rc = lib.acx_gemm_tn_group(own_ctx, len(cases), pa, wsp, need, _stream())
    assert rc == 0, lib.acx_last_error(own_ctx)
    _sync_or_end(rc, own_ctx, "acx_gemm_tn_group")
    assert _intact_from(ws, need)
    off = 0                                               # each split problem's images begin on a 256-byte boundary: the gaps stay NaN
    for c in cases:
        if c.expect[1] > 1:
            used = c.expect[1] * c.N1 * c.N2 * 4
            assert not bool(ws[off // 4:(off + used) // 4].view(torch.float32).isnan().any()), c.name
            off += used
            gap = -off % 256
            assert bool((ws[off // 4:(off + gap) // 4] == T.NAN32).all()), c.name
            off += gap
    assert off == need and any(c.expect[1] > 1 and (c.expect[1] * c.N1 * c.N2 * 4) % 256 for c in cases)
    for c, t in zip(cases, ts):
        r, S = T.ref(c, t)
        ratio = _ratio(c, t["c"], r, S)
        print(f"tn-route-ratio group {c.name} {ratio:.4f}")
        assert ratio <= 1.0, (c.name, ratio)
        assert T.guards_intact(t["c_buf"], c.N1, c.N2) and T.guards_intact(t["a_buf"], c.M, c.N1) and T.guards_intact(t["b_buf"], c.M, c.N2)
        single, _ = _run(own_ctx, c, entry="zp")
        assert torch.equal(t["c"], single["c"]), c.name


def test_group_refusals(own_ctx):
    lib = L.lib()
    cases = [T.by_name(n) for n in T.GROUP[:3]]
    ts = [T.operands(c, DEV) for c in cases]
    need = int(lib.acx_gemm_tn_group_workspace_bytes(3, C.cast(_group_table(cases, ts), C.c_void_p)))
    ws, wsp = _workspace(need)
    arr = _group_table(cases, ts)
    arr[1].B = None
    assert lib.acx_gemm_tn_group(own_ctx, 3, C.cast(arr, C.c_void_p), wsp, need, _stream()) == T.E_BADARG
    assert b"acx_gemm_tn_group: null pointer" in lib.acx_last_error(own_ctx)
    arr = _group_table(cases, ts)
    assert lib.acx_gemm_tn_group(own_ctx, 3, C.cast(arr, C.c_void_p), wsp, need - 256, _stream()) == T.E_WORKSPACE
    assert b"acx_gemm_tn_group: workspace too small" in lib.acx_last_error(own_ctx)
    torch.cuda.synchronize()
    assert all(T.guards_intact(t["c_buf"], 0, 0) for t in ts) and _intact_from(ws, 0)


def test_worst_ratio_per_kernel():
    for kern, (ratio, name) in sorted(WORST.items()):
        print(f"tn-route-worst {T.KERNEL_NAMES[kern]} {ratio:.4f} {name}")
    print(f"tn-route-seconds {time.time() - T0[0]:.1f}")
    assert all(ratio <= 1.0 for ratio, _ in WORST.values())
