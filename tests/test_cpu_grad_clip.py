"""CPU-only checks of gradient clipping (Trainer(gradient_clip_val=..., gradient_clip_algorithm=...)): the Trainer's arguments,
the host-side argument checks of the new C entry points, the wrappers' no-fallback rule, and the numpy restatement the GPU
tests compare against (tests/grad_clip_ref.py) against torch's own clip_grad_norm_ / clip_grad_value_."""
import ctypes as C

import numpy as np
import pytest
import torch

import grad_clip_ref as ref
from anomalyclip_amd import _lib as L
from anomalyclip_amd import ops
from anomalyclip_amd.optim import normalize_clip
from anomalyclip_amd.trainer import Trainer

BADARG, WORKSPACE = -1, -4


def test_trainer_takes_lightnings_clip_arguments():
    t = Trainer()
    assert t.gradient_clip_val is None and t.gradient_clip_algorithm == "norm"
    assert normalize_clip(t.gradient_clip_val, t.gradient_clip_algorithm) == (None, 0.0)
    assert normalize_clip(0, None) == (None, 0.0) and normalize_clip(0.0, "value") == (None, 0.0)
    t = Trainer(gradient_clip_val=1.0)
    assert (t.gradient_clip_val, t.gradient_clip_algorithm) == (1.0, "norm")
    assert normalize_clip(t.gradient_clip_val, t.gradient_clip_algorithm) == ("norm", 1.0)
    t = Trainer(gradient_clip_val=0.5, gradient_clip_algorithm="value", accelerator="gpu", logger=False)
    assert normalize_clip(t.gradient_clip_val, t.gradient_clip_algorithm) == ("value", 0.5)
    with pytest.raises(ValueError, match="gradient_clip_val"):
        Trainer(gradient_clip_val=-1.0)
    with pytest.raises(ValueError, match="gradient_clip_val"):
        Trainer(gradient_clip_val="1.0")
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        Trainer(gradient_clip_val=1.0, gradient_clip_algorithm="l2")
    with pytest.raises(ValueError, match="gradient_clip_algorithm"):
        Trainer(gradient_clip_algorithm="clamp")                       # refused even while clipping is off


def test_train_batch_reads_the_trainer_and_takes_keywords():
    import inspect
    from anomalyclip_amd.anomaly_clip_module import AnomalyCLIPModule
    sig = inspect.signature(AnomalyCLIPModule.train_batch)
    assert list(sig.parameters)[:4] == ["self", "batch", "optimizer", "batch_idx"]
    assert sig.parameters["gradient_clip_val"].default is None and sig.parameters["gradient_clip_algorithm"].default is None


def test_abi_argument_checks_without_gpu():
    lib = L.lib()
    buf = (C.c_float * 64)()
    ws_buf = (C.c_double * 66)()
    ws_at = (C.addressof(ws_buf) + 15) & ~15                           # the workspace is 16-byte aligned
    ptrs = (C.c_void_p * 2)(C.addressof(buf), C.addressof(buf))
    n = (C.c_int64 * 2)(8, 8)
    out = C.addressof(buf)
    # workspace size: one line for the counter + one double per 16384-element chunk, every tensor may end in a partial chunk
    assert lib.acx_grad_norm_workspace_bytes(0, 10) == 0 and lib.acx_grad_norm_workspace_bytes(1, -1) == 0
    assert lib.acx_grad_norm_workspace_bytes(3, 0) == 64 + 8 * 3
    assert lib.acx_grad_norm_workspace_bytes(58, 16384 * 10 + 5) == 64 + 8 * (10 + 58)

    def norm(nseg=2, g=ptrs, nn=n, max_norm=1.0, o=out, w=ws_at, wb=512):
        return lib.acx_grad_norm(None, nseg, g, nn, 1.0, max_norm, o, w, wb, None)
    for bad in (dict(nseg=0), dict(nseg=-3), dict(g=None), dict(nn=None), dict(o=None), dict(w=None), dict(max_norm=-1.0),
                dict(max_norm=float("nan")), dict(nn=(C.c_int64 * 2)(8, -1)), dict(g=(C.c_void_p * 2)(C.addressof(buf), None)),
                dict(w=ws_at + 4)):
        assert norm(**bad) == BADARG, bad
        assert b"acx_grad_norm" in lib.acx_last_error(None)
    assert norm(wb=64 + 8) == WORKSPACE and b"workspace" in lib.acx_last_error(None)

    def adamw(clip=None, value=0.0, g=ptrs):
        return lib.acx_adamw_multi_dev_clip(None, 2, ptrs, g, ptrs, ptrs, n, out, 1.0, 0.9, 0.999, 1e-8, clip, value, None)
    assert adamw(clip=out, value=1.0) == BADARG and b"exclusive" in lib.acx_last_error(None)
    assert adamw(value=float("nan")) == BADARG
    assert adamw(clip=out, g=None) == BADARG and adamw(value=1.0, g=(C.c_void_p * 2)(None, C.addressof(buf))) == BADARG
    assert lib.acx_adamw_multi_dev_clip(None, 2, ptrs, None, ptrs, ptrs, n, out, 1.0, 0.9, 0.999, 1e-8, None, 0.0, None) == BADARG
    assert lib.acx_adamw_multi_dev_clip(None, 0, None, None, None, None, None, None, 1.0, 0.9, 0.999, 1e-8, out, 0.0, None) == 0

    def scale(nseg=2, g=ptrs, nn=n, clip=None, value=1.0):
        return lib.acx_clip_grads(None, nseg, g, nn, 1.0, clip, value, None)
    for bad in (dict(nseg=0), dict(g=None), dict(nn=None), dict(nn=(C.c_int64 * 2)(-8, 8)), dict(clip=out),
                dict(value=float("nan")), dict(g=(C.c_void_p * 2)(None, None))):
        assert scale(**bad) == BADARG, bad
        assert b"acx_clip_grads" in lib.acx_last_error(None)
    assert scale(value=0.0) == 0                                       # nothing to do: no launch


def test_wrappers_refuse_cpu_tensors():
    g = [torch.randn(8), torch.randn(3)]
    rec = torch.zeros(4)
    with pytest.raises(L.AcxError):
        ops.grad_norm_workspace(g)
    with pytest.raises(L.AcxError):
        ops.grad_norm_(g, 1.0, 1.0, rec, torch.zeros(16, dtype=torch.float64))
    with pytest.raises(L.AcxError):
        ops.clip_grads_(g, 1.0, None, 0.5)
    with pytest.raises(L.AcxError):
        ops.adamw_multi_dev_clip_(g, g, g, g, torch.zeros(5), 1.0, 0.9, 0.999, 1e-8, None, 0.5)


def _grads(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * scale for n in (1, 3, 1025, 70000)]


@pytest.mark.parametrize("max_norm", [1e-3, 1.0, 1e4])
def test_restatement_agrees_with_clip_grad_norm(max_norm):
    gs = _grads(3)
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    want, norm = ref.clip([g.numpy() for g in gs], "norm", max_norm)
    # torch adds the per-tensor norms in f32: a few ulp from the fp64 norm
    assert abs(float(total) - float(norm)) <= 4 * np.spacing(np.float32(norm))
    # the coefficient, given the SAME f32 norm, bit for bit
    c_torch = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    assert ref.clip_coef(np.float32(total.item()), max_norm).tobytes() == c_torch.numpy().tobytes()
    for p, w in zip(ps, want):
        assert np.allclose(p.grad.numpy(), w, rtol=1e-6, atol=0)


def test_restatement_coefficient_edge_cases():
    one = np.float32(1.0)
    assert ref.clip_coef(0.0, 1.0) == one and ref.clip_coef(0.5, 1.0) == one          # zero / small gradient: exactly 1
    assert ref.clip_coef(1.5, 1.0) < one
    for norm in (float("nan"), float("inf"), 0.0, 3.0):
        t = torch.clamp(1.0 / (torch.tensor(norm, dtype=torch.float32) + 1e-6), max=1.0)
        assert ref.clip_coef(norm, 1.0).tobytes() == t.numpy().tobytes(), norm           # nan stays nan, inf gives 0
    big = [np.full(5, 1e25, dtype=np.float32)]
    assert np.isfinite(ref.grad_norm(big)) and abs(ref.grad_norm(big) / (1e25 * 5 ** 0.5) - 1) < 1e-6
    assert ref.grad_norm(big, 0.5) == ref.grad_norm([big[0] * np.float32(0.5)])


def test_restatement_agrees_with_clip_grad_value():
    gs = _grads(4)
    gs[1][1] = float("nan")
    ps = [torch.nn.Parameter(torch.zeros_like(g)) for g in gs]
    for p, g in zip(ps, gs):
        p.grad = g.clone()
    torch.nn.utils.clip_grad_value_(ps, 0.25)
    want, _ = ref.clip([g.numpy() for g in gs], "value", 0.25)
    for p, w in zip(ps, want):
        assert np.array_equal(p.grad.numpy(), w, equal_nan=True)
    assert np.isnan(want[1][1])


def test_restatement_adamw_matches_torch():
    g = torch.Generator().manual_seed(6)
    p0 = torch.randn(500, generator=g).double()
    pt = torch.nn.Parameter(p0.clone())
    opt = torch.optim.AdamW([pt], lr=1e-3, weight_decay=0.2)
    p, m, v = p0.numpy(), np.zeros(500), np.zeros(500)
    for step in range(1, 4):
        gr = torch.randn(500, generator=g).double()
        pt.grad = gr.clone()
        opt.step()
        p, m, v = ref.adamw_step(p, gr.numpy(), m, v, 1e-3, 0.2, 0.9, 0.999, 1e-8, step)
    assert np.allclose(pt.detach().numpy(), p, rtol=1e-12, atol=1e-15)
