"""AcxAdamW: torch.optim.AdamW semantics (decoupled weight decay, bias correction, no amsgrad) with the
update executed by the fused libacx kernel acx_adamw -- one HBM pass over (p, g, m, v) per parameter
(16 B read + 12 B written per value).  Param groups / lr scheduling behave like any torch optimizer, so the
reference's configure_optimizers grouping (anomaly_clip_module.py:693-746) carries over unchanged."""
from __future__ import annotations

import torch

from . import ops
from .parallel import _is_dense as parallel_is_dense, same_layout


def normalize_clip(gradient_clip_val, gradient_clip_algorithm=None):
    """Lightning's Trainer(gradient_clip_val, gradient_clip_algorithm) -> (algorithm, value): (None, 0.0) when clipping is off
    (value None or 0); the algorithm defaults to "norm".  A ValueError names the offending key."""
    algo = "norm" if gradient_clip_algorithm is None else str(getattr(gradient_clip_algorithm, "value", gradient_clip_algorithm)).lower()
    if algo not in ("norm", "value"):
        raise ValueError(f"gradient_clip_algorithm must be 'norm' or 'value', got {gradient_clip_algorithm!r}")
    if gradient_clip_val is None:
        return None, 0.0
    if isinstance(gradient_clip_val, bool) or not isinstance(gradient_clip_val, (int, float)) or not gradient_clip_val >= 0:
        raise ValueError(f"gradient_clip_val must be a number >= 0 or None, got {gradient_clip_val!r}")
    val = float(gradient_clip_val)
    return (algo, val) if val > 0 else (None, 0.0)


class AcxAdamW(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        defaults = dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)

    def _hyper_dev(self, device, lrs, wds, b1, b2, step) -> torch.Tensor:
        """the step's per-tensor scalars (ops.adamw_hyper) in device memory: a pinned staging buffer and a device buffer per
        (device, tensor count), kept across steps, the copy asynchronous -- no synchronising upload per step"""
        bufs = self.__dict__.setdefault("_hyper_bufs", {})
        key = (device, len(lrs))
        if key not in bufs:
            n = 1 + 2 * len(lrs)
            bufs[key] = [torch.empty(n, dtype=torch.float32).pin_memory(), torch.empty(n, dtype=torch.float32, device=device), None]
        host, dev, ev = bufs[key]
        if ev is not None:
            ev.synchronize()                       # the previous step's copy has read the staging buffer (long done by now)
        ops.adamw_hyper(lrs, wds, b1, b2, step, host)
        dev.copy_(host, non_blocking=True)
        bufs[key][2] = torch.cuda.Event()
        bufs[key][2].record()
        return dev

    @torch.no_grad()
    def step(self, closure=None, clip=None):
        """clip: None, or (clip_dev, clip_value) -- the device record ops.grad_norm_ wrote (scale every gradient by its
        coefficient) or a clamp value (0: off): the update then runs through acx_adamw_multi_dev_clip, the kernel of the
        whole-step graph, and .grad is left holding the clipped gradient."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        # every tensor that shares (betas, eps, step) -- in practice all of them -- goes into ONE acx_adamw_multi launch
        # (per-tensor lr / weight decay carry the reference's four param groups); 34 launches -> 1 at the UCF config
        batches: dict = {}
        for group in self.param_groups:
            b1, b2 = group["betas"]
            for p in group["params"]:
                if p.grad is None:
                    continue
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    # moments in the PARAMETER's memory layout: the kernel walks the raw memory of (p, g, m, v) elementwise
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                if not (p.is_contiguous() or parallel_is_dense(p)) or not same_layout(st["exp_avg"], p):
                    raise ops.L.AcxError("AcxAdamW updates parameters in place through raw pointers: dense parameters only "
                                         "(row-major, or a permuted-contiguous layout such as channels-last)")
                g = p.grad
                if not same_layout(g, p):             # same physical element order as the parameter
                    g = torch.empty_like(p, memory_format=torch.preserve_format).copy_(g)
                key = (p.device, float(b1), float(b2), float(group["eps"]), int(st["step"]))
                b = batches.setdefault(key, ([], [], [], [], [], []))
                for lst, val in zip(b, (p, g, st["exp_avg"], st["exp_avg_sq"], float(group["lr"]), float(group["weight_decay"]))):
                    lst.append(val)
        for (_, b1, b2, eps, step), (ps, gs, ms, vs, lrs, wds) in batches.items():
            if clip is None:
                ops.adamw_multi_(ps, gs, ms, vs, lrs, wds, b1, b2, eps, step)
                continue
            # a gradient that had to be copied into the parameter's layout (above) is clipped in the copy: hand the result back
            ops.adamw_multi_dev_clip_(ps, gs, ms, vs, self._hyper_dev(ps[0].device, lrs, wds, b1, b2, step), 1.0, b1, b2, eps,
                                      clip[0], clip[1])
            for p, g in zip(ps, gs):
                if g is not p.grad:
                    p.grad.copy_(g)
        ops.WEIGHT_EPOCH[0] += 1
        return loss
