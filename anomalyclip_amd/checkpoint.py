"""Checkpoint interop: load the `state_dict` of a reference Lightning `.ckpt`
(`configs/callbacks/default.yaml:8-14`; keys `net.<module path>`) and the `ncentroid.pt` side-car
(`anomaly_clip_module.py:140-171`) into the mirrors, and write checkpoints the reference can read back.

Training state (what `trainer.fit(..., ckpt_path=)` resumes from, src/train.py:94) travels in Lightning 1.8's keys:
`optimizer_states` = [torch-format optimizer state_dict], `lr_schedulers` = [scheduler state_dict without live objects],
`epoch`, `global_step`; plus the private key `acx_resume` with what Lightning does not save and a bit-identical continuation
needs: per rank the states of torch's CPU generator, the device's generator and numpy's global generator, the train loaders'
own counters and the world size the file was written at."""
from __future__ import annotations

import os
import warnings
from typing import Any, Dict, List, Mapping, Optional, Tuple

import numpy as np
import torch


def split_lightning_state_dict(sd: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """`net.`-prefixed keys of an AnomalyCLIPModule checkpoint -> AnomalyCLIP.state_dict() keys.  CLIP weights
    stored in fp16 (the reference converts with `.float()`, anomaly_clip.py:67) are up-cast."""
    out = {}
    for k, v in sd.items():
        if k.startswith("net."):
            k = k[4:]
        elif "." in k and k.split(".")[0] in ("train_loss", "roc", "auroc", "pr_curve", "average_precision", "f1", "confmat"):
            continue                                  # torchmetrics state of the LightningModule
        out[k] = v.float() if torch.is_tensor(v) and v.is_floating_point() else v
    return out


_CLIP_TEXT_KEYS = ("transformer.", "positional_embedding", "ln_final.", "text_projection")
_CLIP_DROPPED = ("logit_scale", "input_resolution", "context_length", "vocab_size", "attn_mask")


def is_clip_state_dict(sd) -> bool:
    """a plain CLIP state_dict (OpenAI's non-JIT model.state_dict(), open_clip's open_clip_pytorch_model.bin): it has `visual.` keys"""
    return isinstance(sd, Mapping) and any(isinstance(k, str) and k.startswith("visual.") for k in sd)


def from_clip_state_dict(sd: Mapping[str, torch.Tensor]) -> Dict[str, torch.Tensor]:
    """A plain CLIP state_dict -> AnomalyCLIP.state_dict() keys: `visual.*` -> `image_encoder.*`; `transformer.*`,
    `positional_embedding`, `ln_final.*`, `text_projection` -> `text_encoder.*`; `token_embedding.weight` stays; `logit_scale` and
    the JIT archives' `input_resolution` / `context_length` / `vocab_size` (and open_clip's `attn_mask` buffer) are dropped.  Half
    tensors are widened to float32.  Any other key is a ValueError: this is not the CLIP module tree the mirrors have.
    The dict does not say which activation the weights were trained with (OpenAI: "quick_gelu"; open_clip configs without
    `quick_gelu: true`: "gelu"): that is the caller's `act`."""
    out = {}
    for k, v in sd.items():
        if k in _CLIP_DROPPED:
            continue
        if k.startswith("visual."):
            nk = "image_encoder." + k[len("visual."):]
        elif k.startswith(_CLIP_TEXT_KEYS):
            nk = "text_encoder." + k
        elif k == "token_embedding.weight":
            nk = k
        else:
            raise ValueError(f"not a CLIP state_dict key: {k!r} (expected visual.*, transformer.*, positional_embedding, ln_final.*, "
                             "text_projection, token_embedding.weight, logit_scale)")
        out[nk] = v.float() if torch.is_tensor(v) and v.is_floating_point() else v
    return out


def load_into(net: torch.nn.Module, ckpt, strict: bool = True) -> Tuple[list, list]:
    """ckpt: path to a Lightning .ckpt, the loaded dict, a bare state_dict, or a plain CLIP state_dict (`visual.*` keys: it fills the
    two CLIP towers and the token embedding, AnomalyCLIP.load_state_dict; `strict` then covers those alone)."""
    if isinstance(ckpt, str):
        ckpt = torch.load(ckpt, map_location="cpu", weights_only=False)
    sd = ckpt.get("state_dict", ckpt) if isinstance(ckpt, dict) else ckpt
    if is_clip_state_dict(sd):
        missing, unexpected = net.load_state_dict(sd, strict=strict)
        return list(missing), list(unexpected)
    sd = split_lightning_state_dict(sd)
    missing, unexpected = net.load_state_dict(sd, strict=False)
    # buffers the reference recomputes from the class names are allowed to differ in presence only
    if strict and (missing or unexpected):
        raise RuntimeError(f"checkpoint does not match the module tree: missing={missing} unexpected={unexpected}")
    return list(missing), list(unexpected)


def to_lightning_state_dict(net: torch.nn.Module) -> Dict[str, torch.Tensor]:
    return {"net." + k: v.detach().cpu() for k, v in net.state_dict().items()}


# ====================================================================================================== training state
# the keys torch.optim.AdamW's own param groups carry besides ours: written so that the file is what the reference's optimizer wrote
_TORCH_ADAMW_GROUP_DEFAULTS = dict(amsgrad=False, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None)


def read(ckpt) -> Any:
    """path -> the loaded file (on the host); anything else is returned as it is"""
    if isinstance(ckpt, (str, os.PathLike)):
        return torch.load(os.fspath(ckpt), map_location="cpu", weights_only=False)
    return ckpt


def has_training_state(ckpt) -> bool:
    return isinstance(ckpt, Mapping) and bool(ckpt.get("optimizer_states"))


def optimizer_state_dict(optimizer) -> dict:
    """`optimizer.state_dict()` the way torch.optim.AdamW writes it: state keyed by the running parameter index, moments on the
    host, `step` a 0-d float32 tensor (AcxAdamW counts in a Python int)."""
    sd = optimizer.state_dict()
    state = {}
    for idx, st in sd["state"].items():
        if not st:                                    # a parameter that never had a gradient (logit_scale): no entry, as under torch
            continue
        out = {}
        for k, v in st.items():
            if k == "step":
                out[k] = torch.tensor(float(v), dtype=torch.float32)
            else:
                out[k] = v.detach().cpu() if torch.is_tensor(v) else v
        state[idx] = out
    groups = []
    for g in sd["param_groups"]:
        g = dict(g)
        for k, v in _TORCH_ADAMW_GROUP_DEFAULTS.items():
            g.setdefault(k, v)
        groups.append(g)
    return {"state": state, "param_groups": groups}


def _is_plain(v) -> bool:
    if v is None or isinstance(v, (bool, int, float, str, torch.Tensor)):
        return True
    if isinstance(v, (list, tuple)):
        return all(_is_plain(x) for x in v)
    if isinstance(v, dict):
        return all(_is_plain(k) and _is_plain(x) for k, x in v.items())
    return False


def scheduler_state_dict(scheduler) -> dict:
    """`scheduler.state_dict()` without live objects: WarmupCosineAnnealingLR's `successor` is a CosineAnnealingLR that
    references the whole optimizer (accepted and ignored, as in the reference) -- it and anything else that is not plain data
    stays out of the file."""
    return {k: v for k, v in scheduler.state_dict().items() if k != "successor" and _is_plain(v)}


def rng_state(device: Optional[torch.device] = None) -> dict:
    """the state of every generator a training step draws from on this rank: torch's CPU generator (selector masks, the
    DataLoaders' shuffle seeds), the device's generator, numpy's global generator (segment starts)"""
    kind, keys, pos, has_gauss, cached = np.random.get_state()
    out = {"torch_cpu": torch.get_rng_state(), "cuda": None,
           "numpy": (str(kind), torch.from_numpy(np.asarray(keys).astype(np.int64)), int(pos), int(has_gauss), float(cached))}
    if device is not None and torch.device(device).type == "cuda" and torch.cuda.is_available():
        out["cuda"] = torch.cuda.get_rng_state(device)
    return out


def set_rng_state(state: Mapping, device: Optional[torch.device] = None) -> None:
    torch.set_rng_state(state["torch_cpu"])
    kind, keys, pos, has_gauss, cached = state["numpy"]
    np.random.set_state((kind, keys.numpy().astype(np.uint32), int(pos), int(has_gauss), float(cached)))
    if state.get("cuda") is not None and device is not None and torch.device(device).type == "cuda" and torch.cuda.is_available():
        torch.cuda.set_rng_state(state["cuda"], device)


def loader_state(loaders) -> List[dict]:
    """the train loaders' own counters (ResidentTrainLoader._epoch / _shard_seed; None for a loader without them)"""
    if loaders is None:
        return []
    if not isinstance(loaders, (list, tuple)):
        loaders = [loaders]
    return [{"epoch": getattr(l, "_epoch", None), "shard_seed": getattr(l, "_shard_seed", None)} for l in loaders]


def set_loader_state(loaders, states: List[Mapping]) -> None:
    if not isinstance(loaders, (list, tuple)):
        loaders = [loaders]
    for l, st in zip(loaders, states or []):
        if st.get("epoch") is not None and hasattr(l, "_epoch"):
            l._epoch = int(st["epoch"])
        if st.get("shard_seed") is not None and hasattr(l, "_shard_seed"):
            l._shard_seed = int(st["shard_seed"])


def training_state(optimizer, scheduler, rng_states: List[dict], loaders, world_size: int) -> dict:
    """the keys a resumable checkpoint adds to the weights ({} for an optimizer without a state_dict)"""
    if not hasattr(optimizer, "state_dict"):
        return {}
    return {"optimizer_states": [optimizer_state_dict(optimizer)],
            "lr_schedulers": [scheduler_state_dict(scheduler)] if scheduler is not None else [],
            "acx_resume": {"version": 1, "world_size": int(world_size), "rng": list(rng_states),
                           "train_loaders": loader_state(loaders)}}


def save_atomic(obj, path: str) -> None:
    """write `<path>.tmp`, then rename it over `path`: a run killed during the save leaves the previous file whole.  The temporary
    name is fixed, so what a killed save left behind is overwritten by the next one (one writer per path: rank 0).  No fsync: it
    guards against a lost machine, not a killed process, and cost a quarter of the save's time where it was measured (DESIGN.md
    section 4, "Checkpoints and resume")."""
    tmp = path + ".tmp"
    try:
        torch.save(obj, tmp)                          # by name: torch's own file writer (an open Python file costs a fifth more)
        os.replace(tmp, path)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def _group_name(i: int, g: Mapping) -> str:
    return f"param group {i} ({g['name']!r})" if "name" in g else f"param group {i}"


def load_optimizer_state(optimizer, saved: Mapping) -> None:
    """A torch-format optimizer state_dict INTO the optimizer's existing state: moments are copied into the tensors that are
    there (a captured whole-step graph has their addresses baked in, and TrainStepGraph.make_key does not cover them), absent
    ones are created the way AcxAdamW.step / TrainStepGraph._opt_state create them, `step` becomes an int.  Nothing is touched
    before every group size and tensor shape has been checked."""
    groups, sgroups = optimizer.param_groups, saved["param_groups"]
    if len(groups) != len(sgroups):
        raise ValueError(f"optimizer state: the checkpoint holds {len(sgroups)} param groups, configure_optimizers() built "
                         f"{len(groups)}")
    plan = []
    for i, (g, sg) in enumerate(zip(groups, sgroups)):
        if len(g["params"]) != len(sg["params"]):
            raise ValueError(f"optimizer state: {_group_name(i, g)} holds {len(g['params'])} tensors of shapes "
                             f"{[tuple(p.shape) for p in g['params']]}, the checkpoint's group holds {len(sg['params'])}"
                             f"{_saved_shapes(saved, sg)}")
        for j, (p, idx) in enumerate(zip(g["params"], sg["params"])):
            st = saved["state"].get(idx) or None          # an empty entry is no entry
            if st is not None:
                for k in ("exp_avg", "exp_avg_sq"):
                    if k not in st or tuple(st[k].shape) != tuple(p.shape):
                        raise ValueError(f"optimizer state: {_group_name(i, g)}, tensor {j}: the parameter has shape "
                                         f"{tuple(p.shape)}, the checkpoint's {k} has shape "
                                         f"{tuple(st[k].shape) if k in st else None}")
            plan.append((p, st))
    with torch.no_grad():
        for p, st in plan:
            cur = optimizer.state.get(p)                  # (.get: `state` is a defaultdict, a lookup would leave an empty entry)
            if st is None:
                if cur:                                   # stepped here, never in the checkpoint's run: as good as new
                    cur["step"] = 0
                    cur["exp_avg"].zero_()
                    cur["exp_avg_sq"].zero_()
                continue
            if not cur:
                cur = optimizer.state[p]
                cur["step"] = 0
                cur["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                cur["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
            step = st.get("step", 0)
            cur["step"] = int(step.item()) if torch.is_tensor(step) else int(step)
            cur["exp_avg"].copy_(st["exp_avg"])
            cur["exp_avg_sq"].copy_(st["exp_avg_sq"])
    changed = []
    for i, (g, sg) in enumerate(zip(groups, sgroups)):    # what torch's load_state_dict takes from the file: the hyper-parameters
        for k in g:
            if k != "params" and k in sg:
                if k not in ("lr", "initial_lr") and _plain_differs(g[k], sg[k]):     # (the schedule moves lr: it always differs)
                    changed.append(f"{_group_name(i, g)}: {k} = {sg[k]!r} (configured: {g[k]!r})")
                g[k] = sg[k]
    if changed:
        warnings.warn("resume: the checkpoint's optimizer hyper-parameters replace the configured ones, as in "
                      "torch.optim.Optimizer.load_state_dict -- " + "; ".join(changed))


def _plain_differs(a, b) -> bool:
    if isinstance(a, (list, tuple)) and isinstance(b, (list, tuple)):
        return len(a) != len(b) or any(_plain_differs(x, y) for x, y in zip(a, b))
    return a != b


def _saved_shapes(saved: Mapping, sg: Mapping) -> str:
    shapes = [tuple(saved["state"][i]["exp_avg"].shape) for i in sg["params"] if i in saved["state"] and "exp_avg" in saved["state"][i]]
    return f" (shapes of those with state: {shapes})" if shapes else ""


def load_scheduler_state(scheduler, saved: Mapping) -> None:
    """`successor` stays as constructed (a Lightning-written file pickles the reference's; it is ignored either way)"""
    scheduler.load_state_dict({k: v for k, v in saved.items() if k != "successor"})


def load_training_state(ckpt, optimizer, scheduler=None) -> Optional[dict]:
    """Optimizer moments and step counts, scheduler and counters of a checkpoint written by Trainer.save_checkpoint or by
    Lightning, into the objects configure_optimizers() returned.  -> {"epoch", "global_step", "acx_resume" (or None)};
    None, after one warning, for a file without `optimizer_states` (weights only: training starts at epoch 0)."""
    ckpt = read(ckpt)
    if not has_training_state(ckpt):
        warnings.warn("the checkpoint holds no optimizer state (weights only): the weights are loaded, training starts at "
                      "epoch 0 with a fresh optimizer and schedule")
        return None
    load_optimizer_state(optimizer, ckpt["optimizer_states"][0])
    sch = ckpt.get("lr_schedulers") or []
    if scheduler is not None and sch:
        load_scheduler_state(scheduler, sch[0])
    return {"epoch": int(ckpt.get("epoch", -1)), "global_step": int(ckpt.get("global_step", 0)),
            "acx_resume": ckpt.get("acx_resume")}
