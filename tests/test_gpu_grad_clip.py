"""-m gpu: gradient clipping -- the global-norm kernel (acx_grad_norm), the clipped AdamW (acx_adamw_multi_dev_clip), the in-place
scaling (acx_clip_grads), and Trainer(gradient_clip_val=..., gradient_clip_algorithm=...) end to end through the whole-step graph
and the autograd path.  References: tests/grad_clip_ref.py (numpy fp64) and torch's own clip_grad_norm_ / clip_grad_value_ +
torch.optim.AdamW on CPU tensors."""
import os
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import grad_clip_ref as ref
from anomalyclip_amd import init_weights as IW
from anomalyclip_amd import ops
from anomalyclip_amd.optim import AcxAdamW
from anomalyclip_amd.trainer import Trainer
from test_gpu_train import _dp_batch, _dp_module, relerr

DEV = "cuda"
# the grid of test_adamw_multi_tensor_groups_match_torch: ragged sizes, 58 tensors (more than one launch's table of 48)
SIZES = [1, 3, 1023, 1024, 1025, 4096, 70000, 3 * 1024 * 1024 + 5] + [17 + 31 * i for i in range(50)]


def views_of(flat, sizes):
    """views at an ODD element offset of one flat buffer: 4-byte alignment only (parallel.GradBuckets hands out such views)"""
    out, off = [], 1
    for n in sizes:
        out.append(flat[off:off + n])
        off += n
    return out


def on_device(host, sizes):
    flat = torch.zeros(sum(sizes) + 1, device=DEV)
    flat[1:] = host.to(DEV)
    return flat, views_of(flat, sizes)


def norm_record(views, max_norm, scale=1.0, rec=None, ws=None):
    rec = torch.zeros(4, device=DEV) if rec is None else rec
    ws = ops.grad_norm_workspace(views) if ws is None else ws
    ops.grad_norm_(views, scale, max_norm, rec, ws)
    return rec, ws


def bits(t):
    return t.detach().cpu().numpy().tobytes()


def within_one_ulp(got: float, want: float) -> bool:
    return abs(np.float64(got) - np.float64(want)) <= np.float64(np.spacing(np.float32(want)))


def same_value(a, b) -> bool:
    """bit-equal, or both NaN (a NaN's sign and payload are not part of the contract)"""
    return bits(a) == bits(b) or (bool(torch.isnan(a)) and bool(torch.isnan(b)))


@pytest.fixture(scope="module")
def grid_data():
    host = torch.randn(sum(SIZES), generator=torch.Generator().manual_seed(11))
    want = ref.grad_norm([v.numpy() for v in views_of(torch.cat([torch.zeros(1), host]), SIZES)])
    return host, want


# ====================================================================================================== the norm kernel
def test_grad_norm_is_the_fp64_norm_and_replays(grid_data):
    host, want = grid_data
    flat, views = on_device(host, SIZES)
    rec, ws = norm_record(views, 100.0)
    norm = float(rec[0])
    print("norm", norm, "fp64", want, "ulp", float(np.spacing(np.float32(want))))
    assert within_one_ulp(norm, want)
    assert bits(rec[1]) == ref.clip_coef(np.float32(norm), 100.0).tobytes() and float(rec[1]) < 1
    first = rec.clone()
    norm_record(views, 100.0, rec=rec, ws=ws)                        # same scratch: the counter went back to zero
    assert bits(rec[:2]) == bits(first[:2])
    assert float(rec[2]) == 2 * norm                                 # out[2] accumulates across calls
    # replayed from a captured graph into another record
    rec2 = torch.zeros(4, device=DEV)
    graph, side = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=side):
        ops.grad_norm_(views, 1.0, 100.0, rec2, ws)
    for k in range(2):
        graph.replay()
        torch.cuda.synchronize()
        assert bits(rec2[:2]) == bits(first[:2]) and float(rec2[2]) == (k + 1) * norm
    # grad_scale: doubled data read with 0.5 is the same data (x * 0.5 is exact)
    flat.mul_(2.0)
    rec3, _ = norm_record(views, 100.0, scale=0.5, ws=ws)
    assert bits(rec3[:2]) == bits(first[:2])


def test_grad_norm_squares_beyond_f32_range():
    """values of 1e25: their squares overflow f32, not fp64 -- an f32 accumulator returns inf here"""
    sizes = [1025, 70000, 3, 16384, 16385]                           # (one chunk of the kernel exactly, and one element more)
    host = torch.randn(sum(sizes), generator=torch.Generator().manual_seed(12)) * 1e25
    want = ref.grad_norm([host.numpy()])
    _, views = on_device(host, sizes)
    rec, _ = norm_record(views, 1.0)
    assert np.isfinite(float(rec[0])) and within_one_ulp(float(rec[0]), want)
    assert 0 < float(rec[1]) < 1e-20


def test_grad_norm_coefficient_at_the_threshold():
    sizes = [4096, 70000]
    host = torch.randn(sum(sizes), generator=torch.Generator().manual_seed(13))
    _, views = on_device(host, sizes)
    zero, _ = norm_record([torch.zeros(5000, device=DEV), torch.zeros(3, device=DEV)], 1.0)
    assert float(zero[0]) == 0.0 and float(zero[1]) == 1.0           # a zero gradient: coefficient exactly 1
    norm = float(norm_record(views, 1.0)[0][0])
    below, _ = norm_record(views, norm * (1 + 2.0 ** -20))           # the norm just below max_norm
    above, _ = norm_record(views, norm * (1 - 2.0 ** -20))           # ... and just above
    assert float(below[1]) == 1.0 and float(above[1]) < 1.0
    assert bits(above[1]) == ref.clip_coef(np.float32(norm), norm * (1 - 2.0 ** -20)).tobytes()


@pytest.mark.parametrize("bad", [float("inf"), float("nan")])
def test_grad_norm_inf_and_nan_as_torch(bad):
    sizes = [1025, 4096, 3]
    host = torch.randn(sum(sizes), generator=torch.Generator().manual_seed(14))
    host[2000] = bad
    ps = [torch.nn.Parameter(torch.zeros(n)) for n in sizes]
    for p, g in zip(ps, views_of(torch.cat([torch.zeros(1), host]), sizes)):
        p.grad = g.clone()
    total = torch.nn.utils.clip_grad_norm_(ps, 2.0)                  # CPU torch: the norm, and the gradients clipped in place
    coef = torch.clamp(2.0 / (total + 1e-6), max=1.0)
    _, views = on_device(host, sizes)
    rec, _ = norm_record(views, 2.0)
    ops.clip_grads_(views, 1.0, rec, 0.0)
    assert same_value(rec[0], total) and same_value(rec[1], coef), (rec, total, coef)
    for v, p in zip(views, ps):
        assert torch.equal(torch.isnan(v).cpu(), torch.isnan(p.grad)) and torch.equal(torch.isinf(v).cpu(), torch.isinf(p.grad))


# ====================================================================================================== the clipped AdamW
def _hyper(lrs, step):
    h = torch.empty(1 + 2 * len(lrs), dtype=torch.float32)
    ops.adamw_hyper(lrs, [0.2] * len(lrs), 0.9, 0.999, step, h)
    return h.to(DEV)


def test_adamw_clip_with_both_off_is_adamw_multi_dev(grid_data):
    host, _ = grid_data
    gen = torch.Generator().manual_seed(15)
    p0 = torch.randn(sum(SIZES), generator=gen)
    lrs = [(1e-3, 5e-4, 2e-3, 1e-4)[i % 4] for i in range(len(SIZES))]
    runs = []
    for clip in (False, True):
        gflat, gs = on_device(host, SIZES)
        _, ps = on_device(p0, SIZES)
        _, ms = on_device(torch.zeros_like(p0), SIZES)
        _, vs = on_device(torch.zeros_like(p0), SIZES)
        for step in (1, 2):
            if clip:
                ops.adamw_multi_dev_clip_(ps, gs, ms, vs, _hyper(lrs, step), 1.0, 0.9, 0.999, 1e-8, None, 0.0)
            else:
                ops.adamw_multi_dev_(ps, gs, ms, vs, _hyper(lrs, step), 1.0, 0.9, 0.999, 1e-8)
        runs.append((ps, ms, vs, gs))
    for a, b in zip(runs[0], runs[1]):
        assert all(torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("algo,value", [("norm", 100.0), ("value", 0.5)])
def test_adamw_clip_matches_torch_clip_then_adamw(algo, value):
    """AcxAdamW.step(clip=...) over the grid against clip_grad_norm_ / clip_grad_value_ + torch.optim.AdamW on CPU tensors: four
    steps, an lr change in between.  Bound on the parameters: test_adamw_matches_torch's 1e-6 -- the only new operation is one f32
    multiply per gradient by a coefficient that is itself within 2 ulp (norm within 1 ulp, one division), or an exact clamp.
    torch's own f32 norm of these 3.2 M values is 6e-5 off (measured: 1805.7344 against 1805.8484), which the update, being
    invariant to the gradient's scale up to eps, does not see; the clipped gradient left in the buffer and the moments, which do
    scale with the coefficient, are held to the same 1e-6 against the fp64 restatement."""
    g = torch.Generator().manual_seed(7)
    ps = [torch.randn(n, generator=g) for n in SIZES]
    pa = [torch.nn.Parameter(p.clone().to(DEV)) for p in ps]
    pb = [torch.nn.Parameter(p.clone()) for p in ps]
    lrs = [1e-3, 5e-4, 2e-3, 1e-4]

    def groups(params):
        return [{"params": params[i::4], "lr": lrs[i]} for i in range(4)]
    oa = AcxAdamW(groups(pa), weight_decay=0.2)
    ob = torch.optim.AdamW(groups(pb), weight_decay=0.2)
    flat = torch.zeros(sum(SIZES) + 1, device=DEV)
    views = views_of(flat, SIZES)
    rec, ws = torch.zeros(4, device=DEV), ops.grad_norm_workspace(views)
    m64, v64 = [np.zeros(n) for n in SIZES], [np.zeros(n) for n in SIZES]
    for step in range(4):
        raw = []
        for a, b, v in zip(pa, pb, views):
            gr = torch.randn(v.numel(), generator=g)
            v.copy_(gr)
            a.grad, b.grad = v, gr.clone()
            raw.append(gr.numpy())
        want, want_norm = ref.clip(raw, algo, value)
        if step == 2:
            for o in (oa, ob):
                for grp in o.param_groups:
                    grp["lr"] *= 0.5
        if algo == "norm":
            ops.grad_norm_(views, 1.0, value, rec, ws)
            oa.step(clip=(rec, 0.0))
            torch.nn.utils.clip_grad_norm_(pb, value)
            assert float(rec[1]) < 1 and within_one_ulp(float(rec[0]), float(want_norm))
        else:
            oa.step(clip=(None, value))
            torch.nn.utils.clip_grad_value_(pb, value)
        ob.step()
        for i, a in enumerate(pa):                                   # the gradient buffer holds the clipped gradient
            if algo == "value":
                assert torch.equal(a.grad.cpu(), pb[i].grad) and np.array_equal(a.grad.cpu().numpy(), want[i]), (step, i)
                assert float(a.grad.abs().max()) <= value
            else:
                assert relerr(a.grad, want[i]) < 1e-6, (step, i)
            _, m64[i], v64[i] = ref.adamw_step(0.0, want[i], m64[i], v64[i], 0.0, 0.0, 0.9, 0.999, 1e-8, step + 1)
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert relerr(a, b) < 1e-6, (i, SIZES[i])
        assert relerr(oa.state[a]["exp_avg_sq"], v64[i]) < 1e-6 and relerr(oa.state[a]["exp_avg"], m64[i]) < 1e-6, (i, SIZES[i])


# ====================================================================================================== end to end
D = IW.TINY.embed_dim
B = 4


def _batch(step):
    feats, labels, masks = _dp_batch(B, D, 640 + step)
    f, l = feats.to(DEV), labels.to(DEV)
    return ((f[B // 2:], l[B // 2:]), (f[:B // 2], l[:B // 2])), masks


def _module(prompts_table, step_graph=True, foreign=False):
    mod, net = _dp_module(prompts_table, geom="tiny")
    net.step_graph = step_graph
    if foreign:
        mod.optimizer = partial(torch.optim.AdamW, weight_decay=0.2)
    mod.ncentroid = torch.zeros(D, device=DEV)
    return mod, net, mod.configure_optimizers()["optimizer"]


def _step(mod, net, opt, step, **clip):
    batch, masks = _batch(step)
    net.selector_model.generate_mask = lambda b, m=masks: (m[0], m[1])
    mod.train_batch(batch, opt, step, **clip)
    torch.cuda.synchronize()


def _state(mod, net, opt):
    out = {"loss": torch.stack([torch.as_tensor(v).detach().reshape(()) for v in mod.last_losses]).clone()}
    for n, p in net.named_parameters():
        if p.requires_grad:
            out["p:" + n] = p.detach().clone()
            st = opt.state.get(p) or {}
            if "exp_avg" in st:
                out["m:" + n], out["v:" + n] = st["exp_avg"].clone(), st["exp_avg_sq"].clone()
    bn = net.selector_model.bn_layer
    out["bn:mean"], out["bn:var"] = bn.running_mean.clone(), bn.running_var.clone()
    return out


@pytest.fixture(scope="module")
def dry(prompts_table):
    """one UNCLIPPED step of the existing path from the common start: the start, its gradients, the parameters after it, and
    clip values at which clipping bites on every step of the tests below"""
    mod, net, opt = _module(prompts_table)
    start = {n: p.detach().cpu().clone() for n, p in net.named_parameters() if p.requires_grad}
    _step(mod, net, opt, 0)
    grads = {n: p.grad.detach().cpu().clone() for n, p in net.named_parameters() if p.requires_grad and p.grad is not None}
    after = {n: p.detach().cpu().clone() for n, p in net.named_parameters() if p.requires_grad}
    norm = ref.grad_norm([g.numpy() for g in grads.values()])
    gmax = max(float(g.abs().max()) for g in grads.values())
    groups = [{k: v for k, v in grp.items() if k != "params"} | {"names": [n for n, p in net.named_parameters()
                                                                            if any(p is q for q in grp["params"])]}
              for grp in opt.param_groups]
    print("dry step: grad norm", norm, "max |g|", gmax)
    return dict(start=start, grads=grads, after=after, groups=groups, clip={"norm": 0.05 * norm, "value": 0.05 * gmax},
                norm=norm, sg_items=[it[0] for it in next(iter(mod.__dict__["_step_graphs"].values())).program])


@pytest.mark.parametrize("foreign", [False, True], ids=["acx_adamw", "torch_adamw"])
@pytest.mark.parametrize("algo", ["norm", "value"])
def test_clipped_step_graph_bit_identical_to_autograd(prompts_table, dry, algo, foreign):
    """(a) three clipped steps through the whole-step graph and through the autograd path: identical bits in losses, parameters,
    moments, BatchNorm statistics, gradients and the norm record -- with clipping biting on every step"""
    value = dry["clip"][algo]
    runs = [_module(prompts_table, step_graph=sg, foreign=foreign) for sg in (True, False)]
    for step in range(3):
        states = []
        for mod, net, opt in runs:
            _step(mod, net, opt, step, gradient_clip_val=value, gradient_clip_algorithm=algo)
            st = _state(mod, net, opt)
            st["norm"], st["coef"] = mod.last_grad_norm.clone(), mod.last_clip_coef.clone()
            for n, p in net.named_parameters():
                if p.requires_grad and p.grad is not None:
                    st["g:" + n] = p.grad.detach().clone()
            states.append(st)
        a, b = states
        assert a.keys() == b.keys()
        for k in a:
            assert torch.equal(a[k], b[k]), (step, k)
        if algo == "norm":
            assert 0 < float(a["coef"]) < 1 and float(a["norm"]) > value, (step, float(a["coef"]))
        else:
            gm = max(float(v.abs().max()) for k, v in a.items() if k.startswith("g:"))
            assert gm == float(np.float32(value)), (step, gm)                              # the clamp bit
    sgs = runs[0][0].__dict__.get("_step_graphs", {})
    assert len(sgs) == 1 and all(v is not None for v in sgs.values()), getattr(runs[0][0], "step_graph_error", None)
    assert not runs[1][0].__dict__.get("_step_graphs")


@pytest.mark.parametrize("algo", ["norm", "value"])
def test_clipped_step_matches_torch_clip_then_adamw(prompts_table, dry, algo):
    """(b) one clipped step from the common start against: the unclipped step's gradients, clipped by torch on the CPU, then
    torch.optim.AdamW.  The parameters differ from the unclipped step's -- the assertion that fails without the feature."""
    value = dry["clip"][algo]
    mod, net, opt = _module(prompts_table)
    _step(mod, net, opt, 0, gradient_clip_val=value, gradient_clip_algorithm=algo)
    cpu = {n: torch.nn.Parameter(t.clone()) for n, t in dry["start"].items()}
    for n, g in dry["grads"].items():
        cpu[n].grad = g.clone()
    with_grad = [cpu[n] for n in dry["grads"]]
    if algo == "norm":
        total = torch.nn.utils.clip_grad_norm_(with_grad, value)
        print("e2e norm", float(mod.last_grad_norm), "fp64", dry["norm"], "torch f32", float(total))
        assert within_one_ulp(float(mod.last_grad_norm), dry["norm"]) and float(mod.last_clip_coef) < 1
    else:
        torch.nn.utils.clip_grad_value_(with_grad, value)
    torch.optim.AdamW([{"params": [cpu[n] for n in grp["names"] if n in cpu], "lr": grp["lr"], "betas": grp["betas"], "eps": grp["eps"],
                        "weight_decay": grp["weight_decay"]} for grp in dry["groups"]]).step()
    got = {n: p.detach().cpu() for n, p in net.named_parameters() if p.requires_grad}
    for n in cpu:
        assert relerr(got[n], cpu[n]) < 1e-6, n
    # .grad is left holding the clipped gradient (against the fp64 restatement: torch's f32 norm carries its own error)
    want, _ = ref.clip([g.numpy() for g in dry["grads"].values()], algo, value)
    for (n, g), w in zip(dry["grads"].items(), want):
        assert relerr(dict(net.named_parameters())[n].grad, w) < 1e-6, n
    assert any(not torch.equal(got[n], dry["after"][n]) for n in dry["grads"])


def test_defaults_change_nothing(prompts_table, dry):
    """(c) the arguments left at their defaults -- a Trainer without them attached, or explicit None / 0 -- give the bits of
    train_batch without any clip argument, and the captured sequence is today's, item for item"""
    plain, attached, zero = (_module(prompts_table) for _ in range(3))
    object.__setattr__(attached[0], "trainer", Trainer(max_epochs=1))
    for step in range(3):
        _step(*plain, step)
        _step(*attached, step)
        _step(*zero, step, gradient_clip_val=0.0, gradient_clip_algorithm="norm")
        a, b, c = _state(*plain), _state(*attached), _state(*zero)
        for k in a:
            assert torch.equal(a[k], b[k]) and torch.equal(a[k], c[k]), (step, k)
    # the sequence as step_graph._sequence records it for one GPU and the in-graph AdamW: text forward prologue (mark, wait, graph,
    # x mark); weight prep + temporal forward; wait for the text features; selector + loss + selector backward; mark; temporal
    # backward; text stream: wait, text backward + text AdamW, x mark, next step's text forward + its x mark; host bookkeeping;
    # main AdamW; wait for the text parameters
    today = ["record", "x_wait", "graph", "record_x", "graph", "main_wait_x", "graph", "record", "graph", "x_wait", "graph",
             "record_x", "graph", "record_x", "host", "graph", "main_wait_x"]
    for mod, _, _ in (plain, attached, zero):
        sg, = mod.__dict__["_step_graphs"].values()
        assert [it[0] for it in sg.program] == today == dry["sg_items"]
        assert float(mod.last_grad_norm) == 0.0 and float(mod.last_clip_coef) == 1.0


# ------------------------------------------------------------------------------------------------------ Trainer.fit
@pytest.fixture(scope="module")
def tiny_datamodule(tmp_path_factory):
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    from test_gpu_feature_bank import write_dataset
    from test_gpu_head_grid import FULL
    hc = FULL["24x10"]
    hp = write_dataset(tmp_path_factory.mktemp("clip_data"), (5, 241, 300, 700), (240, 1, 999, 64), (1, 13, 3, 5))
    return hc, lambda: AnomalyCLIPDataModule(**hp, num_segments=hc.num_segments, seg_length=hc.seg_length, batch_size=4)


def _fit(tiny_datamodule, save_dir, foreign, **trainer_kw):
    from test_gpu_head_grid import _grid_module
    hc, make_dm = tiny_datamodule
    mod, net = _grid_module(hc)
    mod.hparams["save_dir"] = str(save_dir)
    mod.optimizer = partial(torch.optim.AdamW if foreign else AcxAdamW, weight_decay=0.2)
    norms, step = [], mod.train_batch

    def recording(batch, opt, i=0):
        r = step(batch, opt, i)
        norms.append((mod.last_grad_norm.clone(), mod.last_clip_coef.clone()))
        return r
    mod.train_batch = recording
    trainer = Trainer(max_epochs=2, check_val_every_n_epoch=3, **trainer_kw)
    metrics = trainer.fit(mod, make_dm())
    torch.cuda.synchronize()
    return metrics, [(float(n), float(c)) for n, c in norms], mod


@pytest.mark.parametrize("foreign", [False, True], ids=["acx_adamw", "torch_adamw"])
def test_fit_reports_the_epoch_mean_grad_norm(tiny_datamodule, tmp_path, foreign):
    """(d), (e) Trainer(gradient_clip_val=...).fit, two epochs of two steps: train/grad_norm is the mean of the last epoch's per-step
    norms (summed in f32 on the device: 2 ulp for two terms), every step was clipped; without clipping the key is absent"""
    metrics, norms, mod = _fit(tiny_datamodule, tmp_path / "clipped", foreign, gradient_clip_val=1e-3)
    assert len(norms) == 4 and all(n > 1e-3 and 0 < c < 1 for n, c in norms), norms
    want = (norms[2][0] + norms[3][0]) / 2
    assert abs(metrics["train/grad_norm"] - want) <= 2 * np.spacing(np.float32(want)), (metrics["train/grad_norm"], want)
    if not foreign:
        assert any(v is not None for v in mod.__dict__.get("_step_graphs", {}).values()), getattr(mod, "step_graph_error", None)
        metrics, norms, _ = _fit(tiny_datamodule, tmp_path / "plain", foreign)
        assert "train/grad_norm" not in metrics and all(n == 0.0 and c == 1.0 for n, c in norms)


# ------------------------------------------------------------------------------------------------------ data parallel
DP_CLIP = 1e-3


def _dp_step(table, dev, feats, labels, masks, step_graph=True):
    """one clipped step of a fresh tiny module on these videos -> (norm, coefficient, parameters, clipped gradients)"""
    mod, net = _dp_module(table, geom="tiny")
    net.step_graph = step_graph
    mod.ncentroid = torch.zeros(D, device=dev)
    opt = mod.configure_optimizers()["optimizer"]
    f, l = feats.to(dev), labels.to(dev)
    h = f.shape[0] // 2
    net.selector_model.generate_mask = lambda b, m=masks: (m[0], m[1])
    mod.train_batch(((f[h:], l[h:]), (f[:h], l[:h])), opt, 0, gradient_clip_val=DP_CLIP, gradient_clip_algorithm="norm")
    torch.cuda.synchronize()
    assert any(v is not None for v in (mod.__dict__.get("_step_graphs") or {}).values()) == step_graph, getattr(mod, "step_graph_error", None)
    named = [(n, p) for n, p in net.named_parameters() if p.requires_grad]
    return (float(mod.last_grad_norm), float(mod.last_clip_coef), {n: p.detach().cpu() for n, p in named},
            {n: p.grad.detach().cpu() for n, p in named if p.grad is not None})


def _dp_worker(rank, world, port, q, backend):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    import json
    import torch.distributed as dist
    gpu = rank if backend == "nccl" else 0              # gloo: both ranks share the only GPU (CUDA tensors over gloo)
    torch.cuda.set_device(gpu)
    if backend == "nccl":
        dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", gpu))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from anomalyclip_amd import parallel
        import test_gpu_model
        import test_gpu_train
        test_gpu_model.DEV = test_gpu_train.DEV = dev = f"cuda:{gpu}"
        table = json.load(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "anomalyclip_amd", "data",
                                            "prompts.json")))
        feats, labels, masks = _dp_batch(8, D, 640)
        idx = parallel.shard_videos(8, world, rank)
        mk = [m[idx] for m in masks]
        norm, coef, params, grads = _dp_step(table, dev, feats[idx], labels[idx], mk)
        # the autograd fallback under data parallelism: finish() averages the buffer, the norm is then taken with scale 1 --
        # against g * (1 / world) read from the SUM in the graph path: the same bits at a world size that is a power of two
        n2, c2, p2, g2 = _dp_step(table, dev, feats[idx], labels[idx], mk, step_graph=False)
        differ = [k for k in params if not torch.equal(params[k], p2[k])] + [k for k in grads if not torch.equal(grads[k], g2[k])]
        paths = ("" if (n2, c2) == (norm, coef) else f"norm {norm} / {n2}, coefficient {coef} / {c2}; ") + ", ".join(differ)
        # the reference of test_train_batch_gradbuckets_world2: a third module's LOCAL gradients (plain autograd; SyncBN statistics
        # exchanged inside), summed over the ranks and divided by the world size by hand -- unclipped
        mod, net = _dp_module(table, geom="tiny")
        mod.ncentroid = torch.zeros(D, device=dev)
        net.selector_model.generate_mask = lambda b, m=mk: (m[0], m[1])
        f, l = feats[idx].to(dev), labels[idx].to(dev)
        h = len(idx) // 2
        with torch.enable_grad():
            mod.training_step(((f[h:], l[h:]), (f[:h], l[:h])))["loss"].backward()
        hand = {}
        for n, p in net.named_parameters():
            if p.grad is not None:
                gsum = p.grad.clone()
                dist.all_reduce(gsum)
                hand[n] = (gsum / world).cpu().contiguous().numpy()
        # numpy arrays travel by value (a tensor's shared-memory handle dies with this process)
        q.put((rank, norm, coef, paths, {n: t.numpy() for n, t in params.items()}, {n: t.contiguous().numpy() for n, t in grads.items()},
               hand))
    finally:
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("backend", ["nccl", "gloo"])
def test_clipped_step_two_ranks(backend):
    """two ranks with halves of a batch of 8, gradient_clip_algorithm "norm" biting, through the whole-step graph's data-parallel
    sequence (text exchange, mark, main exchange, join, one norm with 1 / world, both AdamW launches reading the record):
      * parameters, clipped gradients, norm and coefficient are bit-identical on both ranks -- the norm needs no collective;
      * the autograd fallback on the same ranks gives the same bits as the graph path;
      * the norm and the clipped gradients are within test_train_batch_gradbuckets_world2's 1e-5 of that test's reference, the
        ranks' local gradients averaged by hand, clipped by the fp64 restatement.
    "nccl" = RCCL, one GPU per rank (skips below 2 GPUs); "gloo" = the same device code with both ranks on ONE GPU.
    (What two ranks compute is the step on the MEAN of the ranks' losses.  That is not the whole batch's loss -- the smoothness
    term sums over the abnormal videos a rank sees, loss.py:10-17 -- so a single process on all 8 videos takes another step,
    with or without clipping: measured 1.9e-3 apart in the norm.)"""
    if backend == "nccl" and torch.cuda.device_count() < 2:
        pytest.skip(f"needs 2 GPUs (RCCL), found {torch.cuda.device_count()}")
    import socket
    import torch.multiprocessing as mp
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q, backend)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=600) for _ in procs], key=lambda r: r[0])
    for p in procs:
        p.join(timeout=60)
    (na, ca, paths_a, pa, ga, hand), (nb, cb, paths_b, pb, gb, _) = [
        r[1:4] + tuple({n: torch.from_numpy(a) for n, a in d.items()} for d in r[4:]) for r in res]
    print("norm: two ranks", na, nb, "coefficient", ca, cb)
    assert na == nb and ca == cb and 0 < ca < 1
    for n in pa:
        assert torch.equal(pa[n], pb[n]), n
    for n in ga:
        assert torch.equal(ga[n], gb[n]), n
    assert paths_a == "" and paths_b == "", (paths_a, paths_b)          # graph path == autograd fallback, on each rank
    want, want_norm = ref.clip([hand[n].numpy() for n in ga], "norm", DP_CLIP)
    assert set(ga) == set(hand) and abs(na - float(want_norm)) <= 1e-5 * float(want_norm)
    for n, w in zip(ga, want):
        assert relerr(ga[n], w) < 1e-5, n
