"""-m gpu: Trainer.fit(ckpt_path=last.ckpt) continues a run bit for bit.  The 24 x 10 head on 512-wide features, four normal and
four abnormal feature files, batch_size 4 (two steps per epoch), real selector masks (the generators' states are what is under
test), AcxAdamW + WarmupCosineAnnealingLR(warmup_epochs=2, total_epoch=4), four epochs: an uninterrupted run A, a run B that is
interrupted after epoch 1, and a run C that resumes from the last.ckpt B left -- in a fresh module under other global seeds.
Every comparison of A with C is torch.equal; the only numeric bound is test_adamw_matches_torch's 1e-6 for a step of
torch.optim.AdamW against a step of AcxAdamW from the same loaded state."""
import json
import shutil
from functools import partial

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import checkpoint
from anomalyclip_amd.components.scheduler import WarmupCosineAnnealingLR
from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
from anomalyclip_amd.optim import AcxAdamW
from anomalyclip_amd.trainer import Trainer
from test_gpu_feature_bank import write_dataset
from test_gpu_model import relerr

DEV = torch.device("cuda", 0)
EPOCHS = 4
ANOMALY_T = (240, 1, 999, 64)


class Interrupted(Exception):
    pass


class CountingDataModule:
    """the datamodule, with a train_dataloader() that raises on its `fail_at_call`-th call (= before that epoch's first batch)"""

    def __init__(self, dm, fail_at_call=None):
        self._dm, self._calls, self._fail_at_call = dm, 0, fail_at_call

    def __getattr__(self, name):
        return getattr(self._dm, name)

    def train_dataloader(self):
        self._calls += 1
        if self._calls == self._fail_at_call:
            raise Interrupted()
        return self._dm.train_dataloader()


class Run:
    """one module + datamodule; fit() records the loss vector of every step and the optimizer / scheduler of the module (the same
    pair on every configure_optimizers() call: a second fit() of a live module meets its captured graphs and allocated moments)"""

    def __init__(self, hp, save_dir, step_graph=True, fail_at_call=None):
        from test_gpu_head_grid import FULL, _grid_module
        hc = FULL["24x10"]
        self.mod, self.net = _grid_module(hc)
        self.net.step_graph = step_graph
        self.mod.optimizer = partial(AcxAdamW, weight_decay=0.2)
        self.mod.scheduler = partial(WarmupCosineAnnealingLR, warmup_epochs=2, total_epoch=EPOCHS)
        self.mod.hparams["save_dir"] = str(save_dir)
        self.dm = CountingDataModule(AnomalyCLIPDataModule(**hp, num_segments=hc.num_segments, seg_length=hc.seg_length, batch_size=4),
                                     fail_at_call)
        self.losses, self.cfg = [], None
        configure, step = self.mod.configure_optimizers, self.mod.train_batch

        def configure_once():
            if self.cfg is None:
                self.cfg = configure()
            return self.cfg

        def recording(batch, opt, i=0):
            r = step(batch, opt, i)
            self.losses.append(torch.stack([torch.as_tensor(v).detach().reshape(()) for v in self.mod.last_losses]).clone())
            return r
        self.mod.configure_optimizers, self.mod.train_batch = configure_once, recording

    opt = property(lambda self: self.cfg["optimizer"])
    sched = property(lambda self: self.cfg["lr_scheduler"]["scheduler"])

    def fit(self, ckpt_path=None, root=None, val_every=EPOCHS + 1):
        self.trainer = Trainer(max_epochs=EPOCHS, check_val_every_n_epoch=val_every, default_root_dir=None if root is None else str(root))
        self.trainer.fit(self.mod, self.dm, ckpt_path=ckpt_path)
        torch.cuda.synchronize()
        return self

    def trained(self):
        """every trainable parameter and every buffer of the selector (BatchNorm statistics), the moments and the counters"""
        tensors = {n: p.detach().clone() for n, p in self.net.named_parameters() if p.requires_grad}
        tensors.update({"selector_model." + n: b.clone() for n, b in self.net.selector_model.named_buffers()})
        names = {id(p): n for n, p in self.net.named_parameters()}
        moments = {}
        for g in self.opt.param_groups:
            for p in g["params"]:
                st = self.opt.state.get(p)
                moments[names[id(p)]] = (st["step"], st["exp_avg"].clone(), st["exp_avg_sq"].clone()) if st else None
        return dict(tensors=tensors, moments=moments, last_epoch=self.sched.last_epoch, lrs=[g["lr"] for g in self.opt.param_groups],
                    global_step=self.trainer.global_step, current_epoch=self.trainer.current_epoch)


def assert_same(got, want):
    assert got["tensors"].keys() == want["tensors"].keys() and got["moments"].keys() == want["moments"].keys()
    for n, t in want["tensors"].items():
        assert torch.equal(got["tensors"][n], t), n
    for n, m in want["moments"].items():
        g = got["moments"][n]
        assert (g is None) == (m is None), n
        if m is not None:
            assert g[0] == m[0] == 2 * EPOCHS and torch.equal(g[1], m[1]) and torch.equal(g[2], m[2]), n
    for k in ("last_epoch", "lrs", "global_step", "current_epoch"):
        assert got[k] == want[k], k


@pytest.fixture(scope="module")
def dataset(tmp_path_factory):
    root = tmp_path_factory.mktemp("resume_data")
    hp = write_dataset(root, (5, 241, 300, 700), ANOMALY_T, (1, 13, 3, 5))
    # a temporal annotation file that marks a frame range of every test video abnormal: both classes exist in validation
    with open(root / "temporal.txt", "w") as fh:
        for i, T in enumerate(ANOMALY_T):
            fh.write(f"anomaly{i}_{T}.mp4 Anomaly {T // 3} {max(T // 3, 2 * T // 3 - 1)} -1 -1\n")
    return hp, str(root / "temporal.txt")


@pytest.fixture(scope="module")
def scenario(dataset, tmp_path_factory):
    """step_graph -> (A, A's end state, the copy of B's last.ckpt, C): computed once per path, shared by the tests"""
    hp, _ = dataset
    done = {}

    def run(step_graph):
        if step_graph not in done:
            root = tmp_path_factory.mktemp("graph" if step_graph else "autograd")
            torch.manual_seed(77)
            np.random.seed(78)
            a = Run(hp, root / "a", step_graph).fit()
            want = a.trained()
            torch.manual_seed(77)
            np.random.seed(78)
            b = Run(hp, root / "b", step_graph, fail_at_call=3)
            with pytest.raises(Interrupted):
                b.fit(root=root / "b")
            assert len(b.losses) == 4
            copy = str(root / "epoch1.ckpt")
            shutil.copyfile(root / "b" / "checkpoints" / "last.ckpt", copy)
            del b
            torch.manual_seed(5)                                    # other global seeds: the file's generator states decide
            np.random.seed(6)
            torch.cuda.manual_seed(7)
            c = Run(hp, root / "c", step_graph).fit(ckpt_path=copy)
            done[step_graph] = (a, want, copy, c)
        return done[step_graph]
    return run


# ====================================================================================================== 1
@pytest.mark.parametrize("step_graph", [True, False], ids=["step_graph", "autograd"])
def test_resume_equals_the_uninterrupted_run(scenario, step_graph):
    a, want, copy, c = scenario(step_graph)
    assert len(a.losses) == 2 * EPOCHS and len(c.losses) == 4        # C ran epochs 2 and 3 only
    for k, (got, ref) in enumerate(zip(c.losses, a.losses[4:])):
        assert torch.isfinite(got).all() and torch.equal(got, ref), (k, got, ref)
    assert len({tuple(l.tolist()) for l in a.losses}) == 2 * EPOCHS  # (the eight steps are eight different steps)
    got = c.trained()
    assert_same(got, want)
    assert got["global_step"] == 8 and got["current_epoch"] == 3 and got["last_epoch"] == 4
    # the frozen towers came through the file unchanged
    pa = dict(a.net.named_parameters())
    for n, p in c.net.named_parameters():
        if not p.requires_grad:
            assert torch.equal(p, pa[n]), n
    sgs = c.mod.__dict__.get("_step_graphs", {})
    assert (len(sgs) == 1 and all(v is not None for v in sgs.values())) if step_graph else not sgs, getattr(c.mod, "step_graph_error", None)
    ck = torch.load(copy, map_location="cpu", weights_only=False)
    assert ck["epoch"] == 1 and ck["global_step"] == 4 and ck["acx_resume"]["rng"][0]["cuda"] is not None
    assert ck["acx_resume"]["train_loaders"] == [{"epoch": 0, "shard_seed": None}] * 2


# ====================================================================================================== 2
def test_reload_into_a_live_module(scenario):
    """run A's module after its four epochs -- graphs captured, moments allocated -- is taken back to the end of epoch 1 by
    fit(ckpt_path=): the load goes INTO the moment tensors (the captured step holds their addresses), epochs 2-3 run again and
    end where they ended before"""
    a, want, copy, _ = scenario(True)
    ptrs = {n: (a.opt.state[p]["exp_avg"].data_ptr(), a.opt.state[p]["exp_avg_sq"].data_ptr())
            for n, p in a.net.named_parameters() if p.requires_grad and a.opt.state.get(p)}
    graphs = dict(a.mod.__dict__["_step_graphs"])
    assert len(ptrs) > 10 and len(graphs) == 1
    first = list(a.losses)
    a.fit(ckpt_path=copy)
    assert len(a.losses) == 12 and all(torch.equal(x, y) for x, y in zip(a.losses[8:], first[4:]))
    assert_same(a.trained(), want)
    for n, p in a.net.named_parameters():
        if n in ptrs:
            assert (a.opt.state[p]["exp_avg"].data_ptr(), a.opt.state[p]["exp_avg_sq"].data_ptr()) == ptrs[n], n
    assert a.mod.__dict__["_step_graphs"] == graphs                 # the same captured step, not a new one


# ====================================================================================================== 3
def test_optimizer_state_interop_with_torch(scenario):
    """torch.optim.AdamW's state_dict in a Lightning-shaped checkpoint -> AcxAdamW, and AcxAdamW's -> torch.optim.AdamW: the step
    after the load agrees within test_adamw_matches_torch's bound (relative 1e-6), both step counts are 4"""
    _, _, _, c = scenario(True)
    live = c.opt.param_groups
    g = torch.Generator().manual_seed(31)

    def clones(device):
        return [{"params": [torch.nn.Parameter(p.detach().clone().to(device)) for p in grp["params"]], "lr": 1e-3 * (i + 1),
                 "name": grp["name"]} for i, grp in enumerate(live)]

    def grads(params):
        return [None if p.numel() == 1 else torch.randn(p.shape, generator=g) * 0.1 for p in params]   # logit_scale: never a gradient

    cpu = clones("cpu")
    flat_cpu = [p for grp in cpu for p in grp["params"]]
    ref = torch.optim.AdamW(cpu, weight_decay=0.2)
    for _ in range(3):
        for p, gr in zip(flat_cpu, grads(flat_cpu)):
            p.grad = gr
        ref.step()
    # torch -> ours: the weights travel beside the state, as in a checkpoint
    dev = clones(DEV)
    flat_dev = [p for grp in dev for p in grp["params"]]
    with torch.no_grad():
        for p, q in zip(flat_dev, flat_cpu):
            p.copy_(q)
    ours = AcxAdamW(dev, weight_decay=0.2)
    state = checkpoint.load_training_state({"state_dict": {}, "epoch": 0, "global_step": 3, "pytorch-lightning_version": "1.8.3",
                                            "optimizer_states": [ref.state_dict()], "lr_schedulers": []}, ours)
    assert state == {"epoch": 0, "global_step": 3, "acx_resume": None}
    gs = grads(flat_cpu)
    for p, q, gr in zip(flat_cpu, flat_dev, gs):
        p.grad, q.grad = gr, None if gr is None else gr.to(DEV)
    ref.step()
    ours.step()
    for p, q in zip(flat_cpu, flat_dev):
        if p.numel() > 1:
            assert float(ref.state[p]["step"]) == 4 and ours.state[q]["step"] == 4 and isinstance(ours.state[q]["step"], int)
            assert relerr(q, p) < 1e-6
    # ours -> torch: the optimizer state of a file this trainer wrote
    saved = checkpoint.training_state(ours, None, [checkpoint.rng_state(DEV)], None, 1)["optimizer_states"][0]
    back = clones("cpu")
    flat_back = [p for grp in back for p in grp["params"]]
    with torch.no_grad():
        for p, q in zip(flat_back, flat_dev):
            p.copy_(q)
    other = torch.optim.AdamW(back, weight_decay=0.2)
    other.load_state_dict(saved)
    gs = grads(flat_cpu)
    for p, q, gr in zip(flat_back, flat_dev, gs):
        p.grad, q.grad = gr, None if gr is None else gr.to(DEV)
    other.step()
    ours.step()
    for p, q in zip(flat_back, flat_dev):
        if p.numel() > 1:
            assert float(other.state[p]["step"]) == 5 and ours.state[q]["step"] == 5
            assert relerr(q, p) < 1e-6


# ====================================================================================================== 4
def test_epoch_numbering_with_validation_on(dataset, tmp_path):
    """validation after every epoch: the resumed run writes metrics_2.json and metrics_3.json beside the interrupted run's
    metrics_0.json and metrics_1.json, which stay as they were, and the next last.ckpt carries epoch 3"""
    hp, temporal = dataset
    hp = dict(hp, annotation_file_temporal_test=temporal)
    save_dir = tmp_path / "run"
    torch.manual_seed(77)
    np.random.seed(78)
    b = Run(hp, save_dir, fail_at_call=3)
    with pytest.raises(Interrupted):
        b.fit(root=tmp_path / "b", val_every=1)
    copy = str(tmp_path / "epoch1.ckpt")
    shutil.copyfile(tmp_path / "b" / "checkpoints" / "last.ckpt", copy)
    assert sorted(p.name for p in save_dir.glob("metrics_*.json")) == ["metrics_0.json", "metrics_1.json"]
    before = [(save_dir / f"metrics_{e}.json").read_bytes() for e in (0, 1)]
    del b
    torch.manual_seed(5)
    np.random.seed(6)
    c = Run(hp, save_dir).fit(ckpt_path=copy, root=tmp_path / "c", val_every=1)
    assert len(c.losses) == 4
    assert sorted(p.name for p in save_dir.glob("metrics_*.json")) == [f"metrics_{e}.json" for e in range(4)]
    assert [(save_dir / f"metrics_{e}.json").read_bytes() for e in (0, 1)] == before
    for e in range(4):
        m = json.load(open(save_dir / f"metrics_{e}.json"))
        assert m["epoch"] == e and 0.0 <= m["auc_roc"] <= 1.0
    ck = torch.load(tmp_path / "c" / "checkpoints" / "last.ckpt", map_location="cpu", weights_only=False)
    assert ck["epoch"] == 3 and ck["global_step"] == 8 and ck["lr_schedulers"][0]["last_epoch"] == 4
    states = ck["optimizer_states"][0]["state"]                     # the resumed run's own file can be resumed from: no empty entries
    assert 0 not in states and all(set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 8 for st in states.values())
