"""Host only: what `Trainer.save_checkpoint` writes and `Trainer.fit(ckpt_path=)` restores, on a stub module without kernels (the
style of test_cpu_host.py's trainer test).  The stub's `train_batch` draws from torch's CPU generator and from numpy's global one
and moves the optimizer state the way AcxAdamW does, so a resumed run can be compared draw by draw with an uninterrupted one."""
import io
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ("selector_model", "temporal_model", "prompt_learner", "text_projection")
SHAPES = {"selector_model": [(1,)], "temporal_model": [(6, 4), (6,), (3, 6)], "prompt_learner": [(5, 2, 4)], "text_projection": [(4, 3)]}


class Net(torch.nn.Module):
    """four parameter groups with the names of configure_optimizers()'s (anomaly_clip_module.py), and one buffer"""

    def __init__(self, seed=0, shapes=SHAPES):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        for name in GROUPS:
            setattr(self, name, torch.nn.ParameterList([torch.nn.Parameter(torch.randn(*s, generator=g)) for s in shapes[name]]))
        self.register_buffer("running", torch.zeros(3))


class Loader(list):
    """an iterable that yields this rank's shard itself, with ResidentTrainLoader's counters"""
    already_sharded = True

    def __init__(self, items):
        super().__init__(items)
        self._epoch, self._shard_seed = 0, None

    def set_epoch(self, e):
        self._epoch = int(e)


class DataModule:
    def __init__(self, fail_at_call=None):
        self.loaders = [Loader([("n0", 0), ("n1", 1)]), Loader([("a0", 0), ("a1", 1)])]
        self.calls, self.fail_at_call = 0, fail_at_call

    def setup(self, stage):
        pass

    def train_dataloader(self):
        self.calls += 1
        if self.calls == self.fail_at_call:
            raise Interrupted()
        if self.loaders[0]._shard_seed is None:
            for l in self.loaders:
                l._shard_seed = 1234                                # as if agreed on at first use
        return self.loaders


class Interrupted(Exception):
    pass


class Stub:
    device = torch.device("cpu")

    def __init__(self, seed=0, shapes=SHAPES):
        self.hparams = {"save_dir": None}
        self.net = Net(seed, shapes)
        self.calls, self.draws, self.epochs = [], [], []

    def configure_optimizers(self):
        from anomalyclip_amd.components.scheduler import WarmupCosineAnnealingLR
        from anomalyclip_amd.optim import AcxAdamW
        self.calls.append("configure_optimizers")
        groups = [{"params": list(getattr(self.net, n)), "lr": 1e-3 * (i + 1), "name": n} for i, n in enumerate(GROUPS)]
        opt = AcxAdamW(groups, weight_decay=0.2)
        successor = torch.optim.lr_scheduler.CosineAnnealingLR(opt, 4.0)
        sch = WarmupCosineAnnealingLR(opt, total_epoch=4, successor=successor, warmup_epochs=2)
        self.opt, self.sched = opt, sch
        return {"optimizer": opt, "lr_scheduler": {"scheduler": sch, "monitor": "train/loss", "interval": "epoch", "frequency": 1}}

    def on_train_start(self):
        self.calls.append("on_train_start")
        torch.rand(3)                                               # a hook that draws: the resumed epoch must not see it
        np.random.rand(3)

    def train_batch(self, batch, opt, i):
        """draws like a training step (mask, segment starts), then an AdamW-shaped update: state created like AcxAdamW.step"""
        self.calls.append(f"train_batch{i}")
        self.epochs.append(self.trainer.current_epoch)
        draw = (float(torch.rand(1)), float(np.random.rand()), tuple(g["lr"] for g in opt.param_groups))
        self.draws.append(draw)
        with torch.no_grad():
            for g in opt.param_groups:
                for p in g["params"]:
                    if p.shape == (1,):
                        continue                                    # the never-used logit_scale: no gradient, no state
                    st = opt.state[p]
                    if not st:
                        st["step"] = 0
                        st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                        st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["step"] += 1
                    grad = torch.full_like(p, draw[0] - draw[1])
                    st["exp_avg"].mul_(0.9).add_(grad, alpha=0.1)
                    st["exp_avg_sq"].mul_(0.999).addcmul_(grad, grad, value=0.001)
                    p.sub_(g["lr"] * st["exp_avg"] / (st["exp_avg_sq"].sqrt() + 1e-8))
            self.net.running += draw[1]

    def on_train_epoch_end(self):
        self.calls.append("on_train_epoch_end")


def trainer(tmp_path=None, max_epochs=4):
    from anomalyclip_amd.trainer import Trainer
    return Trainer(max_epochs=max_epochs, check_val_every_n_epoch=max_epochs + 1, default_root_dir=str(tmp_path) if tmp_path else None)


def seed(a, b):
    torch.manual_seed(a)
    np.random.seed(b)


def end_state(m):
    moments = [(m.opt.state[p].get("step"), m.opt.state[p].get("exp_avg"), m.opt.state[p].get("exp_avg_sq"))
               for g in m.opt.param_groups for p in g["params"]]
    return ({k: v.clone() for k, v in m.net.state_dict().items()}, moments, m.sched.last_epoch, [g["lr"] for g in m.opt.param_groups])


def assert_same_end_state(a, b):
    assert a[0].keys() == b[0].keys() and all(torch.equal(a[0][k], b[0][k]) for k in a[0])
    assert len(a[1]) == len(b[1])
    for (sa, ma, va), (sb, mb, vb) in zip(a[1], b[1]):
        assert sa == sb and (ma is None) == (mb is None)
        if ma is not None:
            assert torch.equal(ma, mb) and torch.equal(va, vb)
    assert a[2:] == b[2:]


def our_warnings(rec):
    return [str(w.message) for w in rec if "checkpoint" in str(w.message) and ("resume" in str(w.message) or "weights only" in str(w.message))]


@pytest.fixture()
def interrupted(tmp_path):
    """run A (uninterrupted, four epochs) and the last.ckpt a run B left that stopped after epoch 1"""
    seed(77, 78)
    a = Stub()
    trainer().fit(a, DataModule())
    seed(77, 78)
    b = Stub()
    with pytest.raises(Interrupted):
        trainer(tmp_path / "b").fit(b, DataModule(fail_at_call=3))
    return a, str(tmp_path / "b" / "checkpoints" / "last.ckpt")


# ====================================================================================================== what a checkpoint holds
def test_checkpoint_layout(interrupted):
    a, path = interrupted
    ck = torch.load(path, weights_only=False)
    assert set(ck) >= {"state_dict", "epoch", "global_step", "hyper_parameters", "pytorch-lightning_version", "optimizer_states",
                       "lr_schedulers", "acx_resume"}
    assert ck["epoch"] == 1 and ck["global_step"] == 4
    assert len(ck["optimizer_states"]) == 1 and len(ck["lr_schedulers"]) == 1
    osd = ck["optimizer_states"][0]
    # torch's layout: groups hold running indices, state is keyed by them
    assert [g["params"] for g in osd["param_groups"]] == [[0], [1, 2, 3], [4], [5]]
    assert [g["name"] for g in osd["param_groups"]] == list(GROUPS)
    assert sorted(osd["state"]) == [1, 2, 3, 4, 5]                  # logit_scale never had a gradient
    flat = [s for n in GROUPS for s in SHAPES[n]]
    for idx, st in osd["state"].items():
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"}
        assert torch.is_tensor(st["step"]) and st["step"].dtype == torch.float32 and st["step"].dim() == 0 and float(st["step"]) == 4
        assert st["exp_avg"].device.type == "cpu" and tuple(st["exp_avg"].shape) == tuple(st["exp_avg_sq"].shape) == flat[idx]
    sch = ck["lr_schedulers"][0]
    assert "successor" not in sch and sch["last_epoch"] == 2 and sch["total_epoch"] == 4 and sch["warmup_epochs"] == [2] * 4
    acx = ck["acx_resume"]
    assert acx["world_size"] == 1 and len(acx["rng"]) == 1 and set(acx["rng"][0]) == {"torch_cpu", "cuda", "numpy"}
    assert acx["train_loaders"] == [{"epoch": 0, "shard_seed": 1234}] * 2

    def walk(o, where):                                            # plain data only: no optimizer, scheduler or module object
        assert not isinstance(o, (torch.optim.Optimizer, torch.optim.lr_scheduler._LRScheduler, torch.nn.Module)), where
        if isinstance(o, dict):
            for k, v in o.items():
                walk(v, f"{where}[{k!r}]")
        elif isinstance(o, (list, tuple)):
            for i, v in enumerate(o):
                walk(v, f"{where}[{i}]")
        else:
            assert o is None or isinstance(o, (bool, int, float, str, torch.Tensor)), (where, type(o))
    for key in ("optimizer_states", "lr_schedulers", "acx_resume"):
        walk(ck[key], key)


def test_checkpoint_loads_in_torch_without_the_package(interrupted):
    """torch.optim.AdamW and a torch scheduler take the file's states in a process that never imports anomalyclip_amd"""
    _, path = interrupted
    shapes = [s for n in GROUPS for s in SHAPES[n]]
    code = f"""
import sys, torch
ck = torch.load({path!r}, weights_only=False)
assert not any(m.startswith("anomalyclip_amd") for m in sys.modules)
ps = [torch.nn.Parameter(torch.zeros(*s)) for s in {shapes!r}]
opt = torch.optim.AdamW([dict(params=ps[:1]), dict(params=ps[1:4]), dict(params=ps[4:5]), dict(params=ps[5:])], weight_decay=0.2)
opt.load_state_dict(ck["optimizer_states"][0])
assert float(opt.state[ps[1]]["step"]) == 4 and opt.param_groups[1]["name"] == "temporal_model"
for p in ps:
    p.grad = torch.ones_like(p)
opt.step()
assert float(opt.state[ps[1]]["step"]) == 5
sch = torch.optim.lr_scheduler.StepLR(opt, 1)
sch.load_state_dict(ck["lr_schedulers"][0])
assert sch.last_epoch == 2
print("ok")
"""
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]


def test_scheduler_round_trip():
    """saved after each of four epochs, restored into a fresh optimizer + scheduler: the remaining learning rates are the
    uninterrupted schedule's"""
    from anomalyclip_amd import checkpoint
    a = Stub()
    a.configure_optimizers()
    want = []
    for epoch in range(4):
        a.sched.step()
        want.append([g["lr"] for g in a.opt.param_groups])
        buf = io.BytesIO()
        torch.save({"optimizer_states": [checkpoint.optimizer_state_dict(a.opt)],
                    "lr_schedulers": [checkpoint.scheduler_state_dict(a.sched)], "epoch": epoch}, buf)
        buf.seek(0)
        c = Stub(seed=5)
        c.configure_optimizers()
        successor = c.sched.successor
        state = checkpoint.load_training_state(torch.load(buf, weights_only=False), c.opt, c.sched)
        assert state["epoch"] == epoch and c.sched.successor is successor and c.sched.last_epoch == a.sched.last_epoch
        assert [g["lr"] for g in c.opt.param_groups] == want[-1] and c.sched.get_last_lr() == a.sched.get_last_lr()
        later = []
        for _ in range(epoch + 1, 4):
            c.sched.step()
            later.append([g["lr"] for g in c.opt.param_groups])
        # the uninterrupted schedule, from a scheduler of its own
        b = Stub()
        b.configure_optimizers()
        full = []
        for _ in range(4):
            b.sched.step()
            full.append([g["lr"] for g in b.opt.param_groups])
        assert later == full[epoch + 1:]
    assert [w[0] for w in want] == [0.0005, 0.001, pytest.approx(0.0005), pytest.approx(0.0, abs=1e-18)]   # warm-up, peak, half cosine, end


def test_atomic_save(interrupted, monkeypatch):
    """a save that dies half way leaves the previous last.ckpt whole and no temporary file"""
    a, path = interrupted
    before = open(path, "rb").read()
    real_save = torch.save

    def half_then_die(obj, f, *args, **kw):
        buf = io.BytesIO()
        real_save(obj, buf)
        with open(f, "wb") as fh:
            fh.write(buf.getvalue()[: len(buf.getvalue()) // 2])
        raise OSError("killed during the save")
    tr = trainer(os.path.dirname(os.path.dirname(path)))
    tr._optimizer, tr._scheduler, tr.current_epoch, tr.global_step = a.opt, a.sched, 3, 8
    monkeypatch.setattr(torch, "save", half_then_die)
    with pytest.raises(OSError, match="killed"):
        tr.save_checkpoint(a, path)
    monkeypatch.setattr(torch, "save", real_save)
    assert os.listdir(os.path.dirname(path)) == ["last.ckpt"]
    assert open(path, "rb").read() == before and torch.load(path, weights_only=False)["epoch"] == 1
    tr.save_checkpoint(a, path)                                      # and an undisturbed save replaces it
    assert os.listdir(os.path.dirname(path)) == ["last.ckpt"] and torch.load(path, weights_only=False)["epoch"] == 3


# ====================================================================================================== resuming
def test_resume_equals_uninterrupted_run(interrupted):
    a, path = interrupted
    seed(1, 2)                                                       # other global seeds: the file's generator states decide
    c = Stub(seed=9)
    dm = DataModule()
    tr = trainer()
    with warnings.catch_warnings(record=True) as rec:
        warnings.simplefilter("always")
        tr.fit(c, dm, ckpt_path=path)
    assert not our_warnings(rec)
    assert c.epochs == [2, 2, 3, 3] and c.draws == a.draws[4:] and tr.global_step == 8 and tr.current_epoch == 3
    assert_same_end_state(end_state(c), end_state(a))
    assert [(l._epoch, l._shard_seed) for l in dm.loaders] == [(0, 1234)] * 2


def test_resume_from_the_file_of_a_resumed_run(interrupted, tmp_path):
    """pre-empted twice: B stops after epoch 1, C resumes and stops after epoch 2, D resumes from C's last.ckpt and ends where the
    uninterrupted run ends.  A parameter without optimizer state (logit_scale) has no entry in either file."""
    a, path = interrupted
    seed(1, 2)
    c = Stub(seed=9)
    with pytest.raises(Interrupted):
        trainer(tmp_path / "c").fit(c, DataModule(fail_at_call=2), ckpt_path=path)
    assert c.epochs == [2, 2] and c.net.selector_model[0] not in c.opt.state
    second = str(tmp_path / "c" / "checkpoints" / "last.ckpt")
    ck = torch.load(second, weights_only=False)
    assert ck["epoch"] == 2 and ck["global_step"] == 6 and sorted(ck["optimizer_states"][0]["state"]) == [1, 2, 3, 4, 5]
    assert os.listdir(os.path.dirname(second)) == ["last.ckpt"]
    seed(3, 4)
    d = Stub(seed=11)
    tr = trainer()
    tr.fit(d, DataModule(), ckpt_path=second)
    assert d.epochs == [3, 3] and d.draws == a.draws[6:] and tr.global_step == 8
    assert_same_end_state(end_state(d), end_state(a))
    # a file that does carry an empty entry (written by something else) is read as if the entry were absent
    from anomalyclip_amd import checkpoint
    ck["optimizer_states"][0]["state"][0] = {}
    e = Stub(seed=12)
    e.configure_optimizers()
    checkpoint.load_training_state(ck, e.opt, e.sched)
    assert e.net.selector_model[0] not in e.opt.state and all(e.opt.state[p]["step"] == 6 for p in e.net.temporal_model)


def test_changed_hyper_parameters_are_replaced_with_a_warning(interrupted):
    """like torch's load_state_dict the file's group hyper-parameters win; a configured value other than lr that differs is named"""
    from anomalyclip_amd import checkpoint
    _, path = interrupted
    c = Stub(seed=9)
    c.configure_optimizers()
    c.opt.param_groups[1]["weight_decay"] = 0.5
    with pytest.warns(UserWarning, match=r"temporal_model.*weight_decay = 0.2 \(configured: 0.5\)"):
        checkpoint.load_training_state(torch.load(path, weights_only=False), c.opt, c.sched)
    assert c.opt.param_groups[1]["weight_decay"] == 0.2


def test_reload_into_live_optimizer_keeps_the_moment_tensors(interrupted):
    """load_training_state copies INTO the state tensors an optimizer already has (a captured step graph holds their addresses)"""
    from anomalyclip_amd import checkpoint
    a, path = interrupted
    ptrs = [(a.opt.state[p]["exp_avg"].data_ptr(), a.opt.state[p]["exp_avg_sq"].data_ptr()) for p in a.net.temporal_model]
    ck = torch.load(path, weights_only=False)
    checkpoint.load_training_state(ck, a.opt, a.sched)
    for k, p in enumerate(a.net.temporal_model):
        st = a.opt.state[p]
        assert (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr()) == ptrs[k] and st["step"] == 4 and isinstance(st["step"], int)
        assert torch.equal(st["exp_avg"], ck["optimizer_states"][0]["state"][1 + k]["exp_avg"])
    assert a.sched.last_epoch == 2 and a.net.selector_model[0] not in a.opt.state


def test_weight_only_file_starts_at_epoch_0_and_warns_once(interrupted, tmp_path):
    a, path = interrupted
    ck = torch.load(path, weights_only=False)
    old = str(tmp_path / "old.ckpt")
    torch.save({k: ck[k] for k in ("state_dict", "epoch", "global_step", "hyper_parameters")}, old)   # what last.ckpt used to hold
    bare = str(tmp_path / "bare.pt")
    torch.save(ck["state_dict"], bare)
    fresh = Stub(seed=9)
    trainer(max_epochs=2).fit(fresh, DataModule())
    for f in (old, bare):
        c = Stub(seed=9)
        tr = trainer(max_epochs=2)
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            tr.fit(c, DataModule(), ckpt_path=f)
        assert len(our_warnings(rec)) == 1 and "weights only" in our_warnings(rec)[0]
        assert c.calls == fresh.calls and c.epochs == [0, 0, 1, 1] and tr.global_step == 4 and tr.ckpt_path == f
        assert c.draws[0][2] == fresh.draws[0][2] == (0.0,) * 4     # the schedule starts over: warm-up from 0
        assert all(c.opt.state[p]["step"] == 4 for p in c.net.temporal_model)


def test_finished_run_trains_nothing(interrupted, tmp_path):
    a, path = interrupted
    c = Stub(seed=9)
    tr = trainer(tmp_path / "c", max_epochs=2)                       # the file was saved at the end of epoch 1 = max_epochs - 1
    assert tr.fit(c, DataModule(), ckpt_path=path) == {}
    assert not [x for x in c.calls if x.startswith("train_batch")] and tr.global_step == 4 and tr.current_epoch == 1
    assert not os.path.exists(tmp_path / "c")                        # and wrote nothing


def test_world_size_mismatch_restores_everything_but_the_generators(interrupted, tmp_path):
    a, path = interrupted
    ck = torch.load(path, weights_only=False)
    lightning = str(tmp_path / "lightning.ckpt")                     # a Lightning-written file has no acx_resume
    torch.save({k: v for k, v in ck.items() if k != "acx_resume"}, lightning)
    ck["acx_resume"]["world_size"] = 2
    ck["acx_resume"]["rng"] = ck["acx_resume"]["rng"] * 2
    other = str(tmp_path / "world2.ckpt")
    torch.save(ck, other)
    for f, word in ((other, "world size 2"), (lightning, "no generator states")):
        seed(1, 2)
        torch.rand(3)
        np.random.rand(3)
        want = (float(torch.rand(1)), float(np.random.rand()))       # what the generators give after on_train_start's draws
        seed(1, 2)
        c = Stub(seed=9)
        tr = trainer()
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            tr.fit(c, DataModule(), ckpt_path=f)
        assert len(our_warnings(rec)) == 1 and word in our_warnings(rec)[0], our_warnings(rec)
        assert c.draws[0][:2] == want                                # untouched
        assert c.epochs == [2, 2, 3, 3] and tr.global_step == 8
        assert [d[2] for d in c.draws] == [d[2] for d in a.draws[4:]]                 # the schedule continues
        assert all(c.opt.state[p]["step"] == 8 for p in c.net.temporal_model) and c.sched.last_epoch == 4


@pytest.mark.parametrize("what", ["one tensor fewer", "wrong shape"])
def test_mismatched_optimizer_state_is_refused(interrupted, what):
    _, path = interrupted
    shapes = dict(SHAPES)
    shapes["temporal_model"] = [(6, 4), (6,)] if what == "one tensor fewer" else [(6, 4), (6,), (3, 7)]
    c = Stub(seed=9, shapes=shapes)
    c.configure_optimizers()
    from anomalyclip_amd import checkpoint
    ck = torch.load(path, weights_only=False)
    want = r"temporal_model.*\(6,\).*holds 3" if what == "one tensor fewer" else r"temporal_model.*\(3, 7\).*\(3, 6\)"
    with pytest.raises(ValueError, match=want):
        checkpoint.load_training_state(ck, c.opt, c.sched)
    assert not any(c.opt.state[p] for g in c.opt.param_groups for p in g["params"]) and c.sched.last_epoch == 0   # nothing was touched


# ====================================================================================================== gloo, world 2
def _worker(rank, world, port, root, q):
    sys.path.insert(0, REPO)
    sys.path.insert(0, os.path.join(REPO, "tests"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import test_cpu_resume as T
    T.seed(100 + rank, 200 + rank)
    b = T.Stub()
    T.trainer(root, max_epochs=2).fit(b, T.DataModule())
    dist.barrier()
    path = os.path.join(root, "checkpoints", "last.ckpt")
    ok = os.path.isfile(path) and os.listdir(os.path.dirname(path)) == ["last.ckpt"]
    acx = torch.load(path, weights_only=False)["acx_resume"]
    ok &= acx["world_size"] == 2 and len(acx["rng"]) == 2 and not torch.equal(acx["rng"][0]["torch_cpu"], acx["rng"][1]["torch_cpu"])
    want = (float(torch.rand(1)), float(np.random.rand()))           # this rank's generators stand where the save left them
    T.seed(7, 7)                                                     # the same junk on both ranks
    c = T.Stub(seed=9)
    dist.barrier()                                                   # both ranks have read the file before anyone writes the next one
    tr = T.trainer(os.path.join(root, "resumed"), max_epochs=3)
    tr.fit(c, T.DataModule(), ckpt_path=path)
    ok &= c.epochs == [2, 2] and c.draws[0][:2] == want and tr.global_step == 6
    ok &= all(c.opt.state[p]["step"] == 6 for p in c.net.temporal_model)
    q.put((rank, bool(ok), want))
    dist.barrier()
    dist.destroy_process_group()


def test_gloo_world2_each_rank_gets_its_own_generators_back(tmp_path):
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, str(tmp_path), q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in procs)
    for p in procs:
        p.join(timeout=60)
    assert [r[:2] for r in res] == [(0, True), (1, True)], res
    assert res[0][2] != res[1][2]                                    # the two ranks' streams differ
