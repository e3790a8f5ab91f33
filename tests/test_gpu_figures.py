"""-m gpu: acx_curve_decimate against its restatement (tests/curve_decimate_ref.py, checked on the host in test_cpu_figures.py),
entry for entry; metrics.evaluate(figure_columns=W) beside the figure-less evaluate; Trainer.test leaves the four pictures."""
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import figures as F
from anomalyclip_amd import metrics as M
from anomalyclip_amd import ops

import curve_decimate_ref as DR

DEV = torch.device("cuda", 0)
POISON = 0x5A5A5A5A                       # past n_distinct: as a count it would land in the last column with the largest height
BIG = 2 ** 31 - 1
WAVE, GROUP, GROUPS = ops.CURVE_DECIMATE_WAVE_CHUNK, ops.CURVE_DECIMATE_CHUNK, ops.CURVE_DECIMATE_MAX_GROUPS


def record(P, N, k):
    r = L.CurveResult()
    r.n_pos, r.n_neg, r.n_distinct, r.opt_index, r.opt_threshold = int(P), int(N), int(k), -1, 1.0
    return torch.frombuffer(bytearray(bytes(r)), dtype=torch.uint8).to(DEV)


def device_curve(tps, fps, capacity):
    k = len(tps)
    t = np.full(capacity, POISON, dtype=np.int32)
    f = np.full(capacity, POISON, dtype=np.int32)
    t[:k], f[:k] = tps, fps
    return torch.from_numpy(t).to(DEV), torch.from_numpy(f).to(DEV)


def seeded(k, seed):
    tps, fps, P, N = DR.random_curve(np.random.default_rng(seed), k)
    if k and P == 0:
        tps, P = tps + 1, int(tps[-1]) + 1
    return tps, fps, P, N


def _cases():
    """name -> (tps, fps, P, N, columns to try, capacity)"""
    c = {}
    for k in (0, 1, 2, WAVE - 1, WAVE, WAVE + 1, GROUP - 1, GROUP, GROUP + 1):
        tps, fps, P, N = seeded(k, 100 + k) if k else (np.zeros(0, np.int32), np.zeros(0, np.int32), 5, 7)
        c[f"k{k}"] = (tps, fps, P, N, (1, 64), max(k, 1))
    tps, fps, P, N = seeded(100_003, 9)
    c["ragged_100003"] = (tps, fps, P, N, (8, 4096), 100_003)                      # a column spans several workgroups
    c["one_column_by_large_totals"] = (tps, fps, BIG, BIG, (8,), 100_003)          # every count * 8 < 2^31 - 1
    c["one_column_without_negatives"] = (tps + 1, np.zeros_like(fps), P + 1, 0, (8,), 100_003)      # the N == 0 rule (ROC only)
    c["capacity_past_k"] = (tps[:70_001], fps[:70_001], int(tps[70_000]), int(fps[70_000]), (64,), 100_003)
    tps, fps, P, N = seeded(GROUP * GROUPS + 75_713, 10)                           # workgroups walk more than one chunk each
    c["several_chunks_per_workgroup"] = (tps, fps, P, N, (64,), len(tps))
    # a column whose heights all tie (ROC: tps constant while fps crosses the column; PR: precision 1/2 = 2/4 = 3/6 ...)
    j = np.arange(1, 3001, dtype=np.int32)
    c["heights_tie_roc"] = (np.full(3000, 4, np.int32), j, 4, 3000, (1, 8), 3000)
    c["heights_tie_pr_equal_fractions"] = (j, j, 3000, 3000, (1, 8), 3000)
    c["counts_int32_max"] = (np.array([BIG - 2, BIG - 1, BIG - 1, BIG], np.int32), np.array([BIG - 3, BIG - 3, BIG, BIG], np.int32),
                             BIG, BIG, (1, 64, 4096), 4)
    tps, fps, P, N = seeded(5000, 12)
    c["no_positives"] = (np.zeros_like(tps), np.arange(1, 5001, dtype=np.int32), 0, 5000, (1, 64), 5000)
    return c


CASES = _cases()
_REF = {}


def reference(name, mode, W):
    if (name, mode, W) not in _REF:
        tps, fps, P, N, _, _ = CASES[name]
        _REF[(name, mode, W)] = DR.decimate(tps, fps, len(tps), P, N, mode, W)
    return _REF[(name, mode, W)]


@pytest.mark.parametrize("name", list(CASES))
def test_curve_decimate_equals_the_restatement(name):
    tps, fps, P, N, widths, capacity = CASES[name]
    t, f = device_curve(tps, fps, capacity)
    rec = record(P, N, len(tps))
    for W in widths:
        for mode in (DR.ROC, DR.PR):
            got = ops.curve_decimate(t, f, rec, mode, W)
            assert got.shape == (W, 4, 3) and got.dtype == torch.int32
            got = got.cpu().numpy().astype(np.int64)
            want = reference(name, mode, W)
            assert np.array_equal(got, want), (name, W, mode, np.argwhere(got != want)[:5].tolist())
            assert not (got == POISON).any()
    # what the cases are there for
    if name.startswith("one_column"):                                              # (ROC; the first one in PR as well)
        roc = reference(name, DR.ROC, 8)
        assert (roc[1:] == -1).all() and roc[0, 0, 0] == 0 and roc[0, 1, 0] == len(tps) - 1
    if name == "heights_tie_roc":
        roc = reference(name, DR.ROC, 8)
        assert (roc[:, 2, 0] == roc[:, 0, 0]).all() and (roc[:, 3, 0] == roc[:, 0, 0]).all() and (roc[:, 0, 0] >= 0).all()
    if name == "heights_tie_pr_equal_fractions":
        pr = reference(name, DR.PR, 8)
        assert (pr[:, 2, 0] == pr[:, 0, 0]).all() and (pr[:, 3, 0] == pr[:, 0, 0]).all() and (pr[:, 1, 0] > pr[:, 0, 0]).all()
    if name == "no_positives":
        assert (reference(name, DR.PR, 64) == -1).all()


def test_curve_decimate_without_any_capacity_and_refusals():
    empty = torch.empty(0, dtype=torch.int32, device=DEV)
    for mode in (DR.ROC, DR.PR):
        assert (ops.curve_decimate(empty, empty, record(0, 0, 0), mode, 64).cpu() == -1).all()
    t, f = device_curve(*seeded(10, 1)[:2], 10)
    for W in (0, 4097):
        with pytest.raises(L.AcxError):
            ops.curve_decimate(t, f, record(1, 1, 10), 0, W)
    with pytest.raises(L.AcxError):
        ops.curve_decimate(t, f, record(1, 1, 10), 2, 8)
    # a record that claims more points than the arrays hold is cut at the capacity
    tps, fps, P, N = seeded(10, 1)
    got = ops.curve_decimate(t, f, record(P, N, 1 << 40), 0, 8).cpu().numpy()
    assert np.array_equal(got, DR.decimate(tps, fps, 10, P, N, DR.ROC, 8))


def test_curve_decimate_is_deterministic():
    tps, fps, P, N, _, capacity = CASES["ragged_100003"]
    t, f = device_curve(tps, fps, capacity)
    rec = record(P, N, len(tps))
    for mode in (DR.ROC, DR.PR):
        a = ops.curve_decimate(t, f, rec, mode, 8).cpu().numpy().tobytes()
        b = ops.curve_decimate(t, f, rec, mode, 8).cpu().numpy().tobytes()
        assert a == b


# ====================================================================================================== evaluate
def _frames(n, seed, C=14, nid=7):
    rng = np.random.default_rng(seed)
    labels = rng.integers(0, C, n)
    labels[rng.random(n) < 0.55] = nid
    s = np.clip(0.45 * (labels != nid) + 0.6 * rng.random(n), 0, 1).astype(np.float32)
    s[: n // 3] = np.round(s[: n // 3] * 50) / 50                                  # ties: fewer thresholds than frames
    p = rng.random((n, C - 1)).astype(np.float32)
    p = (p / p.sum(1, keepdims=True) * s[:, None]).astype(np.float32)
    return (torch.from_numpy(x).to(DEV) for x in (s, labels.astype(np.int64), p))


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return a.dtype == b.dtype and torch.equal(a, b)
    if isinstance(a, np.ndarray):
        return a.dtype == b.dtype and a.tobytes() == b.tobytes()
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, float):
        return np.float64(a).tobytes() == np.float64(b).tobytes()
    return type(a) is type(b) and a == b


def test_evaluate_with_figure_columns(monkeypatch):
    C, nid, W = 14, 7, 64
    s, labels, p = _frames(5000, 21)
    plain = M.evaluate(s, labels, p, nid, C, curves=True)
    torch.cuda.synchronize()
    # count what waits for the device: Tensor.cpu / .item / .tolist / .numpy of a device tensor, torch.cuda.synchronize
    calls = []
    for name in ("cpu", "item", "tolist"):
        real = getattr(torch.Tensor, name)

        def counted(self, *a, _real=real, _name=name, **kw):
            if self.is_cuda:
                calls.append(_name)
            return _real(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, counted)
    real_sync = torch.cuda.synchronize
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: (calls.append("synchronize"), real_sync(*a, **kw))[1])
    got = M.evaluate(s, labels, p, nid, C, figure_columns=W)
    monkeypatch.undo()
    assert calls == ["cpu"], calls                                                 # exactly one device-to-host synchronisation
    figureless = M.evaluate(s, labels, p, nid, C)
    assert set(got) == set(figureless) | {"roc_points", "pr_points"}
    for k in figureless:
        assert _same(got[k], figureless[k]), k
    both = M.evaluate(s, labels, p, nid, C, curves=True, figure_columns=W)
    for k in plain:
        assert _same(both[k], plain[k]), k
    # the polylines: the restatement applied to the full device curves
    fpr, tpr, _ = plain["roc"]
    k = fpr.numel() - 1
    ks, vs = ops.sort_pairs_batched(s[None], labels.to(torch.int32), descending=True)
    res = torch.zeros(ops.CURVE_RESULT_BYTES, dtype=torch.uint8, device=DEV)
    tps, fps, _ = ops.clf_curve_batched(ks, vs, [nid], [True], res, curves=True)
    r = L.CurveResult.from_buffer_copy(res.cpu().numpy().tobytes())
    P, N = int(r.n_pos), int(r.n_neg)
    assert int(r.n_distinct) == k and 64 < k < 5000 and P > 0 and N > 0
    tps, fps = tps[:k].cpu().numpy(), fps[:k].cpu().numpy()
    for key, mode in (("roc_points", DR.ROC), ("pr_points", DR.PR)):
        x, y = got[key]
        wx, wy = DR.points(DR.decimate(tps, fps, k, P, N, mode, W), mode, P, N)
        assert x.dtype == y.dtype == np.float64 and len(x) <= 4 * W + 1
        assert np.array_equal(x, wx) and np.array_equal(y, wy), key
    assert (got["roc_points"][0][0], got["roc_points"][1][0]) == (0.0, 0.0)
    assert (got["pr_points"][0][0], got["pr_points"][1][0]) == (0.0, 1.0)
    with pytest.raises(ValueError):
        M.evaluate(s, labels, p, nid, C, figure_columns=5000)


# ====================================================================================================== the hook
import test_gpu_frames_mode as FM                      # the tiny-geometry module and its helpers (names only: no test is re-collected)
from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
from anomalyclip_amd.trainer import Trainer

NAMES = [f"Kind{i}" for i in range(7)] + ["Normal"] + [f"Kind{i}" for i in range(8, 14)]
FILES = ["F1.png", "PR.png", "ROC.png", "confusion_matrix.png", "metrics.json"]


def test_trainer_test_writes_the_four_figures(folders, tmp_path):
    root, frames, hp = folders
    labels_file = tmp_path / "labels.csv"
    labels_file.write_text("id,name\n" + "".join(f"{i},{n}\n" for i, n in enumerate(NAMES)))
    launches = []
    real = ops.curve_decimate

    def run(tag, labels, **hparams):
        base = tmp_path / tag
        mod, net = FM.build_module(False, base / "save", base / "logs")
        net.eval()
        mod.hparams.update(hparams)
        dm = AnomalyCLIPDataModule(**{**hp, "labels_file": labels}, frames_root=frames, load_from_features=False, encoder=net, decode="gpu")
        ops.curve_decimate = lambda *a, **kw: (launches.append(tag), real(*a, **kw))[1]
        try:
            metrics = Trainer().test(mod, dm)
        finally:
            ops.curve_decimate = real
        torch.cuda.synchronize()
        return mod, metrics, base / "logs" / "eval" / "runs" / "ckpt"

    mod, metrics, out = run("figures", str(labels_file))
    assert sorted(os.listdir(out)) == FILES
    assert launches == ["figures", "figures"]                                      # the ROC's and the PR curve's
    plain_mod, plain_metrics, plain_out = run("plain", str(labels_file), figures=False)
    assert os.listdir(plain_out) == ["metrics.json"] and launches == ["figures", "figures"]
    assert (out / "metrics.json").read_bytes() == (plain_out / "metrics.json").read_bytes()
    assert json.dumps(metrics, sort_keys=True) == json.dumps(plain_metrics, sort_keys=True)
    assert "roc_points" in mod.last_metrics and "roc_points" not in plain_mod.last_metrics
    for name, size in (("PR.png", (640, 480)), ("ROC.png", (640, 480)), ("F1.png", (640, 480)), ("confusion_matrix.png", (2000, 1800))):
        img = Image.open(out / name)
        assert img.format == "PNG" and img.size == size, name
    # the figures are those of figures.py for what evaluate returned, with the labels file's names on the ticks
    r = mod.last_metrics
    want = tmp_path / "want"
    want.mkdir()
    assert F.write_roc(want / "ROC.png", r["roc_points"], r["auc_roc"], F.DEFAULT_COLUMNS).read_bytes() == (out / "ROC.png").read_bytes()
    assert F.write_pr(want / "PR.png", r["pr_points"], r["auc_pr"], F.DEFAULT_COLUMNS).read_bytes() == (out / "PR.png").read_bytes()
    named = F.write_confusion(want / "named.png", r["confusion_matrix"], NAMES).read_bytes()
    assert named == (out / "confusion_matrix.png").read_bytes()
    # without a labels file the class indices label the ticks; `columns:` sets the plot box
    _, _, idx_out = run("indices", None, figures={"columns": 300})
    assert sorted(os.listdir(idx_out)) == FILES
    indexed = F.write_confusion(want / "indexed.png", r["confusion_matrix"], None).read_bytes()
    assert indexed == (idx_out / "confusion_matrix.png").read_bytes() and indexed != named
    assert (idx_out / "ROC.png").read_bytes() != (out / "ROC.png").read_bytes()
    assert (idx_out / "metrics.json").read_bytes() == (out / "metrics.json").read_bytes()


folders = FM.folders                                   # (the fixture of test_gpu_frames_mode, under its own name)
