"""-m gpu: Trainer.predict on the tiny geometry of test_gpu_frames_mode.py, in frames mode, over a three-column predict list: the
per-video scores are those of score_videos over the test loader's batches, events.json is tests/events_ref.py applied to them,
scores/<video>.npy holds them, and under the defaults the events are the runs of acx_test_counts' y_pred != normal_idx."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import events as EV
from anomalyclip_amd import ops
from anomalyclip_amd.datamodule import AnomalyCLIPDataModule, ResidentTestLoader
from anomalyclip_amd.trainer import Trainer, _to_device

import events_ref as ER
import test_gpu_frames_mode as FM                      # the tiny-geometry module and its helpers (names only: no test is re-collected)

folders = FM.folders                                   # (the fixture of test_gpu_frames_mode, under its own name)
DEV = FM.DEV
NAMES = [f"Kind{i}" for i in range(7)] + ["Normal"] + [f"Kind{i}" for i in range(8, 14)]


def expected_videos(paths, scores, probs, normal_idx, names=None, **kw):
    """the "videos" list of events.json from the restatement (the mean: the f64 reference's, compared within its bound)"""
    s = np.concatenate([x for x in scores])
    p = np.concatenate([x for x in probs])
    off = np.concatenate([[0], np.cumsum([len(x) for x in scores])]).astype(np.int64)
    count, events, stats = ER.find_events_ref(s, p, off, normal_idx, **kw)
    E = kw["max_events"]
    out = []
    for v, path in enumerate(paths):
        evs = []
        for j in range(min(int(count[v]), E)):
            d = {f: int(x) for f, x in zip(EV.EVENT_FIELDS, events[v, j])}
            d.update(peak=float(stats[v, j, 0]), mean=float(stats[v, j, 1]))
            if names is not None:
                d["class_name"] = names[d["class"]]
            evs.append(d)
        out.append({"video": path, "count": int(count[v]), "truncated": bool(count[v] > E), "events": evs})
    return out


def assert_videos_equal(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert {k: g[k] for k in ("video", "count", "truncated")} == {k: w[k] for k in ("video", "count", "truncated")}
        assert len(g["events"]) == len(w["events"])
        for a, b in zip(g["events"], w["events"]):
            assert {k: v for k, v in a.items() if k != "mean"} == {k: v for k, v in b.items() if k != "mean"}
            assert abs(a["mean"] - b["mean"]) <= (b["end"] - b["start"] + 1) * 2.0 ** -52 * abs(b["mean"])


def test_trainer_predict(folders, tmp_path):
    root, frames, hp = folders
    plist = tmp_path / "predict.txt"
    plist.write_text("".join(f"{v} {a} {b}\n" for v, _, a, b, _ in FM.TEST))                  # three columns: no label
    labels_file = tmp_path / "labels.csv"
    labels_file.write_text("id,name\n" + "".join(f"{i},{n}\n" for i, n in enumerate(NAMES)))
    base = tmp_path / "run"
    mod, net = FM.build_module(False, base / "save", base / "logs")
    net.eval()
    dm = AnomalyCLIPDataModule(**{**hp, "labels_file": str(labels_file), "annotation_file_predict": str(plist)}, frames_root=frames,
                               load_from_features=False, encoder=net, decode="gpu")
    # ---- neither hparams.predict.threshold nor the evaluation's metrics.json
    with pytest.raises(ValueError, match=r"metrics\.json.*predict\.threshold"):
        Trainer().predict(mod, dm)
    assert not (base / "logs" / "predict").exists()
    loader = dm.predict_dataloader()
    assert isinstance(loader, ResidentTestLoader) and len(loader) == len(FM.TEST)
    for (tile, lab, label, S, path), (v, _, a, b, _) in zip(loader, FM.TEST):
        assert lab.shape == (1, b - a + 1) and bool((lab == FM.NORMAL_ID).all()) and int(label) == FM.NORMAL_ID
        assert path == [os.path.join(frames, v)]
    # ---- what the test loader's batches of the same videos score, in the same grouping (both videos in one forward)
    with torch.no_grad():
        want = mod.score_videos([_to_device(b, DEV) for b in dm.test_dataloader()])
    w_scores = [s.cpu().numpy() for s, _, _ in want]
    w_probs = [p.cpu().numpy() for _, _, p in want]
    assert [len(s) for s in w_scores] == [b - a + 1 for _, _, a, b, _ in FM.TEST] and w_probs[0].shape[1] == FM.NUM_CLASSES - 1
    thr = float(np.sort(np.concatenate(w_scores))[len(np.concatenate(w_scores)) // 2])          # a score that occurs: equality with hi
    low = float(np.sort(np.concatenate(w_scores))[len(np.concatenate(w_scores)) // 4])
    paths = [os.path.join(frames, v) for v, *_ in FM.TEST]

    # ---- hysteresis, merging and a length filter from hparams.predict
    mod.hparams["predict"] = {"threshold": thr, "low": low, "max_gap": 2, "min_len": 2, "max_events": 16}
    res = Trainer().predict(mod, dm)
    torch.cuda.synchronize()
    assert [r["path"] for r in res] == paths
    for r, (s, _, p) in zip(res, want):
        assert torch.equal(r["abnormal_scores"], s) and torch.equal(r["class_probs"], p)
    out = base / "logs" / "predict" / "runs" / "ckpt"
    assert sorted(os.listdir(out)) == ["events.json", "scores"] and sorted(os.listdir(out / "scores")) == ["t0.npy", "t1.npy"]
    doc = json.load(open(out / "events.json"))
    kw = dict(hi=thr, lo=low, max_gap=2, min_len=2, max_events=16)
    assert doc["params"] == {"threshold": thr, "low": low, "max_gap": 2, "min_len": 2, "max_events": 16, "save_scores": True,
                             "normal_idx": FM.NORMAL_ID}
    assert_videos_equal(doc["videos"], expected_videos(paths, w_scores, w_probs, FM.NORMAL_ID, NAMES, **kw))
    assert_videos_equal([{"video": r["path"], "count": r["events"].total, "truncated": r["events"].truncated,
                          "events": [{**e, "class_name": NAMES[e["class"]]} for e in r["events"]]} for r in res], doc["videos"])
    for name, s, p in zip(("t0", "t1"), w_scores, w_probs):
        table = np.load(out / "scores" / f"{name}.npy")
        assert table.dtype == np.float32 and table.shape == (len(s), FM.NUM_CLASSES)
        assert np.array_equal(table[:, 0], s) and np.array_equal(table[:, 1:], p)

    # ---- the defaults, threshold from the evaluation's metrics.json: the runs of the reference's own prediction rule
    plain = tmp_path / "plain"
    mod2, net2 = FM.build_module(False, plain / "save", plain / "logs")
    net2.eval()
    mod2.hparams["predict"] = {"save_scores": False}
    ev_dir = plain / "logs" / "eval" / "runs" / "ckpt"
    ev_dir.mkdir(parents=True)
    (ev_dir / "metrics.json").write_text(json.dumps({"optimal_threshold": thr, "auc_roc": 0.5}))
    dm2 = AnomalyCLIPDataModule(**{**hp, "annotation_file_predict": str(plist)}, frames_root=frames, load_from_features=False,
                                encoder=net2, decode="gpu")
    res2 = Trainer().predict(mod2, dm2)
    out2 = plain / "logs" / "predict" / "runs" / "ckpt"
    assert os.listdir(out2) == ["events.json"]                                                    # save_scores: false
    doc2 = json.load(open(out2 / "events.json"))
    assert doc2["params"]["threshold"] == thr and doc2["params"]["low"] == thr and doc2["params"]["max_gap"] == 0
    assert all("class_name" not in e for v in doc2["videos"] for e in v["events"])                # no labels file
    n_events = 0
    for r, (s, _, p) in zip(res2, want):
        assert torch.equal(r["abnormal_scores"], s) and torch.equal(r["class_probs"], p)          # (the same weights: seed 31)
        y, _ = ops.eval_counts(s.contiguous(), p.contiguous(), torch.full((s.numel(),), FM.NORMAL_ID, dtype=torch.int64, device=DEV),
                               FM.NUM_CLASSES, FM.NORMAL_ID, torch.tensor([thr], dtype=torch.float32, device=DEV))
        abnormal = (y.cpu().numpy() != FM.NORMAL_ID)
        member = np.zeros(len(abnormal), dtype=bool)
        for e in r["events"]:
            assert not member[e["start"]:e["end"] + 1].any() and e["hot_frames"] == e["end"] - e["start"] + 1
            member[e["start"]:e["end"] + 1] = True
        assert np.array_equal(member, abnormal)
        # maximal runs: as many events as the prediction has rising edges
        assert len(r["events"]) == int(abnormal[0]) + int((abnormal[1:] & ~abnormal[:-1]).sum())
        n_events += len(r["events"])
    assert n_events > 0
