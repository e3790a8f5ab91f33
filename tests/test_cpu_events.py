"""No device: the rules of acx_score_events as tests/events_ref.py restates them -- hand-made cases with literal tables, the
sequential walk against the definitional O(T^2) formulation on seeded inputs -- the entry point's refusals through libacx.so with a
NULL context (no launch), the predict list reader and events.json."""
import ctypes as C
import json

import numpy as np
import pytest

import events_ref as ER

HI, LO, NORMAL = 0.5, 0.25, 2          # 0.25 is warm, 0.5 is hot: both thresholds are met with equality below
C1 = 5


def one_hot(classes):
    p = np.zeros((len(classes), C1), dtype=np.float32)
    p[np.arange(len(classes)), classes] = 1.0
    return p


def run(videos, classes=None, **kw):
    """videos: lists of scores -> both formulations (which must agree) as ([per video: list of 6-tuples], [list of (peak, mean)])"""
    s = np.asarray([x for v in videos for x in v], dtype=np.float32)
    p = one_hot(np.zeros(len(s), dtype=np.int64) if classes is None else np.asarray(classes))
    off = np.concatenate([[0], np.cumsum([len(v) for v in videos])]).astype(np.int64)
    kw.setdefault("max_events", 8)
    got = ER.find_events_ref(s, p, off, NORMAL, HI, LO, **kw)
    ER.assert_tables_equal(ER.find_events_bruteforce(s, p, off, NORMAL, HI, LO, **kw), got)
    count, events, stats = got
    E = kw["max_events"]
    assert (events[np.arange(E)[None, :] >= count[:, None]] == -1).all()
    return ([[tuple(int(x) for x in e) for e in events[v, :min(count[v], E)]] for v in range(len(videos))],
            [[tuple(float(x) for x in st) for st in stats[v, :min(count[v], E)]] for v in range(len(videos))], count)


# ====================================================================================================== hand-made tables
def test_a_run_whose_only_hot_frame_is_its_last():
    ev, st, _ = run([[0, .25, .25, .5, 0]], classes=[0, 0, 0, 2, 0])
    assert ev == [[(1, 3, 3, 1, 1, 3)]]                            # k = 2 >= normal_idx: reported as class 3
    assert st == [[(0.5, 1.0 / 3.0)]]
    assert run([[0, .25, .25, .25, 0]])[0] == [[]]                 # the same run without a hot frame is no event


def test_a_gap_of_exactly_max_gap_merges_and_one_more_does_not():
    ev, st, _ = run([[.5, 0, 0, .5, 0, 0, 0, .5]], max_gap=2)
    assert ev == [[(0, 3, 0, 2, 2, 0), (7, 7, 0, 1, 1, 7)]]
    assert st == [[(0.5, 0.25), (0.5, 0.5)]]                       # the gap's frames count in the mean
    assert run([[.5, 0, 0, .5, 0, 0, 0, .5]], max_gap=3)[0] == [[(0, 7, 0, 3, 3, 0)]]
    assert [e[:2] for e in run([[.5, 0, 0, .5, 0, 0, 0, .5]], max_gap=1)[0][0]] == [(0, 0), (3, 3), (7, 7)]


def test_an_event_of_min_len_minus_one_frames_is_dropped():
    ev, _, count = run([[.5, .5, 0, .5, .5, .5, 0]], min_len=3)
    assert ev == [[(3, 5, 0, 3, 3, 3)]] and count.tolist() == [1]
    assert [e[:2] for e in run([[.5, .5, 0, .5, .5, .5, 0]], min_len=2)[0][0]] == [(0, 1), (3, 5)]


def test_two_short_parts_pass_min_len_only_when_merged():
    ev, st, _ = run([[.5, 0, .5, 0, 0, 0, .5]], max_gap=1, min_len=3)
    assert ev == [[(0, 2, 0, 2, 2, 0)]]                            # (6, 6) stays alone and is too short
    assert st == [[(0.5, 1.0 / 3.0)]]
    assert run([[.5, 0, .5, 0, 0, 0, .5]], max_gap=0, min_len=3)[0] == [[]]


def test_nothing_merges_across_a_video_boundary():
    ev, _, count = run([[0, .5], [], [.5, 0]], max_gap=10 ** 6)
    assert ev == [[(1, 1, 0, 1, 1, 1)], [], [(0, 0, 0, 1, 1, 0)]] and count.tolist() == [1, 0, 1]


def test_vote_tie_and_peak_tie_go_to_the_lowest():
    ev, st, _ = run([[.5, .75, .75, .5]], classes=[3, 1, 3, 1])
    assert ev == [[(0, 3, 1, 2, 4, 1)]]                            # classes 1 and 3 have two votes each; 0.75 first at frame 1
    assert st == [[(0.75, 0.625)]]
    ev, _, _ = run([[.5, .75, .75, .5]], classes=[3, 4, 3, 4])
    assert ev == [[(0, 3, 4, 2, 4, 1)]]                            # k = 3 against k = 4: k = 3, reported past the normal column


def test_nan_scores_are_hot_and_stay_out_of_peak_and_mean():
    nan = float("nan")
    ev, st, _ = run([[0, nan, 0, nan, .25, 0]])
    assert ev == [[(1, 1, 0, 1, 1, 1), (3, 4, 0, 1, 1, 4)]]
    assert np.isnan(st[0][0]).all() and st[0][1] == (0.25, 0.25)


def test_truncation_keeps_the_count():
    ev, _, count = run([[.5, 0] * 6], max_events=4)
    assert count.tolist() == [6] and [e[0] for e in ev[0]] == [0, 2, 4, 6]


# ====================================================================================================== walk == definition
PARAMS = [dict(hi=0.5, lo=0.5), dict(hi=0.625, lo=0.25, max_gap=3), dict(hi=0.5, lo=0.375, max_gap=1, min_len=4),
          dict(hi=0.875, lo=-np.inf, max_gap=0, min_len=2), dict(hi=0.75, lo=0.125, max_gap=7, min_len=9)]


@pytest.mark.parametrize("seed", range(6))
def test_walk_equals_the_definition_on_seeded_inputs(seed):
    rng = np.random.default_rng(seed)
    T = [int(t) for t in rng.integers(0, 201, size=4)] + [0, 1]
    n = sum(T)
    # multiples of 1/8 in [0, 1]: equality with hi and lo occurs; long cold and warm stretches by a slow random walk
    walk = np.clip(np.cumsum(rng.integers(-1, 2, size=n)) + 3, 0, 8)
    s = (np.where(rng.random(n) < 0.7, walk, rng.integers(0, 9, size=n)) / 8.0).astype(np.float32)
    s[rng.random(n) < 0.01] = np.nan
    p = rng.integers(0, 4, size=(n, 7)).astype(np.float32)         # many ties inside a row
    off = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    for kw in PARAMS:
        a = ER.find_events_ref(s, p, off, 3, max_events=16, **kw)
        b = ER.find_events_bruteforce(s, p, off, 3, max_events=16, **kw)
        ER.assert_tables_equal(a, b)
    assert ER.find_events_ref(s, p, off, 3, 0.5)[0].sum() > 0


# ====================================================================================================== the entry point, no device
def test_workspace_bytes_and_refusals_with_a_null_context():
    from anomalyclip_amd import _lib as L
    lib = L.lib()
    ws = lib.acx_score_events_workspace_bytes
    assert ws(0, 0, 1) >= 0 and ws(1_100_000, 290, 1024) >= 0 and ws((1 << 31) - 1, 1, 1) >= 0
    assert ws(1 << 31, 1, 1) == -1 and ws(-1, 1, 1) == -1 and ws(10, -1, 1) == -1 and ws(10, 1, 0) == -1
    buf = (C.c_double * 64)()
    a = C.addressof(buf)

    def call(n=10, V=1, c1=13, normal=7, hi=0.5, lo=0.5, max_gap=0, min_len=1, E=4, wsb=1 << 20):
        rc = lib.acx_score_events(None, a, a, a, n, V, c1, normal, hi, lo, max_gap, min_len, E, a, a, a, a, wsb, None)
        return rc, lib.acx_last_error(None)
    for kw, text in ((dict(lo=0.75), b"lo > hi"), (dict(hi=float("nan")), b"lo > hi"), (dict(max_gap=-1), b"max_gap"),
                     (dict(min_len=0), b"min_len"), (dict(E=0), b"max_events"), (dict(c1=4), b"C1"), (dict(c1=64), b"C1"),
                     (dict(normal=14), b"normal_idx"), (dict(normal=-1), b"normal_idx"), (dict(n=1 << 31), b"n="),
                     (dict(n=-1), b"n="), (dict(V=-1), b"videos"), (dict(V=1 << 22, E=1 << 10), b"slots")):
        rc, msg = call(**kw)
        assert rc == -1 and text in msg and b"acx_score_events" in msg, (kw, rc, msg)
    # valid arguments get as far as the context check: nothing was launched for any of the calls above either
    rc, msg = call()
    assert rc == -1 and b"null context" in msg
    rc, msg = call(c1=5, normal=5, lo=-float("inf"), max_gap=(1 << 31) - 1, n=(1 << 31) - 1)
    assert rc == -1 and b"null context" in msg


def test_ops_wrapper_has_no_host_path():
    import torch
    from anomalyclip_amd import _lib as L, ops
    assert ops.SCORE_EVENTS_CHUNK == 1024
    with pytest.raises(L.AcxError):
        ops.score_events(torch.zeros(4), torch.zeros(4, 13), torch.tensor([0, 4]), 7, 0.5, 0.5, 0, 1, 4)


# ====================================================================================================== the predict list
def _datamodule(tmp_path, **kw):
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    for name in ("normal", "anomaly", "test"):
        (tmp_path / f"{name}.txt").write_text("a/v0 0 9 7\n")
    return AnomalyCLIPDataModule(frames_root=str(tmp_path), annotation_file_normal=str(tmp_path / "normal.txt"),
                                 annotation_file_anomaly=str(tmp_path / "anomaly.txt"), annotation_file_test=str(tmp_path / "test.txt"),
                                 normal_id=7, num_classes=14, **kw)


def test_predict_list_reader(tmp_path):
    from anomalyclip_amd.datamodule import StreamedTestLoader, VideoRecord, read_predict_file
    f = tmp_path / "predict.txt"
    f.write_text("cam/a 0 99\n\ncam/b 10 49 3\n")
    recs = read_predict_file(str(f), "/data", 7)
    assert [(r.video, r.path, r.start_frame, r.end_frame, r.num_frames, r.label) for r in recs] == [
        ("cam/a", "/data/cam/a.npy", 0, 99, 100, 7), ("cam/b", "/data/cam/b.npy", 10, 49, 40, 7)]     # the label column is ignored
    f.write_text("cam/a 0 99\ncam/b 10\n")
    with pytest.raises(ValueError, match=r"predict\.txt:2.*cam/b 10"):
        read_predict_file(str(f), "/data", 7)
    f.write_text("cam/a 0 99 3 4\n")
    with pytest.raises(ValueError, match=r"predict\.txt:1"):
        read_predict_file(str(f), "/data", 7)
    with pytest.raises(ValueError):                               # the other lists keep their four columns
        VideoRecord(["cam/a", "0", "99"], "/data", "x:1")
    f.write_text("cam/a 0 99\ncam/b 10 49 3\n")
    dm = _datamodule(tmp_path, annotation_file_predict=str(f))
    loader = dm.predict_dataloader()
    assert isinstance(loader, StreamedTestLoader) and len(loader) == 2 and loader.annotations is None
    assert loader.frame_labels(1, 40).tolist() == [7] * 40


def test_predict_dataloader_without_the_key_is_refused(tmp_path):
    dm = _datamodule(tmp_path)
    assert dm.hparams.annotation_file_predict is None
    with pytest.raises(ValueError, match="annotation_file_predict"):
        dm.predict_dataloader()


# ====================================================================================================== events.json
def test_write_events_round_trips(tmp_path):
    from anomalyclip_amd import events as EV
    a = EV.EventList([{"start": 3, "end": 9, "class": 8, "votes": 4, "hot_frames": 5, "peak_frame": 6, "peak": 0.75, "mean": 0.5}])
    a.total, a.truncated = 3, True
    b = EV.EventList()
    nanev = [{"start": 0, "end": 0, "class": 0, "votes": 1, "hot_frames": 1, "peak_frame": 0, "peak": float("nan"), "mean": float("nan")}]
    params = {"threshold": 0.5, "low": 0.25, "max_gap": 2, "min_len": 1, "max_events": 1, "save_scores": True, "normal_idx": 7}
    names = [f"Kind{i}" for i in range(14)]
    path = tmp_path / "sub" / "events.json"
    doc = EV.write_events(path, ["x/v0", "x/v1", "x/v2"], [a, b, nanev], params, names)
    text = path.read_text()
    back = json.loads(text)
    assert back == doc and text == json.dumps(doc, indent=4, sort_keys=True)
    assert back["params"] == params
    assert [v["video"] for v in back["videos"]] == ["x/v0", "x/v1", "x/v2"]
    v0 = back["videos"][0]
    assert v0["count"] == 3 and v0["truncated"] is True and v0["events"] == [{**a[0], "class_name": "Kind8"}]
    assert back["videos"][1] == {"video": "x/v1", "count": 0, "truncated": False, "events": []}
    assert back["videos"][2]["events"][0]["peak"] is None and back["videos"][2]["count"] == 1      # json has no NaN
    plain = EV.write_events(tmp_path / "plain.json", ["x/v0"], [a], params)
    assert "class_name" not in plain["videos"][0]["events"][0]
    with pytest.raises(ValueError):
        EV.write_events(tmp_path / "bad.json", ["x/v0"], [a, b], params)
