"""CPU-only checks of packed extraction (anomalyclip_amd/extract.py: plan_launches, encode_videos' host pieces, FeatureWriter, the
`--pack` switch): the launch plan's invariants, the readers' borrowed pool and caller-owned slots, and the background writer's
behaviour when a write fails.  No kernel is launched here."""
import inspect
import os
import threading
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest
import torch
from PIL import Image

from anomalyclip_amd import extract as X

#        lengths, chunk, ncrops, launches, frames in the last launch
CASES = [([1, 7, 16, 23, 40], 16, 1, 6, 7),
         ([1, 7, 16, 23, 40], 16, 5, 29, 3),
         ([0, 5, 0], 8, 1, 1, 5),
         ([600], 512, 10, 12, 39)]


def _frames(launch):
    return sum(i1 - i0 for _, i0, i1 in launch)


@pytest.mark.parametrize("lengths,chunk,ncrops,nlaunch,last", CASES)
def test_plan_launches_invariants(lengths, chunk, ncrops, nlaunch, last):
    plan = X.plan_launches(lengths, ncrops, chunk)
    nb = max(1, chunk // ncrops)
    assert nb == X.batch_frames(types.SimpleNamespace(chunk=chunk), ncrops)
    assert len(plan) == nlaunch and _frames(plan[-1]) == last
    # coverage, exactly once, and order: the pieces read one after the other walk every video from frame 0 to its end
    pieces = [p for launch in plan for p in launch]
    assert all(isinstance(p, tuple) and len(p) == 3 and p[1] < p[2] for p in pieces)
    assert pieces == sorted(pieces)
    seen = {v: 0 for v, T in enumerate(lengths) if T}
    for v, i0, i1 in pieces:
        assert i0 == seen[v] and i1 <= lengths[v]
        seen[v] = i1
    assert seen == {v: T for v, T in enumerate(lengths) if T}
    # size: no launch over the limit, every launch but the last exactly full
    assert all(_frames(launch) == nb for launch in plan[:-1]) and 0 < _frames(plan[-1]) <= nb
    # within a launch a video is one piece
    assert all(len({v for v, _, _ in launch}) == len(launch) for launch in plan)


def test_plan_details_of_the_table_cases():
    """The invariants leave one plan only.  In the first case the videos hold frames 0, 1-7, 8-23, 24-46 and 47-86 of the run and
    the launches cut at every 16th: video 3 lies in launches 1 and 2 (two, not the three the feature request's table says),
    video 4 in launches 2 to 5."""
    plan = X.plan_launches([1, 7, 16, 23, 40], 1, 16)
    assert [i for i, launch in enumerate(plan) if any(v == 3 for v, _, _ in launch)] == [1, 2]
    assert [i for i, launch in enumerate(plan) if any(v == 4 for v, _, _ in launch)] == [2, 3, 4, 5]
    assert plan[2] == [(3, 8, 23), (4, 0, 1)]
    assert plan[0] == [(0, 0, 1), (1, 0, 7), (2, 0, 8)]
    assert X.plan_launches([0, 5, 0], 1, 8) == [[(1, 0, 5)]]
    assert X.plan_launches([], 1, 8) == [] and X.plan_launches([0, 0], 5, 8) == []
    assert X.plan_launches([3], 10, 4) == [[(0, 0, 1)], [(0, 1, 2)], [(0, 2, 3)]]       # chunk < ncrops: one frame per launch


@pytest.mark.parametrize("T,chunk,ncrops", [(600, 512, 10), (40, 16, 5), (16, 16, 1), (1, 16, 5), (33, 16, 1)])
def test_one_video_plan_is_encode_videos_batches(T, chunk, ncrops):
    """FrameFolderReader.batches(n)'s spans, at n = batch_frames: what encode_video launches"""
    n = X.batch_frames(types.SimpleNamespace(chunk=chunk), ncrops)
    spans = [(i, min(T, i + n)) for i in range(0, T, n)]
    assert X.plan_launches([T], ncrops, chunk) == [[(0, i0, i1)] for i0, i1 in spans]


def test_launches_are_made_as_the_lengths_arrive():
    """a full launch is out before the length of the video behind it is asked for (its reader need not be open yet)"""
    asked = []

    def lengths():
        for v, T in enumerate([4, 4, 3]):
            asked.append(v)
            yield T

    it = X._iter_launches(lengths(), 4)
    assert next(it) == [(0, 0, 4)] and asked == [0]
    assert next(it) == [(1, 0, 4)] and asked == [0, 1]
    assert list(it) == [[(2, 0, 3)]]


def test_pack_switches_default_off(tmp_path):
    sig = inspect.signature(X.extract_dataset)
    assert sig.parameters["pack"].default is False and sig.parameters["max_inflight"].default == 4
    assert inspect.signature(X.encode_videos).parameters["lookahead"].default == 2
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    from anomalyclip_amd.feature_bank import FeatureBank
    assert inspect.signature(FeatureBank.from_frames).parameters["pack"].default is False
    assert inspect.signature(AnomalyCLIPDataModule.__init__).parameters["pack"].default is False
    w = tmp_path / "w.pt"
    w.write_bytes(b"")
    base = ["--arch", "tiny", "--weights", str(w), "--frames-root", str(tmp_path), "--out-root", str(tmp_path / "o")]
    assert X.parse_args(base).pack is False
    assert X.parse_args(base + ["--pack"]).pack is True


def _folder(folder, T, hw, seed=0):
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    for t in range(T):
        Image.fromarray(rng.integers(0, 256, (*hw, 3), dtype=np.uint8)).save(os.path.join(folder, f"{t:06d}.png"))


def test_readers_share_a_borrowed_pool_and_decode_into_the_callers_slot(tmp_path):
    root = str(tmp_path)
    _folder(os.path.join(root, "a"), 5, (6, 8), 1)
    _folder(os.path.join(root, "b"), 3, (4, 10), 2)
    start = threading.active_count()
    with ThreadPoolExecutor(max_workers=2) as pool:
        ra = X.FrameFolderReader(root, "a", template="{:06d}.png", pinned=False)
        rb = X.FrameFolderReader(root, "b", template="{:06d}.png", pinned=False)
        ra.borrow(pool)
        rb.borrow(pool)
        slot = np.zeros(3 * 6 * 8 * 3 + 2 * 4 * 10 * 3 + 7, dtype=np.uint8)           # one launch's slot: two pieces, two sizes
        da = slot[:432].reshape(3, 6, 8, 3)
        db = slot[432:672].reshape(2, 4, 10, 3)
        for f in ra.decode_into(2, 5, da) + rb.decode_into(0, 2, db):
            f.result()
        ra.close()
        rb.close()
        assert pool.submit(lambda: 7).result() == 7                                # a borrowed pool outlives its readers
        for r, dst, i0 in ((ra, da, 2), (rb, db, 0)):
            for j in range(dst.shape[0]):
                assert np.array_equal(dst[j], np.asarray(Image.open(r.path(i0 + j)).convert("RGB")))
        assert not slot[672:].any()
    assert threading.active_count() == start
    own = X.FrameFolderReader(root, "a", template="{:06d}.png", pinned=False)      # its own pool: unchanged behaviour
    view = own.decode_batch(0, 5, 0)
    assert view.shape == (5, 6, 8, 3) and threading.active_count() > start
    own.close()
    assert threading.active_count() == start


class _Event:
    def __init__(self):
        self.waited = False

    def synchronize(self):
        self.waited = True


def test_writer_writes_behind_and_bounds_the_buffers_alive(tmp_path):
    start = threading.active_count()
    gate = threading.Event()
    gate.synchronize = gate.wait                    # the first file's "rows" arrive only when the test says so
    w = X.FeatureWriter(max_inflight=2)
    rows = [np.full((3, 4), i, np.float32) for i in range(3)]
    w.acquire()
    w.submit(gate, rows[0], str(tmp_path / "v0"))
    w.acquire()
    ev = _Event()
    w.submit(ev, torch.from_numpy(rows[1]), str(tmp_path / "v1.npy"))
    assert not w._places.acquire(blocking=False)    # two buffers alive and the first write held up: a third would have to wait
    assert not os.path.exists(tmp_path / "v0.npy")
    gate.set()
    w.acquire()                                     # ... until the writer is through with the first
    w.submit(None, rows[2], str(tmp_path / "v2"))
    w.close()
    assert ev.waited and threading.active_count() == start
    for i in range(3):
        assert np.array_equal(np.load(tmp_path / f"v{i}.npy"), rows[i])
    assert not [f for f in os.listdir(tmp_path) if f.endswith(".tmp")]


@pytest.mark.parametrize("fail_after_tmp", [False, True])
def test_writer_failure_on_the_third_video(tmp_path, monkeypatch, fail_after_tmp):
    """the third write fails (before, or after, its .npy.tmp exists): the first two files are there and complete, no .tmp is
    left, the videos behind the failure are not written, the exception reaches the caller, no thread outlives close()"""
    start = threading.active_count()
    real, calls = X.write_features, []

    def failing(out_path, rows):
        calls.append(out_path)
        if len(calls) == 3:
            if fail_after_tmp:
                with open(X.feature_path(out_path) + ".tmp", "wb") as fh:
                    fh.write(b"half a file")
            raise OSError(28, "No space left on device")
        return real(out_path, rows)

    monkeypatch.setattr(X, "write_features", failing)
    done = []
    w = X.FeatureWriter(max_inflight=2, done=done.append)
    rows = [np.random.default_rng(i).standard_normal((5 + i, 8)).astype(np.float32) for i in range(5)]
    raised = None
    for i in range(5):
        try:
            w.acquire()                             # never blocks for good: the writer gives places back after the failure too
        except OSError as e:
            raised = e
            break
        w.submit(_Event(), rows[i], str(tmp_path / f"v{i}"), tag=i)
    with pytest.raises(OSError, match="No space left"):
        w.close()
    assert raised is None or "No space left" in str(raised)
    assert done == [0, 1] and len(calls) == 3
    for i in (0, 1):
        assert X.is_complete(str(tmp_path / f"v{i}"), rows[i].shape) and np.array_equal(np.load(tmp_path / f"v{i}.npy"), rows[i])
    assert sorted(os.listdir(tmp_path)) == ["v0.npy", "v1.npy"]
    assert threading.active_count() == start
    w.close(check=False)                            # closing twice is harmless
