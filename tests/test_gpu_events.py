"""-m gpu: acx_score_events (events.find_events, ops.score_events) against its restatement tests/events_ref.py (held against a second
formulation and hand-made tables in test_cpu_events.py): count and events as whole buffers, the -1 slots included, peak exactly,
mean within len * 2^-52 * mean of the f64 reference (the bound of any summation order over non-negative terms).  Every pattern
runs on videos of 0, 1, 2, 63, 64, 65, B - 1, B, B + 1 and 2 B + 3 frames, B = ops.SCORE_EVENTS_CHUNK, laid end to end in one call:
the empty video sits between two others, and every video's last frame meets the next one's first."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from anomalyclip_amd import _lib as L
from anomalyclip_amd import events as EV
from anomalyclip_amd import ops

import events_ref as ER

DEV = torch.device("cuda", 0)
B = ops.SCORE_EVENTS_CHUNK
LENGTHS = [1, 0, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 3]
FULL = 2 * B + 3
C1, NORMAL = 13, 7
HI, LO = 0.5, 0.25
NAN = float("nan")


def canvas(fill=0.0):
    return np.full(FULL, fill, dtype=np.float32)


def put(c, a, b, v):
    c[a:b] = v
    return c


def _alternate():
    c = canvas()
    c[::2] = 0.75
    return c


def _thresholds():
    c = canvas()
    vals = np.array([LO - 0.125, LO, HI - 0.125, HI, 0.0, LO, LO, 0.0, HI, HI], dtype=np.float32)
    c[:] = vals[(np.arange(FULL) // 3) % len(vals)]
    return c


def _chain():
    c = canvas()
    for a in range(46, FULL, 50):                     # 46 .. 50, 96 .. 100, ..., 2 B - 2 .. 2 B + 2: gaps of 45 frames
        c[a:a + 5] = 0.625
    return c


def _rand_scores():
    rng = np.random.default_rng(77)
    walk = np.clip(np.cumsum(rng.integers(-1, 2, size=FULL)) + 3, 0, 8)
    return (np.where(rng.random(FULL) < 0.7, walk, rng.integers(0, 9, size=FULL)) / 8.0).astype(np.float32)


def _votes(ka, kb):
    """one-hot rows: the run at 0 .. 3 and the run that straddles frame B vote ka, kb, ka, kb"""
    p = np.zeros((FULL, C1), dtype=np.float32)
    for a in (0, B - 2):
        for i in range(4):
            p[a + i, ka if i % 2 == 0 else kb] = 1.0
    return p


# name -> (scores on the 2 B + 3 canvas (None: hot on each video's first three and last three frames), probs on the canvas (None: seeded), parameters)
G = 8
PATTERNS = {
    "all_cold": (canvas(), None, {}),
    "all_hot": (canvas(0.75), None, {}),
    "alternating_E4": (_alternate(), None, dict(max_events=4)),
    "alternating": (_alternate(), None, {}),
    "warm_without_hot": (put(canvas(), 10, B + 50, LO), None, {}),
    "hot_only_in_pass_1": (put(put(canvas(), B - 100, B + 100, LO), B + 50, B + 51, 0.75), None, {}),
    "hot_only_in_pass_0": (put(put(canvas(), B - 100, B + 100, LO), B - 50, B - 49, 0.75), None, {}),
    "gap_exactly_max_gap_over_B": (put(put(canvas(), B - 10, B - 4, 0.75), B + 4, B + 9, 0.75), None, dict(max_gap=G)),
    "gap_max_gap_plus_1_over_B": (put(put(canvas(), B - 10, B - 4, 0.75), B + 5, B + 9, 0.75), None, dict(max_gap=G)),
    "chain_across_three_passes": (_chain(), None, dict(max_gap=45)),
    "chain_broken_by_one_frame": (_chain(), None, dict(max_gap=44)),
    "video_boundary_large_gap": (None, None, dict(max_gap=10 ** 6)),
    "video_boundary_min_len": (None, None, dict(max_gap=10 ** 6, min_len=4)),
    "lo_minus_inf": (_rand_scores(), None, dict(lo=-np.inf, hi=0.875)),
    "equal_to_hi_and_lo": (_thresholds(), None, {}),
    "nan_in_a_cold_stretch": (put(put(canvas(), 1, 2, NAN), B, B + 1, NAN), None, {}),
    "all_nan_event": (put(put(put(canvas(), 0, 2, NAN), B - 3, B + 2, NAN), 40, 44, 0.625), None, dict(max_gap=2)),
    "vote_tie_2_and_5": (put(put(canvas(), 0, 4, 0.75), B - 2, B + 2, 0.75), _votes(5, 2), {}),
    "winner_past_the_normal_column": (put(put(canvas(), 0, 4, 0.75), B - 2, B + 2, 0.75), _votes(9, 9), {}),
    "random_hysteresis": (_rand_scores(), None, dict(hi=0.625, lo=0.25, max_gap=3, min_len=2)),
}


def build(name):
    sc, pr, kw = PATTERNS[name]
    if pr is None:
        pr = (np.random.default_rng(5).integers(0, 5, size=(FULL, C1)) / 4.0).astype(np.float32)       # many ties inside a row
    s, p = [], []
    for T in LENGTHS:
        if sc is None:
            v = np.zeros(T, dtype=np.float32)
            v[:3] = 0.75
            v[max(T - 3, 0):] = 0.75
        else:
            v = sc[:T]
        s.append(v)
        p.append(pr[:T])
    off = np.concatenate([[0], np.cumsum(LENGTHS)]).astype(np.int64)
    kw = {"hi": HI, "lo": LO, "max_gap": 0, "min_len": 1, "max_events": 1024, **kw}
    return np.concatenate(s), np.concatenate(p), off, kw


_REF = {}


def reference(name):
    if name not in _REF:
        s, p, off, kw = build(name)
        _REF[name] = ER.find_events_ref(s, p, off, NORMAL, **kw)
    return _REF[name]


def device(s, p, off):
    return torch.from_numpy(s).to(DEV), torch.from_numpy(p).to(DEV), torch.from_numpy(off).to(DEV)


def raw(s, p, off, kw, normal=NORMAL):
    c, e, st = ops.score_events(*device(s, p, off), normal, kw["hi"], kw["lo"], kw["max_gap"], kw["min_len"], kw["max_events"])
    return c.cpu().numpy(), e.cpu().numpy(), st.cpu().numpy()


def tables(found, E):
    """find_events' lists back as the device tables"""
    V = len(found)
    count = np.array([f.total for f in found], dtype=np.int32)
    events = np.full((V, E, 6), -1, dtype=np.int32)
    stats = np.full((V, E, 2), np.nan, dtype=np.float64)
    for v, lst in enumerate(found):
        assert lst.truncated == (lst.total > E) and len(lst) == min(lst.total, E)
        for j, d in enumerate(lst):
            events[v, j] = [d[f] for f in EV.EVENT_FIELDS]
            stats[v, j] = [d[f] for f in EV.STAT_FIELDS]
    return count, events, stats


@pytest.mark.parametrize("name", list(PATTERNS))
def test_events_equal_the_restatement(name):
    s, p, off, kw = build(name)
    want = reference(name)
    ER.assert_tables_equal(raw(s, p, off, kw), want)
    found = EV.find_events(*device(s, p, off), NORMAL, **kw)
    ER.assert_tables_equal(tables(found, kw["max_events"]), want)


def test_the_patterns_show_what_they_are_meant_to():
    """the reference's own tables: each pattern does produce the situation it is named after"""
    big = len(LENGTHS) - 1                                                          # the video of 2 B + 3 frames
    ev = lambda name, v=big: [tuple(e[:2]) for e in reference(name)[1][v] if e[0] >= 0]
    cnt = lambda name: reference(name)[0].tolist()
    assert cnt("all_cold") == [0] * 10 and cnt("all_hot") == [1, 0] + [1] * 8 and ev("all_hot") == [(0, FULL - 1)]
    assert cnt("alternating_E4")[big] == B + 2 and len(ev("alternating_E4")) == 4 and cnt("alternating")[big] > 1024
    assert cnt("warm_without_hot") == [0] * 10
    assert ev("hot_only_in_pass_1") == ev("hot_only_in_pass_0") == [(B - 100, B + 99)]
    assert ev("hot_only_in_pass_1", 7) == [] and ev("hot_only_in_pass_0", 7) == [(B - 100, B - 1)]      # the video of B frames
    assert ev("gap_exactly_max_gap_over_B") == [(B - 10, B + 8)] and ev("gap_max_gap_plus_1_over_B") == [(B - 10, B - 5), (B + 5, B + 8)]
    assert len(ev("chain_across_three_passes")) == 1 and ev("chain_across_three_passes")[0][1] > 2 * B
    assert len(ev("chain_broken_by_one_frame")) > 30
    assert ev("video_boundary_large_gap") == [(0, FULL - 1)] and ev("video_boundary_large_gap", 0) == [(0, 0)]
    assert ev("video_boundary_min_len", 0) == [] and ev("video_boundary_min_len", 2) == []
    assert ev("lo_minus_inf") == [(0, FULL - 1)]
    assert cnt("nan_in_a_cold_stretch")[big] == 2 and np.isnan(reference("nan_in_a_cold_stretch")[2][big, 0]).all()
    assert ev("all_nan_event") == [(0, 1), (40, 43), (B - 3, B + 1)] and np.isnan(reference("all_nan_event")[2][big, 2]).all()
    tie = reference("vote_tie_2_and_5")[1][big]
    assert tie[:2, 2:4].tolist() == [[2, 2], [2, 2]]
    assert reference("winner_past_the_normal_column")[1][big][:2, 2:4].tolist() == [[10, 4], [10, 4]]


PARAM_SETS = [dict(hi=0.5, lo=0.5, max_gap=0, min_len=1, max_events=1024), dict(hi=0.625, lo=0.25, max_gap=3, min_len=1, max_events=64),
              dict(hi=0.5, lo=0.375, max_gap=1, min_len=4, max_events=1024), dict(hi=0.75, lo=0.125, max_gap=40, min_len=9, max_events=7)]


def random_batch():
    rng = np.random.default_rng(2024)
    T = [int(t) for t in rng.choice(LENGTHS, size=7)]
    n = sum(T)
    walk = np.clip(np.cumsum(rng.integers(-1, 2, size=n)) + 3, 0, 8)
    s = (np.where(rng.random(n) < 0.8, walk, rng.integers(0, 9, size=n)) / 8.0).astype(np.float32)
    p = (rng.integers(0, 5, size=(n, C1)) / 4.0).astype(np.float32)
    return s, p, np.concatenate([[0], np.cumsum(T)]).astype(np.int64)


@pytest.mark.parametrize("k", range(len(PARAM_SETS)))
def test_seeded_random_batch(k):
    s, p, off = random_batch()
    kw = PARAM_SETS[k]
    want = ER.find_events_ref(s, p, off, NORMAL, **kw)
    assert want[0].sum() > 0
    ER.assert_tables_equal(raw(s, p, off, kw), want)


def test_two_calls_give_identical_bytes():
    s, p, off = random_batch()
    kw = PARAM_SETS[1]
    a, b = raw(s, p, off, kw), raw(s, p, off, kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_non_monotone_offsets_are_reported_per_video():
    s, p, off = random_batch()
    kw = PARAM_SETS[0]
    want = ER.find_events_ref(s, p, off, NORMAL, **kw)
    bad = off.copy()
    bad[3] = bad[2] - 1                                         # video 2 ends before it starts; video 3 then starts before video 2
    got = raw(s, p, bad, kw)
    assert got[0][2] == -1 and (got[1][2] == -1).all() and np.isnan(got[2][2]).all()
    for v in (0, 1, 4, 5, 6):                                   # the videos whose own range is sound are found as before
        assert got[0][v] == want[0][v] and np.array_equal(got[1][v], want[1][v])
    past = off.copy()
    past[-1] += 1                                               # the last video would read one row past the arrays
    assert raw(s, p, past, kw)[0][6] == -1
    with pytest.raises(ValueError, match="video 2"):
        EV.find_events(*device(s, p, bad), NORMAL, 0.5)


def test_no_video_and_no_frame():
    s, p = np.zeros(0, np.float32), np.zeros((0, C1), np.float32)
    assert EV.find_events(*device(s, p, np.zeros(1, np.int64)), NORMAL, 0.5) == []
    found = EV.find_events(*device(s, p, np.zeros(4, np.int64)), NORMAL, 0.5)
    assert [list(f) for f in found] == [[], [], []] and not any(f.truncated for f in found)
    with pytest.raises(L.AcxError, match="lo > hi"):
        EV.find_events(*device(s, p, np.zeros(2, np.int64)), NORMAL, 0.5, lo=0.75)
    with pytest.raises(L.AcxError, match="C1"):
        ops.score_events(torch.zeros(3, device=DEV), torch.zeros(3, 4, device=DEV), torch.tensor([0, 3], device=DEV), 2, 0.5, 0.5, 0, 1, 4)


def test_rows_past_2_31_floats_of_probs():
    """n * C1 > 2^31: a video of 40 frames lies, as a whole, past float 2^31 of probs (8.6 GB, never filled but for those rows) behind
    one cold video of all the rows before it, which is walked in 161 thousand passes.  Offsets must be 64-bit."""
    T = 40
    n = (1 << 31) // C1 + 1 + T
    assert (n - T) * C1 >= 1 << 31
    rng = np.random.default_rng(3)
    s_tail = (rng.integers(0, 9, size=T) / 8.0).astype(np.float32)
    p_tail = (rng.integers(0, 5, size=(T, C1)) / 4.0).astype(np.float32)
    scores = torch.zeros(n, dtype=torch.float32, device=DEV)
    probs = torch.empty(n, C1, dtype=torch.float32, device=DEV)
    scores[n - T:].copy_(torch.from_numpy(s_tail))
    probs[n - T:].copy_(torch.from_numpy(p_tail))
    kw = dict(hi=0.5, lo=0.25, max_gap=1, min_len=1, max_events=8)
    c, e, st = ops.score_events(scores, probs, torch.tensor([0, n - T, n], device=DEV), NORMAL, 0.5, 0.25, 1, 1, 8)
    want = ER.find_events_ref(s_tail, p_tail, np.array([0, 0, T]), NORMAL, **kw)
    assert want[0][1] > 0
    ER.assert_tables_equal((c.cpu().numpy(), e.cpu().numpy(), st.cpu().numpy()), want)
    del scores, probs
    torch.cuda.empty_cache()
