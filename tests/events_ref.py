"""The rules of acx_score_events (include/acx.h) restated on the host, twice: `find_events_ref` walks each video frame by frame,
`find_events_bruteforce` decides every frame's membership from the definitions alone in O(T^2).  test_cpu_events.py holds the two
against each other and against hand-made tables; test_gpu_events.py / test_gpu_predict.py hold the kernels against the walk.

Both take numpy arrays (scores f32 [n], probs f32 [n, C1], row_off int [V + 1]) and return
(count int32 [V], events int32 [V, E, 6] = start, end, class, votes, hot_frames, peak_frame, stats f64 [V, E, 2] = peak, mean)
with -1 / NaN in the unused slots, like the device tables."""
import numpy as np


def _argmax_strict(row):
    """strict > from -inf: NaN never wins, ties and an all-NaN row go to the lowest k"""
    best, am = -np.inf, 0
    for k, x in enumerate(row):
        if x > best:
            best, am = x, k
    return am


def _describe(s, p, start, end, hi, normal_idx):
    """the record of the event start .. end (inclusive) of one video: scores s, probabilities p"""
    seg = s[start:end + 1]
    ok = ~np.isnan(seg)
    if ok.any():
        peak = float(seg[ok].max())
        peak_frame = start + int(np.nonzero(ok & (seg == np.float32(peak)))[0][0])
        total = 0.0
        for x in seg[ok]:
            total += float(x)
        mean = total / int(ok.sum())
    else:
        peak, peak_frame, mean = float("nan"), start, float("nan")
    votes = np.zeros(p.shape[1], dtype=np.int64)
    hot = 0
    for t in range(start, end + 1):
        if not (s[t] < np.float32(hi)):
            hot += 1
            votes[_argmax_strict(p[t])] += 1
    k = int(np.argmax(votes))                      # first maximum: the lowest k
    return (start, end, k + 1 if k >= normal_idx else k, int(votes[k]), hot, peak_frame), (peak, mean)


def _tables(per_video, E):
    V = len(per_video)
    count = np.zeros(V, dtype=np.int32)
    events = np.full((V, E, 6), -1, dtype=np.int32)
    stats = np.full((V, E, 2), np.nan, dtype=np.float64)
    for v, lst in enumerate(per_video):
        count[v] = len(lst)
        for j, (e, st) in enumerate(lst[:E]):
            events[v, j], stats[v, j] = e, st
    return count, events, stats


def find_events_ref(scores, probs, row_off, normal_idx, hi, lo=None, max_gap=0, min_len=1, max_events=1024):
    """one sequential walk per video: warm runs -> raw events -> chains -> length filter"""
    lo = hi if lo is None else lo
    hi32, lo32 = np.float32(hi), np.float32(lo)
    out = []
    for v in range(len(row_off) - 1):
        s, p = scores[row_off[v]:row_off[v + 1]], probs[row_off[v]:row_off[v + 1]]
        T = len(s)
        raws, run_start, run_hot = [], None, False
        for t in range(T + 1):
            warm = t < T and not (s[t] < lo32)
            if warm:
                if run_start is None:
                    run_start, run_hot = t, False
                run_hot = run_hot or not (s[t] < hi32)
            elif run_start is not None:
                if run_hot:
                    raws.append((run_start, t - 1))
                run_start = None
        chains = []
        for a, b in raws:
            if chains and a - chains[-1][1] - 1 <= max_gap:
                chains[-1][1] = b
            else:
                chains.append([a, b])
        out.append([_describe(s, p, a, b, hi, normal_idx) for a, b in chains if b - a + 1 >= min_len])
    return _tables(out, max_events)


def find_events_bruteforce(scores, probs, row_off, normal_idx, hi, lo=None, max_gap=0, min_len=1, max_events=1024):
    """membership by definition.  Frame t lies in a raw event iff it is warm and some hot frame u is joined to it by warm frames only.
    Frame t lies in an event iff it lies in a raw event, or raw-event frames a < t < b exist with no raw-event frame strictly
    between them and b - a - 1 <= max_gap.  Events are the maximal runs of member frames (two chains are never adjacent: a gap
    separates them), kept when long enough."""
    lo = hi if lo is None else lo
    hi32, lo32 = np.float32(hi), np.float32(lo)
    out = []
    for v in range(len(row_off) - 1):
        s, p = scores[row_off[v]:row_off[v + 1]], probs[row_off[v]:row_off[v + 1]]
        T = len(s)
        warm = [not (x < lo32) for x in s]
        hot = [not (x < hi32) for x in s]
        cold_before = np.concatenate([[0], np.cumsum([not w for w in warm])])     # cold frames among 0 .. t - 1

        def all_warm(a, b):
            return cold_before[b + 1] == cold_before[a]
        in_raw = [warm[t] and any(hot[u] and all_warm(min(t, u), max(t, u)) for u in range(T)) for t in range(T)]
        member = list(in_raw)
        for t in range(T):
            if not member[t]:
                left = [a for a in range(t) if in_raw[a]]
                right = [b for b in range(t + 1, T) if in_raw[b]]
                if left and right and right[0] - left[-1] - 1 <= max_gap:
                    member[t] = True
        # a chain boundary between two ADJACENT member frames does not exist: adjacent raw-event frames belong to one warm run
        evs = []
        for t in range(T):
            if member[t] and (t == 0 or not member[t - 1]):
                e = t
                while e + 1 < T and member[e + 1]:
                    e += 1
                if e - t + 1 >= min_len:
                    evs.append(_describe(s, p, t, e, hi, normal_idx))
        out.append(evs)
    return _tables(out, max_events)


def assert_tables_equal(got, want, lengths=None):
    """count and events whole, peak exactly (NaN == NaN), mean within len * 2^-52 * mean of the f64 reference: the bound of any
    summation order over non-negative terms"""
    gc, ge, gs = got
    wc, we, ws = want
    assert np.array_equal(gc, wc), (gc, wc)
    assert np.array_equal(ge, we), np.argwhere(ge != we)[:8]
    assert np.array_equal(gs[..., 0], ws[..., 0], equal_nan=True)
    n = (we[..., 1] - we[..., 0] + 1).astype(np.float64)
    gm, wm = gs[..., 1], ws[..., 1]
    assert np.array_equal(np.isnan(gm), np.isnan(wm))
    ok = ~np.isnan(wm)
    assert (np.abs(gm[ok] - wm[ok]) <= n[ok] * 2.0 ** -52 * np.abs(wm[ok])).all(), np.abs(gm[ok] - wm[ok]).max()
