"""The rules of acx_curve_decimate (include/acx.h) restated on the host with Python integers: the yardstick of tests/test_gpu_figures.py,
itself checked against a loop over the points in tests/test_cpu_figures.py.

A classification curve's k points (tps_j, fps_j -- cumulative counts, so neither decreases with j -- and P = n_pos, N = n_neg) are
reduced to a figure's W pixel columns.  Column of point j, by integer division:

    mode 0 (ROC)   x = fps_j / N   column = min(W - 1, fps_j * W // N);  N == 0: column 0
    mode 1 (PR)    x = tps_j / P   column = min(W - 1, tps_j * W // P);  P == 0: no point at all (recall is NaN)

Height of point j: mode 0 tps_j; mode 1 the precision tps_j / (tps_j + fps_j), two of them compared by cross-multiplication
(tps_j + fps_j >= 1 on every curve: it is the number of samples down to the threshold).  Per column four records
(index, tps, fps): the run's first point, last point, lowest point, highest point, ties in the height to the lowest index; an empty
column holds (-1, -1, -1) four times."""
import numpy as np

ROC, PR = 0, 1
EMPTY = -1


def columns_of(tps, fps, P: int, N: int, mode: int, W: int):
    """the column of every point, Python integers; None where the curve has no points (PR without positives)"""
    if mode == PR and P <= 0:
        return None
    x, den = (fps, N) if mode == ROC else (tps, P)
    if den <= 0:
        return [0] * len(x)
    return [min(W - 1, int(v) * W // den) for v in x]


def less(mode: int, ta: int, fa: int, tb: int, fb: int) -> bool:
    """height of (ta, fa) < height of (tb, fb)"""
    if mode == ROC:
        return ta < tb
    return ta * (tb + fb) < tb * (ta + fa)


def decimate(tps, fps, k: int, P: int, N: int, mode: int, W: int) -> np.ndarray:
    """int64 [W, 4, 3]; only the first k entries of tps / fps are read.  Walks the runs of equal column (the columns never
    decrease) and scans each run once for its lowest and highest point."""
    out = np.full((W, 4, 3), EMPTY, dtype=np.int64)
    t = [int(v) for v in np.asarray(tps).reshape(-1)[:k]]
    f = [int(v) for v in np.asarray(fps).reshape(-1)[:k]]
    cols = columns_of(t, f, int(P), int(N), mode, W)
    if not cols:
        return out
    c = np.asarray(cols, dtype=np.int64)
    assert (np.diff(c) >= 0).all(), "cumulative counts do not decrease"
    starts = [0] + (np.flatnonzero(np.diff(c)) + 1).tolist() + [len(cols)]
    for lo, hi in zip(starts[:-1], starts[1:]):
        mn = mx = lo
        for j in range(lo + 1, hi):
            if less(mode, t[j], f[j], t[mn], f[mn]):
                mn = j
            if less(mode, t[mx], f[mx], t[j], f[j]):
                mx = j
        out[cols[lo]] = [(j, t[j], f[j]) for j in (lo, hi - 1, mn, mx)]
    return out


def points(table, mode: int, P: int, N: int):
    """a table -> the polyline (x, y), float64, as metrics.evaluate(figure_columns=W) returns it: every recorded index once, in
    index order, after (0, 0) (ROC: fpr, tpr) or after recall 0 / precision 1 (PR: recall, precision)"""
    seen = {}
    for idx, t, f in np.asarray(table).reshape(-1, 3).tolist():
        if idx >= 0:
            seen[idx] = (t, f)
    xs, ys = ([0.0], [0.0]) if mode == ROC else ([0.0], [1.0])
    for idx in sorted(seen):
        t, f = seen[idx]
        if mode == ROC:
            xs.append(f / N if N else 0.0)
            ys.append(t / P if P else 0.0)
        else:
            xs.append(t / P)
            ys.append(t / (t + f))
    return np.array(xs, dtype=np.float64), np.array(ys, dtype=np.float64)


def random_curve(rng, k: int, p_step: float = 0.3, max_step: int = 3):
    """a seeded curve of k points: every point adds at least one sample -> (tps, fps int32 [k], P, N)"""
    dt = (rng.random(k) < p_step) * rng.integers(1, max_step + 1, k)
    df = rng.integers(0, max_step + 1, k)
    df[(dt + df) == 0] = 1
    tps, fps = np.cumsum(dt), np.cumsum(df)
    return tps.astype(np.int32), fps.astype(np.int32), int(tps[-1]) if k else 0, int(fps[-1]) if k else 0
