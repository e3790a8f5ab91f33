"""No device: the restatement of acx_curve_decimate's rules (tests/curve_decimate_ref.py) against a loop over the points, and the
four evaluation figures of anomalyclip_amd/figures.py drawn from host values."""
import math
import os
from fractions import Fraction

import numpy as np
import pytest
from PIL import Image

from anomalyclip_amd import figures as F

import curve_decimate_ref as DR


# ====================================================================================================== the restatement
def brute(tps, fps, k, P, N, mode, W):
    """per column the list of its points, collected point by point; heights as exact fractions"""
    out = np.full((W, 4, 3), -1, dtype=np.int64)
    if mode == DR.PR and P <= 0:
        return out
    members = {}
    for j in range(k):
        t, f = int(tps[j]), int(fps[j])
        if mode == DR.ROC:
            c = 0 if N <= 0 else min(W - 1, (f * W) // N)
            y = Fraction(t)
        else:
            c = min(W - 1, (t * W) // P)
            y = Fraction(t, t + f)
        members.setdefault(c, []).append((y, j, t, f))
    for c, pts in members.items():
        first, last = min(pts, key=lambda p: p[1]), max(pts, key=lambda p: p[1])
        low = min(pts, key=lambda p: (p[0], p[1]))
        high = min(pts, key=lambda p: (-p[0], p[1]))
        out[c] = [p[1:] for p in (first, last, low, high)]
    return out


@pytest.mark.parametrize("W", [1, 8, 64])
@pytest.mark.parametrize("k", [0, 1, 2, 5, 300])
def test_restatement_equals_a_loop_over_the_points(k, W):
    rng = np.random.default_rng(1000 * k + W)
    tps, fps, P, N = DR.random_curve(rng, k)
    if k and P == 0:
        tps, P = tps + 1, 1 + int(tps[-1])
    for mode in (DR.ROC, DR.PR):
        got = DR.decimate(tps, fps, k, P, N, mode, W)
        assert np.array_equal(got, brute(tps, fps, k, P, N, mode, W)), (k, W, mode)
        assert got.shape == (W, 4, 3)
        if k == 0:
            assert (got == -1).all()


def test_restatement_without_positives_without_negatives_and_at_int32_max():
    rng = np.random.default_rng(7)
    tps, fps, P, N = DR.random_curve(rng, 200)
    zero = np.zeros_like(tps)
    idx = np.arange(1, 201, dtype=np.int32)
    for W in (1, 8, 64):
        # P == 0: the ROC's heights all tie (every record of a column but the last is its first index), the PR curve is empty
        roc = DR.decimate(zero, idx, 200, 0, 200, DR.ROC, W)
        assert np.array_equal(roc, brute(zero, idx, 200, 0, 200, DR.ROC, W))
        filled = roc[roc[:, 0, 0] >= 0]
        assert (filled[:, 2, 0] == filled[:, 0, 0]).all() and (filled[:, 3, 0] == filled[:, 0, 0]).all()
        assert (DR.decimate(zero, idx, 200, 0, 200, DR.PR, W) == -1).all()
        # N == 0: every point of the ROC falls into column 0
        roc = DR.decimate(idx, zero, 200, 200, 0, DR.ROC, W)
        assert np.array_equal(roc, brute(idx, zero, 200, 200, 0, DR.ROC, W))
        assert (roc[1:] == -1).all() and roc[0, 0, 0] == 0 and roc[0, 1, 0] == 199
        # counts of 2^31 - 1: the products pass 2^62
        big = 2 ** 31 - 1
        t = np.array([big - 2, big - 1, big - 1, big], dtype=np.int32)
        f = np.array([big - 3, big - 3, big, big], dtype=np.int32)
        for mode in (DR.ROC, DR.PR):
            assert np.array_equal(DR.decimate(t, f, 4, big, big, mode, W), brute(t, f, 4, big, big, mode, W)), (W, mode)
    # equal fractions of different terms tie: 1/2 and 2/4 -> the lower index stays
    t, f = np.array([1, 2, 3], dtype=np.int32), np.array([1, 2, 2], dtype=np.int32)
    got = DR.decimate(t, f, 3, 3, 2, DR.PR, 1)
    assert got[0].tolist() == [[0, 1, 1], [2, 3, 2], [0, 1, 1], [2, 3, 2]]


def test_points_of_a_table():
    tps, fps, P, N = DR.random_curve(np.random.default_rng(3), 50)
    for mode in (DR.ROC, DR.PR):
        x, y = DR.points(DR.decimate(tps, fps, 50, P, N, mode, 4096), mode, P, N)     # W past every count: nothing is dropped
        t, f = tps.astype(np.float64), fps.astype(np.float64)
        wx, wy = (f / N, t / P) if mode == DR.ROC else (t / P, t / (t + f))
        keep = sorted(set(DR.decimate(tps, fps, 50, P, N, mode, 4096)[:, :, 0].reshape(-1).tolist()) - {-1})
        assert np.array_equal(x[1:], wx[keep]) and np.array_equal(y[1:], wy[keep])
        assert (x[0], y[0]) == ((0.0, 0.0) if mode == DR.ROC else (0.0, 1.0))


# ====================================================================================================== the figures
def decode(path):
    img = Image.open(path)
    assert img.format == "PNG"
    return np.asarray(img.convert("RGB")).astype(np.int32)


def colour_mask(a, rgb):
    return (a[:, :, 0] == rgb[0]) & (a[:, :, 1] == rgb[1]) & (a[:, :, 2] == rgb[2])


def extents(path, rgb, lay):
    """per pixel column of the plot box: (top row, bottom row) of the curve-coloured pixels, or None"""
    m = colour_mask(decode(path), rgb)
    p = lay["plot"]
    out = []
    for x in range(p[0], p[2]):
        rows = np.flatnonzero(m[:, x])
        out.append((int(rows[0]), int(rows[-1])) if rows.size else None)
    return out


def host_points(tps, fps, P, N, mode, W=None):
    """the full polyline (W None) or the decimated one, as evaluate() would return them"""
    k = len(tps)
    if W is not None:
        return DR.points(DR.decimate(tps, fps, k, P, N, mode, W), mode, P, N)
    return DR.points(np.stack([np.arange(k), tps, fps], 1), mode, P, N)


@pytest.mark.parametrize("kind", ["pr", "roc"])
def test_curve_figure_from_host_points(tmp_path, kind):
    mode, write, rgb = (DR.PR, F.write_pr, F.RED) if kind == "pr" else (DR.ROC, F.write_roc, F.BLUE)
    W = 200
    # at most four points per column: 300 points, both counts grow by 1 ... 3 per point, a column is about 3 counts wide
    rng = np.random.default_rng(11)
    tps, fps = (np.cumsum(rng.integers(1, 4, 300)).astype(np.int32) for _ in range(2))
    P, N = int(tps[-1]), int(fps[-1])
    per_column = np.bincount(DR.columns_of(tps.tolist(), fps.tolist(), P, N, mode, W))
    assert 3 <= max(per_column) <= 4
    a = write(tmp_path / "a.png", host_points(tps, fps, P, N, mode, W), 0.8125, W)
    b = write(tmp_path / "b.png", host_points(tps, fps, P, N, mode, W), 0.8125, W)
    full = write(tmp_path / "full.png", host_points(tps, fps, P, N, mode), 0.8125, W)
    assert a.read_bytes() == b.read_bytes()                       # the same inputs, the same bytes
    assert a.read_bytes() == full.read_bytes()                    # the decimation keeps every point of such a curve
    assert sorted(os.listdir(tmp_path)) == ["a.png", "b.png", "full.png"]           # no temporary file stays
    img = decode(a)
    assert img.shape == (480, 640, 3)
    lay = F.layout(kind, columns=W)
    p = lay["plot"]
    assert p[2] - p[0] == W
    m = colour_mask(img, rgb)
    assert m[p[1]:p[3], p[0]:p[2]].any()
    m[p[1]:p[3], p[0]:p[2]] = False
    assert not m.any()                                            # the curve's colour nowhere outside the plot box
    # the default plot box is matplotlib's share of the figure
    assert F.layout(kind)["columns"] == F.DEFAULT_COLUMNS == 496


def dense_curves():
    """three seeded curves of 20,000 points: uniform, 95 % of the points in the first 3 of 512 columns, a step function"""
    k, W = 20000, 512
    rng = np.random.default_rng(2024)
    out = {"uniform": DR.random_curve(rng, k)}
    # crowded: 19,000 points move x by 3 columns' worth in all, the last 1,000 cover the rest
    big = 40
    dt = np.concatenate([(rng.random(19000) < 0.5).astype(np.int64), rng.integers(0, 3, 1000)])
    df = np.concatenate([np.ones(19000, dtype=np.int64), rng.integers(600 * big, 700 * big, 1000)])
    tps, fps = np.cumsum(dt), np.cumsum(df)
    N = int(fps[-1])
    assert int(fps[18999]) * W // N < 3
    out["crowded"] = (tps.astype(np.int32), fps.astype(np.int32), int(tps[-1]), N)
    # steps: long runs where only fps grows, then where only tps grows
    dt, df = np.zeros(k, dtype=np.int64), np.zeros(k, dtype=np.int64)
    for s in range(0, k, 1000):
        (dt if (s // 1000) % 2 else df)[s:s + 1000] = 1
    tps, fps = np.cumsum(dt), np.cumsum(df)
    out["steps"] = (tps.astype(np.int32), fps.astype(np.int32), int(tps[-1]), int(fps[-1]))
    return out, W


def test_dense_curves_keep_every_columns_extent(tmp_path):
    """Largest difference found between the vertical extent of the curve's pixels in a column of the decimated drawing and of the
    full drawing, over the three curves, both modes and all 512 columns: 0 pixels (the polyline is drawn with one-pixel lines,
    whose pixels depend on a segment's end points only, and both drawings have the same segments between columns).  The bound
    is that value: 0."""
    BOUND = 0
    curves, W = dense_curves()
    worst = 0
    for name, (tps, fps, P, N) in curves.items():
        for mode, write, rgb, kind in ((DR.ROC, F.write_roc, F.BLUE, "roc"), (DR.PR, F.write_pr, F.RED, "pr")):
            lay = F.layout(kind, columns=W)
            dec = host_points(tps, fps, P, N, mode, W)
            full = host_points(tps, fps, P, N, mode)
            assert len(dec[0]) <= 4 * W + 1 < len(full[0]) // 4
            e_dec = extents(write(tmp_path / "dec.png", dec, 0.5, W), rgb, lay)
            e_full = extents(write(tmp_path / "full.png", full, 0.5, W), rgb, lay)
            assert len(e_dec) == len(e_full) == W
            assert any(e is not None for e in e_full)
            for x, (a, b) in enumerate(zip(e_dec, e_full)):
                assert (a is None) == (b is None), (name, kind, x, a, b)
                if a is not None:
                    worst = max(worst, abs(a[0] - b[0]), abs(a[1] - b[1]))
    print("largest extent difference:", worst, "pixels")
    assert worst <= BOUND <= 1


def test_confusion_figure(tmp_path):
    C = 14
    rng = np.random.default_rng(5)
    m = rng.random((C, C)) * 0.3
    m[3] = 0.0                                                    # a class without frames
    m[0, 0], m[1, 1], m[2, 5] = 1.0, 0.5, 0.0
    names = [f"Class{i}" for i in range(C)]
    a = F.write_confusion(tmp_path / "confusion_matrix.png", m, names)
    b = F.write_confusion(tmp_path / "again.png", m, names)
    assert a.read_bytes() == b.read_bytes()
    img = decode(a)
    assert img.shape == (1800, 2000, 3)
    lay = F.layout("confusion", classes=C)
    g, (cw, ch) = lay["grid"], lay["cell"]
    assert g[2] <= lay["bar"][0] and lay["bar"][2] < 2000 and g[3] < 1800

    def cell(r, c):                                               # a pixel of the cell beside its annotation
        return img[g[1] + r * ch + 4, g[0] + c * cw + 4]
    lum = lambda px: 0.2126 * px[0] + 0.7152 * px[1] + 0.0722 * px[2]
    assert lum(cell(0, 0)) < lum(cell(1, 1)) < lum(cell(2, 5))
    assert tuple(cell(2, 5)) == (255, 255, 255) and tuple(cell(0, 0)) == F.blues(1.0)
    centre = lambda r, c: img[g[1] + r * ch + ch // 2 - 20:g[1] + r * ch + ch // 2 + 20, g[0] + c * cw + 10:g[0] + (c + 1) * cw - 10]
    # the all-zero row is drawn: white cells, each with its dark "0.00%"; the 100 % cell's text is white
    for c in range(C):
        assert tuple(cell(3, c)) == (255, 255, 255)
        assert (centre(3, c).sum(-1) < 3 * 128).any(), c
    assert (centre(0, 0) == 255).all(-1).any()
    # without names the class indices label the ticks; another matrix, other bytes
    c2 = F.write_confusion(tmp_path / "idx.png", m)
    assert c2.read_bytes() != a.read_bytes() and decode(c2).shape == (1800, 2000, 3)
    # the colour bar runs from dark blue (top) to white (bottom)
    bar = lay["bar"]
    assert tuple(img[bar[1], bar[0] + 2]) == F.blues(1.0) and tuple(img[bar[3] - 1, bar[0] + 2]) == (255, 255, 255)


def test_f1_figure_with_constant_scores(tmp_path):
    f1 = {(i + 1) / 10: 0.25 for i in range(10)}
    a = F.write_f1(tmp_path / "F1.png", f1)
    img = decode(a)
    assert img.shape == (480, 640, 3)
    lay = F.f1_axis(F.layout("f1"), list(f1.values()))
    lo, hi = lay["y_range"]
    assert lo < 0.25 < hi and all(math.isfinite(v) for v, _ in lay["y_ticks"]) and len(lay["y_ticks"]) >= 2
    p = lay["plot"]
    rows = np.flatnonzero(colour_mask(img, F.BLUE).any(1))
    assert rows.size and p[1] < rows[0] and rows[-1] < p[3] - 1 and rows[-1] - rows[0] < F.LINE_W     # one flat line inside the box
    # a rising series: ten points, fitted range
    g = F.write_f1(tmp_path / "F1b.png", {(i + 1) / 10: 0.1 + 0.05 * i for i in range(10)})
    assert colour_mask(decode(g), F.BLUE).any(0).sum() > 300 and g.read_bytes() != a.read_bytes()


@pytest.mark.parametrize("kind", ["pr", "roc"])
def test_nan_area_gives_an_empty_plot_box(tmp_path, kind):
    write, rgb = (F.write_pr, F.RED) if kind == "pr" else (F.write_roc, F.BLUE)
    pts = (np.array([0.0]), np.array([1.0])) if kind == "pr" else (np.array([0.0, 0.5, 1.0]), np.array([0.0, 0.0, 0.0]))
    a = write(tmp_path / "x.png", pts, float("nan"), 64)
    img = decode(a)
    assert img.shape == (480, 640, 3) and not colour_mask(img, rgb).any()
    p = F.layout(kind, columns=64)["plot"]
    box = img[p[1]:p[3], p[0]:p[2]].reshape(-1, 3)
    assert set(map(tuple, np.unique(box, axis=0).tolist())) <= {F.PANEL, F.GRID}
    titled = write(tmp_path / "y.png", pts, 0.5, 64)
    assert titled.read_bytes() != a.read_bytes()                  # (the title differs: "nan" against "50.00")


def test_layout_refusals_and_no_matplotlib():
    with pytest.raises(ValueError):
        F.layout("scatter")
    with pytest.raises(ValueError):
        F.layout("roc", columns=4096)                             # wider than the default figure
    src = open(F.__file__).read()
    assert "import matplotlib" not in src and "import seaborn" not in src
    import anomalyclip_amd.visualizer as V
    assert F._text is V._text                                     # shared with the visualiser, not copied
