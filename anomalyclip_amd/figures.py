"""The four pictures the reference's `test_epoch_end` leaves beside metrics.json (anomaly_clip_module.py:621-691): `PR.png`,
`ROC.png`, `F1.png` and `confusion_matrix.png`.  The reference draws them with matplotlib (style "ggplot") and seaborn's heatmap;
neither is used here.  The pictures have the reference's panels and texts -- title, axis labels, ticks, grid, curve colour, cell
annotations, colour bar -- drawn with Pillow on the host; they do not reproduce matplotlib's pixels.  No device work happens in
this module: the two curves arrive as the polylines `metrics.evaluate(figure_columns=W)` returns, which hold at most four points
per pixel column of the plot box (first, last, lowest, highest: what a line drawn through every point covers in that column), so
the cost of a figure does not grow with the test set.  `layout` returns every rectangle; the writers know no pixel position.

Files are written as `<name>.<pid>.tmp` and renamed into place; the same inputs give the same bytes."""
from __future__ import annotations

import csv
import math
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .visualizer import _text

CURVE_SIZE = (640, 480)                # matplotlib's default figure, 6.4 x 4.8 inch at 100 dpi
CONFUSION_SIZE = (2000, 1800)          # the reference's figsize=(20, 18)
DEFAULT_COLUMNS = 496                  # matplotlib's default axes: 0.125 ... 0.9 of 640 pixels
Y_MAX = 1.1                            # plt.ylim(0, 1.1)
LINE_W = 2                             # the polyline is drawn LINE_W times, one pixel apart (upwards)
RED, BLUE = (255, 0, 0), (0, 0, 255)   # color="red" / color="blue"
PANEL, GRID, TICK_TEXT, BLACK, WHITE = (0xE5, 0xE5, 0xE5), (255, 255, 255), (0x55, 0x55, 0x55), (0, 0, 0), (255, 255, 255)
# the sequential blue map: white, then ColorBrewer's 9-class "Blues" from its second colour on, linear in between
_BLUES = ((255, 255, 255), (0xDE, 0xEB, 0xF7), (0xC6, 0xDB, 0xEF), (0x9E, 0xCA, 0xE1), (0x6B, 0xAE, 0xD6), (0x42, 0x92, 0xC6),
          (0x21, 0x71, 0xB5), (0x08, 0x51, 0x9C), (0x08, 0x30, 0x6B))
KINDS = ("pr", "roc", "f1", "confusion")
_TEXTS = {"pr": ("Recall", "Precision"), "roc": ("False Positive Rate", "True Positive Rate"), "f1": ("threshold", "F1"),
          "confusion": ("Predicted", "True")}


# ---------------------------------------------------------------------------------------------------------------- layout
def layout(kind: str, size: Optional[Tuple[int, int]] = None, columns: Optional[int] = None, classes: int = 14) -> dict:
    """Every rectangle of a figure, as (x0, y0, x1, y1) with exclusive ends, and its fixed texts.  kind: 'pr', 'roc', 'f1' or
    'confusion'; size: (width, height), default the reference's.  For the three line figures `plot` is the plot box -- exactly
    `columns` pixels wide (default: matplotlib's share of the width), so that one decimation column is one pixel column --
    `x_ticks` / `y_ticks` are (value, pixel) pairs (the y ticks of 'f1' depend on the data: `f1_axis`), `y_range` the values at the
    bottom and the top row.  For 'confusion' `grid` holds classes x classes cells of `cell` = (width, height) pixels and `bar` is the
    colour bar."""
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r}: one of {', '.join(repr(k) for k in KINDS)}")
    Wf, Hf = (CONFUSION_SIZE if kind == "confusion" else CURVE_SIZE) if size is None else (int(size[0]), int(size[1]))
    xl, yl = _TEXTS[kind]
    if kind == "confusion":
        C = int(classes)
        if C < 1 or Wf < 20 * C or Hf < 20 * C:
            raise ValueError(f"layout: {C} classes do not fit a {Wf} x {Hf} confusion matrix")
        x0, y0 = Wf // 8, Hf * 3 // 25
        cw, ch = max(1, (Wf * 31 // 50) // C), max(1, (Hf * 77 // 100) // C)       # the axes less the colour bar's fifth
        grid = (x0, y0, x0 + cw * C, y0 + ch * C)
        bx = grid[2] + Wf // 25
        return {"kind": kind, "size": (Wf, Hf), "classes": C, "grid": grid, "cell": (cw, ch),
                "bar": (bx, y0, bx + Wf * 3 // 100, grid[3]), "x_label": (xl, ((grid[0] + grid[2]) // 2, Hf - Hf // 40)),
                "y_label": (yl, (Wf // 50, (grid[1] + grid[3]) // 2)), "font": (max(10, Hf // 90), max(10, Hf // 120), max(10, Hf // 100))}
    W = int(columns) if columns is not None else Wf * 31 // 40
    x0, y0, y1 = Wf // 8, Hf * 3 // 25, Hf - Hf * 11 // 100
    if W < 1 or x0 + W > Wf - 4 or y1 - y0 < 16:
        raise ValueError(f"layout: a plot box of {W} columns does not fit a {Wf} x {Hf} figure")
    plot = (x0, y0, x0 + W, y1)
    lay = {"kind": kind, "size": (Wf, Hf), "columns": W, "plot": plot, "title": ((x0 + x0 + W) // 2, y0 - Hf // 60),
           "x_label": (xl, ((x0 + x0 + W) // 2, Hf - Hf // 60)), "y_label": (yl, (Wf // 50, (y0 + y1) // 2)),
           "font": (max(10, Hf // 34), max(10, Hf // 40), max(10, Hf // 44))}           # title, axis labels, ticks
    if kind == "f1":
        lay["x_range"] = (0.055, 1.045)                                                # 0.1 ... 1.0 and matplotlib's 5 % margins
        lay["x_ticks"] = [(v, _x_pixel(lay, v)) for v in (0.2, 0.4, 0.6, 0.8, 1.0)]
    else:
        lay["x_range"] = (0.0, 1.0)
        lay["y_range"] = (0.0, Y_MAX)
        lay["x_ticks"] = [(v, plot[0] + min(W - 1, int(v * W))) for v in (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)]
        lay["y_ticks"] = [(v, _y_pixel(lay, v)) for v in (0.0, 0.2, 0.4, 0.6, 0.8, 1.0)]
    return lay


def _x_pixel(lay: dict, v: float) -> int:
    """a value of a continuous x axis (the 'f1' figure's)"""
    p, (lo, hi) = lay["plot"], lay["x_range"]
    return p[0] + int(round((v - lo) / (hi - lo) * (p[2] - p[0] - 1)))


def _y_pixel(lay: dict, v: float) -> int:
    p, (lo, hi) = lay["plot"], lay["y_range"]
    return p[3] - 1 - int(round((v - lo) / (hi - lo) * (p[3] - p[1] - 1)))


def column_of(lay: dict, x: float) -> int:
    """the pixel column of a rate x = count / total in 0 ... 1: plot x0 + min(W - 1, floor(x W)), the decimation's column.  The
    1e-10 makes the float product land where count * W // total does: x W is off by a few 1e-12 at most, and a product that is
    not a whole number lies at least 1 / total > 4e-10 away from the next one."""
    W = lay["columns"]
    return lay["plot"][0] + max(0, min(W - 1, int(math.floor(x * W + 1e-10))))


def f1_axis(lay: dict, values: Sequence[float]) -> dict:
    """`lay` of kind 'f1' with the y axis fitted to the data: 5 % margins like matplotlib's, ticks at a 1-2-5 step; a constant
    series gets a range of its own (+- 0.05) instead of a division by zero"""
    v = [float(x) for x in values if math.isfinite(float(x))] or [0.0]
    lo, hi = min(v), max(v)
    if hi - lo < 1e-12:
        lo, hi = lo - 0.05, hi + 0.05
    else:
        m = 0.05 * (hi - lo)
        lo, hi = lo - m, hi + m
    raw = (hi - lo) / 6
    mag = 10.0 ** math.floor(math.log10(raw))
    step = next(s * mag for s in (1, 2, 5, 10) if s * mag >= raw)
    out = dict(lay)
    out["y_range"] = (lo, hi)
    first = math.ceil(lo / step - 1e-9)
    out["y_ticks"] = [(k * step, _y_pixel(out, k * step)) for k in range(first, first + 12) if k * step <= hi + 1e-12]
    return out


# ---------------------------------------------------------------------------------------------------------------- drawing
def _font(size: int):
    from PIL import ImageFont
    try:
        return ImageFont.load_default(size)
    except TypeError:                                             # Pillow before 10.1: the bitmap font only
        return ImageFont.load_default()


def _save(img, path) -> Path:
    path = Path(path)
    tmp = path.with_name(f"{path.name}.{os.getpid()}.tmp")
    try:
        img.save(tmp, format="PNG")
        os.replace(tmp, path)
    finally:
        if tmp.exists():
            tmp.unlink()
    return path


def _fmt(v: float) -> str:
    return f"{v:.10g}"


def _axes(lay: dict, title: str):
    """the figure without its data: the grey plot box with the white grid, tick labels, axis labels, the title"""
    from PIL import Image, ImageDraw
    img = Image.new("RGB", lay["size"], WHITE)
    d = ImageDraw.Draw(img)
    p = lay["plot"]
    ft, fl, fk = (_font(s) for s in lay["font"])
    d.rectangle([p[0], p[1], p[2] - 1, p[3] - 1], fill=PANEL)
    for v, x in lay["x_ticks"]:
        d.line([(x, p[1]), (x, p[3] - 1)], fill=GRID, width=1)
        _text(img, d, fk, (x, p[3] + 6), _fmt(v), TICK_TEXT, anchor="ct")
    for v, y in lay["y_ticks"]:
        if p[1] <= y < p[3]:
            d.line([(p[0], y), (p[2] - 1, y)], fill=GRID, width=1)
            _text(img, d, fk, (p[0] - 6, y), _fmt(v), TICK_TEXT, anchor="rc")
    _text(img, d, ft, lay["title"], title, BLACK, anchor="cb")
    _text(img, d, fl, lay["x_label"][1], lay["x_label"][0], TICK_TEXT, anchor="cb")
    _text(img, d, fl, lay["y_label"][1], lay["y_label"][0], TICK_TEXT, rotate=True, anchor="lc")
    return img, d


def _polyline(d, pts: List[Tuple[int, int]], colour):
    for k in range(LINE_W):
        q = [(x, y - k) for x, y in pts]
        if len(q) > 1:
            d.line(q, fill=colour, width=1)
        elif q:
            d.point(q, fill=colour)


def _write_curve(kind: str, path, points, auc: float, columns: Optional[int], colour, title: str) -> Path:
    lay = layout(kind, columns=columns)
    img, d = _axes(lay, title)
    if not math.isnan(float(auc)):                                # no positives: the title says nan, the plot box stays empty
        x, y = (np.asarray(a, dtype=np.float64).reshape(-1) for a in points)
        ok = np.isfinite(x) & np.isfinite(y)
        _polyline(d, [(column_of(lay, float(a)), _y_pixel(lay, min(max(float(b), 0.0), Y_MAX))) for a, b in zip(x[ok], y[ok])], colour)
    return _save(img, path)


def write_pr(path, points, auc_pr: float, columns: Optional[int] = None) -> Path:
    """PR.png (:628-641): `points` = (recall, precision) -- `evaluate(figure_columns=columns)["pr_points"]`, or any polyline"""
    return _write_curve("pr", path, points, auc_pr, columns, RED, f"PR Curve: {auc_pr * 100:.2f}")


def write_roc(path, points, auc_roc: float, columns: Optional[int] = None) -> Path:
    """ROC.png (:643-656): `points` = (fpr, tpr) -- `evaluate(figure_columns=columns)["roc_points"]`, or any polyline"""
    return _write_curve("roc", path, points, auc_roc, columns, BLUE, f"ROC Curve: {auc_roc * 100:.2f}")


def write_f1(path, f1_scores: Dict[float, float], columns: Optional[int] = None) -> Path:
    """F1.png (:658-671): the ten F1 scores at thresholds 0.1 ... 1.0 (`evaluate()["f1_scores"]`), the y axis fitted to them"""
    xs = [(i + 1) / 10 for i in range(10)]
    ys = [float(f1_scores[x]) for x in xs]
    lay = f1_axis(layout("f1", columns=columns), ys)
    img, d = _axes(lay, f"F1@0.5: {ys[4] * 100:.2f}")
    _polyline(d, [(_x_pixel(lay, x), _y_pixel(lay, y)) for x, y in zip(xs, ys) if math.isfinite(y)], BLUE)
    return _save(img, path)


def blues(v: float) -> Tuple[int, int, int]:
    """the sequential blue map: white at 0, dark blue at 1"""
    v = 0.0 if not math.isfinite(v) else min(max(float(v), 0.0), 1.0)
    t = v * (len(_BLUES) - 1)
    i = min(int(t), len(_BLUES) - 2)
    a, b = _BLUES[i], _BLUES[i + 1]
    return tuple(int(round(a[c] + (b[c] - a[c]) * (t - i))) for c in range(3))


def read_labels(labels_file) -> Optional[List[str]]:
    """the `name` column of the labels CSV (:601-603), every class"""
    if not labels_file or not os.path.isfile(str(labels_file)):
        return None
    with open(labels_file, newline="") as fh:
        return [row["name"] for row in csv.DictReader(fh)]


def write_confusion(path, matrix, class_names: Optional[Sequence[str]] = None, size: Optional[Tuple[int, int]] = None) -> Path:
    """confusion_matrix.png (:673-691): `matrix` [C, C], rows = true class, normalised over each row (`evaluate()
    ["confusion_matrix"]`); every cell is drawn, also those of a class without frames (a row of zeros)"""
    from PIL import Image, ImageDraw
    m = np.asarray(matrix, dtype=np.float64)
    C = m.shape[0]
    assert m.shape == (C, C)
    lay = layout("confusion", size, classes=C)
    names = [str(n) for n in class_names] if class_names is not None and len(class_names) == C else [str(k) for k in range(C)]
    img = Image.new("RGB", lay["size"], WHITE)
    d = ImageDraw.Draw(img)
    g, (cw, ch), bar = lay["grid"], lay["cell"], lay["bar"]
    fl, fa, fk = (_font(s) for s in lay["font"])
    for r in range(C):
        for c in range(C):
            v = float(m[r, c])
            rgb = blues(v)
            x, y = g[0] + c * cw, g[1] + r * ch
            d.rectangle([x, y, x + cw - 1, y + ch - 1], fill=rgb)
            dark = 0.2126 * rgb[0] + 0.7152 * rgb[1] + 0.0722 * rgb[2] < 0.55 * 255
            _text(img, d, fa, (x + cw // 2, y + ch // 2), f"{v:.2%}", WHITE if dark else (0x26, 0x26, 0x26), anchor="cc")
    for k, name in enumerate(names):
        _text(img, d, fk, (g[0] + k * cw + cw // 2, g[3] + 8), name, TICK_TEXT, rotate=True, anchor="ct")
        _text(img, d, fk, (g[0] - 8, g[1] + k * ch + ch // 2), name, TICK_TEXT, anchor="rc")
    _text(img, d, fl, lay["x_label"][1], lay["x_label"][0], BLACK, anchor="cb")
    _text(img, d, fl, lay["y_label"][1], lay["y_label"][0], BLACK, rotate=True, anchor="lc")
    H = bar[3] - bar[1]
    for y in range(H):                                            # 1 at the top
        d.line([(bar[0], bar[1] + y), (bar[2] - 1, bar[1] + y)], fill=blues(1.0 - y / max(1, H - 1)), width=1)
    for v in (0.0, 0.2, 0.4, 0.6, 0.8, 1.0):
        y = bar[3] - 1 - int(round(v * (H - 1)))
        d.line([(bar[2], y), (bar[2] + 5, y)], fill=TICK_TEXT, width=1)
        _text(img, d, fk, (bar[2] + 10, y), _fmt(v), TICK_TEXT, anchor="lc")
    return _save(img, path)


def write_all(run_dir, result: dict, labels_file=None, columns: Optional[int] = None) -> List[Path]:
    """the four files into `run_dir`, from what `metrics.evaluate(per_frame=True, figure_columns=columns)` returned"""
    run_dir = Path(run_dir)
    return [write_pr(run_dir / "PR.png", result["pr_points"], result["auc_pr"], columns),
            write_roc(run_dir / "ROC.png", result["roc_points"], result["auc_roc"], columns),
            write_f1(run_dir / "F1.png", result["f1_scores"], columns),
            write_confusion(run_dir / "confusion_matrix.png", result["confusion_matrix"], read_labels(labels_file))]
