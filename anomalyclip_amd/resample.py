"""Pillow's 8-bit resampling tables, for any of its separable filters.

`Image.resize` on an 8-bit image is two passes (horizontal, then vertical) over 22-bit fixed-point coefficients with an 8-bit
intermediate.  `coeffs` computes one pass's `(bounds, coef, ksize)` on the host in double precision exactly as Pillow's
`precompute_coeffs` / `normalize_coeffs_8bpc` do (the published algorithm of libImaging/Resample.c); the device kernels apply
them: `acx_preprocess_frames` / `acx_preprocess_crops` with the bicubic filter (anomalyclip_amd/preprocess.py), `acx_viz_compose`
with the triangle filter (anomalyclip_amd/visualizer.py)."""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2


def bicubic(x: float) -> float:
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def bilinear(x: float) -> float:
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


FILTERS = {"bicubic": (bicubic, 2.0), "bilinear": (bilinear, 1.0)}      # name -> (kernel, support)


def coeffs(in_size: int, out_size: int, filter: str = "bicubic"):
    """Pillow precompute_coeffs(inSize, 0, inSize, outSize, filter) + normalize_coeffs_8bpc -> (bounds int32 [out_size, 2]:
    (first input sample, number of taps), coef int32 [out_size, ksize], ksize)"""
    kernel, fsupport = FILTERS[filter]
    scale = filterscale = in_size / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = fsupport * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    bounds = np.zeros((out_size, 2), dtype=np.int32)
    kk = np.zeros((out_size, ksize), dtype=np.int32)
    ss = 1.0 / filterscale
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = int(center - support + 0.5)
        if xmin < 0:
            xmin = 0
        xmax = int(center + support + 0.5)
        if xmax > in_size:
            xmax = in_size
        xmax -= xmin
        w = [kernel((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = sum(w)
        for x in range(xmax):
            v = w[x] / ww if ww != 0.0 else w[x]
            kk[xx, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[xx] = (xmin, xmax)
    return bounds, kk, ksize
