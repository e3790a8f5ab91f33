"""Plain-numpy restatement of baseline JPEG reconstruction as Pillow (libjpeg-turbo with its defaults) does it: coefficient blocks +
quantisation tables -> RGB.  Integer "islow" inverse DCT (jidctint: CONST_BITS 13, PASS1_BITS 2, columns first), "fancy" (triangle)
chroma upsampling with the plane's REAL edge replicated, table-exact YCbCr -> RGB.  Shared by tests/test_cpu_jpeg.py (which pins it
and the host entropy decoder to Pillow) and tests/test_gpu_jpeg.py; `host_decode` runs the library's two host entry points through
ctypes, `make_image` / `save_jpeg` write the seeded test images."""
import ctypes as C
import io

import numpy as np
from PIL import Image

A, B, C_, D, E, F_, G, H_, I, J, K, L_ = 2446, 3196, 4433, 6270, 7373, 9633, 12299, 15137, 16069, 16819, 20995, 25172

SIZES = [(16, 16), (17, 23), (45, 67), (33, 31), (8, 40)]          # (H, W)
MODES = [0, 1, 2, "L"]                                            # Pillow's `subsampling` 4:4:4 / 4:2:2 / 4:2:0, and greyscale
QUALITIES = [30, 75, 95, 100]
SIGMAS = [0, 25, 120]


def _pass(x, s):
    """one 8-point pass along axis -1 of an int64 array [..., 8], descaled by s"""
    x0, x1, x2, x3, x4, x5, x6, x7 = (x[..., k] for k in range(8))
    z1 = (x2 + x6) * C_
    t2 = z1 - x6 * H_
    t3 = z1 + x2 * D
    t0 = (x0 + x4) << 13
    t1 = (x0 - x4) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = x7, x5, x3, x1
    z1 = o0 + o3
    z2 = o1 + o2
    z3 = o0 + o2
    z4 = o1 + o3
    z5 = (z3 + z4) * F_
    o0, o1, o2, o3 = o0 * A, o1 * J, o2 * L_, o3 * G
    z1, z2 = z1 * -E, z2 * -K
    z3 = z3 * -I + z5
    z4 = z4 * -B + z5
    o0, o1, o2, o3 = o0 + z1 + z3, o1 + z2 + z4, o2 + z2 + z3, o3 + z1 + z4
    out = np.stack([t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3], -1)
    return (out + (1 << (s - 1))) >> s


def idct_plane(coef, q):
    """coef int16 [bh, bw, 64] (natural order, not dequantised), q [64] -> uint8 plane [bh * 8, bw * 8]"""
    bh, bw, _ = coef.shape
    x = (coef.astype(np.int64) * q.astype(np.int64)).reshape(bh, bw, 8, 8)
    ws = _pass(x.swapaxes(-1, -2), 11).swapaxes(-1, -2)               # pass 1 down the columns
    px = np.clip(_pass(ws, 18) + 128, 0, 255)                         # pass 2 along the rows
    return px.transpose(0, 2, 1, 3).reshape(bh * 8, bw * 8).astype(np.uint8)


def _edge(a, axis, shift):
    """a shifted by one along axis, the edge sample repeated"""
    idx = np.clip(np.arange(a.shape[axis]) + shift, 0, a.shape[axis] - 1)
    return np.take(a, idx, axis=axis)


def upsample(p, hs, vs, H, W):
    """the real samples p [dh, dw] of a chroma plane -> [H, W]"""
    p = p.astype(np.int64)
    if hs == 1:
        return p[:H, :W]
    if vs == 1:
        s, add0, add1, sh = p, 1, 2, 2
        rows = [s]
    else:
        rows = [3 * p + _edge(p, 0, -1), 3 * p + _edge(p, 0, +1)]      # output rows 2r and 2r + 1
        add0, add1, sh = 8, 7, 4
    outs = []
    for s in rows:
        o = np.empty((s.shape[0], s.shape[1] * 2), dtype=np.int64)
        o[:, 0::2] = (3 * s + _edge(s, 1, -1) + add0) >> sh
        o[:, 1::2] = (3 * s + _edge(s, 1, +1) + add1) >> sh
        outs.append(o)
    if vs == 1:
        return outs[0][:H, :W]
    full = np.empty((outs[0].shape[0] * 2, outs[0].shape[1]), dtype=np.int64)
    full[0::2], full[1::2] = outs
    return full[:H, :W]


def _fix(x):
    return int(x * 65536 + 0.5)


def colour(y, cb, cr):
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    r = y + ((_fix(1.402) * cr + 32768) >> 16)
    g = y + ((-_fix(0.34414) * cb + 32768 - _fix(0.71414) * cr) >> 16)
    b = y + ((_fix(1.772) * cb + 32768) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def reconstruct(geom, coef, qt):
    """geom: dict(H, W, ncomp, hs, vs, blocks=[(bh, bw)], offsets=[...]); coef int16 [coef_elems]; qt [ncomp, 64] per component
    -> uint8 [H, W, 3]"""
    H, W, hs, vs = geom["H"], geom["W"], geom["hs"], geom["vs"]
    planes = []
    for c, ((bh, bw), off) in enumerate(zip(geom["blocks"], geom["offsets"])):
        planes.append(idct_plane(coef[off:off + bh * bw * 64].reshape(bh, bw, 64), qt[c]))
    y = planes[0][:H, :W]
    if geom["ncomp"] == 1:
        return np.stack([y, y, y], -1)
    dh, dw = -(-H // vs), -(-W // hs)
    cb, cr = (upsample(p[:dh, :dw], hs, vs, H, W) for p in planes[1:])
    return colour(y, cb, cr)


# ---------------------------------------------------------------------------------------------------------------- the host decoder
def host_decode(data: bytes, guard: int = 0):
    """acx_jpeg_parse + acx_jpeg_entropy_decode through ctypes -> (rc, geom, coef int16 [coef_elems], qt uint16 [ncomp, 64]); with
    `guard` > 0 the coefficient buffer sits between two runs of `guard` marker words, and their survival is asserted"""
    from anomalyclip_amd import _lib as L
    lib = L.lib()
    info = L.JpegInfo()
    buf = (C.c_char * max(1, len(data))).from_buffer_copy(data or b"\0")
    rc = lib.acx_jpeg_parse(C.addressof(buf), len(data), C.addressof(info))
    if rc != 0:
        return rc, None, None, None
    n = int(info.coef_elems)
    arr = np.full(n + 2 * guard, 0x5A5A, dtype=np.int16)
    arr[guard:guard + n] = 0
    rc = lib.acx_jpeg_entropy_decode(C.addressof(buf), len(data), C.addressof(info), arr.ctypes.data + 2 * guard, n)
    if guard:
        assert (arr[:guard] == 0x5A5A).all() and (arr[guard + n:] == 0x5A5A).all(), "guard words overwritten"
    nc = int(info.ncomp)
    geom = dict(H=int(info.height), W=int(info.width), ncomp=nc, hs=int(info.comp_h[0]), vs=int(info.comp_v[0]),
                blocks=[(int(info.blocks_high[c]), int(info.blocks_wide[c])) for c in range(nc)],
                offsets=[int(info.coef_offset[c]) for c in range(nc)], coef_elems=n, restart_interval=int(info.restart_interval))
    qt = np.stack([np.array(info.qtab[int(info.comp_tq[c])][:], dtype=np.uint16) for c in range(nc)])
    return rc, geom, arr[guard:guard + n].copy(), qt


# ---------------------------------------------------------------------------------------------------------------- test images
def make_image(h, w, sigma, seed, grey=False):
    """smooth gradients + a flat patch + Gaussian noise of the given sigma, seeded"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(xx * 5 + yy * 2) % 256, (yy * 7 + 30) % 256, ((xx + yy) * 3 + 90) % 256], -1).astype(np.float64)
    a[: h // 3, : w // 3] = (250, 10, 128)
    if sigma:
        a = a + rng.normal(0, sigma, a.shape)
    a = np.clip(a, 0, 255).astype(np.uint8)
    return a[..., 0] if grey else a


def save_jpeg(a, quality=75, subsampling=None, **kw) -> bytes:
    fh = io.BytesIO()
    if subsampling is not None and a.ndim == 3:
        kw["subsampling"] = subsampling
    Image.fromarray(a).save(fh, "JPEG", quality=quality, **kw)
    return fh.getvalue()


def pillow_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def grid_cases():
    """(name, bytes) over sizes x modes x qualities x noise: the grid of both test files"""
    out = []
    for hi, (h, w) in enumerate(SIZES):
        for mode in MODES:
            for q in QUALITIES:
                for sg in SIGMAS:
                    a = make_image(h, w, sg, seed=hi * 1000 + q * 7 + sg, grey=(mode == "L"))
                    out.append((f"{h}x{w}-s{mode}-q{q}-n{sg}", save_jpeg(a, q, None if mode == "L" else mode)))
    return out
