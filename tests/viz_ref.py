"""What the qualitative-video tests compare with, on the host: a Pillow oracle of the composed picture, DESIGN.md's integer
arithmetic of acx_jpeg_forward restated in numpy, its fp64 counterpart, the coefficient edge cases of the entropy encoder and a walker
over a RIFF file.  Nothing here imports the code under test except `layout`'s helpers, which only return rectangles."""
import io
import struct

import numpy as np
from PIL import Image, ImageDraw

from anomalyclip_amd import visualizer as V

# zigzag position -> natural position (ISO/IEC 10918-1 figure 5)
NATURAL = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                    62, 63])


# ---------------------------------------------------------------------------------------------------------------- composition
def bar_heights(p: np.ndarray, PH: int) -> np.ndarray:
    """floor(p * PH + 0.5) in float32, product and sum rounded separately, clipped to 0 .. PH"""
    v = (np.asarray(p, np.float32) * np.float32(PH)).astype(np.float32) + np.float32(0.5)
    return np.clip(np.floor(v.astype(np.float32)), 0, PH).astype(np.int64)


def top3(p: np.ndarray):
    """the indices of the three largest, the lower index first among equals"""
    return sorted(range(len(p)), key=lambda k: (-float(p[k]), k))[:3]


def compose_oracle(lay: dict, static: np.ndarray, frame: np.ndarray, score: float, p: np.ndarray, i: int, threshold: float) -> np.ndarray:
    """one canvas: the static layer, Pillow's BILINEAR resize pasted into the inner rectangle, then border, bars and cursor with
    ImageDraw.rectangle -- from layout() and the issue's formulas"""
    img = Image.fromarray(static.copy())
    f = lay["frame"]
    img.paste(Image.fromarray(frame).resize((f[2] - f[0], f[3] - f[1]), Image.BILINEAR), (f[0], f[1]))
    d = ImageDraw.Draw(img)
    o, bd = lay["frame_outer"], lay["border"]
    colour = (0, 0, 255) if np.float32(score) < np.float32(threshold) else (255, 0, 0)
    for r in ((o[0], o[1], o[2], o[1] + bd), (o[0], o[3] - bd, o[2], o[3]), (o[0], o[1], o[0] + bd, o[3]), (o[2] - bd, o[1], o[2], o[3])):
        d.rectangle([r[0], r[1], r[2] - 1, r[3] - 1], fill=colour)
    bp = lay["bars_panel"]
    h = bar_heights(p, bp[3] - bp[1])
    hot = top3(p) if np.float32(score) >= np.float32(threshold) else []
    for k in range(lay["C1"]):
        if h[k] > 0:
            r = V.bar_rect(lay, k, int(h[k]))
            d.rectangle([r[0], r[1], r[2] - 1, r[3] - 1], fill=(255, 0, 0) if k in hot else (128, 128, 128))
    sp = lay["score_panel"]
    x = V.cursor_x(lay, i)
    d.rectangle([x, sp[1], x + lay["cursor_w"] - 1, sp[3] - 1], fill=(255, 0, 0))
    return np.asarray(img)


def psnr(a: np.ndarray, b: np.ndarray) -> float:
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return float("inf") if mse == 0 else float(10 * np.log10(255.0 ** 2 / mse))


# ---------------------------------------------------------------------------------------------------------------- forward JPEG
def dct_matrix_fixed() -> np.ndarray:
    """C[u][x] = round(2^14 a(u) cos((2x + 1) u pi / 16)), a(0) = sqrt(1/8), a(u) = 1/2"""
    return np.round(dct_matrix() * 16384).astype(np.int64)


def dct_matrix() -> np.ndarray:
    u, x = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    a = np.where(u == 0, np.sqrt(1 / 8), 0.5)
    return a * np.cos((2 * x + 1) * u * np.pi / 16)


def _blocks(plane: np.ndarray) -> np.ndarray:
    """[h, w] -> [h/8, w/8, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).transpose(0, 2, 1, 3)


def forward_restated(canvas: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """DESIGN.md section 4, "Qualitative videos": the integer arithmetic of acx_jpeg_forward on one canvas [Hc, Wc, 3] uint8 with the
    tables qt [2, 64] -> int16 [Hc * Wc * 3 / 2], luma blocks then Cb then Cr, each [blocks high][blocks wide][64]"""
    c = canvas.astype(np.int64)
    R, G, B = c[..., 0], c[..., 1], c[..., 2]
    y = (19595 * R + 38470 * G + 7471 * B - (128 << 16) + 512) >> 10
    cb = -11059 * R - 21709 * G + 32768 * B
    cr = 32768 * R - 27439 * G - 5329 * B
    mean = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2] + 2048) >> 12
    C = dct_matrix_fixed()
    out = []
    for plane, t in ((y, 0), (mean(cb), 1), (mean(cr), 1)):
        s = _blocks(plane)
        t1 = (np.einsum("ux,abyx->abyu", C, s) + 8192) >> 14          # along the rows
        v = (np.einsum("vy,abyu->abvu", C, t1) + 8192) >> 14          # down the columns
        q64 = qt[t].astype(np.int64).reshape(8, 8) * 64
        n = np.minimum((np.abs(v) + q64 // 2) // q64, 1023)
        out.append((np.sign(v) * n).reshape(-1))
    return np.concatenate(out).astype(np.int16)


def forward_fp64(canvas: np.ndarray, qt: np.ndarray) -> np.ndarray:
    """the same in double precision: JFIF colour conversion, 2x2 mean, level shift, orthonormal DCT, division by the table rounded
    half away from zero (not clamped) -> float64 [Hc * Wc * 3 / 2] of integers"""
    c = canvas.astype(np.float64)
    R, G, B = c[..., 0], c[..., 1], c[..., 2]
    y = 0.299 * R + 0.587 * G + 0.114 * B - 128.0
    cb = -0.168736 * R - 0.331264 * G + 0.5 * B
    cr = 0.5 * R - 0.418688 * G - 0.081312 * B
    mean = lambda p: (p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]) / 4.0
    D = dct_matrix()
    out = []
    for plane, t in ((y, 0), (mean(cb), 1), (mean(cr), 1)):
        v = np.einsum("vy,abyx,ux->abvu", D, _blocks(plane), D) / qt[t].astype(np.float64).reshape(8, 8)
        out.append((np.sign(v) * np.floor(np.abs(v) + 0.5)).reshape(-1))
    return np.concatenate(out)


def pillow_decode(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    im.load()
    return np.asarray(im.convert("RGB"))


# ---------------------------------------------------------------------------------------------------------------- entropy cases
def coef_elems(H: int, W: int) -> int:
    return ((W + 15) // 16) * ((H + 15) // 16) * 6 * 64


def edge_blocks():
    """[(name, block int16 [64] natural order)]: what the Huffman coder treats specially"""
    out = []
    b = np.zeros(64, np.int16)
    b[NATURAL[63]] = 5
    out.append(("only coefficient 63: no EOB", b))
    for run in range(16, 63):                                      # `run` zeros, then a value at zigzag position run + 1
        b = np.zeros(64, np.int16)
        b[NATURAL[run + 1]] = -3 if run & 1 else 7
        out.append((f"zero run {run}", b))
    for v in (1023, -1023):
        b = np.zeros(64, np.int16)
        b[NATURAL[1]] = v
        b[NATURAL[40]] = -v
        b[NATURAL[63]] = v
        out.append((f"AC {v}", b))
    return out


def entropy_cases(H: int, W: int, seed: int = 0):
    """[(name, coefficients int16 [coef_elems])] for an H x W frame"""
    n = coef_elems(H, W)
    nb = n // 64
    rng = np.random.default_rng(seed + H * 7 + W)
    cases = [("all zero", np.zeros(n, np.int16))]
    edges = edge_blocks()
    for k in range(0, len(edges), nb):                             # the edge blocks, as many frames as they need
        c = np.zeros((nb, 64), np.int16)
        part = edges[k:k + nb]
        for j, (_, b) in enumerate(part):
            c[j] = b
        cases.append((f"edge blocks {k}..{k + len(part) - 1}", c.reshape(-1)))
    c = np.zeros((nb, 64), np.int16)                               # DC +-1023 alternating: differences of category 11, both signs
    c[:, 0] = np.where(np.arange(nb) % 2 == 0, 1023, -1023)
    cases.append(("DC differences of category 11", c.reshape(-1)))
    dense = rng.integers(-1023, 1024, size=(nb, 64)).astype(np.int16)          # every byte value, FF among them
    cases.append(("dense random: FF bytes", dense.reshape(-1)))
    sparse = np.where(rng.random((nb, 64)) < 0.1, rng.integers(-40, 41, size=(nb, 64)), 0).astype(np.int16)
    cases.append(("sparse random", sparse.reshape(-1)))
    return cases


# ---------------------------------------------------------------------------------------------------------------- RIFF
def riff_chunks(data: bytes, start: int, end: int):
    """[(fourcc, payload offset, size, list type or None)] of the chunks in data[start:end]; sizes must tile the range exactly"""
    out, p = [], start
    while p < end:
        assert p + 8 <= end, "a chunk header runs past its parent"
        cc, size = data[p:p + 4], struct.unpack_from("<I", data, p + 4)[0]
        assert p + 8 + size <= end, (cc, size, "runs past its parent")
        out.append((cc, p + 8, size, data[p + 8:p + 12] if cc in (b"RIFF", b"LIST") else None))
        p += 8 + size + (size & 1)
    assert p == end, "the chunks do not tile their parent"
    return out


def walk_avi(data: bytes) -> dict:
    """checks the declared sizes of a Motion-JPEG AVI and returns {"frames": [payload bytes], "avih_frames", "strh_length",
    "width", "height", "handler", "index": [(offset of the chunk header from the `movi` fourcc, size)], "movi": offset of that fourcc}"""
    top = riff_chunks(data, 0, len(data))
    assert len(top) == 1 and top[0][0] == b"RIFF" and top[0][3] == b"AVI "
    body = riff_chunks(data, top[0][1] + 4, top[0][1] + top[0][2])
    assert [(c, t) for c, _, _, t in body] == [(b"LIST", b"hdrl"), (b"LIST", b"movi"), (b"idx1", None)]
    hdrl = riff_chunks(data, body[0][1] + 4, body[0][1] + body[0][2])
    assert [(c, t) for c, _, _, t in hdrl] == [(b"avih", None), (b"LIST", b"strl")] and hdrl[0][2] == 56
    avih = struct.unpack_from("<14I", data, hdrl[0][1])
    strl = riff_chunks(data, hdrl[1][1] + 4, hdrl[1][1] + hdrl[1][2])
    assert [c for c, *_ in strl] == [b"strh", b"strf"] and strl[0][2] == 56 and strl[1][2] == 40
    strh = struct.unpack_from("<4s4sIHHIIIIIIII4H", data, strl[0][1])
    strf = struct.unpack_from("<IiiHH4sIiiII", data, strl[1][1])
    assert strh[0] == b"vids" and strf[0] == 40 and strf[5] == b"MJPG" and (strf[1], strf[2]) == (avih[8], avih[9])
    movi = riff_chunks(data, body[1][1] + 4, body[1][1] + body[1][2])
    assert all(c == b"00dc" for c, *_ in movi)
    n = body[2][2] // 16
    assert body[2][2] == 16 * n
    index = [struct.unpack_from("<4sIII", data, body[2][1] + 16 * k) for k in range(n)]
    assert all(e[0] == b"00dc" for e in index)
    return {"frames": [data[o:o + s] for _, o, s, _ in movi], "avih_frames": avih[4], "strh_length": strh[9], "rate": strh[7] / strh[6],
            "width": avih[8], "height": avih[9], "handler": strh[1], "index": [(e[2], e[3]) for e in index], "movi": body[1][1],
            "chunks": [(o - 8, s) for _, o, s, _ in movi]}
