"""The qualitative videos of `data.visualize=True` (reference src/utils/visualizer.py, called from anomaly_clip_module.py:447-456 and
:485-492): per test video one clip that shows the frame with a blue (normal) or red (abnormal) border, the `P(c|A)` bar chart and
the `p(A)` curve with the ground-truth intervals shaded and a cursor on the current frame.

The reference draws a matplotlib figure per frame and hands the figures to `cv2.VideoWriter`.  Here the picture has two layers.
What does not change within a video -- panel frames, guide lines, labels, class names, the title, the score curve, the shaded
ground truth -- is drawn ONCE per video on the host with Pillow (`static_layer`).  What changes per frame -- the resized frame and its
border, the bars, the cursor -- is composed on the device over a copy of that layer (`ops.viz_compose`), for a batch of frames per
launch sequence, from the decoded frames `jpeg.make_reader` delivers and the scores `test_step` already holds there.  The canvases
are turned into quantised JPEG coefficients on the device (`ops.jpeg_forward`), copied to pinned memory and Huffman-coded on a
thread pool (`ops.jpeg_entropy_encode`) while the device works on the next batch.  With `entropy="gpu"` the Huffman coding runs on
the device as well (`ops.jpeg_entropy_encode_dev`): no pool, and what is copied to the host is each frame's file, not its
coefficients.  `layout` returns every rectangle; both layers use it and nothing else knows a pixel position."""
from __future__ import annotations

import csv
import os
import struct
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from . import ops
from . import resample

BORDER = 5                             # the reference's cv2.rectangle thickness
CURSOR_W = 2
CURVE_COLOUR, TRUTH_COLOUR = (0x4E, 0x79, 0xA7), (0xE1, 0x57, 0x59)
MAX_THREADS = 16
ENTROPY = ("host", "gpu")              # where the frames are Huffman-coded


def check_entropy(entropy, key: str = "entropy") -> str:
    if entropy not in ENTROPY:
        raise ValueError(f"{key}={entropy!r}: one of {', '.join(repr(e) for e in ENTROPY)}")
    return entropy

# ISO/IEC 10918-1 Annex K.1 / K.2: the typical quantisation tables, natural (row-major) order
_K1 = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
       18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112,
       100, 103, 99)
_K2 = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32


def quant_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64] (luma, chroma; natural order): the Annex K tables under libjpeg's quality scaling (jpeg_quality_scaling,
    then jpeg_add_quant_table with force_baseline), quality 1 ... 100"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality={quality!r}: 1 ... 100")
    scale = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([_K1, _K2], dtype=np.int64)
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.uint16)


# ---------------------------------------------------------------------------------------------------------------- layout
def layout(canvas: Tuple[int, int], C1: int, frame_hw: Tuple[int, int], T: int) -> dict:
    """Every rectangle of the picture, as (x0, y0, x1, y1) with exclusive ends, for a canvas (width, height), C1 bars, source
    frames (H, W) and a video of T frames.  The upper half holds the frame panel (left) and the bars panel (right), the lower half
    the score panel.  `frame` is the resized source: it keeps the source's aspect ratio (the longer side fills the panel less the
    border, the other is rounded to the nearest pixel) and is centred in `frame_panel`; `frame_outer` is `frame` grown by the
    border.  Bar k covers columns bar_x0 + k * bar_pitch ... + bar_w of `bars_panel`."""
    Wc, Hc = int(canvas[0]), int(canvas[1])
    H, W = int(frame_hw[0]), int(frame_hw[1])
    C1, T = int(C1), int(T)
    if Wc < 160 or Hc < 120:
        raise ValueError(f"canvas={canvas!r}: at least 160 x 120")
    if not 1 <= C1 <= 64 or T < 1 or H < 1 or W < 1:
        raise ValueError(f"layout: 1 <= C1 <= 64, T >= 1 and a non-empty source; got C1={C1}, T={T}, source {H} x {W}")
    fp = (Wc // 40, Hc // 20, Wc // 2 - Wc // 40, Hc // 2 - Hc // 40)
    aw, ah = fp[2] - fp[0] - 2 * BORDER, fp[3] - fp[1] - 2 * BORDER
    if W * ah <= H * aw:                                          # the height fills the panel
        fh, fw = ah, max(1, (W * ah + H // 2) // H)
    else:
        fw, fh = aw, max(1, (H * aw + W // 2) // W)
    fx, fy = fp[0] + BORDER + (aw - fw) // 2, fp[1] + BORDER + (ah - fh) // 2
    bp = (Wc // 2 + Wc // 12, Hc // 20, Wc - Wc // 40, Hc // 2 - Hc // 7)
    pitch = (bp[2] - bp[0]) // C1
    if pitch < 1:
        raise ValueError(f"canvas={canvas!r} is too narrow for {C1} bars")
    bar_w = max(1, pitch * 4 // 5)
    bar_x0 = bp[0] + (bp[2] - bp[0] - pitch * C1) // 2 + (pitch - bar_w) // 2
    sp = (Wc // 12, Hc // 2 + Hc // 20, Wc - Wc // 40, Hc - Hc // 10)
    return {"canvas": (Wc, Hc), "source": (H, W), "C1": C1, "T": T, "border": BORDER, "cursor_w": CURSOR_W,
            "frame_panel": fp, "frame": (fx, fy, fx + fw, fy + fh),
            "frame_outer": (fx - BORDER, fy - BORDER, fx + fw + BORDER, fy + fh + BORDER),
            "bars_panel": bp, "bar_pitch": pitch, "bar_w": bar_w, "bar_x0": bar_x0, "score_panel": sp}


def bar_rect(lay: dict, k: int, h: int) -> Tuple[int, int, int, int]:
    """bar k at height h (rows from the panel's bottom)"""
    x0 = lay["bar_x0"] + k * lay["bar_pitch"]
    return (x0, lay["bars_panel"][3] - h, x0 + lay["bar_w"], lay["bars_panel"][3])


def cursor_x(lay: dict, i: int) -> int:
    """the first column of frame i in the score panel: x0 + (i * (PW - 1)) // T"""
    sp = lay["score_panel"]
    return sp[0] + (i * (sp[2] - sp[0] - 1)) // lay["T"]


def geom_of(lay: dict, threshold: float) -> "L.VizGeom":
    """the layout as acx_viz_compose takes it"""
    g = L.VizGeom()
    g.Wc, g.Hc = lay["canvas"]
    g.H, g.W = lay["source"]
    f, bp, sp = lay["frame"], lay["bars_panel"], lay["score_panel"]
    g.fx, g.fy, g.fw, g.fh, g.border = f[0], f[1], f[2] - f[0], f[3] - f[1], lay["border"]
    g.bx, g.by, g.bh, g.bar_pitch, g.bar_w, g.C1 = lay["bar_x0"], bp[1], bp[3] - bp[1], lay["bar_pitch"], lay["bar_w"], lay["C1"]
    g.sx, g.sy, g.sw, g.sh, g.cursor_w, g.T = sp[0], sp[1], sp[2] - sp[0], sp[3] - sp[1], lay["cursor_w"], lay["T"]
    g.threshold = float(threshold)
    return g


def resize_tables(lay: dict, device) -> tuple:
    """(hbounds, hcoef, hksize, vbounds, vcoef, vksize) of Pillow's BILINEAR resize of the source to the inner rectangle"""
    H, W = lay["source"]
    f = lay["frame"]
    hb, hk, hks = resample.coeffs(W, f[2] - f[0], "bilinear")
    vb, vk, vks = resample.coeffs(H, f[3] - f[1], "bilinear")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
    return t(hb), t(hk), hks, t(vb), t(vk), vks


# ---------------------------------------------------------------------------------------------------------------- static layer
def read_class_names(labels_csv_path) -> Optional[List[str]]:
    """the `name` column of the labels CSV without `Normal`, `RoadAccidents` shortened as the reference does (visualizer.py:232-238)"""
    if not labels_csv_path:
        return None
    with open(labels_csv_path, newline="") as fh:
        names = [row["name"] for row in csv.DictReader(fh)]
    if "Normal" in names:
        names.remove("Normal")
    return [n.replace("RoadAccidents", "RoadAcc.") for n in names]


def _dashed(draw, x0: int, x1: int, y: int, fill, on: int = 6, off: int = 4):
    for x in range(x0, x1, on + off):
        draw.line([(x, y), (min(x + on, x1) - 1, y)], fill=fill, width=1)


def _text(img, draw, font, xy, text: str, fill=(0, 0, 0), rotate: bool = False, anchor: str = "lt"):
    """`text` with its box's `anchor` corner (l / c / r, t / c / b) at xy; rotate: read bottom to top, like matplotlib's rotation=90"""
    from PIL import Image, ImageDraw
    box = draw.textbbox((0, 0), text, font=font)
    w, h = max(1, box[2]), max(1, box[3])
    m = Image.new("L", (w + 2, h + 2), 0)
    ImageDraw.Draw(m).text((1, 1), text, fill=255, font=font)
    if rotate:
        m = m.rotate(90, expand=True)
    x = xy[0] - {"l": 0, "c": m.size[0] // 2, "r": m.size[0]}[anchor[0]]
    y = xy[1] - {"t": 0, "c": m.size[1] // 2, "b": m.size[1]}[anchor[1]]
    img.paste(fill, (int(x), int(y)), m)
    return m.size


def static_layer(lay: dict, scores: np.ndarray, labels: np.ndarray, normal_idx: int, class_names: Optional[Sequence[str]],
                 title: str) -> np.ndarray:
    """uint8 [Hc, Wc, 3]: everything of a video's picture that no frame changes, drawn with Pillow"""
    from PIL import Image, ImageDraw, ImageFont
    Wc, Hc = lay["canvas"]
    C1, T = lay["C1"], lay["T"]
    img = Image.new("RGB", (Wc, Hc), (255, 255, 255))
    d = ImageDraw.Draw(img)
    font = ImageFont.load_default()
    grey, black = (128, 128, 128), (0, 0, 0)
    bp, sp = lay["bars_panel"], lay["score_panel"]
    PH, SH = bp[3] - bp[1], sp[3] - sp[1]
    # the score panel: ground truth, guide lines, the curve, the title
    labels = np.asarray(labels).reshape(-1)
    truth = tuple((255 + c + 1) // 2 for c in TRUTH_COLOUR)                   # alpha 0.5 over the white background
    run = None
    for i in range(len(labels) + 1):
        hot = i < len(labels) and int(labels[i]) != int(normal_idx)
        if hot and run is None:
            run = i
        elif not hot and run is not None:
            d.rectangle([cursor_x(lay, min(run, T - 1)), sp[1], min(cursor_x(lay, min(i, T - 1)) + 1, sp[2] - 1), sp[3] - 1], fill=truth)
            run = None
    for v in (0.25, 0.5, 0.75):
        y = sp[3] - 1 - int(round(v * (SH - 1)))
        _dashed(d, sp[0], sp[2], y, grey)
        _text(img, d, font, (sp[0] - 5, y), f"{v:g}", black, anchor="rc")
    s = np.nan_to_num(np.asarray(scores, dtype=np.float64).reshape(-1), nan=0.0)
    pts = [(cursor_x(lay, i), sp[3] - 1 - int(round(min(max(float(s[i]), 0.0), 1.0) * (SH - 1)))) for i in range(min(T, len(s)))]
    if len(pts) > 1:
        d.line(pts, fill=CURVE_COLOUR, width=1)
    elif pts:
        d.point(pts, fill=CURVE_COLOUR)
    _text(img, d, font, (sp[0] + (sp[2] - sp[0]) // 50, sp[1] + SH // 10), title, black, anchor="lb")
    _text(img, d, font, (sp[0] - Wc // 24, (sp[1] + sp[3]) // 2), "p(A)", black, rotate=True, anchor="rc")
    _text(img, d, font, ((sp[0] + sp[2]) // 2, sp[3] + Hc // 40), "Frame Number", black, anchor="ct")
    # the bars panel: guide lines, class names under the bars
    for v in (0.2, 0.4, 0.6, 0.8):
        _dashed(d, bp[0], bp[2], bp[3] - int(round(v * PH)), grey)
    _text(img, d, font, (bp[0] - Wc // 40, (bp[1] + bp[3]) // 2), "P(c|A)", black, rotate=True, anchor="rc")
    names = list(class_names) if class_names is not None and len(class_names) == C1 else [str(k) for k in range(C1)]
    line_h = max(1, d.textbbox((0, 0), "Ag", font=font)[3] + 2)
    every = -(-line_h // lay["bar_pitch"])                                    # bars closer than a line of text: label every n-th
    for k in range(0, C1, every):
        _text(img, d, font, (lay["bar_x0"] + k * lay["bar_pitch"] + lay["bar_w"] // 2, bp[3] + 4), names[k], black, rotate=True, anchor="ct")
    # the panel frames, one pixel outside what the device draws into
    for r in (bp, sp):
        d.rectangle([r[0] - 1, r[1] - 1, r[2], r[3]], outline=black, width=1)
    return np.array(img, dtype=np.uint8)                                      # (a writable copy)


# ---------------------------------------------------------------------------------------------------------------- container
class AviWriter:
    """A Motion-JPEG AVI 1.0 file: RIFF `AVI ` with `hdrl` (`avih`, one `strl` of `strh` `vids` / `MJPG` and `strf`), `movi` of
    `00dc` chunks (one JFIF file each) and `idx1`; sizes and the frame count are patched at close.

    The reference writes `.mp4` with the `mp4v` codec through cv2.VideoWriter; this stack has no MPEG-4 encoder (and no cv2), and
    every player that reads the one reads Motion-JPEG in AVI, so the clips are `.avi`.

    A stream that would pass `max_file_bytes` (AVI 1.0 sizes are 32-bit) continues in `<stem>.part1.avi`, `<stem>.part2.avi` ...
    Every part is written under a temporary name; close() renames them, the first part `<stem>.avi` last, so that the file whose
    existence means "done" never stands for a torn clip.  abort() removes what was written."""

    HEADER = 224                       # bytes before the first chunk; the `movi` fourcc is at HEADER - 4

    def __init__(self, path, width: int, height: int, fps: float = 30, max_file_bytes: int = 1 << 30):
        self.path = Path(path)
        self.width, self.height, self.fps = int(width), int(height), float(fps)
        self.max_file_bytes = min(int(max_file_bytes), (1 << 31) - 1)
        self.frames = 0                # of all parts
        self._parts: List[Tuple[Path, Path]] = []      # (temporary, final)
        self._fh = None
        self._index: List[Tuple[int, int]] = []
        self._size = 0

    def _final(self, k: int) -> Path:
        return self.path if k == 0 else self.path.with_name(f"{self.path.stem}.part{k}{self.path.suffix}")

    def _open(self):
        final = self._final(len(self._parts))
        tmp = final.with_name(f"{final.name}.{os.getpid()}.tmp")
        self._parts.append((tmp, final))
        self._fh = open(tmp, "wb")
        self._fh.write(b"\0" * self.HEADER)
        self._index, self._size = [], self.HEADER

    def _header(self, nframes: int, movi_bytes: int, riff_bytes: int, largest: int) -> bytes:
        rate, scale = int(round(self.fps * 1000)), 1000
        avih = struct.pack("<14I", int(round(1e6 / self.fps)), int(largest * self.fps), 0, 0x10, nframes, 0, 1, largest, self.width,
                           self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, scale, rate, 0, nframes, largest, 0xFFFFFFFF, 0,
                           0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"LIST" + struct.pack("<I", 4 + 8 + len(strh) + 8 + len(strf)) + b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + \
            b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"LIST" + struct.pack("<I", 4 + 8 + len(avih) + len(strl)) + b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + strl
        head = b"RIFF" + struct.pack("<I", riff_bytes - 8) + b"AVI " + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        assert len(head) == self.HEADER, len(head)
        return head

    def _finish_part(self):
        fh, n = self._fh, len(self._index)
        movi_bytes = self._size - self.HEADER
        fh.write(b"idx1" + struct.pack("<I", 16 * n))
        fh.write(b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in self._index))
        total = self._size + 8 + 16 * n
        fh.seek(0)
        fh.write(self._header(n, movi_bytes, total, max((s for _, s in self._index), default=0)))
        fh.close()
        self._fh = None

    def write(self, data) -> None:
        """one frame: a complete JFIF file (bytes, or a uint8 array)"""
        data = memoryview(data).cast("B")
        n = len(data)
        chunk = 8 + n + (n & 1)
        if self._fh is not None and self._index and self._size + chunk + 8 + 16 * (len(self._index) + 1) > self.max_file_bytes:
            self._finish_part()
        if self._fh is None:
            self._open()
        self._fh.write(b"00dc" + struct.pack("<I", n))
        self._fh.write(data)
        if n & 1:
            self._fh.write(b"\0")
        self._index.append((self._size - self.HEADER + 4, n))
        self._size += chunk
        self.frames += 1

    def close(self) -> List[Path]:
        """finishes the last part and gives every part its name -> the files, in order"""
        if self._fh is None and not self._parts:
            self._open()                                   # (a clip without frames is still a well-formed file)
        if self._fh is not None:
            self._finish_part()
        for tmp, final in reversed(self._parts):
            os.replace(tmp, final)
        done = [final for _, final in self._parts]
        self._parts = []
        return done

    def abort(self) -> None:
        if self._fh is not None:
            self._fh.close()
            self._fh = None
        for tmp, _ in self._parts:
            if tmp.exists():
                tmp.unlink()
        self._parts = []


# ---------------------------------------------------------------------------------------------------------------- the visualizer
class Visualizer:
    """The reference's Visualizer(normal_idx, labels_csv_path, image_tmpl, save_dir, device) -- its five arguments in its order --
    and its process_video(abnormal_scores, class_probs, softmax_similarity, labels, path), which writes
    `<save_dir>/qualitatives_var/<video_name>.avi` (Motion-JPEG: see AviWriter for why not the reference's `.mp4`) unless it exists.

    decode: how the frame files are read ('pil', 'gpu', 'gpu_entropy': anomalyclip_amd/jpeg.py); quality: of the JPEG frames;
    threshold: of the border / bar colours (the reference's 0.5); canvas: (width, height), multiples of 16 -- the default is the
    reference's 12 x 8 inch figure at 100 dpi; frames_root: where the frame folders are when `path` names a feature file
    (`<frames_root>/<class>/<video>`; default: the reference's rule, path component [-3] -> `Anomaly-Frames`); batch: frames per
    launch sequence; threads: Huffman-coding workers (at most 16); max_file_bytes: where a clip continues in a `.partN.avi`;
    entropy: where the frames are Huffman-coded -- 'host' (the thread pool) or 'gpu' (acx_jpeg_entropy_encode_dev: the same files
    byte for byte, no pool; a frame whose file passes the per-frame slot goes through the host coder)."""

    def __init__(self, normal_idx, labels_csv_path, image_tmpl, save_dir, device, *, decode: str = "pil", quality: int = 90,
                 fps: float = 30, threshold: float = 0.5, canvas: Tuple[int, int] = (1200, 800), frames_root: Optional[str] = None,
                 batch: int = 32, threads: int = 8, max_file_bytes: int = 1 << 30, entropy: str = "host"):
        from .jpeg import check_decode
        self.normal_idx = int(normal_idx)
        self.labels_csv_path = labels_csv_path
        self.image_tmpl = image_tmpl
        self.save_dir = Path(save_dir)
        self.device = torch.device(device)
        self.decode = check_decode(decode)
        self.entropy = check_entropy(entropy)
        self.qtabs = quant_tables(quality)
        self.fps, self.threshold = float(fps), float(threshold)
        self.canvas = (int(canvas[0]), int(canvas[1]))
        if self.canvas[0] % 16 or self.canvas[1] % 16:
            raise ValueError(f"canvas={canvas!r}: width and height are multiples of 16 (whole MCUs of a 4:2:0 JPEG)")
        self.frames_root = frames_root
        self.batch = max(1, int(batch))
        self.threads = max(1, min(int(threads), MAX_THREADS))
        self.max_file_bytes = int(max_file_bytes)
        self.frames_written = 0        # of this object's life (measurements)
        self.bytes_to_host = 0         # of the frames' coefficients or files, likewise
        self._pin = [None, None]       # pinned, in rotation: int16 [batch, coef_elems]; entropy="gpu": uint8 [batch, cap]
        self._out: list = []           # per frame of a batch: the worker's output buffer
        self._pool: Optional[ThreadPoolExecutor] = None
        self._qt_dev = None
        self.cap = max(1 << 16, self.canvas[0] * self.canvas[1] * 3 // 4)      # bytes a frame's file rarely passes; then: a retry
        self._dev: Optional[dict] = None                                        # entropy="gpu": the device side's buffers

    # ------------------------------------------------------------------------------------------------------------ where
    def setup_directories(self, path):
        """(frame folder, <save_dir>/qualitatives_var, video name) of a test batch's `path` (visualizer.py:20-30)"""
        p = path[0] if isinstance(path, (list, tuple)) else path
        p = str(p)
        parts = os.path.normpath(p).split(os.path.sep)
        name = parts[-1][:-4] if parts[-1].endswith(".npy") else parts[-1]
        if self.frames_root is not None:
            frame_dir = os.path.join(self.frames_root, parts[-2], name) if len(parts) > 1 else os.path.join(self.frames_root, name)
        elif os.path.isdir(p):
            frame_dir = p
        else:
            if len(parts) < 3:
                raise ValueError(f"{p}: no path component [-3] to replace by 'Anomaly-Frames'; pass frames_root=")
            parts[-3], parts[-1] = "Anomaly-Frames", name
            frame_dir = os.path.sep.join(parts)
        out_dir = self.save_dir / "qualitatives_var"
        out_dir.mkdir(parents=True, exist_ok=True)
        return frame_dir, out_dir, name

    # ------------------------------------------------------------------------------------------------------------ one video
    def process_video(self, abnormal_scores, class_probs, softmax_similarity, labels, path):
        frame_dir, out_dir, name = self.setup_directories(path)
        video_path = out_dir / f"{name}.avi"
        if video_path.exists():
            return
        T = int(abnormal_scores.shape[0])
        if T == 0:
            return
        for i in range(T):
            f = os.path.join(frame_dir, self.image_tmpl.format(i))
            if not os.path.isfile(f):
                raise FileNotFoundError(f"{f}: frame {i} of {T} of the qualitative video {name} is missing")
        p = path[0] if isinstance(path, (list, tuple)) else path
        title = os.path.splitext(str(p).split("/")[-1])[0]
        writer = AviWriter(video_path, *self.canvas, fps=self.fps, max_file_bytes=self.max_file_bytes)
        try:
            self.render(frame_dir, abnormal_scores, softmax_similarity, labels, title, writer)
        except BaseException:
            writer.abort()
            raise
        writer.close()

    def _ensure(self, dev):
        if self._qt_dev is None or self._qt_dev.device != dev:
            self._qt_dev = torch.from_numpy(self.qtabs.view(np.int16).copy()).to(dev)
        n = ops.jpeg_coef_elems(self.canvas[1], self.canvas[0], 3, 2, 2)
        cap = self.cap                                                         # a frame rarely needs more; _encode retries
        while len(self._out) < self.batch:
            self._out.append(np.empty(cap, dtype=np.uint8))
        if self.entropy == "gpu":
            self._ensure_gpu(dev, n, cap)
            return
        if self._pool is None:
            self._pool = ThreadPoolExecutor(max_workers=self.threads)
        for s in (0, 1):
            if self._pin[s] is None:
                self._pin[s] = torch.empty(self.batch, n, dtype=torch.int16).pin_memory()

    def _ensure_gpu(self, dev, n: int, cap: int):
        """entropy="gpu": per slot the batch's coefficients, files, sizes and codes on the device and the files and sizes | codes in
        pinned memory; one workspace (the batches follow each other on one stream); the stream of the copies to the host"""
        d = self._dev
        if d is not None and d["device"] == dev and d["cap"] == cap:
            return
        Wc, Hc = self.canvas
        B = self.batch
        u8 = lambda *shape: torch.empty(*shape, dtype=torch.uint8, device=dev)
        self._dev = {"device": dev, "cap": cap,
                     "header": torch.from_numpy(ops.jpeg_encode_header(self.qtabs, Hc, Wc)).to(dev),
                     "coef": [torch.empty(B, n, dtype=torch.int16, device=dev) for _ in (0, 1)],
                     "files": [u8(B, cap) for _ in (0, 1)],
                     "result": [torch.empty(2, B, dtype=torch.int32, device=dev) for _ in (0, 1)],      # sizes, codes
                     "result_host": [torch.empty(2, B, dtype=torch.int32).pin_memory() for _ in (0, 1)],
                     "workspace": u8(ops.jpeg_entropy_encode_dev_workspace_bytes(Hc, Wc, B)),
                     "copies": torch.cuda.Stream(device=dev)}
        self._pin = [torch.empty(B, cap, dtype=torch.uint8).pin_memory() for _ in (0, 1)]

    def _encode_one(self, slot: int, j: int):
        """frame j of the slot's pinned coefficients -> its JFIF bytes (a view of the worker's buffer)"""
        return self._encode(self._pin[slot][j].numpy(), j)

    def _encode(self, coef: np.ndarray, j: int):
        """one frame's coefficients on the host -> its JFIF bytes (a view of buffer j)"""
        Wc, Hc = self.canvas
        n = ops.jpeg_entropy_encode(coef, self.qtabs, Hc, Wc, self._out[j])
        if n == ops.E_WORKSPACE:
            self._out[j] = np.empty(ops.jpeg_encode_bound(Hc, Wc), dtype=np.uint8)
            n = ops.jpeg_entropy_encode(coef, self.qtabs, Hc, Wc, self._out[j])
        if n < 0:
            raise L.AcxError(f"acx_jpeg_entropy_encode failed [{n}] on frame {j} of a batch")
        return self._out[j][:n]

    def _drain(self, pending, writer: AviWriter):
        slot, n, ev = pending
        if self.entropy == "gpu":
            return self._drain_gpu(slot, n, ev, writer)
        ev.synchronize()
        self.bytes_to_host += n * self._pin[slot].shape[1] * 2
        for data in self._pool.map(lambda j: self._encode_one(slot, j), range(n)):     # in frame order
            writer.write(data)
        self.frames_written += n

    def _code_batch(self, slot: int, n: int):
        """entropy="gpu", after compose_batch wrote the slot's coefficients: the device coder, and its sizes and codes on their way"""
        d = self._dev
        Wc, Hc = self.canvas
        res = d["result"][slot]
        ops.jpeg_entropy_encode_dev(d["coef"][slot][:n], d["header"], Hc, Wc, cap=d["cap"], files=d["files"][slot], nbytes=res[0],
                                    status=res[1], workspace=d["workspace"])
        d["result_host"][slot].copy_(res, non_blocking=True)

    def _drain_gpu(self, slot: int, n: int, ev, writer: AviWriter):
        """the batch's event has the sizes and codes on the host: every frame's file, its bytes only, comes over on the copies'
        stream (the main one is already busy with the next batch), then the frames are appended in order"""
        d = self._dev
        ev.synchronize()
        res = d["result_host"][slot].numpy()
        sizes, codes = res[0, :n].tolist(), res[1, :n].tolist()
        for j, code in enumerate(codes):
            if code not in (0, ops.E_WORKSPACE):
                raise L.AcxError(f"acx_jpeg_entropy_encode failed [{code}] on frame {j} of a batch")
        files, pin = d["files"][slot], self._pin[slot]
        with torch.cuda.stream(d["copies"]):
            for j in range(n):
                if codes[j] == 0:
                    pin[j, :sizes[j]].copy_(files[j, :sizes[j]], non_blocking=True)
                    self.bytes_to_host += sizes[j]
        d["copies"].synchronize()
        for j in range(n):
            if codes[j] == 0:
                writer.write(pin[j, :sizes[j]].numpy())
            else:                                          # the file passes the slot: the host coder's retry, from the coefficients
                coef = d["coef"][slot][j].cpu().numpy()
                self.bytes_to_host += coef.nbytes
                writer.write(self._encode(coef, j))
        self.frames_written += n

    def compose_batch(self, static_dev, frames, scores, softmax, idx, tables, geom, out=None):
        """the device stage of one batch: canvases uint8 [k, Hc, Wc, 3] and their coefficients int16 [k, coef_elems] (`out`, if given)"""
        canv = ops.viz_compose(static_dev, frames, scores, softmax, idx, tables, geom)
        return canv, ops.jpeg_forward(canv, self._qt_dev, out=out)

    def render(self, frame_dir: str, abnormal_scores, softmax_similarity, labels, title: str, writer: AviWriter):
        """the frames 0 ... T - 1 of `frame_dir` into `writer`: batch k + 1 is decoded, composed and transformed on the device
        while batch k is Huffman-coded on the pool and appended (entropy="gpu": coded on the device too, while batch k's files are
        copied and appended)"""
        from . import jpeg
        dev = self.device
        if dev.type != "cuda":
            raise L.AcxError("the Visualizer composes and encodes its frames on the GPU (no CPU fallback)")
        T = int(abnormal_scores.shape[0])
        scores = abnormal_scores.detach().to(dev, torch.float32).contiguous()
        softmax = softmax_similarity.detach().to(dev, torch.float32).contiguous()
        C1 = int(softmax.shape[1])
        root, video = os.path.split(os.path.normpath(frame_dir))
        reader = jpeg.make_reader(self.decode, root, video, 0, T - 1, self.image_tmpl, self.threads)
        lay = layout(self.canvas, C1, reader.frame_size, T)
        geom = geom_of(lay, self.threshold)
        names = read_class_names(self.labels_csv_path)
        static = static_layer(lay, scores.cpu().numpy(), torch.as_tensor(labels).detach().cpu().numpy(), self.normal_idx, names, title)
        with torch.cuda.device(dev):
            self._ensure(dev)
            static_dev = torch.from_numpy(static).to(dev)
            tables = resize_tables(lay, dev)
            idx = torch.arange(T, dtype=torch.int32, device=dev)
            cur = torch.cuda.current_stream(dev)
            side = torch.cuda.Stream(device=dev)
            pending, i0, k = None, 0, 0
            for slot, view in reader.batches(self.batch):
                if view.is_cuda:
                    x8 = view
                else:                                      # Pillow's frames: to the device on a side stream, as extract does
                    with torch.cuda.stream(side):
                        x8 = view.to(dev, non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(side)
                    reader.copied[slot] = ev
                    cur.wait_event(ev)
                    x8.record_stream(cur)
                n = x8.shape[0]
                part = (static_dev, x8, scores[i0:i0 + n], softmax[i0:i0 + n], idx[i0:i0 + n], tables, geom)
                if self.entropy == "gpu":
                    self.compose_batch(*part, out=self._dev["coef"][k & 1][:n])
                    self._code_batch(k & 1, n)
                else:
                    _, coef = self.compose_batch(*part)
                    self._pin[k & 1][:n].copy_(coef, non_blocking=True)
                done = torch.cuda.Event()
                done.record(cur)
                if pending is not None:
                    self._drain(pending, writer)
                pending = (k & 1, n, done)
                i0 += n
                k += 1
            if pending is not None:
                self._drain(pending, writer)
        assert i0 == T, (i0, T)

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True)
            self._pool = None
