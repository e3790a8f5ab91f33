"""CPU-only checks of the qualitative videos' host half: the JPEG entropy encoder against the project's own parser and decoder and
against Pillow, the quantisation tables against the ones Pillow writes, the Motion-JPEG AVI container, and the layout.  No kernel is
launched here."""
import ctypes as C
import io
import os

import numpy as np
import pytest
import torch
from PIL import Image

import viz_ref as R
from anomalyclip_amd import _lib as L
from anomalyclip_amd import jpeg, ops
from anomalyclip_amd import visualizer as V

E_WORKSPACE = -4
SIZES = [(16, 16), (32, 48), (800, 1200)]                         # (H, W): 16x16, 48x32 and 1200x800 as width x height


def encode(coef, qt, H, W, cap=None):
    buf = np.full((ops.jpeg_encode_bound(H, W) if cap is None else cap) + 64, 0xA5, np.uint8)      # 64 guard bytes behind the buffer
    n = ops.jpeg_entropy_encode(coef, qt, H, W, buf[:len(buf) - 64])
    assert bool((buf[len(buf) - 64:] == 0xA5).all()), "written past the end of the buffer"
    return n, buf


# ====================================================================================================== entropy round trip
@pytest.mark.parametrize("H,W", SIZES)
def test_entropy_round_trip(H, W):
    qt = V.quant_tables(90)
    stuffed = False
    for name, coef in R.entropy_cases(H, W):
        n, buf = encode(coef, qt, H, W)
        assert n > 0, (name, n)
        data = buf[:n].tobytes()
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        rc, info = jpeg.parse(data)
        assert rc == 0, (name, rc)
        assert jpeg.geometry_of(info) == (H, W, 3, 2, 2), name                    # inside the device decoder's baseline set
        assert int(info.coef_elems) == coef.size == R.coef_elems(H, W) and int(info.restart_interval) == 0
        for t in range(2):
            assert np.array_equal(np.ctypeslib.as_array(info.qtab[t]), qt[t]), name
        back = np.zeros(coef.size, np.int16)
        assert L.lib().acx_jpeg_entropy_decode(data, len(data), C.byref(info), back.ctypes.data, back.size) == 0, name
        assert np.array_equal(back, coef), name
        stuffed |= b"\xff\x00" in data[int(info.scan_offset):]
        im = Image.open(io.BytesIO(data))
        im.load()                                                                  # Pillow opens and fully decodes it
        assert im.size == (W, H) and im.mode == "RGB", name
        # one byte short: ACX_E_WORKSPACE, nothing behind the buffer touched (encode() checks the guard)
        short, _ = encode(coef, qt, H, W, cap=n - 1)
        assert short == E_WORKSPACE, (name, short)
        exact, buf2 = encode(coef, qt, H, W, cap=n)
        assert exact == n and buf2[:n].tobytes() == data
    assert stuffed, "no case produced an FF byte in its scan"


def test_entropy_encoder_covers_every_edge_block():
    """the cases hold what the issue lists: coefficient 63 alone, every zero run 16 ... 62, AC +-1023, DC differences of category 11"""
    names = [n for n, _ in R.edge_blocks()]
    assert names[0].startswith("only coefficient 63") and [f"zero run {r}" for r in range(16, 63)] == names[1:48]
    assert "AC 1023" in names and "AC -1023" in names
    for H, W in SIZES:
        cases = dict(R.entropy_cases(H, W))
        covered = sum(c.reshape(-1, 64).any(1).sum() for n, c in cases.items() if n.startswith("edge blocks"))
        assert covered == len(names), (H, W)
        dc = cases["DC differences of category 11"].reshape(-1, 64)[:, 0].astype(int)
        assert set(np.abs(np.diff(dc))) == {2046} and set(np.sign(np.diff(dc))) == {1, -1}


def test_entropy_encoder_refusals():
    qt = V.quant_tables(75)
    n = R.coef_elems(16, 16)
    buf = np.zeros(ops.jpeg_encode_bound(16, 16), np.uint8)
    ok = np.zeros(n, np.int16)
    assert ops.jpeg_entropy_encode(ok, qt, 16, 16, buf) > 0
    assert ops.jpeg_entropy_encode(ok[:-64], qt, 16, 16, buf) == -1                # not the frame's coefficient count
    bad = ok.copy()
    bad[5] = 1024                                                                  # an AC value the tables cannot code
    assert ops.jpeg_entropy_encode(bad, qt, 16, 16, buf) == -1
    bad = ok.copy()
    bad[0], bad[64] = 2000, -2000                                                  # a DC difference of category 12
    assert ops.jpeg_entropy_encode(bad, qt, 16, 16, buf) == -1
    q0 = qt.copy()
    q0[1, 7] = 0
    assert ops.jpeg_entropy_encode(ok, q0, 16, 16, buf) == -1
    assert L.lib().acx_jpeg_encode_bound(0, 16) == -1 and L.lib().acx_jpeg_encode_bound(16, 70000) == -1
    assert ops.jpeg_entropy_encode(ok, qt, 16, 16, np.zeros(0, np.uint8)) == E_WORKSPACE


# ====================================================================================================== quantisation tables
@pytest.mark.parametrize("quality", [1, 50, 75, 90, 100])
def test_quant_tables_equal_pillows(quality):
    buf = io.BytesIO()
    Image.fromarray(np.random.default_rng(quality).integers(0, 256, (32, 32, 3), dtype=np.uint8)).save(buf, "JPEG", quality=quality,
                                                                                                         subsampling=2)
    data = buf.getvalue()
    ours = V.quant_tables(quality)
    assert ours.dtype == np.uint16 and ours.shape == (2, 64)
    rc, info = jpeg.parse(data)                                                    # the project's parser: natural order
    assert rc == 0
    for t in range(2):
        assert np.array_equal(np.ctypeslib.as_array(info.qtab[t]), ours[t]), (quality, t)
    # Pillow's own reading of the file: `quantization` is in natural order since Pillow 8.3, in the file's zigzag order before
    q = Image.open(io.BytesIO(data)).quantization
    for t in range(2):
        got = np.array(q[t], dtype=np.uint16)
        assert np.array_equal(got, ours[t]) or np.array_equal(got, ours[t][R.NATURAL]), (quality, t)
    with pytest.raises(ValueError, match="quality"):
        V.quant_tables(0)


# ====================================================================================================== container
def jpeg_frames(n, size=(32, 16), seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        buf = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (size[1], size[0], 3), dtype=np.uint8)).save(buf, "JPEG", quality=60 + (i % 3) * 15)
        out.append(buf.getvalue())
    return out


def check_part(path, frames, size):
    data = open(path, "rb").read()
    a = R.walk_avi(data)
    assert a["avih_frames"] == a["strh_length"] == len(a["frames"]) == len(a["index"]) == len(frames)
    assert (a["width"], a["height"]) == size and a["handler"] == b"MJPG" and a["rate"] == 30
    assert a["frames"] == list(frames)
    for (off, size_), (at, csize), payload in zip(a["index"], a["chunks"], a["frames"]):
        assert a["movi"] + off == at and size_ == csize == len(payload)            # every idx1 offset points at its chunk
        assert data[a["movi"] + off:a["movi"] + off + 4] == b"00dc"
        im = Image.open(io.BytesIO(payload))
        im.load()
        assert im.size == size
    return a


def test_avi_one_file(tmp_path):
    frames = jpeg_frames(7)
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)          # odd sizes are padded to even
    w = V.AviWriter(tmp_path / "clip.avi", 32, 16, fps=30)
    for f in frames[:3]:
        w.write(f)
    assert not (tmp_path / "clip.avi").exists()                                    # under a temporary name until close()
    for f in frames[3:]:
        w.write(np.frombuffer(f, np.uint8))
    assert w.close() == [tmp_path / "clip.avi"] and w.frames == 7
    assert sorted(os.listdir(tmp_path)) == ["clip.avi"]
    check_part(tmp_path / "clip.avi", frames, (32, 16))


def test_avi_parts(tmp_path):
    frames = jpeg_frames(11, seed=3)
    limit = V.AviWriter.HEADER + 3 * (max(map(len, frames)) + 8 + 16) + 64         # about three frames per part
    w = V.AviWriter(tmp_path / "long.avi", 32, 16, max_file_bytes=limit)
    for f in frames:
        w.write(f)
    parts = w.close()
    assert len(parts) >= 3 and parts[0] == tmp_path / "long.avi"
    assert parts[1:] == [tmp_path / f"long.part{k}.avi" for k in range(1, len(parts))]
    assert sorted(os.listdir(tmp_path)) == sorted(p.name for p in parts)
    got = []
    for p in parts:
        assert os.path.getsize(p) <= limit
        n = len(R.walk_avi(open(p, "rb").read())["frames"])
        check_part(p, frames[len(got):len(got) + n], (32, 16))
        got += frames[len(got):len(got) + n]
    assert got == frames                                                           # every frame once, in order


def test_avi_abort_leaves_nothing(tmp_path):
    w = V.AviWriter(tmp_path / "x.avi", 32, 16)
    w.write(jpeg_frames(1)[0])
    w.abort()
    assert os.listdir(tmp_path) == []


def test_process_video_skips_an_existing_output(tmp_path):
    """the output is there: process_video returns without opening a frame (there is none) and without touching the file"""
    viz = V.Visualizer(7, None, "{:06d}.jpg", tmp_path, "cpu", frames_root=str(tmp_path / "no_such_frames"))
    out = tmp_path / "qualitatives_var"
    out.mkdir()
    (out / "v0.avi").write_bytes(b"kept")
    args = (torch.zeros(5), torch.zeros(5, 13), torch.zeros(5, 13), torch.zeros(5, dtype=torch.long))
    assert viz.process_video(*args, [str(tmp_path / "features" / "Arson" / "v0.npy")]) is None
    assert (out / "v0.avi").read_bytes() == b"kept"
    with pytest.raises(FileNotFoundError, match=r"no_such_frames/Arson/v1/000000\.jpg"):   # and a missing frame is named
        viz.process_video(*args, [str(tmp_path / "features" / "Arson" / "v1.npy")])
    assert sorted(os.listdir(out)) == ["v0.avi"]


def test_setup_directories(tmp_path):
    viz = V.Visualizer(7, None, "{:06d}.jpg", tmp_path, "cpu")
    d, out, name = viz.setup_directories(["/data/ucf/Features/Arson/Arson011_x264.npy"])   # the reference's rule
    assert (d, name) == ("/data/ucf/Anomaly-Frames/Arson/Arson011_x264", "Arson011_x264") and out == tmp_path / "qualitatives_var"
    folder = tmp_path / "frames" / "test" / "t0"
    folder.mkdir(parents=True)
    assert viz.setup_directories([str(folder)])[::2] == (str(folder), "t0")                # frames mode: the folder as it is
    viz = V.Visualizer(7, None, "{:06d}.jpg", tmp_path, "cpu", frames_root="/frames")
    assert viz.setup_directories(["/feat/test/t1.npy"])[::2] == ("/frames/test/t1", "t1")
    with pytest.raises(ValueError, match="multiples of 16"):
        V.Visualizer(7, None, "{:06d}.jpg", tmp_path, "cpu", canvas=(1210, 800))
    with pytest.raises(ValueError, match="decode"):
        V.Visualizer(7, None, "{:06d}.jpg", tmp_path, "cpu", decode="cv2")


# ====================================================================================================== layout
def _inside(r, Wc, Hc):
    return 0 < r[0] < r[2] < Wc and 0 < r[1] < r[3] < Hc


def _disjoint(a, b):
    return a[2] <= b[0] or b[2] <= a[0] or a[3] <= b[1] or b[3] <= a[1]


@pytest.mark.parametrize("canvas", [(1200, 800), (320, 240)])
@pytest.mark.parametrize("source", [(240, 320), (720, 1280), (320, 240), (29, 37)])       # (H, W) of 320x240, 1280x720, 240x320, 37x29
@pytest.mark.parametrize("C1", [1, 13, 64])
def test_layout(canvas, source, C1):
    T = 50
    lay = V.layout(canvas, C1, source, T)
    Wc, Hc = canvas
    H, W = source
    panels = [lay["frame_panel"], lay["bars_panel"], lay["score_panel"]]
    bars = [V.bar_rect(lay, k, lay["bars_panel"][3] - lay["bars_panel"][1]) for k in range(C1)]
    for r in panels + [lay["frame"], lay["frame_outer"]] + bars:
        assert _inside(r, Wc, Hc), r
    for i in range(3):
        for j in range(i + 1, 3):
            assert _disjoint(panels[i], panels[j])
    f, o, p = lay["frame"], lay["frame_outer"], lay["frame_panel"]
    assert o == (f[0] - 5, f[1] - 5, f[2] + 5, f[3] + 5) and p[0] <= o[0] and p[1] <= o[1] and o[2] <= p[2] and o[3] <= p[3]
    fw, fh = f[2] - f[0], f[3] - f[1]
    assert abs(fw - W * fh / H) <= 1 or abs(fh - H * fw / W) <= 1                   # the aspect ratio, to within one pixel
    assert fw == p[2] - p[0] - 10 or fh == p[3] - p[1] - 10                         # one side fills the panel
    assert abs((o[0] - p[0]) - (p[2] - o[2])) <= 1 and abs((o[1] - p[1]) - (p[3] - o[3])) <= 1     # centred
    for a, b in zip(bars, bars[1:]):
        assert a[2] <= b[0]
    assert lay["bars_panel"][0] <= bars[0][0] and bars[-1][2] <= lay["bars_panel"][2]
    sp = lay["score_panel"]
    xs = [V.cursor_x(lay, i) for i in range(T)]
    assert xs[0] == sp[0] and xs == sorted(xs) and xs[-1] + lay["cursor_w"] <= sp[2]
    g = V.geom_of(lay, 0.5)
    assert (g.Wc, g.Hc, g.H, g.W, g.C1, g.T) == (Wc, Hc, H, W, C1, T) and (g.fw, g.fh, g.border, g.cursor_w) == (fw, fh, 5, 2)
    # the static layer is drawn from the same rectangles and leaves the device's pixels alone where nothing is drawn yet
    layer = V.static_layer(lay, np.linspace(0, 1, T), np.r_[np.zeros(20), np.ones(10), np.zeros(20)] * 3 + 7 * 0, 0,
                           [f"class{k}" for k in range(C1)], "title")
    assert layer.shape == (Hc, Wc, 3) and layer.dtype == np.uint8 and (layer != 255).any()


def test_layout_refusals():
    with pytest.raises(ValueError, match="C1"):
        V.layout((1200, 800), 65, (240, 320), 10)
    with pytest.raises(ValueError, match="canvas"):
        V.layout((64, 48), 13, (240, 320), 10)
