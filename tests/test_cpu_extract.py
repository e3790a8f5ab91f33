"""CPU-only checks of the feature extractor (anomalyclip_amd/extract.py) and the multi-crop geometry of preprocess.py: the crop
windows and the sliced / mirrored coefficient tables against Pillow, the feature-file writer, the frame-folder reader and the
command line's argument errors.  No kernel is launched here."""
import ctypes as C
import os
import threading

import numpy as np
import pytest
import torch
from PIL import Image

import crops_restated as CR
from anomalyclip_amd import extract as X
from anomalyclip_amd import preprocess as P


@pytest.mark.parametrize("geom", CR.GEOMETRIES)
@pytest.mark.parametrize("ncrops", [1, 5, 10])
def test_crop_windows_match_pillow(geom, ncrops):
    h, w, scale, crop = geom
    assert P.crop_windows(h, w, scale, crop, ncrops) == CR.pil_windows(h, w, scale, crop, ncrops)


def test_mirrored_centre_is_one_column_off_when_the_margin_is_odd():
    """241 x 323 -> 256 x 343: ow - C = 119 is odd; the centre of the mirrored image sits one column right of the plain centre"""
    wins = P.crop_windows(241, 323, 256, 224, 10)
    oh, ow = P.scaled_size(241, 323, 256)
    assert (ow - 224) % 2 == 1
    (t0, l0, f0), (t1, l1, f1) = wins[4], wins[9]
    assert (f0, f1) == (False, True) and t0 == t1 and l1 == ow - 224 - l0 and abs(l1 - l0) == 1
    even = P.crop_windows(240, 320, 256, 224, 10)           # 341 - 224 = 117 is odd as well; 224 x 224 has no margin at all
    assert P.crop_windows(224, 224, 224, 224, 10)[4][:2] == P.crop_windows(224, 224, 224, 224, 10)[9][:2] == (0, 0)
    assert len(even) == 10 and [f for _, _, f in even] == [False] * 5 + [True] * 5


def test_crop_windows_errors_and_defaults():
    with pytest.raises(ValueError, match="ncrops"):
        P.crop_windows(240, 320, 256, 224, 3)
    with pytest.raises(ValueError, match="scale_size"):
        P.crop_windows(240, 320, 200, 224, 5)
    assert [P.default_scale_size(c, 5) for c in (224, 336, 32)] == [256, 384, 36]
    assert P.default_scale_size(224, 1) == 224 and P.default_scale_size(336, 10) == 384
    # one crop at scale == crop is resize_geometry's centre crop
    for h, w in ((240, 320), (360, 201), (224, 224)):
        oh, ow, top, left = P.resize_geometry(h, w, 224)
        assert P.crop_windows(h, w, 224, 224, 1) == [(top, left, False)] and P.scaled_size(h, w, 224) == (oh, ow)


@pytest.mark.parametrize("geom", CR.GEOMETRIES)
@pytest.mark.parametrize("ncrops", [1, 5, 10])
def test_sliced_and_mirrored_tables_equal_pillow_pixels(geom, ncrops):
    h, w, scale, crop = geom
    frame = CR.make_frames(h, w, 1, seed=ncrops)[0].numpy()
    frame[h // 2:, : w // 2] = 0                              # (flat black beside flat white beside noise)
    assert np.array_equal(CR.table_crops(frame, scale, crop, ncrops), CR.pil_crops(frame, scale, crop, ncrops))


def test_abi_rejects_bad_crop_arguments():
    """validation happens before any launch: ncrops outside {1, 5, 10}, scale_size < crop, a window outside the image"""
    from anomalyclip_amd import _lib as L
    lib = L.lib()
    buf = (C.c_int32 * 64)()
    p = C.addressof(buf)
    m = (C.c_float * 3)(0, 0, 0)
    win = (C.c_int32 * 30)()

    def call(oh, ow, crop, ncrops, F=1):
        return lib.acx_preprocess_crops(None, p, p, p, p, p, 5, p, p, 5, F, 240, 320, oh, ow, crop, ncrops, win, m, m, None)
    assert call(256, 341, 224, 3) == -1 and b"ncrops" in lib.acx_last_error(None)
    assert call(200, 266, 224, 5) == -1 and b"scale_size" in lib.acx_last_error(None)
    win[1] = 118                                                   # left + crop > ow
    assert call(256, 341, 224, 5) == -1 and b"window" in lib.acx_last_error(None)
    win[1] = 0
    assert lib.acx_preprocess_crops(None, None, p, p, p, p, 5, p, p, 5, 1, 240, 320, 256, 341, 224, 5, win, m, m, None) == -1
    assert call(256, 341, 224, 5, F=0) == 0                        # empty work is a no-op


# ---------------------------------------------------------------------------------------------------------------- writer
def test_writer_layout_atomic_replace_skip_and_stale_tmp(tmp_path):
    T, ncrops, D = 7, 5, 16
    rows = np.arange(T * ncrops * D, dtype=np.float32).reshape(T * ncrops, D)
    out = str(tmp_path / "sub" / "vid")                             # no suffix: `.npy` is appended; folders are made
    stale = out + ".npy.tmp"
    os.makedirs(os.path.dirname(out))
    open(stale, "wb").write(b"half a file")
    assert not X.is_complete(out, rows.shape)                       # a leftover .tmp alone is not a file
    p = X.write_features(out, rows)
    assert p == out + ".npy" and not os.path.exists(stale)
    got = np.load(p, allow_pickle=False)
    assert got.dtype == np.float32 and np.array_equal(got, rows)
    t, c = 3, 2
    assert np.array_equal(got.reshape(T, ncrops, D)[t, c], rows[t * ncrops + c])     # feature_dataset.py:347's view
    from anomalyclip_amd.feature_stream import FeatureStream
    with open(p, "rb") as fh:                                        # the header FeatureStream reads its geometry from
        assert FeatureStream._npy_header(fh)[0] == (T * ncrops, D)
    assert X.is_complete(out, rows.shape) and X.is_complete(p, rows.shape)
    assert not X.is_complete(out, (T * ncrops + 1, D)) and not X.is_complete(out, (T * ncrops, D + 1))
    np.save(p, rows.astype(np.float64))
    assert not X.is_complete(out, rows.shape)                       # another dtype is not complete either
    open(p, "wb").write(b"\x93NUMPY")                              # a truncated header
    assert not X.is_complete(out, rows.shape)


def test_writer_replaces_in_one_step(tmp_path, monkeypatch):
    """the final name only ever appears through os.replace of the finished .tmp"""
    out = str(tmp_path / "v.npy")
    X.write_features(out, np.zeros((4, 8), np.float32))
    seen = []
    real = os.replace

    def spy(src, dst):
        seen.append((src, dst, np.load(src).shape, np.load(dst).shape))
        return real(src, dst)
    monkeypatch.setattr(os, "replace", spy)
    X.write_features(out, np.ones((6, 8), np.float32))
    assert seen == [(out + ".tmp", out, (6, 8), (4, 8))]
    assert np.load(out).shape == (6, 8)


# ---------------------------------------------------------------------------------------------------------------- reader
def _write_frames(folder, indices, hw=(12, 16), ext="jpg", template="{:06d}.jpg", seed=0):
    os.makedirs(folder, exist_ok=True)
    rng = np.random.default_rng(seed)
    frames = {}
    for i in indices:
        a = rng.integers(0, 256, (hw[0], hw[1], 3), dtype=np.uint8)
        Image.fromarray(a).save(os.path.join(folder, template.format(i)), quality=95)
        frames[i] = a
    return frames


def test_annotation_rows(tmp_path):
    f = tmp_path / "anno.txt"
    f.write_text("Abuse/Abuse001_x264 0 99 1\n\nNormal/N_002 5 17 7 3 4\n")
    assert X.read_annotations(str(f)) == [("Abuse/Abuse001_x264", 0, 99), ("Normal/N_002", 5, 17)]
    f.write_text("a 0 9\n")
    with pytest.raises(ValueError, match="path start end label"):
        X.read_annotations(str(f))


def test_reader_inclusive_range_template_and_order(tmp_path):
    root = str(tmp_path)
    _write_frames(os.path.join(root, "v"), range(0, 12))
    open(os.path.join(root, "v", "notes.txt"), "w").write("x")
    open(os.path.join(root, "v", "0000010.jpg"), "w").write("x")          # seven digits: not the template's name for frame 10
    Image.new("RGB", (16, 12)).save(os.path.join(root, "v", "000003.png"))
    r = X.FrameFolderReader(root, "v", 3, 9, pinned=False)
    assert len(r) == 7 and r.path(0).endswith("000003.jpg") and r.path(6).endswith("000009.jpg")       # end inclusive
    allf = X.FrameFolderReader(root, "v", pinned=False)
    assert allf.indices == list(range(12)) and allf.frame_size == (12, 16)
    assert X.TEMPLATE == "{:06d}.jpg"
    got = [v.clone() for _, v in r.batches(3)]
    assert [g.shape[0] for g in got] == [3, 3, 1] and got[0].dtype == torch.uint8
    want = np.stack([np.asarray(Image.open(r.path(i)).convert("RGB")) for i in range(7)])
    assert np.array_equal(torch.cat(got).numpy(), want)
    slots = [s for s, _ in X.FrameFolderReader(root, "v", pinned=False).batches(5)]
    assert slots == [0, 1, 0]                                              # two buffers in rotation
    _write_frames(os.path.join(root, "w"), (1, 2), template="img_{:05d}.jpg")
    assert X.FrameFolderReader(root, "w", template="img_{:05d}.jpg", pinned=False).indices == [1, 2]
    assert X.list_videos(root) == ["v"]
    with pytest.raises(ValueError, match="no frames"):
        X.FrameFolderReader(root, "w", pinned=False)


def test_reader_size_mismatch_names_the_file(tmp_path):
    root = str(tmp_path)
    _write_frames(os.path.join(root, "v"), range(6))
    Image.new("RGB", (20, 12)).save(os.path.join(root, "v", "000004.jpg"))
    with pytest.raises(ValueError, match=r"000004\.jpg.*12 x 20.*12 x 16"):
        list(X.FrameFolderReader(root, "v", pinned=False).batches(4))


def test_decode_pool_holds_at_most_16_threads(tmp_path, monkeypatch):
    root = str(tmp_path)
    _write_frames(os.path.join(root, "v"), range(64), hw=(8, 8))
    monkeypatch.setattr(os, "cpu_count", lambda: 1 / 0)                    # never asked
    r = X.FrameFolderReader(root, "v", threads=500, pinned=False)
    assert r.threads == 16 == X.MAX_DECODE_THREADS
    seen, lock = set(), threading.Lock()
    real = r._decode

    def spy(i, dst):
        with lock:
            seen.add(threading.get_ident())
        return real(i, dst)
    r._decode = spy
    pool = r.pool()
    assert pool._max_workers == 16
    assert sum(v.shape[0] for _, v in r.batches(64)) == 64
    assert 1 <= len(seen) <= 16
    assert X.FrameFolderReader(root, "v", pinned=False).threads == 8 and X.FrameFolderReader(root, "v", threads=0, pinned=False).threads == 1


# ---------------------------------------------------------------------------------------------------------------- command line
def _cli(argv, capsys):
    with pytest.raises(SystemExit) as e:
        X.parse_args(argv)
    return e.value.code, capsys.readouterr().err


def test_command_line_argument_errors(tmp_path, capsys):
    w = tmp_path / "w.pt"
    w.write_bytes(b"")
    base = ["--arch", "ViT-B/16", "--weights", str(w), "--frames-root", str(tmp_path), "--out-root", str(tmp_path / "o")]
    a = X.parse_args(base + ["--ncrops", "5"])
    assert (a.arch, a.ncrops, a.scale_size, a.precision, a.overwrite, a.annotations) == ("ViT-B/16", 5, None, "auto", False, None)
    code, err = _cli(base + ["--bogus", "1"], capsys)
    assert code == 2 and "unrecognized arguments: --bogus 1" in err
    code, err = _cli(base + ["--ncrops", "3"], capsys)
    assert code == 2 and "--ncrops" in err and "invalid choice: 3" in err
    code, err = _cli(base + ["--scale-size", "200"], capsys)
    assert code == 2 and "--scale-size 200 conflicts with --arch ViT-B/16" in err
    code, err = _cli(base[:2] + base[4:], capsys)
    assert code == 2 and "--weights" in err and "required" in err
    rn = ["--arch", "RN50"] + base[2:]
    code, err = _cli(rn + ["--precision", "bf16"], capsys)
    assert code == 2 and "--precision bf16 conflicts with --arch RN50" in err
    code, err = _cli(["--arch", "ViT-Z/1"] + base[2:], capsys)
    assert code == 2 and "--arch" in err and "ViT-Z/1" in err
    code, err = _cli(base + ["--annotations", str(tmp_path / "missing.txt")], capsys)
    assert code == 2 and "--annotations" in err and "missing.txt" in err


def test_encoder_weights_of_another_arch_are_refused():
    from anomalyclip_amd import init_weights as IW
    enc = X.build_image_encoder("tiny", "f32")
    sd = IW.init_vit_state_dict(IW.TINY, 3, prefix="")
    X.load_encoder_weights(enc, "tiny", sd)                                              # the encoder's own keys
    X.load_encoder_weights(enc, "tiny", {"state_dict": {"net.image_encoder." + k: v.half() for k, v in sd.items()}})
    assert torch.equal(enc.proj.detach(), sd["proj"].half().float())
    with pytest.raises(ValueError, match="do not match arch 'ViT-B/32'"):
        X.load_encoder_weights(X.build_image_encoder("tiny"), "ViT-B/32", sd)
