"""CPU-only: the host half of the JPEG decoder (acx_jpeg_parse + acx_jpeg_entropy_decode, anomalyclip_amd/csrc/acx_jpeg_host.h)
through ctypes, followed by the numpy restatement of the device half (tests/jpeg_restated.py), against Pillow -- equal bytes pin
both at once.  Then what the decoder refuses, what it survives (truncated and corrupted files, guard words around its output, a
sanitizer build of the header as a stand-alone program), and the `decode` switch of the four Python entry points."""
import io
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
from PIL import Image

import jpeg_restated as JR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADARG, E_UNSUPPORTED = 0, -1, -2


def _equal_to_pillow(data: bytes):
    rc, geom, coef, qt = JR.host_decode(data, guard=64)
    assert rc == OK, rc
    ref = JR.pillow_rgb(data)
    assert (geom["H"], geom["W"]) == ref.shape[:2]
    got = JR.reconstruct(geom, coef, qt)
    assert np.array_equal(got, ref), f"{int((got != ref).sum())} bytes differ"
    return geom, qt


@pytest.fixture(scope="module")
def grid():
    return JR.grid_cases()


def test_grid_equals_pillow(grid):
    """5 sizes x (4:4:4, 4:2:2, 4:2:0, greyscale) x quality 30 / 75 / 95 / 100 x noise 0 / 25 / 120, and one 240 x 320 image"""
    assert len(grid) == 5 * 4 * 4 * 3
    seen = set()
    for name, data in grid:
        geom, _ = _equal_to_pillow(data)
        seen.add((geom["ncomp"], geom["hs"], geom["vs"]))
    assert seen == {(3, 1, 1), (3, 2, 1), (3, 2, 2), (1, 1, 1)}
    geom, _ = _equal_to_pillow(JR.save_jpeg(JR.make_image(240, 320, 25, seed=5), 75, 2))
    assert geom["blocks"] == [(30, 40), (15, 20), (15, 20)] and geom["coef_elems"] == 1800 * 64


@pytest.mark.parametrize("kw", [dict(restart_marker_blocks=1), dict(restart_marker_blocks=3), dict(restart_marker_rows=1),
                                dict(restart_marker_rows=2)])
@pytest.mark.parametrize("mode", [0, 1, 2, "L"])
def test_restart_intervals(kw, mode):
    a = JR.make_image(45, 67, 25, seed=11, grey=(mode == "L"))
    plain = JR.save_jpeg(a, 75, None if mode == "L" else mode)
    data = JR.save_jpeg(a, 75, None if mode == "L" else mode, **kw)
    geom, _ = _equal_to_pillow(data)
    assert data != plain, "Pillow wrote no restart markers"
    assert geom["restart_interval"] > 0 and any(bytes([0xFF, 0xD0 + k]) in data for k in range(8))


def _dqt_as_16_bit(data: bytes) -> bytes:
    """the same file with every DQT segment rewritten with 16-bit entries (Pq = 1), the values unchanged"""
    out, p = bytearray(data[:2]), 2
    while data[p + 1] != 0xDA:
        n = int.from_bytes(data[p + 2:p + 4], "big")
        seg = data[p + 4:p + 2 + n]
        if data[p + 1] == 0xDB:
            body = bytearray()
            for q in range(0, len(seg), 65):
                assert seg[q] >> 4 == 0
                body += bytes([0x10 | seg[q]]) + b"".join(bytes([0, v]) for v in seg[q + 1:q + 65])
            out += b"\xff\xdb" + (len(body) + 2).to_bytes(2, "big") + body
        else:
            out += data[p:p + 2 + n]
        p += 2 + n
    return bytes(out + data[p:])


def test_sixteen_bit_and_coarse_quantisation_tables():
    """Pillow clamps the tables it writes to 8 bits (a `qtables=` entry of 1000 comes back as 255), so the 16-bit DQT form is made
    by rewriting the segments of a Pillow file; quality 1 is the coarsest table Pillow makes"""
    a = JR.make_image(33, 31, 25, seed=3)
    data = JR.save_jpeg(a, 75, 2, qtables=[[min(1000, 16 + 40 * k) for k in range(64)]] * 2)
    _, qt = _equal_to_pillow(data)
    assert int(qt.max()) == 255
    wide = _dqt_as_16_bit(data)
    assert len(wide) == len(data) + 128 and np.array_equal(JR.pillow_rgb(wide), JR.pillow_rgb(data))
    _, qt16 = _equal_to_pillow(wide)
    assert np.array_equal(qt16, qt)
    _, qt = _equal_to_pillow(JR.save_jpeg(a, 1, 2))
    assert int(qt.max()) == 255
    _equal_to_pillow(JR.save_jpeg(JR.make_image(17, 23, 120, seed=4, grey=True), 1))


def _unsupported_files():
    """progressive and CMYK as Pillow writes them; 4:1:1 (luma sampled 4 x 1) is nothing Pillow writes -- its "4:1:1" is an alias
    of 4:2:0 -- so the frame header of a 4:2:2 file is rewritten to say so (the header is all acx_jpeg_parse judges by)"""
    a = JR.make_image(45, 67, 25, seed=21)
    cmyk = io.BytesIO()
    Image.fromarray(a).convert("CMYK").save(cmyk, "JPEG", quality=75)
    f411 = bytearray(JR.save_jpeg(a, 75, 1))
    sof = f411.index(b"\xff\xc0")
    assert f411[sof + 11] == 0x21
    f411[sof + 11] = 0x41
    return {"progressive": JR.save_jpeg(a, 75, 2, progressive=True), "cmyk": cmyk.getvalue(), "411": bytes(f411)}


@pytest.mark.parametrize("hw", [(16, 3), (16, 4), (4, 4), (1, 3), (16, 2), (16, 1)])
@pytest.mark.parametrize("sub", [1, 2])
def test_narrow_subsampled_frames_are_left_to_pillow(hw, sub):
    """libjpeg-turbo filters a chroma plane only above two samples per row and replicates below: frames up to 4 pixels wide at
    4:2:2 / 4:2:0 are ACX_E_UNSUPPORTED (the recipe gives 24 ... 175 other bytes on them); width 5 is the first that is taken,
    and 4:4:4 and greyscale are taken at any width"""
    a = JR.make_image(hw[0], hw[1], 25, seed=hw[0] * hw[1])
    assert JR.host_decode(JR.save_jpeg(a, 90, sub))[0] == E_UNSUPPORTED
    _equal_to_pillow(JR.save_jpeg(a, 90, 0))
    _equal_to_pillow(JR.save_jpeg(a[..., 0].copy(), 90))
    for w in (5, 6):
        _equal_to_pillow(JR.save_jpeg(JR.make_image(hw[0], w, 25, seed=w), 90, sub))


@pytest.mark.parametrize("kind", ["progressive", "cmyk", "411"])
def test_unsupported_files_are_reported(kind):
    data = _unsupported_files()[kind]
    if kind != "411":
        assert JR.pillow_rgb(data).shape == (45, 67, 3)          # Pillow reads it: the reader's fallback has something to give
    assert JR.host_decode(data)[0] == E_UNSUPPORTED
    assert JR.host_decode(b"")[0] == E_BADARG and JR.host_decode(b"\x89PNG\r\n\x1a\n" + bytes(64))[0] == E_BADARG


def _damaged(data: bytes):
    """the file cut at 40 evenly spaced lengths, and 40 copies with 1 ... 4 seeded bit flips inside the scan"""
    out = [data[: len(data) * k // 40] for k in range(40)]
    scan = data.rindex(b"\xff\xda")
    rng = np.random.default_rng(99)
    for k in range(40):
        b = bytearray(data)
        for _ in range(1 + k % 4):
            b[int(rng.integers(scan + 14, len(data)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b))
    return out


@pytest.mark.parametrize("mode", [2, "L"])
def test_truncated_and_corrupted_files_end_in_a_code(mode):
    a = JR.make_image(45, 67, 25, seed=31, grey=(mode == "L"))
    data = JR.save_jpeg(a, 75, None if mode == "L" else mode, restart_marker_blocks=4)
    codes = [JR.host_decode(d, guard=256)[0] for d in _damaged(data)]          # (host_decode asserts the guard words)
    assert set(codes) <= {OK, E_BADARG, E_UNSUPPORTED}, set(codes)
    assert all(c != OK for c in codes[:39])                      # a file cut before its last fortieth has lost scan data


def test_sanitizer_build_of_the_host_decoder(tmp_path):
    """tools/jpeg_host_check.cpp (its own main; nothing preloaded, nothing loaded into Python) under AddressSanitizer and
    UndefinedBehaviorSanitizer: whole files, their truncations and seeded bit flips, from exact-size heap copies"""
    clang = next((c for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(c)), None)
    assert clang is not None, "the ROCm clang++ that builds the library is missing"
    exe = str(tmp_path / "jpeg_host_check")
    r = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tools", "jpeg_host_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = []
    cases = {f"ok_{m}_{q}": JR.save_jpeg(JR.make_image(45, 67, 25, seed=41, grey=(m == "L")), q, None if m == "L" else m)
             for m in (0, 1, 2, "L") for q in (30, 100)}
    cases["ok_restart"] = JR.save_jpeg(JR.make_image(33, 31, 120, seed=42), 75, 2, restart_marker_blocks=2)
    cases.update({f"unsupported_{k}": v for k, v in _unsupported_files().items()})
    for name, data in cases.items():
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(data)
        files.append(str(p))
    r = subprocess.run([exe, *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]


# ---------------------------------------------------------------------------------------------------------------- the switch
def test_decode_switch_is_checked_at_every_entry_point(tmp_path):
    """anything but "pil" or "gpu" is a ValueError naming the key, before a frame or the GPU is touched"""
    from anomalyclip_amd import extract as X
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    from anomalyclip_amd.feature_bank import FeatureBank
    enc = SimpleNamespace(output_dim=32)
    rec = [SimpleNamespace(video="v", start_frame=0, end_frame=3, label=0)]
    with pytest.raises(ValueError, match="decode="):
        X.extract_video(enc, np.zeros((1, 8, 8, 3), np.uint8), str(tmp_path / "x"), decode="nonsense")
    with pytest.raises(ValueError, match="decode="):
        X.extract_dataset(enc, None, str(tmp_path), str(tmp_path / "out"), decode="nonsense")
    with pytest.raises(ValueError, match="decode="):
        FeatureBank.from_frames(enc, rec, str(tmp_path), max_bytes=1 << 30, decode="nonsense")
    with pytest.raises(ValueError, match="decode="):
        AnomalyCLIPDataModule(decode="nonsense")
    with pytest.raises(SystemExit) as e:                         # the command line: argparse's own refusal
        X._parser().parse_args(["--arch", "ViT-B/16", "--weights", "w", "--frames-root", "f", "--out-root", "o", "--decode", "nonsense"])
    assert e.value.code == 2
    a = X._parser().parse_args(["--arch", "ViT-B/16", "--weights", "w", "--frames-root", "f", "--out-root", "o"])
    assert a.decode == "pil"                                     # the default stays Pillow
    import inspect
    for fn in (X.extract_video, X.extract_dataset, FeatureBank.from_frames, AnomalyCLIPDataModule.__init__):
        assert inspect.signature(fn).parameters["decode"].default == "pil"
