"""-m gpu: the device half of the JPEG decoder (acx_jpeg_reconstruct through ops.jpeg_reconstruct) against Pillow, bit for bit, on
the grid tests/test_cpu_jpeg.py pins the host half with; then JpegFolderReader against FrameFolderReader, and the `decode="gpu"`
routes of the extractor and of the resident bank against their Pillow routes."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_restated as JR
from anomalyclip_amd import extract as X
from anomalyclip_amd import ops
from anomalyclip_amd.feature_bank import FeatureBank
from anomalyclip_amd.jpeg import JpegFolderReader

DEV = "cuda"


@pytest.fixture(scope="module")
def grid():
    """{(H, W, mode): [(coef, qt, geom, Pillow's RGB)] over quality x noise}: decoded on the host once, shared, left unchanged"""
    out = {}
    for name, data in JR.grid_cases():
        rc, geom, coef, qt = JR.host_decode(data)
        assert rc == 0, name
        size, mode = name.split("-")[:2]
        out.setdefault((geom["H"], geom["W"], mode), []).append((coef, qt, geom, JR.pillow_rgb(data)))
    assert len(out) == 20 and all(len(v) == 12 for v in out.values())
    return out


def _reconstruct(cases):
    """one launch over the frames `cases` (one geometry)"""
    g = cases[0][2]
    coef = torch.from_numpy(np.stack([c[0] for c in cases])).to(DEV)
    qt = torch.from_numpy(np.stack([c[1] for c in cases]).view(np.int16)).to(DEV)
    out = ops.jpeg_reconstruct(coef, qt, g["H"], g["W"], g["ncomp"], g["hs"], g["vs"])
    assert out.shape == (len(cases), g["H"], g["W"], 3) and out.dtype == torch.uint8
    return out.cpu()


# 16 x 16: a single MCU at 4:2:0.  17 x 23 and 33 x 31: partial edge MCUs in both axes, odd chroma widths and heights.  45 x 67: more
# than the 8 blocks of a wave and more than the 32 of a workgroup, a pixel count that is no multiple of a thread's 16.  8 x 40: one
# row of blocks, a chroma plane (20 samples, 3 blocks) narrower than a wave's span of 8 blocks.
@pytest.mark.parametrize("mode", ["s0", "s1", "s2", "sL"])
@pytest.mark.parametrize("size", JR.SIZES)
def test_reconstruct_equals_pillow(grid, size, mode):
    cases = grid[(size[0], size[1], mode)]
    ref = torch.from_numpy(np.stack([c[3] for c in cases]))
    assert torch.equal(_reconstruct(cases[0:5]), ref[0:5])                     # F = 5: five qualities / noise levels in one launch
    assert torch.equal(_reconstruct(cases[5:10]), ref[5:10])
    for k in (0, 10, 11):                                                      # F = 1
        assert torch.equal(_reconstruct(cases[k:k + 1]), ref[k:k + 1]), k


def test_reconstruct_batch_with_per_frame_tables():
    """16 frames of 240 x 320 at 4:2:0, each at its own quality 30 ... 95: the quantisation tables are per frame"""
    cases = []
    for k in range(16):
        data = JR.save_jpeg(JR.make_image(240, 320, 25, seed=100 + k), 30 + (65 * k) // 15, 2)
        rc, geom, coef, qt = JR.host_decode(data)
        assert rc == 0
        cases.append((coef, qt, geom, JR.pillow_rgb(data)))
    assert len({c[1].tobytes() for c in cases}) == 16
    assert torch.equal(_reconstruct(cases), torch.from_numpy(np.stack([c[3] for c in cases])))


def test_reconstruct_refuses_what_it_has_no_kernel_for():
    from anomalyclip_amd import _lib as L
    coef = torch.zeros(1, ops.jpeg_coef_elems(16, 16, 3, 2, 2), dtype=torch.int16, device=DEV)
    qt = torch.ones(1, 3, 64, dtype=torch.int16, device=DEV)
    assert torch.equal(ops.jpeg_reconstruct(coef, qt, 16, 16, 3, 2, 2).cpu(), torch.full((1, 16, 16, 3), 128, dtype=torch.uint8))
    h = ops._h(coef)
    out = torch.empty(1, 16, 16, 3, dtype=torch.uint8, device=DEV)
    call = lambda *geom: L.lib().acx_jpeg_reconstruct(h, coef.data_ptr(), qt.data_ptr(), *geom, 1, coef.data_ptr(), out.data_ptr(), None)
    assert call(16, 16, 3, 1, 2) == -2 and call(16, 16, 4, 1, 1) == -2                                      # ACX_E_UNSUPPORTED
    assert [call(16, w, 3, 2, 2) for w in (2, 3, 4)] == [-2, -2, -2] and call(16, 4, 3, 2, 1) == -2         # (chroma rows of <= 2 samples)
    assert call(0, 16, 3, 1, 1) == -1                                                                       # ACX_E_BADARG


# ---------------------------------------------------------------------------------------------------------------- the reader
def _folder(folder, T, hw, progressive=()):
    os.makedirs(folder, exist_ok=True)
    for t in range(T):
        kw = dict(progressive=True) if t in progressive else {}
        with open(os.path.join(folder, f"{t:06d}.jpg"), "wb") as fh:
            fh.write(JR.save_jpeg(JR.make_image(hw[0], hw[1], 25, seed=500 + t), 60 + 5 * (t % 4), 2, **kw))


@pytest.mark.parametrize("progressive", [(), (4,)])
def test_reader_equals_the_pillow_reader(tmp_path, progressive):
    """batches(3) over 7 frames: 3 + 3 + 1, both slots used twice; with frame 4 progressive, Pillow decodes exactly that one"""
    root = str(tmp_path)
    _folder(os.path.join(root, "v"), 7, (45, 67), progressive)
    want = torch.cat([b.clone() for _, b in X.FrameFolderReader(root, "v", pinned=False).batches(3)])
    r = JpegFolderReader(root, "v", threads=3)
    assert len(r) == 7 and r.frame_size == (45, 67)
    got, slots = [], []
    for slot, b in r.batches(3):
        assert b.is_cuda and b.dtype == torch.uint8
        slots.append(slot)
        got.append(b)
    torch.cuda.synchronize()
    assert slots == [0, 1, 0] and [b.shape[0] for b in got] == [3, 3, 1]
    assert torch.equal(torch.cat(got).cpu(), want)
    assert r.fallbacks == len(progressive)


@pytest.mark.parametrize("sub", [1, 2])
def test_narrowest_subsampled_frames(tmp_path, sub):
    """5 pixels wide (a chroma row of three samples) is the narrowest subsampled frame the kernels take; a 4-pixel-wide video is
    Pillow's frame by frame -- no frame of it gives the reader a geometry -- and counted"""
    cases = []
    for k, h in enumerate((1, 7, 16)):
        data = JR.save_jpeg(JR.make_image(h, 5, 25, seed=70 + k), 90, sub)
        rc, geom, coef, qt = JR.host_decode(data)
        assert rc == 0
        assert torch.equal(_reconstruct([(coef, qt, geom)]), torch.from_numpy(JR.pillow_rgb(data))[None])
    root = str(tmp_path)
    os.makedirs(os.path.join(root, "v"))
    for t in range(5):
        with open(os.path.join(root, "v", f"{t:06d}.jpg"), "wb") as fh:
            fh.write(JR.save_jpeg(JR.make_image(16, 4, 25, seed=80 + t), 90, sub))
    want = torch.cat([b.clone() for _, b in X.FrameFolderReader(root, "v", pinned=False).batches(2)])
    r = JpegFolderReader(root, "v")
    got = torch.cat([b for _, b in r.batches(2)]).cpu()
    assert r.geometry is None and r.fallbacks == 5 and torch.equal(got, want)


def test_reader_raises_what_the_pillow_reader_raises(tmp_path):
    root = str(tmp_path)
    _folder(os.path.join(root, "v"), 4, (16, 16))
    with open(os.path.join(root, "v", "000002.jpg"), "wb") as fh:
        fh.write(JR.save_jpeg(JR.make_image(16, 24, 0, seed=1), 75, 2))
    with pytest.raises(ValueError, match="the video's first frame is 16 x 16"):
        list(JpegFolderReader(root, "v").batches(4))
    _folder(os.path.join(root, "w"), 4, (16, 16))
    with pytest.raises(FileNotFoundError):
        list(JpegFolderReader(root, "w", 0, 5).batches(4))


# ---------------------------------------------------------------------------------------------------------------- the routes
@pytest.mark.parametrize("ncrops", [1, 10])
def test_extract_video_decode_gpu_writes_the_same_file(tmp_path, ncrops):
    from test_gpu_extract import _tiny_vit
    enc, _ = _tiny_vit()
    root = str(tmp_path / "frames")
    _folder(os.path.join(root, "v"), 23, (48, 64), progressive=(7,))
    enc.chunk = 8 * ncrops                                       # three batches of 8 + 8 + 7 frames
    a = X.extract_video(enc, X.FrameFolderReader(root, "v"), str(tmp_path / "pil.npy"), ncrops, decode="pil")
    b = X.extract_video(enc, X.FrameFolderReader(root, "v"), str(tmp_path / "gpu.npy"), ncrops, decode="gpu")
    assert a == b == {"written": True, "frames": 23, "rows": 23 * ncrops}
    pil, gpu = np.load(tmp_path / "pil.npy"), np.load(tmp_path / "gpu.npy")
    assert pil.shape == (23 * ncrops, 128) and np.array_equal(pil, gpu)
    counts = X.extract_dataset(enc, None, root, str(tmp_path / "out"), ncrops, decode="gpu")
    assert counts["written"] == 1 and np.array_equal(np.load(tmp_path / "out" / "v.npy"), pil)


def test_bank_from_frames_decode_gpu_equals_the_pillow_bank(tmp_path):
    from test_gpu_extract import _tiny_vit
    enc, _ = _tiny_vit()
    root = str(tmp_path)
    _folder(os.path.join(root, "a"), 9, (48, 64))
    _folder(os.path.join(root, "b"), 6, (64, 48), progressive=(0,))
    recs = [SimpleNamespace(video="a", start_frame=1, end_frame=8, label=0), SimpleNamespace(video="b", start_frame=0, end_frame=5, label=3)]
    pil = FeatureBank.from_frames(enc, recs, root, ncrops=5)
    gpu = FeatureBank.from_frames(enc, recs, root, ncrops=5, decode="gpu")
    assert gpu.bank.shape == (14 * 5, 128) and torch.equal(gpu.bank, pil.bank)
    assert torch.equal(gpu.row_off, pil.row_off) and torch.equal(gpu.frames, pil.frames)
