"""-m gpu: the device entropy decoder (acx_jpeg_entropy_decode_dev through ops.jpeg_entropy_decode) against the host decoder, bit
for bit and status for status; then JpegEntropyFolderReader against the Pillow reader, and `decode="gpu_entropy"` of the extractor
against `decode="pil"`.  Every damaged file here has been through the CPU build of the kernel's text under the sanitizers first
(tests/test_cpu_jpeg_entropy.py, jpeg_entropy_cases.DAMAGED)."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import jpeg_entropy_cases as EC
import jpeg_restated as JR
from anomalyclip_amd import _lib as L
from anomalyclip_amd import extract as X
from anomalyclip_amd import ops
from anomalyclip_amd.jpeg import JpegEntropyFolderReader

DEV = "cuda"
E_BADARG = -1


def _decode(files, sub_bits=0):
    """one launch over `files` (one geometry) -> (coef int16 [F, n], status int32 [F]) on the host"""
    args, geom, longest = EC.device_batch(files, DEV)
    coef, status = ops.jpeg_entropy_decode(*args, *geom, max_scan_bits=longest, sub_bits=sub_bits)
    assert coef.shape == (len(files), ops.jpeg_coef_elems(*geom)) and coef.dtype == torch.int16
    return coef.cpu(), status.cpu()


def _host(files):
    out = [JR.host_decode(d) for d in files]
    return torch.from_numpy(np.stack([o[2] for o in out])), [o[0] for o in out]


@pytest.fixture(scope="module")
def grid():
    """{mode: {(H, W): [bytes] over quality 30 / 100 x noise 0 / 120}}"""
    out = {}
    for name, data in JR.grid_cases():
        size, mode, q, noise = name.split("-")
        if q in ("q30", "q100") and noise in ("n0", "n120"):
            out.setdefault(mode, {}).setdefault(size, []).append(data)
    assert all(len(v) == 5 and all(len(f) == 4 for f in v.values()) for v in out.values())
    return out


# Each of the 80 cases has more than one subsequence at its smallest sub_bits -- 6 ... 899 of them (counted on the CPU by
# test_pack_equals_a_plain_unstuffing) -- and up to quality 30 that is 32 bits: boundaries fall inside codes, inside value bits, and
# at quality 100 with noise 120 on whole subsequences in which no symbol starts.  1024 bits: a few subsequences, or one.
@pytest.mark.parametrize("mode", ["s0", "s1", "s2", "sL"])
def test_coefficients_equal_the_host_decoder(grid, mode):
    for size, files in grid[mode].items():
        want, codes = _host(files)
        assert codes == [0] * 4
        smallest = max(32, max(ops.jpeg_min_sub_bits(len(EC.pack(d)[2])) for d in files))
        for sub in (smallest, 2 * smallest, max(1024, smallest), 0):
            coef, status = _decode(files, sub)
            assert status.tolist() == [0] * 4, (size, sub)
            assert torch.equal(coef, want), (size, sub)
        for k in (0, 3):                                                       # F = 1
            coef, status = _decode(files[k:k + 1], 0)
            assert status.tolist() == [0] and torch.equal(coef, want[k:k + 1]), (size, k)


def test_files_of_the_cpu_check():
    """the files the sanitizer program decodes: flat images (a wrong block-in-MCU phase survives on their periodic stream), noise at
    quality 100, optimised tables -- each at 32-bit subsequences where its scan allows them, and automatic"""
    for name, data in EC.check_files().items():
        want, codes = _host([data])
        assert codes == [0]
        smallest = ops.jpeg_min_sub_bits(len(EC.pack(data)[2]))
        for sub in (smallest, 0):
            coef, status = _decode([data], sub)
            assert status.tolist() == [0] and torch.equal(coef, want), (name, sub)


def _with_scan_of(data: bytes, nbytes: int) -> bytes:
    """the file with zero bytes put before its end marker until its un-stuffed scan is nbytes long: the blocks are complete before
    them, so both decoders never look at them"""
    have = len(EC.pack(data)[2])
    assert data.endswith(b"\xff\xd9") and have <= nbytes
    return data[:-2] + bytes(nbytes - have) + b"\xff\xd9"


def test_batch_with_per_frame_tables_and_the_subsequence_limit():
    """5 frames of 45 x 67 at 4:2:0 in one launch: standard and optimised tables in turn, scans from 60 bytes to 10 times that and
    more; then a scan of exactly 1024 subsequences of 32 bits, and one byte more, which sub_bits = 32 cannot cover"""
    imgs = [(EC.flat(45, 67, 200), 30, {}), (JR.make_image(45, 67, 25, seed=1), 75, dict(optimize=True)),
            (JR.make_image(45, 67, 120, seed=2), 95, {}), (JR.make_image(45, 67, 0, seed=3), 50, dict(optimize=True)),
            (JR.make_image(45, 67, 60, seed=4), 85, {})]
    files = [JR.save_jpeg(a, q, 2, **kw) for a, q, kw in imgs]
    sizes = [len(EC.pack(d)[2]) for d in files]
    assert max(sizes) > 10 * min(sizes)
    assert len({bytes(EC.pack(d)[3]) for d in files}) >= 3                     # the Huffman records differ frame by frame
    want, codes = _host(files)
    assert codes == [0] * 5
    for sub in (0, ops.jpeg_min_sub_bits(max(sizes))):
        coef, status = _decode(files, sub)
        assert status.tolist() == [0] * 5 and torch.equal(coef, want), sub

    full = _with_scan_of(files[4], 4096)                                       # 1024 * 32 bits
    over = _with_scan_of(files[4], 4097)
    assert ops.jpeg_min_sub_bits(4096) == 32 and ops.jpeg_min_sub_bits(4097) == 64
    want, codes = _host([full, over])
    assert codes == [0, 0] and torch.equal(want[0], want[1])
    for sub in (32, 0):
        coef, status = _decode([full], sub)
        assert status.tolist() == [0] and torch.equal(coef, want[:1]), sub
    args, geom, longest = EC.device_batch([full, over], DEV)
    status = torch.full((2,), 77, dtype=torch.int32, device=DEV)
    with pytest.raises(L.AcxError, match="needs 64"):                          # refused before any launch: nothing is written
        ops.jpeg_entropy_decode(*args, *geom, max_scan_bits=longest, sub_bits=32, status=status)
    assert status.tolist() == [77, 77]
    coef, status = ops.jpeg_entropy_decode(*args, *geom, max_scan_bits=longest, sub_bits=64)
    assert status.tolist() == [0, 0] and torch.equal(coef.cpu(), want)
    with pytest.raises(L.AcxError):
        ops.jpeg_entropy_decode(*args, *geom, max_scan_bits=longest, sub_bits=48)


def test_status_of_damaged_frames_in_a_batch():
    """the eight damaged files of jpeg_entropy_cases.DAMAGED between intact frames: the host decoder's code frame by frame, the
    intact frames untouched by their neighbours, the damaged files the host decoder accepts decoded as it decodes them"""
    base = EC.check_files()[EC.BASE]
    variants = EC.variants(base)
    other = JR.save_jpeg(JR.make_image(45, 67, 25, seed=77), 60, 2, optimize=True)
    files, expect = [base], [0]
    for kind, k, status in EC.DAMAGED:
        files += [variants[(kind, k)], other if len(files) % 4 == 1 else base]
        expect += [status, 0]
    want, codes = _host(files)
    assert codes == expect and sorted(set(expect)) == [E_BADARG, 0]
    for sub in (32, 0):
        coef, status = _decode(files, sub)
        assert status.tolist() == expect, sub
        for j, code in enumerate(expect):
            if code == 0:
                assert torch.equal(coef[j], want[j]), (sub, j)
    # a frame whose scan is not inside the buffer, or not on a word, is a status as well
    args, geom, longest = EC.device_batch([base, base, base], DEV)
    scans, off, bits, huff = args
    off = off.clone()
    off[1] += 8
    bits = bits.clone()
    bits[2] = scans.numel() * 8 + 32
    coef, status = ops.jpeg_entropy_decode(scans, off, bits, huff, *geom, max_scan_bits=longest, sub_bits=0)
    assert status.tolist() == [0, E_BADARG, E_BADARG] and torch.equal(coef[0].cpu(), want[0])
    assert not coef[1:].any()


# ---------------------------------------------------------------------------------------------------------------- the reader
def _folder(folder, T, hw, special=None):
    """frames at 4:2:0; special: {t: "progressive" | "restart" | "cut"}.  "cut" is a scan cut at three quarters of the file and
    closed by an end marker: Pillow fills the rest in, the host decoder refuses it.  (A file that merely stops is an OSError in
    Pillow, and so in every reader.)"""
    os.makedirs(folder, exist_ok=True)
    for t in range(T):
        kind = (special or {}).get(t)
        kw = dict(progressive=True) if kind == "progressive" else dict(restart_marker_blocks=3) if kind == "restart" else {}
        data = JR.save_jpeg(JR.make_image(hw[0], hw[1], 25, seed=500 + t), 60 + 5 * (t % 4), 2, **kw)
        if kind == "cut":
            data = data[: len(data) * 3 // 4] + b"\xff\xd9"
            assert JR.host_decode(data)[0] == E_BADARG
        with open(os.path.join(folder, f"{t:06d}.jpg"), "wb") as fh:
            fh.write(data)


@pytest.mark.parametrize("special", [{}, {1: "restart", 4: "progressive", 6: "cut"}])
def test_reader_equals_the_pillow_reader(tmp_path, special):
    """batches(3) over 8 frames: 3 + 3 + 2, both slots used; the progressive and the cut file are Pillow's (counted), the file with a
    restart interval is the host decoder's (not counted)"""
    root = str(tmp_path)
    _folder(os.path.join(root, "v"), 8, (45, 67), special)
    want = torch.cat([b.clone() for _, b in X.FrameFolderReader(root, "v", pinned=False).batches(3)])
    r = JpegEntropyFolderReader(root, "v", threads=3)
    assert len(r) == 8 and r.frame_size == (45, 67)
    got, slots = [], []
    for slot, b in r.batches(3):
        assert b.is_cuda and b.dtype == torch.uint8
        slots.append(slot)
        got.append(b)
    torch.cuda.synchronize()
    assert slots == [0, 1, 0] and [b.shape[0] for b in got] == [3, 3, 2]
    assert torch.equal(torch.cat(got).cpu(), want)
    assert r.fallbacks == sum(1 for k in special.values() if k != "restart")
    if not special:        # what crossed to the device: each file's size rounded up to 16, and per frame offset, length, tables
        sizes = sum(-(-os.path.getsize(r.path(i)) // 16) * 16 for i in range(8))
        assert r.h2d_bytes == sizes + 8 * (8 + 4 + ops.JPEG_HUFF_BYTES + 3 * 64 * 2)


def test_reader_of_a_video_the_decoder_takes_no_frame_of(tmp_path):
    """all progressive: no geometry, every frame Pillow's, no kernel launched; a missing file raises what the Pillow reader raises"""
    root = str(tmp_path)
    _folder(os.path.join(root, "v"), 4, (16, 24), {t: "progressive" for t in range(4)})
    want = torch.cat([b.clone() for _, b in X.FrameFolderReader(root, "v", pinned=False).batches(3)])
    r = JpegEntropyFolderReader(root, "v")
    got = torch.cat([b for _, b in r.batches(3)]).cpu()
    assert r.geometry is None and r.fallbacks == 4 and torch.equal(got, want)
    _folder(os.path.join(root, "w"), 4, (16, 16))
    with pytest.raises(FileNotFoundError):
        list(JpegEntropyFolderReader(root, "w", 0, 5).batches(4))


@pytest.mark.parametrize("ncrops", [1, 10])
def test_extract_video_decode_gpu_entropy_writes_the_same_file(tmp_path, ncrops):
    from test_gpu_extract import _tiny_vit
    enc, _ = _tiny_vit()
    root = str(tmp_path / "frames")
    _folder(os.path.join(root, "v"), 23, (48, 64), {7: "progressive", 12: "restart"})
    enc.chunk = 8 * ncrops                                       # three batches of 8 + 8 + 7 frames
    a = X.extract_video(enc, X.FrameFolderReader(root, "v"), str(tmp_path / "pil.npy"), ncrops, decode="pil")
    b = X.extract_video(enc, X.FrameFolderReader(root, "v"), str(tmp_path / "dev.npy"), ncrops, decode="gpu_entropy")
    assert a == b == {"written": True, "frames": 23, "rows": 23 * ncrops}
    pil, dev = np.load(tmp_path / "pil.npy"), np.load(tmp_path / "dev.npy")
    assert pil.shape == (23 * ncrops, 128) and np.array_equal(pil, dev)
    counts = X.extract_dataset(enc, None, root, str(tmp_path / "out"), ncrops, decode="gpu_entropy")
    assert counts["written"] == 1 and np.array_equal(np.load(tmp_path / "out" / "v.npy"), pil)
