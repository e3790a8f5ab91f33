"""CPU-only: the host side of `decode="gpu_entropy"` -- acx_jpeg_scan_pack against a plain un-stuffing, on damaged files and
between guard bytes; ops.jpeg_min_sub_bits at its boundaries; the device decoder's own text (anomalyclip_amd/csrc/acx_jpeg_sync.h)
run with its threads emulated serially under AddressSanitizer and UndefinedBehaviorSanitizer (tools/jpeg_device_check.cpp) against
the host decoder; and the third value of the `decode` switch at every entry point.  The damaged files tests/test_gpu_jpeg_entropy.py
gives to the kernel are checked here first (jpeg_entropy_cases.DAMAGED)."""
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import jpeg_entropy_cases as EC
import jpeg_restated as JR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, E_BADARG, E_UNSUPPORTED = 0, -1, -2


# ---------------------------------------------------------------------------------------------------------------- the packer
def test_pack_equals_a_plain_unstuffing():
    """the scans of the whole grid (5 sizes x 4 samplings x 4 qualities x 3 noise levels), each packed into a destination of exactly
    its padded size between guard bytes; and, for the GPU test that relies on it, the number of subsequences of the q 30 / 100 x
    noise 0 / 120 cases at their smallest sub_bits"""
    from anomalyclip_amd import ops
    stuffed, nsub = 0, {}
    for name, data in JR.grid_cases():
        rc, info, payload, huff = EC.pack(data, guard=64)
        assert rc == OK, name
        want = EC.unstuffed(data, int(info.scan_offset))
        assert payload == want, name
        stuffed += len(data) - int(info.scan_offset) - 2 - len(want)
        nc = int(info.ncomp)
        assert list(huff[-8:-4][:nc]) == [int(info.comp_td[c]) for c in range(nc)]
        assert list(huff[-4:][:nc]) == [int(info.comp_ta[c]) for c in range(nc)]
        assert bytes(huff[8:8 + 17]) == bytes(info.huff_bits[0][0]) and bytes(huff[8 + 4 * 17:8 + 5 * 17]) == bytes(info.huff_bits[1][0])
        assert bytes(huff[144:144 + 256]) == bytes(info.huff_vals[0][0])
        size, mode, q, noise = name.split("-")
        if q in ("q30", "q100") and noise in ("n0", "n120"):
            nsub.setdefault(mode, []).append(-(-len(payload) * 8 // max(32, ops.jpeg_min_sub_bits(len(payload)))))
    assert stuffed > 100, "the grid holds no stuffed bytes"
    # every one of the 20 cases of each sampling has more than one subsequence: 6 ... 899 of them
    assert {m: (len(v), min(v) > 1) for m, v in nsub.items()} == {m: (20, True) for m in ("s0", "s1", "s2", "sL")}
    assert min(min(v) for v in nsub.values()) == 6 and max(max(v) for v in nsub.values()) == 899


def test_pack_stops_at_markers_and_drops_fill_bytes():
    """hand-made scans behind a real header: FF 00 is FF, an FF before an FF is dropped, a marker or a lone FF ends the stream"""
    data = JR.save_jpeg(JR.make_image(16, 16, 0, seed=1, grey=True), 75)
    head = data[:EC.scan_offset(data)]
    for scan, want in [(b"\x12\xff\x00\x34\xff\xd9", b"\x12\xff\x34"), (b"\x12\xff\xff\x00\x34\xff\xd9", b"\x12\xff\x34"),
                       (b"\x12\x34\xff", b"\x12\x34"), (b"\x12\xff\xff", b"\x12"), (b"\xff\xd0\x55", b""), (b"", b""),
                       (b"\x01\x02\x03\x04\x05", b"\x01\x02\x03\x04\x05"), (b"\xff\x00\xff\x00", b"\xff\xff")]:
        rc, _, payload, _ = EC.pack(head + scan, guard=16)
        assert (rc, payload) == (OK, want), scan


def test_pack_of_truncated_and_corrupted_files_ends_in_a_code():
    """the file cut at every one of 40 lengths, and the tool's 40 bit-flip variants: a code, the payload never longer than what is
    left of the file, the guard bytes intact (EC.pack asserts them)"""
    for mode in (2, "L"):
        data = JR.save_jpeg(JR.make_image(45, 67, 25, seed=31, grey=(mode == "L")), 75, None if mode == "L" else mode)
        taken = 0
        for key, d in EC.variants(data).items():
            rc, info, payload, _ = EC.pack(d, guard=32)
            assert rc in (OK, E_BADARG, E_UNSUPPORTED), key
            if rc == OK and payload is not None:
                taken += 1
                assert len(payload) <= len(d) - int(info.scan_offset)
                if key[0] == "cut":                      # nothing after the cut: the payload is the rest of the file, un-stuffed
                    rest = d[int(info.scan_offset):]
                    assert payload == (rest[:-1] if rest.endswith(b"\xff") else rest).replace(b"\xff\x00", b"\xff"), key
        assert taken > 40


@pytest.mark.parametrize("mode", [0, 2, "L"])
def test_pack_leaves_restart_files_to_the_host_decoder(mode):
    a = JR.make_image(45, 67, 25, seed=11, grey=(mode == "L"))
    data = JR.save_jpeg(a, 75, None if mode == "L" else mode, restart_marker_blocks=3)
    assert JR.host_decode(data)[0] == OK
    rc, info, _, _ = EC.pack(data, guard=16)
    assert rc == E_UNSUPPORTED and int(info.restart_interval) > 0


def test_pack_refuses_what_the_parser_refuses_and_bad_arguments():
    from anomalyclip_amd import _lib as L
    from anomalyclip_amd import ops
    a = JR.make_image(45, 67, 25, seed=21)
    assert EC.pack(JR.save_jpeg(a, 75, 2, progressive=True))[0] == E_UNSUPPORTED      # (acx_jpeg_parse's answer)
    assert EC.pack(b"")[0] == E_BADARG
    data = JR.save_jpeg(a, 75, 2)
    rc, info, payload, _ = EC.pack(data)
    dst = np.zeros(len(payload) + 8, np.uint8)
    for field, value in (("scan_offset", len(data) + 1), ("scan_offset", 1), ("ncomp", 2)):
        bad = L.JpegInfo.from_buffer_copy(info)
        setattr(bad, field, value)
        assert ops.jpeg_scan_pack(data, bad, dst)[0] == E_BADARG, field
    bad = L.JpegInfo.from_buffer_copy(info)
    bad.comp_ta[1] = 3                                                                 # a table the file never defined
    assert ops.jpeg_scan_pack(data, bad, dst)[0] == E_BADARG
    assert ops.jpeg_scan_pack(data, info, dst)[0] == OK


def test_min_sub_bits_at_its_boundaries():
    from anomalyclip_amd import ops
    assert ops.JPEG_MAX_SUBSEQ == 1024
    assert ops.jpeg_min_sub_bits(0) == 32                        # an empty scan: one subsequence
    assert ops.jpeg_min_sub_bits(1) == 32
    assert ops.jpeg_min_sub_bits(1024 * 32 // 8) == 32           # 1024 * 32 bits: exactly 1024 subsequences of 32
    assert ops.jpeg_min_sub_bits(1024 * 32 // 8 + 1) == 64       # one byte more
    assert ops.jpeg_min_sub_bits(1024 * 64 // 8) == 64 and ops.jpeg_min_sub_bits(1024 * 64 // 8 + 1) == 96
    for n in (99_000, 1 << 20, (1 << 28) - 1):
        s = ops.jpeg_min_sub_bits(n)
        assert s % 32 == 0 and s * 1024 >= n * 8 > (s - 32) * 1024


# ---------------------------------------------------------------------------------------------------------------- the decoder's text
def test_sanitizer_build_of_the_device_decoder(tmp_path):
    """tools/jpeg_device_check.cpp (its own main; nothing preloaded, nothing loaded into Python) under AddressSanitizer and
    UndefinedBehaviorSanitizer: the five phases with the threads emulated serially, over whole files, their 40 truncations and 40
    seeded bit-flip variants, at sub_bits 32, 64 and automatic -- status and coefficients equal the host decoder's.  Its listing
    must hold every damaged file the GPU test uses, with the status that test expects."""
    clang = next((c for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(c)), None)
    assert clang is not None, "the ROCm clang++ that builds the library is missing"
    exe = str(tmp_path / "jpeg_device_check")
    r = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tools", "jpeg_device_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    files = []
    for name, data in EC.check_files().items():
        p = tmp_path / f"{name}.jpg"
        p.write_bytes(data)
        files.append(str(p))
    r = subprocess.run([exe, "--list", *files], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    rows = [line.split("\t") for line in r.stdout.splitlines()]
    seen = {(os.path.basename(f)[:-4], kind, int(k)): int(status) for f, kind, k, status, _, _ in rows}
    assert sum(1 for k in seen if k[1] == "whole") >= 8 and len(seen) > 400
    for kind, k, status in EC.DAMAGED:
        assert seen.get((EC.BASE, kind, k)) == status, (kind, k)
    variants = EC.variants(EC.check_files()[EC.BASE])            # ... and they are the files this module makes
    for kind, k, status in EC.DAMAGED:
        assert JR.host_decode(variants[(kind, k)])[0] == status, (kind, k)
    # the flat files take more than one round to synchronise at 32 bits, the noisy ones hundreds
    rounds = {os.path.basename(f)[:-4]: int(n) for f, kind, _, _, _, n in rows if kind == "whole"}
    assert rounds["flat_s2"] > 1 and rounds["flat_sL"] > 1 and rounds["sL_q100"] > 100


# ---------------------------------------------------------------------------------------------------------------- the switch
class _Accepted(Exception):
    pass


def test_decode_switch_takes_the_third_value_at_every_entry_point(tmp_path, monkeypatch):
    """"gpu_entropy" passes the check of every entry point the switch has ("nonsense" still does not), before a frame or the GPU
    is touched; the command line takes it; the reader it selects has no CPU fallback"""
    from anomalyclip_amd import extract as X
    from anomalyclip_amd import jpeg
    from anomalyclip_amd._lib import AcxError
    from anomalyclip_amd.datamodule import AnomalyCLIPDataModule
    from anomalyclip_amd.feature_bank import FeatureBank
    assert jpeg.DECODERS == ("pil", "gpu", "gpu_entropy") and jpeg.check_decode("gpu_entropy") == "gpu_entropy"
    with pytest.raises(ValueError, match="'pil'.*'gpu'.*'gpu_entropy'"):
        jpeg.check_decode("nonsense")
    real, taken = jpeg.check_decode, []

    def check(decode, key="decode"):
        taken.append(real(decode, key))
        raise _Accepted()

    monkeypatch.setattr(jpeg, "check_decode", check)
    enc = SimpleNamespace(output_dim=32)
    rec = [SimpleNamespace(video="v", start_frame=0, end_frame=3, label=0)]
    calls = [lambda d: X.extract_video(enc, np.zeros((1, 8, 8, 3), np.uint8), str(tmp_path / "x"), decode=d),
             lambda d: X.extract_dataset(enc, None, str(tmp_path), str(tmp_path / "out"), decode=d),
             lambda d: FeatureBank.from_frames(enc, rec, str(tmp_path), max_bytes=1 << 30, decode=d),
             lambda d: AnomalyCLIPDataModule(decode=d)]
    for call in calls:
        with pytest.raises(_Accepted):
            call("gpu_entropy")
        with pytest.raises(ValueError, match="decode="):
            call("nonsense")
    assert taken == ["gpu_entropy"] * 4
    monkeypatch.undo()
    a = X._parser().parse_args(["--arch", "ViT-B/16", "--weights", "w", "--frames-root", "f", "--out-root", "o", "--decode", "gpu_entropy"])
    assert a.decode == "gpu_entropy"
    with pytest.raises(SystemExit):
        X._parser().parse_args(["--arch", "ViT-B/16", "--weights", "w", "--frames-root", "f", "--out-root", "o", "--decode", "nonsense"])
    os.makedirs(tmp_path / "v")
    for t in range(3):
        (tmp_path / "v" / f"{t:06d}.jpg").write_bytes(JR.save_jpeg(JR.make_image(16, 16, 25, seed=t), 75, 2))
    r = jpeg.make_reader("gpu_entropy", str(tmp_path), "v")
    assert type(r) is jpeg.JpegEntropyFolderReader and isinstance(r, jpeg.JpegFolderReader) and len(r) == 3
    assert type(jpeg.make_reader("gpu", str(tmp_path), "v")) is jpeg.JpegFolderReader
    assert type(jpeg.JpegEntropyFolderReader.like(X.FrameFolderReader(str(tmp_path), "v"))) is jpeg.JpegEntropyFolderReader
    if not torch.cuda.is_available():
        with pytest.raises(AcxError, match="no CPU fallback"):
            next(iter(r.batches(2)))
