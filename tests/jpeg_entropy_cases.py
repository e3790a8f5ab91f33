"""The files and damaged variants that tests/test_cpu_jpeg_entropy.py runs through the CPU build of the device entropy decoder
(tools/jpeg_device_check.cpp, under the sanitizers) and tests/test_gpu_jpeg_entropy.py then gives to the kernel: the GPU sees no
damaged file that has not passed on the CPU first.  `variants` restates the tool's own cuts and seeded bit flips."""
import ctypes as C
import re

import numpy as np

import jpeg_restated as JR

BASE = "s2_q30"                        # the file whose damaged variants go to the GPU: 45 x 67 at 4:2:0, quality 30
# (kind, index, the host decoder's status): three truncations, three flipped-bit files it rejects and two it accepts
DAMAGED = [("cut", 24, -1), ("cut", 30, -1), ("cut", 39, -1), ("flip", 4, -1), ("flip", 11, -1), ("flip", 13, -1),
           ("flip", 5, 0), ("flip", 25, 0)]


def flat(h, w, value, grey=False):
    return np.full((h, w) if grey else (h, w, 3), value, dtype=np.uint8)


def check_files():
    """{name: bytes}: what the sanitizer program is run on"""
    out = {f"s{m}_q{q}": JR.save_jpeg(JR.make_image(45, 67, 25, seed=41, grey=(m == "L")), q, None if m == "L" else m)
           for m in (0, 1, 2, "L") for q in (30, 100)}
    # a flat image: every block is the same few bits, so the stream has a short period on which a decoder that is in step with the
    # symbols but one block off in the MCU stays so: only the comparison of the FULL state tells it from a synchronised one.  (At
    # value 128 an MCU is exactly 32 bits and every subsequence starts on one; 200 shifts the stream by the first DC symbols.)
    out["flat_s2"] = JR.save_jpeg(flat(45, 67, 200), 75, 2)
    out["flat_sL"] = JR.save_jpeg(flat(45, 67, 200, grey=True), 75)
    out["flat128_s2"] = JR.save_jpeg(flat(45, 67, 128), 75, 2)
    # quality 100 with heavy noise: symbols of more than 16 bits, so that whole 32-bit subsequences hold no symbol start
    out["noisy_s0_q100"] = JR.save_jpeg(JR.make_image(45, 67, 120, seed=43), 100, 0)
    out["optimized_s2"] = JR.save_jpeg(JR.make_image(45, 67, 25, seed=44), 75, 2, optimize=True)
    return out


def scan_offset(data: bytes) -> int:
    from anomalyclip_amd import _lib as L
    info = L.JpegInfo()
    assert L.lib().acx_jpeg_parse(data, len(data), C.byref(info)) == 0
    return int(info.scan_offset)


def variants(data: bytes):
    """{("cut", k) / ("flip", k): bytes} as tools/jpeg_device_check.cpp makes them: the file cut at 40 evenly spaced lengths, and 40
    copies with 1 ... 4 bit flips inside the scan from its linear congruential generator, seeded by the file's length"""
    out = {("cut", k): data[: len(data) * k // 40] for k in range(40)}
    off = scan_offset(data)
    span = len(data) - off
    seed = (12345 + len(data)) & 0xFFFFFFFF
    for k in range(40):
        b = bytearray(data)
        for _ in range(1 + k % 4):
            seed = (seed * 1664525 + 1013904223) & 0xFFFFFFFF
            at = off + (seed >> 8) % span
            seed = (seed * 1664525 + 1013904223) & 0xFFFFFFFF
            b[at] ^= 1 << ((seed >> 16) & 7)
        out[("flip", k)] = bytes(b)
    return out


def unstuffed(data: bytes, off: int) -> bytes:
    """the entropy-coded segment of a file without restart markers or fill bytes, the plain way"""
    scan = data[off:]
    m = re.search(rb"\xff[^\x00]", scan)
    return scan[: m.start() if m else len(scan)].replace(b"\xff\x00", b"\xff")


def pack(data: bytes, guard: int = 0):
    """acx_jpeg_parse + acx_jpeg_scan_pack -> (rc, info, payload bytes, huff uint8 [HUFF]); with `guard` > 0 the destination is
    exactly the padded payload between two runs of guard bytes, whose survival is asserted"""
    from anomalyclip_amd import _lib as L
    from anomalyclip_amd import ops
    info = L.JpegInfo()
    rc = L.lib().acx_jpeg_parse(data, len(data), C.byref(info))
    if rc != 0:
        return rc, None, None, None
    huff = np.zeros(ops.JPEG_HUFF_BYTES, np.uint8)
    room = -(-max(0, len(data) - int(info.scan_offset)) // 4) * 4
    buf = np.full(room + 2 * guard, 0xA5, np.uint8)
    rc, n = ops.jpeg_scan_pack(data, info, buf[guard:guard + room], huff)
    if rc != 0:
        assert (buf == 0xA5).all(), "a refused scan was written"
        return rc, info, None, None
    pad = -(-n // 4) * 4
    assert not buf[guard + n:guard + pad].any(), "the padding is not zero"
    if guard:
        exact = np.full(pad + 2 * guard, 0xA5, np.uint8)
        rc2, n2 = ops.jpeg_scan_pack(data, info, exact[guard:guard + pad], None)
        assert (rc2, n2) == (0, n) and (exact[:guard] == 0xA5).all() and (exact[guard + pad:] == 0xA5).all(), "guard bytes overwritten"
        assert np.array_equal(exact[guard:guard + pad], buf[guard:guard + pad])
        if pad:
            assert ops.jpeg_scan_pack(data, info, exact[guard:guard + pad - 1], None)[0] == -1
    return 0, info, bytes(buf[guard:guard + n]), huff


def device_batch(files, dev="cuda"):
    """[bytes] of one geometry, all packable -> the arguments of ops.jpeg_entropy_decode up to the geometry, as device tensors, and
    the longest scan in bits"""
    import torch
    from anomalyclip_amd import ops
    from anomalyclip_amd.jpeg import geometry_of
    scans, offs, bits, huffs, geom = [], [], [], [], None
    at = 0
    for data in files:
        rc, info, payload, huff = pack(data)
        assert rc == 0
        geom = geom or geometry_of(info)
        assert geometry_of(info) == geom
        padded = payload + bytes(-len(payload) % 16)
        scans.append(padded)
        offs.append(at * 8)
        bits.append(len(payload) * 8)
        huffs.append(huff)
        at += len(padded)
    blob = np.frombuffer(b"".join(scans) + bytes(16), np.uint8).copy()
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(dev)
    return (t(blob, np.uint8), t(offs, np.int64), t(bits, np.int32), t(np.stack(huffs), np.uint8)), geom, max(bits)
