"""CPU-only: the host side of `Visualizer(entropy="gpu")` -- the device Huffman coder's own text (anomalyclip_amd/csrc/
acx_jpeg_enc_dev.h) run with its lanes in a loop under AddressSanitizer and UndefinedBehaviorSanitizer (tools/
jpeg_encode_dev_check.cpp) against the host coder; acx_jpeg_encode_header against the files the host coder writes; the `entropy`
switch; and the new entry points' declarations."""
import os
import re
import subprocess

import numpy as np
import pytest

import jpeg_encode_dev_cases as EC
import viz_ref as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sanitizer_build_of_the_device_encoder(tmp_path):
    """tools/jpeg_encode_dev_check.cpp (its own main; nothing preloaded, nothing loaded into Python): count, scan, write and stuff
    over emulated lanes from exact-size heap buffers, byte for byte acx_jpeg::entropy_encode's files, `cap` exact and one byte
    short, the refusals, the scan-order map"""
    clang = next((c for c in ("/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++") if os.path.exists(c)), None)
    assert clang is not None, "the ROCm clang++ that builds the library is missing"
    exe = str(tmp_path / "jpeg_encode_dev_check")
    r = subprocess.run([clang, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        os.path.join(REPO, "tools", "jpeg_encode_dev_check.cpp"), "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "jpeg_encode_dev_check: 0 failure(s)" in r.stdout


@pytest.mark.parametrize("quality", [1, 50, 100])
def test_header_is_the_prefix_of_the_host_coders_file(quality):
    from anomalyclip_amd import _lib as L
    from anomalyclip_amd import ops
    from anomalyclip_amd import visualizer as V
    qt = V.quant_tables(quality)
    for H, W in ((16, 16), (33, 47), (800, 1200), (65535, 1)):
        head = ops.jpeg_encode_header(qt, H, W)
        assert head.dtype == np.uint8 and head.shape == (623,) == (ops.JPEG_HEADER_BYTES,)
        if H * W < 1 << 20:
            data = EC.host_file(R.entropy_cases(H, W)[-1][1], qt, H, W)
            assert data[:623] == head.tobytes() and data[623 - 14:623 - 12] == b"\xff\xda"        # the scan follows SOS
    # between guard bytes: a buffer one byte short gets ACX_E_WORKSPACE and nothing behind it
    lib = L.lib()
    buf = np.full(623 + 32, 0xA5, np.uint8)
    assert lib.acx_jpeg_encode_header(qt.ctypes.data, 16, 16, buf.ctypes.data, 622) == ops.E_WORKSPACE and (buf[622:] == 0xA5).all()
    assert lib.acx_jpeg_encode_header(qt.ctypes.data, 16, 16, buf.ctypes.data, 623) == 623 and (buf[623:] == 0xA5).all()
    assert lib.acx_jpeg_encode_header(None, 16, 16, buf.ctypes.data, 623) == ops.E_BADARG
    assert lib.acx_jpeg_encode_header(qt.ctypes.data, 16, 16, None, 623) == ops.E_BADARG
    assert lib.acx_jpeg_encode_header(qt.ctypes.data, 0, 16, buf.ctypes.data, 623) == ops.E_BADARG
    assert lib.acx_jpeg_encode_header(qt.ctypes.data, 16, 65536, buf.ctypes.data, 623) == ops.E_BADARG
    bad = qt.copy()
    bad[1, 63] = 256
    assert lib.acx_jpeg_encode_header(bad.ctypes.data, 16, 16, buf.ctypes.data, 623) == ops.E_BADARG


def test_workspace_bytes_and_their_refusals():
    from anomalyclip_amd import _lib as L
    from anomalyclip_amd import ops
    one, two = ops.jpeg_entropy_encode_dev_workspace_bytes(800, 1200, 1), ops.jpeg_entropy_encode_dev_workspace_bytes(800, 1200, 2)
    longest = 22500 * EC.MAX_BLOCK_BITS // 8                       # the string of a frame whose every block has 1,658 bits
    assert one > longest + 22500 * 4 and two - one > longest + 22500 * 4 and two < 2.2 * one
    for H, W, B in ((0, 16, 1), (16, 0, 1), (65536, 16, 1), (16, 16, 0), (16, 16, 65536), (65535, 833, 1)):
        assert L.lib().acx_jpeg_entropy_encode_dev_workspace_bytes(H, W, B) == 0
        with pytest.raises(L.AcxError):
            ops.jpeg_entropy_encode_dev_workspace_bytes(H, W, B)
    assert ops.jpeg_entropy_encode_dev_workspace_bytes(65535, 832, 1) > 0          # 1,277,952 blocks x 1,658 bits stay below 2^31


def test_entropy_switch():
    from anomalyclip_amd import visualizer as V
    assert V.ENTROPY == ("host", "gpu")
    for bad in ("x", "GPU", None, 1):
        with pytest.raises(ValueError, match="entropy=.*'host'.*'gpu'"):
            V.Visualizer(7, None, "{:06d}.jpg", "unused", "cpu", entropy=bad)
    assert V.Visualizer(7, None, "{:06d}.jpg", "unused", "cpu").entropy == "host"
    v = V.Visualizer(7, None, "{:06d}.jpg", "unused", "cpu", entropy="gpu")
    assert v.entropy == "gpu" and v._pool is None and v.cap == max(1 << 16, 1200 * 800 * 3 // 4)


def test_header_declares_the_new_entry_points():
    """(tests/test_cpu_host.py then holds the library and the ctypes table to them)"""
    from anomalyclip_amd import _lib as L
    text = open(os.path.join(REPO, "include", "acx.h")).read()
    for name, ret in (("acx_jpeg_encode_header", "int64_t"), ("acx_jpeg_entropy_encode_dev_workspace_bytes", "size_t"),
                      ("acx_jpeg_entropy_encode_dev", "int")):
        assert re.search(rf"^{ret} {name}\(", text, re.M), name
        assert name in L.declared_symbols() and hasattr(L.lib(), name)
